// vn_rp_sample.hip — UNREAL's reward-skewed reward-prediction draw from the replay ring on
// gfx950 (vn_unreal_rp_sample, include/vnav.h; DESIGN.md "Reward-skewed reward prediction").
//
// UNREAL (Jaderberg et al. 2016) draws the reward-prediction sample from the replay buffer with
// P(r != 0) = 0.5. deep_rl's sampler is absent, so this is the published rule stated exactly: the
// candidates are the three-frame windows of the ring's filled slots that hold no episode end,
// split by their reward into Q0 (r == 0) and Q1, each ordered by the window index; a draw picks
// the set by a coin of the given skew and an element of it uniformly, with replacement.
//
// One launch of one workgroup. The update it rides in is latency-bound (a 4-env update is
// ~2.4 ms of small launches), so the launch count matters more than the bandwidth:
//   1. classify: wave w takes the 64-candidate chunks w, w + 16, ...; the class of candidate
//      chunk * 64 + lane by coalesced loads, the chunk's |Q0| and |Q1| by __ballot + popcount
//      into LDS (a byte each: a chunk holds 64 candidates). kRsUnroll chunks' loads are issued
//      before their ballots, so a pass over the ring costs nchunks / (16 kRsUnroll) round trips.
//   2. scan: thread t owns the chunks [t * cpt, (t + 1) * cpt); the exclusive prefix of the
//      threads' sums, per set, by a wave scan and the 16 wave totals. Integer sums: every order
//      gives the same bits.
//   3. select: one thread per draw: Philox, the set, idx = (u * |Qk|) >> 64; the owning thread by
//      a binary search of the 1024 prefixes, the chunk by a walk of at most cpt counts, the
//      candidate by re-reading the chunk 16 candidates at a time.
// The limit is the LDS count table: capacity * (T - 2) * S <= VN_RP_SAMPLE_MAX_CANDIDATES.
#include <hip/hip_runtime.h>

#include "vn_common.h"

namespace vn {

constexpr int kRsThreads = 1024;
constexpr int kRsWaves = kRsThreads / 64;
constexpr int kRsChunk = 64;       // candidates per count-table entry: one wave-wide ballot
constexpr int kRsMaxChunks = 16384;
constexpr int kRsUnroll = 4;       // chunks whose loads a wave issues together
constexpr int kRsBatch = 16;       // candidates a select thread re-reads together
static_assert(kRsMaxChunks * (int64_t)kRsChunk == VN_RP_SAMPLE_MAX_CANDIDATES, "the header states the limit");

// Candidate i = (r (T - 2) + (ts - 2)) S + e as its slot, first step tt = ts - 2 and env.
struct RsWindow {
  int r, tt, e;
};

__device__ __forceinline__ RsWindow rs_window(int i, int T, int S) {
  const int q = i / S, r = q / (T - 2);
  return RsWindow{r, q - r * (T - 2), i - q * S};
}

// -1: an episode ends inside the window; else 0 (reward == 0, -0.0 included) or 1.
__device__ __forceinline__ int rs_class(const vn_rp_ring& g, int i) {
  const RsWindow w = rs_window(i, g.T, g.S);
  const int64_t o = ((int64_t)w.r * g.T + w.tt) * g.S + w.e;
  const uint8_t d0 = g.dones[o], d1 = g.dones[o + g.S];
  const float rw = g.rewards[o + 2 * (int64_t)g.S];
  return (d0 | d1) ? -1 : (rw == 0.0f ? 0 : 1);
}

__global__ __launch_bounds__(kRsThreads) void rp_sample_kernel(vn_rp_ring g, int count, uint64_t thr, uint32_t k0,
                                                                uint32_t k1, int32_t* __restrict__ rows_img,
                                                                int32_t* __restrict__ rows_goal,
                                                                int32_t* __restrict__ label, int32_t* __restrict__ src,
                                                                int32_t* __restrict__ stats4) {
  __shared__ uint8_t cnt[2][kRsMaxChunks];
  __shared__ int32_t pre[2][kRsThreads];
  __shared__ int32_t wtot[2][kRsWaves];
  __shared__ int32_t drawn[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t filled64 = g.meta4[1];
  const int filled = (int)(filled64 < 0 ? 0 : (filled64 > g.capacity ? g.capacity : filled64));
  const uint64_t ctr = (uint64_t)g.meta4[2];
  const int ncand = filled * (g.T - 2) * g.S;  // <= kRsMaxChunks * kRsChunk (checked on the host)
  const int nchunks = (ncand + kRsChunk - 1) / kRsChunk;
  const int cpt = (nchunks + kRsThreads - 1) / kRsThreads;
  if (tid < 2) drawn[tid] = 0;

  // 1. the count table
  for (int c0 = wave; c0 < nchunks; c0 += kRsWaves * kRsUnroll) {
    int cls[kRsUnroll];
#pragma unroll
    for (int u = 0; u < kRsUnroll; ++u) {
      const int c = c0 + u * kRsWaves, i = c * kRsChunk + lane;
      cls[u] = (c < nchunks && i < ncand) ? rs_class(g, i) : -1;
    }
#pragma unroll
    for (int u = 0; u < kRsUnroll; ++u) {
      const int c = c0 + u * kRsWaves;
      if (c < nchunks) {  // wave-uniform
        const unsigned long long m0 = __ballot(cls[u] == 0), m1 = __ballot(cls[u] == 1);
        if (lane == 0) {
          cnt[0][c] = (uint8_t)__popcll(m0);
          cnt[1][c] = (uint8_t)__popcll(m1);
        }
      }
    }
  }
  __syncthreads();

  // 2. the exclusive prefix of every thread's run of chunks
  int own[2] = {0, 0};
  {
    const int ca = min(tid * cpt, nchunks), cb = min(ca + cpt, nchunks);
    for (int c = ca; c < cb; ++c) {
      own[0] += cnt[0][c];
      own[1] += cnt[1][c];
    }
  }
  int inc[2] = {own[0], own[1]};
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int a = __shfl_up(inc[0], o), b = __shfl_up(inc[1], o);
    if (lane >= o) {
      inc[0] += a;
      inc[1] += b;
    }
  }
  if (lane == 63) {
    wtot[0][wave] = inc[0];
    wtot[1][wave] = inc[1];
  }
  __syncthreads();
  int total[2] = {0, 0};
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    int before = 0;
#pragma unroll
    for (int w = 0; w < kRsWaves; ++w) {
      const int v = wtot[k][w];
      before += w < wave ? v : 0;
      total[k] += v;
    }
    pre[k][tid] = before + inc[k] - own[k];
  }
  __syncthreads();

  // 3. the draws
  int n_pos = 0, n_used = 0;
  for (int j = tid; j < count; j += kRsThreads) {
    const u32x4 R = philox4x32_10(u32x4{(uint32_t)j, (uint32_t)ctr, (uint32_t)(ctr >> 32), STREAM_RP}, k0, k1);
    int k = (uint64_t)R.x < thr ? 1 : 0;
    if (total[k] == 0) k = 1 - k;
    int lab = -1, from = -1, ri[3] = {0, 0, 0}, rg[3] = {0, 0, 0};
    if (total[k] > 0) {
      const uint64_t u = ((uint64_t)R.y << 32) | R.z;
      const int idx = (int)__umul64hi(u, (uint64_t)total[k]);  // < total[k]
      // the last thread whose prefix is <= idx owns it: the ones after it start beyond idx
      int a = 0, b = kRsThreads - 1;
      while (a < b) {
        const int mid = (a + b + 1) >> 1;
        if (pre[k][mid] <= idx) a = mid;
        else b = mid - 1;
      }
      int rem = idx - pre[k][a];
      int c = a * cpt;  // rem < the run's sum, so the walk ends inside the run
      for (; c + 1 < nchunks; ++c) {
        const int v = cnt[k][c];
        if (rem < v) break;
        rem -= v;
      }
      for (int b0 = 0; b0 < kRsChunk && from < 0; b0 += kRsBatch) {
        int cl[kRsBatch];
#pragma unroll
        for (int q = 0; q < kRsBatch; ++q) {
          const int i = c * kRsChunk + b0 + q;
          cl[q] = i < ncand ? rs_class(g, i) : -1;
        }
#pragma unroll
        for (int q = 0; q < kRsBatch; ++q) {
          if (cl[q] == k && from < 0) {
            if (rem == 0) from = c * kRsChunk + b0 + q;
            else --rem;
          }
        }
      }
    }
    if (from >= 0) {
      const RsWindow w = rs_window(from, g.T, g.S);
      const float rw = g.rewards[((int64_t)w.r * g.T + w.tt + 2) * g.S + w.e];
      lab = rw == 0.0f ? 0 : (rw > 0.0f ? 1 : 2);
      const int64_t n1 = (int64_t)(g.T + 1) * g.S;
      const int32_t* rr = g.rows + (int64_t)w.r * 2 * n1 + (int64_t)w.tt * g.S + w.e;
#pragma unroll
      for (int m = 0; m < 3; ++m) {
        ri[m] = rr[(int64_t)m * g.S];
        rg[m] = rr[n1 + (int64_t)m * g.S];
      }
      n_used += 1;
      n_pos += lab > 0 ? 1 : 0;
    }
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      rows_img[3 * (int64_t)j + m] = ri[m];
      rows_goal[3 * (int64_t)j + m] = rg[m];
    }
    label[j] = lab;
    if (src) src[j] = from;
  }
  for (int o = 32; o > 0; o >>= 1) {
    n_pos += __shfl_xor(n_pos, o);
    n_used += __shfl_xor(n_used, o);
  }
  if (lane == 0) {
    atomicAdd(&drawn[0], n_pos);
    atomicAdd(&drawn[1], n_used);
  }
  __syncthreads();
  if (tid == 0) {
    stats4[0] = total[0];
    stats4[1] = total[1];
    stats4[2] = drawn[0];
    stats4[3] = drawn[1];
  }
}

}  // namespace vn

using namespace vn;

extern "C" int vn_unreal_rp_sample(const vn_rp_ring* ring, int count, double skew, uint64_t seed, int32_t* rows_img,
                                   int32_t* rows_goal, int32_t* label, int32_t* src, int32_t* stats4,
                                   vn_stream_t stream) {
  if (!ring || !rows_img || !rows_goal || !label || !stats4)
    return fail(VN_EINVAL, "vn_unreal_rp_sample: NULL argument");
  if (!ring->rewards || !ring->dones || !ring->rows || !ring->meta4)
    return fail(VN_EINVAL, "vn_unreal_rp_sample: NULL ring buffer");
  if (count <= 0 || ring->T < 3 || ring->S < 1 || ring->capacity < 1 || !(skew >= 0.0 && skew <= 1.0))
    return fail(VN_EINVAL, "vn_unreal_rp_sample: needs count > 0, T >= 3, S >= 1, capacity >= 1, skew in [0, 1]");
  const int64_t windows = (int64_t)ring->capacity * (ring->T - 2);
  if (windows > VN_RP_SAMPLE_MAX_CANDIDATES || windows * ring->S > VN_RP_SAMPLE_MAX_CANDIDATES)
    return fail(VN_EINVAL, "vn_unreal_rp_sample: capacity * (T - 2) * S exceeds VN_RP_SAMPLE_MAX_CANDIDATES");
  const uint64_t thr = (uint64_t)(skew * 4294967296.0);
  hipLaunchKernelGGL(rp_sample_kernel, dim3(1), dim3(kRsThreads), 0, (hipStream_t)stream, *ring, count, thr,
                     (uint32_t)seed, (uint32_t)(seed >> 32), rows_img, rows_goal, label, src, stats4);
  VN_HIP(hipGetLastError());
  return VN_OK;
}
