// vn_visit.hip — state-visit counts and the novelty bonus for gfx950 (DESIGN.md "Visit counts and
// novelty bonus"): the per-env kernel behind vn_visit_enable, which counts every (scene, state)
// an env arrives in and keeps the running episode's seen-set as a bitmap, the table's integer
// statistics, and vn_a2c_novelty_rewards, which adds w_count / sqrt(N(s)) and a first-visit bonus
// to a rollout's rewards.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <new>

#include "vn_common.h"
#include "vn_visit.h"

namespace vn {

constexpr int kVisitThreads = 256;
constexpr int kNoveltyThreads = 1024;
constexpr int kVisitLanes = 8;  // lanes per env unless VN_VISIT_LANES says otherwise (the A/B)

struct VisitArgs {
  const int32_t* recs;      // EnvRec words, NAV_REC_WORDS per env
  const int64_t* cell_off;  // [n_scenes + 1]
  uint32_t* count;          // [C]
  int32_t* rec;             // [2][E]: ep_scene, ep_distinct
  uint32_t* seen;           // [E][W]
  const int32_t* mask;      // refresh form: NULL or [E]
  const uint8_t* done;      // step form
  const int32_t* term;
  int32_t* cell_out;        // step form, each may be NULL
  uint8_t* first_out;
  int32_t* ep_distinct_out;
  int n_envs, n_scenes, W, form, autoreset, add;
};

// LANES lanes per env (8 by default; 64, one wave, and 1, one thread, are the A/B forms). Lane 0
// does the O(1) work; all LANES lanes clear the bitmap of an env whose episode starts, each word
// written once, by one lane, with its final value (the start state's bit or 0).
//
// Step form. The arrival state is (ep_scene, terminal_state) where done (after an auto-reset the
// EnvRec already holds the next episode), else the EnvRec's (scene, state); both clamped into
// the tables as shape_lookup clamps. count[cell] += 1 (the old value is unused: the table after
// the launch is exact in any order); first = the state's bit was clear in seen[e]; the bit is
// set and ep_distinct += first. Where done and auto-reset is on, the next episode starts as in
// the refresh form with add = 1. With auto-reset off a done env's episode simply goes on: its
// seen-set and ep_distinct stay, every later step (the env keeps moving from where it stopped)
// is counted into the same episode and reports ep_distinct again while it is done, and only
// vn_reset's refresh form starts an episode.
//
// Refresh form, for the envs the mask names: seen[e] = {start state}, ep_scene = the EnvRec's
// scene, ep_distinct = 1, and count[start cell] += 1 where `add`.
template <int LANES>
__global__ __launch_bounds__(kVisitThreads) void visit_kernel(VisitArgs a) {
  const int gid = blockIdx.x * kVisitThreads + threadIdx.x;
  const int e = gid / LANES, lane = gid % LANES;
  if (e >= a.n_envs) return;
  const int E = a.n_envs, W = a.W;
  // scene and state are words 0..1 of the record: one 16-byte load
  const int4 w0 = *reinterpret_cast<const int4*>(a.recs + (int64_t)e * NAV_REC_WORDS);
  static_assert(NAV_RW_SCENE == 0 && NAV_RW_STATE == 1, "the record's first words");
  const int sc = min(max(w0.x, 0), a.n_scenes - 1);
  const int64_t off = a.cell_off[sc];
  const int st = min(max(w0.y, 0), (int)(a.cell_off[sc + 1] - off) - 1);
  uint32_t* seen = a.seen + (int64_t)e * W;
  bool start;
  if (a.form == VISIT_FORM_STEP) {
    const bool done = a.done[e] != 0;
    int64_t cell = off + st;
    int local = st;
    if (done) {
      const int psc = min(max(a.rec[e], 0), a.n_scenes - 1);
      const int64_t poff = a.cell_off[psc];
      local = min(max(a.term[e], 0), (int)(a.cell_off[psc + 1] - poff) - 1);
      cell = poff + local;
    }
    const uint32_t bit = 1u << (local & 31);
    const uint32_t word = seen[local >> 5];
    const bool first = (word & bit) == 0;
    start = done && a.autoreset != 0;
    if (lane == 0) {
      atomicAdd(&a.count[cell], 1u);
      const int distinct = a.rec[E + e] + (first ? 1 : 0);
      if (a.cell_out) a.cell_out[e] = (int32_t)cell;
      if (a.first_out) a.first_out[e] = first ? 1 : 0;
      if (a.ep_distinct_out) a.ep_distinct_out[e] = done ? distinct : 0;
      if (!start) {
        if (first) seen[local >> 5] = word | bit;
        a.rec[E + e] = distinct;
      }
    }
  } else {
    start = a.mask == nullptr || a.mask[e] != 0;
  }
  if (!start) return;
  const int sw = st >> 5;
  const uint32_t sbit = 1u << (st & 31);
  for (int w = lane; w < W; w += LANES) seen[w] = w == sw ? sbit : 0u;
  if (lane == 0) {
    a.rec[e] = sc;
    a.rec[E + e] = 1;
    if (a.add) atomicAdd(&a.count[off + st], 1u);
  }
}

// stats[0] += cells of [lo, hi) with count > 0, stats[1] += their sum: wave sums, then one
// integer atomic per wave and counter (exact in any order).
__global__ __launch_bounds__(kVisitThreads) void visit_stats_kernel(const uint32_t* __restrict__ count, int64_t lo,
                                                                    int64_t hi, unsigned long long* __restrict__ stats) {
  unsigned long long nz = 0, sum = 0;
  for (int64_t i = lo + blockIdx.x * (int64_t)kVisitThreads + threadIdx.x; i < hi;
       i += (int64_t)gridDim.x * kVisitThreads) {
    const uint32_t c = count[i];
    nz += c != 0 ? 1 : 0;
    sum += c;
  }
  for (int o = 32; o > 0; o >>= 1) {
    nz += __shfl_xor(nz, o);
    sum += __shfl_xor(sum, o);
  }
  if ((threadIdx.x & 63) == 0 && (nz | sum) != 0) {
    atomicAdd(&stats[0], nz);
    atomicAdd(&stats[1], sum);
  }
}

// vn_a2c_novelty_rewards: one workgroup; thread k takes the elements k, k + 1024, ... in order.
// wc = wc0, wf = wf0, or each times max(0, 1 - *steps_dev / anneal_steps) in fp64 rounded once
// (returns_ex_kernel's anneal; read on the device, so a captured update anneals). Per element,
// every operation one correctly rounded fp32 operation:
//   N = count[cell];  b = wc / sqrt((float)N)   (0 where cell is outside [0, C) or N == 0)
//   f = first ? wf : 0;  out = r + (b + f)
// stats4 = [sum of (b + f), first visits, sum of 1 / sqrt((float)N) over the counted cells, wc]:
// fp64 partial sums per thread in element order, a 64-lane xor tree per wave, the 16 waves'
// sums added in wave order by thread 0, rounded to fp32 once: the same bits from the same input.
__global__ __launch_bounds__(kNoveltyThreads) void novelty_rewards_kernel(
    const float* __restrict__ rewards, const int32_t* __restrict__ cell, const uint8_t* __restrict__ first,
    const uint32_t* __restrict__ count, int64_t C, int64_t n, float wc0, float wf0,
    const int64_t* __restrict__ steps_dev, int64_t anneal_steps, float* __restrict__ out, float* __restrict__ stats) {
  float wc = wc0, wf = wf0;
  if (anneal_steps > 0) {
    const double left = fmax(0.0, 1.0 - (double)*steps_dev / (double)anneal_steps);
    wc = (float)((double)wc0 * left);
    wf = (float)((double)wf0 * left);
  }
  double s_add = 0.0, s_first = 0.0, s_inv = 0.0;
#pragma unroll 4
  for (int64_t i = threadIdx.x; i < n; i += kNoveltyThreads) {
    const int32_t c = cell[i];
    const bool in = c >= 0 && (int64_t)c < C;
    const uint32_t N = in ? count[c] : 0u;
    float b = 0.0f, inv = 0.0f;
    if (N != 0u) {
      // sqrtf and `/` are the correctly rounded root and quotient (hipcc's default
      // -fhip-fp32-correctly-rounded-divide-sqrt); HIP's __fsqrt_rn is the native, ~1 ulp root
      const float q = sqrtf((float)N);
      b = wc / q;
      inv = 1.0f / q;
    }
    const bool fv = first[i] != 0;
    const float add = __fadd_rn(b, fv ? wf : 0.0f);
    out[i] = __fadd_rn(rewards[i], add);
    s_add += (double)add;
    s_first += fv ? 1.0 : 0.0;
    s_inv += (double)inv;
  }
  for (int o = 32; o > 0; o >>= 1) {
    s_add += __shfl_xor(s_add, o);
    s_first += __shfl_xor(s_first, o);
    s_inv += __shfl_xor(s_inv, o);
  }
  __shared__ double part[3][kNoveltyThreads / 64];
  if ((threadIdx.x & 63) == 0) {
    part[0][threadIdx.x >> 6] = s_add;
    part[1][threadIdx.x >> 6] = s_first;
    part[2][threadIdx.x >> 6] = s_inv;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t0 = 0.0, t1 = 0.0, t2 = 0.0;
    for (int k = 0; k < kNoveltyThreads / 64; ++k) {
      t0 += part[0][k];
      t1 += part[1][k];
      t2 += part[2][k];
    }
    stats[0] = (float)t0;
    stats[1] = (float)t1;
    stats[2] = (float)t2;
    stats[3] = wc;
  }
}

void visit_destroy(VisitState* s) {
  if (!s) return;
  void* ptrs[] = {s->cell_off, s->count, s->s_done, s->s_term};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  delete s;
}

int visit_create(VisitState** out, int n_envs, const std::vector<int32_t>& scene_n) {
  *out = nullptr;
  std::vector<int64_t> off(scene_n.size() + 1, 0);
  int max_n = 1;
  for (size_t k = 0; k < scene_n.size(); ++k) {
    off[k + 1] = off[k] + scene_n[k];
    max_n = std::max(max_n, (int)scene_n[k]);
  }
  if (off.back() >= (1ll << 31)) return fail(VN_EINVAL, "vn_visit_enable: 2^31 cells or more");
  VisitState* s = new (std::nothrow) VisitState();
  if (!s) return fail(VN_ENOMEM, "vn_visit_enable: host allocation failed");
  s->n_envs = n_envs;
  s->n_scenes = (int)scene_n.size();
  s->W = (max_n + 31) / 32;
  s->C = off.back();
  s->cell_off_host = off;
  const char* lanes = std::getenv("VN_VISIT_LANES");  // the A/B forms (tools/visit_bench.py): 1, 8 or 64
  const int want = lanes ? std::atoi(lanes) : 0;
  s->lanes = (want == 1 || want == 8 || want == 64) ? want : kVisitLanes;
  const size_t E = (size_t)n_envs, words = (size_t)s->state_words();
  if (hipMalloc((void**)&s->cell_off, off.size() * 8) != hipSuccess ||
      hipMalloc((void**)&s->count, std::max<size_t>(words * 4, 16)) != hipSuccess ||
      hipMalloc((void**)&s->s_done, std::max<size_t>(E, 16)) != hipSuccess ||
      hipMalloc((void**)&s->s_term, std::max<size_t>(E * 4, 16)) != hipSuccess) {
    (void)hipGetLastError();
    visit_destroy(s);
    return fail(VN_ENOMEM, "vn_visit_enable: device allocation failed");
  }
  s->rec = reinterpret_cast<int32_t*>(s->count + s->C);
  s->seen = s->count + s->C + 2 * E;
  hipError_t e = hipMemcpy(s->cell_off, off.data(), off.size() * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(s->count, 0, words * 4);
  if (e == hipSuccess) e = hipMemset(s->s_done, 0, E);
  if (e == hipSuccess) e = hipMemset(s->s_term, 0, E * 4);
  if (e != hipSuccess) {
    visit_destroy(s);
    return hip_fail(e, "vn_visit_enable: build");
  }
  *out = s;
  return VN_OK;
}

int visit_launch(VisitState* s, int form, const void* recs, const int32_t* mask, const uint8_t* done,
                 const int32_t* term, int autoreset, int add, hipStream_t stream) {
  VisitArgs a;
  a.recs = static_cast<const int32_t*>(recs);
  a.cell_off = s->cell_off;
  a.count = s->count;
  a.rec = s->rec;
  a.seen = s->seen;
  a.mask = mask;
  a.done = done;
  a.term = term;
  a.cell_out = s->cell_out;
  a.first_out = s->first_out;
  a.ep_distinct_out = s->ep_distinct_out;
  a.n_envs = s->n_envs;
  a.n_scenes = s->n_scenes;
  a.W = s->W;
  a.form = form;
  a.autoreset = autoreset;
  a.add = add;
  const int64_t threads = (int64_t)s->n_envs * s->lanes;
  const dim3 grid((unsigned)((threads + kVisitThreads - 1) / kVisitThreads)), block(kVisitThreads);
  if (s->lanes == 64)
    hipLaunchKernelGGL(visit_kernel<64>, grid, block, 0, stream, a);
  else if (s->lanes == 8)
    hipLaunchKernelGGL(visit_kernel<8>, grid, block, 0, stream, a);
  else
    hipLaunchKernelGGL(visit_kernel<1>, grid, block, 0, stream, a);
  VN_HIP(hipGetLastError());
  return VN_OK;
}

int visit_clear(VisitState* s, const void* recs, hipStream_t stream) {
  VN_HIP(hipMemsetAsync(s->count, 0, (size_t)s->C * 4, stream));
  return visit_launch(s, VISIT_FORM_REFRESH, recs, nullptr, nullptr, nullptr, 0, 1, stream);
}

int visit_stats(VisitState* s, int scene, int64_t* stats2_dev, hipStream_t stream) {
  const int64_t lo = scene < 0 ? 0 : s->cell_off_host[scene];
  const int64_t hi = scene < 0 ? s->C : s->cell_off_host[scene + 1];
  VN_HIP(hipMemsetAsync(stats2_dev, 0, 2 * sizeof(int64_t), stream));
  const int64_t blocks = std::min<int64_t>(std::max<int64_t>((hi - lo + kVisitThreads - 1) / kVisitThreads, 1), 1024);
  hipLaunchKernelGGL(visit_stats_kernel, dim3((unsigned)blocks), dim3(kVisitThreads), 0, stream, s->count, lo, hi,
                     reinterpret_cast<unsigned long long*>(stats2_dev));
  VN_HIP(hipGetLastError());
  return VN_OK;
}

}  // namespace vn

using namespace vn;

extern "C" {

int vn_a2c_novelty_rewards(const float* rewards, const int32_t* cell, const uint8_t* first, const uint32_t* count,
                           int64_t C, int T, int E, float w_count, float w_first, const int64_t* steps_dev,
                           int64_t anneal_steps, float* rewards_out, float* stats4, vn_stream_t stream) {
  if (!rewards || !cell || !first || !count || !rewards_out || !stats4 || C < 0 || T <= 0 || E <= 0 ||
      (anneal_steps > 0 && !steps_dev))
    return fail(VN_EINVAL, "vn_a2c_novelty_rewards: bad args");
  hipLaunchKernelGGL(novelty_rewards_kernel, dim3(1), dim3(kNoveltyThreads), 0, (hipStream_t)stream, rewards, cell,
                     first, count, C, (int64_t)T * E, w_count, w_first, steps_dev, anneal_steps, rewards_out, stats4);
  VN_HIP(hipGetLastError());
  return VN_OK;
}

}  // extern "C"
