// vn_ppo_minibatch.hip — the PPO minibatch split for gfx950 (DESIGN.md "PPO minibatches"): one
// permutation of the envs per epoch, drawn on the device from the update's own counter, and the
// compaction of one minibatch's [T, Eb] sub-rollout out of the [T, E] rollout buffers. No host
// value enters either launch, so the K M steps of an update stay one captured hipGraph.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "vn_common.h"

namespace vn {

constexpr int kPermThreads = 256;
constexpr int kPermTile = VN_PPO_PERM_TILE;  // keys staged in LDS per pass
constexpr int kPermPerThread = kPermTile / kPermThreads;
static_assert(kPermTile % (4 * kPermThreads) == 0, "a thread fills whole uint4 groups of the tile");

// Key of env e in epoch k: the first word of Philox4x32-10 (k E + e, ctr_lo, ctr_hi, STREAM_PPO).
__device__ __forceinline__ uint32_t perm_key(uint32_t first, uint32_t e, uint64_t ctr, uint32_t k0, uint32_t k1,
                                             uint32_t mask) {
  return philox4x32_10(u32x4{first + e, (uint32_t)ctr, (uint32_t)(ctr >> 32), STREAM_PPO}, k0, k1).x & mask;
}

// Rank by counting: thread e counts the pairs (key_j, j) < (key_e, e) over every env j, the keys
// recomputed by each workgroup and staged through LDS a tile at a time (every lane reads the same
// uint4: a broadcast), then writes perm[rank] = e. The ranks of distinct pairs are distinct, so
// every slot of perm is written exactly once: no atomics, the stable argsort exactly.
__global__ __launch_bounds__(kPermThreads) void env_permutation_kernel(const int64_t* __restrict__ counter_dev,
                                                                      uint32_t first, int E, uint32_t mask,
                                                                      uint32_t k0, uint32_t k1,
                                                                      int32_t* __restrict__ perm) {
  __shared__ uint4 tile[kPermTile / 4];
  uint32_t* tile1 = (uint32_t*)tile;
  const uint64_t ctr = (uint64_t)*counter_dev;
  const int e = blockIdx.x * kPermThreads + threadIdx.x;
  const uint32_t mine = e < E ? perm_key(first, (uint32_t)e, ctr, k0, k1, mask) : 0u;
  int rank = 0;
  for (int base = 0; base < E; base += kPermTile) {
    __syncthreads();  // the tile of the pass before has been read
#pragma unroll
    for (int u = 0; u < kPermPerThread; ++u) {
      const int i = u * kPermThreads + threadIdx.x, j = base + i;
      tile1[i] = j < E ? perm_key(first, (uint32_t)j, ctr, k0, k1, mask) : 0xFFFFFFFFu;
    }
    __syncthreads();
    const int cnt = min(kPermTile, E - base);  // block-uniform
    if (e < E) {
      // envs below e win ties, envs at or above e do not: j < e splits the tile at one point. The
      // padding past cnt never counts (no key is above it, and below <= cnt), so the loop runs
      // over whole uint4 groups with several reads in flight.
      const int below = min(max(e - base, 0), cnt);
      const int groups = (cnt + 3) >> 2;
#pragma unroll 8
      for (int g = 0; g < groups; ++g) {
        const uint4 q = tile[g];
        const int i = g << 2;
        rank += (int)((q.x < mine) | ((q.x == mine) & (i < below))) +
                (int)((q.y < mine) | ((q.y == mine) & (i + 1 < below))) +
                (int)((q.z < mine) | ((q.z == mine) & (i + 2 < below))) +
                (int)((q.w < mine) | ((q.w == mine) & (i + 3 < below)));
      }
    }
  }
  if (e < E) perm[rank] = e;
}

// One grid-stride pass over four segments of destination elements, each written once with plain
// vector stores in destination order (coalesced); the reads of one row are consecutive too:
//   [0, nb)                   the per-sample scalars: rows, action, return, done, mask, goal delta
//   + nb * 2                  out_old rows as two float4
//   + nb * A1                 lra rows, one float each (A1 = A + 1 floats: 5 at A = 4)
//   + 2 * eb * 128            the start states h0 and c0 as float4
// Destination row i = t eb + j reads source row t E + envs[j]. An env index outside [0, E) (a
// permutation that was never drawn) writes nothing instead of reading out of bounds.
__global__ __launch_bounds__(256) void minibatch_gather_kernel(vn_ppo_rollout src, vn_ppo_rollout dst,
                                                               const int32_t* __restrict__ envs, int eb, int T, int E,
                                                               int A1) {
  const int64_t nb = (int64_t)T * eb;
  const bool lstm = dst.masks != nullptr;
  const int64_t s1 = nb, s2 = s1 + nb * 2, s3 = s2 + (lstm ? nb * A1 : 0), s4 = s3 + (lstm ? 2ll * eb * 128 : 0);
  for (int64_t w = blockIdx.x * 256ll + threadIdx.x; w < s4; w += (int64_t)gridDim.x * 256) {
    if (w < s1) {
      const int t = (int)(w / eb), j = (int)(w - (int64_t)t * eb);
      const int e = envs[j];
      if ((unsigned)e >= (unsigned)E) continue;
      const int64_t s = (int64_t)t * E + e;
      dst.rows_img[w] = src.rows_img[s];
      dst.rows_goal[w] = src.rows_goal[s];
      dst.actions[w] = src.actions[s];
      dst.returns[w] = src.returns[s];
      dst.dones[w] = src.dones[s];
      if (lstm) dst.masks[w] = src.masks[s];
      if (dst.goal_delta) dst.goal_delta[w] = src.goal_delta[s] / E * eb;  // a multiple of E: steps back
    } else if (w < s2) {
      const int64_t q = w - s1, i = q >> 1;
      const int t = (int)(i / eb), j = (int)(i - (int64_t)t * eb);
      const int e = envs[j];
      if ((unsigned)e >= (unsigned)E) continue;
      const float4* from = (const float4*)(src.out_old + ((int64_t)t * E + e) * 8);
      ((float4*)dst.out_old)[q] = from[q & 1];
    } else if (w < s3) {
      const int64_t q = w - s2, i = q / A1;
      const int c = (int)(q - i * A1);
      const int t = (int)(i / eb), j = (int)(i - (int64_t)t * eb);
      const int e = envs[j];
      if ((unsigned)e >= (unsigned)E) continue;
      dst.lra[q] = src.lra[((int64_t)t * E + e) * A1 + c];
    } else {
      const int64_t q = w - s3, half = (int64_t)eb * 128;
      const bool second = q >= half;
      const int64_t r = second ? q - half : q;
      const int j = (int)(r >> 7);
      const int e = envs[j];
      if ((unsigned)e >= (unsigned)E) continue;
      const float4* from = (const float4*)(second ? src.c0 : src.h0) + (int64_t)e * 128 + (r & 127);
      ((float4*)(second ? dst.c0 : dst.h0))[r] = *from;
    }
  }
}

}  // namespace vn

using namespace vn;

extern "C" {

int vn_ppo_env_permutation(uint64_t seed, const int64_t* counter_dev, int epoch, int num_envs, int key_bits,
                           int32_t* perm, vn_stream_t stream) {
  if (!counter_dev || !perm || epoch < 0 || num_envs < 1 || key_bits < 1 || key_bits > 32 ||
      ((int64_t)epoch + 1) * num_envs > (int64_t)UINT32_MAX)
    return fail(VN_EINVAL, "vn_ppo_env_permutation: bad args (key_bits 1..32, (epoch + 1) * num_envs < 2^32)");
  const uint32_t mask = key_bits == 32 ? 0xFFFFFFFFu : ((1u << key_bits) - 1u);
  const int blocks = (num_envs + kPermThreads - 1) / kPermThreads;
  hipLaunchKernelGGL(env_permutation_kernel, dim3(blocks), dim3(kPermThreads), 0, (hipStream_t)stream, counter_dev,
                     (uint32_t)((int64_t)epoch * num_envs), num_envs, mask, (uint32_t)seed, (uint32_t)(seed >> 32), perm);
  VN_HIP(hipGetLastError());
  return VN_OK;
}

int vn_ppo_minibatch_gather(const vn_ppo_rollout* src, const vn_ppo_rollout* dst, const int32_t* envs, int count,
                            int T, int num_envs, int num_actions, vn_stream_t stream) {
  if (!src || !dst || !envs || count < 1 || T < 1 || num_envs < 1 || count > num_envs || num_actions < 1 ||
      num_actions > 7 || (int64_t)T * num_envs > INT32_MAX)
    return fail(VN_EINVAL, "vn_ppo_minibatch_gather: bad args");
  for (const vn_ppo_rollout* r : {src, dst})
    if (!r->rows_img || !r->rows_goal || !r->actions || !r->returns || !r->out_old || !r->dones)
      return fail(VN_EINVAL, "vn_ppo_minibatch_gather: NULL rollout buffer");
  const int n_lstm = (dst->masks != nullptr) + (dst->lra != nullptr) + (dst->h0 != nullptr) + (dst->c0 != nullptr);
  if (n_lstm != 0 && n_lstm != 4)
    return fail(VN_EINVAL, "vn_ppo_minibatch_gather: masks, lra, h0 and c0 go together");
  if (n_lstm && (!src->masks || !src->lra || !src->h0 || !src->c0))
    return fail(VN_EINVAL, "vn_ppo_minibatch_gather: the source has no LSTM buffers");
  if (dst->goal_delta && !src->goal_delta)
    return fail(VN_EINVAL, "vn_ppo_minibatch_gather: the source has no goal_delta");
  for (const void* p : {(const void*)src->out_old, (const void*)dst->out_old, (const void*)src->h0,
                        (const void*)dst->h0, (const void*)src->c0, (const void*)dst->c0})
    if (((uintptr_t)p & 15) != 0)
      return fail(VN_EINVAL, "vn_ppo_minibatch_gather: out_old, h0 and c0 must be 16-byte aligned");
  const int A1 = num_actions + 1;
  const int64_t nb = (int64_t)T * count;
  const int64_t work = nb * 3 + (n_lstm ? nb * A1 + 2ll * count * 128 : 0);
  const int blocks = (int)std::min<int64_t>((work + 255) / 256, 2048);
  hipLaunchKernelGGL(minibatch_gather_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, *src, *dst, envs, count,
                     T, num_envs, A1);
  VN_HIP(hipGetLastError());
  return VN_OK;
}

}  // extern "C"
