// vn_ppo_kl.hip — the target-KL early stop of a PPO update for gfx950 (DESIGN.md "PPO target KL"):
// the gate that forms the k3 estimate of KL(old || new) in a fixed order and sets a sticky stop
// flag on the device, and the Adam and RMSprop steps that read that flag and leave every buffer
// untouched once it is set. No host value enters, so a stopped update is still the one captured
// hipGraph, bit-identical to eager.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "vn_common.h"

namespace vn {

constexpr int OUT_LD_KL = 8;
constexpr int kGateThreads = 1024;

// log pi(a) of one row of logits: ppo_softmax_stats of vn_ppo.hip restated for the one entry the
// gate needs (that file's kernels stay as they are). The same sums in the same order, log1pf of
// the other actions' mass once it is below 2^-6; the action's entry is selected, not indexed, so
// the logits stay in registers (an action outside [0, A) selects entry 0, as the loss kernel does).
__device__ __forceinline__ float kl_logp_of(const float* row, int A, int a) {
  float lg[7];
  for (int j = 0; j < 7; ++j) lg[j] = j < A ? row[j] : 0.0f;
  float mx = lg[0];
  for (int j = 1; j < 7; ++j)
    if (j < A) mx = fmaxf(mx, lg[j]);
  int jm = 0;
  for (int j = 6; j >= 0; --j)
    if (j < A && lg[j] == mx) jm = j;
  float s = 0.0f, so = 0.0f;
  for (int j = 0; j < 7; ++j)
    if (j < A) {
      const float e = expf(lg[j] - mx);
      s += e;
      if (j != jm) so += e;
    }
  const float ls = so < 0.015625f ? log1pf(so) : logf(s);
  float lpa = lg[0] - mx - ls;
  for (int j = 1; j < 7; ++j)
    if (j < A) lpa = (j == a) ? lg[j] - mx - ls : lpa;
  return lpa;
}

// gate = [stopped, steps_allowed], kl2 = [the KL of this check, the KL that stopped the update].
// One workgroup, adv_stats_kernel's sum: thread k takes samples k, k + 1024, ... in fp64, a wave
// shuffle, then the 16 waves' sums in wave order; the mean is rounded once to fp32. No atomics:
// the same input gives the same bits, in a captured graph as in eager. A set flag is sticky: the
// launch then writes nothing. Every thread reads the flag before the first barrier and thread 0
// writes it after the last, so no read sees this launch's own write.
__global__ __launch_bounds__(kGateThreads) void kl_gate_kernel(const float* __restrict__ out,
                                                              const float* __restrict__ out_old,
                                                              const int32_t* __restrict__ actions, int n, int A,
                                                              float kl_limit, int32_t* gate, float* kl2) {
  __shared__ double red[kGateThreads / 64];
  if (gate[0] != 0) return;  // workgroup-uniform
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += kGateThreads) {
    const int64_t row = (int64_t)i * OUT_LD_KL;
    const int a = actions[i];
    const float d = kl_logp_of(out + row, A, a) - kl_logp_of(out_old + row, A, a);
    s += (double)(expm1f(d) - d);
  }
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < kGateThreads / 64; ++w) t += red[w];
    const float kl = (float)(t / (double)n);
    kl2[0] = kl;
    if (kl > kl_limit) {
      gate[0] = 1;
      kl2[1] = kl;
    } else {
      gate[1] += 1;
    }
  }
}

// adam_kernel of vn_ppo.hip behind the flag: the same expressions in the same order, so with
// *skip_dev == 0 the same bits. Every wave reads the flag (one uniform load) before its loop.
__global__ __launch_bounds__(256) void adam_gated_kernel(float* __restrict__ params, const float* __restrict__ grads,
                                                         float* __restrict__ m1, float* __restrict__ m2, int64_t n,
                                                         float scale, const float* __restrict__ scalars,
                                                         const float* __restrict__ lr_dev,
                                                         const int64_t* __restrict__ step_dev, float beta1, float beta2,
                                                         float eps, const int32_t* __restrict__ skip_dev) {
  if (*skip_dev != 0) return;
  const float coef = scalars[1] * scale;
  const double t = (double)(*step_dev + 1);
  const double bc1 = 1.0 - pow((double)beta1, t), bc2 = 1.0 - pow((double)beta2, t);
  const float step_size = (float)((double)*lr_dev / bc1);
  const float sqrt_bc2 = (float)sqrt(bc2);
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float g = grads[i] * coef;
    const float m = m1[i] * beta1 + (1.0f - beta1) * g;
    const float v = m2[i] * beta2 + (1.0f - beta2) * g * g;
    m1[i] = m;
    m2[i] = v;
    params[i] += -step_size * (m / (sqrtf(v) / sqrt_bc2 + eps));
  }
}

// Behind adam_gated_kernel on the stream; a skipped step leaves the count where it was.
__global__ void adam_advance_gated_kernel(int64_t* step_dev, const int32_t* __restrict__ skip_dev) {
  if (*skip_dev == 0) *step_dev += 1;
}

// rmsprop_kernel of vn_a2c.hip (its lr_dev form) behind the flag, as above.
__global__ __launch_bounds__(256) void rmsprop_gated_kernel(float* __restrict__ params,
                                                            const float* __restrict__ grads, float* __restrict__ sq,
                                                            int64_t n, float scale, const float* __restrict__ scalars,
                                                            const float* __restrict__ lr_dev, float alpha, float eps,
                                                            const int32_t* __restrict__ skip_dev) {
  if (*skip_dev != 0) return;
  const float coef = scalars[1] * scale;
  const float lr = *lr_dev;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float g = grads[i] * coef;
    const float s = sq[i] * alpha + (1.0f - alpha) * g * g;
    sq[i] = s;
    params[i] += -lr * (g / (sqrtf(s) + eps));
  }
}

}  // namespace vn

using namespace vn;

extern "C" {

int vn_ppo_kl_gate(const float* out, const float* out_old, const int32_t* actions, int n, int num_actions,
                   float kl_limit, int32_t* gate_dev, float* kl_dev, vn_stream_t stream) {
  if (!out || !out_old || !actions || !gate_dev || !kl_dev || n <= 0 || num_actions < 1 || num_actions > 7 ||
      !(kl_limit >= 0.0f))
    return fail(VN_EINVAL, "vn_ppo_kl_gate: bad args");
  hipLaunchKernelGGL(kl_gate_kernel, dim3(1), dim3(kGateThreads), 0, (hipStream_t)stream, out, out_old, actions, n,
                     num_actions, kl_limit, gate_dev, kl_dev);
  VN_HIP(hipGetLastError());
  return VN_OK;
}

int vn_adam_step_gated(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float scale,
                       const float* scalars2, const float* lr_dev, int64_t* step_dev, float beta1, float beta2,
                       float eps, const int32_t* skip_dev, vn_stream_t stream) {
  if (!params || !grads || !exp_avg || !exp_avg_sq || !scalars2 || !lr_dev || !step_dev || !skip_dev || n <= 0)
    return fail(VN_EINVAL, "vn_adam_step_gated: bad args");
  hipStream_t st = (hipStream_t)stream;
  const int blocks = (int)std::min<int64_t>((n + 255) / 256, 2048);
  hipLaunchKernelGGL(adam_gated_kernel, dim3(blocks), dim3(256), 0, st, params, grads, exp_avg, exp_avg_sq, n, scale,
                     scalars2, lr_dev, step_dev, beta1, beta2, eps, skip_dev);
  hipLaunchKernelGGL(adam_advance_gated_kernel, dim3(1), dim3(1), 0, st, step_dev, skip_dev);
  VN_HIP(hipGetLastError());
  return VN_OK;
}

int vn_rmsprop_step_gated(float* params, const float* grads, float* square_avg, int64_t n, float scale,
                          const float* scalars2, const float* lr_dev, float alpha, float eps, const int32_t* skip_dev,
                          vn_stream_t stream) {
  if (!params || !grads || !square_avg || !scalars2 || !lr_dev || !skip_dev || n <= 0)
    return fail(VN_EINVAL, "vn_rmsprop_step_gated: bad args");
  const int blocks = (int)std::min<int64_t>((n + 255) / 256, 2048);
  hipLaunchKernelGGL(rmsprop_gated_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, params, grads, square_avg,
                     n, scale, scalars2, lr_dev, alpha, eps, skip_dev);
  VN_HIP(hipGetLastError());
  return VN_OK;
}

}  // extern "C"
