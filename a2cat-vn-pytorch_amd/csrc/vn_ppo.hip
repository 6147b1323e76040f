// vn_ppo.hip — the PPO epoch's own launches and Adam for gfx950 (DESIGN.md "PPO epochs"): the
// advantage statistics of a stored rollout, the clipped-surrogate loss gradient of one epoch
// (vn_a2c_loss_grad's launch shape, against the behaviour policy's stored head outputs), and
// torch's Adam on the flat parameter buffer with the learning rate and the step count read on
// the device, so a captured update stays valid.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "vn_common.h"

namespace vn {

constexpr int OUT_LD_PPO = 8;
constexpr int kAdvThreads = 1024;

// softmax_stats_loss of vn_a2c.hip, restated (that file's kernels stay as they are): the same
// sums in the same order, log1pf of the other actions' mass once it is below 2^-6.
__device__ __forceinline__ void ppo_softmax_stats(const float* lg, int A, float* p, float* logp, float& H) {
  float mx = lg[0];
  for (int j = 1; j < A; ++j) mx = fmaxf(mx, lg[j]);
  int jm = 0;
  for (int j = A - 1; j >= 0; --j)
    if (lg[j] == mx) jm = j;
  float s = 0.0f, so = 0.0f;
  for (int j = 0; j < A; ++j) {
    const float e = expf(lg[j] - mx);
    s += e;
    if (j != jm) so += e;
  }
  const float ls = so < 0.015625f ? log1pf(so) : logf(s);
  H = 0.0f;
  for (int j = 0; j < A; ++j) {
    logp[j] = lg[j] - mx - ls;
    p[j] = expf(logp[j]);
    H -= p[j] * logp[j];
  }
}

// The sum of one fp64 value per thread over the workgroup, in a fixed order (wave shuffle, then
// the waves' sums in wave order), returned to every thread.
__device__ __forceinline__ double adv_block_sum(double v, double* red) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
  __syncthreads();  // red may still be read from the pass before
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  for (int w = 0; w < kAdvThreads / 64; ++w) s += red[w];
  return s;
}

// stats2 = [mean, 1 / (std + eps)] of adv_i = returns[i] - out_old[i][A], population std. One
// workgroup: thread k sums elements k, k + 1024, ... in fp64, the workgroup's sum in a fixed
// order; the mean first, then the squares centred on the fp64 mean. No atomics, rounded once.
__global__ __launch_bounds__(kAdvThreads) void adv_stats_kernel(const float* __restrict__ returns,
                                                               const float* __restrict__ out_old, int n, int A,
                                                               float eps, float* __restrict__ stats2) {
  __shared__ double red[kAdvThreads / 64];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += kAdvThreads)
    s += (double)(returns[i] - out_old[(int64_t)i * OUT_LD_PPO + A]);
  const double mean = adv_block_sum(s, red) / (double)n;
  double q = 0.0;
  for (int i = threadIdx.x; i < n; i += kAdvThreads) {
    const double c = (double)(returns[i] - out_old[(int64_t)i * OUT_LD_PPO + A]) - mean;
    q += c * c;
  }
  const double var = adv_block_sum(q, red) / (double)n;
  if (threadIdx.x == 0) {
    stats2[0] = (float)mean;
    stats2[1] = (float)(1.0 / (sqrt(var) + (double)eps));
  }
}

// dL/d(head outputs) of one PPO epoch, one thread per sample (loss_grad_kernel's shape):
//   L = vc mean(lv) - mean(min(r A^, clamp(r, 1 - c, 1 + c) A^)) - ec mean(H),
// r = exp(logp_a - logp_old_a), A^ = R - V_old, normalised by norm2 = [mean, rstd] (read here,
// on the device) when given. The surrogate's gradient flows where the unclipped term is the
// minimum (a tie included); lv = (R - V)^2, or with cv > 0 the larger of that and the square
// against V_old + clamp(V - V_old, -cv, cv), whose gradient is 0. out and out_old may be one
// buffer (neither is written). stats += block sums of (lv, -min(s1, s2), H, R); pstats += block
// sums of (expm1(d) - d, [|r - 1| > c], r, [the clipped value term was the larger]).
__global__ __launch_bounds__(256) void ppo_loss_grad_kernel(const float* out, const float* out_old,
                                                            const int32_t* __restrict__ actions,
                                                            const float* __restrict__ returns,
                                                            const float* __restrict__ norm2, int n, int A, float clip,
                                                            float cv, float vc, float ec, float inv_n,
                                                            float* __restrict__ dout, float* stats, float* pstats) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (i < n) {
    float lg[7], p[7], lp[7], po[7], lpo[7], H, Ho;
    const int64_t row = (int64_t)i * OUT_LD_PPO;
    for (int j = 0; j < A; ++j) lg[j] = out_old[row + j];
    ppo_softmax_stats(lg, A, po, lpo, Ho);
    for (int j = 0; j < A; ++j) lg[j] = out[row + j];
    ppo_softmax_stats(lg, A, p, lp, H);
    const int a = actions[i];
    const float R = returns[i];
    const float V = out[row + A], Vo = out_old[row + A];
    float lpa = lp[0], lpoa = lpo[0];  // selected, not indexed: the arrays stay in registers
    for (int j = 1; j < A; ++j) {
      lpa = (j == a) ? lp[j] : lpa;
      lpoa = (j == a) ? lpo[j] : lpoa;
    }
    const float d = lpa - lpoa;
    const float r = expf(d);
    float adv = R - Vo;
    if (norm2) adv = (adv - norm2[0]) * norm2[1];
    const float rc = fminf(fmaxf(r, 1.0f - clip), 1.0f + clip);
    const float s1 = r * adv, s2 = rc * adv;
    const bool active = s1 <= s2;
    const float g = active ? -adv * r : 0.0f;
    for (int j = 0; j < A; ++j) {
      const float ind = (j == a) ? 1.0f : 0.0f;
      dout[row + j] = (g * (ind - p[j]) + ec * p[j] * (lp[j] + H)) * inv_n;
    }
    const float e1 = R - V;
    float lv = e1 * e1, vflag = 0.0f;
    bool vgrad = true;
    if (cv > 0.0f) {
      // inside the clip range Vc is V itself, not Vo + (V - Vo): the two squares then tie exactly
      const float dv = V - Vo;
      const float Vc = fabsf(dv) > cv ? Vo + copysignf(cv, dv) : V;
      const float e2 = R - Vc;
      const float q2 = e2 * e2;
      vgrad = lv >= q2;
      vflag = vgrad ? 0.0f : 1.0f;
      lv = fmaxf(lv, q2);
    }
    dout[row + A] = vgrad ? vc * (-2.0f * e1) * inv_n : 0.0f;
    for (int j = A + 1; j < OUT_LD_PPO; ++j) dout[row + j] = 0.0f;
    s[0] = lv;
    s[1] = -fminf(s1, s2);
    s[2] = H;
    s[3] = R;
    s[4] = expm1f(d) - d;
    s[5] = fabsf(r - 1.0f) > clip ? 1.0f : 0.0f;
    s[6] = r;
    s[7] = vflag;
  }
  __shared__ float red[4][8];
  for (int off = 32; off > 0; off >>= 1)
    for (int k = 0; k < 8; ++k) s[k] += __shfl_down(s[k], off);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0)
    for (int k = 0; k < 8; ++k) red[w][k] = s[k];
  __syncthreads();
  if (threadIdx.x < 8) {
    const int k = threadIdx.x;
    const float v = red[0][k] + red[1][k] + red[2][k] + red[3][k];
    atomicAdd(k < 4 ? &stats[k] : &pstats[k - 4], v);
  }
}

// torch's Adam (no weight decay, no amsgrad) on the flat buffers, rmsprop_kernel's grid-stride
// shape. t = *step_dev + 1 and lr = *lr_dev are read here; the bias corrections 1 - beta^t are
// formed in fp64 and rounded once each into the two fp32 factors the element loop uses.
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ params, const float* __restrict__ grads,
                                                   float* __restrict__ m1, float* __restrict__ m2, int64_t n,
                                                   float scale, const float* __restrict__ scalars,
                                                   const float* __restrict__ lr_dev,
                                                   const int64_t* __restrict__ step_dev, float beta1, float beta2,
                                                   float eps) {
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

// Behind adam_kernel on the stream: every read of the step count above has completed.
__global__ void adam_advance_kernel(int64_t* step_dev) { *step_dev += 1; }

}  // namespace vn

using namespace vn;

extern "C" {

int vn_ppo_adv_stats(const float* returns, const float* out_old, int n, int num_actions, float eps,
                     float* stats2_dev, vn_stream_t stream) {
  if (!returns || !out_old || !stats2_dev || n <= 0 || num_actions < 1 || num_actions > 7 || !(eps > 0.0f))
    return fail(VN_EINVAL, "vn_ppo_adv_stats: bad args");
  hipLaunchKernelGGL(adv_stats_kernel, dim3(1), dim3(kAdvThreads), 0, (hipStream_t)stream, returns, out_old, n,
                     num_actions, eps, stats2_dev);
  VN_HIP(hipGetLastError());
  return VN_OK;
}

// The loss-gradient launch behind both entries: `clear` zeroes the two sum vectors first.
static int ppo_loss_grad_launch(const char* who, bool clear, const float* out, const float* out_old,
                                const int32_t* actions, const float* returns, const float* adv_stats2_dev, int n,
                                int num_actions, float clip, float value_clip, float value_coef, float entropy_coef,
                                float* dout, float* stats4, float* ppo_stats4, vn_stream_t stream) {
  if (!out || !out_old || !actions || !returns || !dout || !stats4 || !ppo_stats4 || n <= 0 || num_actions < 1 ||
      num_actions > 7 || !(clip > 0.0f))
    return fail(VN_EINVAL, std::string(who) + ": bad args");
  hipStream_t st = (hipStream_t)stream;
  if (clear) {
    VN_HIP(hipMemsetAsync(stats4, 0, 4 * sizeof(float), st));
    VN_HIP(hipMemsetAsync(ppo_stats4, 0, 4 * sizeof(float), st));
  }
  hipLaunchKernelGGL(ppo_loss_grad_kernel, dim3((n + 255) / 256), dim3(256), 0, st, out, out_old, actions, returns,
                     adv_stats2_dev, n, num_actions, clip, value_clip, value_coef, entropy_coef, 1.0f / (float)n, dout,
                     stats4, ppo_stats4);
  VN_HIP(hipGetLastError());
  return VN_OK;
}

int vn_ppo_loss_grad(const float* out, const float* out_old, const int32_t* actions, const float* returns,
                     const float* adv_stats2_dev, int n, int num_actions, float clip, float value_clip,
                     float value_coef, float entropy_coef, float* dout, float* stats4, float* ppo_stats4,
                     vn_stream_t stream) {
  return ppo_loss_grad_launch("vn_ppo_loss_grad", true, out, out_old, actions, returns, adv_stats2_dev, n, num_actions,
                              clip, value_clip, value_coef, entropy_coef, dout, stats4, ppo_stats4, stream);
}

int vn_ppo_loss_grad_acc(const float* out, const float* out_old, const int32_t* actions, const float* returns,
                         const float* adv_stats2_dev, int n, int num_actions, float clip, float value_clip,
                         float value_coef, float entropy_coef, float* dout, float* stats4, float* ppo_stats4,
                         vn_stream_t stream) {
  return ppo_loss_grad_launch("vn_ppo_loss_grad_acc", false, out, out_old, actions, returns, adv_stats2_dev, n,
                              num_actions, clip, value_clip, value_coef, entropy_coef, dout, stats4, ppo_stats4, stream);
}

int vn_adam_step_dev(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float scale,
                     const float* scalars2, const float* lr_dev, int64_t* step_dev, float beta1, float beta2,
                     float eps, vn_stream_t stream) {
  if (!params || !grads || !exp_avg || !exp_avg_sq || !scalars2 || !lr_dev || !step_dev || n <= 0)
    return fail(VN_EINVAL, "vn_adam_step_dev: bad args");
  hipStream_t st = (hipStream_t)stream;
  const int blocks = (int)std::min<int64_t>((n + 255) / 256, 2048);
  hipLaunchKernelGGL(adam_kernel, dim3(blocks), dim3(256), 0, st, params, grads, exp_avg, exp_avg_sq, n, scale,
                     scalars2, lr_dev, step_dev, beta1, beta2, eps);
  hipLaunchKernelGGL(adam_advance_kernel, dim3(1), dim3(1), 0, st, step_dev);
  VN_HIP(hipGetLastError());
  return VN_OK;
}

}  // extern "C"
