// vn_shaping.hip — geodesic reward shaping and GAE(lambda) for gfx950 (DESIGN.md "Reward shaping
// and GAE"): the per-env progress kernel behind vn_nav_progress, which reports the action-graph
// distance to the goal before and after every step from the nav tables, and vn_a2c_returns_ex,
// the returns scan that adds the potential-based term w (d_before - gamma_phi d_after) to the
// reward and forms either the n-step return or the lambda-return.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>

#include "vn_common.h"
#include "vn_shaping.h"

namespace vn {

constexpr int kShapeThreads = 256;
constexpr int OUT_LD_SHAPE = 8;

struct ShapeArgs {
  const int32_t* recs;     // EnvRec words, NAV_REC_WORDS per env
  const NavScene* scenes;
  const int16_t* geo;
  int32_t* rec;            // [3][E]: scene, goal, distance
  const int32_t* mask;     // refresh form: NULL or [E]
  const uint8_t* done;     // step form
  const uint8_t* trunc;
  const int32_t* term;
  int32_t* dist_before;    // step form, each may be NULL
  int32_t* dist_after;
  int32_t* progress;
  int n_envs, n_scenes, form;
};

// geo[scene][goal][state] with scene, goal and state clamped to the tables, as nav_step_body
// looks them up: a bad vn_set_state table or progress state reads inside the allocation.
__device__ __forceinline__ int shape_lookup(const ShapeArgs& a, int scene, int goal, int state) {
  const NavScene S = a.scenes[min(max(scene, 0), a.n_scenes - 1)];
  const int n = S.n;
  const int s = min(max(state, 0), n - 1), g = min(max(goal, 0), n - 1);
  return (int)a.geo[S.geo_off + (int64_t)g * n + s];
}

// One thread per env. Step form, behind the step's nav launch: before = the record's distance;
// after = 0 on success (done, not truncated), the finished episode's distance at
// terminal_state on a truncation (scene and goal from the record: after an auto-reset the
// EnvRec already holds the next episode), else the distance of the EnvRec's state;
// progress = before - after where both are reachable (>= 0), else 0. Then, in both forms, the
// record takes the EnvRec's scene, goal and distance (refresh form: where the mask says so).
__global__ __launch_bounds__(kShapeThreads) void shape_progress_kernel(ShapeArgs a) {
  const int e = blockIdx.x * kShapeThreads + threadIdx.x;
  if (e >= a.n_envs) return;
  const int E = a.n_envs;
  // scene, state and goal are words 0..2 of the record: one 16-byte load
  const int4 w0 = *reinterpret_cast<const int4*>(a.recs + (int64_t)e * NAV_REC_WORDS);
  static_assert(NAV_RW_SCENE == 0 && NAV_RW_STATE == 1 && NAV_RW_GOAL == 2, "the record's first words");
  const int sc = w0.x, st = w0.y, gl = w0.z;
  const int d = shape_lookup(a, sc, gl, st);
  if (a.form == SHAPE_FORM_STEP) {
    const int before = a.rec[2 * (int64_t)E + e];
    const bool done = a.done[e] != 0, trunc = a.trunc[e] != 0;
    int after = d;
    if (done && !trunc) after = 0;
    else if (done) after = shape_lookup(a, a.rec[e], a.rec[E + e], a.term[e]);
    const int prog = (before >= 0 && after >= 0) ? before - after : 0;
    if (a.dist_before) a.dist_before[e] = before;
    if (a.dist_after) a.dist_after[e] = after;
    if (a.progress) a.progress[e] = prog;
  } else if (a.mask && a.mask[e] == 0) {
    return;
  }
  a.rec[e] = sc;
  a.rec[E + e] = gl;
  a.rec[2 * (int64_t)E + e] = d;
}

// vn_a2c_returns_ex: one thread per env, t = T-1 .. 0. w = w0, or w0 max(0, 1 - *steps_dev /
// anneal_steps) in fp64 rounded once (loss_grad_expert_kernel's anneal; read on the device, so a
// captured update anneals). Every operation below is one correctly rounded fp32 operation, in
// this order (nd = 1 - done is exact):
//   shaping, only where dist != NULL and w != 0:
//     F  = w * fma(-gamma_phi, after, before)   2 roundings (F = 0 where a distance is < 0)
//     r' = r + F                                1 rounding
//   otherwise r' = r, untouched: a -0.0 reward keeps its sign.
//   lambda == 1:  R = fma(gamma * R, nd, r')    2 roundings (returns_kernel's expression)
//     -> 2 roundings per step unshaped, 5 shaped.
//   lambda != 1:  y = fma(gamma * V', nd, r')   2 roundings (V' = V_{t+1}, V_T the bootstrap)
//                 delta = y - V                 1 rounding
//                 G = fma(gl * nd, G, delta)    1 rounding, gl = gamma * lambda rounded once: a
//                                               relative error of the coefficient, counted as 1
//                 returns = G + V               1 rounding
//     -> 6 roundings per step unshaped, 9 shaped.
// stats (int64, zeroed by the host call): sum of before and of after over the steps where both
// are >= 0, and the number of the other steps; integer atomics, exact in any order. Formed
// whenever dist != NULL, whatever w is.
__global__ __launch_bounds__(kShapeThreads) void returns_ex_kernel(
    const float* __restrict__ rewards, const uint8_t* __restrict__ dones, const float* __restrict__ boot_out,
    const float* __restrict__ out, const int32_t* __restrict__ dist, int T, int E, int A, float gamma, float lambda,
    float w0, float gamma_phi, const int64_t* __restrict__ steps_dev, int64_t anneal_steps, float* __restrict__ returns,
    unsigned long long* __restrict__ stats) {
  const int e = blockIdx.x * kShapeThreads + threadIdx.x;
  float w = w0;
  if (anneal_steps > 0) {
    const double left = 1.0 - (double)*steps_dev / (double)anneal_steps;
    w = (float)((double)w0 * fmax(0.0, left));
  }
  const bool shaped = dist != nullptr && w != 0.0f;
  const bool gae = lambda != 1.0f;
  const float gl = __fmul_rn(gamma, lambda);
  long long sb = 0, sa = 0, bad = 0;
  if (e < E) {
    float Vn = boot_out[(int64_t)e * OUT_LD_SHAPE + A];
    float R = Vn, G = 0.0f;
    for (int t = T - 1; t >= 0; --t) {
      const int64_t i = (int64_t)t * E + e;
      float r = rewards[i];
      if (dist) {
        const int b = dist[(2 * (int64_t)t) * E + e], af = dist[(2 * (int64_t)t + 1) * E + e];
        const bool ok = b >= 0 && af >= 0;
        sb += ok ? b : 0;
        sa += ok ? af : 0;
        bad += ok ? 0 : 1;
        if (shaped) {
          const float F = ok ? __fmul_rn(w, __fmaf_rn(-gamma_phi, (float)af, (float)b)) : 0.0f;
          r = __fadd_rn(r, F);
        }
      }
      const float nd = 1.0f - (float)dones[i];
      if (!gae) {
        R = r + gamma * R * nd;
        returns[i] = R;
      } else {
        const float V = out[i * OUT_LD_SHAPE + A];
        const float y = __fmaf_rn(__fmul_rn(gamma, Vn), nd, r);
        const float delta = __fsub_rn(y, V);
        G = __fmaf_rn(__fmul_rn(gl, nd), G, delta);
        returns[i] = __fadd_rn(G, V);
        Vn = V;
      }
    }
  }
  if (dist) {  // wave sums, then one atomic per wave and counter
    for (int o = 32; o > 0; o >>= 1) {
      sb += __shfl_xor(sb, o);
      sa += __shfl_xor(sa, o);
      bad += __shfl_xor(bad, o);
    }
    if ((threadIdx.x & 63) == 0) {
      atomicAdd(&stats[0], (unsigned long long)sb);
      atomicAdd(&stats[1], (unsigned long long)sa);
      atomicAdd(&stats[2], (unsigned long long)bad);
    }
  }
}

void shape_destroy(ShapeState* s) {
  if (!s) return;
  if (s->rec) (void)hipFree(s->rec);
  if (s->s_term) (void)hipFree(s->s_term);
  delete s;
}

int shape_create(ShapeState** out, int n_envs) {
  *out = nullptr;
  ShapeState* s = new (std::nothrow) ShapeState();
  if (!s) return fail(VN_ENOMEM, "vn_nav_progress: host allocation failed");
  s->n_envs = n_envs;
  const size_t E = (size_t)n_envs;
  if (hipMalloc((void**)&s->rec, std::max<size_t>(3 * E * 4, 16)) != hipSuccess ||
      hipMalloc((void**)&s->s_term, std::max<size_t>(E * 4, 16)) != hipSuccess) {
    (void)hipGetLastError();
    shape_destroy(s);
    return fail(VN_ENOMEM, "vn_nav_progress: device allocation failed");
  }
  hipError_t e = hipMemset(s->rec, 0, 3 * E * 4);
  if (e == hipSuccess) e = hipMemset(s->s_term, 0, E * 4);
  if (e != hipSuccess) {
    shape_destroy(s);
    return hip_fail(e, "vn_nav_progress: build");
  }
  *out = s;
  return VN_OK;
}

int shape_launch(ShapeState* s, const NavState* nav, int form, const void* recs, const int32_t* mask,
                 const uint8_t* done, const uint8_t* trunc, const int32_t* term, hipStream_t stream) {
  ShapeArgs a;
  a.recs = static_cast<const int32_t*>(recs);
  a.scenes = nav->scenes;
  a.geo = nav->geo;
  a.rec = s->rec;
  a.mask = mask;
  a.done = done;
  a.trunc = trunc;
  a.term = term;
  a.dist_before = s->dist_before;
  a.dist_after = s->dist_after;
  a.progress = s->progress;
  a.n_envs = s->n_envs;
  a.n_scenes = nav->n_scenes;
  a.form = form;
  hipLaunchKernelGGL(shape_progress_kernel, dim3((s->n_envs + kShapeThreads - 1) / kShapeThreads),
                     dim3(kShapeThreads), 0, stream, a);
  VN_HIP(hipGetLastError());
  return VN_OK;
}

}  // namespace vn

using namespace vn;

extern "C" {

int vn_a2c_returns_ex(const float* rewards, const uint8_t* dones, const float* bootstrap_out, const float* out,
                      const int32_t* dist, int T, int E, int num_actions, float gamma, float lambda, float weight,
                      float gamma_phi, const int64_t* steps_dev, int64_t anneal_steps, float* returns,
                      int64_t* stats3_dev, vn_stream_t stream) {
  if (!rewards || !dones || !bootstrap_out || !returns || !stats3_dev || T <= 0 || E <= 0 || num_actions < 1 ||
      num_actions > 7 || !(lambda >= 0.0f && lambda <= 1.0f) || (lambda != 1.0f && !out) ||
      (anneal_steps > 0 && !steps_dev))
    return fail(VN_EINVAL, "vn_a2c_returns_ex: bad args");
  hipStream_t st = (hipStream_t)stream;
  VN_HIP(hipMemsetAsync(stats3_dev, 0, 3 * sizeof(int64_t), st));
  hipLaunchKernelGGL(returns_ex_kernel, dim3((E + kShapeThreads - 1) / kShapeThreads), dim3(kShapeThreads), 0, st,
                     rewards, dones, bootstrap_out, out, dist, T, E, num_actions, gamma, lambda, weight, gamma_phi,
                     steps_dev, anneal_steps, returns, reinterpret_cast<unsigned long long*>(stats3_dev));
  VN_HIP(hipGetLastError());
  return VN_OK;
}

}  // extern "C"
