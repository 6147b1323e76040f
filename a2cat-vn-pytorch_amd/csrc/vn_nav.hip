// vn_nav.hip — navigation info of vn_step for gfx950: the action-graph geodesic tables and the
// per-env distance / optimal action / success / SPL outputs (DESIGN.md "vn_step: navigation
// info").
//
// geo[g][s] is the least number of actions from state s to goal g along graph[.][0..3]
// (-1 = no edge): 0 on the goal, -1 where the goal cannot be reached. It is not the scenes'
// spd table, which is the reference sampler's cell distance plus a rotation term. int16,
// goal-major: the five lookups of a step (the state and its four neighbours) share one goal row.
//
// nav_geodesic_kernel builds one goal row per 256-thread workgroup, in LDS, by pulling: at
// level d every unreached state with a neighbour at d - 1 takes d. It runs once per
// vn_nav_enable. nav_step_kernel, one thread per env, follows every env_kernel launch while
// nav is enabled: it reads the env's record as the step left it and this step's done /
// truncated / ep_length, and keeps a two-word record per env (start distance, length offset).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>

#include "vn_common.h"
#include "vn_nav.h"

namespace vn {

typedef int32_t nav_i32x4 __attribute__((ext_vector_type(4), may_alias, aligned(16)));

constexpr int kNavThreads = 256;

// One workgroup per (scene, goal): blockIdx.y = scene, blockIdx.x = goal (< the largest n).
__global__ __launch_bounds__(kNavThreads) void nav_geodesic_kernel(const NavScene* __restrict__ scenes,
                                                                   const int32_t* __restrict__ graph,
                                                                   int16_t* __restrict__ geo) {
  __shared__ int16_t dist[kNavMaxStates];
  const NavScene S = scenes[blockIdx.y];
  const int n = S.n, g = blockIdx.x;
  if (g >= n) return;  // block-uniform
  for (int s = threadIdx.x; s < n; s += kNavThreads) dist[s] = s == g ? 0 : -1;
  __syncthreads();
  const nav_i32x4* rows = reinterpret_cast<const nav_i32x4*>(graph) + S.graph_off;
  // Pull form: no reversed graph. A value written at level d is d or was -1, never d - 1, so
  // readers of this level cannot mistake it and one buffer is enough. At most n - 1 levels
  // exist, which bounds the loop whatever the graph holds.
  for (int d = 1; d < n; ++d) {
    int changed = 0;
    for (int s = threadIdx.x; s < n; s += kNavThreads) {
      if (dist[s] >= 0) continue;
      const nav_i32x4 nb = rows[s];
      bool hit = false;
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const int v = nb[a];
        if ((unsigned)v < (unsigned)n && dist[v] == d - 1) hit = true;
      }
      if (hit) {
        dist[s] = (int16_t)d;
        changed = 1;
      }
    }
    if (!__syncthreads_or(changed)) break;
  }
  int16_t* out = geo + S.geo_off + (int64_t)g * n;
  for (int s = threadIdx.x; s < n; s += kNavThreads) out[s] = dist[s];
}

struct NavArgs {
  const int32_t* recs;  // EnvRec words, NAV_REC_WORDS per env
  const NavScene* scenes;
  const int16_t* geo;
  int32_t* rec;  // [2][E]
  float* acc;    // [4][E]
  const uint8_t* done;
  const uint8_t* trunc;
  const int32_t* ep_len;
  int32_t* geo_dist;
  int32_t* opt_action;
  uint8_t* opt_mask;
  uint8_t* ep_success;
  float* ep_spl;
  int32_t* ep_start;
  int n_envs, n_scenes, form;
};

// form NAV_FORM_STEP: the six outputs, the accumulators where done, and the next episode's
// record when the env was just reset. NAV_FORM_RESET (after vn_reset): distance, mask, action
// and the record of envs at elapsed == 0; counts nothing. NAV_FORM_ENABLE: the same for every
// env, a running episode measured from here (offset = elapsed). NAV_FORM_OUTPUTS: distance,
// mask and action only.
__global__ __launch_bounds__(kNavThreads) void nav_step_kernel(NavArgs a) {
  const int e = blockIdx.x * kNavThreads + threadIdx.x;
  if (e >= a.n_envs) return;
  const int E = a.n_envs;
  const nav_i32x4* R = reinterpret_cast<const nav_i32x4*>(a.recs + (int64_t)e * NAV_REC_WORDS);
  const nav_i32x4 w0 = R[0], w1 = R[1], nb = R[2];
  // this step's values and the nav record, issued with the record's loads: behind the output
  // stores below they would wait for one more round trip (the stores may alias them)
  const bool step = a.form == NAV_FORM_STEP;
  int l = 0, off = 0, ep_len = 0;
  bool done = false, trunc = false;
  if (step) {
    l = a.rec[e];
    off = a.rec[E + e];
    done = a.done[e] != 0;
    trunc = a.trunc[e] != 0;
    ep_len = a.ep_len[e];
  }
  // a scene or state outside the tables (a bad vn_set_state table) is looked up clamped
  const NavScene S = a.scenes[min(max(w0[NAV_RW_SCENE], 0), a.n_scenes - 1)];
  const int n = S.n;
  const int s = min(max(w0[NAV_RW_STATE], 0), n - 1), g = min(max(w0[NAV_RW_GOAL], 0), n - 1);
  const int elapsed = w1[NAV_RW_ELAPSED - 4];
  const int16_t* row = a.geo + S.geo_off + (int64_t)g * n;
  // the five lookups, all in the goal's row, issued together (-2: no edge)
  int dn[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int v = nb[k];
    dn[k] = (unsigned)v < (unsigned)n ? (int)row[v] : -2;
  }
  const int d = row[s];
  int mask = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (d > 0 && dn[k] == d - 1) mask |= 1 << k;
  if (a.geo_dist) a.geo_dist[e] = d;
  if (a.opt_mask) a.opt_mask[e] = (uint8_t)mask;
  if (a.opt_action) a.opt_action[e] = mask ? __builtin_ctz(mask) : -1;
  if (a.form == NAV_FORM_OUTPUTS) return;
  if (step) {
    const bool success = done && !trunc;
    float spl = 0.0f;
    if (success && l >= 0) {
      const int p = ep_len - off;
      spl = l == 0 ? 1.0f : (float)l / (float)max(p, l);
    }
    if (a.ep_start) a.ep_start[e] = l;
    if (a.ep_success) a.ep_success[e] = success ? 1 : 0;
    if (a.ep_spl) a.ep_spl[e] = spl;
    if (done) {
      a.acc[e] += 1.0f;
      a.acc[E + e] += success ? 1.0f : 0.0f;
      a.acc[2 * (int64_t)E + e] += spl;
      a.acc[3 * (int64_t)E + e] += (float)l;
    }
  }
  if (a.form == NAV_FORM_ENABLE || elapsed == 0) {
    a.rec[e] = d;
    a.rec[E + e] = elapsed;
  }
}

// Fixed-order sums of the four per-env accumulators, then zeroed (as vn_a2c_episode_stats).
__global__ __launch_bounds__(kNavThreads) void nav_stats_kernel(float* __restrict__ acc, int E,
                                                                float* __restrict__ stats4) {
  float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int e = threadIdx.x; e < E; e += kNavThreads)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      s[k] += acc[(int64_t)k * E + e];
      acc[(int64_t)k * E + e] = 0.0f;
    }
  __shared__ float red[4][kNavThreads / 64];
#pragma unroll
  for (int k = 0; k < 4; ++k)
    for (int o = 32; o > 0; o >>= 1) s[k] += __shfl_xor(s[k], o);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int k = 0; k < 4; ++k) red[k][w] = s[k];
  __syncthreads();
  if (threadIdx.x < 4) {
    float t = 0.0f;
    for (int i = 0; i < kNavThreads / 64; ++i) t += red[threadIdx.x][i];
    stats4[threadIdx.x] = t;
  }
}

void nav_destroy(NavState* s) {
  if (!s) return;
  void* ptrs[] = {s->scenes, s->geo, s->rec, s->acc, s->s_done, s->s_trunc, s->s_len};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  delete s;
}

int nav_create(NavState** out, int n_envs, const std::vector<NavScene>& scenes, const int32_t* graph_dev) {
  *out = nullptr;
  NavState* s = new (std::nothrow) NavState();
  if (!s) return fail(VN_ENOMEM, "vn_nav_enable: host allocation failed");
  s->n_envs = n_envs;
  s->n_scenes = (int)scenes.size();
  s->scenes_host = scenes;
  int64_t elems = 0;
  int max_n = 0;
  for (NavScene& S : s->scenes_host) {
    S.geo_off = elems;  // every table starts on a 16-byte boundary
    elems += ((int64_t)S.n * S.n + 7) / 8 * 8;
    max_n = std::max(max_n, S.n);
  }
  const size_t E = (size_t)n_envs;
  auto alloc = [](void** p, size_t bytes) { return hipMalloc(p, std::max<size_t>(bytes, 16)) == hipSuccess; };
  const bool ok = alloc((void**)&s->scenes, scenes.size() * sizeof(NavScene)) &&
                  alloc((void**)&s->geo, (size_t)elems * 2) && alloc((void**)&s->rec, 2 * E * 4) &&
                  alloc((void**)&s->acc, 4 * E * 4) && alloc((void**)&s->s_done, E) && alloc((void**)&s->s_trunc, E) &&
                  alloc((void**)&s->s_len, E * 4);
  if (!ok) {
    (void)hipGetLastError();
    nav_destroy(s);
    return fail(VN_ENOMEM, "vn_nav_enable: device allocation failed");
  }
  hipError_t e = hipMemcpy(s->scenes, s->scenes_host.data(), scenes.size() * sizeof(NavScene), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(s->rec, 0, 2 * E * 4);
  if (e == hipSuccess) e = hipMemset(s->acc, 0, 4 * E * 4);
  if (e == hipSuccess) e = hipMemset(s->s_done, 0, E);
  if (e == hipSuccess) e = hipMemset(s->s_trunc, 0, E);
  if (e == hipSuccess) e = hipMemset(s->s_len, 0, E * 4);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(nav_geodesic_kernel, dim3(max_n, s->n_scenes), dim3(kNavThreads), 0, 0, s->scenes, graph_dev,
                       s->geo);
    e = hipGetLastError();
  }
  if (e != hipSuccess) {
    nav_destroy(s);
    return hip_fail(e, "vn_nav_enable: build");
  }
  *out = s;
  return VN_OK;
}

int nav_launch(NavState* s, int form, const void* recs, const uint8_t* done, const uint8_t* trunc,
               const int32_t* ep_len, hipStream_t stream) {
  NavArgs a;
  a.recs = static_cast<const int32_t*>(recs);
  a.scenes = s->scenes;
  a.geo = s->geo;
  a.rec = s->rec;
  a.acc = s->acc;
  a.done = done;
  a.trunc = trunc;
  a.ep_len = ep_len;
  a.geo_dist = s->geo_dist;
  a.opt_action = s->opt_action;
  a.opt_mask = s->opt_mask_out ? s->opt_mask_out : s->opt_mask;
  a.ep_success = s->ep_success;
  a.ep_spl = s->ep_spl;
  a.ep_start = s->ep_start;
  a.n_envs = s->n_envs;
  a.n_scenes = s->n_scenes;
  a.form = form;
  hipLaunchKernelGGL(nav_step_kernel, dim3((s->n_envs + kNavThreads - 1) / kNavThreads), dim3(kNavThreads), 0, stream,
                     a);
  VN_HIP(hipGetLastError());
  return VN_OK;
}

int nav_episode_stats(NavState* s, float* stats4, hipStream_t stream) {
  hipLaunchKernelGGL(nav_stats_kernel, dim3(1), dim3(kNavThreads), 0, stream, s->acc, s->n_envs, stats4);
  VN_HIP(hipGetLastError());
  return VN_OK;
}

}  // namespace vn
