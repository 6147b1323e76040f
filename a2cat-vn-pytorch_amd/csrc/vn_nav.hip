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
//
// Fixed-episode evaluation (DESIGN.md "Fixed-episode evaluation"): nav_step_log_kernel is the
// step form that also writes the per-episode log (vn_nav_set_episode_log); nav_count_kernel,
// nav_scan_kernel and nav_draw_kernel draw (start, goal) pairs by geodesic distance from a
// scene's table (vn_nav_sample_episodes), off the step path.
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
//
// LOG: the per-episode log (vn_nav_set_episode_log). A compile-time parameter with launch
// arguments of its own, so the log-off kernel is the code it was before the log existed.
struct NavLog {
  vn_episode_log b;
  const float* ep_ret;  // this step's ep_return output
};
struct NoLog {};

template <bool LOG, typename LG>
__device__ __forceinline__ void nav_step_body(const NavArgs& a, const LG& lg) {
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
      if constexpr (LOG) {
        const int k = lg.b.count[e];
        if (k < min(lg.b.want[e], lg.b.capacity)) {
          const int64_t i = (int64_t)k * E + e;
          lg.b.success[i] = success ? 1 : 0;
          lg.b.length[i] = ep_len - off;
          lg.b.start_dist[i] = l;
          lg.b.spl[i] = spl;
          lg.b.ep_return[i] = lg.ep_ret[e];
        }
        lg.b.count[e] = k + 1;
      }
    }
  }
  if (a.form == NAV_FORM_ENABLE || elapsed == 0) {
    a.rec[e] = d;
    a.rec[E + e] = elapsed;
  }
}

__global__ __launch_bounds__(kNavThreads) void nav_step_kernel(NavArgs a) { nav_step_body<false>(a, NoLog{}); }

// NAV_FORM_STEP only.
__global__ __launch_bounds__(kNavThreads) void nav_step_log_kernel(NavArgs a, NavLog lg) {
  nav_step_body<true>(a, lg);
}

// ---- vn_nav_sample_episodes -----------------------------------------------------------------
// Q = {(g, s) : lo <= geo[g][s] <= hi}, ordered by g then s. Goal rows are only 2-byte aligned
// (odd n), so every table read here is a 2-byte load; none of this is on the step path.

// One workgroup per goal row: cnt[g] = the row's qualifying states. Integer sums: any order
// gives the same bits, and this one is fixed.
__global__ __launch_bounds__(kNavThreads) void nav_count_kernel(const int16_t* __restrict__ tab, int n, int lo, int hi,
                                                                int32_t* __restrict__ cnt) {
  const int g = blockIdx.x;
  const int16_t* row = tab + (int64_t)g * n;
  int c = 0;
  for (int s = threadIdx.x; s < n; s += kNavThreads) {
    const int d = row[s];
    c += (d >= lo && d <= hi) ? 1 : 0;
  }
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
  __shared__ int red[kNavThreads / 64];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int i = 0; i < kNavThreads / 64; ++i) t += red[i];
    cnt[g] = t;
  }
}

// One workgroup: off[g] = sum of cnt[0..g-1] for g = 0..n (off[n] = |Q|), 64-bit. Thread t owns
// the goals [t * per, (t + 1) * per), per <= 64 for n <= kNavMaxStates.
__global__ __launch_bounds__(kNavThreads) void nav_scan_kernel(const int32_t* __restrict__ cnt, int n,
                                                               int64_t* __restrict__ off) {
  __shared__ int64_t part[kNavThreads];
  const int per = (n + kNavThreads - 1) / kNavThreads;
  const int g0 = min(threadIdx.x * per, n), g1 = min(g0 + per, n);
  int64_t t = 0;
  for (int g = g0; g < g1; ++g) t += cnt[g];
  part[threadIdx.x] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t run = 0;
    for (int i = 0; i < kNavThreads; ++i) {
      const int64_t v = part[i];
      part[i] = run;
      run += v;
    }
    off[n] = run;
  }
  __syncthreads();
  int64_t run = part[threadIdx.x];
  for (int g = g0; g < g1; ++g) {
    off[g] = run;
    run += cnt[g];
  }
}

// One wave per draw. The goal by a wave-uniform binary search of the scanned offsets, the state
// by a rank-select inside the goal's row, 64 states per __ballot (64 bits wide on gfx950).
__global__ __launch_bounds__(kNavThreads) void nav_draw_kernel(const int16_t* __restrict__ tab, int n, int lo, int hi,
                                                               const int64_t* __restrict__ off, int count, uint32_t k0,
                                                               uint32_t k1, uint32_t salt,
                                                               int32_t* __restrict__ start_goal,
                                                               int32_t* __restrict__ dist) {
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * (kNavThreads / 64) + (threadIdx.x >> 6);
  if (j >= count) return;  // wave-uniform
  const uint64_t total = (uint64_t)off[n];
  if (total == 0) return;
  const u32x4 r = philox4x32_10(u32x4{(uint32_t)j, 0u, salt, STREAM_EPISODES}, k0, k1);
  const uint64_t u = ((uint64_t)r.x << 32) | r.y;
  const int64_t idx = (int64_t)__umul64hi(u, total);  // < total
  // the first goal whose end offset lies beyond idx: goals without a pair are passed over
  int a = 0, b = n - 1;
  while (a < b) {
    const int mid = (a + b) >> 1;
    if (off[mid + 1] <= idx) a = mid + 1;
    else b = mid;
  }
  const int g = a;
  int k = (int)(idx - off[g]);  // rank of the state among the row's qualifying ones
  const int16_t* row = tab + (int64_t)g * n;
  for (int base = 0; base < n; base += 64) {
    const int s = base + lane;
    const int d = s < n ? (int)row[s] : -1;
    const bool q = d >= lo && d <= hi;  // lo >= 1: the padding lanes never qualify
    const unsigned long long m = __ballot(q);
    const int c = __popcll(m);
    if (k < c) {
      if (q && __popcll(m & ((1ull << lane) - 1ull)) == k) {
        start_goal[2 * (int64_t)j] = s;
        start_goal[2 * (int64_t)j + 1] = g;
        if (dist) dist[j] = d;
      }
      return;
    }
    k -= c;
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
  void* ptrs[] = {s->scenes, s->geo, s->rec, s->acc, s->s_done, s->s_trunc, s->s_len,
                  s->s_ret,  s->ep_cnt, s->ep_off};
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
                  alloc((void**)&s->s_len, E * 4) && alloc((void**)&s->s_ret, E * 4) &&
                  alloc((void**)&s->ep_cnt, (size_t)max_n * 4) && alloc((void**)&s->ep_off, ((size_t)max_n + 1) * 8);
  s->max_n = max_n;
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
  if (e == hipSuccess) e = hipMemset(s->s_ret, 0, E * 4);
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
               const int32_t* ep_len, const float* ep_ret, hipStream_t stream) {
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
  const dim3 grid((s->n_envs + kNavThreads - 1) / kNavThreads);
  if (form == NAV_FORM_STEP && s->log.capacity > 0) {
    const NavLog lg{s->log, ep_ret};
    hipLaunchKernelGGL(nav_step_log_kernel, grid, dim3(kNavThreads), 0, stream, a, lg);
  } else {
    hipLaunchKernelGGL(nav_step_kernel, grid, dim3(kNavThreads), 0, stream, a);
  }
  VN_HIP(hipGetLastError());
  return VN_OK;
}

int nav_set_episode_log(NavState* s, const vn_episode_log* log) {
  if (log && (log->capacity <= 0 || !log->want || !log->count || !log->success || !log->length ||
              !log->start_dist || !log->spl || !log->ep_return))
    return fail(VN_EINVAL, "vn_nav_set_episode_log: capacity <= 0 or a NULL buffer");
  VN_HIP(hipDeviceSynchronize());
  if (!log) {
    s->log = vn_episode_log{};
    return VN_OK;
  }
  VN_HIP(hipMemset(log->count, 0, (size_t)s->n_envs * 4));
  VN_HIP(hipDeviceSynchronize());
  s->log = *log;
  return VN_OK;
}

int nav_sample_episodes(NavState* s, int scene, int dist_lo, int dist_hi, int count, uint64_t seed, uint32_t salt,
                        int32_t* start_goal, int32_t* dist, int64_t* total_host, hipStream_t stream) {
  if (scene < 0 || scene >= s->n_scenes || dist_lo < 1 || dist_hi < dist_lo || count <= 0 || !start_goal ||
      !total_host)
    return fail(VN_EINVAL, "vn_nav_sample_episodes: bad arguments");
  const NavScene& S = s->scenes_host[scene];
  const int n = S.n, hi = std::min(dist_hi, 32767);
  const int16_t* tab = s->geo + S.geo_off;
  int64_t total = 0;
  if (n > 0) {
    hipLaunchKernelGGL(nav_count_kernel, dim3(n), dim3(kNavThreads), 0, stream, tab, n, dist_lo, hi, s->ep_cnt);
    hipLaunchKernelGGL(nav_scan_kernel, dim3(1), dim3(kNavThreads), 0, stream, s->ep_cnt, n, s->ep_off);
    VN_HIP(hipGetLastError());
    VN_HIP(hipMemcpyAsync(&total, s->ep_off + n, 8, hipMemcpyDeviceToHost, stream));
    VN_HIP(hipStreamSynchronize(stream));
  }
  if (total > 0) {
    const int waves = kNavThreads / 64;
    hipLaunchKernelGGL(nav_draw_kernel, dim3((count + waves - 1) / waves), dim3(kNavThreads), 0, stream, tab, n,
                       dist_lo, hi, s->ep_off, count, (uint32_t)seed, (uint32_t)(seed >> 32), salt, start_goal, dist);
    VN_HIP(hipGetLastError());
    VN_HIP(hipStreamSynchronize(stream));  // the scratch is free for the next call
  }
  *total_host = total;
  return VN_OK;
}

int nav_episode_stats(NavState* s, float* stats4, hipStream_t stream) {
  hipLaunchKernelGGL(nav_stats_kernel, dim3(1), dim3(kNavThreads), 0, stream, s->acc, s->n_envs, stats4);
  VN_HIP(hipGetLastError());
  return VN_OK;
}

}  // namespace vn
