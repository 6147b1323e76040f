// vn_curriculum.hip — the geodesic start curriculum for gfx950 (DESIGN.md "Geodesic
// curriculum"): start tables sorted by the nav tables' action distance, per-scene success
// counters, and the level controller that moves the threshold on the device.
//
// Per scene, with D the largest entry of its geo table and B = D + 2:
//   key(g, s)  = clamp(geo[g][s], -1, D) + 1        (0 = unreachable, 1 = the goal itself)
//   order[g][] = the states sorted stably by key(g, .)
//   count[g][b] = #states with key(g, s) <= b
// the layout reset_env (vn_env.hip) draws from, so the env kernels stay as they are: the near
// set of level L is order[g][count[g][1] .. count[g][L + 1]).
//
// cur_maxd_kernel and cur_sort_kernel run once per vn_nav_curriculum. cur_count_kernel follows
// the nav launch of every step while window > 0; cur_advance_kernel is vn_nav_curriculum_advance.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <string>

#include "vn_common.h"
#include "vn_curriculum.h"

namespace vn {

constexpr int kCurThreads = 256;

// One workgroup per (scene, goal): the scene's D by an integer max, exact in any order.
// Goal rows are only 2-byte aligned (odd n): 2-byte loads.
__global__ __launch_bounds__(kCurThreads) void cur_maxd_kernel(const CurScene* __restrict__ scenes,
                                                               const int16_t* __restrict__ geo,
                                                               int32_t* __restrict__ maxd) {
  const CurScene S = scenes[blockIdx.y];
  const int n = S.n, g = blockIdx.x;
  if (g >= n) return;  // block-uniform
  const int16_t* row = geo + S.geo_off + (int64_t)g * n;
  int m = 0;
  for (int s = threadIdx.x; s < n; s += kCurThreads) m = max(m, (int)row[s]);
  for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o));
  if ((threadIdx.x & 63) == 0 && m > 0) atomicMax(&maxd[blockIdx.y], m);
}

__device__ __forceinline__ int wave_inclusive_scan(int v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(v, o);
    if (lane >= o) v += t;
  }
  return v;
}

// One wave per (scene, goal): blockIdx.y = scene, blockIdx.x = goal (< the largest n). A stable
// counting sort of the goal's row, kCurWindow buckets at a time: the row's keys are staged in
// LDS once, and each pass histograms the keys of its window, scans them into bucket starts
// behind the states of all lower keys, and scatters the states in ascending order. Within a
// 64-state chunk a lane's rank among equal keys is the number of lower lanes with that key
// (__ballot), one distinct key per round, so equal keys keep ascending state order. A bucket's
// cursor ends at its inclusive count, which is count[g][b].
// Dynamic LDS: kCurWindow cursors, then the largest scene's n keys (uint16: key <= 16384).
__global__ __launch_bounds__(64) void cur_sort_kernel(const CurScene* __restrict__ scenes,
                                                      const int16_t* __restrict__ geo,
                                                      int32_t* __restrict__ order, int32_t* __restrict__ count) {
  extern __shared__ int32_t cur_lds[];
  int32_t* cursor = cur_lds;
  uint16_t* keys = reinterpret_cast<uint16_t*>(cur_lds + kCurWindow);
  const CurScene S = scenes[blockIdx.y];
  const int n = S.n, g = blockIdx.x, lane = threadIdx.x;
  if (g >= n) return;  // block-uniform
  const int D = S.D, B = D + 2;
  const int16_t* row = geo + S.geo_off + (int64_t)g * n;
  for (int s = lane; s < n; s += 64) keys[s] = (uint16_t)(min(max((int)row[s], -1), D) + 1);
  int32_t* ord = order + S.order_off + (int64_t)g * n;
  int32_t* cnt = count + S.cnt_off + (int64_t)g * B;
  int below = 0;  // states with a key under the window (wave-uniform)
  for (int b0 = 0; b0 < B; b0 += kCurWindow) {
    const int w = min(kCurWindow, B - b0);
    for (int i = lane; i < w; i += 64) cursor[i] = 0;
    __syncthreads();
    for (int s = lane; s < n; s += 64) {
      const int k = (int)keys[s] - b0;
      if ((unsigned)k < (unsigned)w) atomicAdd(&cursor[k], 1);
    }
    __syncthreads();
    for (int i0 = 0; i0 < w; i0 += 64) {
      const int i = i0 + lane;
      const int v = i < w ? cursor[i] : 0;
      const int incl = wave_inclusive_scan(v, lane);
      if (i < w) cursor[i] = below + incl - v;
      below += __shfl(incl, 63);
    }
    __syncthreads();
    for (int s0 = 0; s0 < n; s0 += 64) {
      const int s = s0 + lane;
      const int k = s < n ? (int)keys[s] - b0 : -1;
      const bool in = (unsigned)k < (unsigned)w;
      unsigned long long pending = __ballot(in);
      while (pending) {  // wave-uniform
        const int leader = __ffsll((long long)pending) - 1;
        const int kl = __shfl(k, leader);
        const bool mine = in && k == kl;
        const unsigned long long m = __ballot(mine);
        // the histogram counted these states: cursor[kl] + |m| <= n
        if (mine) ord[cursor[kl] + __popcll(m & ((1ull << lane) - 1ull))] = s;
        __syncthreads();
        if (lane == leader) cursor[kl] += __popcll(m);
        __syncthreads();
        pending &= ~m;
      }
    }
    for (int i = lane; i < w; i += 64) cnt[b0 + i] = cursor[i];
    __syncthreads();
  }
}

// One thread per env, behind the step's nav launch. count != 0: an env with done adds its
// finished episode to the counters of the scene that episode ran in (integer atomics: the same
// inputs give the same bits in any order). Always: ep_scene = the record's scene, which after
// an auto-reset is the new episode's. A scene outside the table is clamped, as the nav step does.
__global__ __launch_bounds__(kCurThreads) void cur_count_kernel(const int32_t* __restrict__ recs,
                                                                const uint8_t* __restrict__ done,
                                                                const uint8_t* __restrict__ trunc,
                                                                int32_t* __restrict__ ep_scene,
                                                                int32_t* __restrict__ state, int n_envs,
                                                                int n_scenes, int count) {
  const int e = blockIdx.x * kCurThreads + threadIdx.x;
  if (e >= n_envs) return;
  const int sc = min(max(recs[(int64_t)e * NAV_REC_WORDS + NAV_RW_SCENE], 0), n_scenes - 1);
  if (count && done[e]) {
    const int was = min(max(ep_scene[e], 0), n_scenes - 1);
    atomicAdd(&state[n_scenes + was], 1);
    if (!trunc[e]) atomicAdd(&state[2 * n_scenes + was], 1);
  }
  ep_scene[e] = sc;
}

struct CurRule {
  int32_t window, step, level_min;
  float up, down;
};

__device__ __forceinline__ int cur_clamp_level(int level, int level_min, int D) {
  return min(max(level, min(level_min, D)), D);
}

// One thread per scene: the decision of every scene whose window is full.
__global__ __launch_bounds__(kCurThreads) void cur_advance_kernel(int32_t* __restrict__ state, int n_scenes,
                                                                  CurRule r, CurSceneTable t) {
  const int k = blockIdx.x * kCurThreads + threadIdx.x;
  if (k >= n_scenes) return;
  const int d = state[n_scenes + k];
  if (d < r.window) return;
  const int D = state[3 * n_scenes + k];
  int level = state[k];
  const float rate = (float)state[2 * n_scenes + k] / (float)d;
  if (rate >= r.up) level = min(level + r.step, D);
  else if (rate <= r.down) level = max(level - r.step, min(r.level_min, D));
  state[k] = level;
  state[n_scenes + k] = 0;
  state[2 * n_scenes + k] = 0;
  t.words[(int64_t)k * t.stride_words + t.oi_word] = level;
}

// vn_nav_curriculum_set_state: rows 0..2 of src, the level held to [min(level_min, D), D] (a
// level above D would index past the scene's count rows), and the scene table's threshold.
__global__ __launch_bounds__(kCurThreads) void cur_set_state_kernel(const int32_t* __restrict__ src,
                                                                    int32_t* __restrict__ state, int n_scenes,
                                                                    int level_min, CurSceneTable t) {
  const int k = blockIdx.x * kCurThreads + threadIdx.x;
  if (k >= n_scenes) return;
  const int level = cur_clamp_level(src[k], level_min, state[3 * n_scenes + k]);
  state[k] = level;
  state[n_scenes + k] = src[n_scenes + k];
  state[2 * n_scenes + k] = src[2 * n_scenes + k];
  t.words[(int64_t)k * t.stride_words + t.oi_word] = level;
}

void cur_destroy(CurState* s) {
  if (!s) return;
  void* ptrs[] = {s->scenes, s->order, s->count, s->state, s->ep_scene};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  delete s;
}

int cur_create(CurState** out, const NavState* nav, const vn_geo_curriculum& cfg,
               const std::vector<int64_t>& order_off) {
  *out = nullptr;
  CurState* s = new (std::nothrow) CurState();
  if (!s) return fail(VN_ENOMEM, "vn_nav_curriculum: host allocation failed");
  const int S = nav->n_scenes;
  s->n_envs = nav->n_envs;
  s->n_scenes = S;
  s->cfg = cfg;
  s->scenes_host.resize(S);
  int64_t order_elems = 0;
  int max_n = 0;
  for (int k = 0; k < S; ++k) {
    const NavScene& N = nav->scenes_host[k];
    s->scenes_host[k] = CurScene{N.geo_off, order_off[k], 0, N.n, 0};
    order_elems = std::max(order_elems, order_off[k] + (int64_t)N.n * N.n);
    max_n = std::max(max_n, N.n);
  }
  auto alloc = [](void** p, size_t bytes) { return hipMalloc(p, std::max<size_t>(bytes, 16)) == hipSuccess; };
  auto oom = [&]() {
    (void)hipGetLastError();
    cur_destroy(s);
    return fail(VN_ENOMEM, "vn_nav_curriculum: device allocation failed");
  };
  auto bad = [&](hipError_t e) {
    cur_destroy(s);
    return hip_fail(e, "vn_nav_curriculum: build");
  };
  if (!(alloc((void**)&s->scenes, (size_t)S * sizeof(CurScene)) && alloc((void**)&s->state, (size_t)S * 16) &&
        alloc((void**)&s->ep_scene, (size_t)s->n_envs * 4) && alloc((void**)&s->order, (size_t)order_elems * 4)))
    return oom();
  hipError_t e = hipMemcpy(s->scenes, s->scenes_host.data(), (size_t)S * sizeof(CurScene), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(s->state, 0, (size_t)S * 16);
  if (e == hipSuccess) e = hipMemset(s->ep_scene, 0, (size_t)s->n_envs * 4);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(cur_maxd_kernel, dim3(max_n, S), dim3(kCurThreads), 0, 0, s->scenes, nav->geo,
                       s->state + 3 * (size_t)S);
    e = hipGetLastError();
  }
  std::vector<int32_t> st((size_t)S * 4, 0);
  if (e == hipSuccess) e = hipMemcpy(st.data() + 3 * (size_t)S, s->state + 3 * (size_t)S, (size_t)S * 4,
                                     hipMemcpyDeviceToHost);
  if (e != hipSuccess) return bad(e);
  int64_t cnt_elems = 0;
  for (int k = 0; k < S; ++k) {
    CurScene& C = s->scenes_host[k];
    C.D = st[3 * (size_t)S + k];
    if (C.D < 0 || C.D >= std::max(C.n, 1)) {  // a geodesic is a simple path: D <= n - 1
      cur_destroy(s);
      return fail(VN_EHIP, "vn_nav_curriculum: scene " + std::to_string(k) + " has a geodesic table entry of " +
                               std::to_string(C.D) + " with " + std::to_string(C.n) + " states");
    }
    C.cnt_off = cnt_elems;
    cnt_elems += (int64_t)C.n * (C.D + 2);
    st[k] = std::min(std::max(cfg.level, std::min(cfg.level_min, C.D)), C.D);
  }
  if (!alloc((void**)&s->count, (size_t)cnt_elems * 4)) return oom();
  e = hipMemcpy(s->scenes, s->scenes_host.data(), (size_t)S * sizeof(CurScene), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(s->state, st.data(), (size_t)S * 16, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    const size_t lds = (size_t)kCurWindow * 4 + ((size_t)max_n * 2 + 3) / 4 * 4;  // <= 33 KB
    hipLaunchKernelGGL(cur_sort_kernel, dim3(max_n, S), dim3(64), lds, 0, s->scenes, nav->geo, s->order, s->count);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) return bad(e);
  *out = s;
  return VN_OK;
}

int cur_count_launch(CurState* s, const void* recs, const uint8_t* done, const uint8_t* trunc, int count,
                     hipStream_t stream) {
  hipLaunchKernelGGL(cur_count_kernel, dim3((s->n_envs + kCurThreads - 1) / kCurThreads), dim3(kCurThreads), 0, stream,
                     static_cast<const int32_t*>(recs), done, trunc, s->ep_scene, s->state, s->n_envs, s->n_scenes,
                     count);
  VN_HIP(hipGetLastError());
  return VN_OK;
}

int cur_advance(CurState* s, hipStream_t stream) {
  if (s->cfg.window <= 0) return VN_OK;
  const CurRule r{s->cfg.window, s->cfg.step, s->cfg.level_min, s->cfg.up, s->cfg.down};
  hipLaunchKernelGGL(cur_advance_kernel, dim3((s->n_scenes + kCurThreads - 1) / kCurThreads), dim3(kCurThreads), 0,
                     stream, s->state, s->n_scenes, r, s->table);
  VN_HIP(hipGetLastError());
  return VN_OK;
}

int cur_get_state(CurState* s, int32_t* dst, hipStream_t stream) {
  VN_HIP(hipMemcpyAsync(dst, s->state, (size_t)s->n_scenes * 16, hipMemcpyDeviceToDevice, stream));
  return VN_OK;
}

int cur_set_state(CurState* s, const int32_t* src, const void* recs, hipStream_t stream) {
  hipLaunchKernelGGL(cur_set_state_kernel, dim3((s->n_scenes + kCurThreads - 1) / kCurThreads), dim3(kCurThreads), 0,
                     stream, src, s->state, s->n_scenes, s->cfg.level_min, s->table);
  VN_HIP(hipGetLastError());
  return cur_count_launch(s, recs, nullptr, nullptr, 0, stream);
}

}  // namespace vn
