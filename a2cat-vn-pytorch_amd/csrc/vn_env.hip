// vn_env.hip — batched cached-scene env.step for gfx950 (CDNA4).
//
// Semantics restate THORDiscreteCachedEnv (environments/gym_ai2thor/envs/cached.py):
//   transition  nxt = graph[s][a]; -1 = blocked                     (cached.py:74-79)
//   terminal    goal == state                                        (cached.py:83)
//   reward      -reward_configuration[1], goal -> [0], blocked -> [2] (cached.py:84-88)
//   obs         (frame[s], frame[g]), or the previous obs on terminal (cached.py:90-98)
//   reset       goal ~ U[0,N), start ~ U[0,N) until spd[start][goal] > 0 (cached.py:38-45)
// batched the way deep_rl's SubprocVecEnv drives it (auto-reset on done, the reset
// observation replaces the terminal one) under gym's TimeLimit(900).
//
// Design (DESIGN.md "vn_step"): one wave64 per env, 4 envs per 256-thread workgroup.
// Everything an env carries from launch to launch is one 128-B record (EnvRec): the seven
// state words, the running return, the four graph neighbours of the current state, the
// scene fields a step needs (row bases, graph offset, terminal_obs, the three rewards) and
// the output-reuse record. A wave reads it with two wide scalar loads issued together with
// actions[e]; one round trip later it knows the next state and the arena rows to emit, and
// the frame loads issue at once. Lane 0 writes the record back (wide vector stores) and the
// scalar outputs after the first frame loads are in flight. Only a reset (rare) reads the
// scene table again and refreshes the cached fields. A reset runs 64 Philox start candidates
// in parallel, one per lane, and a wave ballot picks the first valid one - the same result
// as the sequential rejection loop over the same counter stream.
// The frames are streamed with 16-B lanes, 8 loads in flight per lane; with output reuse on
// (vn_set_output_reuse) a frame whose output row already holds it is not copied.
// vn_step_aux / vn_observe_aux (AuxiliaryGraph's five-tuple observation) are the same kernel
// with a five-frame tail: depth, segmentation and goal segmentation rows leave the caller's
// aux arenas in the same launch, under the same reuse rule, with records of their own (AuxRec).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "vn_common.h"
#include "vn_curriculum.h"
#include "vn_nav.h"
#include "vn_shaping.h"
#include "vn_unit_float.h"
#include "vn_visit.h"

namespace vn {

static thread_local std::string g_last_error;
void set_error(const std::string& msg) { g_last_error = msg; }
int fail(int code, const std::string& msg) {
  set_error(msg);
  return code;
}
int hip_fail(hipError_t e, const char* what) {
  set_error(std::string(what) + ": " + hipGetErrorString(e));
  return VN_EHIP;
}
const std::string& last_error() { return g_last_error; }

struct SceneDev {
  int64_t row_base;  // first arena row (frame) of the scene
  int64_t spd_off;   // element offset of the scene's [N][N] spd block (and curriculum order block)
  int64_t cnt_off;   // element offset of the scene's [N][maxd+2] curriculum count block
  int64_t comp_base; // first arena row of the scene's companion frames, -1 = second output is the goal frame
  int32_t graph_off; // first row of the scene's [N][4] adjacency block
  int32_t n;         // states
  int32_t maxd;      // largest spd value of the scene
  int32_t cur_oi;    // curriculum threshold floor(c*(maxd+offset)+1) clamped to [0, maxd] (host, fp64)
  int32_t cur_mode;  // 0 off, 1 uniform over 0 < spd <= opt, 2 0.9 / 0.1 split (graph/util.py:88-117)
  float r_goal, r_step, r_coll;
  int32_t terminal_obs;
};

enum { ST_SCENE = 0, ST_STATE, ST_GOAL, ST_OBS, ST_ELAPSED, ST_EPISODE, ST_SCHED, ST_COUNT };

// The per-env record, as 32-bit words (floats as their bits). Words 0..17 are what a step
// reads and, up to word 11, rewrites; 12..17 change only when a reset changes the scene.
enum {
  RW_ST = 0,          // [ST_COUNT] state words, in vn_get_state's order
  RW_RET = 7,         // running return of the unfinished episode (f32)
  RW_NB = 8,          // [4] graph[state][0..3] of the current scene
  RW_ROW_BASE = 12,   // SceneDev::row_base
  RW_COMP_BASE = 13,  // SceneDev::comp_base (-1 = none)
  RW_GRAPH_TOBS = 14, // SceneDev::graph_off << 1 | (terminal_obs != 0)
  RW_R_GOAL = 15,     // the scene's three rewards (f32)
  RW_R_STEP = 16,
  RW_R_COLL = 17,
  RW_OUT_ROW = 18,    // [2] arena row last written to the image / goal output row
  RW_OUT_ADDR = 20,   // [2] x 64 bit: that output row's address (0 matches nothing); bit 63
                      // (kOutF32) set when the row was written as f32 planes, not u8 HWC
  RW_USED = 24,
  RW_WORDS = 32,
};
struct alignas(128) EnvRec {
  int32_t w[RW_WORDS];
};
static_assert(sizeof(EnvRec) == 128, "one record per 128-B line");
// what the nav kernels (vn_nav.hip) read of a record
static_assert(NAV_RW_SCENE == RW_ST + ST_SCENE && NAV_RW_STATE == RW_ST + ST_STATE && NAV_RW_GOAL == RW_ST + ST_GOAL &&
                  NAV_RW_ELAPSED == RW_ST + ST_ELAPSED && NAV_RW_NB == RW_NB && NAV_REC_WORDS == RW_WORDS,
              "vn_nav.h restates the record layout");
// A u8 row and an f32 row at one address are different contents: the record tells them apart
// on the device, so replayed graphs and interleaved vn_step / vn_step_f32 calls stay correct.
constexpr uint64_t kOutF32 = 1ull << 63;

// The output-reuse records of the three auxiliary frames (vn_step_aux / vn_observe_aux: depth,
// segmentation, goal segmentation): EnvRec has 8 free words and these need 9, so they live in
// an array of their own, allocated with vn_set_aux_arena and touched only by the five-frame
// instantiations. Same meaning as RW_OUT_ROW / RW_OUT_ADDR, the rows being aux-arena rows.
enum {
  AW_ROW = 0,   // [3] aux-arena row last written to the depth / segmentation / goal segmentation row
  AW_ADDR = 4,  // [3] x 64 bit: that output row's address | kOutF32 (0 matches nothing)
  AW_USED = 10,
  AW_WORDS = 16,
};
struct alignas(64) AuxRec {
  int32_t w[AW_WORDS];
};
static_assert(sizeof(AuxRec) == 64, "one aux record per 64-B line");

typedef int32_t i32x16 __attribute__((ext_vector_type(16), may_alias, aligned(64)));
typedef int32_t i32x8 __attribute__((ext_vector_type(8), may_alias, aligned(32)));
typedef int32_t i32x4 __attribute__((ext_vector_type(4), may_alias, aligned(16)));
typedef int32_t i32x2 __attribute__((ext_vector_type(2), may_alias, aligned(8)));

struct EnvArgs {
  const SceneDev* scenes;
  const int32_t* graph;
  const int32_t* spd;
  const uint8_t* arena;
  int64_t frame_bytes;
  EnvRec* recs;  // [n_envs]
  const int32_t* env_scene;
  const int32_t* tasks;
  const int32_t* sched;
  const int32_t* cur_order;  // per scene, per goal: states sorted by spd[s][g] (stable)
  const int32_t* cur_count;  // per scene, per goal: #states with clamp(spd,-1,maxd)+1 <= b
  uint32_t* flags;
  int n_tasks, sched_len, max_steps, autoreset, n_envs;
  int cur_mode;  // any scene with a curriculum (the per-scene mode is SceneDev::cur_mode)
  uint32_t k0, k1;
  // per call
  const int32_t* actions;
  const int32_t* mask;
  uint8_t* obs;
  uint8_t* goal_out;
  float* reward;
  uint8_t* done;
  int32_t* state_out;
  float* info_ret;
  int32_t* info_len;
  int32_t* info_term;
  uint8_t* info_trunc;
  int32_t* info_img_row;
  int32_t* info_goal_row;
  // vn_step_a2c: action sampled in the step, then the rollout's per-step bookkeeping
  const float* pol_out;
  int pol_A;
  uint32_t pk0, pk1;
  const int64_t* pctr_dev;
  uint64_t pctr;
  int32_t* act_out;
  int64_t* prev_action;
  float* prev_reward;
  float* prev_mask;
  float* lra_next;
  float* mask_next;
  float* stats_env;
  const float* head_w;  // optional: heads computed here (vn_a2c_step.head_weight)
  const float* head_b;
  const float* head_x;
  float* head_out;
  // output reuse (DESIGN.md "vn_step: output reuse"): whether this launch may skip a frame
  // whose destination row already holds it (the record's RW_OUT_* words say what it holds)
  int reuse;
  // float observations (FMT_F32 instantiations only): pixels per frame (H W) and channels;
  // obs / goal_out then point at float [n_envs][C][H][W]
  int px, ch;
};

// The five-frame instantiations' arguments (vn_step_aux / vn_observe_aux): EnvArgs, which
// stays the kernel argument of every other instantiation, plus the aux arenas, the three
// further outputs (any may be NULL: not written, record left alone) and their records.
struct EnvAuxArgs : EnvArgs {
  const uint8_t* depth_arena;  // [rows][px][dch]
  const uint8_t* seg_arena;    // [rows][px][sch]
  AuxRec* arecs;               // [n_envs]
  uint8_t* out_depth;          // u8 [E][px][dch], or float [E][dch][px]
  uint8_t* out_seg;
  uint8_t* out_gseg;
  int dch, sch;
};

// MODE_STEP_HEADS: a step of vn_step_a2c that also computes the policy heads (its own
// instantiation, so the plain step keeps its register budget)
enum { MODE_STEP = 0, MODE_RESET = 1, MODE_OBSERVE = 2, MODE_STEP_HEADS = 3 };
// The frame tail's output format: u8 HWC rows (VEC = 16 / 4 / 1 bytes per lane), or f32 CHW
// rows (VEC = 16: the 4-pixel lanes of cvt_two_frames, VEC = 4: cvt_frames_scalar). Own
// instantiations, so the u8 kernels are the code they were.
enum { FMT_U8 = 0, FMT_F32 = 1 };
// AUX = 1: the five-frame tail (image, goal, depth, segmentation, goal segmentation) of
// vn_step_aux / vn_observe_aux, taking EnvAuxArgs. A template parameter of its own, so every
// AUX = 0 instantiation keeps its code and its kernel argument.
template <int AUX>
struct env_args_of {
  typedef EnvArgs type;
};
template <>
struct env_args_of<1> {
  typedef EnvAuxArgs type;
};
constexpr int kEnvsPerBlock = 4;
constexpr int kStartRounds = 16;  // 1024 rejection attempts before flagging

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

// Wave-cooperative reset of env e (all 64 lanes call with uniform arguments). k is the env's
// reset count, sp its schedule position (advanced here when the schedule supplies the pair).
__device__ void reset_env(const EnvArgs& a, int e, int lane, int k, int& sp, int& sc, int& s, int& g) {
  if (a.sched_len > 0 && sp < a.sched_len) {
    sc = a.env_scene[e];
    const int n = a.scenes[sc].n;
    s = a.sched[((int64_t)e * a.sched_len + sp) * 2 + 0];
    g = a.sched[((int64_t)e * a.sched_len + sp) * 2 + 1];
    if ((unsigned)s >= (unsigned)n || (unsigned)g >= (unsigned)n) {
      if (lane == 0) atomicOr(a.flags, (uint32_t)VN_FLAG_BAD_SCHEDULE);
      s = min(max(s, 0), n - 1);
      g = min(max(g, 0), n - 1);
    }
    sp += 1;
    return;
  }
  const u32x4 rg = philox4x32_10(u32x4{(uint32_t)e, (uint32_t)k, 0u, STREAM_GOAL}, a.k0, a.k1);
  if (a.n_tasks > 0) {
    const int t = (int)uniform_below(rg.x, (uint32_t)a.n_tasks);
    sc = a.tasks[2 * t];
    g = a.tasks[2 * t + 1];
    if (g < 0) g = (int)uniform_below(rg.y, (uint32_t)a.scenes[sc].n);
  } else {
    sc = a.env_scene[e];
    g = (int)uniform_below(rg.x, (uint32_t)a.scenes[sc].n);
  }
  const SceneDev S = a.scenes[sc];
  const int32_t* spd = a.spd + S.spd_off;
  s = -1;
  if (a.cur_mode > 0 && S.cur_mode > 0) {
    // curriculum (graph/util.py:88-143, environments/gym_graph/graph.py:43-52):
    // opt = c * (maxd + offset) + 1 (S.cur_oi = its floor); candidates 0 < spd <= opt, uniform (mode 1) or
    // 0.9 over them / 0.1 over the farther ones (mode 2); one O(1) draw from the sorted table
    const int oi = S.cur_oi;
    const int32_t* cnt = a.cur_count + S.cnt_off + (int64_t)g * (S.maxd + 2);
    const int lo = cnt[1], hi = cnt[oi + 1], n = S.n;
    const u32x4 r = philox4x32_10(u32x4{(uint32_t)e, (uint32_t)k, 0u, STREAM_START}, a.k0, a.k1);
    // far set when the 0.1 coin says so (and it is not empty) or when the near set is empty
    const bool use_far = (S.cur_mode == 2 && r.y >= 3865470566u && hi < n) || hi <= lo;  // 0.9 * 2^32
    const int b0 = use_far ? hi : lo, b1 = use_far ? n : hi;
    if (b1 > b0) s = a.cur_order[S.spd_off + (int64_t)g * n + b0 + (int)uniform_below(r.x, (uint32_t)(b1 - b0))];
  }
  for (int round = 0; round < kStartRounds && s < 0; ++round) {
    const uint32_t att = (uint32_t)(round * 64 + lane);
    const u32x4 r = philox4x32_10(u32x4{(uint32_t)e, (uint32_t)k, att, STREAM_START}, a.k0, a.k1);
    const int cand = (int)uniform_below(r.x, (uint32_t)S.n);
    const bool ok = spd[(int64_t)cand * S.n + g] > 0;
    const unsigned long long m = __ballot(ok);
    if (m) {
      s = __shfl(cand, __ffsll((long long)m) - 1);
      break;
    }
  }
  if (s < 0) {  // bounded search exhausted: flag and take attempt 0
    if (lane == 0) atomicOr(a.flags, (uint32_t)VN_FLAG_RESET_EXHAUSTED);
    const u32x4 r = philox4x32_10(u32x4{(uint32_t)e, (uint32_t)k, 0u, STREAM_START}, a.k0, a.k1);
    s = (int)uniform_below(r.x, (uint32_t)S.n);
  }
  s = uni(s);
}

// Copy the image frame and goal frame of one env: 16-B lanes, 4 x 2 loads in flight. The
// output rows are written with nontemporal (`nt`) stores; loads keep the default policy.
// Measured (tools/copybench.hip cache-policy sweep over the 16 load/store combinations, and
// the bench, tools/ab/copy_variants.sh): at 4096 envs default stores 57-60 us, any single nt
// stream 54-56 us; at 32768 envs per GPU nt on both stores 446 us (6.2 TB/s) vs 551 us
// default and 545-563 us with nt loads; nt on all four streams is the slowest everywhere.
//
// Both copy routines take `mid`, the wave's scalar work (lane 0's record and output stores):
// it runs once, after the first trip's loads are issued and before their data is waited
// for, so the first frame-data wait does not sit behind those stores' acknowledgements.
__device__ __forceinline__ void st16_nt(uint4* p, const uint4 v) {
  __builtin_nontemporal_store(v.x, &p->x);
  __builtin_nontemporal_store(v.y, &p->y);
  __builtin_nontemporal_store(v.z, &p->z);
  __builtin_nontemporal_store(v.w, &p->w);
}

template <int VEC, class Mid>
__device__ __forceinline__ void copy_two_frames(uint8_t* __restrict__ d1, const uint8_t* __restrict__ s1,
                                                uint8_t* __restrict__ d2, const uint8_t* __restrict__ s2,
                                                int64_t bytes, int lane, Mid mid) {
  if constexpr (VEC == 16) {
    constexpr int U = 4;
    const int n = (int)(bytes >> 4);
    const uint4* a = reinterpret_cast<const uint4*>(s1);
    const uint4* b = reinterpret_cast<const uint4*>(s2);
    uint4* x = reinterpret_cast<uint4*>(d1);
    uint4* y = reinterpret_cast<uint4*>(d2);
    int i = lane;
    {  // first trip, mid() inside it. Its U loads per stream are always issued, so the number
       // in flight at mid() is fixed. A frame shorter than one trip (n < 64 U) reads its first
       // chunks as a stand-in and is copied by the loops below
      const bool full = 64 * U <= n;  // wave-uniform
      const int i0 = full ? lane : min(lane, n - 1), step = full ? 64 : 0;
      uint4 va[U], vb[U];
#pragma unroll
      for (int u = 0; u < U; ++u) va[u] = a[i0 + step * u];
#pragma unroll
      for (int u = 0; u < U; ++u) vb[u] = b[i0 + step * u];
      mid();
      if (full) {
#pragma unroll
        for (int u = 0; u < U; ++u) st16_nt(x + i + 64 * u, va[u]);
#pragma unroll
        for (int u = 0; u < U; ++u) st16_nt(y + i + 64 * u, vb[u]);
        i += 64 * U;
      }
    }
    for (; i + 64 * (U - 1) < n; i += 64 * U) {
      uint4 va[U], vb[U];
#pragma unroll
      for (int u = 0; u < U; ++u) va[u] = a[i + 64 * u];
#pragma unroll
      for (int u = 0; u < U; ++u) vb[u] = b[i + 64 * u];
#pragma unroll
      for (int u = 0; u < U; ++u) st16_nt(x + i + 64 * u, va[u]);
#pragma unroll
      for (int u = 0; u < U; ++u) st16_nt(y + i + 64 * u, vb[u]);
    }
    for (; i < n; i += 64) {
      const uint4 a0 = a[i], b0 = b[i];
      st16_nt(x + i, a0);
      st16_nt(y + i, b0);
    }
  } else if constexpr (VEC == 4) {
    mid();
    const int n = (int)(bytes >> 2);
    const uint32_t* a = reinterpret_cast<const uint32_t*>(s1);
    const uint32_t* b = reinterpret_cast<const uint32_t*>(s2);
    uint32_t* x = reinterpret_cast<uint32_t*>(d1);
    uint32_t* y = reinterpret_cast<uint32_t*>(d2);
    for (int i = lane; i < n; i += 64) {
      const uint32_t a0 = a[i], b0 = b[i];
      x[i] = a0;
      y[i] = b0;
    }
  } else {
    mid();
    for (int64_t i = lane; i < bytes; i += 64) {
      d1[i] = s1[i];
      d2[i] = s2[i];
    }
  }
}

// Copy one frame (the other one of the env is already in its output row): the same 8 x 16 B
// in flight per lane as copy_two_frames, on one stream. The trip count is wave-uniform; the
// remainder (1323 uint4 per 84x84x3 frame = 2 trips of 512 + 299) issues all its predicated
// loads before its stores.
template <int VEC, class Mid>
__device__ __forceinline__ void copy_one_frame(uint8_t* __restrict__ d, const uint8_t* __restrict__ s,
                                               int64_t bytes, int lane, Mid mid) {
  if constexpr (VEC == 16) {
    constexpr int U = 8;
    const int n = (int)(bytes >> 4);
    const uint4* a = reinterpret_cast<const uint4*>(s);
    uint4* x = reinterpret_cast<uint4*>(d);
    int base = 0;
    {  // first trip, mid() inside it: always U loads (see copy_two_frames)
      const bool full = 64 * U <= n;  // wave-uniform
      const int i0 = full ? lane : min(lane, n - 1), step = full ? 64 : 0;
      uint4 v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) v[u] = a[i0 + step * u];
      mid();
      if (full) {
#pragma unroll
        for (int u = 0; u < U; ++u) st16_nt(x + lane + 64 * u, v[u]);
        base = 64 * U;
      }
    }
    for (; base + 64 * U <= n; base += 64 * U) {
      const int i = base + lane;
      uint4 v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) v[u] = a[i + 64 * u];
#pragma unroll
      for (int u = 0; u < U; ++u) st16_nt(x + i + 64 * u, v[u]);
    }
    if (base < n) {
      const int i = base + lane;
      uint4 v[U] = {};
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (i + 64 * u < n) v[u] = a[i + 64 * u];
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (i + 64 * u < n) st16_nt(x + i + 64 * u, v[u]);
    }
  } else if constexpr (VEC == 4) {
    mid();
    const int n = (int)(bytes >> 2);
    const uint32_t* a = reinterpret_cast<const uint32_t*>(s);
    uint32_t* x = reinterpret_cast<uint32_t*>(d);
    for (int i = lane; i < n; i += 64) x[i] = a[i];
  } else {
    mid();
    for (int64_t i = lane; i < bytes; i += 64) d[i] = s[i];
  }
}

// Float observations (vn_step_f32 / vn_observe_f32; DESIGN.md "vn_step: float observations"):
// the u8 HWC arena row leaves as three f32 planes [3][H][W] of float(u8) / 255
// (unit_from_byte_value: the division's bits). A lane owns 4 consecutive pixels, group q:
// one 12-B load at byte 12 q (a wave instruction reads 768 contiguous bytes), 12
// conversions, and one 16-B nt store per plane at float 4 q (a wave instruction writes 1024
// contiguous bytes of a plane), so nothing is staged in LDS and no line is stored in parts.
// Needs P = H W a multiple of 4 and 16-B aligned planes; anything else takes cvt_frames_scalar.
typedef uint32_t u32x3 __attribute__((ext_vector_type(3), may_alias, aligned(4)));
typedef float f32x4 __attribute__((ext_vector_type(4), may_alias, aligned(16)));

__device__ __forceinline__ u32x3 ld12(const uint8_t* __restrict__ s, int q) {
  return *reinterpret_cast<const u32x3*>(s + 12 * q);
}
template <int K>
__device__ __forceinline__ float unit_byte(uint32_t w) {
  return unit_from_byte_value((float)((w >> (8 * K)) & 0xffu));  // v_cvt_f32_ubyteK
}
// bytes r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3 of pixels 4 q .. 4 q + 3
__device__ __forceinline__ void cvt_store12(float* __restrict__ d, int P, int q, const u32x3 w) {
  // one plane's 4 floats are converted and stored at a time (the scheduling barriers): left
  // to itself the scheduler converts a whole trip before its first store (132 VGPRs, 3 waves
  // per SIMD), and with a barrier per group only it still needs 84
  __builtin_amdgcn_sched_barrier(0);
  const f32x4 pr = {unit_byte<0>(w.x), unit_byte<3>(w.x), unit_byte<2>(w.y), unit_byte<1>(w.z)};
  __builtin_nontemporal_store(pr, reinterpret_cast<f32x4*>(d + 4 * q));
  __builtin_amdgcn_sched_barrier(0);
  const f32x4 pg = {unit_byte<1>(w.x), unit_byte<0>(w.y), unit_byte<3>(w.y), unit_byte<2>(w.z)};
  __builtin_nontemporal_store(pg, reinterpret_cast<f32x4*>(d + P + 4 * q));
  __builtin_amdgcn_sched_barrier(0);
  const f32x4 pb = {unit_byte<2>(w.x), unit_byte<1>(w.y), unit_byte<0>(w.z), unit_byte<3>(w.z)};
  __builtin_nontemporal_store(pb, reinterpret_cast<f32x4*>(d + 2 * P + 4 * q));
  __builtin_amdgcn_sched_barrier(0);
}

// Both frames of one env: 4 + 4 loads of 12 B in flight per lane, a trip is 256 groups
// (1024 pixels) of each frame. The structure is copy_two_frames': a first trip with a fixed
// load count around mid(), wave-uniform full trips, and a remainder (84 x 84 = 1764 groups =
// 6 trips + 228) whose predicated loads are all issued before its stores.
template <class Mid>
__device__ __forceinline__ void cvt_two_frames(float* __restrict__ d1, const uint8_t* __restrict__ s1,
                                               float* __restrict__ d2, const uint8_t* __restrict__ s2, int P,
                                               int lane, Mid mid) {
  constexpr int U = 4;
  const int n = P >> 2;
  int base = 0;
  {  // first trip, mid() inside it: always U loads per stream (see copy_two_frames)
    const bool full = 64 * U <= n;  // wave-uniform
    const int i0 = full ? lane : min(lane, n - 1), step = full ? 64 : 0;
    u32x3 va[U], vb[U];
#pragma unroll
    for (int u = 0; u < U; ++u) va[u] = ld12(s1, i0 + step * u);
#pragma unroll
    for (int u = 0; u < U; ++u) vb[u] = ld12(s2, i0 + step * u);
    mid();
    if (full) {
#pragma unroll
      for (int u = 0; u < U; ++u) cvt_store12(d1, P, lane + 64 * u, va[u]);
#pragma unroll
      for (int u = 0; u < U; ++u) cvt_store12(d2, P, lane + 64 * u, vb[u]);
      base = 64 * U;
    }
  }
  for (; base + 64 * U <= n; base += 64 * U) {
    const int i = base + lane;
    u32x3 va[U], vb[U];
#pragma unroll
    for (int u = 0; u < U; ++u) va[u] = ld12(s1, i + 64 * u);
#pragma unroll
    for (int u = 0; u < U; ++u) vb[u] = ld12(s2, i + 64 * u);
#pragma unroll
    for (int u = 0; u < U; ++u) cvt_store12(d1, P, i + 64 * u, va[u]);
#pragma unroll
    for (int u = 0; u < U; ++u) cvt_store12(d2, P, i + 64 * u, vb[u]);
  }
  if (base < n) {
    const int i = base + lane;
    u32x3 va[U] = {}, vb[U] = {};
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (i + 64 * u < n) va[u] = ld12(s1, i + 64 * u);
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (i + 64 * u < n) vb[u] = ld12(s2, i + 64 * u);
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (i + 64 * u < n) cvt_store12(d1, P, i + 64 * u, va[u]);
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (i + 64 * u < n) cvt_store12(d2, P, i + 64 * u, vb[u]);
  }
}

// One frame (the other one of the env is already in its output row): the same 8 loads in
// flight on one stream, a trip is 512 groups (2048 pixels); 84 x 84 = 3 trips + 228.
template <class Mid>
__device__ __forceinline__ void cvt_one_frame(float* __restrict__ d, const uint8_t* __restrict__ s, int P, int lane,
                                              Mid mid) {
  constexpr int U = 8;
  const int n = P >> 2;
  int base = 0;
  {  // first trip, mid() inside it: always U loads
    const bool full = 64 * U <= n;  // wave-uniform
    const int i0 = full ? lane : min(lane, n - 1), step = full ? 64 : 0;
    u32x3 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = ld12(s, i0 + step * u);
    mid();
    if (full) {
#pragma unroll
      for (int u = 0; u < U; ++u) cvt_store12(d, P, lane + 64 * u, v[u]);
      base = 64 * U;
    }
  }
  for (; base + 64 * U <= n; base += 64 * U) {
    const int i = base + lane;
    u32x3 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = ld12(s, i + 64 * u);
#pragma unroll
    for (int u = 0; u < U; ++u) cvt_store12(d, P, i + 64 * u, v[u]);
  }
  if (base < n) {
    const int i = base + lane;
    u32x3 v[U] = {};
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (i + 64 * u < n) v[u] = ld12(s, i + 64 * u);
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (i + 64 * u < n) cvt_store12(d, P, i + 64 * u, v[u]);
  }
}

// A one-channel frame (the depth row of vn_step_aux): the row is its own plane. A lane owns the
// same 4 consecutive pixels, group q: one 4-B load at byte 4 q (a wave instruction reads 256
// contiguous bytes), 4 conversions, one 16-B nt store at float 4 q (1024 contiguous bytes).
// Each group is converted and stored between scheduling barriers, as in cvt_store12, so a
// trip's conversions are not all done before its first store.
__device__ __forceinline__ uint32_t ld4(const uint8_t* __restrict__ s, int q) {
  return *reinterpret_cast<const uint32_t*>(s + 4 * q);
}
__device__ __forceinline__ void cvt_store4(float* __restrict__ d, int q, const uint32_t w) {
  __builtin_amdgcn_sched_barrier(0);
  const f32x4 v = {unit_byte<0>(w), unit_byte<1>(w), unit_byte<2>(w), unit_byte<3>(w)};
  __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(d + 4 * q));
  __builtin_amdgcn_sched_barrier(0);
}

// cvt_one_frame's structure on one plane: 8 loads in flight per lane, a trip is 512 groups
// (2048 pixels): 84 x 84 = 3 trips + 228, 64 x 64 = 2 trips exactly. A first trip with a fixed
// load count around mid(), wave-uniform full trips, and a remainder whose predicated loads
// are all issued before its stores.
template <class Mid>
__device__ __forceinline__ void cvt_one_plane(float* __restrict__ d, const uint8_t* __restrict__ s, int P, int lane,
                                              Mid mid) {
  constexpr int U = 8;
  const int n = P >> 2;
  int base = 0;
  {  // first trip, mid() inside it: always U loads
    const bool full = 64 * U <= n;  // wave-uniform
    const int i0 = full ? lane : min(lane, n - 1), step = full ? 64 : 0;
    uint32_t v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = ld4(s, i0 + step * u);
    mid();
    if (full) {
#pragma unroll
      for (int u = 0; u < U; ++u) cvt_store4(d, lane + 64 * u, v[u]);
      base = 64 * U;
    }
  }
  for (; base + 64 * U <= n; base += 64 * U) {
    const int i = base + lane;
    uint32_t v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = ld4(s, i + 64 * u);
#pragma unroll
    for (int u = 0; u < U; ++u) cvt_store4(d, i + 64 * u, v[u]);
  }
  if (base < n) {
    const int i = base + lane;
    uint32_t v[U] = {};
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (i + 64 * u < n) v[u] = ld4(s, i + 64 * u);
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (i + 64 * u < n) cvt_store4(d, i + 64 * u, v[u]);
  }
}

// The fallback (P % 4 != 0, channels != 3 or planes that are only 4-B aligned): one element
// per lane and trip, plane by plane. d2 / s2 may be NULL (one frame).
__device__ __forceinline__ void cvt_frames_scalar(float* __restrict__ d1, const uint8_t* __restrict__ s1,
                                                  float* __restrict__ d2, const uint8_t* __restrict__ s2, int P,
                                                  int C, int lane) {
  for (int c = 0; c < C; ++c) {
    for (int p = lane; p < P; p += 64) {
      d1[(int64_t)c * P + p] = unit_from_u8(s1[(int64_t)p * C + c]);
      if (d2) d2[(int64_t)c * P + p] = unit_from_u8(s2[(int64_t)p * C + c]);
    }
  }
}

// The scene fields a record caches (a reset or vn_set_state may change the env's scene).
struct SceneCache {
  int32_t row_base, comp_base;
  uint32_t graph_tobs;
  float r_goal, r_step, r_coll;
};
__device__ __forceinline__ SceneCache scene_cache(const SceneDev& S) {
  return SceneCache{(int32_t)S.row_base, (int32_t)S.comp_base,
                    ((uint32_t)S.graph_off << 1) | (S.terminal_obs != 0 ? 1u : 0u), S.r_goal, S.r_step, S.r_coll};
}
__device__ __forceinline__ void store_scene_cache(EnvRec* R, const SceneCache& c) {
  *reinterpret_cast<i32x4*>(R->w + RW_ROW_BASE) =
      i32x4{c.row_base, c.comp_base, (int32_t)c.graph_tobs, __float_as_int(c.r_goal)};
  *reinterpret_cast<i32x2*>(R->w + RW_R_STEP) = i32x2{__float_as_int(c.r_step), __float_as_int(c.r_coll)};
}
__device__ __forceinline__ void store_out_record(EnvRec* R, int32_t row1, int32_t row2, uint64_t a1, uint64_t a2) {
  *reinterpret_cast<i32x2*>(R->w + RW_OUT_ROW) = i32x2{row1, row2};
  *reinterpret_cast<i32x4*>(R->w + RW_OUT_ADDR) =
      i32x4{(int32_t)(uint32_t)a1, (int32_t)(uint32_t)(a1 >> 32), (int32_t)(uint32_t)a2, (int32_t)(uint32_t)(a2 >> 32)};
}

// One frame of the five-frame tail (vn_step_aux): its output row, its arena row, the row's
// elements and channels. VEC / FMT pick the loop as in the two-frame tails; the float vector
// form is launched only for 3-channel frames with a 1-channel depth, which takes cvt_one_plane.
struct AuxFrame {
  uint8_t* d;
  const uint8_t* s;
  int64_t n;
  int ch;
};
// frame k of the five: image, goal, depth, segmentation, goal segmentation
__device__ __forceinline__ AuxFrame aux_frame(const EnvAuxArgs& a, int k, int32_t img_row, int32_t goal_row, int64_t n0,
                                              int64_t n2, int64_t n3, uint8_t* d0, uint8_t* d1, uint8_t* d2,
                                              uint8_t* d3, uint8_t* d4) {
  const int32_t row = (k == 1 || k == 4) ? goal_row : img_row;
  const uint8_t* base = k < 2 ? a.arena : k == 2 ? a.depth_arena : a.seg_arena;
  const int64_t n = k < 2 ? n0 : k == 2 ? n2 : n3;
  return AuxFrame{k == 0 ? d0 : k == 1 ? d1 : k == 2 ? d2 : k == 3 ? d3 : d4, base + (int64_t)row * n, n,
                  k < 2 ? a.ch : k == 2 ? a.dch : a.sch};
}
template <int VEC, int FMT, class Mid>
__device__ __forceinline__ void write_one_frame(const AuxFrame f, int P, int lane, Mid mid) {
  if constexpr (FMT == FMT_U8) {
    copy_one_frame<VEC>(f.d, f.s, f.n, lane, mid);
  } else if constexpr (VEC == 16) {
    if (f.ch == 1)
      cvt_one_plane(reinterpret_cast<float*>(f.d), f.s, P, lane, mid);
    else
      cvt_one_frame(reinterpret_cast<float*>(f.d), f.s, P, lane, mid);
  } else {
    mid();
    cvt_frames_scalar(reinterpret_cast<float*>(f.d), f.s, nullptr, nullptr, P, f.ch, lane);
  }
}

__device__ __forceinline__ void store_aux_record(AuxRec* A, int32_t r0, int32_t r1, int32_t r2, uint64_t a0,
                                                 uint64_t a1, uint64_t a2) {
  *reinterpret_cast<i32x4*>(A->w + AW_ROW) = i32x4{r0, r1, r2, 0};
  *reinterpret_cast<i32x4*>(A->w + AW_ADDR) =
      i32x4{(int32_t)(uint32_t)a0, (int32_t)(uint32_t)(a0 >> 32), (int32_t)(uint32_t)a1, (int32_t)(uint32_t)(a1 >> 32)};
  *reinterpret_cast<i32x2*>(A->w + AW_ADDR + 4) = i32x2{(int32_t)(uint32_t)a2, (int32_t)(uint32_t)(a2 >> 32)};
}

template <int MODE, int VEC, int FMT = FMT_U8, int AUX = 0>
__global__ __launch_bounds__(256) void env_kernel(typename env_args_of<AUX>::type a) {
  const int lane = threadIdx.x & 63;
  const int e = uni(blockIdx.x * kEnvsPerBlock + (threadIdx.x >> 6));
  if (e >= a.n_envs) return;
  const int n_envs = a.n_envs;
  EnvRec* R = a.recs + e;

  // the whole record, wave-uniform, in two scalar loads issued together (before any store
  // of the wave)
  const i32x16 lo = *reinterpret_cast<const i32x16*>(R->w);
  const i32x8 hi = *reinterpret_cast<const i32x8*>(R->w + 16);
  int sc = lo[ST_SCENE], s = lo[ST_STATE], g = lo[ST_GOAL], os = lo[ST_OBS];
  int t = lo[ST_ELAPSED], ep = lo[ST_EPISODE], sp = lo[ST_SCHED];
  SceneCache C{lo[RW_ROW_BASE], lo[RW_COMP_BASE], (uint32_t)lo[RW_GRAPH_TOBS], __int_as_float(lo[RW_R_GOAL]),
               __int_as_float(hi[RW_R_STEP - 16]), __int_as_float(hi[RW_R_COLL - 16])};
  const int32_t rec_r1 = hi[RW_OUT_ROW - 16], rec_r2 = hi[RW_OUT_ROW + 1 - 16];
  const uint64_t rec_a1 = (uint32_t)hi[RW_OUT_ADDR - 16] | ((uint64_t)(uint32_t)hi[RW_OUT_ADDR + 1 - 16] << 32);
  const uint64_t rec_a2 = (uint32_t)hi[RW_OUT_ADDR + 2 - 16] | ((uint64_t)(uint32_t)hi[RW_OUT_ADDR + 3 - 16] << 32);
  // the aux frames' record, issued with the two loads above (five-frame instantiations only)
  i32x16 ax = {};
  if constexpr (AUX != 0) ax = *reinterpret_cast<const i32x16*>(a.arecs[e].w);

  // the caller's action, loaded together with the record (vn_step_a2c samples its own)
  int act_in = 0;
  if constexpr (MODE == MODE_STEP) {
    if (a.actions) act_in = a.actions[e];
  }

  // what lane 0 stores once the frame address is known (MODE_STEP / MODE_STEP_HEADS)
  bool scene_changed = false, bad = false, done = false, limit = false, terminal = false;
  int act = 0, term_state = 0, ep_len = 0;
  float r = 0.0f, ret = 0.0f, new_ret = 0.0f;

  if constexpr (MODE == MODE_STEP || MODE == MODE_STEP_HEADS) {
    if (a.pol_out) {  // the policy's categorical draw for this env (vn_policy_sample_dev's)
      float lg[7], p[7], lp[7], H;
      if constexpr (MODE == MODE_STEP_HEADS) {
        // the heads of this env (logits, value): vn_policy_heads' skinny product for one row —
        // 32 lanes, 4 consecutive k at 4 kl + 128 i, fma chains, a 32-lane xor tree, + bias:
        // the same sums in the same order (both 32-lane halves compute them)
        const int kl = lane & 31;
        const float* x = a.head_x + (int64_t)e * 512;
        float4 xv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) xv[i] = *reinterpret_cast<const float4*>(x + 4 * kl + 128 * i);
        float sj[8], bj[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) bj[j] = a.head_b[min(j, a.pol_A)];
#pragma unroll
        for (int j = 0; j < 8; ++j) {  // all rows' loads in flight together (A + 1 <= 8)
          const float* w = a.head_w + (int64_t)min(j, a.pol_A) * 512;
          float s = 0.0f;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float4 wv = *reinterpret_cast<const float4*>(w + 4 * kl + 128 * i);
            s = fmaf(xv[i].x, wv.x, s);
            s = fmaf(xv[i].y, wv.y, s);
            s = fmaf(xv[i].z, wv.z, s);
            s = fmaf(xv[i].w, wv.w, s);
          }
          sj[j] = s;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
#pragma unroll
          for (int o = 16; o > 0; o >>= 1) sj[j] += __shfl_xor(sj[j], o, 32);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if (j <= a.pol_A) {
            const float v = sj[j] + bj[j];
            if (j < a.pol_A) lg[j] = v;
            if (lane == 0) a.head_out[(int64_t)e * 8 + j] = v;
          }
        }
      } else {
        for (int j = 0; j < a.pol_A; ++j) lg[j] = a.pol_out[(int64_t)e * 8 + j];
      }
      const uint64_t ctr = a.pctr + (a.pctr_dev ? (uint64_t)*a.pctr_dev : 0ull);
      act = uni(sample_action(lg, a.pol_A, a.pk0, a.pk1, ctr, (uint32_t)e, p, lp, H));
    } else {
      act = act_in;
    }
    // the transition comes from the record's cached neighbours: no graph load on this path
    bad = (unsigned)act > 3u;
    int nxt = -1;
    if (!bad) nxt = act == 0 ? lo[RW_NB] : act == 1 ? lo[RW_NB + 1] : act == 2 ? lo[RW_NB + 2] : lo[RW_NB + 3];
    const bool collided = nxt == -1;
    if (!collided) s = nxt;
    terminal = (s == g);
    r = C.r_step;
    if (terminal) r = C.r_goal;
    if (collided) r = C.r_coll;
    if (!terminal || (C.graph_tobs & 1u)) os = s;
    t += 1;
    limit = a.max_steps > 0 && t >= a.max_steps;
    done = terminal || limit;
    ret = __int_as_float(lo[RW_RET]) + r;
    term_state = os;
    ep_len = t;
    new_ret = ret;
    if (done && a.autoreset) {  // rare: the slower path re-reads the scene table
      reset_env(a, e, lane, ep, sp, sc, s, g);
      os = s;
      t = 0;
      ep += 1;
      new_ret = 0.0f;
      C = scene_cache(a.scenes[sc]);
      scene_changed = true;
    }
  } else if constexpr (MODE == MODE_RESET) {
    if (a.mask == nullptr || a.mask[e] != 0) {
      reset_env(a, e, lane, ep, sp, sc, s, g);
      C = scene_cache(a.scenes[sc]);
      const i32x4 nb = *reinterpret_cast<const i32x4*>(a.graph + ((int64_t)(C.graph_tobs >> 1) + s) * 4);
      if (lane == 0) {
        *reinterpret_cast<i32x4*>(R->w + 0) = i32x4{sc, s, g, s};
        *reinterpret_cast<i32x4*>(R->w + 4) = i32x4{0, ep + 1, sp, __float_as_int(0.0f)};
        *reinterpret_cast<i32x4*>(R->w + RW_NB) = nb;
        store_scene_cache(R, C);
      }
    }
    return;
  }

  // the new state's neighbours, for the next step's record: needed only by lane 0's stores,
  // which follow the first frame loads
  i32x4 nb = i32x4{lo[RW_NB], lo[RW_NB + 1], lo[RW_NB + 2], lo[RW_NB + 3]};
  if constexpr (MODE == MODE_STEP || MODE == MODE_STEP_HEADS)
    nb = *reinterpret_cast<const i32x4*>(a.graph + ((int64_t)(C.graph_tobs >> 1) + s) * 4);

  const int32_t img_row = C.row_base + os, goal_row = C.comp_base >= 0 ? C.comp_base + os : C.row_base + g;

  // lane 0's stores: the record, the step's scalar outputs, the a2c bookkeeping. row1/row2,
  // addr1/addr2: the output record to leave (written when `out_rec`).
  auto emit = [&](bool out_rec, int32_t row1, int32_t row2, uint64_t addr1, uint64_t addr2)
                  __attribute__((always_inline)) {
    if (lane != 0) return;
    if constexpr (MODE == MODE_STEP || MODE == MODE_STEP_HEADS) {
      *reinterpret_cast<i32x4*>(R->w + 0) = i32x4{sc, s, g, os};
      *reinterpret_cast<i32x4*>(R->w + 4) = i32x4{t, ep, sp, __float_as_int(new_ret)};
      *reinterpret_cast<i32x4*>(R->w + RW_NB) = nb;
      if (scene_changed) store_scene_cache(R, C);
    }
    if (out_rec) store_out_record(R, row1, row2, addr1, addr2);
    if constexpr (MODE == MODE_STEP || MODE == MODE_STEP_HEADS) {
      if (bad) atomicOr(a.flags, (uint32_t)VN_FLAG_BAD_ACTION);
      if (a.reward) a.reward[e] = r;
      if (a.done) a.done[e] = done ? 1 : 0;
      if (a.state_out) a.state_out[e] = s;
      if (a.info_ret) a.info_ret[e] = ret;
      if (a.info_len) a.info_len[e] = ep_len;
      if (a.info_term) a.info_term[e] = term_state;
      if (a.info_trunc) a.info_trunc[e] = (limit && !terminal) ? 1 : 0;
    } else {
      if (a.state_out) a.state_out[e] = s;
    }
    if (a.info_img_row) a.info_img_row[e] = img_row;
    if (a.info_goal_row) a.info_goal_row[e] = goal_row;
    if constexpr (MODE == MODE_STEP || MODE == MODE_STEP_HEADS) {
      if (a.pol_out) {  // vn_a2c_step_post's bookkeeping for this env
        const float m = done ? 0.0f : 1.0f;
        a.act_out[e] = act;
        if (a.prev_action) a.prev_action[e] = act;
        if (a.prev_reward) a.prev_reward[e] = r;
        if (a.prev_mask) a.prev_mask[e] = m;
        if (a.mask_next) a.mask_next[e] = m;
        if (a.lra_next) {
          for (int j = 0; j < a.pol_A; ++j) a.lra_next[(int64_t)e * (a.pol_A + 1) + j] = j == act ? m : 0.0f;
          a.lra_next[(int64_t)e * (a.pol_A + 1) + a.pol_A] = r * m;
        }
        if (a.stats_env && done) {
          a.stats_env[e] += 1.0f;
          a.stats_env[n_envs + e] += ret;
          a.stats_env[2 * (int64_t)n_envs + e] += (float)ep_len;
        }
      }
    }
  };

  if constexpr (MODE == MODE_STEP_HEADS) {  // vn_step_a2c is index-only: no frame tail
    emit(false, 0, 0, 0, 0);
    return;
  }
  if constexpr (AUX != 0) {
    // The five-frame tail: frame k = image, goal, depth, segmentation, goal segmentation, the
    // last three from the aux arenas at img_row / img_row / goal_row. One frame at a time
    // through the one-frame loops, each frame kept or written by the rule of the two-frame
    // tails (all decisions wave-uniform); lane 0's stores run inside the first trip of the
    // first frame written, or alone when all five are kept. A NULL aux output is never
    // written and keeps its record.
    constexpr uint64_t fbit = FMT == FMT_F32 ? kOutF32 : 0;
    constexpr int ES = FMT == FMT_F32 ? 4 : 1;  // bytes per output element
    const int P = a.px;
    const int64_t n0 = a.frame_bytes, n2 = (int64_t)P * a.dch, n3 = (int64_t)P * a.sch;  // elements per row
    uint8_t* d0 = a.obs + (int64_t)e * n0 * ES;
    uint8_t* d1 = a.goal_out + (int64_t)e * n0 * ES;
    uint8_t* d2 = a.out_depth ? a.out_depth + (int64_t)e * n2 * ES : nullptr;
    uint8_t* d3 = a.out_seg ? a.out_seg + (int64_t)e * n3 * ES : nullptr;
    uint8_t* d4 = a.out_gseg ? a.out_gseg + (int64_t)e * n3 * ES : nullptr;
    const uint64_t t0 = (uint64_t)d0 | fbit, t1 = (uint64_t)d1 | fbit, t2 = (uint64_t)d2 | fbit,
                   t3 = (uint64_t)d3 | fbit, t4 = (uint64_t)d4 | fbit;
    const int32_t xr2 = ax[AW_ROW], xr3 = ax[AW_ROW + 1], xr4 = ax[AW_ROW + 2];
    const uint64_t xa2 = (uint32_t)ax[AW_ADDR] | ((uint64_t)(uint32_t)ax[AW_ADDR + 1] << 32);
    const uint64_t xa3 = (uint32_t)ax[AW_ADDR + 2] | ((uint64_t)(uint32_t)ax[AW_ADDR + 3] << 32);
    const uint64_t xa4 = (uint32_t)ax[AW_ADDR + 4] | ((uint64_t)(uint32_t)ax[AW_ADDR + 5] << 32);
    int todo = 0;  // bit k: frame k is written by this launch
    if (!(a.reuse && rec_a1 == t0 && rec_r1 == img_row)) todo |= 1;
    if (!(a.reuse && rec_a2 == t1 && rec_r2 == goal_row)) todo |= 2;
    if (d2 && !(a.reuse && xa2 == t2 && xr2 == img_row)) todo |= 4;
    if (d3 && !(a.reuse && xa3 == t3 && xr3 == img_row)) todo |= 8;
    if (d4 && !(a.reuse && xa4 == t4 && xr4 == goal_row)) todo |= 16;
    auto mid = [&]() __attribute__((always_inline)) {
      emit(true, img_row, goal_row, t0, t1);
      if (lane == 0)
        store_aux_record(a.arecs + e, d2 ? img_row : xr2, d3 ? img_row : xr3, d4 ? goal_row : xr4, d2 ? t2 : xa2,
                         d3 ? t3 : xa3, d4 ? t4 : xa4);
    };
    if (todo == 0) {
      mid();
    } else {
      // the first frame written carries lane 0's stores, so what they store is dead after its
      // first trip; the others follow through the same loops with nothing in the middle
      write_one_frame<VEC, FMT>(aux_frame(a, __builtin_ctz(todo), img_row, goal_row, n0, n2, n3, d0, d1, d2, d3, d4), P,
                                lane, mid);
      todo &= todo - 1;
#pragma nounroll
      while (todo != 0) {
        write_one_frame<VEC, FMT>(aux_frame(a, __builtin_ctz(todo), img_row, goal_row, n0, n2, n3, d0, d1, d2, d3, d4),
                                  P, lane, []() {});
        todo &= todo - 1;
      }
    }
  } else if constexpr (FMT == FMT_F32) {
    // the float tail: the rows of the u8 tail below, F floats each, addresses recorded with
    // kOutF32 (a u8 record never matches here, nor a float record there)
    const int64_t F = a.frame_bytes;
    const int P = a.px;
    float* o1 = reinterpret_cast<float*>(a.obs);
    float* o2 = reinterpret_cast<float*>(a.goal_out);
    if (o1 != nullptr && o2 != nullptr) {
      float* d1 = o1 + (int64_t)e * F;
      float* d2 = o2 + (int64_t)e * F;
      const uint64_t t1 = (uint64_t)d1 | kOutF32, t2 = (uint64_t)d2 | kOutF32;
      const bool keep1 = a.reuse && rec_a1 == t1 && rec_r1 == img_row;
      const bool keep2 = a.reuse && rec_a2 == t2 && rec_r2 == goal_row;
      auto mid = [&]() __attribute__((always_inline)) { emit(true, img_row, goal_row, t1, t2); };
      const uint8_t* s1 = a.arena + (int64_t)img_row * F;
      const uint8_t* s2 = a.arena + (int64_t)goal_row * F;
      if (keep1 && keep2) {
        mid();
      } else if constexpr (VEC == 16) {
        if (!keep1 && !keep2)
          cvt_two_frames(d1, s1, d2, s2, P, lane, mid);
        else
          cvt_one_frame(keep1 ? d2 : d1, keep1 ? s2 : s1, P, lane, mid);
      } else {
        mid();
        if (!keep1 && !keep2)
          cvt_frames_scalar(d1, s1, d2, s2, P, a.ch, lane);
        else
          cvt_frames_scalar(keep1 ? d2 : d1, keep1 ? s2 : s1, nullptr, nullptr, P, a.ch, lane);
      }
    } else if (o1 != nullptr || o2 != nullptr) {
      const int k = o1 ? 0 : 1;  // which frame: always converted, its record updated
      float* d = (k == 0 ? o1 : o2) + (int64_t)e * F;
      const uint8_t* src = a.arena + (int64_t)(k == 0 ? img_row : goal_row) * F;
      // the other frame's record no longer holds if this row was its destination (either format)
      const uint64_t oa = k == 0 ? rec_a2 : rec_a1;
      const uint64_t other = (oa & ~kOutF32) == (uint64_t)d ? 0 : oa;
      if (k == 0)
        emit(true, img_row, rec_r2, (uint64_t)d | kOutF32, other);
      else
        emit(true, rec_r1, goal_row, other, (uint64_t)d | kOutF32);
      cvt_frames_scalar(d, src, nullptr, nullptr, P, a.ch, lane);
    } else {
      emit(false, 0, 0, 0, 0);
    }
  } else if (a.obs != nullptr && a.goal_out != nullptr) {
    const int64_t F = a.frame_bytes;
    uint8_t* d1 = a.obs + (int64_t)e * F;
    uint8_t* d2 = a.goal_out + (int64_t)e * F;
    // a frame is skipped when this env's last write to the same row put the same arena row
    // there (the caller leaves the rows alone in between: vn_set_output_reuse's contract)
    const bool keep1 = a.reuse && rec_a1 == (uint64_t)d1 && rec_r1 == img_row;
    const bool keep2 = a.reuse && rec_a2 == (uint64_t)d2 && rec_r2 == goal_row;
    auto mid = [&]() __attribute__((always_inline)) { emit(true, img_row, goal_row, (uint64_t)d1, (uint64_t)d2); };
    if (!keep1 && !keep2) {
      copy_two_frames<VEC>(d1, a.arena + (int64_t)img_row * F, d2, a.arena + (int64_t)goal_row * F, F, lane, mid);
    } else if (!keep1 || !keep2) {
      uint8_t* d = keep1 ? d2 : d1;
      const int32_t row = keep1 ? goal_row : img_row;
      copy_one_frame<VEC>(d, a.arena + (int64_t)row * F, F, lane, mid);
    } else {
      mid();
    }
  } else if (a.obs != nullptr || a.goal_out != nullptr) {
    const int64_t F = a.frame_bytes;
    const int k = a.obs ? 0 : 1;  // which frame: always copied, its record updated
    uint8_t* d = (k == 0 ? a.obs : a.goal_out) + (int64_t)e * F;
    const uint8_t* src = a.arena + (int64_t)(k == 0 ? img_row : goal_row) * F;
    // the other frame's record no longer holds if this row was its destination
    const uint64_t oa = k == 0 ? rec_a2 : rec_a1;
    const uint64_t other = oa == (uint64_t)d ? 0 : oa;
    if (k == 0)
      emit(true, img_row, rec_r2, (uint64_t)d, other);
    else
      emit(true, rec_r1, goal_row, other, (uint64_t)d);
    for (int64_t i = lane; i < F; i += 64) d[i] = src[i];
  } else {
    emit(false, 0, 0, 0, 0);
  }
}

// vn_get_state / vn_get_episode_returns: dst[f][e] = word (w0 + f) of env e's record.
__global__ void rec_gather_kernel(const EnvRec* recs, int n_envs, int w0, int nw, int32_t* dst) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_envs) return;
  for (int f = 0; f < nw; ++f) dst[(int64_t)f * n_envs + e] = recs[e].w[w0 + f];
}

// vn_set_episode_returns / the schedule position: word w of every record = src[e] (or 0).
__global__ void rec_scatter_kernel(EnvRec* recs, int n_envs, int w, const int32_t* src) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_envs) return;
  recs[e].w[w] = src ? src[e] : 0;
}

// vn_set_state: the seven state words from the [7][E] table, then the cached neighbours and
// scene fields that belong to the new (scene, state). A scene or state outside the tables
// is kept as given but looked up clamped, so a bad table cannot make this kernel read past them.
__global__ void set_state_kernel(EnvRec* recs, int n_envs, const int32_t* src, const SceneDev* scenes,
                                 int n_scenes, const int32_t* graph) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_envs) return;
  EnvRec* R = recs + e;
  for (int f = 0; f < ST_COUNT; ++f) R->w[RW_ST + f] = src[(int64_t)f * n_envs + e];
  const SceneDev S = scenes[min(max(src[(int64_t)ST_SCENE * n_envs + e], 0), n_scenes - 1)];
  const int s = min(max(src[(int64_t)ST_STATE * n_envs + e], 0), S.n - 1);
  *reinterpret_cast<i32x4*>(R->w + RW_NB) = *reinterpret_cast<const i32x4*>(graph + ((int64_t)S.graph_off + s) * 4);
  store_scene_cache(R, scene_cache(S));
}

__global__ void synth_frames_kernel(uint8_t* arena, int64_t row_base, int n_rows, int64_t frame_bytes,
                                    uint32_t scene_id) {
  const int64_t words = frame_bytes >> 2;
  const int64_t total = words * n_rows;
  uint32_t* dst = reinterpret_cast<uint32_t*>(arena + row_base * frame_bytes);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = i / words, w = i - row * words;
    dst[i] = frame_hash(scene_id, (uint32_t)row, (uint32_t)w);
  }
}

// dst[i] = src[rows[i]] for rows of row_bytes (one wave per row, 16-B lanes when aligned).
__global__ __launch_bounds__(256) void gather_rows_kernel(const uint8_t* __restrict__ src, int64_t row_bytes,
                                                          const int32_t* __restrict__ rows, int n,
                                                          uint8_t* __restrict__ dst) {
  const int lane = threadIdx.x & 63;
  const int i = uni(blockIdx.x * 4 + (threadIdx.x >> 6));
  if (i >= n) return;
  const uint8_t* s = src + (int64_t)rows[i] * row_bytes;
  uint8_t* d = dst + (int64_t)i * row_bytes;
  if ((row_bytes & 15) == 0) {
    const uint4* a = reinterpret_cast<const uint4*>(s);
    uint4* b = reinterpret_cast<uint4*>(d);
    for (int64_t j = lane; j < (row_bytes >> 4); j += 64) b[j] = a[j];
  } else {
    for (int64_t j = lane; j < row_bytes; j += 64) d[j] = s[j];
  }
}

__global__ void random_actions_kernel(int32_t* actions, int n, uint32_t k0, uint32_t k1, uint64_t step) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const u32x4 r = philox4x32_10(u32x4{(uint32_t)e, (uint32_t)step, (uint32_t)(step >> 32), STREAM_ACTION}, k0, k1);
  actions[e] = (int32_t)(r.x >> 30);
}

}  // namespace vn

using namespace vn;

struct vn_ctx {
  int device = 0;
  int n_envs = 0, n_scenes = 0;
  uint64_t seed = 0;
  int64_t frame_bytes = 0, n_rows = 0;
  int px = 0, channels = 0;  // frame_bytes = px * channels
  uint8_t* arena = nullptr;
  int32_t* graph = nullptr;
  int32_t* spd = nullptr;
  SceneDev* scenes = nullptr;
  std::vector<SceneDev> scenes_host;
  EnvRec* recs = nullptr;  // [n_envs] per-env records (state, return, cached fields, output record)
  int32_t* env_scene = nullptr;
  int32_t* tasks = nullptr;
  int n_tasks = 0;
  int32_t* sched = nullptr;
  int sched_len = 0;
  std::vector<int32_t> spd_host;  // kept for building curriculum tables on demand
  int32_t* cur_order = nullptr;
  int32_t* cur_count = nullptr;
  int cur_mode = 0;
  double cur_c = 0.0;
  uint32_t* flags = nullptr;
  int max_steps = 900, autoreset = 1;
  float* info_ret = nullptr;
  int32_t* info_len = nullptr;
  int32_t* info_term = nullptr;
  uint8_t* info_trunc = nullptr;
  int32_t* info_img_row = nullptr;
  int32_t* info_goal_row = nullptr;
  // output reuse: the host switch (what each env last wrote is in its record)
  int reuse = 0;       // vn_set_output_reuse
  int reuse_arm = 0;   // the next two-frame launch still writes every row
  // vn_set_aux_arena: the caller's depth / segmentation arenas (borrowed) and the aux
  // frames' output records (owned, allocated with the first arena)
  const uint8_t* depth_arena = nullptr;
  const uint8_t* seg_arena = nullptr;
  int depth_ch = 0, seg_ch = 0;
  AuxRec* arecs = nullptr;
  // vn_nav_enable: the geodesic tables, the per-env nav record and its outputs (vn_nav.hip)
  NavState* nav = nullptr;
  // vn_nav_curriculum: the geodesic start tables, counters and levels (vn_curriculum.hip). While
  // it is set the reset path reads its tables, and scenes_spd keeps the scene table as it was
  // (cnt_off, maxd, cur_oi, cur_mode of the spd curriculum) for switching it off again
  CurState* cur = nullptr;
  std::vector<SceneDev> scenes_spd;
  // vn_nav_progress: the per-env progress record and its outputs (vn_shaping.hip)
  ShapeState* shape = nullptr;
  // vn_visit_enable: the visit table, the per-env seen-sets and their outputs (vn_visit.hip)
  VisitState* visit = nullptr;
};

namespace {

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int d) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    (void)hipSetDevice(d);
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

EnvArgs make_args(vn_ctx* c) {
  EnvArgs a;
  std::memset(&a, 0, sizeof(a));
  a.scenes = c->scenes;
  a.graph = c->graph;
  a.spd = c->spd;
  a.arena = c->arena;
  a.frame_bytes = c->frame_bytes;
  a.recs = c->recs;
  a.env_scene = c->env_scene;
  a.tasks = c->tasks;
  a.sched = c->sched;
  a.cur_order = c->cur ? c->cur->order : c->cur_order;
  a.cur_count = c->cur ? c->cur->count : c->cur_count;
  a.cur_mode = c->cur ? 1 : c->cur_mode;
  a.flags = c->flags;
  a.n_tasks = c->n_tasks;
  a.sched_len = c->sched_len;
  a.max_steps = c->max_steps;
  a.autoreset = c->autoreset;
  a.n_envs = c->n_envs;
  a.k0 = (uint32_t)c->seed;
  a.k1 = (uint32_t)(c->seed >> 32);
  a.info_ret = c->info_ret;
  a.info_len = c->info_len;
  a.info_term = c->info_term;
  a.info_trunc = c->info_trunc;
  a.info_img_row = c->info_img_row;
  a.info_goal_row = c->info_goal_row;
  a.px = c->px;
  a.ch = c->channels;
  return a;
}

// Navigation info (vn_nav_enable): a step's nav kernel reads done, truncated and ep_length of
// the step, so where the caller set none the nav state's own arrays stand in and env_kernel
// writes them as it would a caller's.
void nav_fill(vn_ctx* c, EnvArgs& a) {
  if (c->visit) {  // the visit kernel reads done and terminal_state
    if (!a.done) a.done = c->visit->s_done;
    if (!a.info_term) a.info_term = c->visit->s_term;
  }
  if (!c->nav) return;
  if (!a.done) a.done = c->nav->s_done;
  if (!a.info_trunc) a.info_trunc = c->nav->s_trunc;
  if (!a.info_len) a.info_len = c->nav->s_len;
  if (c->nav->log.capacity > 0 && !a.info_ret) a.info_ret = c->nav->s_ret;
  if (c->shape && !a.info_term) a.info_term = c->shape->s_term;  // the progress kernel reads it
}
// After the step's env_kernel launch (rc = its result), on the same stream.
int nav_side_launches(vn_ctx* c, const EnvArgs& a, int rc, hipStream_t stream) {
  if (rc != VN_OK || !c->nav) return rc;
  rc = nav_launch(c->nav, NAV_FORM_STEP, c->recs, a.done, a.info_trunc, a.info_len, a.info_ret, stream);
  if (rc == VN_OK && c->shape)
    rc = shape_launch(c->shape, c->nav, SHAPE_FORM_STEP, c->recs, nullptr, a.done, a.info_trunc, a.info_term, stream);
  if (rc != VN_OK || !c->cur || c->cur->cfg.window <= 0) return rc;
  return cur_count_launch(c->cur, c->recs, a.done, a.info_trunc, 1, stream);
}
// The visit launch goes behind the step's other side launches and shares no data with them.
int nav_after_step(vn_ctx* c, const EnvArgs& a, int rc, hipStream_t stream) {
  rc = nav_side_launches(c, a, rc, stream);
  if (rc != VN_OK || !c->visit) return rc;
  return visit_launch(c->visit, VISIT_FORM_STEP, c->recs, nullptr, a.done, a.info_term, c->autoreset, 1, stream);
}
// The episodes of the envs a launch outside a step has started (vn_reset: the masked ones, each
// counted at its start; vn_set_state: all, uncounted, since a restore follows).
int visit_refresh(vn_ctx* c, int rc, const int32_t* mask, int add, hipStream_t stream) {
  if (rc != VN_OK || !c->visit) return rc;
  return visit_launch(c->visit, VISIT_FORM_REFRESH, c->recs, mask, nullptr, nullptr, 0, add, stream);
}
// The progress record of the envs a launch outside a step may have moved (vn_reset: the masked
// ones; vn_set_state: all), from their records.
int shape_refresh(vn_ctx* c, int rc, const int32_t* mask, hipStream_t stream) {
  if (rc != VN_OK || !c->shape) return rc;
  return shape_launch(c->shape, c->nav, SHAPE_FORM_REFRESH, c->recs, mask, nullptr, nullptr, nullptr, stream);
}
// After a launch that may have moved envs to another scene outside a step (vn_reset,
// vn_set_state): the adaptive curriculum notes every env's scene again and counts nothing.
int cur_refresh(vn_ctx* c, int rc, hipStream_t stream) {
  if (rc != VN_OK || !c->cur || c->cur->cfg.window <= 0) return rc;
  return cur_count_launch(c->cur, c->recs, nullptr, nullptr, 0, stream);
}

// Whether a launch writing to (obs, goal) may skip rows that already hold their frame. The
// first executed two-frame launch after vn_set_output_reuse(ctx, 1) consumes the armed full
// write. A launch that is only being captured into a graph has not run yet (and may never):
// while armed it is recorded as a full write and leaves the arm for the next eager launch.
// A one-frame launch copies unconditionally and leaves the arm for the next two-frame one.
int take_reuse(vn_ctx* c, const void* obs, const void* goal, hipStream_t stream) {
  if (!obs || !goal || !c->reuse) return 0;
  if (!c->reuse_arm) return 1;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(stream, &cap) != hipSuccess) {
    (void)hipGetLastError();  // e.g. the legacy stream while another one captures: not a capture of ours
    cap = hipStreamCaptureStatusNone;
  }
  if (cap == hipStreamCaptureStatusNone) c->reuse_arm = 0;
  return 0;
}

template <int MODE>
int launch_env(vn_ctx* c, const EnvArgs& a, hipStream_t stream) {
  const dim3 grid((c->n_envs + kEnvsPerBlock - 1) / kEnvsPerBlock), block(64 * kEnvsPerBlock);
  const int64_t F = c->frame_bytes;
  const bool al16 = (F % 16 == 0) && ((uintptr_t)a.obs % 16 == 0) && ((uintptr_t)a.goal_out % 16 == 0);
  const bool al4 = (F % 4 == 0) && ((uintptr_t)a.obs % 4 == 0) && ((uintptr_t)a.goal_out % 4 == 0);
  if (al16)
    hipLaunchKernelGGL((env_kernel<MODE, 16>), grid, block, 0, stream, a);
  else if (al4)
    hipLaunchKernelGGL((env_kernel<MODE, 4>), grid, block, 0, stream, a);
  else
    hipLaunchKernelGGL((env_kernel<MODE, 1>), grid, block, 0, stream, a);
  VN_HIP(hipGetLastError());
  return VN_OK;
}

// The float tail: 4-pixel lanes when the frame is 3 channels of a multiple of 4 pixels and
// both rows' planes are 16-B aligned (every plane then is: F and P floats are multiples of 16 B).
template <int MODE>
int launch_env_f32(vn_ctx* c, const EnvArgs& a, hipStream_t stream) {
  const dim3 grid((c->n_envs + kEnvsPerBlock - 1) / kEnvsPerBlock), block(64 * kEnvsPerBlock);
  const bool vec = c->channels == 3 && c->px % 4 == 0 && (uintptr_t)a.obs % 16 == 0 && (uintptr_t)a.goal_out % 16 == 0;
  if (vec)
    hipLaunchKernelGGL((env_kernel<MODE, 16, FMT_F32>), grid, block, 0, stream, a);
  else
    hipLaunchKernelGGL((env_kernel<MODE, 4, FMT_F32>), grid, block, 0, stream, a);
  VN_HIP(hipGetLastError());
  return VN_OK;
}

// vn_step_aux / vn_observe_aux: `base` holds everything but the frames. Checks the output set,
// then launches the five-frame instantiation whose lane width every written row allows: for
// u8 the widest of 16 / 4 / 1 bytes that divides all three row sizes and both ends of every
// row; for f32 the 4-pixel lanes when the frames are 3 + 3 + 1 channels of a multiple of 4
// pixels with 16-B aligned planes, else the scalar form. Nothing is launched on an error.
template <int MODE>
int launch_env_aux(vn_ctx* c, const EnvArgs& base, const vn_obs_set* o, const char* who, hipStream_t stream) {
  const std::string w(who);
  if (!o) return fail(VN_EINVAL, w + ": obs is NULL");
  if (!c->depth_arena || !c->seg_arena || !c->arecs) return fail(VN_EINVAL, w + ": no aux arena (vn_set_aux_arena)");
  if (o->format != VN_OBS_U8_HWC && o->format != VN_OBS_F32_CHW) return fail(VN_EINVAL, w + ": unknown format");
  if (!o->image || !o->goal) return fail(VN_EINVAL, w + ": image and goal must not be NULL");
  const bool f32 = o->format == VN_OBS_F32_CHW;
  const int64_t P = c->px, es = f32 ? 4 : 1;
  const int64_t elems[5] = {c->frame_bytes, c->frame_bytes, P * c->depth_ch, P * c->seg_ch, P * c->seg_ch};
  const uintptr_t outs[5] = {(uintptr_t)o->image, (uintptr_t)o->goal, (uintptr_t)o->depth, (uintptr_t)o->segmentation,
                             (uintptr_t)o->goal_segmentation};
  uintptr_t all = 0;
  for (int k = 0; k < 5; ++k) all |= outs[k];
  if (f32 && (all & 3)) return fail(VN_EINVAL, w + ": float outputs must be 4-byte aligned");
  for (int i = 0; i < 5; ++i) {
    for (int j = i + 1; j < 5; ++j) {
      if (!outs[i] || !outs[j]) continue;
      const uintptr_t ei = outs[i] + (uintptr_t)(c->n_envs * elems[i] * es);
      const uintptr_t ej = outs[j] + (uintptr_t)(c->n_envs * elems[j] * es);
      if (outs[i] < ej && outs[j] < ei) return fail(VN_EINVAL, w + ": two outputs overlap");
    }
  }
  EnvAuxArgs a;
  std::memset(&a, 0, sizeof(a));
  static_cast<EnvArgs&>(a) = base;
  a.obs = reinterpret_cast<uint8_t*>(o->image);
  a.goal_out = reinterpret_cast<uint8_t*>(o->goal);
  a.out_depth = reinterpret_cast<uint8_t*>(o->depth);
  a.out_seg = reinterpret_cast<uint8_t*>(o->segmentation);
  a.out_gseg = reinterpret_cast<uint8_t*>(o->goal_segmentation);
  a.depth_arena = c->depth_arena;
  a.seg_arena = c->seg_arena;
  a.arecs = c->arecs;
  a.dch = c->depth_ch;
  a.sch = c->seg_ch;
  a.reuse = take_reuse(c, o->image, o->goal, stream);
  const dim3 grid((c->n_envs + kEnvsPerBlock - 1) / kEnvsPerBlock), block(64 * kEnvsPerBlock);
  const uintptr_t ends = all | (uintptr_t)c->depth_arena | (uintptr_t)c->seg_arena;
  if (f32) {
    const bool vec = c->channels == 3 && c->seg_ch == 3 && c->depth_ch == 1 && P % 4 == 0 && all % 16 == 0 &&
                     ((uintptr_t)c->depth_arena | (uintptr_t)c->seg_arena) % 4 == 0;
    if (vec)
      hipLaunchKernelGGL((env_kernel<MODE, 16, FMT_F32, 1>), grid, block, 0, stream, a);
    else
      hipLaunchKernelGGL((env_kernel<MODE, 4, FMT_F32, 1>), grid, block, 0, stream, a);
  } else {
    const int64_t sizes = elems[0] | elems[2] | elems[3];
    if (sizes % 16 == 0 && ends % 16 == 0)
      hipLaunchKernelGGL((env_kernel<MODE, 16, FMT_U8, 1>), grid, block, 0, stream, a);
    else if (sizes % 4 == 0 && ends % 4 == 0)
      hipLaunchKernelGGL((env_kernel<MODE, 4, FMT_U8, 1>), grid, block, 0, stream, a);
    else
      hipLaunchKernelGGL((env_kernel<MODE, 1, FMT_U8, 1>), grid, block, 0, stream, a);
  }
  VN_HIP(hipGetLastError());
  return VN_OK;
}

void free_ctx(vn_ctx* c) {
  if (!c) return;
  void* ptrs[] = {c->arena, c->graph, c->spd, c->scenes, c->recs, c->env_scene,
                  c->tasks, c->sched, c->flags, c->cur_order, c->cur_count, c->arecs};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  nav_destroy(c->nav);
  cur_destroy(c->cur);
  shape_destroy(c->shape);
  visit_destroy(c->visit);
  delete c;
}

}  // namespace

extern "C" {

const char* vn_version(void) { return "vnav 0.1.0 gfx950"; }

int vn_last_error(char* buf, size_t len) {
  if (!buf || len == 0) return VN_EINVAL;
  const std::string& m = vn::last_error();
  const size_t n = std::min(len - 1, m.size());
  std::memcpy(buf, m.data(), n);
  buf[n] = 0;
  return VN_OK;
}

int vn_create(const vn_scene_desc* scenes, int n_scenes, int n_envs, uint64_t seed, int device,
              vn_ctx** out) {
  if (!out) return fail(VN_EINVAL, "vn_create: out is NULL");
  *out = nullptr;
  if (!scenes || n_scenes <= 0) return fail(VN_EINVAL, "vn_create: need at least one scene");
  if (n_envs <= 0) return fail(VN_EINVAL, "vn_create: n_envs must be > 0");
  const int H = scenes[0].height, W = scenes[0].width, C = scenes[0].channels;
  if (H <= 0 || W <= 0 || C <= 0) return fail(VN_EINVAL, "vn_create: bad frame shape");
  const int64_t F = (int64_t)H * W * C;
  if (F >= (1ll << 31)) return fail(VN_EINVAL, "vn_create: frames of 2^31 bytes or more");
  int64_t rows = 0, graph_rows = 0, spd_elems = 0;
  std::vector<SceneDev> sh(n_scenes);
  for (int k = 0; k < n_scenes; ++k) {
    const vn_scene_desc& d = scenes[k];
    if (d.height != H || d.width != W || d.channels != C)
      return fail(VN_EINVAL, "vn_create: all scenes must share one frame shape");
    if (d.n_states <= 0 || !d.graph || !d.spd) return fail(VN_EINVAL, "vn_create: scene missing graph/spd");
    if (!d.observations && (F % 4) != 0)
      return fail(VN_EINVAL, "vn_create: synthetic frames need frame bytes % 4 == 0");
    sh[k].row_base = rows;
    sh[k].graph_off = (int32_t)graph_rows;
    sh[k].spd_off = spd_elems;
    sh[k].n = d.n_states;
    sh[k].r_goal = d.reward_goal;
    sh[k].r_step = d.reward_step;
    sh[k].r_coll = d.reward_collision;
    sh[k].terminal_obs = d.terminal_obs;
    rows += d.n_states;
    sh[k].comp_base = -1;
    if (d.companion) {
      sh[k].comp_base = rows;
      rows += d.n_states;
    }
    graph_rows += d.n_states;
    spd_elems += (int64_t)d.n_states * d.n_states;
  }
  if (rows >= (1ll << 31)) return fail(VN_EINVAL, "vn_create: more than 2^31 frames");
  // Host-side conversion int64 -> int32 with range checks (the h5 datasets are int64).
  std::vector<int32_t> g32(graph_rows * 4);
  std::vector<int32_t> spd32(spd_elems);
  for (int k = 0; k < n_scenes; ++k) {
    const vn_scene_desc& d = scenes[k];
    const int64_t n = d.n_states;
    for (int64_t i = 0; i < n * 4; ++i) {
      const int64_t v = d.graph[i];
      if (v < -1 || v >= n) return fail(VN_EINVAL, "vn_create: graph entry out of range");
      g32[(int64_t)sh[k].graph_off * 4 + i] = (int32_t)v;
    }
    int32_t mx = 0;
    for (int64_t i = 0; i < n * n; ++i) {
      const int64_t v = d.spd[i];
      spd32[sh[k].spd_off + i] = (int32_t)std::max<int64_t>(std::min<int64_t>(v, INT32_MAX), INT32_MIN);
      mx = std::max(mx, spd32[sh[k].spd_off + i]);
    }
    if (mx > (1 << 20)) return fail(VN_EINVAL, "vn_create: spd values above 2^20");
    sh[k].maxd = mx;
  }
  int64_t cnt_elems = 0;
  for (int k = 0; k < n_scenes; ++k) {
    sh[k].cnt_off = cnt_elems;
    cnt_elems += (int64_t)sh[k].n * (sh[k].maxd + 2);
  }
  DeviceGuard guard(device);
  vn_ctx* c = new (std::nothrow) vn_ctx();
  if (!c) return fail(VN_ENOMEM, "vn_create: host allocation failed");
  c->device = device;
  c->n_envs = n_envs;
  c->n_scenes = n_scenes;
  c->seed = seed;
  c->frame_bytes = F;
  c->px = H * W;
  c->channels = C;
  c->n_rows = rows;
  c->scenes_host = sh;
  c->spd_host = spd32;
  auto alloc = [&](void** p, size_t bytes) -> bool {
    return hipMalloc(p, std::max<size_t>(bytes, 16)) == hipSuccess;
  };
  bool ok = alloc((void**)&c->arena, (size_t)(rows * F)) && alloc((void**)&c->graph, g32.size() * 4) &&
            alloc((void**)&c->spd, spd32.size() * 4) && alloc((void**)&c->scenes, sh.size() * sizeof(SceneDev)) &&
            alloc((void**)&c->recs, (size_t)n_envs * sizeof(EnvRec)) &&
            alloc((void**)&c->env_scene, (size_t)n_envs * 4) && alloc((void**)&c->flags, 4);
  if (!ok) {
    free_ctx(c);
    return fail(VN_ENOMEM, "vn_create: device allocation failed");
  }
  hipError_t e = hipSuccess;
  std::vector<int32_t> es(n_envs);
  for (int i = 0; i < n_envs; ++i) es[i] = i % n_scenes;
  if (e == hipSuccess) e = hipMemcpy(c->graph, g32.data(), g32.size() * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(c->spd, spd32.data(), spd32.size() * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(c->scenes, sh.data(), sh.size() * sizeof(SceneDev), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(c->env_scene, es.data(), es.size() * 4, hipMemcpyHostToDevice);
  // zero records: reset count and schedule position 0, and a null output address, which
  // matches no destination (the first launch writes every row)
  if (e == hipSuccess) e = hipMemset(c->recs, 0, (size_t)n_envs * sizeof(EnvRec));
  if (e == hipSuccess) e = hipMemset(c->flags, 0, 4);
  for (int k = 0; k < n_scenes && e == hipSuccess; ++k) {
    const vn_scene_desc& d = scenes[k];
    if (d.companion)
      e = hipMemcpy(c->arena + sh[k].comp_base * F, d.companion, (size_t)d.n_states * F, hipMemcpyHostToDevice);
    if (e != hipSuccess) break;
    if (d.observations) {
      e = hipMemcpy(c->arena + sh[k].row_base * F, d.observations, (size_t)d.n_states * F, hipMemcpyHostToDevice);
    } else {
      hipLaunchKernelGGL(synth_frames_kernel, dim3(2048), dim3(256), 0, 0, c->arena, sh[k].row_base, d.n_states, F,
                         d.synth_id);
      e = hipGetLastError();
    }
  }
  if (e != hipSuccess) {
    free_ctx(c);
    return hip_fail(e, "vn_create: upload");
  }
  // The constructor's reset (cached.py:36): every env starts from a sampled (start, goal).
  EnvArgs a = make_args(c);
  int rc = launch_env<MODE_RESET>(c, a, 0);
  if (rc == VN_OK) {
    e = hipDeviceSynchronize();
    if (e != hipSuccess) rc = hip_fail(e, "vn_create: initial reset");
  }
  if (rc != VN_OK) {
    free_ctx(c);
    return rc;
  }
  *out = c;
  return VN_OK;
}

int vn_destroy(vn_ctx* c) {
  if (!c) return VN_OK;
  DeviceGuard guard(c->device);
  (void)hipDeviceSynchronize();
  free_ctx(c);
  return VN_OK;
}

int vn_num_envs(vn_ctx* c) { return c ? c->n_envs : VN_EINVAL; }

int vn_reset(vn_ctx* c, const int32_t* env_mask_dev, vn_stream_t stream) {
  if (!c) return fail(VN_EINVAL, "vn_reset: NULL ctx");
  DeviceGuard guard(c->device);
  EnvArgs a = make_args(c);
  a.mask = env_mask_dev;
  int rc = launch_env<MODE_RESET>(c, a, (hipStream_t)stream);
  if (rc == VN_OK && c->nav)
    rc = cur_refresh(c, shape_refresh(c, nav_launch(c->nav, NAV_FORM_RESET, c->recs, nullptr, nullptr, nullptr,
                                                    nullptr, (hipStream_t)stream),
                                      env_mask_dev, (hipStream_t)stream), (hipStream_t)stream);
  return visit_refresh(c, rc, env_mask_dev, 1, (hipStream_t)stream);
}

int vn_observe(vn_ctx* c, uint8_t* obs_dev, uint8_t* goal_dev, int32_t* state_dev, vn_stream_t stream) {
  if (!c) return fail(VN_EINVAL, "vn_observe: NULL ctx");
  DeviceGuard guard(c->device);
  EnvArgs a = make_args(c);
  a.obs = obs_dev;
  a.goal_out = goal_dev;
  a.state_out = state_dev;
  a.reuse = take_reuse(c, obs_dev, goal_dev, (hipStream_t)stream);
  return launch_env<MODE_OBSERVE>(c, a, (hipStream_t)stream);
}

int vn_step(vn_ctx* c, const int32_t* actions_dev, uint8_t* obs_dev, uint8_t* goal_dev, float* reward_dev,
            uint8_t* done_dev, int32_t* state_dev, vn_stream_t stream) {
  if (!c) return fail(VN_EINVAL, "vn_step: NULL ctx");
  if (!actions_dev) return fail(VN_EINVAL, "vn_step: actions is NULL");
  DeviceGuard guard(c->device);
  EnvArgs a = make_args(c);
  a.actions = actions_dev;
  a.obs = obs_dev;
  a.goal_out = goal_dev;
  a.reward = reward_dev;
  a.done = done_dev;
  a.state_out = state_dev;
  a.reuse = take_reuse(c, obs_dev, goal_dev, (hipStream_t)stream);
  nav_fill(c, a);
  return nav_after_step(c, a, launch_env<MODE_STEP>(c, a, (hipStream_t)stream), (hipStream_t)stream);
}

int vn_observe_f32(vn_ctx* c, float* obs_chw_dev, float* goal_chw_dev, int32_t* state_dev, vn_stream_t stream) {
  if (!c) return fail(VN_EINVAL, "vn_observe_f32: NULL ctx");
  if (((uintptr_t)obs_chw_dev | (uintptr_t)goal_chw_dev) & 3)
    return fail(VN_EINVAL, "vn_observe_f32: float outputs must be 4-byte aligned");
  DeviceGuard guard(c->device);
  EnvArgs a = make_args(c);
  a.obs = reinterpret_cast<uint8_t*>(obs_chw_dev);
  a.goal_out = reinterpret_cast<uint8_t*>(goal_chw_dev);
  a.state_out = state_dev;
  a.reuse = take_reuse(c, obs_chw_dev, goal_chw_dev, (hipStream_t)stream);
  return launch_env_f32<MODE_OBSERVE>(c, a, (hipStream_t)stream);
}

int vn_step_f32(vn_ctx* c, const int32_t* actions_dev, float* obs_chw_dev, float* goal_chw_dev, float* reward_dev,
                uint8_t* done_dev, int32_t* state_dev, vn_stream_t stream) {
  if (!c) return fail(VN_EINVAL, "vn_step_f32: NULL ctx");
  if (!actions_dev) return fail(VN_EINVAL, "vn_step_f32: actions is NULL");
  if (((uintptr_t)obs_chw_dev | (uintptr_t)goal_chw_dev) & 3)
    return fail(VN_EINVAL, "vn_step_f32: float outputs must be 4-byte aligned");
  DeviceGuard guard(c->device);
  EnvArgs a = make_args(c);
  a.actions = actions_dev;
  a.obs = reinterpret_cast<uint8_t*>(obs_chw_dev);
  a.goal_out = reinterpret_cast<uint8_t*>(goal_chw_dev);
  a.reward = reward_dev;
  a.done = done_dev;
  a.state_out = state_dev;
  a.reuse = take_reuse(c, obs_chw_dev, goal_chw_dev, (hipStream_t)stream);
  nav_fill(c, a);
  return nav_after_step(c, a, launch_env_f32<MODE_STEP>(c, a, (hipStream_t)stream), (hipStream_t)stream);
}

int vn_set_aux_arena(vn_ctx* c, const uint8_t* depth_dev, int depth_channels, const uint8_t* seg_dev,
                     int seg_channels) {
  if (!c) return fail(VN_EINVAL, "vn_set_aux_arena: NULL ctx");
  if (!depth_dev && !seg_dev) {  // clear: the records stay allocated, nothing reads them
    c->depth_arena = c->seg_arena = nullptr;
    c->depth_ch = c->seg_ch = 0;
    return VN_OK;
  }
  if (!depth_dev || !seg_dev) return fail(VN_EINVAL, "vn_set_aux_arena: need both arenas (or both NULL)");
  if (depth_channels <= 0 || seg_channels <= 0) return fail(VN_EINVAL, "vn_set_aux_arena: bad channel count");
  if ((int64_t)c->px * std::max(depth_channels, seg_channels) >= (1ll << 31))
    return fail(VN_EINVAL, "vn_set_aux_arena: rows of 2^31 bytes or more");
  DeviceGuard guard(c->device);
  const size_t bytes = (size_t)c->n_envs * sizeof(AuxRec);
  if (!c->arecs && hipMalloc((void**)&c->arecs, bytes) != hipSuccess) {
    c->arecs = nullptr;
    return fail(VN_ENOMEM, "vn_set_aux_arena: device allocation failed");
  }
  // null addresses match no destination: new arenas are other bytes, so every aux row is
  // written once more (after any launch still using the old records)
  VN_HIP(hipDeviceSynchronize());
  VN_HIP(hipMemset(c->arecs, 0, bytes));
  c->depth_arena = depth_dev;
  c->seg_arena = seg_dev;
  c->depth_ch = depth_channels;
  c->seg_ch = seg_channels;
  return VN_OK;
}

int vn_observe_aux(vn_ctx* c, const vn_obs_set* obs, int32_t* state_dev, vn_stream_t stream) {
  if (!c) return fail(VN_EINVAL, "vn_observe_aux: NULL ctx");
  DeviceGuard guard(c->device);
  EnvArgs a = make_args(c);
  a.state_out = state_dev;
  return launch_env_aux<MODE_OBSERVE>(c, a, obs, "vn_observe_aux", (hipStream_t)stream);
}

int vn_step_aux(vn_ctx* c, const int32_t* actions_dev, const vn_obs_set* obs, float* reward_dev, uint8_t* done_dev,
                int32_t* state_dev, vn_stream_t stream) {
  if (!c) return fail(VN_EINVAL, "vn_step_aux: NULL ctx");
  if (!actions_dev) return fail(VN_EINVAL, "vn_step_aux: actions is NULL");
  DeviceGuard guard(c->device);
  EnvArgs a = make_args(c);
  a.actions = actions_dev;
  a.reward = reward_dev;
  a.done = done_dev;
  a.state_out = state_dev;
  nav_fill(c, a);
  return nav_after_step(c, a, launch_env_aux<MODE_STEP>(c, a, obs, "vn_step_aux", (hipStream_t)stream),
                        (hipStream_t)stream);
}

int vn_step_a2c(vn_ctx* c, const vn_a2c_step* p, float* reward_dev, uint8_t* done_dev, int32_t* state_dev,
                vn_stream_t stream) {
  if (!c) return fail(VN_EINVAL, "vn_step_a2c: NULL ctx");
  if (!p || !p->policy_out || !p->actions || p->num_actions < 1 || p->num_actions > 7)
    return fail(VN_EINVAL, "vn_step_a2c: bad a2c arguments");
  DeviceGuard guard(c->device);
  EnvArgs a = make_args(c);
  a.reward = reward_dev;
  a.done = done_dev;
  a.state_out = state_dev;
  a.pol_out = p->policy_out;
  a.pol_A = p->num_actions;
  a.pk0 = (uint32_t)p->seed;
  a.pk1 = (uint32_t)(p->seed >> 32);
  a.pctr_dev = p->counter_base_dev;
  a.pctr = p->counter;
  a.act_out = p->actions;
  a.prev_action = p->prev_action;
  a.prev_reward = p->prev_reward;
  a.prev_mask = p->prev_mask;
  a.lra_next = p->lra_next;
  a.mask_next = p->mask_next;
  a.stats_env = p->episode_stats_env;
  nav_fill(c, a);
  if (p->head_weight) {
    if (!p->head_bias || !p->head_input || !p->head_out || p->head_out != p->policy_out)
      return fail(VN_EINVAL, "vn_step_a2c: head_weight needs head_bias, head_input and head_out == policy_out");
    if ((reinterpret_cast<uintptr_t>(p->head_weight) | reinterpret_cast<uintptr_t>(p->head_input)) & 15)
      return fail(VN_EINVAL, "vn_step_a2c: head_weight / head_input must be 16-byte aligned");
    a.head_w = p->head_weight;
    a.head_b = p->head_bias;
    a.head_x = p->head_input;
    a.head_out = p->head_out;
    return nav_after_step(c, a, launch_env<MODE_STEP_HEADS>(c, a, (hipStream_t)stream), (hipStream_t)stream);
  }
  return nav_after_step(c, a, launch_env<MODE_STEP>(c, a, (hipStream_t)stream), (hipStream_t)stream);
}

int vn_nav_enable(vn_ctx* c, int on) {
  if (!c) return fail(VN_EINVAL, "vn_nav_enable: NULL ctx");
  std::vector<NavScene> ns(c->n_scenes);
  for (int k = 0; k < c->n_scenes && on; ++k) {
    const SceneDev& S = c->scenes_host[k];
    if (S.n > kNavMaxStates)
      return fail(VN_EINVAL, "vn_nav_enable: scene " + std::to_string(k) + " has " + std::to_string(S.n) +
                                 " states, more than " + std::to_string(kNavMaxStates));
    ns[k] = NavScene{0, S.n, S.graph_off};
  }
  DeviceGuard guard(c->device);
  VN_HIP(hipDeviceSynchronize());
  if (c->cur) {  // its tables are built from the nav tables that go away here
    const int rc = vn_nav_curriculum(c, nullptr);
    if (rc != VN_OK) return rc;
  }
  shape_destroy(c->shape);  // its lookups read the nav tables that go away here
  c->shape = nullptr;
  nav_destroy(c->nav);
  c->nav = nullptr;
  if (!on) return VN_OK;
  NavState* nav = nullptr;
  int rc = nav_create(&nav, c->n_envs, ns, c->graph);
  if (rc != VN_OK) return rc;
  // every env's record from its current state: a running episode is measured from here
  rc = nav_launch(nav, NAV_FORM_ENABLE, c->recs, nullptr, nullptr, nullptr, nullptr, 0);
  if (rc == VN_OK) {
    const hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) rc = hip_fail(e, "vn_nav_enable: build");
  }
  if (rc != VN_OK) {
    nav_destroy(nav);
    return rc;
  }
  c->nav = nav;
  return VN_OK;
}

int vn_set_nav_buffers(vn_ctx* c, int32_t* geo_dist, int32_t* optimal_action, uint8_t* optimal_mask,
                       uint8_t* ep_success, float* ep_spl, int32_t* ep_start_dist) {
  if (!c) return fail(VN_EINVAL, "vn_set_nav_buffers: NULL ctx");
  if (!c->nav) return fail(VN_ESTATE, "vn_set_nav_buffers: navigation info is not enabled (vn_nav_enable)");
  DeviceGuard guard(c->device);
  VN_HIP(hipDeviceSynchronize());
  c->nav->geo_dist = geo_dist;
  c->nav->opt_action = optimal_action;
  c->nav->opt_mask = optimal_mask;
  c->nav->opt_mask_out = nullptr;
  c->nav->ep_success = ep_success;
  c->nav->ep_spl = ep_spl;
  c->nav->ep_start = ep_start_dist;
  // the new buffers hold the current distance, mask and action at once
  const int rc = nav_launch(c->nav, NAV_FORM_OUTPUTS, c->recs, nullptr, nullptr, nullptr, nullptr, 0);
  if (rc != VN_OK) return rc;
  VN_HIP(hipDeviceSynchronize());
  return VN_OK;
}

int vn_set_nav_mask_output(vn_ctx* c, uint8_t* optimal_mask) {
  if (!c) return fail(VN_EINVAL, "vn_set_nav_mask_output: NULL ctx");
  if (!c->nav) return fail(VN_ESTATE, "vn_set_nav_mask_output: navigation info is not enabled (vn_nav_enable)");
  c->nav->opt_mask_out = optimal_mask;
  return VN_OK;
}

int vn_nav_table(vn_ctx* c, int scene, const int16_t** geo_dev, int32_t* n) {
  if (!c || scene < 0 || scene >= c->n_scenes) return fail(VN_EINVAL, "vn_nav_table: bad args");
  if (!c->nav) return fail(VN_ESTATE, "vn_nav_table: navigation info is not enabled (vn_nav_enable)");
  if (geo_dev) *geo_dev = c->nav->geo + c->nav->scenes_host[scene].geo_off;
  if (n) *n = c->nav->scenes_host[scene].n;
  return VN_OK;
}

int vn_get_nav_state(vn_ctx* c, int32_t* dst, vn_stream_t stream) {
  if (!c || !dst) return fail(VN_EINVAL, "vn_get_nav_state: NULL argument");
  if (!c->nav) return fail(VN_ESTATE, "vn_get_nav_state: navigation info is not enabled (vn_nav_enable)");
  DeviceGuard guard(c->device);
  VN_HIP(hipMemcpyAsync(dst, c->nav->rec, (size_t)c->n_envs * 8, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return VN_OK;
}

int vn_set_nav_state(vn_ctx* c, const int32_t* src, vn_stream_t stream) {
  if (!c || !src) return fail(VN_EINVAL, "vn_set_nav_state: NULL argument");
  if (!c->nav) return fail(VN_ESTATE, "vn_set_nav_state: navigation info is not enabled (vn_nav_enable)");
  DeviceGuard guard(c->device);
  VN_HIP(hipMemcpyAsync(c->nav->rec, src, (size_t)c->n_envs * 8, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return VN_OK;
}

int vn_nav_progress(vn_ctx* c, int on) {
  if (!c) return fail(VN_EINVAL, "vn_nav_progress: NULL ctx");
  if (!c->nav) return fail(VN_ESTATE, "vn_nav_progress: navigation info is not enabled (vn_nav_enable)");
  DeviceGuard guard(c->device);
  VN_HIP(hipDeviceSynchronize());
  shape_destroy(c->shape);
  c->shape = nullptr;
  if (!on) return VN_OK;
  ShapeState* sh = nullptr;
  int rc = shape_create(&sh, c->n_envs);
  if (rc != VN_OK) return rc;
  // every env's record from its current state: a running episode is measured from here
  rc = shape_launch(sh, c->nav, SHAPE_FORM_REFRESH, c->recs, nullptr, nullptr, nullptr, nullptr, 0);
  if (rc == VN_OK) {
    const hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) rc = hip_fail(e, "vn_nav_progress: enable");
  }
  if (rc != VN_OK) {
    shape_destroy(sh);
    return rc;
  }
  c->shape = sh;
  return VN_OK;
}

int vn_set_nav_progress_outputs(vn_ctx* c, int32_t* dist_before, int32_t* dist_after, int32_t* progress) {
  if (!c) return fail(VN_EINVAL, "vn_set_nav_progress_outputs: NULL ctx");
  if (!c->shape) return fail(VN_ESTATE, "vn_set_nav_progress_outputs: progress is not enabled (vn_nav_progress)");
  c->shape->dist_before = dist_before;
  c->shape->dist_after = dist_after;
  c->shape->progress = progress;
  return VN_OK;
}

int vn_get_nav_progress_state(vn_ctx* c, int32_t* dst, vn_stream_t stream) {
  if (!c || !dst) return fail(VN_EINVAL, "vn_get_nav_progress_state: NULL argument");
  if (!c->shape) return fail(VN_ESTATE, "vn_get_nav_progress_state: progress is not enabled (vn_nav_progress)");
  DeviceGuard guard(c->device);
  VN_HIP(hipMemcpyAsync(dst, c->shape->rec, (size_t)c->n_envs * 12, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return VN_OK;
}

int vn_set_nav_progress_state(vn_ctx* c, const int32_t* src, vn_stream_t stream) {
  if (!c || !src) return fail(VN_EINVAL, "vn_set_nav_progress_state: NULL argument");
  if (!c->shape) return fail(VN_ESTATE, "vn_set_nav_progress_state: progress is not enabled (vn_nav_progress)");
  DeviceGuard guard(c->device);
  VN_HIP(hipMemcpyAsync(c->shape->rec, src, (size_t)c->n_envs * 12, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return VN_OK;
}

int vn_visit_enable(vn_ctx* c, int on) {
  if (!c) return fail(VN_EINVAL, "vn_visit_enable: NULL ctx");
  DeviceGuard guard(c->device);
  VisitState* vs = nullptr;
  if (on) {  // built first: a refusal leaves the context as it was
    std::vector<int32_t> ns(c->n_scenes);
    for (int k = 0; k < c->n_scenes; ++k) ns[k] = c->scenes_host[k].n;
    int rc = visit_create(&vs, c->n_envs, ns);
    if (rc != VN_OK) return rc;
    // every env's episode from its current state: a running episode is covered from here
    rc = visit_launch(vs, VISIT_FORM_REFRESH, c->recs, nullptr, nullptr, nullptr, 0, 1, 0);
    if (rc != VN_OK) {
      visit_destroy(vs);
      return rc;
    }
  }
  const hipError_t e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    visit_destroy(vs);
    return hip_fail(e, "vn_visit_enable");
  }
  visit_destroy(c->visit);
  c->visit = vs;
  return VN_OK;
}

int vn_set_visit_outputs(vn_ctx* c, int32_t* cell, uint8_t* first, int32_t* ep_distinct) {
  if (!c) return fail(VN_EINVAL, "vn_set_visit_outputs: NULL ctx");
  if (!c->visit) return fail(VN_ESTATE, "vn_set_visit_outputs: visit counts are not enabled (vn_visit_enable)");
  c->visit->cell_out = cell;
  c->visit->first_out = first;
  c->visit->ep_distinct_out = ep_distinct;
  return VN_OK;
}

int vn_visit_table(vn_ctx* c, int scene, const uint32_t** count_dev, int32_t* n) {
  if (!c || scene < 0 || scene >= c->n_scenes) return fail(VN_EINVAL, "vn_visit_table: bad args");
  if (!c->visit) return fail(VN_ESTATE, "vn_visit_table: visit counts are not enabled (vn_visit_enable)");
  if (count_dev) *count_dev = c->visit->count + c->visit->cell_off_host[scene];
  if (n) *n = (int32_t)(c->visit->cell_off_host[scene + 1] - c->visit->cell_off_host[scene]);
  return VN_OK;
}

int vn_visit_cells(vn_ctx* c, const uint32_t** count_dev, const int64_t** cell_off_dev, int64_t* cells) {
  if (!c) return fail(VN_EINVAL, "vn_visit_cells: NULL ctx");
  if (!c->visit) return fail(VN_ESTATE, "vn_visit_cells: visit counts are not enabled (vn_visit_enable)");
  if (count_dev) *count_dev = c->visit->count;
  if (cell_off_dev) *cell_off_dev = c->visit->cell_off;
  if (cells) *cells = c->visit->C;
  return VN_OK;
}

int vn_visit_get_state(vn_ctx* c, int32_t* dst, vn_stream_t stream) {
  if (!c || !dst) return fail(VN_EINVAL, "vn_visit_get_state: NULL argument");
  if (!c->visit) return fail(VN_ESTATE, "vn_visit_get_state: visit counts are not enabled (vn_visit_enable)");
  DeviceGuard guard(c->device);
  VN_HIP(hipMemcpyAsync(dst, c->visit->count, (size_t)c->visit->state_words() * 4, hipMemcpyDeviceToDevice,
                        (hipStream_t)stream));
  return VN_OK;
}

int vn_visit_set_state(vn_ctx* c, const int32_t* src, vn_stream_t stream) {
  if (!c || !src) return fail(VN_EINVAL, "vn_visit_set_state: NULL argument");
  if (!c->visit) return fail(VN_ESTATE, "vn_visit_set_state: visit counts are not enabled (vn_visit_enable)");
  DeviceGuard guard(c->device);
  VN_HIP(hipMemcpyAsync(c->visit->count, src, (size_t)c->visit->state_words() * 4, hipMemcpyDeviceToDevice,
                        (hipStream_t)stream));
  return VN_OK;
}

int vn_visit_clear(vn_ctx* c, vn_stream_t stream) {
  if (!c) return fail(VN_EINVAL, "vn_visit_clear: NULL ctx");
  if (!c->visit) return fail(VN_ESTATE, "vn_visit_clear: visit counts are not enabled (vn_visit_enable)");
  DeviceGuard guard(c->device);
  return visit_clear(c->visit, c->recs, (hipStream_t)stream);
}

int vn_visit_stats(vn_ctx* c, int scene, int64_t* stats2_dev, vn_stream_t stream) {
  if (!c || !stats2_dev || scene < -1 || scene >= c->n_scenes) return fail(VN_EINVAL, "vn_visit_stats: bad args");
  if (!c->visit) return fail(VN_ESTATE, "vn_visit_stats: visit counts are not enabled (vn_visit_enable)");
  DeviceGuard guard(c->device);
  return visit_stats(c->visit, scene, stats2_dev, (hipStream_t)stream);
}

int vn_nav_episode_stats(vn_ctx* c, float* stats4, vn_stream_t stream) {
  if (!c || !stats4) return fail(VN_EINVAL, "vn_nav_episode_stats: NULL argument");
  if (!c->nav) return fail(VN_ESTATE, "vn_nav_episode_stats: navigation info is not enabled (vn_nav_enable)");
  DeviceGuard guard(c->device);
  return nav_episode_stats(c->nav, stats4, (hipStream_t)stream);
}

int vn_nav_sample_episodes(vn_ctx* c, int scene, int dist_lo, int dist_hi, int count, uint64_t seed, uint32_t salt,
                           int32_t* start_goal_dev, int32_t* dist_dev, int64_t* total_host, vn_stream_t stream) {
  if (!c) return fail(VN_EINVAL, "vn_nav_sample_episodes: NULL ctx");
  if (!c->nav) return fail(VN_ESTATE, "vn_nav_sample_episodes: navigation info is not enabled (vn_nav_enable)");
  DeviceGuard guard(c->device);
  return nav_sample_episodes(c->nav, scene, dist_lo, dist_hi, count, seed, salt, start_goal_dev, dist_dev,
                             total_host, (hipStream_t)stream);
}

int vn_nav_set_episode_log(vn_ctx* c, const vn_episode_log* log) {
  if (!c) return fail(VN_EINVAL, "vn_nav_set_episode_log: NULL ctx");
  if (!c->nav) return fail(VN_ESTATE, "vn_nav_set_episode_log: navigation info is not enabled (vn_nav_enable)");
  DeviceGuard guard(c->device);
  return nav_set_episode_log(c->nav, log);
}

int vn_nav_curriculum(vn_ctx* c, const vn_geo_curriculum* cfg) {
  if (!c) return fail(VN_EINVAL, "vn_nav_curriculum: NULL ctx");
  if (!c->nav) return fail(VN_ESTATE, "vn_nav_curriculum: navigation info is not enabled (vn_nav_enable)");
  if (cfg) {
    const char* bad = nullptr;
    if (cfg->mode != 1 && cfg->mode != 2) bad = "mode must be 1 or 2";
    else if (cfg->level < 1) bad = "level must be >= 1";
    else if (cfg->level_min < 1) bad = "level_min must be >= 1";
    else if (cfg->step < 1) bad = "step must be >= 1";
    else if (cfg->window < 0) bad = "window must be >= 0";
    else if (!(cfg->down >= 0.0f && cfg->down < cfg->up && cfg->up <= 1.0f)) bad = "need 0 <= down < up <= 1";
    if (bad) return fail(VN_EINVAL, std::string("vn_nav_curriculum: ") + bad);
  }
  DeviceGuard guard(c->device);
  VN_HIP(hipDeviceSynchronize());
  if (!cfg) {
    if (!c->cur) return VN_OK;
    VN_HIP(hipMemcpy(c->scenes, c->scenes_spd.data(), c->scenes_spd.size() * sizeof(SceneDev), hipMemcpyHostToDevice));
    c->scenes_host = c->scenes_spd;
    c->scenes_spd.clear();
    cur_destroy(c->cur);
    c->cur = nullptr;
    return VN_OK;
  }
  // the new tables first: a failure below leaves the context as it was
  std::vector<int64_t> order_off(c->n_scenes);
  for (int k = 0; k < c->n_scenes; ++k) order_off[k] = c->scenes_host[k].spd_off;
  CurState* cur = nullptr;
  int rc = cur_create(&cur, c->nav, *cfg, order_off);
  if (rc != VN_OK) return rc;
  static_assert(sizeof(SceneDev) % 4 == 0 && offsetof(SceneDev, cur_oi) % 4 == 0, "the level is a word of the table");
  cur->table = CurSceneTable{reinterpret_cast<int32_t*>(c->scenes), (int)(sizeof(SceneDev) / 4),
                             (int)(offsetof(SceneDev, cur_oi) / 4)};
  std::vector<SceneDev> sh = c->scenes_host;
  std::vector<int32_t> st((size_t)c->n_scenes * 4);
  hipError_t e = hipMemcpy(st.data(), cur->state, st.size() * 4, hipMemcpyDeviceToHost);
  for (int k = 0; k < c->n_scenes; ++k) {
    sh[k].cnt_off = cur->scenes_host[k].cnt_off;
    sh[k].maxd = cur->scenes_host[k].D;
    sh[k].cur_oi = st[k];
    sh[k].cur_mode = cfg->mode;
  }
  if (e == hipSuccess) {
    rc = cur_count_launch(cur, c->recs, nullptr, nullptr, 0, 0);  // ep_scene from the records
    if (rc == VN_OK) e = hipDeviceSynchronize();
  }
  // the scene table last: nothing of the context has changed before this copy
  if (e == hipSuccess && rc == VN_OK)
    e = hipMemcpy(c->scenes, sh.data(), sh.size() * sizeof(SceneDev), hipMemcpyHostToDevice);
  if (e != hipSuccess || rc != VN_OK) {
    cur_destroy(cur);
    return rc != VN_OK ? rc : hip_fail(e, "vn_nav_curriculum: enable");
  }
  if (c->cur) cur_destroy(c->cur);  // reconfigured: scenes_spd already holds the spd curriculum's table
  else c->scenes_spd = c->scenes_host;
  c->scenes_host = sh;
  c->cur = cur;
  return VN_OK;
}

int vn_nav_curriculum_advance(vn_ctx* c, vn_stream_t stream) {
  if (!c) return fail(VN_EINVAL, "vn_nav_curriculum_advance: NULL ctx");
  if (!c->cur) return fail(VN_ESTATE, "vn_nav_curriculum_advance: the geodesic curriculum is off (vn_nav_curriculum)");
  DeviceGuard guard(c->device);
  return cur_advance(c->cur, (hipStream_t)stream);
}

int vn_nav_curriculum_get_state(vn_ctx* c, int32_t* dst, vn_stream_t stream) {
  if (!c || !dst) return fail(VN_EINVAL, "vn_nav_curriculum_get_state: NULL argument");
  if (!c->cur) return fail(VN_ESTATE, "vn_nav_curriculum_get_state: the geodesic curriculum is off (vn_nav_curriculum)");
  DeviceGuard guard(c->device);
  return cur_get_state(c->cur, dst, (hipStream_t)stream);
}

int vn_nav_curriculum_set_state(vn_ctx* c, const int32_t* src, vn_stream_t stream) {
  if (!c || !src) return fail(VN_EINVAL, "vn_nav_curriculum_set_state: NULL argument");
  if (!c->cur) return fail(VN_ESTATE, "vn_nav_curriculum_set_state: the geodesic curriculum is off (vn_nav_curriculum)");
  DeviceGuard guard(c->device);
  return cur_set_state(c->cur, src, c->recs, (hipStream_t)stream);
}

int vn_nav_curriculum_tables(vn_ctx* c, int scene, const int32_t** order_dev, const int32_t** count_dev, int32_t* n,
                             int32_t* D) {
  if (!c || scene < 0 || scene >= c->n_scenes) return fail(VN_EINVAL, "vn_nav_curriculum_tables: bad args");
  if (!c->cur) return fail(VN_ESTATE, "vn_nav_curriculum_tables: the geodesic curriculum is off (vn_nav_curriculum)");
  const CurScene& S = c->cur->scenes_host[scene];
  if (order_dev) *order_dev = c->cur->order + S.order_off;
  if (count_dev) *count_dev = c->cur->count + S.cnt_off;
  if (n) *n = S.n;
  if (D) *D = S.D;
  return VN_OK;
}

int vn_set_info_buffers(vn_ctx* c, float* ep_return, int32_t* ep_length, int32_t* terminal_state,
                        uint8_t* truncated, int32_t* img_row, int32_t* goal_row) {
  if (!c) return fail(VN_EINVAL, "vn_set_info_buffers: NULL ctx");
  c->info_ret = ep_return;
  c->info_len = ep_length;
  c->info_term = terminal_state;
  c->info_trunc = truncated;
  c->info_img_row = img_row;
  c->info_goal_row = goal_row;
  return VN_OK;
}

int vn_set_schedule(vn_ctx* c, const int32_t* start_goal_dev, int len) {
  if (!c) return fail(VN_EINVAL, "vn_set_schedule: NULL ctx");
  if (len < 0 || (len > 0 && !start_goal_dev)) return fail(VN_EINVAL, "vn_set_schedule: bad schedule");
  DeviceGuard guard(c->device);
  if (c->sched) {
    VN_HIP(hipDeviceSynchronize());
    VN_HIP(hipFree(c->sched));
    c->sched = nullptr;
  }
  c->sched_len = 0;
  if (len > 0) {
    const size_t bytes = (size_t)c->n_envs * len * 2 * 4;
    if (hipMalloc((void**)&c->sched, bytes) != hipSuccess) return fail(VN_ENOMEM, "vn_set_schedule: alloc");
    VN_HIP(hipMemcpy(c->sched, start_goal_dev, bytes, hipMemcpyDefault));
    c->sched_len = len;
  }
  hipLaunchKernelGGL(rec_scatter_kernel, dim3((c->n_envs + 255) / 256), dim3(256), 0, 0, c->recs, c->n_envs,
                     RW_ST + ST_SCHED, (const int32_t*)nullptr);
  VN_HIP(hipGetLastError());
  return VN_OK;
}

int vn_set_tasks(vn_ctx* c, const int32_t* tasks_host, int n_tasks) {
  if (!c) return fail(VN_EINVAL, "vn_set_tasks: NULL ctx");
  if (n_tasks < 0 || (n_tasks > 0 && !tasks_host)) return fail(VN_EINVAL, "vn_set_tasks: bad tasks");
  for (int t = 0; t < n_tasks; ++t) {
    const int sc = tasks_host[2 * t], g = tasks_host[2 * t + 1];
    if (sc < 0 || sc >= c->n_scenes) return fail(VN_EINVAL, "vn_set_tasks: scene out of range");
    if (g < -1 || g >= c->scenes_host[sc].n) return fail(VN_EINVAL, "vn_set_tasks: goal out of range");
  }
  DeviceGuard guard(c->device);
  if (c->tasks) {
    VN_HIP(hipDeviceSynchronize());
    VN_HIP(hipFree(c->tasks));
    c->tasks = nullptr;
  }
  c->n_tasks = 0;
  if (n_tasks > 0) {
    if (hipMalloc((void**)&c->tasks, (size_t)n_tasks * 8) != hipSuccess) return fail(VN_ENOMEM, "vn_set_tasks: alloc");
    VN_HIP(hipMemcpy(c->tasks, tasks_host, (size_t)n_tasks * 8, hipMemcpyHostToDevice));
    c->n_tasks = n_tasks;
  }
  return VN_OK;
}

int vn_set_env_scenes(vn_ctx* c, const int32_t* env_scene_host) {
  if (!c || !env_scene_host) return fail(VN_EINVAL, "vn_set_env_scenes: NULL argument");
  for (int e = 0; e < c->n_envs; ++e)
    if (env_scene_host[e] < 0 || env_scene_host[e] >= c->n_scenes)
      return fail(VN_EINVAL, "vn_set_env_scenes: scene out of range");
  DeviceGuard guard(c->device);
  VN_HIP(hipMemcpy(c->env_scene, env_scene_host, (size_t)c->n_envs * 4, hipMemcpyHostToDevice));
  return VN_OK;
}

int vn_set_curriculum_scenes(vn_ctx* c, double complexity, const int32_t* modes_host, const double* offsets_host) {
  if (!c || !modes_host || !offsets_host) return fail(VN_EINVAL, "vn_set_curriculum_scenes: NULL argument");
  if (!(complexity >= 0.0)) return fail(VN_EINVAL, "vn_set_curriculum: bad complexity");
  if (c->cur)  // it would upload the spd curriculum's scene table over the geodesic one
    return fail(VN_ESTATE, "vn_set_curriculum: the geodesic curriculum is on (vn_nav_curriculum(ctx, NULL) first)");
  int any = 0;
  for (int i = 0; i < c->n_scenes; ++i) {
    if (modes_host[i] < 0 || modes_host[i] > 2) return fail(VN_EINVAL, "vn_set_curriculum: bad mode");
    any |= modes_host[i];
  }
  DeviceGuard guard(c->device);
  if (any && !c->cur_order) {
    // per scene and goal: states sorted by spd[s][g] (stable counting sort) + inclusive counts
    int64_t n_order = 0, n_cnt = 0;
    for (const SceneDev& S : c->scenes_host) {
      n_order += (int64_t)S.n * S.n;
      n_cnt += (int64_t)S.n * (S.maxd + 2);
    }
    std::vector<int32_t> order(n_order), cnt(n_cnt);
    for (const SceneDev& S : c->scenes_host) {
      const int n = S.n, B = S.maxd + 2;
      const int32_t* spd = c->spd_host.data() + S.spd_off;
      std::vector<int32_t> hist(B);
      for (int g = 0; g < n; ++g) {
        std::fill(hist.begin(), hist.end(), 0);
        for (int s = 0; s < n; ++s) hist[std::min(std::max(spd[(int64_t)s * n + g], -1), S.maxd) + 1]++;
        int32_t* cg = cnt.data() + S.cnt_off + (int64_t)g * B;
        int run = 0;
        for (int b = 0; b < B; ++b) {
          const int h = hist[b];
          hist[b] = run;  // start of bucket b
          run += h;
          cg[b] = run;    // inclusive count
        }
        int32_t* og = order.data() + S.spd_off + (int64_t)g * n;
        for (int s = 0; s < n; ++s) og[hist[std::min(std::max(spd[(int64_t)s * n + g], -1), S.maxd) + 1]++] = s;
      }
    }
    if (hipMalloc((void**)&c->cur_order, std::max<size_t>(order.size() * 4, 16)) != hipSuccess ||
        hipMalloc((void**)&c->cur_count, std::max<size_t>(cnt.size() * 4, 16)) != hipSuccess)
      return fail(VN_ENOMEM, "vn_set_curriculum: device allocation failed");
    VN_HIP(hipMemcpy(c->cur_order, order.data(), order.size() * 4, hipMemcpyHostToDevice));
    VN_HIP(hipMemcpy(c->cur_count, cnt.data(), cnt.size() * 4, hipMemcpyHostToDevice));
  }
  for (int i = 0; i < c->n_scenes; ++i) {  // the reference computes opt in Python floats (fp64)
    SceneDev& S = c->scenes_host[i];
    const double opt = complexity * ((double)S.maxd + offsets_host[i]) + 1.0;
    S.cur_oi = (int32_t)std::min<double>(std::max<double>(std::floor(opt), 0.0), (double)S.maxd);
    S.cur_mode = modes_host[i];
  }
  VN_HIP(hipMemcpy(c->scenes, c->scenes_host.data(), c->scenes_host.size() * sizeof(SceneDev), hipMemcpyHostToDevice));
  c->cur_mode = any ? 1 : 0;
  c->cur_c = complexity;
  return VN_OK;
}

int vn_set_curriculum(vn_ctx* c, double complexity, int mode, double offset) {
  if (!c) return fail(VN_EINVAL, "vn_set_curriculum: NULL ctx");
  std::vector<int32_t> modes(c->n_scenes, mode);
  std::vector<double> offsets(c->n_scenes, offset);
  return vn_set_curriculum_scenes(c, complexity, modes.data(), offsets.data());
}


int vn_set_max_episode_steps(vn_ctx* c, int max_steps) {
  if (!c) return fail(VN_EINVAL, "vn_set_max_episode_steps: NULL ctx");
  c->max_steps = max_steps;
  return VN_OK;
}

int vn_set_autoreset(vn_ctx* c, int on) {
  if (!c) return fail(VN_EINVAL, "vn_set_autoreset: NULL ctx");
  c->autoreset = on ? 1 : 0;
  return VN_OK;
}

int vn_set_output_reuse(vn_ctx* c, int on) {
  if (!c) return fail(VN_EINVAL, "vn_set_output_reuse: NULL ctx");
  c->reuse = on ? 1 : 0;
  c->reuse_arm = c->reuse;
  return VN_OK;
}

int vn_random_actions(vn_ctx* c, int32_t* actions_dev, uint64_t step, vn_stream_t stream) {
  if (!c || !actions_dev) return fail(VN_EINVAL, "vn_random_actions: NULL argument");
  DeviceGuard guard(c->device);
  hipLaunchKernelGGL(random_actions_kernel, dim3((c->n_envs + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                     actions_dev, c->n_envs, (uint32_t)c->seed ^ 0xA5A5A5A5u, (uint32_t)(c->seed >> 32), step);
  VN_HIP(hipGetLastError());
  return VN_OK;
}

int vn_gather_rows(const uint8_t* src_dev, int64_t row_bytes, const int32_t* rows_dev, int n, uint8_t* dst_dev,
                   vn_stream_t stream) {
  if (!src_dev || !rows_dev || !dst_dev || row_bytes <= 0 || n < 0) return fail(VN_EINVAL, "vn_gather_rows: bad args");
  if (n == 0) return VN_OK;
  hipLaunchKernelGGL(gather_rows_kernel, dim3((n + 3) / 4), dim3(256), 0, (hipStream_t)stream, src_dev, row_bytes,
                     rows_dev, n, dst_dev);
  VN_HIP(hipGetLastError());
  return VN_OK;
}

int vn_get_state(vn_ctx* c, int32_t* dst, vn_stream_t stream) {
  if (!c || !dst) return fail(VN_EINVAL, "vn_get_state: NULL argument");
  DeviceGuard guard(c->device);
  hipLaunchKernelGGL(rec_gather_kernel, dim3((c->n_envs + 255) / 256), dim3(256), 0, (hipStream_t)stream, c->recs,
                     c->n_envs, RW_ST, ST_COUNT, dst);
  VN_HIP(hipGetLastError());
  return VN_OK;
}

int vn_set_state(vn_ctx* c, const int32_t* src, vn_stream_t stream) {
  if (!c || !src) return fail(VN_EINVAL, "vn_set_state: NULL argument");
  DeviceGuard guard(c->device);
  hipLaunchKernelGGL(set_state_kernel, dim3((c->n_envs + 255) / 256), dim3(256), 0, (hipStream_t)stream, c->recs,
                     c->n_envs, src, c->scenes, c->n_scenes, c->graph);
  VN_HIP(hipGetLastError());
  return visit_refresh(c, cur_refresh(c, shape_refresh(c, VN_OK, nullptr, (hipStream_t)stream), (hipStream_t)stream),
                       nullptr, 0, (hipStream_t)stream);
}

int vn_get_episode_returns(vn_ctx* c, float* dst, vn_stream_t stream) {
  if (!c || !dst) return fail(VN_EINVAL, "vn_get_episode_returns: NULL argument");
  DeviceGuard guard(c->device);
  hipLaunchKernelGGL(rec_gather_kernel, dim3((c->n_envs + 255) / 256), dim3(256), 0, (hipStream_t)stream, c->recs,
                     c->n_envs, RW_RET, 1, reinterpret_cast<int32_t*>(dst));
  VN_HIP(hipGetLastError());
  return VN_OK;
}

int vn_set_episode_returns(vn_ctx* c, const float* src, vn_stream_t stream) {
  if (!c || !src) return fail(VN_EINVAL, "vn_set_episode_returns: NULL argument");
  DeviceGuard guard(c->device);
  hipLaunchKernelGGL(rec_scatter_kernel, dim3((c->n_envs + 255) / 256), dim3(256), 0, (hipStream_t)stream, c->recs,
                     c->n_envs, RW_RET, reinterpret_cast<const int32_t*>(src));
  VN_HIP(hipGetLastError());
  return VN_OK;
}

int vn_frame_arena(vn_ctx* c, const uint8_t** arena, int64_t* frame_bytes, int64_t* n_rows) {
  if (!c) return fail(VN_EINVAL, "vn_frame_arena: NULL ctx");
  if (arena) *arena = c->arena;
  if (frame_bytes) *frame_bytes = c->frame_bytes;
  if (n_rows) *n_rows = c->n_rows;
  return VN_OK;
}

int vn_scene_row_base(vn_ctx* c, int scene, int64_t* row_base) {
  if (!c || !row_base || scene < 0 || scene >= c->n_scenes) return fail(VN_EINVAL, "vn_scene_row_base: bad args");
  *row_base = c->scenes_host[scene].row_base;
  return VN_OK;
}

int vn_error_flags_sync(vn_ctx* c, uint32_t* flags, int clear) {
  if (!c || !flags) return fail(VN_EINVAL, "vn_error_flags_sync: NULL argument");
  DeviceGuard guard(c->device);
  VN_HIP(hipDeviceSynchronize());
  VN_HIP(hipMemcpy(flags, c->flags, 4, hipMemcpyDeviceToHost));
  if (clear) VN_HIP(hipMemset(c->flags, 0, 4));
  return VN_OK;
}

}  // extern "C"
