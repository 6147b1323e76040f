// Navigation info of vn_step (DESIGN.md "vn_step: navigation info"): the per-scene action-graph
// geodesic tables and the per-env nav record behind vn_nav_enable. The kernels live in
// vn_nav.hip; vn_env.hip owns the context and calls these after its env_kernel launches.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/vnav.h"

namespace vn {

// The words of the per-env record (EnvRec, vn_env.hip) the nav kernels read: three 16-byte
// loads. vn_env.hip checks these against its own layout.
enum {
  NAV_RW_SCENE = 0,
  NAV_RW_STATE = 1,
  NAV_RW_GOAL = 2,
  NAV_RW_ELAPSED = 4,
  NAV_RW_NB = 8,
  NAV_REC_WORDS = 32,
};

constexpr int kNavMaxStates = 16384;  // int16 distances, one goal row in 32 KB of LDS

// Nav's per-scene fields: an array of its own, so SceneDev keeps its layout.
struct NavScene {
  int64_t geo_off;    // element offset of the scene's [n][n] int16 table, goal-major
  int32_t n;          // states
  int32_t graph_off;  // first row of the scene's [n][4] adjacency block
};

enum { NAV_FORM_STEP = 0, NAV_FORM_RESET = 1, NAV_FORM_ENABLE = 2, NAV_FORM_OUTPUTS = 3 };

struct NavState {
  int n_envs = 0, n_scenes = 0;
  std::vector<NavScene> scenes_host;
  NavScene* scenes = nullptr;
  int16_t* geo = nullptr;    // all scenes' tables
  int32_t* rec = nullptr;    // [2][E]: start distance, length offset
  float* acc = nullptr;      // [4][E]: finished episodes, successes, SPL sum, start-distance sum
  // stand-ins for done / truncated / ep_length where the caller set none
  uint8_t* s_done = nullptr;
  uint8_t* s_trunc = nullptr;
  int32_t* s_len = nullptr;
  // vn_set_nav_buffers
  int32_t* geo_dist = nullptr;
  int32_t* opt_action = nullptr;
  uint8_t* opt_mask = nullptr;
  uint8_t* ep_success = nullptr;
  float* ep_spl = nullptr;
  int32_t* ep_start = nullptr;
  // vn_set_nav_mask_output: where the following launches write the mask instead of opt_mask
  uint8_t* opt_mask_out = nullptr;
  // vn_nav_set_episode_log: the caller's buffers (capacity 0 = off) and the stand-in for the
  // ep_return info buffer, used only while a log is set
  vn_episode_log log = {};
  float* s_ret = nullptr;
  // vn_nav_sample_episodes' scratch: qualifying pairs per goal and their exclusive scan
  // ([max_n + 1], the last element the total)
  int max_n = 0;
  int32_t* ep_cnt = nullptr;
  int64_t* ep_off = nullptr;
};

// Allocates everything and builds the tables from the device graph ([rows][4] int32); the
// caller then runs nav_launch(NAV_FORM_ENABLE). graph_off / n per scene. VN_* code.
int nav_create(NavState** out, int n_envs, const std::vector<NavScene>& scenes, const int32_t* graph_dev);
void nav_destroy(NavState* s);
// One thread per env, after the env kernel on `stream`. done / trunc / ep_len: this step's
// (NAV_FORM_STEP only); ep_ret: the step's ep_return output, read only while a log is set.
int nav_launch(NavState* s, int form, const void* recs, const uint8_t* done, const uint8_t* trunc,
               const int32_t* ep_len, const float* ep_ret, hipStream_t stream);
// vn_nav_set_episode_log / vn_nav_sample_episodes on a live nav state (arguments checked here).
int nav_set_episode_log(NavState* s, const vn_episode_log* log);
int nav_sample_episodes(NavState* s, int scene, int dist_lo, int dist_hi, int count, uint64_t seed, uint32_t salt,
                        int32_t* start_goal, int32_t* dist, int64_t* total_host, hipStream_t stream);
int nav_episode_stats(NavState* s, float* stats4, hipStream_t stream);

}  // namespace vn
