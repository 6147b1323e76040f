// Geodesic start curriculum (DESIGN.md "Geodesic curriculum"): per-goal start tables sorted by
// the nav tables' action distance, per-scene success counters and the level controller behind
// vn_nav_curriculum. The kernels live in vn_curriculum.hip; vn_env.hip owns the context, points
// its reset path at these tables and calls the launches below.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/vnav.h"
#include "vn_nav.h"

namespace vn {

// Buckets a sort pass keeps in LDS. A goal row with more distinct keys (B = D + 2) is sorted in
// ceil(B / kCurWindow) passes over the staged row, so no scene the nav tables accept is refused.
constexpr int kCurWindow = 256;

struct CurScene {
  int64_t geo_off;    // NavScene::geo_off
  int64_t order_off;  // element offset of the scene's [n][n] order block (SceneDev::spd_off)
  int64_t cnt_off;    // element offset of the scene's [n][D + 2] count block
  int32_t n;
  int32_t D;          // largest geo entry of the scene (0 when nothing is reachable)
};

// Where the level lives in the env kernels' scene table: word oi_word of every stride_words.
struct CurSceneTable {
  int32_t* words;
  int stride_words, oi_word;
};

struct CurState {
  int n_envs = 0, n_scenes = 0;
  vn_geo_curriculum cfg = {};
  std::vector<CurScene> scenes_host;
  CurScene* scenes = nullptr;
  int32_t* order = nullptr;     // per scene, per goal: states sorted stably by key(g, .)
  int32_t* count = nullptr;     // per scene, per goal: #states with key <= b, b < D + 2
  int32_t* state = nullptr;     // [4][S]: level, done, succ, D
  int32_t* ep_scene = nullptr;  // [E]: scene of the running episode
  CurSceneTable table = {};
};

// Builds the tables from the nav state's geodesic tables and sets every scene's level from cfg
// (checked by the caller). order_off[k]: the scene's offset in the order block. Synchronises.
// Touches nothing but its own allocations. VN_* code; on failure everything is freed.
int cur_create(CurState** out, const NavState* nav, const vn_geo_curriculum& cfg, const std::vector<int64_t>& order_off);
void cur_destroy(CurState* s);
// After the nav launch of a step, on its stream: counts the finished episodes, then notes every
// env's scene. count = 0: the refresh form (notes the scenes only).
int cur_count_launch(CurState* s, const void* recs, const uint8_t* done, const uint8_t* trunc, int count,
                     hipStream_t stream);
int cur_advance(CurState* s, hipStream_t stream);
int cur_get_state(CurState* s, int32_t* dst, hipStream_t stream);
int cur_set_state(CurState* s, const int32_t* src, const void* recs, hipStream_t stream);

}  // namespace vn
