// State-visit counts (DESIGN.md "Visit counts and novelty bonus"): the per-state visit table and
// the per-episode seen-set behind vn_visit_enable, and their launches. The kernels, and
// vn_a2c_novelty_rewards, live in vn_visit.hip; vn_env.hip owns the context and calls the launch
// below behind the step's other side launches. Nothing here reads the nav tables.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/vnav.h"
#include "vn_nav.h"

namespace vn {

enum { VISIT_FORM_STEP = 0, VISIT_FORM_REFRESH = 1 };

struct VisitState {
  int n_envs = 0, n_scenes = 0;
  int W = 0;      // words of one env's seen bitmap: ceil(max_n / 32)
  int lanes = 8;  // lanes per env of the launch (VN_VISIT_LANES = 1, 8 or 64: the A/B forms)
  int64_t C = 0;  // cells: the scenes' state counts summed
  std::vector<int64_t> cell_off_host;  // [n_scenes + 1]
  int64_t* cell_off = nullptr;
  // one allocation of C + 2 E + E W words, the layout vn_visit_get_state copies out:
  uint32_t* count = nullptr;  // [C]
  int32_t* rec = nullptr;     // [2][E]: scene and distinct states of the running episode
  uint32_t* seen = nullptr;   // [E][W]: bit s of row e = the running episode has been in state s
  // stand-ins for done / terminal_state where the caller set none
  uint8_t* s_done = nullptr;
  int32_t* s_term = nullptr;
  // vn_set_visit_outputs
  int32_t* cell_out = nullptr;
  uint8_t* first_out = nullptr;
  int32_t* ep_distinct_out = nullptr;

  int64_t state_words() const { return C + (int64_t)n_envs * (2 + W); }
};

// Allocates and zeroes everything; the caller then runs the refresh form with add = 1.
// scene_n: states per scene. VN_EINVAL if they sum to 2^31 or more. VN_* code.
int visit_create(VisitState** out, int n_envs, const std::vector<int32_t>& scene_n);
void visit_destroy(VisitState* s);
// A group of `lanes` lanes per env on `stream`. VISIT_FORM_STEP: behind the step's env launch,
// with this step's done / term; starts the next episode of a done env when `autoreset`.
// VISIT_FORM_REFRESH: starts the episode of every env whose mask word is not 0 (mask NULL: every
// env) from its EnvRec, adding 1 to the start cell's count when `add`; writes no output.
int visit_launch(VisitState* s, int form, const void* recs, const int32_t* mask, const uint8_t* done,
                 const int32_t* term, int autoreset, int add, hipStream_t stream);
// count = 0, then the refresh form with add = 1 for every env.
int visit_clear(VisitState* s, const void* recs, hipStream_t stream);
// stats2 = [cells with count > 0, sum of the counts] of one scene, or of all with scene = -1.
int visit_stats(VisitState* s, int scene, int64_t* stats2_dev, hipStream_t stream);

}  // namespace vn
