// Geodesic reward shaping (DESIGN.md "Reward shaping and GAE"): the per-env progress record
// behind vn_nav_progress and its launch. The kernels, and vn_a2c_returns_ex, live in
// vn_shaping.hip; vn_env.hip owns the context and calls the launch below behind the nav launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vnav.h"
#include "vn_nav.h"

namespace vn {

enum { SHAPE_FORM_STEP = 0, SHAPE_FORM_REFRESH = 1 };

struct ShapeState {
  int n_envs = 0;
  int32_t* rec = nullptr;     // [3][E]: scene, goal and distance of the running episode
  int32_t* s_term = nullptr;  // stand-in for terminal_state where the caller set none
  // vn_set_nav_progress_outputs
  int32_t* dist_before = nullptr;
  int32_t* dist_after = nullptr;
  int32_t* progress = nullptr;
};

// Allocates the record and the stand-in; the caller then runs the refresh form. VN_* code.
int shape_create(ShapeState** out, int n_envs);
void shape_destroy(ShapeState* s);
// One thread per env on `stream`. SHAPE_FORM_STEP: behind the step's nav launch, with this
// step's done / trunc / term. SHAPE_FORM_REFRESH: the record of every env whose mask word is
// not 0 (mask NULL: every env) from its EnvRec; writes no output.
int shape_launch(ShapeState* s, const NavState* nav, int form, const void* recs, const int32_t* mask,
                 const uint8_t* done, const uint8_t* trunc, const int32_t* term, hipStream_t stream);

}  // namespace vn
