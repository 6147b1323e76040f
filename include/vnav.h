/*
 * vnav.h — C ABI of libvnav.so, the MI355X-native batched cached-scene
 * visual-navigation engine (env.step hot path + A2C policy kernels).
 *
 * Every entry point returns 0 on success or a negative VN_E* code; the text of
 * the last error of the calling thread is available from vn_last_error().
 * Device buffers are caller-owned (e.g. torch tensors) and passed as raw
 * pointers; the library owns only the scene cache, per-env state and RNG keys.
 * All launches are stream-ordered and asynchronous; nothing here synchronises
 * the device except the explicitly named *_sync getters. A context is bound to
 * one GPU and is not thread-safe.
 *
 * Reference interfaces each group replaces (paths inside the reference repo
 * felipefelixarias/a2cat-vn-pytorch):
 *   vn_create/vn_destroy  <- THORDiscreteCachedEnv.__init__ loading the h5
 *                            datasets (environments/gym_ai2thor/envs/cached.py:19-36)
 *                            and THORCachedEnv.ensure_scene_loaded
 *                            (environments/gym_thor_cached.py:25-35)
 *   vn_reset              <- THORDiscreteCachedEnv.reset / _get_random_start_goal_tuple
 *                            (cached.py:38-57), THORCachedEnv.reset (gym_thor_cached.py:45-50)
 *   vn_observe            <- _render_observation / observe (cached.py:59-60,
 *                            gym_thor_cached.py:52-53)
 *   vn_step               <- THORDiscreteCachedEnv.step (cached.py:74-99) batched as the
 *                            deep_rl SubprocVecEnv.step with auto-reset
 *                            (experiments/thor_cached_auxiliary.py:66-67) and gym's
 *                            TimeLimit(max_episode_steps=900)
 *                            (environments/gym_ai2thor/__init__.py:45-49)
 *   vn_step_f32 / vn_observe_f32 <- the same under the wrappers TransposeImage +
 *                            ScaledFloatFrame (experiments/thor_cached_auxiliary.py:59-64)
 *   vn_policy_*           <- BigGoalHouseModel trunk + heads (models/goal.py:36-59,77-92)
 *   vn_a2c_*              <- the deep_rl A2C update used by the Trainer
 *                            (experiments/thor_cached_auxiliary.py:26-42)
 */
#ifndef VNAV_H
#define VNAV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vn_ctx vn_ctx;
typedef void* vn_stream_t; /* a hipStream_t; NULL = the null stream */

enum {
  VN_OK = 0,
  VN_EINVAL = -1,   /* bad argument */
  VN_EHIP = -2,     /* HIP runtime error */
  VN_ENOMEM = -3,   /* device allocation failed */
  VN_ESTATE = -4,   /* call not valid in the context's current state */
};

/* Device-side error flags (sticky; read with vn_error_flags_sync). */
enum {
  VN_FLAG_BAD_ACTION = 1u << 0,     /* an action outside [0,4) was treated as a blocked move */
  VN_FLAG_RESET_EXHAUSTED = 1u << 1,/* no start with spd[s][g] > 0 found within the bounded search */
  VN_FLAG_BAD_SCHEDULE = 1u << 2,   /* a schedule entry was out of range */
};

/* One cached scene (the h5 layout written by graph/util.py:202-247):
 *   graph        [N][4] int64, -1 = blocked (row convention util.py:212-218,231-232)
 *   spd          [N][N] int64 shortest_path_distance (used by reset, cached.py:43)
 *   observations [N][H][W][C] uint8, or NULL to synthesise frames on the device
 *                from the counter hash (scene_id, state, word) documented in DESIGN.md
 * Rewards follow reward_configuration (cached.py:70-72, 84-88): a plain move
 * returns reward_step (cached.py uses -0.0), reaching the goal reward_goal, a
 * blocked move reward_collision. terminal_obs = 0 re-emits the previous
 * observation on a terminal step (cached.py:90-96); 1 emits the goal-state frame
 * (graph/env.py:130-133). */
typedef struct vn_scene_desc {
  int32_t n_states;
  int32_t height, width, channels;
  const int64_t* graph;
  const int64_t* spd;
  const uint8_t* observations;
  float reward_goal;
  float reward_step;
  float reward_collision;
  int32_t terminal_obs;
  uint32_t synth_id; /* scene id fed to the frame hash when observations == NULL */
  /* [n_states][H][W][C] or NULL. When set, the second output of every observation is the
   * companion frame of the emitted state instead of the goal frame: OrientedGraphEnv's
   * observation (rgb, third-person rgb) of ThorGridWorld.render (graph/thor_graph.py:15-33,
   * environments/gym_graph/graph.py:56-58). */
  const uint8_t* companion;
} vn_scene_desc;

/* ---- environment ------------------------------------------------------- */

int vn_create(const vn_scene_desc* scenes, int n_scenes, int n_envs, uint64_t seed,
              int device, vn_ctx** out);
int vn_destroy(vn_ctx* ctx);

/* Re-sample (scene, start, goal) for every env whose env_mask_dev[e] != 0
 * (NULL = all envs). */
int vn_reset(vn_ctx* ctx, const int32_t* env_mask_dev, vn_stream_t stream);

/* Write the current (image, goal) frames, [n_envs][H][W][C] uint8 each, and the
 * current state index per env; any output may be NULL. Also refreshes the img_row /
 * goal_row info buffers (vn_set_info_buffers). */
int vn_observe(vn_ctx* ctx, uint8_t* obs_dev, uint8_t* goal_dev, int32_t* state_dev,
               vn_stream_t stream);

/* One batched env.step. actions_dev: [n_envs] int32. Outputs per env: the
 * (image, goal) frames (NULL skips the gather: index-only step), reward f32,
 * done u8, state int32 (after any auto-reset). */
int vn_step(vn_ctx* ctx, const int32_t* actions_dev, uint8_t* obs_dev, uint8_t* goal_dev,
            float* reward_dev, uint8_t* done_dev, int32_t* state_dev, vn_stream_t stream);

/* vn_step / vn_observe with the frames as a PyTorch policy takes them: float32
 * [n_envs][C][H][W] in [0, 1], the reference's TransposeImage + ScaledFloatFrame wrappers
 * (experiments/thor_cached_auxiliary.py:59-64) done while the frame leaves the scene cache.
 * Every value is float(u8) / 255.0f as IEEE fp32 division, bit for bit (ScaledFloatFrame's
 * np.float32(u8) / 255.0; a multiplication by 1/255 is not). Everything else is vn_step's /
 * vn_observe's: either frame pointer NULL (that frame is not written, the other one always
 * is), both NULL (index-only), companion frames as the second output, the info buffers, and
 * output reuse (vn_set_output_reuse: the same contract, for the float rows). The per-env
 * record also holds the format of what it wrote, so u8 and f32 calls may be mixed, into the
 * same memory too: a row written in one format is never taken for the other. The pointers
 * must be 4-byte aligned; rows whose planes are 16-byte aligned, of 3-channel frames with
 * H W a multiple of 4, take the vector path (16-byte stores). */
int vn_observe_f32(vn_ctx* ctx, float* obs_chw_dev, float* goal_chw_dev, int32_t* state_dev,
                   vn_stream_t stream);
int vn_step_f32(vn_ctx* ctx, const int32_t* actions_dev, float* obs_chw_dev, float* goal_chw_dev,
                float* reward_dev, uint8_t* done_dev, int32_t* state_dev, vn_stream_t stream);

/* ---- the five-frame observation of AuxiliaryGraph-v0 in the step's own launch ----
 * GoalGymGraphAuxiliaryEnv.observe (environments/gym_graph/graph.py:96-120) returns (rgb, goal
 * rgb, depth, segmentation, goal segmentation); experiments/thor_cached_auxiliary.py:76 makes
 * that env.
 *
 * vn_set_aux_arena registers the depth [rows][H][W][depth_channels] and segmentation
 * [rows][H][W][seg_channels] uint8 arenas (device memory, row-indexed like the frame arena:
 * vn_frame_arena, vn_scene_row_base). The caller owns the memory and keeps it alive and
 * unchanged while it is registered; the context only borrows it. Both pointers NULL clear the
 * setting. Like the other vn_set_* calls it replaces launch arguments: a captured graph holds
 * the old ones and must be recaptured. Setting arenas forgets what the aux outputs hold (their
 * next write is a full one) and synchronises the device. */
int vn_set_aux_arena(vn_ctx* ctx, const uint8_t* depth_dev, int depth_channels, const uint8_t* seg_dev,
                     int seg_channels);

enum {
  VN_OBS_U8_HWC = 0,  /* uint8 [n_envs][H][W][C], the arenas' own layout */
  VN_OBS_F32_CHW = 1, /* float [n_envs][C][H][W], float(u8) / 255 (vn_step_f32's arithmetic) */
};
/* The five outputs of one call, all in `format`. depth and segmentation are the aux-arena rows
 * at the info img_row, goal_segmentation the segmentation row at the info goal_row (whatever the
 * scene type: with companion frames goal_row is the companion row). In VN_OBS_U8_HWC the
 * pointers are uint8_t*: image / goal [n_envs][H][W][C], depth [n_envs][H][W][depth_channels],
 * the two segmentations [n_envs][H][W][seg_channels]. In VN_OBS_F32_CHW they are float*,
 * 4-byte aligned: [n_envs][channels][H][W] each. */
typedef struct vn_obs_set {
  void* image;
  void* goal;
  void* depth;
  void* segmentation;
  void* goal_segmentation;
  int32_t format;
} vn_obs_set;
/* vn_step / vn_observe (vn_step_f32 / vn_observe_f32 in VN_OBS_F32_CHW) with all five frames
 * written by the one launch. Scalars, info buffers, flags, auto-reset and companion frames are
 * theirs. image and goal must both be non-NULL; each of depth, segmentation, goal_segmentation
 * may be NULL: that frame is not written and what the context recorded about it stays.
 * Without an aux arena, or with two outputs that overlap, the call returns VN_EINVAL and
 * launches nothing.
 * Output reuse (vn_set_output_reuse) covers all five: per env and per output the context records
 * the destination row's address (with its format) and the arena row last written there, and with
 * reuse on a frame is skipped only when the recorded address is this launch's destination and the
 * recorded row is the row to emit (depth and segmentation change with the image row, goal
 * segmentation with the goal row). image and goal share their records with vn_step / vn_step_f32,
 * so two-frame and five-frame calls may be mixed into the same buffers. The armed full write of
 * vn_set_output_reuse(ctx, 1) writes all five, and a launch captured while armed is recorded as
 * a full write of all five and leaves the arm alone. Added to that contract: within one call
 * the five destinations do not overlap, and a caller who passes a buffer in another role than
 * before (say the segmentation buffer as goal_segmentation) calls vn_set_output_reuse(ctx, 1)
 * first. u8 rows take 16-byte lanes when H W is a multiple of 16 and every pointer is 16-byte
 * aligned (4-byte lanes for multiples of 4, bytes otherwise); float rows take the vector path
 * for 3 + 3 + 1 channels, H W a multiple of 4 and 16-byte aligned outputs. */
int vn_observe_aux(vn_ctx* ctx, const vn_obs_set* obs, int32_t* state_dev, vn_stream_t stream);
int vn_step_aux(vn_ctx* ctx, const int32_t* actions_dev, const vn_obs_set* obs, float* reward_dev,
                uint8_t* done_dev, int32_t* state_dev, vn_stream_t stream);

/* The A2C rollout's env step (the trainer's fast path; vn_step stays the gym/VecEnv
 * boundary): the action of env e is sampled in the step from the policy's output row e
 * (categorical over logits 0..A-1 of policy_out [E][8], Philox stream 3 with counter
 * (e, *counter_base_dev + counter), key seed — the draw of vn_policy_sample_dev), the
 * index-only step runs on it, and the per-step bookkeeping of vn_a2c_step_post follows
 * in the same launch: the next step's recurrent inputs (last action one-hot and reward,
 * times the episode mask m = 1 - done) and the finished-episode statistics accumulated per
 * env into episode_stats_env [3][E] (count, return sum, length sum; reduced and cleared by
 * vn_a2c_episode_stats). Optional outputs may be NULL. The a2c step is index-only by
 * construction: it has no frame outputs (the frames are addressed through the img_row /
 * goal_row info buffers), and its kernel with the heads fused carries no frame-copy code. */
typedef struct vn_a2c_step {
  const float* policy_out;          /* [E][8] */
  int num_actions;                  /* 1..7 */
  uint64_t seed;
  const int64_t* counter_base_dev;  /* may be NULL (base 0) */
  uint64_t counter;
  int32_t* actions;                 /* [E] sampled actions (out) */
  int64_t* prev_action;             /* [E] */
  float* prev_reward;               /* [E] */
  float* prev_mask;                 /* [E] */
  float* lra_next;                  /* [E][A+1] */
  float* mask_next;                 /* [E] */
  float* episode_stats_env;         /* [3][E], accumulated */
  /* Optional (a few envs): the policy heads computed in the same launch. With head_weight
   * non-NULL the logits and value of env e are head_bias + head_weight . head_input[e]
   * (head_weight [A+1][512], head_input [E][512], the same sums in the same order as
   * vn_policy_heads), written to head_out [E][8] — the buffer policy_out points at — and
   * sampled from; otherwise they are read from policy_out. */
  const float* head_weight;
  const float* head_bias;
  const float* head_input;
  float* head_out;
} vn_a2c_step;
int vn_step_a2c(vn_ctx* ctx, const vn_a2c_step* a2c, float* reward_dev, uint8_t* done_dev,
                int32_t* state_dev, vn_stream_t stream);

/* Optional persistent per-env info outputs written by every vn_step (any may be NULL):
 *   ep_return/ep_length: the finished episode's sum of rewards / length where done
 *     (RewardCollector statistics, experiments/thor_cached_auxiliary.py:60);
 *   terminal_state: the state index the single env returned as its terminal state;
 *   truncated: 1 where done came from the TimeLimit only;
 *   img_row/goal_row: global frame rows (arena rows, see vn_frame_arena) of the
 *     emitted frames — the zero-copy handle the fused policy input gather uses. */
int vn_set_info_buffers(vn_ctx* ctx, float* ep_return, int32_t* ep_length,
                        int32_t* terminal_state, uint8_t* truncated, int32_t* img_row,
                        int32_t* goal_row);

/* Test-mode exact replay: schedule_dev [n_envs][len][2] = (start, goal) consumed in
 * order by each env's subsequent resets (then back to the RNG). len = 0 clears. */
int vn_set_schedule(vn_ctx* ctx, const int32_t* start_goal_dev, int len);

/* Multi-scene tasks (gym_thor_cached.py:45-50): tasks_host [n][2] = (scene, goal);
 * goal = -1 draws a uniform goal. n = 0 restores fixed env->scene assignment. */
int vn_set_tasks(vn_ctx* ctx, const int32_t* tasks_host, int n_tasks);
/* Fixed env -> scene assignment (default e mod n_scenes). */
int vn_set_env_scenes(vn_ctx* ctx, const int32_t* env_scene_host);
int vn_set_max_episode_steps(vn_ctx* ctx, int max_steps); /* <= 0: no limit */

/* Curriculum start sampling (set_complexity / set_hardness: graph/util.py:88-143,
 * environments/gym_graph/graph.py:43-52, graph/env.py:101-106,
 * experiments/thor_cached_auxiliary.py:68-70). opt = complexity*(maxd + offset) + 1 with
 * maxd the scene's largest spd; starts with 0 < spd[s][g] <= opt are drawn uniformly
 * (mode 1, OrientedGraphEnv/sample_initial_state) or with probability 0.9 among them and
 * 0.1 among the farther ones (mode 2, SimpleGraphEnv/sample_initial_position); mode 0 =
 * off (uniform rejection sampling of cached.py). One O(1) draw from per-goal sorted tables
 * built on the first call. complexity and offset are fp64 (the reference computes opt in
 * Python floats, so floor(opt) matches it bit for bit). */
int vn_set_curriculum(vn_ctx* ctx, double complexity, int mode, double offset);
/* Per-scene (mode, offset) arrays of n_scenes entries (host memory). */
int vn_set_curriculum_scenes(vn_ctx* ctx, double complexity, const int32_t* modes_host,
                             const double* offsets_host);
int vn_set_autoreset(vn_ctx* ctx, int on);                /* default on */

/* Output reuse for callers that step into the same obs_dev / goal_dev buffers every call.
 * The context records, per env and in device memory (stream order), the address of the
 * image row and of the goal row it last wrote and the arena row whose bytes went there.
 * With reuse on, a vn_step / vn_observe that gets both buffers skips the copy of a frame
 * whose destination row is the recorded address and already holds the arena row to emit
 * (the goal frame between resets; the image on a blocked move or a kept terminal
 * observation). The kernel cannot see other writers, so this is a contract: with reuse on,
 * nothing but vn_step / vn_observe of this context writes to those rows between two calls,
 * and no row is shared by two envs. Off by default (every launch writes every row).
 * on = 1: the first launch with both buffers after the call still writes every row (call
 * it again whenever the buffers' contents may have changed hands, e.g. a freshly allocated
 * buffer at a recycled address); later ones may skip. Host-only, no synchronisation. A
 * captured launch replays correctly: the records live on the device. A launch that is
 * captured into a graph while the full write is still armed is recorded as a full write
 * (every replay of it writes every row) and does not use the arm up: the next launch that
 * is executed directly still writes every row. */
int vn_set_output_reuse(vn_ctx* ctx, int on);

/* Synthetic uniform actions in [0,4) from Philox(seed, env, step). */
int vn_random_actions(vn_ctx* ctx, int32_t* actions_dev, uint64_t step, vn_stream_t stream);
/* dst[i] = src[rows[i]] (rows of row_bytes, device memory): gathers the auxiliary frames
 * (depth, segmentation) of AuxiliaryGraph's 5-tuple observation (environments/gym_graph/
 * graph.py:96-120) by the env's img_row/goal_row indices. */
int vn_gather_rows(const uint8_t* src_dev, int64_t row_bytes, const int32_t* rows_dev, int n, uint8_t* dst_dev,
                   vn_stream_t stream);

/* Scene ingest: resize n packed uint8 frames [n][h][w][c] -> [n][oh][ow][c] on the device, as
 * the reference's cached env does per emitted frame (skimage.transform.resize(frame,
 * image_size, anti_aliasing=True), environments/gym_ai2thor/envs/cached.py:62-64), stored as
 * round(255 x) bytes. Per output byte, in this order (DESIGN.md "Scene ingest: resize on the
 * device"):
 *   1. Gaussian along the rows axis on the uint8 input, fp64 without contraction, in scipy's
 *      symmetric order acc = x[i] w[R]; acc += (x[i+j] + x[i-j]) w[j+R] for j = -R..-1; the
 *      result is floored to a byte. The border mirrors without repeating the edge sample
 *      (period 2 (n - 1), any number of reflections; n = 1: always sample 0);
 *   2. the same along the columns axis on those bytes, floored to a byte again;
 *   3. bilinear sampling at r = (i + 0.5) h / oh - 0.5, c = (j + 0.5) w / ow - 0.5 in 64-bit
 *      integers: S / D with D = 4 oh ow, rounded to nearest, ties to even.
 * taps_*_host: the axis's 2R+1 normalised weights on the host, fp64, w[k + R] for k = -R..R
 * (vnav.scenes.resize_taps); they are read before the call returns and travel in the launch
 * arguments, so their bits are the caller's and the call allocates and copies nothing. Only
 * w[0..R] enter the sum (the symmetric form). NULL with radius 0 skips the axis's pass.
 * oh == h && ow == w is a plain device-to-device copy. Stream-ordered on the current device; src
 * and dst need no alignment and must not overlap.
 * VN_EINVAL, with nothing written: NULL frames; n, a size or a channel count <= 0; c not 1 or 3;
 * oh > h or ow > w (upsampling would need the warp's border rule); a radius outside
 * 0..VN_RESIZE_MAX_RADIUS (32 covers every factor up to 17 per axis: R = int(2 (f - 1) + 0.5));
 * NULL taps with a radius > 0; w * c > VN_RESIZE_MAX_ROW_BYTES (two filtered rows must fit
 * the workgroup's LDS). */
#define VN_RESIZE_MAX_RADIUS 32
#define VN_RESIZE_MAX_ROW_BYTES 24576
int vn_resize_frames(const uint8_t* src_dev, int64_t n, int h, int w, int c, int oh, int ow,
                     const double* taps_rows_host, int radius_rows, const double* taps_cols_host, int radius_cols,
                     uint8_t* dst_dev, vn_stream_t stream);

/* Per-env state tensors (device, [n_envs] int32 each): for checkpoint/resume and tests.
 * Order: scene, state, goal, obs_state, elapsed, episode(reset count), sched_pos.
 * Both are small stream-ordered kernels over the context's per-env records; vn_set_state
 * also rebuilds what a record caches for its (scene, state): graph neighbours, row bases,
 * rewards. Scene and state must be inside the tables vn_create was given. */
int vn_get_state(vn_ctx* ctx, int32_t* dst_dev_7xE, vn_stream_t stream);
int vn_set_state(vn_ctx* ctx, const int32_t* src_dev_7xE, vn_stream_t stream);
/* Running (unfinished) episode return per env, [n_envs] f32 on the device: the rest of the
 * per-env state a checkpoint needs (the finished-episode return RewardCollector reports,
 * A18, is this sum at done). Tasks, scene assignment and curriculum are configuration and
 * are re-applied by the caller. */
int vn_get_episode_returns(vn_ctx* ctx, float* dst_dev_E, vn_stream_t stream);
int vn_set_episode_returns(vn_ctx* ctx, const float* src_dev_E, vn_stream_t stream);

/* Navigation info: geodesic distance to the goal, optimal action, success and SPL per env.
 * on = 1 builds, per scene and on the device, the action-graph geodesic table geo[g][s]: the
 * least number of actions that lead from state s to state g along graph[.][0..3] (-1 = no
 * edge); 0 for s == g, -1 where g cannot be reached. int16, goal-major. This is not the
 * scene's spd table, which ranks start states for the sampler and counts no rotations in
 * place. It also allocates the per-env nav record (start distance, length offset) and the
 * per-env accumulators, and starts every env's record from its current state: an env with
 * elapsed > 0 is measured from here (start distance = its current distance, length offset =
 * elapsed); every later episode has offset 0. A scene of more than 16384 states returns
 * VN_EINVAL and enables nothing. on = 0 frees everything. Replaces launch arguments like the
 * vn_set_* calls: synchronises, and a captured graph must be recaptured.
 * While enabled, vn_step / vn_step_f32 / vn_step_aux / vn_step_a2c launch one more small kernel
 * on the caller's stream after the step's own, vn_reset a refresh form of it (distance, mask,
 * action and the start record of the envs it reset; it counts nothing). vn_set_state leaves the
 * nav record alone: restore it with vn_set_nav_state right after; the next step recomputes
 * distance, mask and action. */
int vn_nav_enable(vn_ctx* ctx, int on);
/* Persistent [n_envs] device outputs, written for every env by every step (any may be NULL):
 *   geo_dist: geo[goal][state] of the state the step leaves the env in (after an auto-reset
 *     the new episode's state and goal);
 *   optimal_mask: bit a set iff graph[state][a] != -1, geo_dist > 0 and
 *     geo[goal][graph[state][a]] == geo_dist - 1; 0 on the goal and where it is unreachable;
 *   optimal_action: lowest set bit of the mask, -1 if the mask is 0;
 *   ep_start_dist: geodesic distance at the start of the episode this step belonged to (the
 *     finished episode where done, never the new one);
 *   ep_success: done && !truncated (reaching the goal exactly at the time limit succeeds);
 *   ep_spl: 0 unless ep_success; then, with l = ep_start_dist and p = the finished episode's
 *     length minus the length offset, (float)l / (float)max(p, l), one fp32 division; 1 when
 *     l == 0, 0 when l < 0.
 * The call also writes the current geo_dist / optimal_mask / optimal_action into the new
 * buffers. VN_ESTATE before vn_nav_enable. Synchronises. */
int vn_set_nav_buffers(vn_ctx* ctx, int32_t* geo_dist, int32_t* optimal_action, uint8_t* optimal_mask,
                       uint8_t* ep_success, float* ep_spl, int32_t* ep_start_dist);
/* Redirects only the optimal_mask output of the following nav launches to another [n_envs]
 * device buffer, e.g. a trainer's per-step slot, as vn_set_info_buffers does for the row
 * outputs: a host-side pointer swap, no launch and no synchronisation (a launch captured in a
 * graph keeps the pointer it was recorded with). NULL restores the buffer given to
 * vn_set_nav_buffers, which also drops any redirection. The caller owns the buffer and keeps it
 * alive while launches may write it. VN_ESTATE before vn_nav_enable. */
int vn_set_nav_mask_output(vn_ctx* ctx, uint8_t* optimal_mask_E);
/* The scene's [n][n] int16 table on the device, indexed [goal][state]. */
int vn_nav_table(vn_ctx* ctx, int scene, const int16_t** geo_dev, int32_t* n);
/* The part of the nav record a checkpoint needs, [2][n_envs] int32 on the device: start
 * distance, length offset. Stream-ordered copies. */
int vn_get_nav_state(vn_ctx* ctx, int32_t* dst_dev_2xE, vn_stream_t stream);
int vn_set_nav_state(vn_ctx* ctx, const int32_t* src_dev_2xE, vn_stream_t stream);
/* stats4 (device) = fixed-order sums over envs of the per-env accumulators: finished
 * episodes, successes, SPL sum, start-distance sum (an unreachable start adds its -1); the
 * accumulators are then zeroed. Same inputs, same bits. No host argument: capturable. */
int vn_nav_episode_stats(vn_ctx* ctx, float* stats4_dev, vn_stream_t stream);

/* Geodesic progress of every step (DESIGN.md "Reward shaping and GAE"): the action-graph
 * distance to the goal before and after the step, for a dense progress reward formed by the
 * trainer (vn_a2c_returns_ex). The step's own reward, ep_return and every other output stay as
 * they are. on = 1 allocates a per-env record [3][n_envs] int32 (scene, goal and distance of the
 * running episode) and starts it from every env's current state; on = 0 frees it. While it is
 * on, vn_step / vn_step_f32 / vn_step_aux / vn_step_a2c launch one more small kernel behind the
 * nav launch (before the curriculum's), one thread per env:
 *   before = the record's distance;
 *   after  = 0 where done && !truncated (the state is the goal); geo[goal][terminal_state] of
 *            the finished episode's scene and goal where done && truncated (after an auto-reset
 *            the env already holds the next episode, so scene and goal come from the record and
 *            the state from the step's terminal_state, looked up clamped to the table);
 *            otherwise the distance of the state the step left the env in;
 *   progress = before - after where both are >= 0, else 0 (-1: the goal is unreachable);
 * then the record takes the env's scene, goal and distance (after an auto-reset the new
 * episode's). vn_reset launches the refresh form for the envs it reset, vn_set_state for every
 * env. terminal_state is read from the vn_set_info_buffers buffer, or from a stand-in of the
 * progress state where the caller set none. Synchronises and replaces launch arguments (a
 * captured graph must be recaptured). VN_ESTATE before vn_nav_enable; vn_nav_enable (either way)
 * first switches progress off. */
int vn_nav_progress(vn_ctx* ctx, int on);
/* Where the following progress launches write, [n_envs] int32 on the device each, any may be
 * NULL (not written): a host-side pointer swap like vn_set_nav_mask_output, no launch and no
 * synchronisation (a launch captured in a graph keeps the pointers it was recorded with). The
 * caller owns the buffers. VN_ESTATE before vn_nav_progress. */
int vn_set_nav_progress_outputs(vn_ctx* ctx, int32_t* dist_before, int32_t* dist_after, int32_t* progress);
/* The progress record, [3][n_envs] int32 on the device: scene, goal, distance. Stream-ordered
 * copies; set after vn_set_state, which refreshes the record from the env states. */
int vn_get_nav_progress_state(vn_ctx* ctx, int32_t* dst_dev_3xE, vn_stream_t stream);
int vn_set_nav_progress_state(vn_ctx* ctx, const int32_t* src_dev_3xE, vn_stream_t stream);

/* State-visit counts (DESIGN.md "Visit counts and novelty bonus"). Independent of vn_nav_enable:
 * no geodesic table is needed. on = 1 allocates, on the device,
 *   cell_off [n_scenes + 1] int64: the prefix sum of the scenes' state counts; state s of scene
 *     k is cell cell_off[k] + s, and C = cell_off[n_scenes] (VN_EINVAL if C >= 2^31);
 *   count [C] uint32, zeroed: how often an env arrived in the cell;
 *   per env the scene of the running episode (ep_scene), the number of distinct states it has
 *     been in (ep_distinct) and their bitmap seen[W], W = ceil(max n_states / 32) words;
 * then starts every env from its current state (its bit set, ep_distinct = 1, its cell counted
 * once). While it is on, vn_step / vn_step_f32 / vn_step_aux / vn_step_a2c launch one more small
 * kernel behind their other side launches, a group of 8 lanes per env:
 *   the arrival state is (ep_scene, terminal_state) where done (after an auto-reset the env
 *     already holds the next episode), else the env's (scene, state); both are clamped into the
 *     tables; cell = cell_off[scene] + state;
 *   count[cell] += 1 (an atomic add whose old value is unused: the table after the launch is
 *     exact and independent of order);
 *   first = the state's bit was clear in seen; the bit is set and ep_distinct += first;
 *   the outputs of vn_set_visit_outputs are written;
 *   where done and auto-reset is on, the next episode starts: seen cleared, ep_scene = the env's
 *     scene, the start state's bit set, ep_distinct = 1, and the start cell counted once.
 * With auto-reset off (vn_set_autoreset(ctx, 0)) a done env's episode goes on: its seen-set and
 * ep_distinct stay, later steps (the env keeps moving from where it stopped, terminal re-emit
 * steps included) are counted into the same episode, and every done step reports ep_distinct;
 * the episode starts with vn_reset. vn_reset starts the episode of the envs it reset, counting
 * their start cells; vn_set_state starts every env's episode without counting (restore the
 * visit state with vn_visit_set_state after it). terminal_state and done are read from the
 * caller's buffers, or from stand-ins of the visit state where the caller set none.
 * Synchronises and replaces launch arguments (a captured graph must be recaptured). A refusal
 * leaves the context as it was. on = 0 frees everything. */
int vn_visit_enable(vn_ctx* ctx, int on);
/* Where the following visit launches write, [n_envs] on the device each, any may be NULL (not
 * written): cell int32 (the arrival cell), first uint8 (1 = the episode's first visit of it),
 * ep_distinct int32 (the finished episode's distinct states where done, else 0). A host-side
 * pointer swap like vn_set_nav_progress_outputs: no launch, no synchronisation. The caller owns
 * the buffers. VN_ESTATE before vn_visit_enable. */
int vn_set_visit_outputs(vn_ctx* ctx, int32_t* cell, uint8_t* first, int32_t* ep_distinct);
/* The live table of one scene ([*n] uint32), and of all scenes with its offsets ([*cells] uint32,
 * [n_scenes + 1] int64): device pointers into the visit state, valid until vn_visit_enable.
 * Any output pointer may be NULL. VN_ESTATE before vn_visit_enable. */
int vn_visit_table(vn_ctx* ctx, int scene, const uint32_t** count_dev, int32_t* n);
int vn_visit_cells(vn_ctx* ctx, const uint32_t** count_dev, const int64_t** cell_off_dev, int64_t* cells);
/* The visit state a checkpoint needs, C + n_envs (2 + W) 32-bit words on the device: count [C],
 * then the [2][n_envs] int32 record (ep_scene, ep_distinct), then seen [n_envs][W]. Stream-ordered
 * copies; set after vn_set_state, which starts every episode again. */
int vn_visit_get_state(vn_ctx* ctx, int32_t* dst_dev, vn_stream_t stream);
int vn_visit_set_state(vn_ctx* ctx, const int32_t* src_dev, vn_stream_t stream);
/* count = 0, then every env starts from its current state as vn_visit_enable starts it. On
 * `stream`, with no host value: may be captured in a graph. */
int vn_visit_clear(vn_ctx* ctx, vn_stream_t stream);
/* stats2_dev, int64 [2] on the device, zeroed by the call: the number of cells with count > 0
 * and the sum of the counts, of one scene or of all (scene = -1). Integer sums: the same bits
 * from the same table. VN_EINVAL: NULL stats2_dev, scene outside -1 .. n_scenes - 1. */
int vn_visit_stats(vn_ctx* ctx, int scene, int64_t* stats2_dev, vn_stream_t stream);

/* Fixed-episode evaluation (DESIGN.md "Fixed-episode evaluation").
 * Draws `count` (start, goal) pairs of `scene`, with replacement, uniformly from
 * Q = {(g, s) : dist_lo <= geo[g][s] <= dist_hi}, Q ordered by g, then by s. Exact, so a host
 * restatement reproduces it bit for bit: draw j takes r = Philox4x32-10((j, 0, salt, 5), key =
 * seed), u = r.x * 2^32 + r.y, idx = (u * total) >> 64 with total = |Q| (<= 2^28), and is the
 * idx-th pair of Q. dist_lo >= 1, so the goal itself and unreachable pairs (-1) never qualify;
 * dist_hi is clamped to 32767. start_goal_dev [count][2] = (start, goal); dist_dev [count] =
 * geo[g][s] of each pair, may be NULL; *total_host = |Q|. total == 0 returns VN_OK and writes no
 * pair. Off the step path: three small launches on `stream`, and the call synchronises with it.
 * Its scratch belongs to the nav state. VN_ESTATE before vn_nav_enable. VN_EINVAL, with nothing
 * written: scene out of range, dist_lo < 1, dist_hi < dist_lo, count <= 0, NULL start_goal_dev
 * or total_host. */
int vn_nav_sample_episodes(vn_ctx* ctx, int scene, int dist_lo, int dist_hi, int count, uint64_t seed,
                           uint32_t salt, int32_t* start_goal_dev, int32_t* dist_dev, int64_t* total_host,
                           vn_stream_t stream);
/* Per-episode log of the nav step. The buffers are the caller's, on the device; nothing is
 * allocated per step. While a log is set, the nav launch behind every vn_step* does, for an env
 * with done: k = count[e]; if k < want[e] it writes slot k (index k * n_envs + e) with exactly
 * the values the step's own ep_success / ep_spl / ep_start_dist outputs carry, the finished
 * episode's length minus the nav length offset and its return; then count[e] = k + 1. Slots at
 * or beyond want[e] are never written. The return is read from the ep_return info buffer
 * (vn_set_info_buffers), or from a stand-in of the nav state where the caller set none.
 * The call zeroes count, replaces launch arguments like the vn_set_* calls (it synchronises; a
 * captured graph holds the arguments it was recorded with), and log = NULL switches the log
 * off. VN_ESTATE before vn_nav_enable; VN_EINVAL for capacity <= 0 or any NULL buffer. */
typedef struct vn_episode_log {
  int32_t capacity;    /* slots per env */
  const int32_t* want; /* [n_envs] episodes to record for env e, 0..capacity */
  int32_t* count;      /* [n_envs] finished so far; zeroed by the call */
  uint8_t* success;    /* [capacity][n_envs], slot-major: adjacent envs write adjacent bytes */
  int32_t* length;     /* finished episode's length minus the nav length offset */
  int32_t* start_dist;
  float* spl;
  float* ep_return;
} vn_episode_log;
int vn_nav_set_episode_log(vn_ctx* ctx, const vn_episode_log* log);

/* Geodesic start curriculum (DESIGN.md "Geodesic curriculum"): resets draw the start among the
 * states within `level` actions of the goal, in the unit of geo_dist and SPL, and the level
 * moves with the measured success rate on the device.
 * vn_nav_curriculum(cfg) builds, per scene and on the device, from the geodesic table: D = its
 * largest entry, key(g, s) = clamp(geo[g][s], -1, D) + 1, order[g][] = the states sorted stably
 * by key (equal keys in ascending state order), count[g][b] = #states with key <= b for
 * b < D + 2. Resets then draw from these tables exactly as vn_set_curriculum's draw does from
 * its own: near set 0 < geo <= level; mode 1 uniform over it; mode 2 with probability 0.9 over it
 * and 0.1 over the farther states; an empty near set falls to the farther ones, then to the
 * rejection loop. The env kernels are unchanged. Costs n^2 int32 per scene for the order table
 * (what vn_set_curriculum's table costs) plus n (D + 2) for the counts; any D the nav tables
 * can hold is accepted. cfg = NULL switches it off and restores what was there before bit for
 * bit: a vn_set_curriculum that was active is active again with its threshold, otherwise
 * starts are uniform. Calling it again replaces the configuration and restarts levels and
 * counters. Synchronises and replaces launch arguments (a captured graph must be recaptured).
 * VN_ESTATE before vn_nav_enable. VN_EINVAL: mode not 1 or 2, level < 1, level_min < 1,
 * step < 1, window < 0, or not 0 <= down < up <= 1. VN_ENOMEM with everything freed. Every
 * refusal leaves the context as it was. While it is on, vn_set_curriculum* return VN_ESTATE;
 * vn_nav_enable (either way) first switches it off.
 * Per scene the state is int32 level, done, succ; per env ep_scene, the scene of the running
 * episode. While window > 0 every vn_step* launches one more small kernel behind the nav
 * launch: an env with done adds 1 to done[ep_scene[e]], and to succ[ep_scene[e]] unless
 * truncated; then ep_scene[e] = the env's scene. vn_reset and vn_set_state launch its refresh
 * form (ep_scene only). With window == 0 no launch is added anywhere. */
typedef struct vn_geo_curriculum {
  int32_t mode;      /* 1 uniform over 0 < geo <= level, 2 the 0.9 / 0.1 split */
  int32_t level;     /* start level, clamped per scene to [min(level_min, D), D] */
  int32_t level_min; /* >= 1 */
  int32_t step;      /* >= 1 */
  int32_t window;    /* finished episodes per decision; 0 = fixed level */
  float up, down;    /* 0 <= down < up <= 1 */
} vn_geo_curriculum;
int vn_nav_curriculum(vn_ctx* ctx, const vn_geo_curriculum* cfg);
/* One small launch on `stream`, no host value: capturable, and a captured update stays valid
 * while the level moves. For every scene with done >= window: r = (float)succ / (float)done
 * (one fp32 division); r >= up: level = min(level + step, D); else r <= down: level =
 * max(level - step, min(level_min, D)); then done = succ = 0 and the scene's threshold takes
 * the level. window == 0: launches nothing, VN_OK. VN_ESTATE while the curriculum is off. */
int vn_nav_curriculum_advance(vn_ctx* ctx, vn_stream_t stream);
/* [4][n_scenes] int32 on the device: level, done, succ, D. Stream-ordered. set_state takes rows
 * 0..2 (row 3 is ignored), holds each level to [min(level_min, D), D], writes the scenes'
 * thresholds and sets ep_scene from the env records: call it after vn_set_state. */
int vn_nav_curriculum_get_state(vn_ctx* ctx, int32_t* dst_dev_4xS, vn_stream_t stream);
int vn_nav_curriculum_set_state(vn_ctx* ctx, const int32_t* src_dev_4xS, vn_stream_t stream);
/* The scene's tables on the device: order [n][n], count [n][D + 2], both indexed by goal. */
int vn_nav_curriculum_tables(vn_ctx* ctx, int scene, const int32_t** order_dev, const int32_t** count_dev,
                             int32_t* n, int32_t* D);

/* Scene-cache arena: all scenes' frames back to back, row = frame. */
int vn_frame_arena(vn_ctx* ctx, const uint8_t** arena_dev, int64_t* frame_bytes,
                   int64_t* n_rows);
int vn_scene_row_base(vn_ctx* ctx, int scene, int64_t* row_base);

int vn_error_flags_sync(vn_ctx* ctx, uint32_t* flags, int clear);
int vn_num_envs(vn_ctx* ctx);


/* ---- policy: BigGoalHouseModel trunk + heads (models/goal.py:36-59,77-92) ---- */

typedef struct vn_policy vn_policy;

/* Frames for a batch of n samples (uint8 HWC, as the env emits them): sample i uses
 * image + image_rows[i]*frame_bytes and goal + goal_rows[i]*frame_bytes (rows NULL =
 * i). Passing the scene-cache arena (vn_frame_arena) with the env's img_row/goal_row
 * info makes the policy input a zero-copy gather. image_f32/goal_f32, when set, are
 * dense float [n][3][H][W] frames (the reference's TransposeImage + ScaledFloatFrame
 * output) used instead. */
typedef struct vn_frames {
  const uint8_t* image;
  const uint8_t* goal;
  const int32_t* image_rows;
  const int32_t* goal_rows;
  int64_t frame_bytes;
  const float* image_f32;
  const float* goal_f32;
} vn_frames;

/* frame 84x84 or 174x174; num_actions 1..7. Parameters live in one flat fp32 buffer:
 * per layer (conv1, conv2, conv3, conv4, conv_merge, head) W [Cout][ky][kx][Cin] (K padded
 * to a multiple of 4) then b [Cout]; the head stacks policy_logits (rows 0..A-1) and critic
 * (row A). layout12 = (w, b) float offsets per layer. */
int vn_policy_create(int frame_h, int frame_w, int num_actions, vn_policy** out);
int vn_policy_destroy(vn_policy* p);
int vn_policy_info(vn_policy* p, int64_t* n_params, int64_t* act_floats_per_sample, int64_t* layout12);
int vn_policy_workspace_floats(vn_policy* p, int64_t n_samples, int64_t* floats);
/* out [n][8]: logits in 0..A-1, value at A (out may be NULL for a VN_POLICY_LSTM policy:
 * trunk only, features kept in the activation store). Activations of the n samples are kept at
 * sample offset act_offset of an activation store holding act_capacity samples. */
int vn_policy_forward(vn_policy* p, const float* params, const vn_frames* frames, int n, float* acts,
                      int64_t act_capacity, int64_t act_offset, float* out, vn_stream_t stream);
/* Gradients of the n samples stored from offset 0 given dL/d(out) [n][8]; overwrites grads
 * (flat, same layout as params). Consumes the stored activations (conv1's are overwritten). */
int vn_policy_backward(vn_policy* p, const float* params, const vn_frames* frames, int n, float* acts,
                       int64_t act_capacity, const float* dout, float* grads, float* workspace,
                       vn_stream_t stream);

/* ---- recurrent core: MaskedRNN(nn.LSTM(512 + A + 1, 512)) (models/goal.py:61-67, 91-92) ----
 * A policy created with VN_POLICY_LSTM appends W_cat [2048][xcat] = [W_ih | 0 pad | W_hh]
 * (torch gate order i, f, g, o), b_ih [2048], b_hh [2048] to the flat parameters; its heads
 * read h_t instead of the conv_merge features. info8 = (W_cat, b_ih, b_hh offsets, xcat,
 * xoff = column of h in W_cat, lin = 512 + A + 1, hidden 512, 0).
 * Step t of a batch of E: x5 [E][512] conv_merge features (the trunk activations stored
 * by vn_policy_forward with out == NULL), lra [E][A+1] (one-hot last action, last reward;
 * NULL = zeros), mask [E] (0 resets the carried state: m * h_prev, m * c_prev; NULL = 1),
 * h_prev/c_prev [E][512] (NULL = zeros). Writes xcat [E][xcat], gates scratch [E][2048],
 * acts [E][2048] (i, f, g, o), c_out, h_out [E][512] — keep xcat/acts/c/h of every step of a
 * rollout (rows t*E + e) for vn_lstm_backward. */
#define VN_POLICY_LSTM 1
int vn_policy_create_ex(int frame_h, int frame_w, int num_actions, int flags, vn_policy** out);
int vn_policy_lstm_info(vn_policy* p, int64_t* info8);
int vn_lstm_forward_step(vn_policy* p, const float* params, int E, const float* x5, const float* lra,
                         const float* mask, const float* h_prev, const float* c_prev, float* xcat, float* gates,
                         float* acts, float* c_out, float* h_out, vn_stream_t stream);
/* Heads on n feature rows [n][512] -> out [n][8]. */
int vn_policy_heads(vn_policy* p, const float* params, const float* feat, int n, float* out, vn_stream_t stream);
int vn_lstm_workspace_floats(vn_policy* p, int T, int E, int64_t* floats);
/* BPTT within one rollout (the state entering it is a constant): writes the head and LSTM
 * gradients into grads and dL/d(conv_merge pre-activation) [T*E][512] into dz5_all. */
int vn_lstm_backward(vn_policy* p, const float* params, int T, int E, const float* dout, const float* h_all,
                     const float* xcat_all, const float* acts_all, const float* c_all, const float* c_init,
                     const float* mask_all, const float* x5_all, float* dz5_all, float* grads, float* workspace,
                     vn_stream_t stream);
/* vn_lstm_backward plus dh_extra [T][extra_envs][512]: another head's gradient w.r.t. h_t of
 * envs 0..extra_envs-1 (pixel control, vn_pc_backward), added to the policy heads'. */
int vn_lstm_backward_ex(vn_policy* p, const float* params, int T, int E, const float* dout, const float* h_all,
                        const float* xcat_all, const float* acts_all, const float* c_all, const float* c_init,
                        const float* mask_all, const float* x5_all, const float* dh_extra, int extra_envs,
                        float* dz5_all, float* grads, float* workspace, vn_stream_t stream);
/* Trunk gradients (conv1..conv_merge) of the n stored samples from dz5 [n][512]. */
int vn_policy_backward_trunk(vn_policy* p, const float* params, const vn_frames* frames, int n, float* acts,
                             int64_t act_capacity, const float* dz5, float* grads, float* workspace,
                             vn_stream_t stream);

/* ---- aux deconv heads: AuxiliaryBigGoalHouseModel (models/goal.py:144-189) and the
 * auxiliary deconv loss (experiments/ai2_auxiliary/trainer.py:9-55) ----
 * A policy created with VN_POLICY_AUX appends W1 [32][4][4][48], b1 [48] (the three heads'
 * ConvTranspose2d(32,16,4,2) side by side: depth 0-15, mask 16-31, goal mask 32-47) and
 * W2 [48][4][4][8], b2 [8] (ConvTranspose2d(16,C,4,2) per head, block diagonal: depth ->
 * channel 0, mask -> 1-3, goal mask -> 4-6, 7 padding). info8 = (W1, b1, W2, b2 offsets,
 * AH, AW = first deconv map, PH, PW = prediction map). Heads read conv_base's output (X4)
 * from the activation store of vn_policy_forward; a1 [n][AH][AW][48], pred [n][PH][PW][8]. */
#define VN_POLICY_AUX 2
/* BigHouseModel (models/bignet.py:26-75) instead of BigGoalHouseModel: image only (the goal
 * frames are ignored), Conv(3,32,k8,s4) ReLU, Conv(32,64,k4,s2) ReLU, Conv(64,32,k3) ReLU,
 * Linear(7*7*32, 512) ReLU (84x84 frames only, as the reference's Linear fixes), then the same
 * heads / recurrent core. Layer slots: conv1 [32][8][8][3], conv2 [64][4][4][32],
 * conv3 [32][3][3][64], (conv4 slot empty), conv_merge, head. */
#define VN_POLICY_BIGHOUSE 4
typedef struct vn_aux_targets {
  const float* table;           /* [rows][PH][PW][4] from vn_aux_target_table */
  const int32_t* image_rows;    /* [n] row of each sample's state (vn_frames.image_rows) */
  const int32_t* goal_rows;     /* [n] row of each sample's goal */
} vn_aux_targets;
int vn_policy_aux_info(vn_policy* p, int64_t* info8);
int vn_aux_workspace_floats(vn_policy* p, int64_t* floats);
int vn_aux_forward(vn_policy* p, const float* params, float* acts, int64_t act_capacity, int n, float* a1,
                   float* pred, float* workspace, vn_stream_t stream);
/* Per-state targets, built once per scene cache: table [n_rows][PH][PW][4] = (depth, seg0-2)
 * of avg_pool(centre crop(obs/255), 4) (compute_auxiliary_target, trainer.py:9-15) from the
 * depth [rows][H][W][1] and segmentation [rows][H][W][3] arenas (row-indexed like the frame
 * arena). */
int vn_aux_target_table(vn_policy* p, const uint8_t* depth, const uint8_t* segmentation, int height, int width,
                        int64_t n_rows, float* table, vn_stream_t stream);
/* dpred = weight * d(sum of per-head MSE)/dpred against the image row's (depth, seg) and the
 * goal row's seg targets; stats4[0..2] += per-head sums of squared errors. */
int vn_aux_loss_grad(vn_policy* p, const float* pred, int n, const vn_aux_targets* targets, float weight,
                     float* dpred, float* stats4, vn_stream_t stream);
/* vn_aux_forward + vn_aux_loss_grad in one pass: the second head layer computes each
 * prediction pixel and its loss gradient together (the trainer's path: the prediction is
 * never stored; pred is scratch, written only for maps too large for the fused kernel). */
int vn_aux_forward_loss_grad(vn_policy* p, const float* params, float* acts, int64_t act_capacity, int n,
                             float* a1, float* pred, const vn_aux_targets* targets, float weight,
                             float* dpred, float* stats4, float* workspace, vn_stream_t stream);
/* Head gradients into grads and dL/dX4 [n][h3][w3][32] (before conv_base's ReLU mask) into
 * dx4; consumes a1. */
int vn_aux_backward(vn_policy* p, const float* params, float* acts, int64_t act_capacity, int n, float* a1,
                    const float* dpred, float* grads, float* dx4, float* workspace, vn_stream_t stream);
/* ---- UNREAL heads: pixel control and reward prediction (models/goal.py:94-133,
 * models/bignet.py:77-111) ----
 * A policy created with VN_POLICY_UNREAL appends, 16-byte aligned (BigGoalHouseModel):
 *   pc_base W [2592][512] (rows in (y, x, c) order of the reference's (32, 9, 9) view), b [2592];
 *   pc W1 [32][4][4][64], b1 [64]: pc_value's ConvTranspose2d(32,32,4,2) -> channels 0-31,
 *     pc_action's -> 32-63;
 *   pc W2 [64][4][4][8], b2 [8]: block diagonal, pc_value's ConvTranspose2d(32,A,4,2) ->
 *     channels 0..A-1 from rows 0-31, pc_action's ConvTranspose2d(32,1,4,2) -> channel A from
 *     rows 32-63, the rest padding;
 *   rp W [3][3 * FCIN] (FCIN = h3 * w3 * 32; the three frames' conv_base maps, NHWC each:
 *     the reference's Linear(9*9*32*3, 3) at 174x174), b [4] (3 + pad).
 * With VN_POLICY_BIGHOUSE (BigHouseModel: one ConvTranspose2d(32, C, 4, 2) + ReLU per branch):
 *   pc_base W, b as above; pc W1 [32][4][4][8], b1 [8]: pc_value's ConvTranspose2d(32,A,4,2)
 *     -> channels 0..A-1, pc_action's ConvTranspose2d(32,1,4,2) -> channel A, the rest padding;
 *   no second layer (W2, b2 empty: their offsets equal rp W's); rp W [3][3 * 1568] (the
 *     reference's Linear(9*9*32*3, 3) fits 100x100 frames only: in_features derived), b [4].
 *   The pixel-control map is 20x20 (p2 [n][20][20][8], q [n][20][20][A]); a1 is unused (NULL ok);
 *   conv_base's output is X3, whose gradient vn_policy_backward_ex takes as dx4_extra.
 * info8 = (pc_base W, pc_base b, W1, b1, W2, b2, rp W, rp b offsets). */
#define VN_POLICY_UNREAL 8
int vn_policy_unreal_info(vn_policy* p, int64_t* info8);
int vn_pc_workspace_floats(vn_policy* p, int64_t* floats);
/* pixel_control (goal.py:131-137; bignet.py:105-111 with VN_POLICY_BIGHOUSE: a1 unused, p2
 * [n][20][20][8], q [n][20][20][A]) on feature rows h [n][512] (the LSTM outputs): writes
 * pcb [n][9][9][32], a1 [n][20][20][64], p2 [n][42][42][8] (kept for the backward) and
 * q [n][42][42][A] = (pc_value + pc_action) - mean_c(pc_action) (q may be NULL: not formed). */
int vn_pc_forward(vn_policy* p, const float* params, const float* h, int n, float* pcb, float* a1, float* p2,
                  float* q, float* workspace, vn_stream_t stream);
/* From dL/dq [n][42][42][A] (or dq == NULL: p2 already holds dL/dp2, as
 * vn_unreal_pc_loss_grad leaves it): the pixel-control parameter gradients into grads
 * (overwritten) and dL/dh [n][512] into dh (stored, or added to dh when accumulate != 0).
 * Consumes pcb, a1 and p2 (overwritten by their gradients). */
int vn_pc_backward(vn_policy* p, const float* params, const float* h, int n, float* pcb, float* a1, float* p2,
                   const float* dq, float* grads, float* dh, int accumulate, float* workspace, vn_stream_t stream);
/* reward_prediction (goal.py:121-129): out [n][4] = logits of x [n][3 * FCIN] (column 3 unused). */
int vn_rp_forward(vn_policy* p, const float* params, const float* x, int n, float* out, vn_stream_t stream);
/* rp gradients into grads (overwritten) from dL/dout [n][4] (column 3 ignored); dx [n][3 * FCIN]
 * (may be NULL) = dout x W. workspace: vn_pc_workspace_floats. */
int vn_rp_backward(vn_policy* p, const float* params, const float* x, int n, const float* dout, float* grads,
                   float* dx, float* workspace, vn_stream_t stream);
/* ---- UNREAL losses of the trainer (deep_rl's UnrealTrainer, absent: parity unpinned; the
 * published algorithm, csrc/vn_unreal_loss.hip, weights experiments/thor_cached_auxiliary.py:39-41) ----
 * Sequences are the first S envs of a rollout of T steps x E envs (rows t*E + e).
 * Pixel control: p2 [(T+1)*S][42][42][8] from vn_pc_forward on rows t*S + e (row T*S + e: the
 * bootstrap observation), q = (v + a) - a formed from it; pseudo-reward r_t = mean over each
 * 4x4 cell and 3 channels of |obs_{t+1} - obs_t| / 255 on the centre 168x168 crop of the u8
 * image frames (arena rows rows_img[t*E + e], rows_last[e] for obs_T); R_T = max_a q_T,
 * R_t = r_t + gamma (1 - done_t) R_{t+1} with r_t = 0 on a done step (the next frame is the
 * auto-reset frame of the next episode: recorded deviation); p2 is overwritten by dL/dp2 of weight *
 * mean((q_t[a_t] - R_t)^2) (under the value ReLU; 0 on the bootstrap rows), ready for
 * vn_pc_backward with dq == NULL; stats[0] += sum of squared errors. */
int vn_unreal_pc_loss_grad(float* p2, const int32_t* actions, const uint8_t* dones, const uint8_t* arena,
                           int64_t frame_bytes, int height, int width, const int32_t* rows_img,
                           const int32_t* rows_last, int T, int E, int S, int num_actions, float gamma, float weight,
                           float* stats, vn_stream_t stream);
/* The same on a cells x cells map: 42 (above) or 20 (BigHouseModel's p2 [(T+1)*S][20][20][8],
 * the centre 80x80 crop of 84x84 frames). */
int vn_unreal_pc_loss_grad_ex(float* p2, int cells, const int32_t* actions, const uint8_t* dones,
                              const uint8_t* arena, int64_t frame_bytes, int height, int width,
                              const int32_t* rows_img, const int32_t* rows_last, int T, int E, int S, int num_actions,
                              float gamma, float weight, float* stats, vn_stream_t stream);
/* Reward prediction: logits [(T-2)*S][4] of samples j = (ts-2)*S + e (frames ts-2..ts of env
 * e); class of rewards[ts][e]: 0 (r = 0), 1 (r > 0), 2 (r < 0); samples with a done at ts-2
 * or ts-1 are skipped. dlogits = weight * d mean CE / dlogits; stats2 = (mean CE, count). */
int vn_unreal_rp_loss_grad(const float* logits, const float* rewards, const uint8_t* dones, int T, int E, int S,
                           float weight, float* dlogits, float* stats2, vn_stream_t stream);
/* The same loss on explicit labels: label[j] = 0 / 1 / 2 is sample j's class, any other value
 * (-1 by convention) leaves it unused (dlogits row 0, not counted). Same thread mapping and
 * reduction order as vn_unreal_rp_loss_grad: equal logits under equivalent labels give equal
 * bits. stats2 = (mean CE over the used samples, used count). VN_EINVAL: a NULL buffer, n <= 0. */
int vn_unreal_rp_loss_grad_labels(const float* logits /* [n][4] */, const int32_t* label /* [n], -1 = unused */,
                                  int n, float weight, float* dlogits, float* stats2, vn_stream_t stream);

/* Reward-skewed reward-prediction draw from the replay ring (UNREAL's P(r != 0) = skew; DESIGN.md
 * "Reward-skewed reward prediction"). The ring is the trainer's: the first S envs' record of
 * every stored rollout and vn_replay_push_draw's meta, all read on the device.
 *
 * Candidates: windows (r, ts, e), r < min(meta4[1], capacity), 2 <= ts < T, e < S, with
 * dones[r][ts-2][e] == 0 and dones[r][ts-1][e] == 0; index i = (r (T-2) + (ts-2)) S + e. Q0 =
 * the candidates with rewards[r][ts][e] == 0 (-0.0 included), Q1 = the rest, both ordered by i.
 * Draw j: R = Philox4x32-10((j, c_lo, c_hi, STREAM_RP = 6), key = seed), c = meta4[2];
 * k = (R.x < (uint64)(skew * 2^32)) ? 1 : 0; an empty Qk gives k = 1 - k; both empty: the draw
 * is void (label = src = -1, all six rows 0). Else idx = ((R.y 2^32 + R.z) |Qk|) >> 64 and the
 * sample is Qk's idx-th element: rows_img[j][m] = rows[r][0][(ts-2+m) S + e], rows_goal[j][m] =
 * rows[r][1][...], m = 0..2; label = 0 (reward == 0), 1 (> 0), 2 (< 0); src = i. With replacement.
 * stats4 is written: [|Q0|, |Q1|, draws with label > 0, non-void draws]. The ring and meta are only
 * read; no host value varies per call and nothing synchronises, so a captured graph replays it.
 * One launch of one workgroup; capacity * (T - 2) * S <= VN_RP_SAMPLE_MAX_CANDIDATES.
 * VN_EINVAL, nothing written: a NULL pointer other than src, count <= 0, T < 3, S < 1,
 * capacity < 1, skew outside [0, 1], more candidates than the limit. */
#define VN_RP_SAMPLE_MAX_CANDIDATES 1048576
typedef struct vn_rp_ring {
  const float* rewards;  /* [capacity][T][S] */
  const uint8_t* dones;  /* [capacity][T][S] */
  const int32_t* rows;   /* [capacity][2][(T+1)*S]: image rows, then goal rows; row t*S + e, t = T the bootstrap */
  const int64_t* meta4;  /* vn_replay_push_draw's meta: [1] filled slots, [2] draw counter */
  int32_t capacity, T, S;
} vn_rp_ring;
int vn_unreal_rp_sample(const vn_rp_ring* ring, int count, double skew, uint64_t seed,
                        int32_t* rows_img /* [count][3] */, int32_t* rows_goal /* [count][3] */,
                        int32_t* label /* [count] */, int32_t* src /* [count], may be NULL */, int32_t* stats4,
                        vn_stream_t stream);
/* dx [(T-2)*S][3][fcin] (vn_rp_backward's input gradient) onto dx4 rows t*E + e, e < S
 * (stored, or added when accumulate != 0; other rows untouched). */
int vn_unreal_rp_scatter(const float* dx, int T, int E, int S, int fcin, float* dx4, int accumulate,
                         vn_stream_t stream);
/* The losses' inputs in one launch: h_pc [(T+1)*S][512] = h_all rows t*E + e (t < T, e < S)
 * then boot_h rows e < S; rp_x [(T-2)*S][3][fcin] (may be NULL) slot k of sample t*S + e =
 * x4 row (t+k)*E + e (conv_base maps of frames t..t+2). h_pc == NULL (h_all / boot_h unused) gathers
 * only rp_x. */
int vn_unreal_gather(const float* h_all, const float* boot_h, const float* x4, int T, int E, int S, int fcin,
                     float* h_pc, float* rp_x, vn_stream_t stream);
/* Value replay on rows t*E + e, e < S: dout[.][A] += weight * d mean((V - R)^2) / dV;
 * stats[0] += sum of squared errors. */
int vn_unreal_vr_grad(const float* out, const float* returns, int T, int E, int S, int num_actions, float weight,
                      float* dout, float* stats, vn_stream_t stream);

/* General backward: from dL/d(out) [n][8] (dz5 == NULL) or from dz5 [n][512] (recurrent
 * policies, heads and LSTM done by vn_lstm_backward); dx4_extra [n][h3][w3][32] (aux heads,
 * may be NULL) is added to conv_base's output gradient under its ReLU mask. */
int vn_policy_backward_ex(vn_policy* p, const float* params, const vn_frames* frames, int n, float* acts,
                          int64_t act_capacity, const float* dout, const float* dz5, const float* dx4_extra,
                          float* grads, float* workspace, vn_stream_t stream);

/* ---- goal-frame deduplication: shared_base on the goal frame once per episode ----
 * BigGoalHouseModel runs shared_base on the goal frame at every step (models/goal.py:88), but
 * an env's goal frame does not change within an episode. A goal run is a sample whose goal is
 * new — the first step of a rollout, or the step after a done (the env auto-reset) — followed
 * by the same env's later steps up to its next done. With goal runs the policy computes conv1 /
 * conv2 of a goal frame only at the run's first sample, conv_base reads every sample's goal
 * map from its run start, and the backward sums a run's goal-map gradients before conv2's
 * weight / input gradient and conv1's weight gradient: the same outputs (bitwise: the
 * kernels are batch-independent) and the same gradients up to summation order. Samples are
 * time-major (t*E + e). */
typedef struct vn_goal_runs {
  const int32_t* goal_list;   /* samples (of the call) that start a goal run, ascending */
  const int32_t* goal_count;  /* device scalar: entries of goal_list */
  const int32_t* goal_delta;  /* [n] offset (<= 0, in samples) to the sample holding this sample's goal maps */
  const int32_t* run_length;  /* backward: [n] steps of the run starting at each listed sample */
  int num_envs;               /* backward: E, the sample stride between an env's steps */
} vn_goal_runs;
/* *supported = 1 when the policy takes goal runs for calls of n samples (84x84 / 174x174
 * uint8 frames, n > 16, no VN_*_GENERIC override set); else 0. */
int vn_policy_goal_runs_supported(vn_policy* p, int n, int* supported);
/* vn_policy_forward with the goal runs of this call's n samples (goals != NULL; an unsupported
 * configuration is an error, not a silent fallback). */
int vn_policy_forward_goals(vn_policy* p, const float* params, const vn_frames* frames, int n, float* acts,
                            int64_t act_capacity, int64_t act_offset, float* out, const vn_goal_runs* goals,
                            vn_stream_t stream);
/* vn_policy_backward_ex over samples whose forward ran with these goal runs (the goal maps
 * of non-start samples were never computed: a backward without the runs would read them). */
int vn_policy_backward_goals(vn_policy* p, const float* params, const vn_frames* frames, int n, float* acts,
                             int64_t act_capacity, const float* dout, const float* dz5, const float* dx4_extra,
                             float* grads, float* workspace, const vn_goal_runs* goals, vn_stream_t stream);
/* Rollout step t's goal runs (before its forward): new[e] = done_prev == NULL || done_prev[e]
 * (done_prev = step t - 1's dones; NULL at t = 0); delta[e] = new ? 0 : delta_prev[e] - E;
 * list = the envs with new goals, ascending; *count = their number. One workgroup. */
int vn_goal_runs_step(const uint8_t* done_prev, const int32_t* delta_prev, int E, int32_t* delta, int32_t* list,
                      int32_t* count, vn_stream_t stream);
/* The update's goal runs over the rollout's T*E samples (dones [T][E]): list = the run starts
 * ascending, run_length [T*E] at each start, *count. One workgroup. */
int vn_goal_runs_rollout(const uint8_t* dones, int T, int E, int32_t* list, int32_t* run_length, int32_t* count,
                         vn_stream_t stream);

/* ---- A2C (the deep_rl trainer contract; DESIGN.md "A2C contract") ---- */
int vn_policy_sample(const float* out, int n, int num_actions, uint64_t seed, uint64_t counter,
                     int32_t* actions, float* logp, float* entropy, float* value, vn_stream_t stream);
/* actions[i] = argmax over logits 0..A-1 of out [n][8]; on an exact tie the first (lowest)
 * maximal index wins, as numpy / torch argmax. Columns >= A are not read. */
int vn_policy_greedy(const float* out, int n, int num_actions, int32_t* actions, vn_stream_t stream);
int vn_a2c_returns(const float* rewards, const uint8_t* dones, const float* bootstrap_out, int T, int E,
                   int num_actions, float gamma, float* returns, vn_stream_t stream);
/* vn_a2c_returns with geodesic reward shaping and GAE(lambda) (DESIGN.md "Reward shaping and
 * GAE"), one launch of the same shape. dist [T][2][E] int32: per step the distance before and
 * after it (vn_set_nav_progress_outputs), may be NULL. out [T*E][8]: the rollout's head outputs,
 * value in column num_actions; read only when lambda != 1 and may be NULL otherwise.
 *   w  = weight when anneal_steps <= 0, else weight * max(0, 1 - *steps_dev / anneal_steps) in
 *        fp64 rounded once to fp32, read on the device by the launch (a captured update anneals);
 *   F  = w (float(before) - gamma_phi float(after)) where both are >= 0, else 0;
 *   r' = r + F; where dist == NULL or w == 0 nothing is added and r' is r by bits (-0.0 stays);
 *   lambda == 1: R_t = r'_t + gamma R_{t+1} (1 - done_t), vn_a2c_returns' expression: with
 *        dist == NULL or w == 0 the result is vn_a2c_returns' bit for bit;
 *   lambda != 1: delta_t = r'_t + gamma V_{t+1} (1 - done_t) - V_t (V_T = the bootstrap),
 *        G_t = delta_t + gamma lambda (1 - done_t) G_{t+1}, G_T = 0, returns_t = G_t + V_t: the
 *        lambda-return, so vn_a2c_loss_grad*'s returns - V is the GAE advantage.
 * stats3_dev, int64 on the device, zeroed by the call: with dist, the sums of before and of
 * after over the steps where both are >= 0 and the number of the other steps (integer atomics:
 * exact and order-independent); the mean shaping term is w (sum_b - gamma_phi sum_a) / (T E).
 * VN_EINVAL, nothing written: a NULL rewards / dones / bootstrap_out / returns / stats3_dev,
 * out NULL with lambda != 1, T <= 0, E <= 0, num_actions outside 1..7, lambda outside [0, 1],
 * anneal_steps > 0 without steps_dev. */
int vn_a2c_returns_ex(const float* rewards, const uint8_t* dones, const float* bootstrap_out, const float* out,
                      const int32_t* dist, int T, int E, int num_actions, float gamma, float lambda, float weight,
                      float gamma_phi, const int64_t* steps_dev, int64_t anneal_steps, float* returns,
                      int64_t* stats3_dev, vn_stream_t stream);
/* The novelty bonus of a rollout (DESIGN.md "Visit counts and novelty bonus"), one launch.
 * rewards [T][E] f32 (never written), cell [T][E] int32 and first [T][E] uint8 (the histories
 * of vn_set_visit_outputs), count [C] uint32 (vn_visit_cells) as it stands at the launch, i.e.
 * at the end of the rollout. With wc = w_count and wf = w_first when anneal_steps <= 0, else
 * each times max(0, 1 - *steps_dev / anneal_steps) in fp64 rounded once to fp32, read on the
 * device by the launch (a captured update anneals), per element, N = count[cell]:
 *   b = wc / sqrt(float(N)), 0 where cell < 0, cell >= C or N == 0;
 *   f = wf where first, else 0;
 *   rewards_out = r + (b + f);
 * every operation one correctly rounded fp32 operation (a -0.0 reward with b = f = 0 becomes
 * +0.0, IEEE's sum). stats4 [4] f32 on the device = (sum of b + f, number of first visits,
 * sum of 1 / sqrt(float(N)) over the elements with N > 0, wc): fp64 sums in a fixed order
 * rounded once, the same bits from the same inputs. rewards_out must not overlap rewards.
 * VN_EINVAL, nothing written: a NULL rewards / cell /
 * first / count / rewards_out / stats4, C < 0, T <= 0, E <= 0, anneal_steps > 0 without
 * steps_dev. */
int vn_a2c_novelty_rewards(const float* rewards, const int32_t* cell, const uint8_t* first, const uint32_t* count,
                           int64_t C, int T, int E, float w_count, float w_first, const int64_t* steps_dev,
                           int64_t anneal_steps, float* rewards_out, float* stats4, vn_stream_t stream);
int vn_a2c_loss_grad(const float* out, const int32_t* actions, const float* returns, int n,
                     int num_actions, float value_coef, float entropy_coef, float* dout,
                     float* stats4, vn_stream_t stream);
/* vn_a2c_loss_grad with the shortest-path expert term (DESIGN.md "Expert loss from the
 * navigation tables"), one launch of the same shape. expert_mask [n] uint8: per sample the
 * optimal_mask of the state it observed; M = its bits below num_actions, M == 0 = no label
 * (the sample adds nothing). With p, logp, H, adv as vn_a2c_loss_grad computes them and
 * q = sum_{a in M} p_a (log q formed from the log-probabilities, finite and accurate however
 * little mass the mask holds):
 *   L = vc mean(A^2) - pg mean(A logp_a) - ec mean(H) - w mean([M != 0] log q)
 *   dout[i][j] = (pg (-adv (ind - p_j)) + ec p_j (logp_j + H)) / n + w / n (p_j - [j in M] exp(logp_j - log q))
 * the value column and columns > num_actions as vn_a2c_loss_grad. w = expert_weight when
 * anneal_steps <= 0, else expert_weight * max(0, 1 - *steps_dev / anneal_steps) in fp64 rounded
 * once to fp32; steps_dev is read on the device by the launch, so a captured update anneals.
 * stats4 = vn_a2c_loss_grad's (the policy term unscaled by pg). expert_stats4 = [sum of -log q
 * over the samples with M != 0, how many of them sampled an action in M, their number, w].
 * Both are zeroed by the call. With pg_coef == 1 and w == 0 or every M == 0, dout equals
 * vn_a2c_loss_grad's bit for bit. VN_EINVAL, nothing written: a NULL buffer (steps_dev may be
 * NULL when anneal_steps <= 0), n <= 0, num_actions outside 1..7. */
int vn_a2c_loss_grad_expert(const float* out, const int32_t* actions, const float* returns,
                            const uint8_t* expert_mask, int n, int num_actions, float value_coef,
                            float entropy_coef, float pg_coef, float expert_weight, const int64_t* steps_dev,
                            int64_t anneal_steps, float* dout, float* stats4, float* expert_stats4,
                            vn_stream_t stream);
/* Rollout bookkeeping after env step t (one launch): the next step's recurrent inputs —
 * last action one-hot and last reward times the episode mask m = 1 - done, and m itself
 * (UnrealEnvBaseWrapper's extra input, models/goal.py:63-64; mask rule of MaskedRNN,
 * unpinned) into lra_next [E][A+1] / mask_next [E] — prev_* carries, and the finished
 * episodes' (count, return sum, length sum) added to episode_stats3 in a fixed order
 * (deep_rl RewardCollector, experiments/thor_cached_auxiliary.py:59-64). Pointers other
 * than the inputs and episode_stats3 may be NULL. */
int vn_a2c_step_post(const int32_t* actions, const float* rewards, const uint8_t* dones,
                     const float* ep_return, const int32_t* ep_length, int E, int num_actions,
                     int64_t* prev_action, float* prev_reward, float* prev_mask, float* lra_next,
                     float* mask_next, float* episode_stats3, vn_stream_t stream);
/* stats3 = the fixed-order sums over envs of episode_stats_env [3][E] (vn_step_a2c's
 * accumulators: finished-episode count, return sum, length sum), which are then zeroed. */
int vn_a2c_episode_stats(float* episode_stats_env, int E, float* stats3, vn_stream_t stream);
/* scalars2 = (total norm of scale*grads, clip coefficient) computed on the device. */
int vn_grad_norm(const float* grads, int64_t n, float scale, float max_norm, double* partial_512,
                 float* scalars2, vn_stream_t stream);
int vn_rmsprop_step(float* params, const float* grads, float* square_avg, int64_t n, float scale,
                    const float* scalars2, float lr, float alpha, float eps, vn_stream_t stream);
/* vn_grad_norm with up to two gradient addends joined first: grads[i] += add_j[i] for i in
 * [lo_j, hi_j) (add_j NULL = none), written back to grads, then the norm of scale*grads —
 * the side passes' sums (a replayed aux batch's trunk gradient, the replayed UNREAL pass's
 * trunk / heads / LSTM gradient) without a launch of their own; bitwise equal to the adds
 * followed by vn_grad_norm. */
int vn_grad_norm_join(float* grads, int64_t n, const float* add0, int64_t lo0, int64_t hi0, const float* add1,
                      int64_t lo1, int64_t hi1, float scale, float max_norm, double* partial_512,
                      float* scalars2, vn_stream_t stream);

/* The replay ring on the device (deep_rl's replay buffer behind AuxiliaryTrainer's
 * self.replay.sample_sequence(), experiments/ai2_auxiliary/trainer.py:27-31; deep_rl is
 * absent, so capacity and sequence shape are parity unpinned). One call pushes a rollout's
 * record into slot meta4[0] and draws this update's slot among the filled ones — no host
 * value, so an update with replay sources is captured in a hipGraph (A2CTrainer(cuda_graph=True)).
 * meta4 = int64 [next slot, filled slots, draw counter, last drawn slot]. Segment j copies
 * rows x cols elements of elem_bytes (1 or 4) from src (row r at src + r*src_ld elements) to
 * ring + slot*slot_elems (packed rows) and, when cur != NULL, the drawn slot's elements to cur
 * (packed). The draw: k = uniform_below(Philox4x32-10(ctr_lo, ctr_hi, 0, STREAM_REPLAY = 4)
 * under key seed, min(filled + 1, capacity)); then meta4 = [(slot + 1) % capacity,
 * min(filled + 1, capacity), ctr + 1, k]. At most 16 segments. */
typedef struct vn_replay_seg {
  const void* src;
  int64_t src_ld;
  void* ring;
  void* cur;
  int64_t slot_elems;
  int32_t rows, cols, elem_bytes, pad_;
} vn_replay_seg;
int vn_replay_push_draw(const vn_replay_seg* segs, int nseg, int64_t* meta4, int capacity, uint64_t seed,
                        vn_stream_t stream);

/* Device-side schedule, so that one update has no per-call host arguments and can be
 * captured once in a hipGraph and replayed (A2CTrainer(cuda_graph=True)):
 *   vn_a2c_schedule: state3 = int64 [next counter base, env-steps so far, this update's
 *     counter base]; this update's base = state3[0] (then += T), lr_out = lr0 * (1 -
 *     min(state3[1] / max_time_steps, 1)) computed in double (LinearSchedule,
 *     experiments/thor_cached_auxiliary.py:37), then state3[1] += steps_per_update;
 *   vn_policy_sample_dev: vn_policy_sample with counter = *counter_base_dev + offset;
 *   vn_rmsprop_step_dev: vn_rmsprop_step with lr read from lr_dev.
 * Bit-identical to the host-argument forms fed the same values. */
int vn_a2c_schedule(int64_t* state3, float* lr_out, double lr0, double max_time_steps,
                    int64_t steps_per_update, int T, vn_stream_t stream);
/* First launch of a rollout (replaces vn_a2c_schedule + the step-0 input copies):
 * vn_a2c_schedule's update of state3 / lr_out, img/goal_row_dst[e] = *_src[e] (step 0's
 * frame rows) and, when mask0 != NULL, mask0[e] = prev_mask[e] and lra0 [E][A+1] =
 * [one_hot(prev_action[e]) | prev_reward[e]] * prev_mask[e] (vn_a2c_step_post's form). */
int vn_a2c_rollout_begin(int64_t* state3, float* lr_out, double lr0, double max_time_steps,
                         int64_t steps_per_update, int T, const int32_t* img_row_src,
                         const int32_t* goal_row_src, int32_t* img_row_dst, int32_t* goal_row_dst, int E,
                         const int64_t* prev_action, const float* prev_reward, const float* prev_mask,
                         int num_actions, float* mask0, float* lra0, vn_stream_t stream);
/* An update's metric vector out9 = [stats4 * inv_n, scalars2[0] (grad norm), aux loss =
 * sum over the three heads of aux3[h] / aux_numel3[h] (0 when aux3 == NULL), episode_stats3]
 * in one launch. */
int vn_a2c_metrics(const float* stats4, float inv_n, const float* scalars2, const float* aux3,
                   const float* aux_numel3, const float* episode_stats3, float* out9, vn_stream_t stream);
/* vn_a2c_metrics + the UNREAL loss means: out[9..11] = [unreal4[0] * norm3[0] (pc),
 * unreal4[1] * norm3[1] (rp), unreal4[3] * norm3[2] (vr)] when unreal4 != NULL (out holds 12). */
int vn_a2c_metrics_ex(const float* stats4, float inv_n, const float* scalars2, const float* aux3,
                      const float* aux_numel3, const float* episode_stats3, const float* unreal4,
                      const float* unreal_norm3, float* out, vn_stream_t stream);
int vn_policy_sample_dev(const float* out, int n, int num_actions, uint64_t seed,
                         const int64_t* counter_base_dev, uint64_t counter_offset, int32_t* actions,
                         float* logp, float* entropy, float* value, vn_stream_t stream);
int vn_rmsprop_step_dev(float* params, const float* grads, float* square_avg, int64_t n, float scale,
                        const float* scalars2, const float* lr_dev, float alpha, float eps,
                        vn_stream_t stream);

/* PPO epochs over a stored rollout (DESIGN.md "PPO epochs", csrc/vn_ppo.hip). out / out_old /
 * dout are [n][8] rows as in vn_a2c_loss_grad: logits in columns 0..A-1, the value in column A;
 * out_old is the behaviour policy's copy of the rollout's out, fixed for the whole update.
 *
 * vn_ppo_adv_stats: stats2_dev [2] f32 on the device = [mean, 1 / (std + eps)] of
 * adv_i = returns[i] - out_old[i][A], std the population standard deviation (divide by n; n == 1
 * gives std = 0). One launch: fp64 sums in a fixed order, the mean first, then the squares centred
 * on it, each result rounded once to fp32; no atomics, so the same input gives the same bits.
 * VN_EINVAL, nothing written: a NULL buffer, n <= 0, num_actions outside 1..7, eps <= 0. */
int vn_ppo_adv_stats(const float* returns, const float* out_old, int n, int num_actions, float eps,
                     float* stats2_dev, vn_stream_t stream);
/* The clipped-surrogate loss gradient of one epoch, one launch of vn_a2c_loss_grad's shape. With
 * p, logp, H of out and logp_old of out_old as vn_a2c_loss_grad computes them, a the action,
 * R = returns[i], V = out[i][A], V_old = out_old[i][A], c = clip, cv = value_clip:
 *   d = logp_a - logp_old_a, r = expf(d);
 *   adv = R - V_old; A^ = (adv - mean) rstd with [mean, rstd] = adv_stats2_dev read on the
 *   device (vn_ppo_adv_stats' output), A^ = adv when adv_stats2_dev == NULL;
 *   s1 = r A^, s2 = clamp(r, 1 - c, 1 + c) A^; the surrogate is min(s1, s2), and its gradient
 *   flows where s1 <= s2 (a tie included): g = -A^ r there, else 0;
 *   dout[i][j] = (g (ind_j - p_j) + ec p_j (logp_j + H)) / n for j < A;
 *   value head, e1 = R - V: with cv <= 0, lv = e1^2 and dout[i][A] = vc (-2 e1) / n (the A2C
 *   convention); else Vc = V_old + clamp(V - V_old, -cv, cv), e2 = R - Vc, lv = max(e1^2, e2^2)
 *   and dout[i][A] is as above where e1^2 >= e2^2, else 0;
 *   columns above A are 0.
 * stats4 = sums of (lv, -min(s1, s2), H, R), the layout vn_a2c_metrics_ex reads. ppo_stats4 =
 * sums of (expm1f(d) - d, [|r - 1| > c], r, [e2^2 > e1^2]): the first is the k3 estimate of
 * KL(old || new), accurate near r = 1. Both are zeroed by the call. When out_old is out itself
 * (neither is written) r is exactly 1 and the policy and value columns are vn_a2c_loss_grad's
 * expression. VN_EINVAL, nothing written: a NULL buffer (adv_stats2_dev may be NULL), n <= 0,
 * num_actions outside 1..7, clip <= 0. */
int vn_ppo_loss_grad(const float* out, const float* out_old, const int32_t* actions, const float* returns,
                     const float* adv_stats2_dev, int n, int num_actions, float clip, float value_clip,
                     float value_coef, float entropy_coef, float* dout, float* stats4, float* ppo_stats4,
                     vn_stream_t stream);
/* vn_ppo_loss_grad without the clearing: stats4 and ppo_stats4 are added to, so the launches of one
 * epoch's minibatches leave the epoch's sums (the caller clears them before the first). dout and
 * the 1 / n of the means are this call's n samples' own. Same arguments, same refusals. */
int vn_ppo_loss_grad_acc(const float* out, const float* out_old, const int32_t* actions, const float* returns,
                         const float* adv_stats2_dev, int n, int num_actions, float clip, float value_clip,
                         float value_coef, float entropy_coef, float* dout, float* stats4, float* ppo_stats4,
                         vn_stream_t stream);

/* PPO minibatches (DESIGN.md "PPO minibatches", csrc/vn_ppo_minibatch.hip): an epoch's shuffled
 * split of the envs and the compaction of one minibatch's sub-rollout, both on the device.
 *
 * vn_ppo_env_permutation: perm [num_envs] int32 = the stable argsort of the envs' keys, ties by
 * env index (numpy's argsort(keys, kind="stable") exactly). Key of env e in epoch k: the first
 * output word of Philox4x32-10 on the counter (k num_envs + e, ctr_lo, ctr_hi, 7 = STREAM_PPO)
 * under the key (seed_lo, seed_hi), masked to its low key_bits bits (32 = the whole word; fewer
 * force ties); ctr = *counter_dev, an int64 read on the device (the update's counter base of
 * vn_a2c_rollout_begin's schedule). One launch of ceil(num_envs / 256) workgroups, rank by
 * counting over keys staged in LDS VN_PPO_PERM_TILE at a time: no atomics, every slot written
 * once, the same bits on every run. VN_EINVAL, nothing written: a NULL pointer, epoch < 0,
 * num_envs < 1, key_bits outside 1..32, (epoch + 1) num_envs >= 2^32. */
#define VN_PPO_PERM_TILE 1024
int vn_ppo_env_permutation(uint64_t seed, const int64_t* counter_dev, int epoch, int num_envs, int key_bits,
                           int32_t* perm, vn_stream_t stream);
/* The buffers of a rollout in time-major layout, row t E + e: the [T, E] source, or the compact
 * [T, count] destination (row t count + j). */
typedef struct vn_ppo_rollout {
  int32_t* rows_img;    /* [T E] frame rows (vn_frames.image_rows) */
  int32_t* rows_goal;   /* [T E] */
  int32_t* actions;     /* [T E] */
  float* returns;       /* [T E] */
  float* out_old;       /* [T E][8] the behaviour policy's head outputs, 16-byte aligned */
  uint8_t* dones;       /* [T E] */
  float* masks;         /* [T E] LSTM episode masks (NULL with lra, h0, c0: a feed-forward policy) */
  float* lra;           /* [T E][A + 1] last action one-hot | last reward */
  float* h0;            /* [E][512] the state entering the rollout, 16-byte aligned */
  float* c0;            /* [E][512] */
  int32_t* goal_delta;  /* [T E] vn_goal_runs.goal_delta (may be NULL): scaled by count / E on the way */
} vn_ppo_rollout;
/* dst row t count + j = src row t num_envs + envs[j] for every buffer above (h0 / c0: row j =
 * row envs[j]), envs [count] int32 on the device (a slice of vn_ppo_env_permutation's perm).
 * goal_delta, a multiple of the sample stride, is rescaled to the destination's stride. One
 * launch; every destination element is written once by a plain vector store, rows past T count
 * are not touched; an envs[j] outside [0, num_envs) writes nothing for that env. VN_EINVAL,
 * nothing written: a NULL struct or envs, a NULL rows / actions / returns / out_old / dones on
 * either side, some but not all of dst's masks / lra / h0 / c0, a dst buffer whose src is NULL,
 * count outside 1..num_envs, T < 1, num_actions outside 1..7, a misaligned out_old / h0 / c0. */
int vn_ppo_minibatch_gather(const vn_ppo_rollout* src, const vn_ppo_rollout* dst, const int32_t* envs, int count,
                            int T, int num_envs, int num_actions, vn_stream_t stream);

/* torch's Adam without weight decay or amsgrad on the flat buffers, vn_rmsprop_step_dev's shape:
 *   g = grads (scalars2[1] scale); m = beta1 m + (1 - beta1) g; v = beta2 v + (1 - beta2) g^2;
 *   t = *step_dev + 1; bc1 = 1 - beta1^t and bc2 = 1 - beta2^t formed in fp64 on the device;
 *   p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps), lr = *lr_dev.
 * lr and t are read on the device, so a captured update stays valid. step_dev (int64) advances by
 * one per call, in a launch of its own behind the step. VN_EINVAL, nothing written: a NULL
 * buffer, n <= 0. */
int vn_adam_step_dev(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float scale,
                     const float* scalars2, const float* lr_dev, int64_t* step_dev, float beta1, float beta2,
                     float eps, vn_stream_t stream);

/* PPO target KL (DESIGN.md "PPO target KL", csrc/vn_ppo_kl.hip): the early stop of an update's
 * epochs, decided and applied on the device so that the update stays one captured hipGraph.
 *
 * vn_ppo_kl_gate: gate_dev [2] int32 = [stopped, steps_allowed], kl_dev [2] f32 = [the KL of the
 * last check, the KL that stopped the update]. With gate_dev[0] != 0 on entry the launch writes
 * nothing (the stop is sticky until the caller zeroes the buffers). Otherwise
 *   kl = (1 / n) sum_i (expm1f(d_i) - d_i), d_i = logp_a - logp_old_a as vn_ppo_loss_grad forms it
 * (the k3 estimate behind ppo_stats4[0]), summed as vn_ppo_adv_stats sums: one launch of one
 * workgroup, fp64 sums in a fixed order, the mean rounded once to fp32, no atomics, so the same
 * input gives the same bits. kl_dev[0] = kl; then kl > kl_limit (strict) sets gate_dev[0] = 1 and
 * kl_dev[1] = kl, else gate_dev[1] += 1. out and out_old may be one buffer (kl is then exactly 0).
 * VN_EINVAL, nothing written: a NULL buffer, n <= 0, num_actions outside 1..7, kl_limit negative
 * or NaN. */
int vn_ppo_kl_gate(const float* out, const float* out_old, const int32_t* actions, int n, int num_actions,
                   float kl_limit, int32_t* gate_dev, float* kl_dev, vn_stream_t stream);
/* vn_adam_step_dev / vn_rmsprop_step_dev behind a flag read on the device: with *skip_dev == 0 the
 * same expressions and the same bits; with *skip_dev != 0 nothing is written, not the parameters,
 * not the moments or square_avg, and not Adam's step_dev (its advance launch reads the flag too).
 * VN_EINVAL, nothing written: a NULL buffer (skip_dev included), n <= 0. */
int vn_adam_step_gated(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float scale,
                       const float* scalars2, const float* lr_dev, int64_t* step_dev, float beta1, float beta2,
                       float eps, const int32_t* skip_dev, vn_stream_t stream);
int vn_rmsprop_step_gated(float* params, const float* grads, float* square_avg, int64_t n, float scale,
                          const float* scalars2, const float* lr_dev, float alpha, float eps, const int32_t* skip_dev,
                          vn_stream_t stream);

/* Copy the message of the calling thread's last error (NUL-terminated). */
int vn_last_error(char* buf, size_t len);
const char* vn_version(void);

/* Diagnostics: launch an empty kernel of `tag` (1..65535) workgroups of 64 lanes on the
 * stream. A kernel trace records its grid size, which marks where a test (or any phase of
 * a program) begins in a trace (tests/conftest.py, tools/test_kernel_map.py). */
int vn_trace_marker(int tag, vn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VNAV_H */
