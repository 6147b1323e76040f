"""A2C rollout/update loop on one GPU per process (RCCL all-reduce across processes).

Mirrors the deep_rl Trainer surface the reference drives (train.py:24-25,
experiments/thor_cached_auxiliary.py:26-56): hyper-parameters as attributes with the
reference's values (num_steps 20, gamma .99, RMSprop alpha .99 / eps 1e-5, grad-norm
clip 0.5, lr 7e-4 -> 0 linearly over max_time_steps), ``step()`` = one rollout of
num_steps on every local env + one update, ``run()`` loops to max_time_steps,
``create_env`` / ``create_model`` hooks. The loss is the standard A2C stated in
DESIGN.md ("A2C contract"; value/entropy coefficients are not visible in the
reference — deep-rl 0.2.9 is absent — so parity is unpinned at this level).

Everything per step is a device launch: policy forward on frames gathered zero-copy
from the scene cache by row index, categorical sampling, env step (index-only), then
returns, loss gradient, backward, one flat-buffer all-reduce, norm, clip + RMSprop. No
host synchronisation inside ``step(sync=False)``. The per-update values (sampling counter,
learning rate) come from a device-side schedule (``vn_a2c_rollout_begin``), so one update has no
per-call host arguments: with ``cuda_graph=True`` it is captured once in a hipGraph and
replayed (single process), which removes the per-launch host cost that dominates small
batches (the reference's own run is 4 envs x 20 steps, ~400 launches per update).

With a recurrent net (``recurrent=True``) each step also runs the LSTM core: the input is
[conv_merge features | one-hot last action | last reward] and the carried (h, c), both
zeroed where an episode starts (mask m_t = 1 - done_{t-1}); the update back-propagates
through the T steps of the rollout (truncated BPTT) and (h, c) carry on to the next.

With ``aux_weight > 0`` (AuxiliaryTrainer, experiments/ai2_auxiliary/trainer.py:21-55; its
default auxiliary_weight is 0.05, the logged thor-cached-auxiliary experiment sets 0.1 at
experiments/thor_cached_auxiliary.py:42) the update adds the deconv loss of AuxiliaryBigGoalHouseModel's
depth / segmentation / goal-segmentation heads against avg-pooled targets gathered from
the env's aux arena by row. The reference computes it on a sequence sampled from
UnrealTrainer's replay buffer (deep_rl, absent); here it uses the on-policy rollout batch
(documented deviation, parity unpinned at the trainer level).

With ``unreal=True`` (BigGoalHouseModel's pixel-control and reward-prediction heads,
models/goal.py:94-137; UnrealTrainer's losses with the weights pc 0.05, rp 1.0, vr 1.0 of
experiments/thor_cached_auxiliary.py:39-41) each update also runs, on the rollout sequences
of the first ``unreal_envs`` envs: pixel control (n-step Q-learning on the pixel change of
the image frames, gamma_pc 0.9, on the LSTM features, bootstrap from the last observation),
reward prediction (the sign class of the reward after three consecutive frames of one
episode, from their conv_base maps) and value replay (the critic against the n-step
returns). deep_rl draws these sequences from its replay buffer (absent): here they are the
on-policy sequences, and the loss formulas are the published algorithm's (parity unpinned,
csrc/vn_unreal_loss.hip, oracle/unreal.py).
"""
import ctypes
import os
import time

import numpy as np
import torch

from . import _lib, checkpoint, evaluation
from . import dist as vdist
from .metrics import metric_layout
from .policy import OUT_LD, AuxTargets, PolicyNet, frames_from_rows


# rows at or below which vn_policy_heads takes its skinny path (kSkinnyRows, csrc/vn_skinny.h):
# there the env-step launch computes the heads with the same sums (vn_a2c_step.head_weight)
_FUSED_HEADS_MAX_ENVS = 16
# eps of the PPO advantage normalisation (adv - mean) / (std + eps)
_PPO_ADV_EPS = 1e-8


class A2CTrainer:
    def __init__(self, env, net=None, params=None, num_steps=20, gamma=0.99, learning_rate=7e-4,
                 max_time_steps=2e6, rms_alpha=0.99, rms_epsilon=1e-5, max_gradient_norm=0.5,
                 value_coefficient=0.5, entropy_coefficient=0.01, seed=0, process_group=None, recurrent=False,
                 aux_weight=0.0, arch="goal", cuda_graph=False, aux_source="rollout", replay_size=8,
                 capture_collectives=False, allreduce_buckets=1, time_collectives=False, dedup_goals=None,
                 unreal=False, pc_weight=0.05, rp_weight=1.0, vr_weight=1.0, pc_gamma=0.9, unreal_envs=16,
                 unreal_source="rollout", nav_metrics=False, expert_weight=None, expert_anneal_steps=0,
                 pg_coefficient=1.0, geo_curriculum=None, shaping_weight=None, shaping_gamma=1.0,
                 shaping_anneal_steps=0, gae_lambda=1.0, rp_sampling="sequence", rp_batch=None, rp_skew=0.5,
                 novelty_weight=0.0, first_visit_weight=0.0, novelty_anneal_steps=0, ppo_clip=None, ppo_epochs=4,
                 ppo_value_clip=0.0, ppo_normalize_advantage=True, optimizer="rmsprop", adam_betas=(0.9, 0.999),
                 adam_epsilon=1e-5, ppo_target_kl=None, ppo_kl_host_stop=False, ppo_minibatches=1):
        self.env = env
        self.lib = _lib.load()
        # check before every replayed UNREAL pass that the side stream's buffers and gradient
        # block are disjoint from the main stream's (_check_side_stream_disjoint)
        self.debug_streams = bool(os.environ.get("VN_DEBUG_STREAMS"))
        self.device = env.device
        self.num_steps = int(num_steps)
        self.gamma = float(gamma)
        self.learning_rate = float(learning_rate)
        self.max_time_steps = float(max_time_steps)
        self.rms_alpha = float(rms_alpha)
        self.rms_epsilon = float(rms_epsilon)
        self.max_gradient_norm = float(max_gradient_norm)
        self.value_coefficient = float(value_coefficient)
        self.entropy_coefficient = float(entropy_coefficient)
        self.seed = int(seed)
        self.group = process_group
        self.world, self.rank = vdist.world_of(process_group)
        # ppo_clip (None = off): update() runs ppo_epochs epochs of the clipped surrogate over the
        # stored rollout instead of one A2C step (_ppo_update, DESIGN.md "PPO epochs"): full-batch
        # epochs, or with ppo_minibatches > 1 shuffled minibatches of whole envs.
        # Each combination refused here is out of scope, not impossible.
        self.ppo = ppo_clip is not None
        self.ppo_epochs = int(ppo_epochs)
        self.ppo_value_clip = float(ppo_value_clip)
        self.ppo_normalize_advantage = bool(ppo_normalize_advantage)
        self._on_ppo_epoch = None
        if self.ppo_epochs < 1:
            raise ValueError("ppo_epochs must be at least 1, got %r" % (ppo_epochs,))
        if self.ppo:
            self.ppo_clip = float(ppo_clip)
            if not self.ppo_clip > 0.0:
                raise ValueError("ppo_clip must be > 0, got %r" % (ppo_clip,))
            if self.world > 1:
                raise ValueError("ppo_clip does not run at world > 1 yet: the advantage statistics would need a "
                                 "cross-rank reduction")
            if unreal:
                raise ValueError("ppo_clip does not run with unreal=True yet: the UNREAL losses have no epoch loop")
            if aux_source == "replay":
                raise ValueError("ppo_clip does not run with aux_source='replay' yet: the replayed aux batch has its "
                                 "own trunk pass, which the epochs do not repeat")
            if expert_weight is not None:
                raise ValueError("ppo_clip does not run with expert_weight yet: the expert term lives in the A2C "
                                 "loss-gradient launch")
        # ppo_minibatches M (1 = off, the full-batch epochs above): every epoch draws one permutation
        # of the envs on the device and takes M optimiser steps, each on the whole sequences of about
        # E / M envs (_ppo_minibatch_epochs, DESIGN.md "PPO minibatches")
        self.ppo_minibatches = int(ppo_minibatches)
        self._on_ppo_minibatch = None
        if not 1 <= self.ppo_minibatches <= env.num_envs:
            raise ValueError("ppo_minibatches must lie in 1..num_envs = %d (a minibatch holds whole envs), got %r"
                             % (env.num_envs, ppo_minibatches))
        if self.ppo_minibatches > 1 and not self.ppo:
            raise ValueError("ppo_minibatches > 1 splits the epochs of a PPO update: it needs ppo_clip (the A2C "
                             "update takes one step per rollout and has nothing to split)")
        # ppo_target_kl (None = off): before every optimiser step of a PPO update the k3 estimate of
        # KL(old || new) over the step's own samples is formed on the device (vn_ppo_kl_gate), and
        # once it exceeds 1.5 * target (the rule of Stable-Baselines3 and Spinning Up) that step and
        # every later one of the update change nothing (DESIGN.md "PPO target KL"). The launches
        # still run, so the update stays one captured graph; ppo_kl_host_stop (eager only) reads the
        # flag after each check and leaves the loops instead, to the same bits.
        self.ppo_target_kl = None if ppo_target_kl is None else float(ppo_target_kl)
        self.ppo_kl_host_stop = bool(ppo_kl_host_stop)
        if self.ppo_target_kl is not None:
            if not self.ppo:
                raise ValueError("ppo_target_kl stops the epochs of a PPO update early: it needs ppo_clip (the A2C "
                                 "update takes one step per rollout and has nothing to stop)")
            if not self.ppo_target_kl > 0.0:  # NaN too
                raise ValueError("ppo_target_kl must be > 0, got %r" % (ppo_target_kl,))
            with np.errstate(over="ignore"):  # a target past fp32's range is a limit of inf: never stopped
                self._kl_limit = float(np.float32(1.5 * self.ppo_target_kl))
        if self.ppo_kl_host_stop:
            if self.ppo_target_kl is None:
                raise ValueError("ppo_kl_host_stop reads the stop flag of ppo_target_kl: it needs ppo_target_kl")
            if cuda_graph:
                raise ValueError("ppo_kl_host_stop runs host code between the epochs, which a captured hipGraph "
                                 "cannot replay: use cuda_graph=False")
        # optimizer: "rmsprop" (the reference's) or "adam" (torch's Adam, vn_adam_step_dev), with
        # plain A2C or PPO, at any world
        if optimizer not in ("rmsprop", "adam"):
            raise ValueError("optimizer must be 'rmsprop' or 'adam', got %r" % (optimizer,))
        self.optimizer = optimizer
        self.adam_betas = (float(adam_betas[0]), float(adam_betas[1]))
        self.adam_epsilon = float(adam_epsilon)
        if allreduce_buckets not in (1, 2):
            raise ValueError("allreduce_buckets must be 1 or 2")
        self.allreduce_buckets = int(allreduce_buckets)
        self.time_collectives = bool(time_collectives)
        if self.time_collectives and cuda_graph:
            raise ValueError("time_collectives records HIP events per update, which a captured hipGraph would replay "
                             "as fixed events: use one or the other")
        # exposed all-reduce time: the pending update's event pair and a running (sum, count)
        self._coll_pending = []
        self._coll_sum_ms, self._coll_count = 0.0, 0
        self._head_work = None
        self.aux_weight = float(aux_weight)
        self.net = net if net is not None else PolicyNet(env.frame_shape[:2], env.num_actions, self.device,
                                                         recurrent=recurrent, aux=self.aux_weight > 0, arch=arch,
                                                         unreal=unreal)
        self.recurrent = self.net.recurrent
        if self.aux_weight > 0 and (not self.net.aux or getattr(env, "aux_arena", None) is None):
            raise ValueError("aux_weight > 0 needs an aux policy (aux=True) and scenes with depth + segmentation")
        self.A = self.net.num_actions
        self.params = params if params is not None else self.net.init_params(self.seed)
        vdist.broadcast_params_(self.params, group=self.group)
        P = self.net.n_params
        E, T = env.num_envs, self.num_steps
        N = T * E
        kw = dict(device=self.device)
        self.grads = torch.zeros(P, dtype=torch.float32, **kw)
        self.square_avg = torch.zeros(P, dtype=torch.float32, **kw)
        if self.optimizer == "adam":
            self.exp_avg = torch.zeros(P, dtype=torch.float32, **kw)
            self.exp_avg_sq = torch.zeros(P, dtype=torch.float32, **kw)
            self.adam_step = torch.zeros(1, dtype=torch.int64, **kw)  # updates taken, read on the device
        self.acts = self.net.new_acts(N)
        self.boot_acts = self.net.new_acts(E)
        self.out = torch.zeros((N, OUT_LD), dtype=torch.float32, **kw)
        self.boot_out = torch.zeros((E, OUT_LD), dtype=torch.float32, **kw)
        self.rows_img = torch.zeros(N, dtype=torch.int32, **kw)
        self.rows_goal = torch.zeros(N, dtype=torch.int32, **kw)
        self.actions = torch.zeros(N, dtype=torch.int32, **kw)
        self.rewards = torch.zeros((T, E), dtype=torch.float32, **kw)
        self.dones = torch.zeros((T, E), dtype=torch.bool, **kw)
        self.states = torch.zeros(E, dtype=torch.int32, **kw)
        self.returns = torch.zeros(N, dtype=torch.float32, **kw)
        self.dout = torch.zeros((N, OUT_LD), dtype=torch.float32, **kw)
        self.stats = torch.zeros(4, dtype=torch.float32, **kw)
        if self.ppo:
            # the behaviour policy's head outputs, fixed for the update; [mean, rstd] of its
            # advantages; the last epoch's [kl sum, clipped samples, ratio sum, value-clipped samples]
            self.out_old = torch.zeros((N, OUT_LD), dtype=torch.float32, **kw)
            self.adv_stats = torch.zeros(2, dtype=torch.float32, **kw)
            self.ppo_stats = torch.zeros(4, dtype=torch.float32, **kw)
            if self.ppo_target_kl is not None:
                # vn_ppo_kl_gate's [stopped, steps allowed] and [the last check's KL, the KL that
                # stopped the update], zeroed when an update begins
                self.kl_gate = torch.zeros(2, dtype=torch.int32, **kw)
                self.kl_dev = torch.zeros(2, dtype=torch.float32, **kw)
        self.norm_partial = torch.zeros(512, dtype=torch.float64, **kw)
        self.scalars = torch.zeros(2, dtype=torch.float32, **kw)
        self.episode_stats = torch.zeros(3, dtype=torch.float32, **kw)  # count, return sum, length sum
        # nav_metrics: success rate and SPL of the finished episodes from the env's navigation
        # info (vn_nav_enable); nav_stats = [episodes, successes, SPL sum, start-distance sum] of
        # the last rollout. Episodes already running are measured from here on.
        self.nav_metrics = bool(nav_metrics)
        if self.nav_metrics:
            if not env.nav_info:
                env.set_nav_info(True)
            self.nav_stats = torch.zeros(4, dtype=torch.float32, **kw)
        # expert_weight (None = off): the shortest-path expert term -w mean log sum_{a in M} pi(a)
        # on the rollout's samples, M = the env's optimal_mask of the state each sample observed
        # (DESIGN.md "Expert loss from the navigation tables"). expert_mask [T, E]: step t's nav
        # launch writes slot t + 1 (the state it leaves the env in is step t + 1's observation),
        # slot 0 is copied from the env's own buffer when a rollout begins. expert_stats =
        # [sum of -log q, agreeing samples, labelled samples, the weight used]; expert_steps =
        # the env-step count the update's learning rate is computed from.
        self.expert = expert_weight is not None
        self.pg_coefficient = float(pg_coefficient)
        if not self.expert and self.pg_coefficient != 1.0:
            raise ValueError("pg_coefficient != 1 needs the expert term (expert_weight): without it nothing would "
                             "train the policy head")
        if self.expert:
            self.expert_weight = float(expert_weight)
            self.expert_anneal_steps = int(expert_anneal_steps)
            if not env.nav_info:
                env.set_nav_info(True)
            if "optimal_mask" not in env._info:
                raise ValueError("expert_weight needs the env's optimal_mask buffer (set_nav_info was given None)")
            self.expert_mask = torch.zeros((T, E), dtype=torch.uint8, **kw)
            self.expert_stats = torch.zeros(4, dtype=torch.float32, **kw)
            self.expert_steps = torch.zeros(1, dtype=torch.int64, **kw)
        # shaping_weight (None = off) and gae_lambda (1 = the n-step return): the returns of the
        # update come from vn_a2c_returns_ex (DESIGN.md "Reward shaping and GAE"), which adds
        # w (d_before - shaping_gamma d_after) to every reward, w annealed linearly to 0 over
        # shaping_anneal_steps env steps (0: constant), and forms the lambda-return. shape_dist
        # [T, 2, E]: step t's progress launch writes the distances before and after it into slot
        # t. The env's reward, ep_return and the LSTM's last-reward input stay the environment's
        # own. shape_stats = [sum of before, sum of after, invalid steps] of the last update;
        # shape_steps = the env-step count the anneal reads. With None and 1.0 nothing is
        # allocated and vn_a2c_returns is called as before.
        self.gae_lambda = float(gae_lambda)
        if not 0.0 <= self.gae_lambda <= 1.0:
            raise ValueError("gae_lambda must lie in [0, 1], got %r" % (gae_lambda,))
        self.shaping = shaping_weight is not None
        self.returns_ex = self.shaping or self.gae_lambda != 1.0
        self.shaping_weight = float(shaping_weight) if self.shaping else 0.0
        self.shaping_gamma = float(shaping_gamma)
        self.shaping_anneal_steps = int(shaping_anneal_steps) if self.shaping else 0
        if self.returns_ex:
            self.shape_stats = torch.zeros(3, dtype=torch.int64, **kw)
            self.shape_steps = torch.zeros(1, dtype=torch.int64, **kw)
            self.shape_dist = None
        if self.shaping:
            if not env.nav_info:
                env.set_nav_info(True)
            if not env.nav_progress:
                env.set_nav_progress(True)
            self.shape_dist = torch.zeros((T, 2, E), dtype=torch.int32, **kw)
        # geo_curriculum (None = off): VectorEnv.set_geodesic_curriculum's keyword arguments. Starts
        # are drawn within `level` actions of the goal, and with window > 0 every update ends its
        # rollout with one curriculum_advance(), inside the captured graph too: the level moves on
        # the device, so the graph stays valid. Enabled here, before any capture and after the nav
        # setup above (set_nav_info would switch it off). At world > 1 every rank adapts on its own
        # envs, with no collective: curriculum_level is this rank's mean over scenes.
        self.geo_curriculum = None if geo_curriculum is None else dict(geo_curriculum)
        if self.geo_curriculum is not None:
            env.set_geodesic_curriculum(**self.geo_curriculum)
            self.cur_state = torch.zeros((4, len(env.scenes)), dtype=torch.int32, **kw)
        # device schedule: [next sampling-counter base (updates * T), env-steps so far, this
        # update's counter base] and the learning rate of the update (vn_a2c_schedule)
        self.sched = torch.zeros(3, dtype=torch.int64, **kw)
        self.lr_dev = torch.zeros(1, dtype=torch.float32, **kw)
        # rp_sampling: where the reward-prediction samples come from. "sequence" = the three-frame
        # windows of the rollout the other UNREAL losses run on. "skewed" = rp_batch windows drawn
        # from every filled slot of the replay ring with P(reward != 0) = rp_skew, the published
        # rule (vn_unreal_rp_sample, DESIGN.md "Reward-skewed reward prediction"): their 3 rp_batch
        # frames ride behind the replayed pass's own trunk rows. rp_batch None = unreal_envs.
        if rp_sampling not in ("sequence", "skewed"):
            raise ValueError("rp_sampling must be 'sequence' or 'skewed'")
        self.rp_sampling = rp_sampling
        self.rp_skewed = rp_sampling == "skewed"
        self.rp_skew = float(rp_skew)
        self.rp_batch = None if rp_batch is None else int(rp_batch)
        if self.rp_skewed:
            if not (unreal and unreal_source == "replay"):
                raise ValueError("rp_sampling='skewed' draws from the replay ring: it needs unreal=True and "
                                 "unreal_source='replay'")
            if os.environ.get("VN_REPLAY_MERGED"):
                raise ValueError("rp_sampling='skewed' does not run with VN_REPLAY_MERGED=1: the merged pass runs the "
                                 "aux heads on the replayed pass's activation store, which here also holds the "
                                 "sampled frames")
            if not 0.0 <= self.rp_skew <= 1.0:
                raise ValueError("rp_skew must lie in [0, 1], got %r" % (rp_skew,))
            if self.rp_batch is not None and self.rp_batch < 1:
                raise ValueError("rp_batch must be at least 1, got %r" % (rp_batch,))
        # novelty_weight / first_visit_weight (both 0 = off): the returns of the update are formed
        # from rewards_aug = reward + w_count / sqrt(N(s)) + w_first [first visit of the episode]
        # (vn_a2c_novelty_rewards, DESIGN.md "Visit counts and novelty bonus"), N the env's visit
        # table at the end of the rollout, both weights annealed linearly to 0 over
        # novelty_anneal_steps env steps (0: constant). visit_cell / visit_first [T, E]: step t's
        # visit launch writes slot t. Everything else stays on the env's own reward: episode
        # returns, the LSTM's last-reward input, the UNREAL labels and the replay ring. With both
        # weights 0 nothing is allocated and no launch is added.
        self.novelty_weight = float(novelty_weight)
        self.first_visit_weight = float(first_visit_weight)
        self.novelty_anneal_steps = int(novelty_anneal_steps)
        if self.novelty_weight < 0 or self.first_visit_weight < 0:
            raise ValueError("novelty_weight and first_visit_weight must be >= 0, got %r, %r"
                             % (novelty_weight, first_visit_weight))
        if self.novelty_anneal_steps < 0:
            raise ValueError("novelty_anneal_steps must be >= 0, got %r" % (novelty_anneal_steps,))
        self.novelty = self.novelty_weight != 0.0 or self.first_visit_weight != 0.0
        if self.novelty:
            if not env.visit_counts:
                env.set_visit_counts(True)
            self.visit_cell = torch.zeros((T, E), dtype=torch.int32, **kw)
            self.visit_first = torch.zeros((T, E), dtype=torch.bool, **kw)
            self.rewards_aug = torch.zeros((T, E), dtype=torch.float32, **kw)
            self.novelty_stats = torch.zeros(4, dtype=torch.float32, **kw)
            self.novelty_steps = torch.zeros(1, dtype=torch.int64, **kw)
            self.visit_seen = torch.zeros(2, dtype=torch.int64, **kw)  # [states seen, visits] of this rank
        self._metric_layout = metric_layout(bool(unreal), self.nav_metrics, self.expert, self.geo_curriculum is not None,
                                            self.shaping, self.rp_skewed, self.novelty,
                                            ppo=self.ppo,  # step()'s vector: {segment: (offset, width)}
                                            ppo_kl=self.ppo_target_kl is not None)
        self.workspace = torch.empty(self.net.workspace_floats(N), dtype=torch.float32, **kw)
        # what _forward_stored / _backward read beside the frames: the LSTM inputs and start state
        # (recurrent), and the aux heads' targets; the minibatches have their own (self.mb)
        self._seq, self._aux_targets = {}, None
        if self.recurrent:
            X = self.net.lstm["xcat"]
            A1 = self.A + 1
            f32 = dict(dtype=torch.float32, **kw)
            self.xcat = torch.zeros((N, X), **f32)
            self.lstm_acts = torch.zeros((N, 2048), **f32)
            # h and c of every step in one [2][T*E][512] buffer, and the carry into the next
            # rollout in one [2][E][512] buffer: the carry is one strided copy per update
            self._hc_all = torch.zeros((2, N, 512), **f32)
            self.h_all, self.c_all = self._hc_all[0], self._hc_all[1]
            self.gates = torch.zeros((E, 2048), **f32)
            self.masks = torch.ones((T, E), **f32)
            self.lra = torch.zeros((T, E, A1), **f32)
            self._hc0 = torch.zeros((2, E, 512), **f32)  # state entering the rollout
            if self.ppo:  # the rollout's last (h, c), saved before an epoch's re-forward overwrites them
                self._hc_last = torch.zeros((2, E, 512), **f32)
            self.h0, self.c0 = self._hc0[0], self._hc0[1]
            self._seq = dict(lra=self.lra, masks=self.masks, h0=self.h0, c0=self.c0)
            self.prev_action = torch.zeros(E, dtype=torch.int64, **kw)
            self.prev_reward = torch.zeros(E, **f32)
            self.prev_mask = torch.zeros(E, **f32)    # 0: the first step starts every episode
            self.boot_xcat = torch.zeros((E, X), **f32)
            self.boot_la = torch.zeros((E, 2048), **f32)
            self.boot_c = torch.zeros((E, 512), **f32)
            self.boot_h = torch.zeros((E, 512), **f32)
            self.boot_mask = torch.zeros(E, **f32)
            self.boot_lra = torch.zeros((E, A1), **f32)
            self.dz5 = torch.zeros((N, 512), **f32)
            self.lstm_ws = torch.empty(self.net.lstm_workspace_floats(T, E), **f32)
        if self.aux_weight > 0:
            self.a1, self.pred = self.net.aux_buffers(N)
            self.dpred = torch.empty_like(self.pred)
            self.dx4 = torch.zeros((N, self.net.fc_in), dtype=torch.float32, **kw)
            self.aux_stats = torch.zeros(4, dtype=torch.float32, **kw)
            self.aux_ws = torch.empty(self.net.aux_workspace_floats(), dtype=torch.float32, **kw)
            self.aux_table = self.net.aux_target_table(*env.aux_arena)  # once per scene cache
            self._aux_targets = AuxTargets(self.aux_table.data_ptr(), self.rows_img.data_ptr(),
                                           self.rows_goal.data_ptr())
            ph, pw = self.net.aux_layout["p_hw"]
            self._aux_numel = torch.tensor([1.0, 3.0, 3.0], device=self.device) * (N * ph * pw)
        # aux batch source: "rollout" = the on-policy batch (its trunk activations are reused),
        # "replay" = a sequence from the last replay_size rollouts (AuxiliaryTrainer's
        # self.replay.sample_sequence(), experiments/ai2_auxiliary/trainer.py:29): its own
        # trunk forward + backward, gradients added to the on-policy ones
        if aux_source not in ("rollout", "replay"):
            raise ValueError("aux_source must be 'rollout' or 'replay'")
        if unreal_source not in ("rollout", "replay"):
            raise ValueError("unreal_source must be 'rollout' or 'replay'")
        self.aux_source = aux_source
        self.unreal_source = unreal_source if unreal else "rollout"
        # the replay ring of the last replay_size rollouts (deep_rl's replay buffer, absent: its
        # capacity and sequence shape are parity unpinned); one stored rollout is drawn per update.
        # Push and draw run on the device (vn_replay_push_draw: meta = [next slot, filled, draw
        # counter, drawn slot]), so an update with replay sources is captured by cuda_graph=True.
        self.replay = aux_source == "replay" or self.unreal_source == "replay"
        if self.replay:
            self.replay_rows = torch.zeros((int(replay_size), 2, N), dtype=torch.int32, **kw)
            self.replay_meta = torch.zeros(4, dtype=torch.int64, **kw)
            self._replay_seed = vdist.rank_seed(self.seed + 17, self.rank) & ((1 << 64) - 1)
        if aux_source == "replay":
            if self.aux_weight <= 0:
                raise ValueError("aux_source='replay' needs aux_weight > 0")
            self.aux_rows = torch.zeros((2, N), dtype=torch.int32, **kw)
            self.aux_acts = self.net.new_acts(N)
            self.aux_out = torch.zeros((N, OUT_LD), dtype=torch.float32, **kw)
            self.aux_dz5 = torch.zeros((N, 512), dtype=torch.float32, **kw)
            self.aux_grads = torch.zeros(P, dtype=torch.float32, **kw)
            self._aux_targets_replay = AuxTargets(self.aux_table.data_ptr(), self.aux_rows[0].data_ptr(),
                                                  self.aux_rows[1].data_ptr())
        # compute_auxiliary_loss overridden by a subclass: called every update (autograd on a
        # GoalNavPolicy view of the flat parameters), its gradient added before the all-reduce
        self._setup_unreal(unreal, pc_weight, rp_weight, vr_weight, pc_gamma, unreal_envs)
        # opt-in (VN_REPLAY_MERGED=1), both batches replayed and the UNREAL record holding every
        # env (S == E, the logged run's 4 envs): the replayed UNREAL pass's trunk forward covers
        # the aux batch's samples (rows t*S + e = t*E + e), so the aux heads can run on it inside
        # the side pass, their dX4 joining its trunk backward — one trunk forward + backward of
        # the replayed rollout instead of two. Measured slower (2.51 vs 2.40 ms per 4-env update,
        # tools/ab/replay_ab.sh): the side stream becomes the critical path while the main
        # stream idles, so the two passes stay the default.
        self._merged_replay = (self.aux_source == "replay" and self.unreal_source == "replay"
                               and self.unreal_S == E and bool(os.environ.get("VN_REPLAY_MERGED")))
        # VN_UNREAL_INLINE=1: the replayed UNREAL pass runs on the main stream before the A2C
        # backward instead of beside it (the race check: both forms must give the same update)
        self._unreal_inline = bool(os.environ.get("VN_UNREAL_INLINE"))
        if self.replay:
            self._replay_segs = self._replay_segments()
        self._custom_aux = type(self).compute_auxiliary_loss is not A2CTrainer.compute_auxiliary_loss
        if self._custom_aux and self.ppo:
            raise ValueError("ppo_clip does not run with a compute_auxiliary_loss override yet: its autograd pass "
                             "is not repeated per epoch")
        if self._custom_aux and cuda_graph:
            raise ValueError("a compute_auxiliary_loss override runs torch autograd per update: use cuda_graph=False")
        self.aux_losses = {}
        self._model_view = None
        arena, fb, _, _ = env.frame_arena()
        self._arena, self._fb = arena, fb
        # goal-frame deduplication (vn_goal_runs): an env's goal frame is constant within an
        # episode, so shared_base runs on it once per goal run — at the rollout's first step and
        # after each done — and the backward sums a run's goal-map gradients before conv2 /
        # conv1 (same outputs, gradients up to summation order). Runs where the policy's
        # kernels take frame lists (84x84 / 174x174, more than 16 envs).
        # dedup_goals None = on where supported. Not with companion frames (OrientedGraphEnv's
        # third-person view, vn_env.hip goal_row = companion row + state): that second frame
        # changes at every step, so a run start's maps are not the later steps' maps.
        companion = any(getattr(s, "companion", None) is not None for s in getattr(env, "scenes", ()))
        if dedup_goals and companion:
            raise ValueError("dedup_goals=True needs a goal frame that is constant within an episode; these scenes "
                             "emit companion frames (a per-step third-person view) as the second frame")
        self.dedup_goals = (dedup_goals is None or bool(dedup_goals)) and not companion and \
            self.net.arch == "goal" and self.net.goal_runs_supported(E)
        if self.dedup_goals:
            i32 = dict(dtype=torch.int32, **kw)
            self.goal_delta = torch.zeros((T, E), **i32)
            self.goal_list_step = torch.zeros((T, E), **i32)
            self.goal_count = torch.zeros(T + 1, **i32)  # per step, then the update's
            self.goal_list = torch.zeros(N, **i32)
            self.goal_run_length = torch.zeros(N, **i32)
            self._goal_runs_step = []
            for t in range(T):
                g = _lib.GoalRuns()
                g.goal_list = self.goal_list_step[t].data_ptr()
                g.goal_count = self.goal_count[t:t + 1].data_ptr()
                g.goal_delta = self.goal_delta[t].data_ptr()
                g.num_envs = E
                self._goal_runs_step.append(g)
            g = _lib.GoalRuns()
            g.goal_list = self.goal_list.data_ptr()
            g.goal_count = self.goal_count[T:T + 1].data_ptr()
            g.goal_delta = self.goal_delta.data_ptr()
            g.run_length = self.goal_run_length.data_ptr()
            g.num_envs = E
            self._goal_runs_update = g
        # the rollout's fused env steps (vn_step_a2c): sampling + step + bookkeeping, one launch
        # per step; per-env episode statistics reduced once per rollout (vn_a2c_episode_stats)
        self.stats_env = torch.zeros((3, E), dtype=torch.float32, **kw)
        # a few envs, recurrent: the heads of each rollout step run inside its env-step launch
        # (vn_a2c_step.head_weight: vn_policy_heads' skinny sums, bit-identical), one launch
        # fewer per step
        self._fused_heads = self.recurrent and E <= _FUSED_HEADS_MAX_ENVS
        self._a2c_steps = [self._a2c_step_args(t) for t in range(T)]
        if self.ppo_minibatches > 1:
            self._setup_ppo_minibatches()
        env.observe(gather=False)  # refresh the obs row buffers for the first forward
        self.num_updates = 0
        self.total_steps = 0
        self.cuda_graph = bool(cuda_graph)
        self.on_ppo_epoch = None
        self.on_ppo_minibatch = None
        if self.cuda_graph and self.world > 1:
            if not vdist.capturable(process_group):
                raise ValueError("cuda_graph=True at world > 1 needs the nccl (RCCL) backend: a gloo all-reduce "
                                 "cannot be captured in a hipGraph")
            if not capture_collectives:
                # the captured RCCL all-reduce has not run against eager updates on a multi-GPU
                # node (DESIGN.md "Multi-GPU"): opt in explicitly
                raise ValueError("cuda_graph=True at world > 1 captures the RCCL all-reduces in the hipGraph, which "
                                 "is not yet validated against eager updates: pass capture_collectives=True to opt in")
        self._graph = None
        self._graph_out = None
        self._graph_gen = None

    def _setup_ppo_minibatches(self):
        """The split of ppo_minibatches = M > 1: minibatch m of an epoch holds the envs
        perm[lo_m:lo_{m+1}], lo_m = floor(m E / M). Allocated here: the permutation and the compact
        [T, ceil(E / M)] copies of the rollout's index and input buffers (a smaller minibatch uses
        their front). The activations of a minibatch live in the rollout's own buffers at the
        smaller row count, so nothing of the size of a frame or a feature map is added."""
        net, E, T, M = self.net, self.env.num_envs, self.num_steps, self.ppo_minibatches
        A1 = self.A + 1
        self.mb_bounds = [m * E // M for m in range(M + 1)]
        sizes = sorted({hi - lo for lo, hi in zip(self.mb_bounds, self.mb_bounds[1:])})
        cap_e = sizes[-1]
        cap = T * cap_e
        i32 = dict(dtype=torch.int32, device=self.device)
        f32 = dict(dtype=torch.float32, device=self.device)
        self.ppo_perm = torch.zeros(E, **i32)
        self._ppo_seed = vdist.rank_seed(self.seed, self.rank)  # the sampling key; the stream id is the draw's own
        mb = self.mb = dict(rows_img=torch.zeros(cap, **i32), rows_goal=torch.zeros(cap, **i32),
                            actions=torch.zeros(cap, **i32), returns=torch.zeros(cap, **f32),
                            out_old=torch.zeros((cap, OUT_LD), **f32),
                            dones=torch.zeros(cap, dtype=torch.bool, device=self.device))
        src = dict(rows_img=self.rows_img, rows_goal=self.rows_goal, actions=self.actions, returns=self.returns,
                   out_old=self.out_old, dones=self.dones)
        if self.recurrent:
            mb.update(masks=torch.zeros(cap, **f32), lra=torch.zeros((cap, A1), **f32))
            self.mb_hc0 = torch.zeros((2, cap_e, 512), **f32)
            mb.update(h0=self.mb_hc0[0], c0=self.mb_hc0[1])
            src.update(masks=self.masks, lra=self.lra, h0=self.h0, c0=self.c0)
        # goal runs per minibatch where the policy takes them at its row count
        self._mb_goal_runs = {}
        if self.dedup_goals:
            mb["goal_delta"] = torch.zeros(cap, **i32)
            src["goal_delta"] = self.goal_delta
            for eb in sizes:
                if net.goal_runs_supported(T * eb):
                    g = _lib.GoalRuns()
                    g.goal_list = self.goal_list.data_ptr()
                    g.goal_count = self.goal_count[T:T + 1].data_ptr()
                    g.goal_delta = mb["goal_delta"].data_ptr()
                    g.run_length = self.goal_run_length.data_ptr()
                    g.num_envs = eb
                    self._mb_goal_runs[eb] = g
        self._mb_src = _lib.PpoRollout(**{k: v.data_ptr() for k, v in src.items()})
        self._mb_dst = _lib.PpoRollout(**{k: v.data_ptr() for k, v in mb.items()})
        self._mb_frames = self._frames(mb["rows_img"], mb["rows_goal"])
        self._mb_aux_targets = None
        if self.aux_weight > 0:
            self._mb_aux_targets = AuxTargets(self.aux_table.data_ptr(), mb["rows_img"].data_ptr(),
                                              mb["rows_goal"].data_ptr())
        # the scratch of the backward at the minibatch's launch regimes, where it is the larger
        need = max(net.workspace_floats(T * eb) for eb in sizes)
        if need > self.workspace.numel():
            self.workspace = torch.empty(need, **f32)
        if self.recurrent:
            need = max(net.lstm_workspace_floats(T, eb) for eb in sizes)
            if need > self.lstm_ws.numel():
                self.lstm_ws = torch.empty(need, **f32)

    def _setup_unreal(self, unreal, pc_weight, rp_weight, vr_weight, pc_gamma, unreal_envs):
        """Buffers of the UNREAL losses: the first S envs' T + 1 LSTM features (the last row
        the bootstrap's) through the pixel-control heads, their T - 2 three-frame conv_base
        samples through reward prediction. unreal_source 'replay': the same losses on the first
        S envs' sequences of a stored rollout (their own trunk, LSTM and heads pass)."""
        self.unreal = bool(unreal)
        if not self.unreal:
            self.unreal_source = "rollout"
            return
        net, E, T = self.net, self.env.num_envs, self.num_steps
        if not (net.unreal and net.recurrent):
            raise ValueError("unreal=True needs a recurrent policy with the UNREAL heads")
        H, W = self.env.frame_shape[:2]
        C = self.pc_cells = net.pc_side  # 42 (goal.py:72, 112) or 20 (BigHouseModel, bignet.py:77-91)
        if H < 4 * C or W < 4 * C:
            raise ValueError("pixel control crops %d cells of 4 px: frames need >= %d px" % (C, 4 * C))
        if T < 3:
            raise ValueError("reward prediction needs num_steps >= 3")
        self.pc_weight, self.rp_weight, self.vr_weight = float(pc_weight), float(rp_weight), float(vr_weight)
        self.pc_gamma = float(pc_gamma)
        S = self.unreal_S = max(1, min(int(unreal_envs), E))
        kw = dict(dtype=torch.float32, device=self.device)
        n_pc = (T + 1) * S
        self.h_pc = torch.zeros((n_pc, 512), **kw)
        self.pcb, self.pc_a1, self.pc_p2, _ = net.pc_buffers(n_pc, with_q=False)
        self.dh_pc = torch.zeros((n_pc, 512), **kw)
        self.pc_ws = torch.empty(net.pc_workspace_floats(), **kw)
        F = net.fc_in
        # reward-prediction samples: every window of the S sequences, or rp_batch drawn ones (then
        # rp_x / rp_dx are views of the replayed pass's own buffers, _setup_unreal_replay)
        n_rp = self.rp_n = (self.rp_batch or S) if self.rp_skewed else (T - 2) * S
        if not self.rp_skewed:
            self.rp_x = torch.zeros((n_rp, 3 * F), **kw)
            self.rp_dx = torch.zeros((n_rp, 3 * F), **kw)
        self.rp_out = torch.zeros((n_rp, 4), **kw)
        self.rp_dout = torch.zeros((n_rp, 4), **kw)
        # rp's gradient w.r.t. conv_base's map: into the aux heads' dX4 when those run on the
        # rollout, else into its own buffer (rows of envs >= S stay zero)
        self.rp_into_aux = self.aux_weight > 0 and self.aux_source == "rollout"
        self.unreal_dx4 = None if self.rp_into_aux else torch.zeros((T * E, F), **kw)
        self.unreal_stats = torch.zeros(4, **kw)  # pc sum sq, rp mean CE, rp samples, vr sum sq
        self._unreal_norm = torch.tensor([1.0 / (T * S * C * C), 1.0, 1.0 / (T * S)], **kw)
        if self.unreal_source == "replay":
            self._setup_unreal_replay()

    def _setup_unreal_replay(self):
        """The replay ring's per-rollout record of the first S envs (rows t*S + e, the
        bootstrap observation at t = T) and the buffers of their forward / backward pass."""
        net, E, T, S = self.net, self.env.num_envs, self.num_steps, self.unreal_S
        R = self.replay_rows.shape[0]
        A1 = self.A + 1
        n = (T + 1) * S
        f32 = dict(dtype=torch.float32, device=self.device)
        i32 = dict(dtype=torch.int32, device=self.device)
        self.ur = dict(rows=torch.zeros((R, 2, n), **i32), actions=torch.zeros((R, T * S), **i32),
                       rewards=torch.zeros((R, T, S), **f32),
                       dones=torch.zeros((R, T, S), dtype=torch.bool, device=self.device),
                       masks=torch.zeros((R, T + 1, S), **f32), lra=torch.zeros((R, T + 1, S, A1), **f32),
                       hc0=torch.zeros((R, 2, S, 512), **f32))
        if self.shaping:  # the first S envs' distances before and after every step
            self.ur["shape_dist"] = torch.zeros((R, T, 2, S), **i32)
        if self.returns_ex:
            self.ur_shape_stats = torch.zeros(3, dtype=torch.int64, device=self.device)
        # the slot drawn this update, copied out of the ring by vn_replay_push_draw (fixed
        # addresses: the replayed pass's launches do not depend on which slot was drawn)
        self.ur_cur = {key: torch.zeros_like(v[0]) for key, v in self.ur.items()}
        # rp_sampling='skewed': the 3 rp_n sampled frames (sample-major: window j's frames are rows
        # n + 3 j + m) ride behind the drawn slot's n rows through the same trunk forward and
        # backward. One row table holds both (the slot's rows drawn into its first n columns, the
        # sampler's output behind them); conv_base's maps of the appended rows are rp's input as
        # they lie, and the appended rows of dX4 are its input gradient: no gather, no scatter.
        cap = self.ur_cap = n + (3 * self.rp_n if self.rp_skewed else 0)
        if self.rp_skewed:
            if R * (T - 2) * S > _lib.RP_SAMPLE_MAX_CANDIDATES:
                raise ValueError("rp_sampling='skewed': replay_size * (num_steps - 2) * unreal_envs = %d windows exceed "
                                 "the sampler's %d" % (R * (T - 2) * S, _lib.RP_SAMPLE_MAX_CANDIDATES))
            self.ur_rows_ext = torch.zeros((2, cap), **i32)
            self.ur_cur["rows"] = self.ur_rows_ext[:, :n]
            self.rp_rows = self.ur_rows_ext[:, n:].unflatten(1, (self.rp_n, 3))  # [2][rp_n][3] views
            self.rp_label = torch.zeros(self.rp_n, **i32)
            self.rp_src = torch.zeros(self.rp_n, **i32)
            self.rp_draw_stats = torch.zeros(4, **i32)  # |Q0|, |Q1|, draws with a reward, non-void draws
            u = self.ur
            self._rp_ring = _lib.RpRing(u["rewards"].data_ptr(), u["dones"].data_ptr(), u["rows"].data_ptr(),
                                        self.replay_meta.data_ptr(), R, T, S)
            # the counter is the ring's own draw counter (replay_meta[2]): no state of its own
            self._rp_seed = vdist.rank_seed(self.seed + 29, self.rank) & ((1 << 64) - 1)
        X = net.lstm["xcat"]
        # Side-stream-owned (update(): the replayed pass runs on self._side_u beside the A2C
        # backward): the buffers _side_owned() lists. Nothing on the main stream may touch them
        # between the fork and the join — checked by _check_side_stream_disjoint
        # (VN_DEBUG_STREAMS=1 or A2CTrainer.debug_streams) and tests/test_unreal_gpu.py.
        self.ur_acts = net.new_acts(cap)
        self.ur_xcat = torch.zeros((n, X), **f32)
        self.ur_lacts = torch.zeros((n, 2048), **f32)
        self.ur_hc = torch.zeros((2, n, 512), **f32)
        self.ur_gates = torch.zeros((S, 2048), **f32)
        self.ur_out = torch.zeros((n, OUT_LD), **f32)
        self.ur_returns = torch.zeros(T * S, **f32)
        self.ur_dout = torch.zeros((n, OUT_LD), **f32)
        self.ur_dz5 = torch.zeros((cap, 512), **f32)  # the sampled frames' rows stay zero
        # the bootstrap rows stay zero; skewed: so do the slot's rows, rp writes the appended ones
        self.ur_dx4 = torch.zeros((cap, net.fc_in), **f32)
        self.ur_grads = torch.zeros(net.n_params, **f32)
        self.ur_ws = torch.empty(net.workspace_floats(cap), **f32)
        if self.rp_skewed:
            F = net.fc_in
            self.rp_x = net.x4(self.ur_acts, cap)[n:].view(self.rp_n, 3 * F)
            self.rp_dx = self.ur_dx4[n:].view(self.rp_n, 3 * F)
        self.ur_lstm_ws = torch.empty(net.lstm_workspace_floats(T + 1, S), **f32)
        # the grads of the trunk, heads and LSTM (everything before the aux / UNREAL blocks)
        self._ur_add_end = net.lstm["bhh"] + 2048
        # the replayed pass runs on a side stream beside the A2C backward (update()): its own
        # policy handle, so its small-batch split-K products have their own scratch
        self._net_u = PolicyNet(net.frame_hw, net.num_actions, self.device, recurrent=net.recurrent, aux=net.aux,
                                arch=net.arch, unreal=net.unreal)
        self._side_u = torch.cuda.Stream(device=self.device)
        self._ev_u0, self._ev_u1 = torch.cuda.Event(), torch.cuda.Event()

    def _unreal_head_losses(self, net, out, returns, dout, h, x4, actions, rewards, dones, rows_img, rows_last, T, E, S,
                            dx4, accumulate, h_src=(None, None)):
        """The UNREAL head losses on the first S of E envs' sequences, on the handle ``net``: value
        replay of ``out`` into ``dout``; pixel control on ``h`` (rows t*S + e, the bootstrap's at
        t = T), dL/dh into dh_pc; reward prediction on three consecutive conv_base maps of ``x4``,
        dL/dX4 into ``dx4`` (added when ``accumulate``); both heads' gradients into grads.
        ``h_src``: (steps' h, bootstrap's h) of all E envs, gathered into ``h`` by the launch that
        gathers the rp input (NULL: ``h`` holds them already)."""
        lib, A, F, P, st = self.lib, self.A, net.fc_in, _lib.ptr, self._stream()
        self.unreal_stats.zero_()
        if self.vr_weight > 0:
            _lib.check(lib.vn_unreal_vr_grad(P(out), P(returns), T, E, S, A, ctypes.c_float(self.vr_weight), P(dout),
                                             P(self.unreal_stats[3:]), st), "vn_unreal_vr_grad")
        if not self.rp_skewed:  # (skewed: replayed pass only, h in place and rp_x = the appended maps)
            _lib.check(lib.vn_unreal_gather(P(h_src[0]), P(h_src[1]), P(x4), T, E, S, F,
                                            None if h_src[0] is None else P(h), P(self.rp_x), st), "vn_unreal_gather")
        n_pc = (T + 1) * S
        net.pc_forward(self.params, h, n_pc, self.pcb, self.pc_a1, self.pc_p2, None, self.pc_ws)
        H, W = self.env.frame_shape[:2]
        # q formed from p2 in the loss kernel, which leaves dL/dp2 in p2 for the backward
        _lib.check(lib.vn_unreal_pc_loss_grad_ex(P(self.pc_p2), self.pc_cells, P(actions), P(dones),
                                                 ctypes.c_void_p(self._arena), ctypes.c_int64(self._fb), H, W,
                                                 P(rows_img), P(rows_last), T, E, S, A, ctypes.c_float(self.pc_gamma),
                                                 ctypes.c_float(self.pc_weight), P(self.unreal_stats), st),
                   "vn_unreal_pc_loss_grad")
        net.pc_backward(self.params, h, n_pc, self.pcb, self.pc_a1, self.pc_p2, None, self.grads, self.dh_pc, self.pc_ws)
        n_rp = self.rp_n
        net.rp_forward(self.params, self.rp_x, n_rp, self.rp_out)
        if self.rp_skewed:
            # the sampled windows: classes from the sampler's labels (-1 = a void draw); rp_dx is
            # the appended slice of the replayed pass's dX4, so nothing is scattered
            _lib.check(lib.vn_unreal_rp_loss_grad_labels(P(self.rp_out), P(self.rp_label), n_rp,
                                                         ctypes.c_float(self.rp_weight), P(self.rp_dout),
                                                         P(self.unreal_stats[1:3]), st),
                       "vn_unreal_rp_loss_grad_labels")
            net.rp_backward(self.params, self.rp_x, n_rp, self.rp_dout, self.grads, self.rp_dx, self.pc_ws)
            return
        _lib.check(lib.vn_unreal_rp_loss_grad(P(self.rp_out), P(rewards), P(dones), T, E, S,
                                              ctypes.c_float(self.rp_weight), P(self.rp_dout),
                                              P(self.unreal_stats[1:3]), st), "vn_unreal_rp_loss_grad")
        net.rp_backward(self.params, self.rp_x, n_rp, self.rp_dout, self.grads, self.rp_dx, self.pc_ws)
        _lib.check(lib.vn_unreal_rp_scatter(P(self.rp_dx), T, E, S, F, P(dx4), int(accumulate), st),
                   "vn_unreal_rp_scatter")

    # deep_rl hook names (experiments/thor_cached_auxiliary.py:50-56)
    def create_env(self, kwargs):
        return self.env

    def create_model(self):
        return self.net

    def sample_training_batch(self):
        """deep_rl's UnrealTrainer.sample_training_batch (AuxiliaryTrainer adds the
        'auxiliary_batch', experiments/ai2_auxiliary/trainer.py:27-31): one rollout of
        num_steps on every local env. Returns (batch, report): the batch references the
        trainer's device buffers (valid until the next rollout), the report holds the
        finished-episode statistics [count, return sum, length sum] as a device tensor."""
        self.rollout()
        batch = RolloutBatch(self, self.rows_img, self.rows_goal)
        if self.replay:
            aux = self._replay_push_and_sample()
            if aux is not None:
                batch["auxiliary_batch"] = aux
        return batch, {"episode_stats": self.episode_stats}

    def compute_auxiliary_loss(self, model, batch, device):
        """deep_rl hook (experiments/ai2_auxiliary/trainer.py:33-43): extra loss terms on a
        batch -> (loss tensor or None, {name: float}). The default adds nothing here: the
        deconv loss of aux_weight > 0 is computed by the fused kernels inside update().
        An override receives a GoalNavPolicy view of the flat parameters (``model``) and the
        RolloutBatch; its loss's parameter gradient is added to the update's gradient
        before the all-reduce, clip and RMSprop."""
        return None, {}

    def model_view(self):
        """GoalNavPolicy (BigHousePolicy) over this trainer's PolicyNet whose parameter aliases
        the flat device buffer the kernels update."""
        if self._model_view is None:
            from .policy import GoalNavPolicy
            self._model_view = GoalNavPolicy.wrap(self.net, self.params)
        return self._model_view

    def _returns(self, rewards, dones, boot_out, out, T, E, returns, replayed=False):
        """The returns of T steps of E envs: vn_a2c_returns, or with shaping / GAE on
        vn_a2c_returns_ex (the same launch shape) with this trainer's gamma, lambda and shaping
        arguments; ``replayed``: on the drawn slot's distances, under the current weight."""
        P, c_float, st = _lib.ptr, ctypes.c_float, self._stream()
        if not self.returns_ex:
            _lib.check(self.lib.vn_a2c_returns(P(rewards), P(dones), P(boot_out), T, E, self.A, c_float(self.gamma),
                                               P(returns), st), "vn_a2c_returns")
            return
        dist = self.ur_cur.get("shape_dist") if replayed else self.shape_dist
        stats = self.ur_shape_stats if replayed else self.shape_stats
        _lib.check(self.lib.vn_a2c_returns_ex(
            P(rewards), P(dones), P(boot_out), P(out), P(dist), T, E, self.A, c_float(self.gamma),
            c_float(self.gae_lambda), c_float(self.shaping_weight), c_float(self.shaping_gamma), P(self.shape_steps),
            ctypes.c_int64(self.shaping_anneal_steps), P(returns), P(stats), st), "vn_a2c_returns_ex")

    def _novelty_rewards(self):
        """rewards_aug of the rollout just sampled: one vn_a2c_novelty_rewards launch on the visit
        histories and the env's table as it stands, and the table's statistics for the metrics.
        The input of the returns only: self.rewards stays the env's own."""
        P, c_float, env, T = _lib.ptr, ctypes.c_float, self.env, self.num_steps
        count, _, cells = env.visit_cells()
        _lib.check(self.lib.vn_a2c_novelty_rewards(
            P(self.rewards), P(self.visit_cell), P(self.visit_first), ctypes.c_void_p(count), ctypes.c_int64(cells), T,
            env.num_envs, c_float(self.novelty_weight), c_float(self.first_visit_weight), P(self.novelty_steps),
            ctypes.c_int64(self.novelty_anneal_steps), P(self.rewards_aug), P(self.novelty_stats), self._stream()),
            "vn_a2c_novelty_rewards")
        env.visit_stats(out=self.visit_seen)
        return self.rewards_aug

    def _return_rewards(self):
        """The rewards the update's returns are formed from: the env's own, or with a novelty
        bonus rewards_aug (one launch, _novelty_rewards)."""
        return self._novelty_rewards() if self.novelty else self.rewards

    def shaping_weight_at(self, steps):
        """The annealed shaping weight at an env-step count, as the device forms it: fp64, rounded
        once to fp32."""
        w = float(np.float32(self.shaping_weight))
        if self.shaping_anneal_steps > 0:
            w = w * max(0.0, 1.0 - float(steps) / float(self.shaping_anneal_steps))
        return float(np.float32(w))

    def _replay_segments(self):
        """The vn_replay_push_draw segments (include/vnav.h vn_replay_seg) of this trainer's
        ring: the frame rows of every sample (drawn into aux_rows for a replayed aux batch) and,
        with unreal_source='replay', the first S envs' record (frame rows of steps 0..T - 1 and
        of the bootstrap observation, actions, rewards, dones, the LSTM inputs of steps 0..T and
        the (h, c) the rollout started from), drawn into ur_cur."""
        E, T, N = self.env.num_envs, self.num_steps, self.num_steps * self.env.num_envs
        segs = []

        def seg(src, ld, rows, cols, ring, slot_elems, cur):
            eb = src.element_size()
            assert ring.element_size() == eb and (cur is None or cur.element_size() == eb)
            assert src.is_contiguous() and ring.is_contiguous() and (cur is None or cur.is_contiguous())
            segs.append(_lib.ReplaySeg(src.data_ptr(), ld, ring.data_ptr(), None if cur is None else cur.data_ptr(),
                                       slot_elems, rows, cols, eb, 0))

        aux = self.aux_source == "replay"
        for j, rows in enumerate((self.rows_img, self.rows_goal)):
            seg(rows, N, 1, N, self.replay_rows[0, j], 2 * N, self.aux_rows[j] if aux else None)
        if self.unreal_source == "replay":
            S, A1 = self.unreal_S, self.A + 1
            n = (T + 1) * S
            u, c, info = self.ur, self.ur_cur, self.env._info
            for j, (rows, last) in enumerate(((self.rows_img, info["img_row"]), (self.rows_goal, info["goal_row"]))):
                seg(rows, E, T, S, u["rows"][0, j], 2 * n, c["rows"][j])
                seg(last, S, 1, S, u["rows"][0, j, T * S:], 2 * n, c["rows"][j, T * S:])
            seg(self.actions, E, T, S, u["actions"][0], T * S, c["actions"])
            seg(self.rewards, E, T, S, u["rewards"][0], T * S, c["rewards"])
            seg(self.dones, E, T, S, u["dones"][0], T * S, c["dones"])
            seg(self.masks, E, T, S, u["masks"][0], (T + 1) * S, c["masks"])
            seg(self.boot_mask, S, 1, S, u["masks"][0, T], (T + 1) * S, c["masks"][T])
            seg(self.lra, E * A1, T, S * A1, u["lra"][0], (T + 1) * S * A1, c["lra"])
            seg(self.boot_lra, S * A1, 1, S * A1, u["lra"][0, T], (T + 1) * S * A1, c["lra"][T])
            seg(self._hc0, E * 512, 2, S * 512, u["hc0"][0], 2 * S * 512, c["hc0"])
            if self.shaping:
                seg(self.shape_dist, E, 2 * T, S, u["shape_dist"][0], 2 * T * S, c["shape_dist"])
        return (_lib.ReplaySeg * len(segs))(*segs)

    @property
    def replay_filled(self):
        """Filled slots of the replay ring (reads the device meta: synchronises)."""
        return int(self.replay_meta[1])

    def _replay_push_and_sample(self):
        """Store this rollout's frame rows (and, for the UNREAL losses, the first S envs'
        sequences) in the replay ring and draw one stored rollout (uniform over the filled
        slots) for this update's replayed batches, on the device in one call
        (vn_replay_push_draw: no host value, capturable). Returns the aux batch (None without
        aux replay)."""
        R = self.replay_rows.shape[0]
        _lib.check(self.lib.vn_replay_push_draw(self._replay_segs, len(self._replay_segs), _lib.ptr(self.replay_meta),
                                                R, self._replay_seed, self._stream()), "vn_replay_push_draw")
        if self.aux_source != "replay":
            return None
        return RolloutBatch(self, self.aux_rows[0], self.aux_rows[1])

    def _unreal_replay_losses(self):
        """UnrealTrainer's losses on the first S envs of the stored rollout drawn this update
        (deep_rl samples its sequences from a replay buffer, experiments/ai2_auxiliary/trainer.py
        :21-31; its sequence shape and initial state are absent, parity unpinned): trunk forward
        of their T + 1 observations, the LSTM over T + 1 steps from the (h, c) the rollout started
        from, the heads; value replay against their n-step returns (bootstrapped from step T),
        pixel control on their h, reward prediction on their conv_base maps; then the LSTM and
        trunk backward of those losses: the pixel-control and reward-prediction blocks straight
        into grads, the trunk / heads / LSTM gradients into ur_grads, which update() adds after
        the side stream's join. Runs on the second policy handle (its own split-K scratch)."""
        net = self._net_u
        T, S = self.num_steps, self.unreal_S
        n = (T + 1) * S
        u = self.ur_cur  # the slot vn_replay_push_draw drew this update
        rows = u["rows"]
        cap = self.ur_cap  # n, or with the skewed rp draw n + 3 rp_n: the sampled frames behind the slot's
        if self.rp_skewed:
            # this update's windows from the whole ring (after its push: the counter and the filled
            # count are read on the device), their frame rows straight behind the slot's
            P = _lib.ptr
            _lib.check(self.lib.vn_unreal_rp_sample(ctypes.byref(self._rp_ring), self.rp_n,
                                                    ctypes.c_double(self.rp_skew), self._rp_seed,
                                                    P(self.rp_rows[0]), P(self.rp_rows[1]), P(self.rp_label),
                                                    P(self.rp_src), P(self.rp_draw_stats), self._stream()),
                       "vn_unreal_rp_sample")
        frame_rows = self.ur_rows_ext if self.rp_skewed else rows
        frames = self._frames(frame_rows[0], frame_rows[1])
        net.forward(self.params, frames, cap, self.ur_acts, cap, 0, None)
        if self._merged_replay:  # the aux heads on the replayed rows t*E + e < T*E (aux_rows' frames)
            N = T * S
            self.aux_stats.zero_()
            net.aux_forward_loss_grad(self.params, self.ur_acts, n, N, self.a1, self.pred, self._aux_targets_replay,
                                      self.aux_weight, self.dpred, self.aux_stats, self.aux_ws)
            net.aux_backward(self.params, self.ur_acts, n, N, self.a1, self.dpred, self.grads, self.ur_dx4, self.aux_ws)
        x5 = net.x5(self.ur_acts, cap)  # the LSTM and the heads run on the slot's n rows only
        h_r, c_r = self.ur_hc[0], self.ur_hc[1]
        h0, c0 = u["hc0"][0], u["hc0"][1]
        net.lstm_sequence(self.params, T + 1, S, x5, u["lra"], u["masks"], h0, c0, self.ur_xcat, self.ur_gates,
                          self.ur_lacts, c_r, h_r)
        net.heads(self.params, h_r, n, self.ur_out)
        self.ur_dout.zero_()
        rew, don = u["rewards"], u["dones"]
        # the drawn slot's returns (V and the bootstrap from ur_out), then the heads' losses on
        # the replayed h (rows t*S + e, the bootstrap at t = T) and conv_base maps
        self._returns(rew, don, self.ur_out[T * S:], self.ur_out, T, S, self.ur_returns, replayed=True)
        self._unreal_head_losses(net, self.ur_out, self.ur_returns, self.ur_dout, h_r, net.x4(self.ur_acts, cap),
                                 u["actions"], rew, don, rows[0], rows[0][T * S:], T, S, S, self.ur_dx4,
                                 self._merged_replay)
        # BPTT over the T + 1 replayed steps (value replay's dout + pixel control's dh), the trunk
        net.lstm_backward(self.params, T + 1, S, self.ur_dout, h_r, self.ur_xcat, self.ur_lacts, c_r, c0,
                          u["masks"], x5, self.ur_dz5, self.ur_grads, self.ur_lstm_ws, dh_extra=self.dh_pc,
                          extra_envs=S)
        net.backward_ex(self.params, frames, cap, self.ur_acts, cap, None, self.ur_dz5, self.ur_dx4, self.ur_grads,
                        self.ur_ws)

    def _side_grad_range(self):
        """[lo, hi) of the flat gradient the replayed UNREAL pass writes on the side stream: the
        pixel-control and reward-prediction blocks (include/vnav.h VN_POLICY_UNREAL layout),
        from the aux heads' block on when those run in the same pass (_merged_replay)."""
        lo = min(self.net.unreal_layout.values())
        if self._merged_replay:
            lo = min(lo, self.net.aux_layout["w1"])
        return lo, self.net.n_params

    def _side_owned(self):
        """(name, tensor) the side stream writes between the fork and the join."""
        lo, hi = self._side_grad_range()
        out = [(k, getattr(self, k)) for k in ("ur_acts", "ur_xcat", "ur_lacts", "ur_hc", "ur_gates", "ur_out",
                                               "ur_returns", "ur_dout", "ur_dz5", "ur_dx4", "ur_grads", "ur_ws",
                                               "ur_lstm_ws", "h_pc", "pcb", "pc_a1", "pc_p2", "dh_pc", "pc_ws",
                                               "rp_x", "rp_dx", "rp_out", "rp_dout", "unreal_stats")]
        out += [("ur_cur." + k, v) for k, v in self.ur_cur.items()]
        if self.rp_skewed:  # the sampler's outputs (rp_x / rp_dx above are slices of ur_acts / ur_dx4)
            out += [(k, getattr(self, k)) for k in ("ur_rows_ext", "rp_label", "rp_src", "rp_draw_stats")]
        if self._merged_replay:
            out += [(k, getattr(self, k)) for k in ("a1", "pred", "dpred", "aux_ws", "aux_stats")]
        out = [(k, t) for k, t in out if t is not None]  # (pc_a1: BigHouseModel's heads have no first layer)
        return out + [("grads[pc/rp]", self.grads[lo:hi])]

    def _main_owned(self):
        """(name, tensor) the main stream writes while the side stream runs."""
        lo, _ = self._side_grad_range()
        names = ("acts", "workspace", "dout", "returns", "stats", "out", "dz5", "dx4", "lstm_ws", "xcat", "lstm_acts",
                 "aux_acts", "aux_out", "aux_dz5", "aux_grads", "unreal_dx4", "norm_partial", "scalars", "_hc0", "h_all",
                 "c_all", "goal_list", "goal_run_length", "goal_count", "rewards_aug", "novelty_stats", "visit_seen")
        if not self._merged_replay:
            names += ("a1", "pred", "dpred", "aux_ws", "aux_stats")
        out = [(k, getattr(self, k)) for k in names if isinstance(getattr(self, k, None), torch.Tensor)]
        return out + [("grads[trunk/heads/lstm/aux]", self.grads[:lo])]

    def _check_side_stream_disjoint(self):
        """The replayed UNREAL pass runs on a side stream beside the A2C backward (update()); it
        is race-free only while (1) its gradient block [pc_w, P) lies past every block the main
        stream writes and past the range the join adds ([0, _ur_add_end)), and (2) no buffer it
        writes shares memory with a buffer the main stream writes. Raises RuntimeError naming
        the first overlap (debug check: VN_DEBUG_STREAMS=1 or trainer.debug_streams = True)."""
        lo, hi = self._side_grad_range()
        net = self.net
        main_end = max(b + net.shapes[k][0] for k, (_, b) in net.offsets.items() if net.shapes[k][0])
        if net.lstm:
            main_end = max(main_end, net.lstm["bhh"] + 2048)
        if net.aux_layout and not self._merged_replay:
            main_end = max(main_end, net.aux_layout["b2"] + 8)
        if main_end > lo or self._ur_add_end > lo:
            raise RuntimeError("side-stream gradient block [%d, %d) overlaps the main stream's blocks (end %d) or the "
                               "join range [0, %d)" % (lo, hi, main_end, self._ur_add_end))

        def span(t):
            a = t.data_ptr()
            return a, a + t.numel() * t.element_size()

        main = [(k, span(t)) for k, t in self._main_owned() if t.numel()]
        for ks, ts in self._side_owned():
            if not ts.numel():
                continue
            a0, a1 = span(ts)
            for km, (b0, b1) in main:
                if a0 < b1 and b0 < a1:
                    raise RuntimeError("side-stream buffer %s overlaps main-stream buffer %s" % (ks, km))

    def _stream(self):
        return _lib.stream_ptr(self.device)

    def _a2c_step_args(self, t):
        """vn_a2c_step of rollout step t: sample from out[t], write actions[t], the next step's
        (last action, last reward) * mask and mask (the bootstrap slots after the last step),
        the recurrent carries and the per-env episode statistics."""
        E, T = self.env.num_envs, self.num_steps
        sl = slice(t * E, (t + 1) * E)
        s = _lib.A2CStep()
        s.policy_out = self.out[sl].data_ptr()
        s.num_actions = self.A
        s.seed = vdist.rank_seed(self.seed, self.rank)
        s.counter_base_dev = self.sched.data_ptr() + 2 * self.sched.element_size()
        s.counter = t
        s.actions = self.actions[sl].data_ptr()
        if self.recurrent:
            s.prev_action = self.prev_action.data_ptr()
            s.prev_reward = self.prev_reward.data_ptr()
            s.prev_mask = self.prev_mask.data_ptr()
            s.lra_next = (self.lra[t + 1] if t + 1 < T else self.boot_lra).data_ptr()
            s.mask_next = (self.masks[t + 1] if t + 1 < T else self.boot_mask).data_ptr()
        s.episode_stats_env = self.stats_env.data_ptr()
        if self._fused_heads:  # the heads of h_t in the same launch (out[t] written there)
            w_off, b_off = self.net.offsets["head"]
            s.head_weight = self.params.data_ptr() + 4 * w_off
            s.head_bias = self.params.data_ptr() + 4 * b_off
            s.head_input = self.h_all[sl].data_ptr()
            s.head_out = self.out[sl].data_ptr()
        return s

    def _frames(self, img_rows, goal_rows):
        return frames_from_rows(self._arena, self._fb, img_rows, goal_rows)

    def current_lr(self):
        """LinearSchedule(7e-4, 0, max_time_steps) (experiments/thor_cached_auxiliary.py:37)."""
        frac = min(self.total_steps / self.max_time_steps, 1.0) if self.max_time_steps > 0 else 0.0
        return self.learning_rate * (1.0 - frac)

    def _policy_step(self, t, frames):
        """Forward of step t of the rollout into self.out[t*E:(t+1)*E]."""
        net, E, N = self.net, self.env.num_envs, self.num_steps * self.env.num_envs
        sl = slice(t * E, (t + 1) * E)
        goals = None
        if self.dedup_goals:  # step t's new goals: all at t = 0, else the envs done at t - 1
            P = _lib.ptr
            _lib.check(self.lib.vn_goal_runs_step(P(self.dones[t - 1]) if t else None,
                                                  P(self.goal_delta[t - 1]) if t else None, E,
                                                  P(self.goal_delta[t]), P(self.goal_list_step[t]),
                                                  P(self.goal_count[t:t + 1]), self._stream()), "vn_goal_runs_step")
            goals = self._goal_runs_step[t]
        if not self.recurrent:
            net.forward(self.params, frames, E, self.acts, N, t * E, self.out[sl], goals=goals)
            return
        # step 0's mask / last action-reward come from vn_a2c_rollout_begin, later steps' from
        # the env step before them
        net.forward(self.params, frames, E, self.acts, N, t * E, None, goals=goals)
        hp = self.h0 if t == 0 else self.h_all[(t - 1) * E:t * E]
        cp = self.c0 if t == 0 else self.c_all[(t - 1) * E:t * E]
        net.lstm_step(self.params, E, net.x5(self.acts, N)[sl], self.lra[t], self.masks[t], hp, cp, self.xcat[sl],
                      self.gates, self.lstm_acts[sl], self.c_all[sl], self.h_all[sl])
        if not self._fused_heads:
            net.heads(self.params, self.h_all[sl], E, self.out[sl])

    def _bootstrap(self, frames):
        net, E = self.net, self.env.num_envs
        if not self.recurrent:
            net.forward(self.params, frames, E, self.boot_acts, E, 0, self.boot_out)
            return
        T = self.num_steps
        net.forward(self.params, frames, E, self.boot_acts, E, 0, None)
        last = slice((T - 1) * E, T * E)
        net.lstm_step(self.params, E, net.x5(self.boot_acts, E), self.boot_lra, self.boot_mask, self.h_all[last],
                      self.c_all[last], self.boot_xcat, self.gates, self.boot_la, self.boot_c, self.boot_h)
        net.heads(self.params, self.boot_h, E, self.boot_out)

    def _rollout_begin(self):
        """One launch: the device schedule, step 0's frame rows (later steps' rows are written
        into their slots by the env step before them) and, recurrent, step 0's mask and
        [one_hot(a) | r] * m from the carried last action / reward / mask."""
        E, T, P, info, rec = self.env.num_envs, self.num_steps, _lib.ptr, self.env._info, self.recurrent
        _lib.check(self.lib.vn_a2c_rollout_begin(
            P(self.sched), P(self.lr_dev), ctypes.c_double(self.learning_rate), ctypes.c_double(self.max_time_steps),
            ctypes.c_int64(T * E * self.world), T, P(info["img_row"]), P(info["goal_row"]), P(self.rows_img),
            P(self.rows_goal), E, P(self.prev_action) if rec else None, P(self.prev_reward) if rec else None,
            P(self.prev_mask) if rec else None, self.A, P(self.masks) if rec else None, P(self.lra) if rec else None,
            self._stream()), "vn_a2c_rollout_begin")

    def _redirect_rows(self, t):
        """The arena rows of the frames step t emits go straight into step t + 1's slots (the last
        step's into the env's own info rows: the bootstrap and the next rollout read them there)."""
        E = self.env.num_envs
        if t + 1 < self.num_steps:
            nxt = slice((t + 1) * E, (t + 2) * E)
            self.env.set_row_outputs(self.rows_img[nxt], self.rows_goal[nxt])
        else:
            self.env.set_row_outputs(None, None)

    def rollout(self):
        env, lib = self.env, self.lib
        E, T = env.num_envs, self.num_steps
        info = env._info
        if self.expert:
            # slot 0 = the mask of the state this rollout starts from (the last step of the one
            # before, a reset or a restored checkpoint left it in the env's own buffer), and the
            # step count the schedule below computes this update's learning rate from
            self.expert_mask[0].copy_(info["optimal_mask"])
            self.expert_steps.copy_(self.sched[1:2])
        if self.returns_ex:  # the step count the shaping weight's anneal reads, as the expert's
            self.shape_steps.copy_(self.sched[1:2])
        if self.novelty:  # and the novelty weights' anneal
            self.novelty_steps.copy_(self.sched[1:2])
        self._rollout_begin()
        for t in range(T):
            sl = slice(t * E, (t + 1) * E)
            self._policy_step(t, self._frames(self.rows_img[sl], self.rows_goal[sl]))
            self._redirect_rows(t)
            if self.expert:  # the mask of the state this step leaves: step t + 1's label
                env.set_nav_mask_output(self.expert_mask[t + 1] if t + 1 < T else None)
            if self.shaping:  # this step's distances before and after it: slot t
                env.set_nav_progress_outputs(self.shape_dist[t, 0], self.shape_dist[t, 1])
            if self.novelty:  # this step's arrival cell and first-visit flag: slot t
                env.set_visit_outputs(self.visit_cell[t], self.visit_first[t], None)
            # one launch: the categorical draw from out[t] (Philox counter = updates * T + t from
            # the device schedule), the index-only env step, and the next step's recurrent
            # inputs, carries and episode statistics
            env.step_a2c(self._a2c_steps[t], self.rewards[t], self.dones[t], self.states)
        if self.shaping:  # steps outside a rollout (an evaluation) write the env's own buffers
            env.set_nav_progress_outputs(None, None)
        if self.novelty:
            env.set_visit_outputs(None, None, None)
        _lib.check(lib.vn_a2c_episode_stats(_lib.ptr(self.stats_env), E, _lib.ptr(self.episode_stats), self._stream()),
                   "vn_a2c_episode_stats")
        if self.nav_metrics:
            env.nav_episode_stats(out=self.nav_stats)
        # bootstrap value of the final observation
        self._bootstrap(self._frames(info["img_row"], info["goal_row"]))

    def update(self, batch=None):
        """One A2C update on the rollout just sampled (``batch`` from sample_training_batch;
        None = the trainer's own rollout buffers with the on-policy aux batch; with
        unreal_source='replay' the rollout is then pushed into the ring and a sequence drawn). With
        ppo_clip set: ppo_epochs epochs over the same rollout (_ppo_update)."""
        if self.ppo:
            return self._ppo_update()
        lib, net = self.lib, self.net
        E, T, A = self.env.num_envs, self.num_steps, self.A
        N = T * E
        st = self._stream()
        aux_batch = batch.get("auxiliary_batch") if batch is not None else None
        if batch is None and self.replay:
            # a bare rollout(): store it and draw this update's sequence now (the replayed aux
            # batch included, as sample_training_batch() would have)
            aux_batch = self._replay_push_and_sample()
        u_side = self.unreal and self.unreal_source == "replay"
        if u_side:
            # the replayed UNREAL pass reads the parameters and its own ring slot and writes its
            # own buffers and the pc / rp gradient blocks, which the A2C backward never touches:
            # it runs on a side stream from here; its trunk / heads / LSTM gradients are added
            # after the join below, in the unforked order
            if self.debug_streams:
                self._check_side_stream_disjoint()
            if self._unreal_inline:
                self._unreal_replay_losses()
            else:
                main = torch.cuda.current_stream(self.device)
                self._ev_u0.record(main)
                self._side_u.wait_event(self._ev_u0)
                with torch.cuda.stream(self._side_u):
                    self._unreal_replay_losses()
                    self._ev_u1.record(self._side_u)
        self._returns(self._return_rewards(), self.dones, self.boot_out, self.out, T, E, self.returns)
        if self.expert:  # the same launch shape, with the expert term: the update gains no launch
            _lib.check(lib.vn_a2c_loss_grad_expert(
                _lib.ptr(self.out), _lib.ptr(self.actions), _lib.ptr(self.returns), _lib.ptr(self.expert_mask), N, A,
                ctypes.c_float(self.value_coefficient), ctypes.c_float(self.entropy_coefficient),
                ctypes.c_float(self.pg_coefficient), ctypes.c_float(self.expert_weight), _lib.ptr(self.expert_steps),
                ctypes.c_int64(self.expert_anneal_steps), _lib.ptr(self.dout), _lib.ptr(self.stats),
                _lib.ptr(self.expert_stats), st), "vn_a2c_loss_grad_expert")
        else:
            _lib.check(lib.vn_a2c_loss_grad(_lib.ptr(self.out), _lib.ptr(self.actions), _lib.ptr(self.returns), N, A,
                                            ctypes.c_float(self.value_coefficient),
                                            ctypes.c_float(self.entropy_coefficient), _lib.ptr(self.dout),
                                            _lib.ptr(self.stats), st), "vn_a2c_loss_grad")
        dx4 = None
        unreal_dh = None
        if self._merged_replay:
            pass  # the aux heads run inside the replayed UNREAL pass (side stream)
        elif self.aux_weight > 0 and aux_batch is not None:
            # replayed sequence: its own trunk forward, the heads' loss and backward, and the
            # trunk backward of dL/dX4 alone into aux_grads (added after the main backward)
            self.aux_stats.zero_()
            af = self._frames(aux_batch.rows_img, aux_batch.rows_goal)
            net.forward(self.params, af, N, self.aux_acts, N, 0, None if self.recurrent else self.aux_out)
            net.aux_forward_loss_grad(self.params, self.aux_acts, N, N, self.a1, self.pred, self._aux_targets_replay,
                                      self.aux_weight, self.dpred, self.aux_stats, self.aux_ws)
            net.aux_backward(self.params, self.aux_acts, N, N, self.a1, self.dpred, self.grads, self.dx4, self.aux_ws)
            net.backward_ex(self.params, af, N, self.aux_acts, N, None, self.aux_dz5, self.dx4, self.aux_grads,
                            self.workspace)
        elif self.aux_weight > 0:  # deconv heads: forward, loss gradient, backward -> dL/dX4
            # (in line: a side stream measured slower — their persistent kernels size their grids
            # to the whole chip, so nothing runs beside them; DESIGN "Two streams in the update")
            self.aux_stats.zero_()
            dx4 = self._aux_heads_backward(N, self._aux_targets)
        if self.unreal and self.unreal_source == "rollout":  # after the aux heads: rp adds to their dX4
            S = self.unreal_S
            dx4 = self.dx4 if self.rp_into_aux else self.unreal_dx4
            self._unreal_head_losses(net, self.out, self.returns, self.dout, self.h_pc, net.x4(self.acts, N),
                                     self.actions, self.rewards, self.dones, self.rows_img, self.env._info["img_row"],
                                     T, E, S, dx4, self.rp_into_aux, h_src=(self.h_all, self.boot_h))
            unreal_dh = self.dh_pc[:T * S]
        goals = self._rollout_goal_runs(self.dones, T, E)
        self._backward(E, self._frames(self.rows_img, self.rows_goal), self._seq, goals, dx4, dh_extra=unreal_dh,
                       extra_envs=self.unreal_S if self.unreal else 0)
        if self.recurrent:  # (h, c) after the last step carry into the next rollout (one copy launch)
            self._carry_states()
        # the side passes' gradient sums: in the norm's first pass (vn_grad_norm_join) on one
        # rank with no override; before the all-reduce / the override's autograd otherwise
        joins = []
        if aux_batch is not None and not self._merged_replay:
            w, _ = self.net.offsets["conv1"]
            _, b = self.net.offsets["fc"]
            joins.append((self.aux_grads, w, b + self.net.shapes["fc"][0]))
        if u_side:
            if not self._unreal_inline:
                torch.cuda.current_stream(self.device).wait_event(self._ev_u1)
            joins.append((self.ur_grads, 0, self._ur_add_end))
        fuse_join = self.world == 1 and not self._custom_aux
        if not fuse_join:
            for g, lo, hi in joins:
                self.grads[lo:hi].add_(g[lo:hi])
            joins = []
        if self._custom_aux:
            loss, self.aux_losses = self.compute_auxiliary_loss(self.model_view(), batch, self.device)
            if loss is not None:
                g, = torch.autograd.grad(loss, self.model_view().params, allow_unused=True)
                if g is not None:
                    self.grads.add_(g)
        scale = self._allreduce_tail()
        if not joins:
            return self._optimizer_step(scale, False)
        (a0, lo0, hi0), (a1, lo1, hi1) = (joins + [(None, 0, 0)])[:2]
        _lib.check(lib.vn_grad_norm_join(_lib.ptr(self.grads), net.n_params, _lib.ptr(a0), lo0, hi0, _lib.ptr(a1), lo1,
                                         hi1, ctypes.c_float(scale), ctypes.c_float(self.max_gradient_norm),
                                         _lib.ptr(self.norm_partial), _lib.ptr(self.scalars), st), "vn_grad_norm_join")
        self._clipped_step(scale, False)

    def _rollout_goal_runs(self, dones, T, E):
        """The goal runs of a stored [T, E] rollout (run starts ascending, run lengths) from its
        ``dones``: one vn_goal_runs_rollout launch into the update's lists. Returns the GoalRuns
        for the policy's calls over its T * E rows; None, and no launch, where those take none."""
        if not self.dedup_goals:
            return None
        goals = self._goal_runs_update if E == self.env.num_envs else self._mb_goal_runs.get(E)
        if goals is not None:
            P = _lib.ptr
            _lib.check(self.lib.vn_goal_runs_rollout(P(dones), T, E, P(self.goal_list), P(self.goal_run_length),
                                                     P(self.goal_count[T:T + 1]), self._stream()),
                       "vn_goal_runs_rollout")
        return goals

    def _forward_stored(self, E, frames, seq, goals):
        """The stored rollout, or E of its envs, under the current parameters, into the rollout's
        own activation buffers and self.out: one trunk call over the T * E rows of ``frames``;
        recurrent, the T LSTM steps from seq's (h0, c0) over its stored lra and masks
        (lstm_sequence), then the heads. The activation store keeps its capacity of N rows."""
        net, T = self.net, self.num_steps
        n, N = T * E, T * self.env.num_envs
        if not self.recurrent:
            net.forward(self.params, frames, n, self.acts, N, 0, self.out, goals=goals)
            return
        net.forward(self.params, frames, n, self.acts, N, 0, None, goals=goals)
        net.lstm_sequence(self.params, T, E, net.x5(self.acts, N), seq["lra"], seq["masks"], seq["h0"], seq["c0"],
                          self.xcat, self.gates, self.lstm_acts, self.c_all, self.h_all)
        net.heads(self.params, self.h_all, n, self.out)

    def _aux_heads_backward(self, n, targets):
        """The deconv heads on the first n rows of the rollout's activations: forward with the loss
        gradient against ``targets`` (sums added to aux_stats), backward into their gradient
        blocks and self.dx4. Returns dx4; None, and no launch, without targets."""
        if targets is None:
            return None
        net, N = self.net, self.num_steps * self.env.num_envs
        net.aux_forward_loss_grad(self.params, self.acts, N, n, self.a1, self.pred, targets, self.aux_weight,
                                  self.dpred, self.aux_stats, self.aux_ws)
        net.aux_backward(self.params, self.acts, N, n, self.a1, self.dpred, self.grads, self.dx4, self.aux_ws)
        return self.dx4

    def _backward(self, E, frames, seq, goals, dx4, dh_extra=None, extra_envs=0):
        """self.dout and ``dx4`` (the heads' dL/dX4, None without) back through the T * E rows of
        ``frames`` in the rollout's activation buffers, into grads: recurrent, the LSTM backward
        from seq's c0 under its masks (``dh_extra``: pixel control's dL/dh of the first
        ``extra_envs`` envs) and the trunk backward of dz5; else the heads and trunk backward of dout."""
        net, T = self.net, self.num_steps
        n, N = T * E, T * self.env.num_envs
        if not self.recurrent:
            net.backward_ex(self.params, frames, n, self.acts, N, self.dout, None, dx4, self.grads, self.workspace,
                            goals=goals)
            return
        net.lstm_backward(self.params, T, E, self.dout, self.h_all, self.xcat, self.lstm_acts, self.c_all,
                          seq["c0"], seq["masks"], net.x5(self.acts, N), self.dz5, self.grads, self.lstm_ws,
                          dh_extra=dh_extra, extra_envs=extra_envs)
        # the heads + LSTM (+ aux heads) gradients are final here: at world > 1 their all-reduce
        # runs on RCCL's stream while the trunk backward runs on this one (no launch at world 1)
        self._allreduce_head_bucket()
        net.backward_ex(self.params, frames, n, self.acts, N, None, self.dz5, dx4, self.grads, self.workspace,
                        goals=goals)

    def _clipped_step(self, scale, gated):
        """One RMSprop or Adam step on the gradient the norm launch has measured (scalars: the clip
        factor), lr from the device schedule (== current_lr() of the host counters) and Adam's step
        count from the device: nothing of the host enters, so a captured update stays valid.
        ``gated``: the entry point that reads ppo_target_kl's stop flag and writes nothing once set."""
        P, c_float = _lib.ptr, ctypes.c_float
        name = "vn_%s_step_%s" % (self.optimizer, "gated" if gated else "dev")
        if self.optimizer == "adam":
            state = (P(self.exp_avg), P(self.exp_avg_sq))
            hyper = (P(self.adam_step), c_float(self.adam_betas[0]), c_float(self.adam_betas[1]),
                     c_float(self.adam_epsilon))
        else:
            state, hyper = (P(self.square_avg),), (c_float(self.rms_alpha), c_float(self.rms_epsilon))
        gate = (P(self.kl_gate),) if gated else ()
        _lib.check(getattr(self.lib, name)(P(self.params), P(self.grads), *state, self.net.n_params, c_float(scale),
                                           P(self.scalars), P(self.lr_dev), *hyper, *gate, self._stream()), name)

    def _optimizer_step(self, scale, gated):
        """The norm of the gradient just formed (times ``scale``, 1 / world) and one clipped step."""
        _lib.check(self.lib.vn_grad_norm(_lib.ptr(self.grads), self.net.n_params, ctypes.c_float(scale),
                                         ctypes.c_float(self.max_gradient_norm), _lib.ptr(self.norm_partial),
                                         _lib.ptr(self.scalars), self._stream()), "vn_grad_norm")
        self._clipped_step(scale, gated)

    @property
    def on_ppo_epoch(self):
        """None, or a callable(k) run after epoch k's optimiser step of a PPO update (eager mode
        only: a captured update has no host code between its launches)."""
        return self._on_ppo_epoch

    @on_ppo_epoch.setter
    def on_ppo_epoch(self, fn):
        if fn is not None and self.cuda_graph:
            raise ValueError("on_ppo_epoch runs host code between the epochs, which a captured hipGraph cannot "
                             "replay: use cuda_graph=False")
        self._on_ppo_epoch = fn

    @property
    def on_ppo_minibatch(self):
        """None, or a callable(k, m) run after the optimiser step of minibatch m of epoch k (with
        ppo_minibatches > 1; eager mode only, as on_ppo_epoch)."""
        return self._on_ppo_minibatch

    @on_ppo_minibatch.setter
    def on_ppo_minibatch(self, fn):
        if fn is not None and self.cuda_graph:
            raise ValueError("on_ppo_minibatch runs host code between the minibatches, which a captured hipGraph "
                             "cannot replay: use cuda_graph=False")
        self._on_ppo_minibatch = fn

    def _ppo_update(self):
        """ppo_epochs full-batch epochs of the clipped surrogate on the rollout just sampled
        (DESIGN.md "PPO epochs"). The returns, the behaviour policy's head outputs (out_old) and
        the advantage statistics are formed once and stay fixed. Epoch 0 runs on the rollout's own
        stored activations, as the A2C update does; every later epoch first re-forwards the stored
        rollout under the current parameters (_forward_stored: the backward consumes activations).
        After the loss-gradient launch each epoch is the A2C update's own chain (_aux_heads_backward,
        _backward, _optimizer_step). The carried (h, c) is the behaviour policy's: saved before the
        first re-forward, written into (h0, c0) after the last epoch, so c0 is the rollout's start
        state for every epoch's LSTM backward. No host value enters: the K epochs are captured in
        the update's one hipGraph. With ppo_minibatches > 1 the epochs are _ppo_minibatch_epochs';
        what is formed once here and the carry are the same. With ppo_target_kl every optimiser step
        has the KL check in front of it (_ppo_kl_gate, DESIGN.md "PPO target KL"): its buffers are
        zeroed here, and once it has fired the remaining epochs run their launches and change nothing."""
        lib, P, c_float = self.lib, _lib.ptr, ctypes.c_float
        E, T, A = self.env.num_envs, self.num_steps, self.A
        N = T * E
        st = self._stream()
        self._returns(self._return_rewards(), self.dones, self.boot_out, self.out, T, E, self.returns)
        self.out_old.copy_(self.out)
        if self.ppo_normalize_advantage:
            _lib.check(lib.vn_ppo_adv_stats(P(self.returns), P(self.out_old), N, A, c_float(_PPO_ADV_EPS), P(self.adv_stats),
                                            st), "vn_ppo_adv_stats")
        if self.recurrent:
            self._hc_last.copy_(self._hc_all.view(2, T, E, 512)[:, T - 1])
        if self.ppo_target_kl is not None:  # the stop is this update's own
            self.kl_gate.zero_()
            self.kl_dev.zero_()
        if self.ppo_minibatches > 1:
            self._ppo_minibatch_epochs()
            if self.recurrent:
                self._hc0.copy_(self._hc_last)
            return
        frames = self._frames(self.rows_img, self.rows_goal)
        # the rollout's goal runs, for every epoch's re-forward and backward alike
        goals = self._rollout_goal_runs(self.dones, T, E)
        gated = self.ppo_target_kl is not None
        for k in range(self.ppo_epochs):
            if k > 0:
                self._forward_stored(E, frames, self._seq, goals)
            if self._ppo_kl_gate(self.out, self.out_old, self.actions, N):
                break
            _lib.check(lib.vn_ppo_loss_grad(
                P(self.out), P(self.out_old), P(self.actions), P(self.returns),
                P(self.adv_stats) if self.ppo_normalize_advantage else None, N, A, c_float(self.ppo_clip),
                c_float(self.ppo_value_clip), c_float(self.value_coefficient), c_float(self.entropy_coefficient),
                P(self.dout), P(self.stats), P(self.ppo_stats), st), "vn_ppo_loss_grad")
            if self.aux_weight > 0:  # the deconv heads on the rollout batch, as the A2C update runs them
                self.aux_stats.zero_()
            self._backward(E, frames, self._seq, goals, self._aux_heads_backward(N, self._aux_targets))
            self._optimizer_step(1.0, gated)
            if self._on_ppo_epoch is not None:
                self._on_ppo_epoch(k)
        if self.recurrent:
            self._hc0.copy_(self._hc_last)

    def _ppo_kl_gate(self, out, out_old, actions, n):
        """The target-KL check in front of one optimiser step: vn_ppo_kl_gate over the step's own n
        samples, between the forward that produced ``out`` and the loss-gradient launch. Once it
        has fired, the gated optimiser steps of the update change nothing. Returns True only with
        ppo_kl_host_stop, when the host has read the flag and found it set: the caller then leaves
        its loops, which ends with the same bits as running them out."""
        if self.ppo_target_kl is None:
            return False
        P = _lib.ptr
        _lib.check(self.lib.vn_ppo_kl_gate(P(out), P(out_old), P(actions), n, self.A, ctypes.c_float(self._kl_limit),
                                           P(self.kl_gate), P(self.kl_dev), self._stream()), "vn_ppo_kl_gate")
        return self.ppo_kl_host_stop and bool(self.kl_gate[0].item())  # a 4-byte copy and a sync

    def _ppo_minibatch_epochs(self):
        """The epochs of a PPO update in ppo_minibatches = M shuffled minibatches of whole envs
        (DESIGN.md "PPO minibatches"). Per epoch one permutation of the envs, keyed by the update's
        counter (sched[2], read on the device); per minibatch one gather of its [T, Eb] sub-rollout
        into the compact buffers (self.mb), then the full-batch epoch's chain at Eb envs in the
        rollout's own activation buffers: _forward_stored from the gathered start states (epoch 0
        too: the rollout's stored activations are in the full-batch layout), loss gradient with the
        mean over the minibatch's own samples and the rollout's advantage statistics,
        _aux_heads_backward, _backward, _optimizer_step. The sums behind the metrics are cleared
        when an epoch begins and added to by its minibatches, so they end as the final epoch's over
        all N samples."""
        lib, P, c_float = self.lib, _lib.ptr, ctypes.c_float
        E, T, A, M = self.env.num_envs, self.num_steps, self.A, self.ppo_minibatches
        st = self._stream()
        mb, frames = self.mb, self._mb_frames
        counter = self.sched[2:3]
        gated = self.ppo_target_kl is not None
        stopped = False  # ppo_kl_host_stop: the host has seen the stop flag set
        for k in range(self.ppo_epochs):
            _lib.check(lib.vn_ppo_env_permutation(self._ppo_seed, P(counter), k, E, 32, P(self.ppo_perm), st),
                       "vn_ppo_env_permutation")
            self.stats.zero_()
            self.ppo_stats.zero_()
            if self.aux_weight > 0:
                self.aux_stats.zero_()
            for m in range(M):
                lo, eb = self.mb_bounds[m], self.mb_bounds[m + 1] - self.mb_bounds[m]
                nb = T * eb
                _lib.check(lib.vn_ppo_minibatch_gather(ctypes.byref(self._mb_src), ctypes.byref(self._mb_dst),
                                                       P(self.ppo_perm[lo:]), eb, T, E, A, st),
                           "vn_ppo_minibatch_gather")
                goals = self._rollout_goal_runs(mb["dones"], T, eb)  # from its gathered dones
                self._forward_stored(eb, frames, mb, goals)
                # the KL over the minibatch's own samples against its gathered out_old
                stopped = self._ppo_kl_gate(self.out, mb["out_old"], mb["actions"], nb)
                if stopped:
                    break
                _lib.check(lib.vn_ppo_loss_grad_acc(
                    P(self.out), P(mb["out_old"]), P(mb["actions"]), P(mb["returns"]),
                    P(self.adv_stats) if self.ppo_normalize_advantage else None, nb, A, c_float(self.ppo_clip),
                    c_float(self.ppo_value_clip), c_float(self.value_coefficient), c_float(self.entropy_coefficient),
                    P(self.dout), P(self.stats), P(self.ppo_stats), st), "vn_ppo_loss_grad_acc")
                # the deconv heads on the minibatch: targets by its gathered rows
                self._backward(eb, frames, mb, goals, self._aux_heads_backward(nb, self._mb_aux_targets))
                self._optimizer_step(1.0, gated)
                if self._on_ppo_minibatch is not None:
                    self._on_ppo_minibatch(k, m)
            if stopped:  # left inside epoch k: it did not finish, its hook does not run
                break
            if self._on_ppo_epoch is not None:
                self._on_ppo_epoch(k)

    def _buckets_split(self):
        """Two gradient buckets when the head bucket is final before the trunk backward:
        [head.w, P) = heads + LSTM + aux heads (flat layout, include/vnav.h), [0, head.w) =
        the conv / conv_merge trunk. One bucket otherwise (feed-forward nets compute heads and
        trunk in one call; a compute_auxiliary_loss override may touch every parameter)."""
        return (self.world > 1 and self.allreduce_buckets == 2 and self.recurrent and not self._custom_aux
                and self.unreal_source != "replay")  # the replayed UNREAL pass adds to head / LSTM grads later

    def _allreduce_head_bucket(self):
        self._head_work = None
        if not self._buckets_split():
            return
        hw, _ = self.net.offsets["head"]
        self._head_work = vdist.allreduce_async_(self.grads[hw:], self.group)

    def _allreduce_tail(self):
        """The remaining all-reduce (the trunk bucket, or the whole flat gradient) and the
        wait for the head bucket; returns the 1/world scale. With time_collectives the
        compute-stream time from here to the all-reduced gradient (the exposed, not
        overlapped, collective time) is recorded per update."""
        if self.world == 1:
            return 1.0
        ev = None
        if self.time_collectives:
            self._collect_pending()
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()
        if self._head_work is not None:
            hw, _ = self.net.offsets["head"]
            scale = vdist.allreduce_gradients_(self.grads[:hw], self.group)
            self._head_work.wait()
            self._head_work = None
        else:
            scale = vdist.allreduce_gradients_(self.grads, self.group)  # RCCL, one flat bucket
        if ev is not None:
            ev[1].record()
            self._coll_pending.append(ev)
        return scale

    def _collect_pending(self, wait=False):
        """Fold the completed event pairs into the running (sum, count): non-blocking unless
        ``wait`` or more than 8 pairs are pending, so the record stays bounded however long
        the run and the host does not stall behind the device."""
        keep = []
        for k, ev in enumerate(self._coll_pending):
            if wait or len(self._coll_pending) - k > 8 or ev[1].query():
                ev[1].synchronize()
                self._coll_sum_ms += ev[0].elapsed_time(ev[1])
                self._coll_count += 1
            else:
                keep.append(ev)
        self._coll_pending = keep

    def collective_ms(self):
        """Mean exposed all-reduce time per update (ms) over the updates since the last call
        (syncs on the last update's events); None when nothing was recorded."""
        self._collect_pending(wait=True)
        if not self._coll_count:
            return None
        ms = self._coll_sum_ms / self._coll_count
        self._coll_sum_ms, self._coll_count = 0.0, 0
        return ms

    def _carry_states(self):
        """(h0, c0) = (h, c) of the rollout's last step, both in one strided copy."""
        E, T = self.env.num_envs, self.num_steps
        self._hc0.copy_(self._hc_all.view(2, T, E, 512)[:, T - 1])

    def _update_metrics(self):
        """rollout + update; returns the device metric vector (metrics.metric_layout)."""
        batch, _ = self.sample_training_batch()
        if self.geo_curriculum is not None:  # the rollout's episodes decide the next rollout's level
            self.env.curriculum_advance()
            self.env.curriculum_state(out=self.cur_state)
        self.update(batch)
        N = self.num_steps * self.env.num_envs
        # the base segment [stats / N, grad norm, aux loss (sum of the per-head MSEs, trainer.py:51-54),
        # episode stats, the UNREAL losses' means] in one launch; / N is torch's tensor / scalar
        # (times the f32 reciprocal); the means are averaged over ranks too
        layout = self._metric_layout
        m = torch.empty(layout["base"][1], dtype=torch.float32, device=self.device)
        aux = self.aux_weight > 0
        P = _lib.ptr
        _lib.check(self.lib.vn_a2c_metrics_ex(P(self.stats), ctypes.c_float(np.float32(1.0) / np.float32(N)),
                                              P(self.scalars), P(self.aux_stats) if aux else None,
                                              P(self._aux_numel) if aux else None, P(self.episode_stats),
                                              P(self.unreal_stats) if self.unreal else None,
                                              P(self._unreal_norm) if self.unreal else None, P(m), self._stream()),
                   "vn_a2c_metrics_ex")
        vdist.reduce_metrics_(m, 6, self.group)
        if self.unreal and self.world > 1:
            m[9:] /= self.world
        # the segments that ride behind the kernel's in the same fetch, each formed at its turn
        f64, rsum = torch.float64, lambda t: vdist.reduce_metrics_(t, 0, self.group)  # summed over ranks
        tails = {
            "nav": lambda: [rsum(self.nav_stats.clone())],
            "expert": lambda: [rsum(self.expert_stats[:3].clone()), self.expert_stats[3:]],
            "curriculum": lambda: [self.cur_state[0].to(torch.float32).mean().reshape(1)],
            # the sums are exact in fp64 below 2^53: the vector turns fp64 here
            "shaping": lambda: [rsum(self.shape_stats[:2].to(f64)), self.shape_steps.to(f64)],
            # counts below 2^24: exact in either width (the vector's: fp64 behind the shaping sums)
            "rp_sampling": lambda: [rsum(self.rp_draw_stats.to(f64 if self.shaping else torch.float32))],
            # the bonus sums over ranks; the table is this rank's own (tables are not reduced)
            "novelty": lambda: [rsum(self.novelty_stats[:2].to(f64 if self.shaping else torch.float32)),
                                self.visit_seen[:1].to(f64 if self.shaping else torch.float32)],
        }
        if self.ppo:  # the final epoch's sums (fp32 sums of at most N terms; the vector's width)
            tails["ppo"] = lambda: [self.ppo_stats.to(f64 if self.shaping else torch.float32)]
        if self.ppo_target_kl is not None:  # steps allowed, stopped, the KL at the stop (0 when not stopped)
            wide = f64 if self.shaping else torch.float32
            tails["ppo_kl"] = lambda: [self.kl_gate.flip(0).to(wide), self.kl_dev[1:].to(wide)]
        for name in list(layout)[1:]:
            parts = tails[name]()
            m = torch.cat([m.to(parts[0].dtype)] + parts)
        assert m.numel() == sum(list(layout.values())[-1])  # the last segment's offset + width
        return m

    def _graph_update(self):
        """The update through a captured hipGraph: the first update runs eagerly (kernel
        attributes and occupancy caches are set up), the second is captured — capture
        records the launches without running them — and every update replays it."""
        gen = getattr(self.env, "config_generation", 0)
        if self._graph is not None and gen != self._graph_gen:
            # the env was reconfigured after capture (tables, schedule, curriculum, limits):
            # the graph's launches point at the old buffers and arguments — capture again
            self._graph, self._graph_out = None, None
        if self._graph is None:
            if self.num_updates == 0:
                return self._update_metrics()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._graph_out = self._update_metrics()
            self._graph, self._graph_gen = g, gen
        self._graph.replay()
        return self._graph_out

    def step(self, sync=True):
        """One rollout (num_steps x num_envs) + one update. Returns the metric dict
        (deep_rl log keys) as floats when sync, else as device tensors."""
        t0 = time.perf_counter()
        m = self._graph_update() if self.cuda_graph else self._update_metrics()
        N = self.num_steps * self.env.num_envs
        self.total_steps += N * self.world
        self.num_updates += 1
        if not sync:
            # a graph replay writes the same static tensor every update: hand out a copy
            return {"raw": m.clone() if self.cuda_graph else m}
        vals = m.tolist()
        seg = {name: vals[o:o + w] for name, (o, w) in self._metric_layout.items()}
        vl, al, ent, ret_mean, gnorm, aux_loss, eps, rsum, lsum = seg["base"][:9]
        unreal = dict(zip(("pc_loss", "rp_loss", "vr_loss"), seg["base"][9:]))  # empty without the UNREAL losses
        nav = {}
        if self.nav_metrics:
            n_ep, n_ok, spl_sum, _ = seg["nav"]
            nav = {"success_rate": n_ok / n_ep if n_ep else float("nan"),
                   "spl": spl_sum / n_ep if n_ep else float("nan")}
        expert, expert_term = {}, 0.0
        if self.expert:
            nlq, agree, valid, w = seg["expert"]
            expert = {"expert_loss": nlq / valid if valid else float("nan"),
                      "expert_agreement": agree / valid if valid else float("nan"), "expert_weight": w}
            expert_term = w * nlq / (N * self.world)  # w * expert_loss * valid / N
        cur = {"curriculum_level": seg["curriculum"][0]} if self.geo_curriculum is not None else {}
        shaping = {}
        if self.shaping:  # the mean shaping term per env step, formed in fp64 from the exact sums
            sb, sa, steps = seg["shaping"]
            w = self.shaping_weight_at(steps)
            shaping = {"shaping_reward": w * (sb - float(np.float32(self.shaping_gamma)) * sa) / (N * self.world),
                       "shaping_weight": w}
        rp = {}
        if self.rp_skewed:  # the ring's candidates by reward and this update's draws, summed over ranks
            rp = dict(zip(("rp_candidates_zero", "rp_candidates_nonzero", "rp_drawn_nonzero", "rp_drawn"),
                          seg["rp_sampling"]))
        novelty = {}
        if self.novelty:  # the mean bonus per env step, the share of first visits, this rank's covered states
            added, firsts, seen = seg["novelty"]
            novelty = {"novelty_bonus": added / (N * self.world), "first_visit_rate": firsts / (N * self.world),
                       "states_seen": seen}
        ppo = {}
        if self.ppo:  # the final epoch's means over the N samples
            ppo = dict(zip(("approx_kl", "clip_fraction", "ratio_mean", "value_clip_fraction"),
                           (x / N for x in seg["ppo"])))
        if self.ppo_target_kl is not None:
            # the optimiser steps the update took before the KL check fired (ppo_epochs *
            # ppo_minibatches when it did not). With ppo_kl_host_stop the loops end at the stop, so
            # approx_kl and the other sums above are those of the last epoch that ran (with
            # minibatches: of its minibatches that ran) instead of the final one's.
            ppo.update(zip(("ppo_steps", "kl_stopped", "kl_at_stop"), seg["ppo_kl"]))
        dt = time.perf_counter() - t0
        return {
            "step": self.total_steps, "updates": self.num_updates,
            "value_loss": vl, "action_loss": al, "entropy": ent,
            "loss": self.value_coefficient * vl + self.pg_coefficient * al - self.entropy_coefficient * ent +
            expert_term + (
                self.pc_weight * unreal["pc_loss"] + self.rp_weight * unreal["rp_loss"] +
                self.vr_weight * unreal["vr_loss"] if unreal else 0.0),
            "episodes": eps, "reward": rsum / eps if eps else float("nan"),
            "episode_length": lsum / eps if eps else float("nan"),
            "grad_norm": gnorm, "return_mean": ret_mean, "fps": N * self.world / dt,
            **({"aux_loss": aux_loss} if self.aux_weight > 0 else {}),
            **unreal,
            **nav,
            **expert,
            **cur,
            **shaping,
            **rp,
            **novelty,
            **ppo,
        }

    def run(self, log_every=10, logger=print):
        while self.total_steps < self.max_time_steps:
            metrics = self.step(sync=(self.num_updates % log_every == 0))
            if "raw" not in metrics and self.rank == 0 and logger:
                logger(metrics)
        return self

    _RECURRENT_STATE = ("h0", "c0", "prev_action", "prev_reward", "prev_mask")

    # off the update path: the functions of evaluation.py and checkpoint.py, which take the trainer
    evaluate = evaluation.evaluate
    evaluate_episodes = evaluation.evaluate_episodes
    _run_episodes = evaluation._run_episodes
    _rollout_greedy = evaluation._rollout_greedy
    state_dict = checkpoint.state_dict
    params_state_dict = checkpoint.params_state_dict
    load_params_state_dict = checkpoint.load_params_state_dict
    load_state_dict = checkpoint.load_state_dict
    _load_replay_state = checkpoint._load_replay_state


class RolloutBatch(dict):
    """A sampled batch (deep_rl's batch dict): the frame rows of every sample in the scene
    cache (time-major, row t*E + e) plus the trainer's rollout buffers; ``observations()``
    gathers the uint8 frames batch-first [E, T, H, W, 3] as the reference's wrappers
    deliver them (a device copy: only hooks that need pixels call it)."""

    def __init__(self, trainer, rows_img, rows_goal):
        super().__init__()
        self.trainer, self.rows_img, self.rows_goal = trainer, rows_img, rows_goal
        T, E = trainer.num_steps, trainer.env.num_envs
        self["actions"] = trainer.actions.view(T, E)
        self["rewards"] = trainer.rewards
        self["dones"] = trainer.dones

    def observations(self):
        tr = self.trainer
        T, E = tr.num_steps, tr.env.num_envs
        shape = tuple(tr.env.frame_shape)
        out = []
        for rows in (self.rows_img, self.rows_goal):
            dst = torch.empty((T * E,) + shape, dtype=torch.uint8, device=tr.device)
            _lib.check(tr.lib.vn_gather_rows(ctypes.c_void_p(tr._arena), int(tr._fb), _lib.ptr(rows), T * E,
                                             _lib.ptr(dst), tr._stream()), "vn_gather_rows")
            out.append(dst.view((T, E) + shape).transpose(0, 1))
        return tuple(out)
