"""An A2CTrainer's current policy evaluated on its own envs, with no update: deep_rl's Trainer.test()
and the fixed-episode evaluation (DESIGN.md "Fixed-episode evaluation"). Functions that take the
trainer, off the update path."""
import numpy as np
import torch

from . import _lib
from . import dist as vdist
from . import episodes as vep
from .checkpoint import env_state, restore_env_state

# the trainer's tensors that a fixed-episode evaluation's rollouts write, besides the recurrent carry
_TRAINER_STATE = ("sched", "lr_dev", "stats_env", "episode_stats", "nav_stats", "shape_steps",
                  "novelty_steps")


def evaluate(tr, episodes=10, max_rollouts=10000):
    """deep_rl's Trainer.test() on this trainer's envs: the current policy (sampled
    actions), no update, until ``episodes`` episodes have finished on all ranks together
    (or ``max_rollouts`` rollouts). The recurrent state carries across rollouts as in
    training; the learning-rate step count is left as it was. Returns the episode count
    and the mean reward and length of the finished episodes; with ``nav_metrics`` also
    their success rate, mean SPL and mean start distance (geodesic, in actions); with the
    expert term on also ``expert_agreement``, the share of the labelled samples whose
    sampled action starts a shortest path."""
    saved_sched = tr.sched.clone()  # sampling counter and step count: evaluation leaves both
    # the curriculum's counters see the rollouts below: levels, counters back afterwards
    saved_cur = tr.env.curriculum_state().clone() if tr.geo_curriculum is not None else None
    # and the visit counts: the table, the records and the seen-sets come back bit for bit
    # (meanwhile the table counts the evaluation alone: ``states_seen`` and ``coverage`` below)
    saved_visits = tr.env.get_visit_state() if getattr(tr.env, "visit_counts", False) else None
    if saved_visits is not None:
        tr.env.clear_visits()
    tot = torch.zeros(7 if tr.nav_metrics else 3, dtype=torch.float64)
    agree = torch.zeros(2, dtype=torch.float64)  # agreeing, labelled samples
    for _ in range(int(max_rollouts)):
        tr.rollout()
        if tr.recurrent:  # (h, c) after the last step carry on, as update() does
            tr._carry_states()
        st = tr.episode_stats.to(torch.float64)
        if tr.nav_metrics:
            st = torch.cat([st, tr.nav_stats.to(torch.float64)])
        vdist.reduce_metrics_(st, 0, tr.group)
        tot += st.cpu()
        if tr.expert:
            M = tr.expert_mask.view(-1).to(torch.int32) & ((1 << tr.A) - 1)
            hit = (M >> tr.actions) & 1
            ag = torch.stack([hit.sum(), (M != 0).sum()]).to(torch.float64)
            agree += vdist.reduce_metrics_(ag, 0, tr.group).cpu()
        if tot[0] >= episodes:
            break
    tr.sched.copy_(saved_sched)
    if saved_cur is not None:
        tr.env.set_curriculum_state(saved_cur)
    visits = {}
    if saved_visits is not None:  # this rank's: the tables are per rank and are not reduced
        seen = int(tr.env.visit_stats()[0])
        visits = {"states_seen": seen, "coverage": seen / sum(s.n_states for s in tr.env.scenes)}
        tr.env.set_visit_state(saved_visits)
    n, rsum, lsum = tot.tolist()[:3]
    out = {"episodes": n, "reward": rsum / n if n else float("nan"),
           "episode_length": lsum / n if n else float("nan"), **visits}
    if tr.nav_metrics:
        n_ep, n_ok, spl_sum, start_sum = tot.tolist()[3:]
        nan = float("nan")
        out.update(success_rate=n_ok / n_ep if n_ep else nan, spl=spl_sum / n_ep if n_ep else nan,
                   start_distance=start_sum / n_ep if n_ep else nan)
    if tr.expert:
        out["expert_agreement"] = float(agree[0] / agree[1]) if agree[1] else float("nan")
    return out


def _rollout_greedy(tr):
    """rollout() with the argmax action instead of the sampled one, composed of existing
    entry points: the forward, explicit heads, vn_policy_greedy, an index-only vn_step and
    vn_a2c_step_post. No statistics are kept: the evaluation reads the episode log."""
    env, lib, P = tr.env, tr.lib, _lib.ptr
    E, T, A, info = env.num_envs, tr.num_steps, tr.A, env._info
    tr._rollout_begin()
    scratch = torch.zeros(3, dtype=torch.float32, device=tr.device)
    for t in range(T):
        sl = slice(t * E, (t + 1) * E)
        tr._policy_step(t, tr._frames(tr.rows_img[sl], tr.rows_goal[sl]))
        if tr._fused_heads:  # the sampled step computes the heads itself
            tr.net.heads(tr.params, tr.h_all[sl], E, tr.out[sl])
        tr._redirect_rows(t)
        _lib.check(lib.vn_policy_greedy(P(tr.out[sl]), E, A, P(tr.actions[sl]), tr._stream()), "vn_policy_greedy")
        env.step(tr.actions[sl], out=dict(reward=tr.rewards[t], done=tr.dones[t], state=tr.states), gather=False)
        s = tr._a2c_steps[t]  # the sampled step's carries and next-step slots (NULL: not recurrent)
        _lib.check(lib.vn_a2c_step_post(
            P(tr.actions[sl]), P(tr.rewards[t]), P(tr.dones[t]), P(info["ep_return"]), P(info["ep_length"]), E, A,
            s.prev_action, s.prev_reward, s.prev_mask, s.lra_next, s.mask_next, P(scratch), tr._stream()),
            "vn_a2c_step_post")


def evaluate_episodes(tr, episode_set, policy="sample", max_episode_steps=None, seed=0):
    """Run every episode of ``episode_set`` (vnav.EpisodeSet) exactly once with the current
    policy and leave the trainer and its envs as they were. ``policy``: "sample" (the
    rollout's categorical draw) or "greedy" (argmax). ``max_episode_steps``: the time limit
    during the evaluation (default: the env's own; every episode must end, so there must be
    one). ``seed`` fixes the sampling counters: the same set, parameters and seed give the
    same results. Needs ``nav_metrics=True``.
    The episodes are placed statically on the envs (episodes.assign_episodes) and run by an
    exact-replay schedule; the results come from the per-episode log alone, so episodes an env
    runs after its list are never counted. At world > 1 every rank runs its share
    (episodes.world_slice); the sums are reduced over ranks, the per-episode arrays are this
    rank's (``index`` holds their positions in the set).
    Returns a dict: ``episodes``, ``success_rate``, ``spl``, ``episode_length``, ``reward``,
    ``start_distance`` over all episodes, ``buckets`` (a list of the same per distance
    bucket, with ``bucket`` = (lo, hi)), and ``per_episode`` (arrays ``index``, ``success``,
    ``length``, ``spl``, ``start_distance``, ``reward``)."""
    env = tr.env
    if not tr.nav_metrics:
        raise ValueError("evaluate_episodes needs A2CTrainer(nav_metrics=True)")
    if policy not in ("sample", "greedy"):
        raise ValueError('policy must be "sample" or "greedy", got %r' % (policy,))
    limit = int(env.max_episode_steps if max_episode_steps is None else max_episode_steps)
    if limit <= 0:
        raise ValueError("evaluate_episodes needs a time limit > 0: every episode must end")
    if len(episode_set) == 0:
        raise ValueError("the episode set is empty")
    episode_set.validate(env)
    index = vep.world_slice(len(episode_set), tr.rank, tr.world)
    per = {k: np.zeros(0, dtype=dt) for k, dt in (("success", bool), ("length", np.int32), ("spl", np.float32),
                                                  ("start_distance", np.int32), ("reward", np.float32))}
    if len(index):
        per = tr._run_episodes(episode_set.subset(index), policy, limit, int(seed))
    per["index"] = index
    # sums per bucket (the last row: all episodes), reduced over ranks in fp64
    nb = len(episode_set.buckets)
    bucket = episode_set.bucket[index]
    sums = np.zeros((nb + 1, 6), dtype=np.float64)
    for b in range(nb + 1):
        sel = np.ones(len(index), dtype=bool) if b == nb else bucket == b
        sums[b] = [sel.sum(), per["success"][sel].sum(), per["spl"][sel].astype(np.float64).sum(),
                   per["length"][sel].sum(), per["reward"][sel].astype(np.float64).sum(),
                   per["start_distance"][sel].sum()]
    if tr.world > 1:
        sums = vdist.reduce_metrics_(torch.as_tensor(sums, device=tr.device), 0, tr.group).cpu().numpy()

    def means(row):
        n = row[0]
        d = n if n else float("nan")
        return {"episodes": int(n), "success_rate": row[1] / d, "spl": row[2] / d, "episode_length": row[3] / d,
                "reward": row[4] / d, "start_distance": row[5] / d}
    out = means(sums[nb])
    out["buckets"] = [dict(means(sums[b]), bucket=episode_set.buckets[b]) for b in range(nb)]
    out["per_episode"] = per
    return out


def _run_episodes(tr, eps, policy, limit, seed):
    """evaluate_episodes on this rank's episodes: the per-episode arrays in their order."""
    env = tr.env
    E, T = env.num_envs, tr.num_steps
    env_scenes, ep_env, ep_slot, want, slots = vep.assign_episodes(eps.scene, E, len(env.scenes))
    # [E, slots, 2] (start, goal): an env's unused slots repeat a valid pair of its scene
    first = {int(k): int(np.nonzero(eps.scene == k)[0][0]) for k in np.unique(eps.scene)}
    pad = np.array([first[int(k)] for k in env_scenes])
    sched = np.stack([eps.start[pad], eps.goal[pad]], axis=1)[:, None, :].repeat(slots, axis=1).astype(np.int32)
    sched[ep_env, ep_slot, 0], sched[ep_env, ep_slot, 1] = eps.start, eps.goal
    # what the evaluation changes, saved
    torch.cuda.synchronize(tr.device)
    config = dict(schedule=env._schedule, env_scenes=env.env_scenes.copy(), limit=env.max_episode_steps)
    saved_env = env_state(tr)
    saved = {k: getattr(tr, k).clone() for k in _TRAINER_STATE + tr._RECURRENT_STATE if hasattr(tr, k)}
    try:
        env.set_env_scenes(env_scenes)
        env.set_max_episode_steps(limit)
        env.set_schedule(sched)
        log = env.set_episode_log(slots, want)
        _lib.check(tr.lib.vn_reset(env._ctx, None, env._stream()), "vn_reset")
        env.observe(gather=False)
        # the sampling counter base from the seed; carries and last action / reward / mask zero
        tr.sched.copy_(torch.tensor([(seed & 0xFFFFFFFF) << 20, int(saved["sched"][1]), 0], dtype=torch.int64))
        if tr.recurrent:
            for k in tr._RECURRENT_STATE:
                getattr(tr, k).zero_()
        bound = slots * limit + T
        steps = 0
        while True:
            if policy == "greedy":
                tr._rollout_greedy()
            else:
                tr.rollout()
            if tr.recurrent:
                tr._carry_states()
            steps += T
            if int(log.remaining()) == 0:  # one poll per rollout
                break
            if steps >= bound:
                raise RuntimeError("evaluate_episodes: %d episodes unfinished after %d steps (bound %d)"
                                   % (int(log.remaining()), steps, bound))
        g = (torch.as_tensor(ep_slot, device=tr.device), torch.as_tensor(ep_env, device=tr.device))
        per = {"success": log.success[g].cpu().numpy().astype(bool), "length": log.length[g].cpu().numpy(),
               "spl": log.spl[g].cpu().numpy(), "start_distance": log.start_distance[g].cpu().numpy(),
               "reward": log.ep_return[g].cpu().numpy()}
    finally:
        # everything back: configuration first, then the per-env state it would reset
        env.set_episode_log(None)
        env.set_schedule(config["schedule"])
        env.set_env_scenes(config["env_scenes"])
        env.set_max_episode_steps(config["limit"])
        restore_env_state(tr, saved_env)
        env.nav_episode_stats()  # the per-env accumulators of the surplus episodes: dropped
        env.refresh_nav_outputs()
        env.observe(gather=False)
        for k, v in saved.items():
            getattr(tr, k).copy_(v)
        torch.cuda.synchronize(tr.device)
    return per
