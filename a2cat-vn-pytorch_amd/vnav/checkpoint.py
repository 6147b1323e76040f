"""A2CTrainer's checkpoints, and the ordered table of per-env state that they and the fixed-episode
evaluation (evaluation.py) save and restore. Functions that take the trainer, off the update path."""
import warnings

import torch

# The envs' state in the order it must be restored, one row per kind: (checkpoint key, enabled for
# this trainer, the VectorEnv method that returns a fresh device table, the one that restores it).
# The states go first: set_state starts the progress record again from the states it sets and notes
# the restored envs' scenes for the curriculum, so those two tables go in after it.
ENV_STATE = (
    ("env_state", lambda tr: True, "get_state", "set_state"),
    ("env_ep_return", lambda tr: True, "get_episode_returns", "set_episode_returns"),
    ("env_nav", lambda tr: tr.nav_metrics, "get_nav_state", "set_nav_state"),
    ("env_curriculum", lambda tr: tr.geo_curriculum is not None, "curriculum_state", "set_curriculum_state"),
    ("env_nav_progress", lambda tr: tr.shaping, "get_nav_progress_state", "set_nav_progress_state"),
    # the visit table, the episode records and the seen bitmaps, whoever switched the counts on
    # (set_state has started every record again, uncounted)
    ("env_visits", lambda tr: getattr(tr.env, "visit_counts", False), "get_visit_state", "set_visit_state"),
)


def env_state(tr):
    """{key: device table} of the per-env state this trainer has, in ENV_STATE's order."""
    return {key: getattr(tr.env, get)() for key, enabled, get, _ in ENV_STATE if enabled(tr)}


def restore_env_state(tr, saved, missing=None):
    """Put env_state()'s tables back in ENV_STATE's order; ``missing(tr, key)`` stands in for a
    table this trainer has and ``saved`` lacks (None: KeyError)."""
    for key, enabled, _, put in ENV_STATE:
        if enabled(tr):
            if key == "env_nav_progress" and not tr.env.nav_progress:  # a set_nav_info on the way switched it off
                tr.env.set_nav_progress(True)
            if key in saved or missing is None:
                getattr(tr.env, put)(saved[key].to(tr.device))
            else:
                missing(tr, key)


def _without_env_table(tr, key):
    """load_state_dict on a checkpoint saved without one of this trainer's per-env tables."""
    env = tr.env
    if key == "env_nav":
        warnings.warn("checkpoint holds no navigation state (saved without nav_metrics): the running "
                      "episodes are measured from their current positions")
        env.set_nav_info(True)
        if tr.geo_curriculum is not None:  # set_nav_info switched it off
            env.set_geodesic_curriculum(**tr.geo_curriculum)
    elif key == "env_curriculum":
        warnings.warn("checkpoint holds no curriculum state (saved without geo_curriculum): every scene "
                      "starts from the configured level")
        env.set_geodesic_curriculum(**tr.geo_curriculum)
    elif key == "env_nav_progress":  # set_state has started the record from the restored states
        warnings.warn("checkpoint holds no progress state (saved without shaping_weight): the running "
                      "episodes' distances start from their current positions")
    elif key == "env_visits":  # set_state has started the records; the table keeps what it holds
        warnings.warn("checkpoint holds no visit state (saved without visit counts): the table is not "
                      "restored and the running episodes' coverage starts from their current positions")
    else:
        raise KeyError(key)


_ADAM_STATE = ("exp_avg", "exp_avg_sq", "adam_step")


def _adam_state(tr):
    """Adam's moments and step count of an optimizer='adam' trainer ({} otherwise)."""
    if getattr(tr, "optimizer", "rmsprop") != "adam":
        return {}
    return {k: getattr(tr, k).cpu() for k in _ADAM_STATE}


def _load_adam_state(tr, sd):
    """Adam's state from a checkpoint; one saved without it (an RMSprop run's) starts the moments
    and the step count at zero, with a warning."""
    if getattr(tr, "optimizer", "rmsprop") != "adam":
        return
    if all(k in sd for k in _ADAM_STATE):
        for k in _ADAM_STATE:
            getattr(tr, k).copy_(sd[k].to(tr.device))
        return
    warnings.warn("checkpoint holds no Adam state (saved with optimizer='rmsprop'): the moments and the step "
                  "count start at zero")
    for k in _ADAM_STATE:
        getattr(tr, k).zero_()


def state_dict(tr):
    sd = {"params": tr.params.detach().cpu(), "square_avg": tr.square_avg.cpu(),
          **{key: v.cpu() for key, v in env_state(tr).items()},
          "num_updates": tr.num_updates, "sched": tr.sched.cpu(),
          "total_steps": tr.total_steps, "seed": tr.seed, "rank": tr.rank, "world": tr.world, **_adam_state(tr)}
    if tr.recurrent:
        for k in tr._RECURRENT_STATE:
            sd[k] = getattr(tr, k).cpu()
    if tr.replay:  # the replay ring and its draw stream resume exactly
        sd["replay_rows"] = tr.replay_rows.cpu()
        sd["replay_meta"] = tr.replay_meta.cpu()  # next slot, filled, draw counter, drawn slot
        if tr.unreal_source == "replay":
            for key, v in tr.ur.items():
                sd["ur_" + key] = v.cpu()
    return sd


def params_state_dict(tr):
    """The world-agnostic part of the state: parameters, RMSprop state and the update /
    step counters (what a single-process ``test()`` needs after distributed training)."""
    return {"params": tr.params.detach().cpu(), "square_avg": tr.square_avg.cpu(),
            "num_updates": tr.num_updates, "total_steps": tr.total_steps, "sched": tr.sched.cpu(),
            "seed": tr.seed, "world": tr.world, "params_only": True, **_adam_state(tr)}


def load_params_state_dict(tr, sd):
    """Parameters (and RMSprop state, counters when present) of any world's checkpoint;
    the env state and recurrent carry of this trainer are left as they are."""
    if tuple(sd["params"].shape) != tuple(tr.params.shape):
        raise ValueError("checkpoint holds %d parameters, this policy has %d"
                         % (sd["params"].numel(), tr.params.numel()))
    tr.params.copy_(sd["params"].to(tr.device))
    if "square_avg" in sd:
        tr.square_avg.copy_(sd["square_avg"].to(tr.device))
    _load_adam_state(tr, sd)
    tr.num_updates = int(sd.get("num_updates", tr.num_updates))
    tr.total_steps = int(sd.get("total_steps", tr.total_steps))
    if "sched" in sd:
        tr.sched.copy_(sd["sched"].to(tr.device))


def load_state_dict(tr, sd):
    """Restore a state_dict() of this rank (env shard, running returns, recurrent carry
    are per rank; the env count must match)."""
    E = tr.env.num_envs
    if tuple(sd["env_ep_return"].shape) != (E,):
        raise ValueError("checkpoint holds %d envs, this trainer has %d" % (sd["env_ep_return"].shape[0], E))
    if "world" in sd and (int(sd["world"]), int(sd["rank"])) != (tr.world, tr.rank):
        raise ValueError("checkpoint of rank %d/%d loaded on rank %d/%d"
                         % (int(sd["rank"]), int(sd["world"]), tr.rank, tr.world))
    tr.params.copy_(sd["params"].to(tr.device))
    tr.square_avg.copy_(sd["square_avg"].to(tr.device))
    _load_adam_state(tr, sd)
    restore_env_state(tr, sd, missing=_without_env_table)
    if tr.expert:  # the env's own mask buffer = the restored states' masks (the next rollout's slot 0)
        tr.env.refresh_nav_outputs()
    tr.num_updates = int(sd["num_updates"])
    tr.total_steps = int(sd["total_steps"])
    if "sched" in sd:
        tr.sched.copy_(sd["sched"].to(tr.device))
    else:  # checkpoints from before the schedule was saved
        tr.sched.copy_(torch.tensor([tr.num_updates * tr.num_steps, tr.total_steps, 0], dtype=torch.int64))
    if tr.recurrent:
        for k in tr._RECURRENT_STATE:
            getattr(tr, k).copy_(sd[k].to(tr.device))
    if tr.replay:
        _load_replay_state(tr, sd)
    tr.env.observe(gather=False)


def _load_replay_state(tr, sd):
    """The replay ring of a checkpoint. The ring restarts empty (with a warning) when the
    checkpoint has no ring, a ring of another capacity, or no UNREAL record while this
    trainer replays the UNREAL losses (a checkpoint of aux-only replay or of
    unreal_source='rollout'): restoring the frame rows alone would draw slots whose UNREAL
    record is empty. Checkpoints from before the device-side ring (host draw stream,
    'replay_fill_pos') keep their slots; the draw stream restarts at counter 0."""
    ring = sd.get("replay_rows")
    need_ur = tr.unreal_source == "replay"
    why = None
    if ring is None:
        why = "the checkpoint holds no replay ring"
    elif tuple(ring.shape) != tuple(tr.replay_rows.shape):
        why = "the checkpoint's ring is %s, this trainer's %s" % (tuple(ring.shape), tuple(tr.replay_rows.shape))
    elif need_ur and any("ur_" + key not in sd for key in tr.ur):
        why = ("the checkpoint's ring holds no shaping distances (saved without shaping_weight)"
               if all("ur_" + key in sd for key in tr.ur if key != "shape_dist") else
               "the checkpoint has no UNREAL record in its ring (saved without unreal_source='replay')")
    if why is not None:
        warnings.warn("replay ring restarts empty: " + why)
        tr.replay_rows.zero_()
        tr.replay_meta.zero_()
        if need_ur:
            for v in tr.ur.values():
                v.zero_()
        return
    tr.replay_rows.copy_(ring.to(tr.device))
    if "replay_meta" in sd:
        tr.replay_meta.copy_(sd["replay_meta"].to(tr.device))
    else:
        pos_filled = [int(x) for x in sd["replay_fill_pos"]]
        tr.replay_meta.copy_(torch.tensor([pos_filled[1], pos_filled[0], 0, 0], dtype=torch.int64))
    if need_ur:
        for key, v in tr.ur.items():
            v.copy_(sd["ur_" + key].to(tr.device))
