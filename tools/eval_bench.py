"""What the fixed-episode evaluation costs (DESIGN.md "Fixed-episode evaluation"), in one process,
sides alternating, device time between one event pair around the timed launches:

  (a) step(out=) with nav_info on and the episode log off against the log on (every env records
      up to 64 episodes), `rounds` rounds of `steps` timed steps after `warmup` warm-up steps, at
        envs4096_scenes20   the bench's 20 synthetic scenes, 4096 envs, 84x84, time limit 30
        envs4_172           4 envs of one 172x172 scene (a launch is the cost), time limit 30
      With --parent-lib (a libvnav.so built from the parent commit) its nav_info step is a third
      side: the same kernel as the log-off side, so the two should lie inside one spread.
  (b) the one-off VectorEnv.sample_episodes (count, scan, draw; synchronises) on the largest
      bench scene: wall-clock ms for 4096 draws.
  (c) A2CTrainer.evaluate_episodes at 4096 envs (LSTM policy, 20 scenes, 128 episodes per scene
      and bucket, time limit 100): wall-clock seconds and episodes per second.

Prints one JSON line.

    python tools/eval_bench.py [--rounds 5] [--steps 1000] [--warmup 300] [--parent-lib PATH]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "a2cat-vn-pytorch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

SEED, LIMIT, CAP = 1000, 30, 64
NEW_SYMBOLS = ("vn_nav_sample_episodes", "vn_nav_set_episode_log")
_LIBS = {}


def use_lib(path):
    """Bind vnav to the library at `path` (None: the tree's own). A parent build lacks the new
    exports, so they are left out of the binding while it is in use."""
    from vnav import _lib
    if "own" not in _LIBS:
        _LIBS["own"] = (_lib.LIB_PATH, dict(_lib.SIGNATURES))
    own_path, sigs = _LIBS["own"]
    _lib.SIGNATURES.clear()
    _lib.SIGNATURES.update({k: v for k, v in sigs.items() if path is None or k not in NEW_SYMBOLS})
    _lib.LIB_PATH = own_path if path is None else path
    _lib._lib = None


def spread(xs):
    xs = sorted(xs)
    return {"min": xs[0], "median": float(np.median(xs)), "max": xs[-1], "runs": xs}


def time_route(side, lib, scenes, E, warmup, K, dev):
    """Device microseconds per step(out=): a fresh env, `warmup` steps, then K timed."""
    import vnav
    use_lib(lib if side == "parent" else None)
    env = vnav.VectorEnv(scenes, E, seed=SEED, device=dev, nav_info=True, max_episode_steps=LIMIT)
    log = env.set_episode_log(CAP, np.full(E, CAP)) if side == "log_on" else None
    out = dict(reward=torch.empty(E, dtype=torch.float32, device=dev),
               done=torch.empty(E, dtype=torch.bool, device=dev),
               state=torch.empty(E, dtype=torch.int32, device=dev),
               image=torch.empty((E,) + env.obs_shape, dtype=torch.uint8, device=dev),
               goal=torch.empty((E,) + env.obs_shape, dtype=torch.uint8, device=dev))
    actions = torch.empty((warmup + K, E), dtype=torch.int32, device=dev)
    for t in range(warmup + K):
        env.random_actions(t, out=actions[t])
    views = list(actions.unbind(0))
    for t in range(warmup):
        env.step(views[t], out=out)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    ev0.record()
    for t in range(warmup, warmup + K):
        env.step(views[t], out=out)
    ev1.record()
    torch.cuda.synchronize(dev)
    us = ev0.elapsed_time(ev1) / K * 1e3
    flags = env.error_flags()
    logged = int(torch.minimum(log.count, log.want).sum()) if log is not None else None
    env.close()
    del env, out
    torch.cuda.empty_cache()
    use_lib(None)
    return us, flags, logged


def time_sampler(scene, dev, rounds, count=4096):
    import vnav
    env = vnav.VectorEnv([scene], 64, seed=SEED, device=dev, nav_info=True)
    ms, total = [], 0
    for r in range(rounds + 1):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        _, _, total = env.sample_episodes(0, count, 4, 8, seed=r, salt=1)
        torch.cuda.synchronize(dev)
        if r:  # the first call loads the kernels
            ms.append((time.perf_counter() - t0) * 1e3)
    env.close()
    return {"ms": spread(ms), "states": scene.n_states, "draws": count, "pairs_4_8": total}


def time_evaluate(scenes, dev, rounds, E=4096, per_bucket=128, limit=100):
    import vnav
    env = vnav.VectorEnv(scenes, E, seed=SEED, device=dev, max_episode_steps=900)
    tr = vnav.A2CTrainer(env, num_steps=20, seed=SEED, recurrent=True, nav_metrics=True)
    eps = vnav.EpisodeSet.sample(env, per_bucket, seed=SEED)
    secs, res = [], None
    for r in range(rounds + 1):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        res = tr.evaluate_episodes(eps, max_episode_steps=limit, seed=r)
        if r:
            secs.append(time.perf_counter() - t0)
    env.close()
    s = spread(secs)
    return {"seconds": s, "episodes": len(eps), "episodes_per_s": len(eps) / s["median"], "envs": E,
            "time_limit": limit, "success_rate": res["success_rate"], "spl": res["spl"],
            "episode_length": res["episode_length"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--scenes", type=int, default=20)
    ap.add_argument("--parent-lib", default=None, help="libvnav.so of the parent commit: a third side of (a)")
    a = ap.parse_args()
    import vnav
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench needs the GPU (no CPU timing)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    scenes = [vnav.synthetic_scene(k) for k in range(a.scenes)]
    big = [vnav.synthetic_scene(0, frame_shape=(172, 172, 3))]
    sides = (("parent",) if a.parent_lib else ()) + ("log_off", "log_on")
    res = {"tool": "eval_bench", "unit": "us per step(out=) (device, one event pair)",
           "config": {"seed": SEED, "warmup": a.warmup, "steps": a.steps, "rounds": a.rounds, "time_limit": LIMIT,
                      "log_capacity": CAP, "parent_lib": bool(a.parent_lib)}, "points": {}}
    flags = 0
    for name, sc, E in (("envs4096_scenes20", scenes, 4096), ("envs4_172", big, 4)):
        us = {s: [] for s in sides}
        logged = None
        for _ in range(a.rounds):
            for side in sides:
                t, f, n = time_route(side, a.parent_lib, sc, E, a.warmup, a.steps, dev)
                us[side].append(t)
                flags |= f
                logged = n if n is not None else logged
        pt = {s: spread(us[s]) for s in sides}
        pt.update(envs=E, scenes=len(sc), frame=list(sc[0].frame_shape), episodes_logged=logged,
                  log_cost_us=pt["log_on"]["median"] - pt["log_off"]["median"])
        res["points"][name] = pt
    res["sample_episodes"] = time_sampler(max(scenes, key=lambda s: s.n_states), dev, a.rounds)
    res["evaluate_episodes"] = time_evaluate(scenes, dev, min(a.rounds, 3))
    res["error_flags"] = flags
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
