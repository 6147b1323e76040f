"""What the navigation info costs per step: device time of step(out=) with nav_info off against
nav_info on (one more small launch after the step's own), in one process, routes alternating,
5 rounds of 1000 timed steps after 300 warm-up steps, one event pair around the timed launches,
actions generated beforehand. Three operating points:

  envs4096_scenes20    the bench's: 20 synthetic scenes, 4096 envs, 84x84
  envs32768_scenes20   the same scenes, 32768 envs
  envs4_172            4 envs of one 172x172 scene (the few-env regime, where a launch is the cost)

and the one-off vn_nav_enable time (tables of the 20 bench scenes built on the device, wall clock
around VectorEnv.set_nav_info, which synchronises). Prints one JSON line.

    python tools/nav_info_bench.py [--rounds 5] [--steps 1000] [--warmup 300]
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

SEED = 1000


def spread(xs):
    xs = sorted(xs)
    return {"min": xs[0], "median": float(np.median(xs)), "max": xs[-1], "runs": xs}


def time_route(nav, scenes, E, warmup, K, dev):
    """Device microseconds per step(out=): a fresh env, `warmup` steps, then K timed."""
    import vnav
    env = vnav.VectorEnv(scenes, E, seed=SEED, device=dev, nav_info=nav)
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
    stats = env.nav_episode_stats().tolist() if nav else None
    env.close()
    del env, out
    torch.cuda.empty_cache()
    return us, flags, stats


def time_enable(scenes, dev, rounds):
    """Wall-clock milliseconds of enabling nav on a context of `scenes` (build + first refresh)."""
    import vnav
    env = vnav.VectorEnv(scenes, 64, seed=SEED, device=dev)
    ms = []
    for _ in range(rounds):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        env.set_nav_info(True)
        torch.cuda.synchronize(dev)
        ms.append((time.perf_counter() - t0) * 1e3)
        env.set_nav_info(False)
    states = [s.n_states for s in scenes]
    env.close()
    return {"ms": spread(ms), "scenes": len(scenes), "states": states,
            "table_bytes": int(sum(2 * n * n for n in states))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--scenes", type=int, default=20)
    a = ap.parse_args()
    import vnav
    if not torch.cuda.is_available():
        raise SystemExit("nav_info_bench needs the GPU (no CPU timing)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    scenes = [vnav.synthetic_scene(k) for k in range(a.scenes)]
    big = [vnav.synthetic_scene(0, frame_shape=(172, 172, 3))]
    res = {"tool": "nav_info_bench", "unit": "us per step(out=) (device, one event pair)",
           "config": {"seed": SEED, "warmup": a.warmup, "steps": a.steps, "rounds": a.rounds}, "points": {}}
    flags = 0
    for name, sc, E in (("envs4096_scenes20", scenes, 4096), ("envs32768_scenes20", scenes, 32768),
                        ("envs4_172", big, 4)):
        us = {False: [], True: []}
        stats = None
        for _ in range(a.rounds):
            for nav in (False, True):
                t, f, st = time_route(nav, sc, E, a.warmup, a.steps, dev)
                us[nav].append(t)
                flags |= f
                stats = st or stats
        off, on = spread(us[False]), spread(us[True])
        res["points"][name] = {"envs": E, "scenes": len(sc), "frame": list(sc[0].frame_shape), "nav_off": off,
                               "nav_on": on, "nav_cost_us": on["median"] - off["median"],
                               "nav_stats_whole_run": stats}
    res["enable"] = time_enable(scenes, dev, a.rounds)
    res["error_flags"] = flags
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
