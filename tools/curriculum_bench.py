"""What the geodesic start curriculum costs: device time of step(out=) with nav info on against
the same with a fixed level (no launch added) and with an adaptive level (one count launch per
step, plus one curriculum_advance() per step here, the worst case: a trainer advances once per
rollout), in one process, routes alternating, 5 rounds of 1000 timed steps after 300 warm-up
steps, one event pair around the timed launches, actions generated beforehand. Two operating
points, those of tools/nav_info_bench.py:

  envs4096_scenes20    the bench's: 20 synthetic scenes, 4096 envs, 84x84
  envs4_172            4 envs of one 172x172 scene (the few-env regime, where a launch is the cost)

and the one-off table build (wall clock around VectorEnv.set_geodesic_curriculum on the 20 bench
scenes, which synchronises), next to the nav tables' own build. Writes
profiles/curriculum/curriculum_bench.json and prints the same JSON line.

    python tools/curriculum_bench.py [--rounds 5] [--steps 1000] [--warmup 300] [--out DIR]
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
ROUTES = ("nav", "fixed", "adaptive", "adaptive_advance")
ADAPT = dict(level=1, mode=1, window=64, up=0.8, down=0.3, step=1, level_min=1)


def spread(xs):
    xs = sorted(xs)
    return {"min": xs[0], "median": float(np.median(xs)), "max": xs[-1], "runs": xs}


def time_route(route, scenes, E, warmup, K, dev):
    """Device microseconds per step(out=): a fresh env, `warmup` steps, then K timed."""
    import vnav
    env = vnav.VectorEnv(scenes, E, seed=SEED, device=dev, nav_info=True)
    if route == "fixed":
        env.set_geodesic_curriculum(level=4)
    elif route != "nav":
        env.set_geodesic_curriculum(**ADAPT)
    advance = route == "adaptive_advance"
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
        if advance:
            env.curriculum_advance()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    ev0.record()
    for t in range(warmup, warmup + K):
        env.step(views[t], out=out)
        if advance:
            env.curriculum_advance()
    ev1.record()
    torch.cuda.synchronize(dev)
    us = ev0.elapsed_time(ev1) / K * 1e3
    flags = env.error_flags()
    state = env.curriculum_state().cpu().numpy().tolist() if route != "nav" else None
    env.close()
    del env, out
    torch.cuda.empty_cache()
    return us, flags, state


def time_enable(scenes, dev, rounds):
    """Wall-clock milliseconds of building the nav tables and, on top, the curriculum's."""
    import vnav
    env = vnav.VectorEnv(scenes, 64, seed=SEED, device=dev)
    nav_ms, cur_ms = [], []
    for _ in range(rounds):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        env.set_nav_info(True)
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        env.set_geodesic_curriculum(level=1)
        torch.cuda.synchronize(dev)
        t2 = time.perf_counter()
        nav_ms.append((t1 - t0) * 1e3)
        cur_ms.append((t2 - t1) * 1e3)
        D = env.curriculum_state().cpu().numpy()[3].tolist()
        env.set_nav_info(False)
    states = [s.n_states for s in scenes]
    env.close()
    return {"nav_ms": spread(nav_ms), "curriculum_ms": spread(cur_ms), "scenes": len(scenes), "states": states, "D": D,
            "order_bytes": int(sum(4 * n * n for n in states)),
            "count_bytes": int(sum(4 * n * (d + 2) for n, d in zip(states, D)))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--scenes", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "curriculum"))
    a = ap.parse_args()
    import vnav
    if not torch.cuda.is_available():
        raise SystemExit("curriculum_bench needs the GPU (no CPU timing)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    scenes = [vnav.synthetic_scene(k) for k in range(a.scenes)]
    big = [vnav.synthetic_scene(0, frame_shape=(172, 172, 3))]
    res = {"tool": "curriculum_bench", "unit": "us per step(out=) (device, one event pair)",
           "config": {"seed": SEED, "warmup": a.warmup, "steps": a.steps, "rounds": a.rounds, "adaptive": ADAPT},
           "points": {}}
    flags = 0
    for name, sc, E in (("envs4096_scenes20", scenes, 4096), ("envs4_172", big, 4)):
        us = {r: [] for r in ROUTES}
        last = {}
        for _ in range(a.rounds):
            for r in ROUTES:
                t, f, st = time_route(r, sc, E, a.warmup, a.steps, dev)
                us[r].append(t)
                flags |= f
                last[r] = st
        sp = {r: spread(us[r]) for r in ROUTES}
        res["points"][name] = dict(
            {"envs": E, "scenes": len(sc), "frame": list(sc[0].frame_shape)}, **sp,
            fixed_cost_us=sp["fixed"]["median"] - sp["nav"]["median"],
            adaptive_cost_us=sp["adaptive"]["median"] - sp["nav"]["median"],
            advance_cost_us=sp["adaptive_advance"]["median"] - sp["adaptive"]["median"],
            final_levels=last["adaptive_advance"][0])
    res["enable"] = time_enable(scenes, dev, a.rounds)
    res["error_flags"] = flags
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "curriculum_bench.json"), "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
