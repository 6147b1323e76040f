"""What the five-frame observation of AuxiliaryGraph-v0 costs per step: device time of three routes
to (image, goal, depth, segmentation, goal segmentation), in one process, alternating, 300 warm-up +
1000 timed steps, one event pair around the timed launches, actions generated beforehand:

  a  VN_AUX_OBS_GATHER=1: the two-frame step(out=) + three vn_gather_rows into fresh tensors
     (the form before vn_step_aux)
  b  step(out=) with five uint8 buffers: one vn_step_aux launch
  c  the same with obs_format = aux_format = "f32_chw"

at two operating points: 4096 envs, 84x84, 4 synthetic scenes with seeded random depth /
segmentation; and 4 envs at 172x172 on one oriented scene (the reference's own shape,
experiments/thor_cached_auxiliary.py). Also in the result: the frames each route executes per
launch, counted on the CPU from the oracle's rows (rows whose arena row changed), priced in bytes.
Writes profiles/aux_obs/aux_obs_bench.json and prints it as one JSON line.

    python tools/aux_obs_bench.py [--rounds 5] [--steps 1000] [--warmup 300]
    python tools/aux_obs_bench.py --count-cpu       # the executed-frame count only, no GPU
    python tools/aux_obs_bench.py --routes b --points big --rounds 1   # a short profiled run
"""
import argparse
import dataclasses
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "a2cat-vn-pytorch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

SEED = 1000
KEYS = ("image", "goal", "depth", "segmentation", "goal_segmentation")
NAMES = {"a": "a_step_plus_three_gathers", "b": "b_fused_u8", "c": "c_fused_f32_chw"}


def spread(xs):
    xs = sorted(xs)
    return {"min": xs[0], "median": float(np.median(xs)), "max": xs[-1], "runs": xs}


def with_aux(scene, seed):
    rng = np.random.RandomState(seed)
    H, W = scene.frame_shape[:2]
    return dataclasses.replace(scene, depth=rng.randint(0, 256, size=(scene.n_states, H, W, 1), dtype=np.uint8),
                               segmentation=rng.randint(0, 256, size=(scene.n_states, H, W, 3), dtype=np.uint8))


def scenes_of(point):
    """(scenes, envs, host frames wanted). big: 4 synthetic scenes of 84x84 (device-synthesised
    frames); ref: one 5x5 oriented scene of 172x172 random frames with one fixed goal."""
    import vnav
    if point == "big":
        return [with_aux(vnav.synthetic_scene(k), 50 + k) for k in range(4)], 4096
    rng = np.random.RandomState(7)
    maze = rng.rand(5, 5) > 0.2
    maze[0, 0] = True
    mk = lambda c: rng.randint(0, 256, size=(5, 5, 4, 172, 172, c), dtype=np.uint8)  # noqa: E731
    return [vnav.oriented_scene(maze, mk(3), [(0, 0, 1)], depths=mk(1), segmentations=mk(3))], 4


def time_route(route, scenes, E, warmup, K, dev):
    """Device microseconds per step of one route: a fresh env, `warmup` steps, then K timed."""
    import vnav
    fmt = "f32_chw" if route == "c" else "u8_hwc"
    env = vnav.VectorEnv(scenes, E, seed=SEED, device=dev, aux_observations=True, obs_format=fmt, aux_format=fmt)
    dtype = torch.float32 if route == "c" else torch.uint8
    out = dict(reward=torch.empty(E, dtype=torch.float32, device=dev), done=torch.empty(E, dtype=torch.bool, device=dev),
               state=torch.empty(E, dtype=torch.int32, device=dev),
               image=torch.empty((E,) + env.obs_shape, dtype=dtype, device=dev),
               goal=torch.empty((E,) + env.obs_shape, dtype=dtype, device=dev))
    if route != "a":
        for k, s in zip(KEYS[2:], env.aux_shapes):
            out[k] = torch.empty((E,) + s, dtype=dtype, device=dev)
    actions = torch.empty((warmup + K, E), dtype=torch.int32, device=dev)
    for t in range(warmup + K):
        env.random_actions(t, out=actions[t])
    views = list(actions.unbind(0))
    if route == "a":
        os.environ["VN_AUX_OBS_GATHER"] = "1"
    else:
        os.environ.pop("VN_AUX_OBS_GATHER", None)
    try:
        for t in range(warmup):
            env.step(views[t], out=out)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        ev0.record()
        for t in range(warmup, warmup + K):
            frames = env.step(views[t], out=out)[0]
        ev1.record()
        torch.cuda.synchronize(dev)
    finally:
        os.environ.pop("VN_AUX_OBS_GATHER", None)
    assert len(frames) == 5 and (route == "a") != (frames[2] is out.get("depth"))
    us = ev0.elapsed_time(ev1) / K * 1e3
    flags = env.error_flags()
    del env, out, frames
    torch.cuda.empty_cache()
    return us, flags


def count_rows_cpu(scenes, E, warmup, K):
    """Frames per launch each route executes in the timed window, from oracle.envs.VectorEnvOracle
    with RandomState(0) uniform actions (as tools/float_obs_bench.py --count-cpu), and their
    bytes (HW = pixels per frame): route a copies image / goal rows that changed (2 x 3 HW each)
    and gathers all three aux rows (2 x 7 HW per env); route b copies only changed rows of all five
    (depth HW and segmentation 3 HW with the image row, goal segmentation 3 HW with the goal row);
    route c reads the same rows and writes them as floats (5 bytes moved per element)."""
    from oracle import envs as oe
    sd = [dict(graph=s.graph, spd=s.spd, rewards=s.rewards, terminal_obs=s.terminal_obs) for s in scenes]
    tasks = [(i, g) for i, s in enumerate(scenes) for g in s.goals] if all(s.goals for s in scenes) else None
    o = oe.VectorEnvOracle(sd, E, SEED, max_steps=900, tasks=tasks)
    rng = np.random.RandomState(0)
    prev = o.observe()
    ci = cg = 0
    for t in range(warmup + K):
        r = o.step(rng.randint(0, 4, size=E).astype(np.int32))
        if t >= warmup:
            ci += int((r["img_row"] != prev["img_row"]).sum())
            cg += int((r["goal_row"] != prev["goal_row"]).sum())
        prev = r
    hw = int(np.prod(scenes[0].frame_shape[:2]))
    fi, fg = ci / (K * E), cg / (K * E)
    b_elems = fi * 7 * hw + fg * 6 * hw  # elements route b / c move per env-step
    return {"envs": E, "steps": [warmup, warmup + K], "img_rows_changed_frac": fi, "goal_rows_changed_frac": fg,
            "frames_per_launch": {"a": (fi + fg + 3) * E, "b": (3 * fi + 2 * fg) * E, "c": (3 * fi + 2 * fg) * E},
            "bytes_per_launch": {"a": (2 * 3 * hw * (fi + fg) + 2 * 7 * hw) * E, "b": 2 * b_elems * E,
                                 "c": 5 * b_elems * E},
            "model_b_over_a": 2 * b_elems / (2 * 3 * hw * (fi + fg) + 2 * 7 * hw)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--routes", default="abc")
    ap.add_argument("--points", default="big,ref", help="big: 4096 envs 84x84; ref: 4 envs 172x172")
    ap.add_argument("--count-cpu", action="store_true", help="only the executed-frame count (CPU oracle)")
    ap.add_argument("--no-count", action="store_true", help="skip the CPU count (a short profiled run)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "aux_obs", "aux_obs_bench.json"))
    a = ap.parse_args()
    points = [p for p in a.points.split(",") if p]
    res = {"tool": "aux_obs_bench", "unit": "us per step (device, one event pair)",
           "config": {"seed": SEED, "warmup": a.warmup, "steps": a.steps, "rounds": a.rounds}, "points": {}}
    if not a.count_cpu:
        if not torch.cuda.is_available():
            raise SystemExit("aux_obs_bench needs the GPU (no CPU timing)")
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
    routes = [r for r in "abc" if r in a.routes]
    flags = 0
    for point in points:
        scenes, E = scenes_of(point)
        pr = {"envs": E, "scenes": len(scenes), "frame": list(scenes[0].frame_shape)}
        if not a.count_cpu:
            us = {r: [] for r in routes}
            for _ in range(a.rounds):
                for r in routes:
                    t, f = time_route(r, scenes, E, a.warmup, a.steps, dev)
                    us[r].append(t)
                    flags |= f
            pr["routes"] = {NAMES[r]: spread(us[r]) for r in routes}
            if "a" in us:
                for r in routes:
                    if r != "a":
                        pr["ratio_%s_over_a" % r] = float(np.median(us[r]) / np.median(us["a"]))
        if not a.no_count:
            pr["cpu_count"] = count_rows_cpu(scenes, E, a.warmup, a.steps)
        res["points"][point] = pr
    res["error_flags"] = flags
    if not a.count_cpu and a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
