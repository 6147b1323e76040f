"""What float observations cost at the gym / VecEnv boundary: device time per step of three routes
to float32 [E,3,H,W] / 255 frames, in one process, alternating, at the bench's operating point
(20 synthetic scenes, 4096 envs, 84x84, seed 1000, TimeLimit 900, 300 warm-up + 1000 timed steps,
one event pair around the timed launches, actions generated beforehand):

  a  u8 step(out=) + vnav.to_float_chw on both frames (permute -> to(float32) -> / 255)
  b  u8 step(out=) + torch.div(x.permute(0, 3, 1, 2), 255, out=preallocated) on both frames
  c  VectorEnv(obs_format="f32_chw").step(out=): the conversion in the step's own launch

Route c also runs at 1024 envs / 1 scene and at 32768 envs / 20 scenes, and the float rows it
executes are counted (rows whose arena row changed, from an index-only run of the same
trajectory) and priced at 5 F bytes each (F read as u8, 4 F written as f32). Prints one JSON line.

    python tools/float_obs_bench.py [--rounds 5] [--steps 1000] [--warmup 300]
    python tools/float_obs_bench.py --count-cpu     # the row count from the CPU oracle, no GPU
"""
import argparse
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


def spread(xs):
    xs = sorted(xs)
    return {"min": xs[0], "median": float(np.median(xs)), "max": xs[-1], "runs": xs}


def scalar_bufs(E, dev):
    return dict(reward=torch.empty(E, dtype=torch.float32, device=dev),
                done=torch.empty(E, dtype=torch.bool, device=dev),
                state=torch.empty(E, dtype=torch.int32, device=dev))


def time_route(route, scenes, E, warmup, K, dev):
    """Device microseconds per step of one route: a fresh env, `warmup` steps, then K timed."""
    import vnav
    fmt = "f32_chw" if route == "c" else "u8_hwc"
    env = vnav.VectorEnv(scenes, E, seed=SEED, device=dev, obs_format=fmt)
    dtype = torch.float32 if route == "c" else torch.uint8
    out = dict(scalar_bufs(E, dev), image=torch.empty((E,) + env.obs_shape, dtype=dtype, device=dev),
               goal=torch.empty((E,) + env.obs_shape, dtype=dtype, device=dev))
    H, W, C = env.frame_shape
    pre = None
    if route == "b":
        pre = (torch.empty((E, C, H, W), dtype=torch.float32, device=dev),
               torch.empty((E, C, H, W), dtype=torch.float32, device=dev))
    actions = torch.empty((warmup + K, E), dtype=torch.int32, device=dev)
    for t in range(warmup + K):
        env.random_actions(t, out=actions[t])
    views = list(actions.unbind(0))

    def step(t):
        (img, goal), _, _, _ = env.step(views[t], out=out)
        if route == "a":
            return vnav.to_float_chw(img), vnav.to_float_chw(goal)
        if route == "b":
            torch.div(img.permute(0, 3, 1, 2), 255, out=pre[0])
            torch.div(goal.permute(0, 3, 1, 2), 255, out=pre[1])
            return pre
        return img, goal

    for t in range(warmup):
        step(t)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    ev0.record()
    for t in range(warmup, warmup + K):
        step(t)
    ev1.record()
    torch.cuda.synchronize(dev)
    us = ev0.elapsed_time(ev1) / K * 1e3
    flags = env.error_flags()
    del env, out, pre
    torch.cuda.empty_cache()
    return us, flags


def count_rows_device(scenes, E, warmup, K, dev):
    """Frames per step that route c converts in the timed window: rows whose arena row differs
    from the previous step's (index-only run of the same seed and actions)."""
    import vnav
    env = vnav.VectorEnv(scenes, E, seed=SEED, device=dev)
    prev = None
    changed = torch.zeros((), dtype=torch.int64, device=dev)
    for t in range(warmup + K):
        _, _, _, info = env.step(env.random_actions(t), gather=False)
        rows = torch.stack((info["img_row"], info["goal_row"]))
        if t >= warmup:
            changed += (rows != prev).sum()
        prev = rows
    return changed.item() / K


def count_rows_cpu(n_scenes, E, warmup, K):
    """The same count from oracle.envs.VectorEnvOracle with RandomState(0) uniform actions."""
    import vnav
    from oracle.envs import VectorEnvOracle
    scenes = [vnav.synthetic_scene(k) for k in range(n_scenes)]
    sd = [dict(graph=s.graph, spd=s.spd, rewards=s.rewards, terminal_obs=s.terminal_obs) for s in scenes]
    o = VectorEnvOracle(sd, E, SEED, max_steps=900)
    rng = np.random.RandomState(0)
    prev = o.observe()
    changed = [0, 0]
    for t in range(warmup + K):
        r = o.step(rng.randint(0, 4, size=E).astype(np.int32))
        if t >= warmup:
            changed[0] += int((r["img_row"] != prev["img_row"]).sum())
            changed[1] += int((r["goal_row"] != prev["goal_row"]).sum())
        prev = r
    F = int(np.prod(scenes[0].frame_shape))
    per_step = (changed[0] + changed[1]) / K
    return {"envs": E, "scenes": n_scenes, "steps": [warmup, warmup + K],
            "img_rows_changed_frac": changed[0] / (K * E), "goal_rows_changed_frac": changed[1] / (K * E),
            "frames_per_step": per_step, "bytes_per_launch": per_step * 5 * F}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--scenes", type=int, default=20)
    ap.add_argument("--routes", default="abc", help="routes to time, e.g. c for a short profiled run")
    ap.add_argument("--skip-other-configs", action="store_true", help="only the main operating point")
    ap.add_argument("--count-cpu", action="store_true", help="only count route c's rows with the CPU oracle")
    a = ap.parse_args()
    if a.count_cpu:
        print(json.dumps({"tool": "float_obs_bench", "cpu_count": count_rows_cpu(a.scenes, a.envs, a.warmup, a.steps)}))
        return
    import vnav
    if not torch.cuda.is_available():
        raise SystemExit("float_obs_bench needs the GPU (no CPU timing)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    scenes = [vnav.synthetic_scene(k) for k in range(a.scenes)]
    F = int(np.prod(scenes[0].frame_shape))
    names = {"a": "a_u8_step_plus_to_float_chw", "b": "b_u8_step_plus_div_out", "c": "c_f32_chw_step"}
    routes = [r for r in "abc" if r in a.routes]
    us = {r: [] for r in routes}
    flags = 0
    for _ in range(a.rounds):
        for route in routes:
            t, f = time_route(route, scenes, a.envs, a.warmup, a.steps, dev)
            us[route].append(t)
            flags |= f
    res = {"tool": "float_obs_bench", "unit": "us per step (device, one event pair)",
           "config": {"envs": a.envs, "scenes": a.scenes, "frame": list(scenes[0].frame_shape), "seed": SEED,
                      "warmup": a.warmup, "steps": a.steps, "rounds": a.rounds},
           "routes": {names[r]: spread(us[r]) for r in routes}}
    med = {k: float(np.median(v)) for k, v in us.items()}
    for r in routes:
        if r != "c" and "c" in med:
            res["speedup_c_over_" + r] = med[r] / med["c"]
    if "c" in med:
        frames = count_rows_device(scenes, a.envs, a.warmup, a.steps, dev)
        bytes_c = frames * 5 * F
        res["c_bytes"] = {"frames_per_step": frames, "bytes_per_launch": bytes_c,
                          "tb_per_s": bytes_c / (med["c"] * 1e-6) / 1e12}
    other = {}
    for name, n_sc, E in (() if a.skip_other_configs else
                          (("envs1024_scenes1", 1, 1024), ("envs32768_scenes20", a.scenes, 32768))):
        sc = scenes[:n_sc]
        runs = [time_route("c", sc, E, a.warmup, a.steps, dev)[0] for _ in range(2)]
        fr = count_rows_device(sc, E, a.warmup, a.steps, dev)
        other[name] = {"us": runs, "frames_per_step": fr, "bytes_per_launch": fr * 5 * F,
                       "tb_per_s": fr * 5 * F / (min(runs) * 1e-6) / 1e12}
    res["c_other_configs"] = other
    res["error_flags"] = flags
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
