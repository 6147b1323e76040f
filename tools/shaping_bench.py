"""What geodesic reward shaping and GAE cost, and whether shaping helps a small task.

--mode cost (default), in one process, routes alternating, 5 rounds after a warm-up, one event pair
around the timed launches:

  step    device time of step(out=) with nav info on against nav info + progress (one more
          launch of one thread per env), 1000 timed steps after 300, at
            envs4096_scenes20   20 synthetic scenes, 4096 envs, 84x84 (the bench's)
            envs4_172           4 envs of one 172x172 scene (where a launch is the cost)
  update  device time of A2CTrainer.step() with shaping and GAE off against on
          (shaping_weight=0.5, annealed, gae_lambda=0.95), at
            envs4096_84_lstm    4096 envs, 84x84, LSTM, eager
            envs4_174_graph     4 envs, 174x174, LSTM, captured hipGraph

--mode learn: the expert test's setting (one 6x6 scene with one goal, 16 envs x 20 steps, 120
updates, feed-forward 84x84, limit 30): success rate of the finished episodes over the last 20
updates with shaping weight 0 and with --weight, 3 seeds each.

Writes <out>/shaping_bench.json or <out>/shaping_learn.json and prints the same JSON line.

    python tools/shaping_bench.py [--mode cost|learn] [--rounds 5] [--out DIR]
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
SHAPING = dict(shaping_weight=0.5, shaping_gamma=0.99, shaping_anneal_steps=10 ** 9, gae_lambda=0.95)


def spread(xs):
    xs = sorted(xs)
    return {"min": xs[0], "median": float(np.median(xs)), "max": xs[-1], "runs": xs}


def time_step(progress, scenes, E, warmup, K, dev):
    """Device microseconds per step(out=): a fresh env, `warmup` steps, then K timed."""
    import vnav
    env = vnav.VectorEnv(scenes, E, seed=SEED, device=dev, nav_info=True, nav_progress=progress)
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
    env.close()
    del env, out
    torch.cuda.empty_cache()
    return us, flags


def time_update(on, scenes, E, graph, warmup, K, dev):
    """Device milliseconds per A2CTrainer.step()."""
    import vnav
    env = vnav.VectorEnv(scenes, E, seed=SEED, device=dev)
    tr = vnav.A2CTrainer(env, recurrent=True, nav_metrics=True, cuda_graph=graph, seed=1, **(SHAPING if on else {}))
    for _ in range(warmup):
        tr.step(sync=False)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    ev0.record()
    for _ in range(K):
        tr.step(sync=False)
    ev1.record()
    torch.cuda.synchronize(dev)
    ms = ev0.elapsed_time(ev1) / K
    env.close()
    del tr, env
    torch.cuda.empty_cache()
    return ms


def cost(a, dev):
    import vnav
    scenes = [vnav.synthetic_scene(k) for k in range(20)]
    res = {"tool": "shaping_bench", "mode": "cost",
           "config": {"seed": SEED, "rounds": a.rounds, "steps": a.steps, "warmup": a.warmup, "updates": a.updates,
                      "update_warmup": a.update_warmup, "shaping": SHAPING},
           "step": {"unit": "us per step(out=) (device, one event pair)"},
           "update": {"unit": "ms per update (device, one event pair)"}}
    flags = 0
    big = [vnav.synthetic_scene(0, frame_shape=(172, 172, 3))]
    for name, sc, E in (("envs4096_scenes20", scenes, 4096), ("envs4_172", big, 4)):
        us = {False: [], True: []}
        for _ in range(a.rounds):
            for progress in (False, True):
                t, f = time_step(progress, sc, E, a.warmup, a.steps, dev)
                us[progress].append(t)
                flags |= f
        off, on = spread(us[False]), spread(us[True])
        res["step"][name] = {"envs": E, "frame": list(sc[0].frame_shape), "nav": off, "nav_progress": on,
                             "progress_cost_us": on["median"] - off["median"]}
    points = (("envs4096_84_lstm", scenes, 4096, False, 1),
              ("envs4_174_graph", [vnav.synthetic_scene(0, frame_shape=(174, 174, 3))], 4, True, 10))
    for name, sc, E, graph, mult in points:
        ms = {False: [], True: []}
        for _ in range(a.rounds):
            for on in (False, True):
                ms[on].append(time_update(on, sc, E, graph, a.update_warmup, a.updates * mult, dev))
        off, on = spread(ms[False]), spread(ms[True])
        res["update"][name] = {"envs": E, "frame": list(sc[0].frame_shape), "cuda_graph": graph,
                               "updates_timed": a.updates * mult, "off": off, "shaping_gae_on": on,
                               "cost_ms": on["median"] - off["median"]}
    res["error_flags"] = flags
    return res, "shaping_bench.json"


def learn_run(seed, weight, updates, dev):
    import vnav
    scene = vnav.synthetic_scene(0, grid=6)
    env = vnav.VectorEnv([scene], 16, seed=seed + 1, device=dev, max_episode_steps=30)
    env.set_tasks([(0, 7)])
    env.reset()
    tr = vnav.A2CTrainer(env, num_steps=20, seed=seed, max_time_steps=1e6, nav_metrics=True, shaping_weight=weight,
                         shaping_gamma=0.99)
    ok = eps = 0.0
    curve = []
    for u in range(updates):
        tr.step()
        n_ep, n_ok = (float(x) for x in tr.nav_stats[:2].cpu())
        curve.append([n_ep, n_ok])
        if u >= updates - 20:
            eps += n_ep
            ok += n_ok
    env.close()
    return ok / eps if eps else float("nan"), curve


def learn(a, dev):
    res = {"tool": "shaping_bench", "mode": "learn",
           "config": {"scene": "synthetic_scene(0, grid=6)", "task": [0, 7], "envs": 16, "num_steps": 20,
                      "updates": a.learn_updates, "limit": 30, "weight": a.weight, "shaping_gamma": 0.99,
                      "seeds": [0, 1, 2], "measure": "successes / finished episodes over the last 20 updates"},
           "runs": {}}
    for w in (0.0, a.weight):
        rates = []
        for seed in (0, 1, 2):
            r, _ = learn_run(seed, w, a.learn_updates, dev)
            rates.append(r)
        res["runs"]["weight_%g" % w] = {"success_rate": rates, "mean": float(np.mean(rates)),
                                        "spread": float(max(rates) - min(rates))}
    r0, r1 = res["runs"]["weight_0"], res["runs"]["weight_%g" % a.weight]
    res["gap"] = r1["mean"] - r0["mean"]
    res["seed_spread"] = max(r0["spread"], r1["spread"])
    res["gap_exceeds_3x_spread"] = bool(res["gap"] > 3 * res["seed_spread"])
    return res, "shaping_learn.json"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("cost", "learn"), default="cost")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--updates", type=int, default=30)
    ap.add_argument("--update-warmup", type=int, default=5)
    ap.add_argument("--learn-updates", type=int, default=120)
    ap.add_argument("--weight", type=float, default=0.1)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "shaping"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("shaping_bench needs the GPU (no CPU timing)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res, name = cost(a, dev) if a.mode == "cost" else learn(a, dev)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, name), "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
