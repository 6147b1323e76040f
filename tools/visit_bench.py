"""What the state-visit counts and the novelty bonus cost, and what the bonus does on two small tasks.

--mode cost (default), in one process, variants alternating, 5 rounds after a warm-up, one event
pair around the timed launches:

  step    device time of step(out=) with visits off and on (one more launch) with 64, 8 and 1
          lanes per env (VN_VISIT_LANES: the thread mappings measured against each other), 1000
          timed steps after 300, at
            envs4096_scenes20   20 synthetic scenes (1344 states: 42 bitmap words), 4096 envs,
                                84x84 (the bench's)
            envs32768_scenes20  the same scenes, 32768 envs
            envs4_172           4 envs of one 172x172 scene (where a launch is the cost)
            envs4096_grid60     4096 envs of one 60x60-cell scene (the widest bitmap here)
          each with uniform starts and at the reset-heavy operating point of bench.py's short
          legs: set_hardness(0.01) and episodes cut at 2 steps, so about half the envs start an
          episode, and clear their bitmap, on every step
  update  device time of A2CTrainer.step() with the bonus off against on (novelty_weight=0.1,
          first_visit_weight=0.05), at
            envs4096_84_lstm    4096 envs, 84x84, LSTM, eager
            envs4_174_graph     4 envs, 174x174, LSTM, captured hipGraph

--mode learn: the expert test's setting (one 6x6 scene with one goal, 16 envs x 20 steps, 120
updates, feed-forward 84x84, limit 30) and one 24x24 synthetic scene with one goal (limit 200):
success rate of the finished episodes over the last 20 updates and the states seen after the last
update, with novelty weight 0 (visit counts on, no bonus) and with --weight, 3 seeds each.

Writes <out>/visit_bench.json or <out>/visit_learn.json and prints the same JSON line.

    python tools/visit_bench.py [--mode cost|learn] [--rounds 5] [--out DIR]
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
NOVELTY = dict(novelty_weight=0.1, first_visit_weight=0.05)
VARIANTS = ("off", "lanes64", "lanes8", "lanes1")


def spread(xs):
    xs = sorted(xs)
    return {"min": xs[0], "median": float(np.median(xs)), "max": xs[-1], "runs": xs}


def time_step(variant, scenes, E, short, warmup, K, dev):
    """Device microseconds per step(out=): a fresh env, `warmup` steps, then K timed. Returns
    also the share of envs that finished an episode per timed step."""
    import vnav
    env = vnav.VectorEnv(scenes, E, seed=SEED, device=dev, max_episode_steps=2 if short else 900)
    if short:
        env.set_hardness(0.01)
        env.reset()
    if variant != "off":
        os.environ["VN_VISIT_LANES"] = variant[len("lanes"):]
        try:
            env.set_visit_counts(True)
        finally:
            os.environ.pop("VN_VISIT_LANES", None)
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
    before = env.get_state()[5].to(torch.int64).sum()  # the episode counters
    ev0.record()
    for t in range(warmup, warmup + K):
        env.step(views[t], out=out)
    ev1.record()
    torch.cuda.synchronize(dev)
    us = ev0.elapsed_time(ev1) / K * 1e3
    resets = float(env.get_state()[5].to(torch.int64).sum() - before) / (K * E)
    flags = env.error_flags()
    env.close()
    del env, out
    torch.cuda.empty_cache()
    return us, resets, flags


def time_update(on, scenes, E, graph, warmup, K, dev):
    """Device milliseconds per A2CTrainer.step()."""
    import vnav
    env = vnav.VectorEnv(scenes, E, seed=SEED, device=dev)
    tr = vnav.A2CTrainer(env, recurrent=True, cuda_graph=graph, seed=1, **(NOVELTY if on else {}))
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
    res = {"tool": "visit_bench", "mode": "cost",
           "config": {"seed": SEED, "rounds": a.rounds, "steps": a.steps, "warmup": a.warmup, "updates": a.updates,
                      "update_warmup": a.update_warmup, "novelty": NOVELTY,
                      "reset_heavy": {"hardness": 0.01, "max_episode_steps": 2}},
           "step": {"unit": "us per step(out=) (device, one event pair)"},
           "update": {"unit": "ms per update (device, one event pair)"}}
    flags = 0
    big = [vnav.synthetic_scene(0, frame_shape=(172, 172, 3))]
    wide = [vnav.synthetic_scene(0, grid=60)]
    points = (("envs4096_scenes20", scenes, 4096), ("envs32768_scenes20", scenes, 32768), ("envs4_172", big, 4),
              ("envs4096_grid60", wide, 4096))
    for name, sc, E in points:
        if a.skip_32768 and E == 32768:
            continue
        for label, short in (("uniform", False), ("reset_heavy", True)):
            us = {v: [] for v in VARIANTS}
            resets = 0.0
            for _ in range(a.rounds):
                for v in VARIANTS:
                    t, resets, f = time_step(v, sc, E, short, a.warmup, a.steps, dev)
                    us[v].append(t)
                    flags |= f
            sp = {v: spread(us[v]) for v in VARIANTS}
            res["step"]["%s_%s" % (name, label)] = dict(
                sp, envs=E, frame=list(sc[0].frame_shape), states=[s.n_states for s in sc][:1],
                resets_per_env_step=resets,
                cost_us={v: sp[v]["median"] - sp["off"]["median"] for v in VARIANTS[1:]})
    points = (("envs4096_84_lstm", scenes, 4096, False, 1),
              ("envs4_174_graph", [vnav.synthetic_scene(0, frame_shape=(174, 174, 3))], 4, True, 10))
    for name, sc, E, graph, mult in points:
        ms = {False: [], True: []}
        for _ in range(a.rounds):
            for on in (False, True):
                ms[on].append(time_update(on, sc, E, graph, a.update_warmup, a.updates * mult, dev))
        off, on = spread(ms[False]), spread(ms[True])
        res["update"][name] = {"envs": E, "frame": list(sc[0].frame_shape), "cuda_graph": graph,
                               "updates_timed": a.updates * mult, "off": off, "novelty_on": on,
                               "cost_ms": on["median"] - off["median"]}
    res["error_flags"] = flags
    return res, "visit_bench.json"


def goal_far_from_walls(scene):
    """A fixed goal of a scene: the state whose mean shortest-path distance to the others is least."""
    spd = np.asarray(scene.spd, dtype=np.float64)
    spd = np.where(spd < 0, spd.max() + 1, spd)
    return int(spd.mean(axis=0).argmin())


def learn_run(task, seed, weight, updates, dev):
    import vnav
    if task == "grid6":
        scene, goal, limit = vnav.synthetic_scene(0, grid=6), 7, 30
    else:
        scene, limit = vnav.synthetic_scene(0, grid=24), 200
        goal = goal_far_from_walls(scene)
    env = vnav.VectorEnv([scene], 16, seed=seed + 1, device=dev, max_episode_steps=limit, visit_counts=True)
    env.set_tasks([(0, goal)])
    env.reset()
    env.clear_visits()
    tr = vnav.A2CTrainer(env, num_steps=20, seed=seed, max_time_steps=1e6, nav_metrics=True, novelty_weight=weight)
    ok = eps = 0.0
    for u in range(updates):
        tr.step()
        n_ep, n_ok = (float(x) for x in tr.nav_stats[:2].cpu())
        if u >= updates - 20:
            eps += n_ep
            ok += n_ok
    seen = int(env.visit_stats()[0])
    env.close()
    return ok / eps if eps else float("nan"), seen, scene.n_states


def learn(a, dev):
    res = {"tool": "visit_bench", "mode": "learn",
           "config": {"tasks": {"grid6": "synthetic_scene(0, grid=6), goal 7, limit 30",
                                "grid24": "synthetic_scene(0, grid=24), the most central goal, limit 200"},
                      "envs": 16, "num_steps": 20, "updates": a.learn_updates, "weight": a.weight, "seeds": [0, 1, 2],
                      "measure": "successes / finished episodes over the last 20 updates; states with a count > 0 "
                                 "after the last update"},
           "runs": {}}
    for task in ("grid6", "grid24"):
        res["runs"][task] = {}
        for w in (0.0, a.weight):
            rates, seen, n = [], [], 0
            for seed in (0, 1, 2):
                r, s, n = learn_run(task, seed, w, a.learn_updates, dev)
                rates.append(r)
                seen.append(s)
            res["runs"][task]["weight_%g" % w] = {"success_rate": rates, "states_seen": seen, "states": n}
    return res, "visit_learn.json"


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
    ap.add_argument("--skip-32768", action="store_true", help="leave the 32768-env point out (device memory)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "visits"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("visit_bench needs the GPU (no CPU timing)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res, name = cost(a, dev) if a.mode == "cost" else learn(a, dev)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, name), "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
