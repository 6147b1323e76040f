"""What a PPO epoch costs beside the A2C update it repeats, Adam against RMSprop, and what K = 4
epochs do on one small task.

--mode cost (default), in one process, variants alternating, 5 rounds after a warm-up, one event
pair around the timed updates: device time of A2CTrainer.step() (rollout + update) for
  a2c        the trainer built without the new arguments (the parent commit's update, bit for bit)
  ppo1/2/4   ppo_clip=0.2 with 1, 2 and 4 epochs (RMSprop)
  a2c_adam   the A2C update with optimizer="adam"
at
  envs4096_84_lstm    4096 envs, 84x84, LSTM, eager
  envs4_174_graph     4 envs, 174x174, LSTM, captured hipGraph
and from the medians: ppo1 - a2c (the loss-gradient launch, the copy of out and the advantage
statistics), the cost of one extra epoch ((ppo4 - ppo1) / 3 and ppo2 - ppo1), and that cost as a
share of the A2C step.

--mode learn: the expert test's setting (one 6x6 scene with one goal, 16 envs x 20 steps, 120
updates, feed-forward 84x84, limit 30, the seeds of shaping_bench / visit_bench): success rate of
the finished episodes over the last 20 updates and their number, A2C against PPO K = 4 (RMSprop at
the same learning rate, and Adam), 3 seeds each.

--minibatches M [M ...] (DESIGN.md "PPO minibatches"): the same two modes on the minibatch split.
cost: PPO with 1 and 4 epochs at every M given (4096 envs; the 4-env batch at M = 1 and 2), variants
alternating as above; from the medians the cost of one minibatch step, (K4 - K1) / (3 M), beside
1 / M of a full-batch epoch, and the back-to-back launch intervals of vn_ppo_env_permutation and
vn_ppo_minibatch_gather on their own. learn: PPO K = 4 with Adam at every M given. Writes
<out>/ppo_minibatch_bench.json or <out>/ppo_minibatch_learn.json (default <out>:
profiles/ppo_minibatch).

--target-kl KL [KL ...] (DESIGN.md "PPO target KL"): the same two modes on the target-KL stop.
cost: PPO K = 4 at M = 1 and 4 without the argument (the parent commit's update, bit for bit) and
with ppo_target_kl at every KL given (give one that never fires, as 1e30, for the cost of the gate
itself), at both points, variants alternating as above; and, at 4096 envs M = 1, a target of 1e-30,
which fires at epoch 1's check, in the gated form and with ppo_kl_host_stop: what leaving the loops
saves. learn: PPO K = 4, M = 4 with RMSprop and with Adam, without a target and at every KL given;
beside the success rate the last update's clip_fraction and the mean ppo_steps over the run. Writes
<out>/ppo_kl_bench.json or <out>/ppo_kl_learn.json (default <out>: profiles/ppo_kl).

Writes <out>/ppo_bench.json or <out>/ppo_learn.json and prints the same JSON line.

    python tools/ppo_bench.py [--mode cost|learn] [--minibatches M [M ...]] [--target-kl KL [KL ...]]
                              [--rounds 5] [--out DIR]
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
VARIANTS = {"a2c": {}, "ppo1": dict(ppo_clip=0.2, ppo_epochs=1), "ppo2": dict(ppo_clip=0.2, ppo_epochs=2),
            "ppo4": dict(ppo_clip=0.2, ppo_epochs=4), "a2c_adam": dict(optimizer="adam")}


def spread(xs):
    xs = sorted(xs)
    return {"min": xs[0], "median": float(np.median(xs)), "max": xs[-1], "runs": xs}


def time_update(kw, scenes, E, graph, warmup, K, dev):
    """Device milliseconds per A2CTrainer.step()."""
    import vnav
    env = vnav.VectorEnv(scenes, E, seed=SEED, device=dev)
    tr = vnav.A2CTrainer(env, recurrent=True, cuda_graph=graph, seed=1, **kw)
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


def launch_intervals(dev, calls=200):
    """Microseconds per call of the two minibatch launches on their own, back to back on one
    stream between one event pair (an interval, not a kernel time: it cannot go below the
    launch rate)."""
    import ctypes

    from vnav import _lib
    from vnav.policy import OUT_LD
    lib, P, st = _lib.load(), _lib.ptr, _lib.stream_ptr(dev)
    T, E, A = 20, 4096, 4
    i32, f32 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float32, device=dev)
    ctr = torch.zeros(1, dtype=torch.int64, device=dev)
    perm = torch.zeros(E, **i32)

    def timed(fn):
        for _ in range(10):
            fn()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        ev0.record()
        for _ in range(calls):
            fn()
        ev1.record()
        torch.cuda.synchronize(dev)
        return ev0.elapsed_time(ev1) * 1000.0 / calls

    out = {"unit": "us per call, %d calls back to back" % calls, "T": T, "E": E}
    for n in (4096, 32768):
        big = torch.zeros(n, **i32)
        out["env_permutation_E%d" % n] = timed(lambda: _lib.check(
            lib.vn_ppo_env_permutation(1, P(ctr), 0, n, 32, P(big), st), "vn_ppo_env_permutation"))
    _lib.check(lib.vn_ppo_env_permutation(1, P(ctr), 0, E, 32, P(perm), st), "vn_ppo_env_permutation")

    def bufs(envs):
        n = T * envs
        return dict(rows_img=torch.zeros(n, **i32), rows_goal=torch.zeros(n, **i32), actions=torch.zeros(n, **i32),
                    returns=torch.zeros(n, **f32), out_old=torch.zeros((n, OUT_LD), **f32),
                    dones=torch.zeros(n, dtype=torch.bool, device=dev), masks=torch.zeros(n, **f32),
                    lra=torch.zeros((n, A + 1), **f32), h0=torch.zeros((envs, 512), **f32),
                    c0=torch.zeros((envs, 512), **f32))

    src = bufs(E)
    s = _lib.PpoRollout(**{k: v.data_ptr() for k, v in src.items()})
    for M in (4, 16):
        eb = E // M
        dst = bufs(eb)
        d = _lib.PpoRollout(**{k: v.data_ptr() for k, v in dst.items()})
        out["minibatch_gather_M%d" % M] = timed(lambda: _lib.check(
            lib.vn_ppo_minibatch_gather(ctypes.byref(s), ctypes.byref(d), P(perm), eb, T, E, A, st),
            "vn_ppo_minibatch_gather"))
    return out


def cost_minibatches(a, dev):
    import vnav
    K = 4
    res = {"tool": "ppo_bench", "mode": "cost", "minibatches": a.minibatches,
           "config": {"seed": SEED, "rounds": a.rounds, "updates": a.updates, "update_warmup": a.update_warmup,
                      "epochs": [1, K]},
           "update": {"unit": "ms per A2CTrainer.step() (device, one event pair)"}}
    points = (("envs4096_84_lstm", [vnav.synthetic_scene(k) for k in range(20)], 4096, False, 1,
               sorted(set(a.minibatches) | {1})),
              ("envs4_174_graph", [vnav.synthetic_scene(0, frame_shape=(174, 174, 3))], 4, True, 10, [1, 2]))
    for name, sc, E, graph, mult, Ms in points:
        variants = {"k%d_m%d" % (k, M): dict(ppo_clip=0.2, ppo_epochs=k, ppo_minibatches=M) for M in Ms for k in (1, K)}
        ms = {v: [] for v in variants}
        for _ in range(a.rounds):
            for v, kw in variants.items():
                ms[v].append(time_update(kw, sc, E, graph, a.update_warmup, a.updates * mult, dev))
        sp = {v: spread(ms[v]) for v in variants}
        med = {v: sp[v]["median"] for v in variants}
        full_epoch = (med["k%d_m1" % K] - med["k1_m1"]) / (K - 1)  # one re-forwarding full-batch epoch
        derived = {}
        for M in Ms:
            if M == 1:
                continue
            step = (med["k%d_m%d" % (K, M)] - med["k1_m%d" % M]) / ((K - 1) * M)
            derived["m%d" % M] = {
                "k4_minus_full_batch_k4_ms": med["k%d_m%d" % (K, M)] - med["k%d_m1" % K],
                "minibatch_step_ms": step, "full_batch_epoch_over_m_ms": full_epoch / M,
                "regime_gap_ms": step - full_epoch / M, "epoch_ms": step * M,
                "epoch_over_full_batch_epoch": step * M / full_epoch}
        res["update"][name] = dict(sp, envs=E, frame=list(sc[0].frame_shape), cuda_graph=graph,
                                   updates_timed=a.updates * mult, full_batch_epoch_ms=full_epoch, derived=derived)
    res["launches"] = launch_intervals(dev)
    return res, "ppo_minibatch_bench.json"


def cost_target_kl(a, dev):
    import vnav
    K, Ms = 4, (1, 4)
    res = {"tool": "ppo_bench", "mode": "cost", "target_kl": a.target_kl,
           "config": {"seed": SEED, "rounds": a.rounds, "updates": a.updates, "update_warmup": a.update_warmup,
                      "epochs": K, "minibatches": list(Ms), "stop_target": 1e-30},
           "update": {"unit": "ms per A2CTrainer.step() (device, one event pair)"}}
    points = (("envs4096_84_lstm", [vnav.synthetic_scene(k) for k in range(20)], 4096, False, 1),
              ("envs4_174_graph", [vnav.synthetic_scene(0, frame_shape=(174, 174, 3))], 4, True, 10))
    for name, sc, E, graph, mult in points:
        variants = {}
        for M in Ms:
            base = dict(ppo_clip=0.2, ppo_epochs=K, ppo_minibatches=M)
            variants["k4_m%d" % M] = base
            for kl in a.target_kl:
                variants["k4_m%d_kl%g" % (M, kl)] = dict(base, ppo_target_kl=kl)
        if not graph:  # the stop at epoch 1 of 4: every launch still run, against leaving the loops
            stop = dict(ppo_clip=0.2, ppo_epochs=K, ppo_target_kl=1e-30)
            variants["k4_m1_stop_gated"] = stop
            variants["k4_m1_stop_host"] = dict(stop, ppo_kl_host_stop=True)
        ms = {v: [] for v in variants}
        for r in range(a.rounds):
            for v, kw in variants.items():
                ms[v].append(time_update(kw, sc, E, graph, a.update_warmup, a.updates * mult, dev))
                print("%s round %d %s: %.3f ms" % (name, r, v, ms[v][-1]), file=sys.stderr, flush=True)
        sp = {v: spread(ms[v]) for v in variants}
        med = {v: sp[v]["median"] for v in variants}
        derived = {}
        for M in Ms:
            off = "k4_m%d" % M
            for kl in a.target_kl:
                on = "k4_m%d_kl%g" % (M, kl)
                derived[on] = {"gate_cost_ms": med[on] - med[off],
                               "by_round": [x - y for x, y in zip(ms[on], ms[off])],
                               "off_spread_ms": sp[off]["max"] - sp[off]["min"]}
        if not graph:
            derived["host_stop_saves_ms"] = {"median": med["k4_m1_stop_gated"] - med["k4_m1_stop_host"],
                                             "by_round": [x - y for x, y in zip(ms["k4_m1_stop_gated"],
                                                                                ms["k4_m1_stop_host"])],
                                             "per_skipped_epoch_ms":
                                                 (med["k4_m1_stop_gated"] - med["k4_m1_stop_host"]) / (K - 1)}
        res["update"][name] = dict(sp, envs=E, frame=list(sc[0].frame_shape), cuda_graph=graph,
                                   updates_timed=a.updates * mult, derived=derived)
    return res, "ppo_kl_bench.json"


def cost(a, dev):
    if a.target_kl:
        return cost_target_kl(a, dev)
    if a.minibatches:
        return cost_minibatches(a, dev)
    import vnav
    res = {"tool": "ppo_bench", "mode": "cost",
           "config": {"seed": SEED, "rounds": a.rounds, "updates": a.updates, "update_warmup": a.update_warmup,
                      "variants": VARIANTS},
           "update": {"unit": "ms per A2CTrainer.step() (device, one event pair)"}}
    points = (("envs4096_84_lstm", [vnav.synthetic_scene(k) for k in range(20)], 4096, False, 1),
              ("envs4_174_graph", [vnav.synthetic_scene(0, frame_shape=(174, 174, 3))], 4, True, 10))
    for name, sc, E, graph, mult in points:
        ms = {v: [] for v in VARIANTS}
        for _ in range(a.rounds):
            for v, kw in VARIANTS.items():
                ms[v].append(time_update(kw, sc, E, graph, a.update_warmup, a.updates * mult, dev))
        sp = {v: spread(ms[v]) for v in VARIANTS}
        med = {v: sp[v]["median"] for v in VARIANTS}
        epoch = (med["ppo4"] - med["ppo1"]) / 3.0
        res["update"][name] = dict(
            sp, envs=E, frame=list(sc[0].frame_shape), cuda_graph=graph, updates_timed=a.updates * mult,
            ppo1_minus_a2c_ms={"median": med["ppo1"] - med["a2c"],
                               "by_round": [x - y for x, y in zip(ms["ppo1"], ms["a2c"])]},
            extra_epoch_ms={"from_ppo4": epoch, "from_ppo2": med["ppo2"] - med["ppo1"]},
            extra_epoch_share_of_a2c_step=epoch / med["a2c"],
            adam_minus_rmsprop_ms={"median": med["a2c_adam"] - med["a2c"],
                                   "by_round": [x - y for x, y in zip(ms["a2c_adam"], ms["a2c"])]})
    return res, "ppo_bench.json"


LEARN = {"a2c": {}, "ppo4": dict(ppo_clip=0.2, ppo_epochs=4),
         "ppo4_adam": dict(ppo_clip=0.2, ppo_epochs=4, optimizer="adam")}


def learn_run(kw, seed, updates, dev):
    import vnav
    scene, goal, limit = vnav.synthetic_scene(0, grid=6), 7, 30
    env = vnav.VectorEnv([scene], 16, seed=seed + 1, device=dev, max_episode_steps=limit)
    env.set_tasks([(0, goal)])
    env.reset()
    tr = vnav.A2CTrainer(env, num_steps=20, seed=seed, max_time_steps=1e6, nav_metrics=True, **kw)
    ok = eps = 0.0
    kl = clipped = None  # A2C reports neither
    steps = []  # ppo_steps of every update (with ppo_target_kl)
    for u in range(updates):
        m = tr.step()
        if "ppo_steps" in m:
            steps.append(m["ppo_steps"])
        n_ep, n_ok = (float(x) for x in tr.nav_stats[:2].cpu())
        if u >= updates - 20:
            eps += n_ep
            ok += n_ok
        kl, clipped = m.get("approx_kl", kl), m.get("clip_fraction", clipped)
    env.close()
    return ok / eps if eps else float("nan"), eps, kl, clipped, float(np.mean(steps)) if steps else None


def learn(a, dev):
    variants, name = LEARN, "ppo_learn.json"
    if a.minibatches:
        variants = {"ppo4_adam_m%d" % M: dict(ppo_clip=0.2, ppo_epochs=4, optimizer="adam", ppo_minibatches=M)
                    for M in a.minibatches}
        name = "ppo_minibatch_learn.json"
    if a.target_kl:
        variants = {}
        for opt in ("rmsprop", "adam"):
            base = dict(ppo_clip=0.2, ppo_epochs=4, ppo_minibatches=4, optimizer=opt)
            variants["ppo4_m4_%s" % opt] = base
            for t in a.target_kl:
                variants["ppo4_m4_%s_kl%g" % (opt, t)] = dict(base, ppo_target_kl=t)
        name = "ppo_kl_learn.json"
    res = {"tool": "ppo_bench", "mode": "learn",
           "config": {"task": "synthetic_scene(0, grid=6), goal 7, limit 30", "envs": 16, "num_steps": 20,
                      "updates": a.learn_updates, "seeds": [0, 1, 2], "variants": variants,
                      "measure": "successes / finished episodes over the last 20 updates, and their number; "
                                 "approx_kl and clip_fraction of the last update"},
           "runs": {}}
    for v, kw in variants.items():
        rows = [learn_run(kw, seed, a.learn_updates, dev) for seed in (0, 1, 2)]
        print("%s: success %s" % (v, ["%.3f" % r[0] for r in rows]), file=sys.stderr, flush=True)
        res["runs"][v] = {"success_rate": [r[0] for r in rows], "episodes": [r[1] for r in rows],
                             "approx_kl": [r[2] for r in rows], "clip_fraction": [r[3] for r in rows]}
        if a.target_kl:
            res["runs"][v]["ppo_steps_mean"] = [r[4] for r in rows]
    return res, name


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("cost", "learn"), default="cost")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--updates", type=int, default=30)
    ap.add_argument("--update-warmup", type=int, default=5)
    ap.add_argument("--learn-updates", type=int, default=120)
    ap.add_argument("--minibatches", type=int, nargs="+", default=None, metavar="M",
                    help="measure the minibatch split at these M (writes ppo_minibatch_*.json)")
    ap.add_argument("--target-kl", type=float, nargs="+", default=None, metavar="KL",
                    help="measure the target-KL stop at these targets (writes ppo_kl_*.json)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.target_kl and not min(a.target_kl) > 0:
        ap.error("--target-kl must be > 0")
    if a.minibatches and min(a.minibatches) < 1:
        ap.error("--minibatches must be at least 1")
    if a.out is None:
        sub = "ppo_kl" if a.target_kl else "ppo_minibatch" if a.minibatches else "ppo"
        a.out = os.path.join(REPO, "profiles", sub)
    if not torch.cuda.is_available():
        raise SystemExit("ppo_bench needs the GPU (no CPU timing)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res, name = cost(a, dev) if a.mode == "cost" else learn(a, dev)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, name), "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
