"""What the reward-skewed reward-prediction draw costs per update, and what it changes in the rp batch.

In one process, rp_sampling "sequence" and "skewed" alternating, --rounds rounds after a warm-up, one
event pair around the timed updates, at two operating points:

  envs4_174_graph     thor-cached-auxiliary's batch (vnav.train's registered experiment: 4 envs x
                      20 steps, 174x174, LSTM + aux + UNREAL, both batches replayed, hardness 0.01,
                      captured hipGraph)
  envs4096_174        4096 envs, 174x174, LSTM + aux + UNREAL with both replay sources,
                      unreal_envs=16, eager

Per mode: ms per update (min / median / max over the rounds) and, over --stat-updates updates of one
further trainer, the mean used-sample count of the rp loss and (skewed) the mean of
rp_drawn_nonzero / rp_drawn; for "sequence" the share of used windows with a non-zero reward is
counted from the drawn slot on the host.

Writes <out>/rp_sampling_bench.json and prints the same JSON line.

    python tools/rp_sampling_bench.py [--rounds 5] [--points envs4_174_graph,envs4096_174] [--out DIR]
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

MODES = ("sequence", "skewed")


def spread(xs):
    xs = sorted(xs)
    return {"min": xs[0], "median": float(np.median(xs)), "max": xs[-1], "runs": xs}


def make(point, mode, dev):
    """(trainer, close) of an operating point under one mode."""
    import vnav
    from vnav import train
    if point == "envs4_174_graph":
        exp = train.make_trainer("thor-cached-auxiliary", device=dev, logger=None, save=False, rp_sampling=mode)
        tr = exp._setup()
        return tr, tr.env.close
    frame, rng, scenes = (174, 174, 3), np.random.default_rng(0), []
    for k in range(4):  # synthetic scenes with depth + segmentation frames, as bench.py's 174x174 legs build them
        sc = vnav.synthetic_scene(k, frame_shape=frame)
        sc.depth = rng.integers(0, 256, size=(sc.n_states,) + frame[:2] + (1,), dtype=np.uint8)
        sc.segmentation = rng.integers(0, 256, size=(sc.n_states,) + frame[:2] + (3,), dtype=np.uint8)
        sc.__post_init__()
        scenes.append(sc)
    env = vnav.VectorEnv(scenes, 4096, seed=2000, device=dev, max_episode_steps=900)
    tr = vnav.A2CTrainer(env, num_steps=20, seed=7, max_time_steps=1e12, recurrent=True, aux_weight=0.1, unreal=True,
                         unreal_envs=16, aux_source="replay", unreal_source="replay", rp_sampling=mode)
    return tr, env.close


def time_updates(point, mode, warmup, K, dev):
    tr, close = make(point, mode, dev)
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
    close()
    del tr
    torch.cuda.empty_cache()
    return ms


def batch_stats(point, mode, updates, dev):
    """Means over `updates` updates: rp samples the loss used, and their non-zero-reward share."""
    tr, close = make(point, mode, dev)
    used, share, cand = [], [], []
    for _ in range(updates):
        m = tr.step(sync=True)
        used.append(float(tr.unreal_stats[2]))
        if mode == "skewed":
            if m["rp_drawn"]:
                share.append(m["rp_drawn_nonzero"] / m["rp_drawn"])
            cand.append([m["rp_candidates_zero"], m["rp_candidates_nonzero"]])
        else:  # the drawn slot's windows, as vn_unreal_rp_loss_grad uses them
            r, d = tr.ur_cur["rewards"].cpu().numpy(), tr.ur_cur["dones"].cpu().numpy()
            ok = ~d[:-2] & ~d[1:-1]
            if ok.sum():
                share.append(float(((r[2:] != 0) & ok).sum() / ok.sum()))
    close()
    del tr
    torch.cuda.empty_cache()
    out = {"updates": updates, "rp_used_mean": float(np.mean(used)),
           "nonzero_share_mean": float(np.mean(share)) if share else None, "updates_with_a_sample": len(share)}
    if cand:
        out["candidates_zero_mean"], out["candidates_nonzero_mean"] = (float(v) for v in np.mean(cand, axis=0))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--points", default="envs4_174_graph,envs4096_174")
    ap.add_argument("--updates", type=int, default=300, help="timed updates per round at 4 envs")
    ap.add_argument("--updates-big", type=int, default=3, help="timed updates per round at 4096 envs")
    ap.add_argument("--warmup", type=int, default=5, help="(4096 envs: 1)")
    ap.add_argument("--stat-updates", type=int, default=200)
    ap.add_argument("--stat-updates-big", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "rp_sampling"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rp_sampling_bench needs the GPU (no CPU timing)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"tool": "rp_sampling_bench", "unit": "ms per update (device, one event pair)",
           "config": {"rounds": a.rounds, "updates": a.updates, "updates_big": a.updates_big, "warmup": a.warmup,
                      "stat_updates": a.stat_updates, "stat_updates_big": a.stat_updates_big}, "points": {}}
    for point in a.points.split(","):
        big = point == "envs4096_174"
        K, W = (a.updates_big, 1) if big else (a.updates, a.warmup)
        ms = {m: [] for m in MODES}
        for _ in range(a.rounds):
            for mode in MODES:
                ms[mode].append(time_updates(point, mode, W, K, dev))
        entry = {"updates_timed": K, "warmup": W}
        for mode in MODES:
            entry[mode] = {"ms_per_update": spread(ms[mode]),
                           "rp_batch": batch_stats(point, mode, a.stat_updates_big if big else a.stat_updates, dev)}
        entry["cost_ms"] = entry["skewed"]["ms_per_update"]["median"] - entry["sequence"]["ms_per_update"]["median"]
        res["points"][point] = entry
        print(json.dumps({point: entry}), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "rp_sampling_bench.json"), "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
