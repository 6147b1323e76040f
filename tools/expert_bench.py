"""What the expert term costs per update: milliseconds per A2CTrainer.step(sync=False) with
nav_metrics=True alone against nav_metrics=True + expert_weight, in one process, the two sides
alternating, 5 rounds of `updates` timed updates after `warmup`, one event pair around the timed
updates. Two operating points:

  envs4096_84_lstm     4096 envs over 20 synthetic scenes, 84x84, the LSTM policy, eager
  envs4_174_graph      4 envs of one 174x174 scene, the LSTM policy, cuda_graph=True

Expert on adds two small device copies per rollout (slot 0 of the mask history and the step
count the weight anneals on) and replaces vn_a2c_loss_grad's launch by one of the same shape.
Prints one JSON line.

    python tools/expert_bench.py [--rounds 5] [--updates 30] [--warmup 5]
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


def spread(xs):
    xs = sorted(xs)
    return {"min": xs[0], "median": float(np.median(xs)), "max": xs[-1], "runs": xs}


def time_side(expert, scenes, E, graph, warmup, K, dev):
    import vnav
    env = vnav.VectorEnv(scenes, E, seed=1000, device=dev)
    kw = dict(expert_weight=0.5, expert_anneal_steps=10 ** 9) if expert else {}
    tr = vnav.A2CTrainer(env, recurrent=True, nav_metrics=True, cuda_graph=graph, seed=1, **kw)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--updates", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import vnav
    if not torch.cuda.is_available():
        raise SystemExit("expert_bench needs the GPU (no CPU timing)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    points = (("envs4096_84_lstm", [vnav.synthetic_scene(k) for k in range(20)], 4096, False, 1),
              ("envs4_174_graph", [vnav.synthetic_scene(0, frame_shape=(174, 174, 3))], 4, True, 10))
    res = {"tool": "expert_bench", "unit": "ms per update (device, one event pair)",
           "config": {"rounds": a.rounds, "updates": a.updates, "warmup": a.warmup}, "points": {}}
    for name, sc, E, graph, mult in points:
        ms = {False: [], True: []}
        for _ in range(a.rounds):
            for expert in (False, True):
                ms[expert].append(time_side(expert, sc, E, graph, a.warmup, a.updates * mult, dev))
        off, on = spread(ms[False]), spread(ms[True])
        res["points"][name] = {"envs": E, "frame": list(sc[0].frame_shape), "cuda_graph": graph,
                               "updates_timed": a.updates * mult, "nav_metrics_only": off, "expert_on": on,
                               "expert_cost_ms": on["median"] - off["median"]}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
