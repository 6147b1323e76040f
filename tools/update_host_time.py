"""Host-bound time per eager update, on any tree of this project: the wall time of step(sync=False)
with cuda_graph=False, a synchronise on both sides of the timed window, for the reference's own
regime (4 envs x 20 steps, recurrent, about 400 launches per update) and for PPO with K = 4 epochs
in M = 2 minibatches at 8 envs. The device work of two trees with one library is the same, so what
differs between them is the Python between the launches. Prints one JSON line; run the trees to be
compared alternately, one process per run.

    python tools/update_host_time.py [--tree DIR] [--steps 100] [--warmup 30]
"""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--warmup", type=int, default=30)
a = ap.parse_args()
for p in (a.tree, os.path.join(a.tree, "a2cat-vn-pytorch_amd")):
    sys.path.insert(0, p)

import torch  # noqa: E402

import vnav  # noqa: E402
from oracle.update_checks import maze_scene  # noqa: E402

assert os.path.abspath(vnav.__file__).startswith(os.path.abspath(a.tree)), vnav.__file__

CONFIGS = {"a2c_lstm_e4_t20": dict(envs=4, kw={}),
           "ppo_k4_m2_e8_t20": dict(envs=8, kw=dict(ppo_clip=0.2, ppo_epochs=4, ppo_minibatches=2))}
res = {}
for name, c in CONFIGS.items():
    env = vnav.VectorEnv([maze_scene((84, 84), False)[0]], c["envs"], seed=5, max_episode_steps=30)
    tr = vnav.A2CTrainer(env, num_steps=20, seed=9, max_time_steps=1e9, recurrent=True, cuda_graph=False, **c["kw"])
    for _ in range(a.warmup):
        tr.step(sync=False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        tr.step(sync=False)
    torch.cuda.synchronize()
    res[name] = round((time.perf_counter() - t0) / a.steps * 1e3, 4)  # ms per update
    env.close()
print(json.dumps(res))
