"""Off is off by bits: sha256 of the parameters, the optimiser state and the metric vectors after
three updates of trainers built without ppo_target_kl, on any tree of this project.

The configurations are the six of profiles/ppo/off_bits_*.json (LSTM, feed-forward, captured graph
with goal runs, aux heads, BigHouse, shaping + GAE + novelty) and, because the stop lives in the PPO
update, one with PPO on: K = 2 epochs in M = 4 minibatches at 8 envs with Adam. Run it on the parent
commit's tree and on the change and compare the two files.

    python tools/ppo_kl_bits.py [--tree DIR] --out FILE
"""
import argparse
import hashlib
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--out", required=True)
a = ap.parse_args()
for p in (a.tree, os.path.join(a.tree, "a2cat-vn-pytorch_amd")):
    sys.path.insert(0, p)

import torch  # noqa: E402

import vnav  # noqa: E402
from oracle.update_checks import maze_scene  # noqa: E402

assert os.path.abspath(vnav.__file__).startswith(os.path.abspath(a.tree)), vnav.__file__

CONFIGS = {
    "goal_lstm_e5": dict(envs=5, kw=dict(arch="goal", recurrent=True)),
    "goal_ff_e64": dict(envs=64, kw=dict(arch="goal", recurrent=False)),
    "goal_lstm_e64_graph": dict(envs=64, kw=dict(arch="goal", recurrent=True, cuda_graph=True, dedup_goals=True)),
    "goal_lstm_aux_e5": dict(envs=5, aux=True, kw=dict(arch="goal", recurrent=True, aux_weight=0.1)),
    "bighouse_lstm_e5": dict(envs=5, kw=dict(arch="bighouse", recurrent=True)),
    "goal_lstm_shaped_e8": dict(envs=8, kw=dict(arch="goal", recurrent=True, shaping_weight=0.1, gae_lambda=0.95,
                                                novelty_weight=0.05)),
    "ppo_adam_m4_e8": dict(envs=8, kw=dict(arch="goal", recurrent=True, optimizer="adam", ppo_clip=0.2, ppo_epochs=2,
                                           ppo_minibatches=4)),
}


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def run(c):
    scene = maze_scene((84, 84), c.get("aux", False))[0]
    env = vnav.VectorEnv([scene], c["envs"], seed=5, max_episode_steps=4)
    tr = vnav.A2CTrainer(env, num_steps=6, seed=9, max_time_steps=1e6, **c["kw"])
    raws = [tr.step(sync=False)["raw"].clone() for _ in range(3)]
    torch.cuda.synchronize()
    r = {"params": sha(tr.params), "square_avg": sha(tr.square_avg), "metrics": sha(torch.cat([x.double() for x in raws])),
         "state_dict_keys": sorted(tr.state_dict())}
    if tr.optimizer == "adam":
        r["exp_avg"], r["exp_avg_sq"], r["adam_step"] = sha(tr.exp_avg), sha(tr.exp_avg_sq), int(tr.adam_step)
    env.close()
    return r


res = {name: run(c) for name, c in CONFIGS.items()}
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write(json.dumps(res, indent=1, sort_keys=True) + "\n")
print(json.dumps({k: v["params"][:16] for k, v in res.items()}))
