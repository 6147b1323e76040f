"""The update by bits: sha256 of the parameters, the optimiser state and the metric vectors after
three updates of one trainer per update chain, on any tree of this project. Run it on the parent
commit's tree and on the change and compare the two files; only public constructor arguments are
used, so one copy of this script runs against both.

The configurations: the six of profiles/ppo/off_bits_*.json (LSTM, feed-forward, captured graph
with goal runs, aux heads, BigHouse, shaping + GAE + novelty); PPO with RMSprop, Adam in a captured
graph, aux heads, goal runs at 18 envs, minibatches with Adam and feed-forward; the target-KL stop
firing at the first check after a step and never firing in a captured graph; the replayed UNREAL
pass (174 x 174 frames: pixel control needs 168), the replayed aux batch and the expert term.

    python tools/update_bits.py [--tree DIR] --out FILE
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

PPO = dict(ppo_clip=0.2, ppo_epochs=2)
M4 = dict(optimizer="adam", ppo_minibatches=4, **PPO)
CONFIGS = {
    "goal_lstm_e5": dict(envs=5, kw=dict(arch="goal", recurrent=True)),
    "goal_ff_e64": dict(envs=64, kw=dict(arch="goal", recurrent=False)),
    "goal_lstm_e64_graph": dict(envs=64, kw=dict(arch="goal", recurrent=True, cuda_graph=True, dedup_goals=True)),
    "goal_lstm_aux_e5": dict(envs=5, aux=True, kw=dict(arch="goal", recurrent=True, aux_weight=0.1)),
    "bighouse_lstm_e5": dict(envs=5, kw=dict(arch="bighouse", recurrent=True)),
    "goal_lstm_shaped_e8": dict(envs=8, kw=dict(arch="goal", recurrent=True, shaping_weight=0.1, gae_lambda=0.95,
                                                novelty_weight=0.05)),
    "ppo_goal_lstm_e5": dict(envs=5, kw=dict(arch="goal", recurrent=True, **PPO)),
    "ppo_adam_graph_e5": dict(envs=5, kw=dict(arch="goal", recurrent=True, optimizer="adam", cuda_graph=True, **PPO)),
    "ppo_aux_e5": dict(envs=5, aux=True, kw=dict(arch="goal", recurrent=True, aux_weight=0.1, **PPO)),
    "ppo_goal_runs_e18": dict(envs=18, steps=3, kw=dict(arch="goal", recurrent=True, dedup_goals=True, **PPO)),
    "ppo_adam_m4_e8": dict(envs=8, kw=dict(arch="goal", recurrent=True, **M4)),
    "unreal_replay_e5": dict(envs=5, hw=(174, 174), kw=dict(recurrent=True, unreal=True, unreal_source="replay",
                                                            unreal_envs=2, replay_size=2)),
    "aux_replay_e5": dict(envs=5, aux=True, kw=dict(recurrent=True, aux_weight=0.1, aux_source="replay",
                                                    replay_size=2)),
    "expert_adam_e5": dict(envs=5, kw=dict(recurrent=True, expert_weight=0.5, optimizer="adam")),
    "ppo_ff_m2_e6": dict(envs=6, kw=dict(recurrent=False, ppo_clip=0.2, ppo_epochs=2, ppo_minibatches=2)),
    "ppo_kl_fires_rms_e5": dict(envs=5, kw=dict(recurrent=True, ppo_target_kl=1e-9, **PPO)),
    "ppo_kl_fires_adam_m4_e8": dict(envs=8, kw=dict(recurrent=True, ppo_target_kl=1e-9, **M4)),
    "ppo_kl_quiet_graph_e5": dict(envs=5, kw=dict(recurrent=True, ppo_target_kl=1e9, cuda_graph=True, **PPO)),
}


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def run(c):
    scene = maze_scene(c.get("hw", (84, 84)), c.get("aux", False))[0]
    env = vnav.VectorEnv([scene], c["envs"], seed=5, max_episode_steps=4)
    tr = vnav.A2CTrainer(env, num_steps=c.get("steps", 6), seed=9, max_time_steps=1e6, **c["kw"])
    raws = [tr.step(sync=False)["raw"].clone() for _ in range(3)]
    torch.cuda.synchronize()
    r = {"params": sha(tr.params), "square_avg": sha(tr.square_avg), "metrics": sha(torch.cat([x.double() for x in raws])),
         "state_dict_keys": sorted(tr.state_dict()),
         # the vectors themselves: a sum of float atomics may end an ulp apart from run to run
         # (the aux heads' and the UNREAL losses' statistics), which the hash alone cannot place
         "metric_values": [[float(v).hex() for v in x.tolist()] for x in raws]}
    if tr.optimizer == "adam":
        r["exp_avg"], r["exp_avg_sq"], r["adam_step"] = sha(tr.exp_avg), sha(tr.exp_avg_sq), int(tr.adam_step)
    if hasattr(tr, "kl_gate"):
        r["kl_gate"] = tr.kl_gate.tolist()
    env.close()
    return r


res = {}
failed = []
for name, c in CONFIGS.items():
    try:
        res[name] = run(c)
    except (ValueError, vnav._lib.VnavError) as e:  # a refused configuration is recorded, and fails the run below
        res[name] = {"error": "%s: %s" % (type(e).__name__, e)}
        failed.append(name)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write(json.dumps(res, indent=1, sort_keys=True) + "\n")
print(json.dumps({k: v.get("params", v.get("error"))[:16] for k, v in res.items()}))
if failed:
    raise SystemExit("configurations refused: %s" % ", ".join(failed))
