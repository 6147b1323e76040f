"""A2CTrainer(nav_metrics=True) and the --test table: the navigation sums ride beside the
update without touching it (parameters and RMSprop state bitwise as without them), evaluate()
reports success rate / SPL / start distance, and the nav record travels with the checkpoint."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

E, T, UPDATES = 4, 5, 3


def _vnav():
    import vnav
    return vnav


def make(nav, recurrent, graph, seed=9):
    vnav = _vnav()
    sc = [vnav.synthetic_scene(k, grid=6) for k in range(2)]  # 84 x 84 frames
    env = vnav.VectorEnv(sc, E, seed=5, max_episode_steps=6)
    return vnav.A2CTrainer(env, num_steps=T, seed=seed, max_time_steps=400, recurrent=recurrent, cuda_graph=graph,
                           nav_metrics=nav)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("recurrent", [False, True], ids=["ff", "lstm"])
def test_update_is_bitwise_unchanged(recurrent, graph):
    runs = {}
    for nav in (False, True):
        tr = make(nav, recurrent, graph)
        ms = [tr.step(sync=True) for _ in range(UPDATES)]
        torch.cuda.synchronize()
        runs[nav] = (tr.params.clone(), tr.square_avg.clone(), ms, tr)
    off, on = runs[False], runs[True]
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])
    for a, b in zip(on[2], off[2]):
        assert set(a) - set(b) == {"success_rate", "spl"}
        for k in b:
            if k != "fps":
                assert a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]), k
        if a["episodes"]:
            assert 0.0 <= a["spl"] <= a["success_rate"] <= 1.0
        else:
            assert a["spl"] != a["spl"] and a["success_rate"] != a["success_rate"]
    assert sum(m["episodes"] for m in on[2]) >= E  # max_episode_steps 6 < 15 steps
    assert not hasattr(off[3], "nav_stats") and not off[3].env.nav_info
    # nav_stats = the last rollout's sums, its episode count the a2c one
    st = on[3].nav_stats.cpu().numpy()
    assert st[0] == on[3].episode_stats.cpu().numpy()[0] == on[2][-1]["episodes"]
    assert 0 <= st[2] <= st[1] <= st[0]


@pytest.mark.parametrize("recurrent", [False, True], ids=["ff", "lstm"])
def test_evaluate_reports_nav_metrics(recurrent):
    tr = make(True, recurrent, False)
    tr.step()
    res = tr.evaluate(episodes=12)
    assert res["episodes"] >= 12
    assert 0.0 <= res["spl"] <= res["success_rate"] <= 1.0
    assert np.isfinite(res["start_distance"]) and res["start_distance"] >= 1.0  # starts are off the goal
    plain = make(False, recurrent, False).evaluate(episodes=4)
    assert set(plain) == {"episodes", "reward", "episode_length"}


def test_checkpoint_carries_nav_state():
    a = make(True, True, False)
    a.step()
    a.step()
    sd = a.state_dict()
    assert tuple(sd["env_nav"].shape) == (2, E) and sd["env_nav"].dtype == torch.int32
    want = []
    for _ in range(3):
        a.step()
        want.append(a.nav_stats.clone())
    b = make(True, True, False, seed=9)
    b.load_state_dict(sd)
    for w in want:
        b.step()
        assert torch.equal(b.nav_stats, w)
    assert torch.equal(b.params, a.params)
    assert sum(float(w[0]) for w in want) >= E
    # a checkpoint without the key: a warning, and the nav state starts from the current positions
    old = {k: v for k, v in sd.items() if k != "env_nav"}
    c = make(True, True, False)
    gen = c.env.config_generation
    with pytest.warns(UserWarning, match="navigation state"):
        c.load_state_dict(old)
    assert c.env.config_generation > gen
    st = c.env.get_state().cpu().numpy()
    nav = c.env.get_nav_state().cpu().numpy()
    assert np.array_equal(nav[1], st[4])  # length offset = elapsed
    assert np.array_equal(nav[0], c.env.nav_outputs()["distance_to_goal"].cpu().numpy())
    c.step()
    # and one saved without nav_metrics loads into a trainer without them, silently
    d = make(False, True, False)
    d.load_state_dict(old)


def test_cli_test_table_has_nav_columns(tmp_path):
    from vnav import train
    logs = []
    kw = dict(env_kwargs=dict(grid=(6, 6), frame=(84, 84), goal=(3, 3, 0), num_envs=8), save_dir=str(tmp_path),
              max_time_steps=8 * 20 * 3, saving_period=0, episode_log_interval=1, logger=logs.append)
    exp = train.make_trainer("thor-cached-auxiliary", nav_metrics=True, **kw)
    exp.run()
    rows = [l for l in logs if l.startswith("---")]
    assert rows and all("success_rate" in r and "| spl" in r for r in rows)
    assert "env_nav" in torch.load(exp.checkpoint_path, weights_only=True)
    logs.clear()
    ev = train.make_trainer("thor-cached-auxiliary", **kw)
    res = ev.test(episodes=5)
    assert ev.trainer.nav_metrics
    table = [l for l in logs if l.startswith("---")][-1]
    for col in ("success_rate", "spl", "start_distance", "episodes", "reward", "episode_length"):
        assert "| " + col in table, col
    assert 0.0 <= res["spl"] <= res["success_rate"] <= 1.0
    import json
    last = json.loads(open(os.path.join(str(tmp_path), "metrics.jsonl")).read().strip().split("\n")[-1])
    assert {"success_rate", "spl", "start_distance"} <= set(last)
