"""A2CTrainer(expert_weight=...): the per-step mask history of the index-only rollout against
nav_ref's masks of the states each step observed, one update's dout against tests/expert_ref.py,
and the trainer-level contracts: off changes nothing, the captured hipGraph anneals as eager does,
a resume is exact, and imitation raises the agreement with the expert."""
import numpy as np
import pytest
import torch

import expert_ref as er
import nav_ref as nr

pytestmark = pytest.mark.gpu

ST_SCENE, ST_STATE, ST_GOAL, ST_ELAPSED = 0, 1, 2, 4
BASE_KEYS = {"step", "updates", "value_loss", "action_loss", "entropy", "loss", "episodes", "reward",
             "episode_length", "grad_norm", "return_mean", "fps"}
EXPERT_KEYS = {"expert_loss", "expert_agreement", "expert_weight"}


def _vnav():
    import vnav
    return vnav


def make(E, T, limit=6, n_scenes=2, env_seed=5, tasks=None, **kw):
    vnav = _vnav()
    sc = [vnav.synthetic_scene(k, grid=6) for k in range(n_scenes)]  # 84 x 84 frames
    env = vnav.VectorEnv(sc, E, seed=env_seed, max_episode_steps=limit)
    if tasks is not None:
        env.set_tasks(tasks)
        env.reset()
    opts = dict(num_steps=T, seed=9, max_time_steps=1e6)
    opts.update(kw)
    return vnav.A2CTrainer(env, **opts)


def tables(tr):
    graphs = [np.asarray(s.graph) for s in tr.env.scenes]
    return graphs, [nr.geodesic(g) for g in graphs]


def masks_of(tr, tabs, table):
    tb = table.cpu().numpy()
    return er.observed_masks(tabs[0], tabs[1], tb[ST_SCENE], tb[ST_STATE], tb[ST_GOAL])


# ---- 5. the mask history ------------------------------------------------------------------

@pytest.mark.parametrize("E", [1, 5, 257])
def test_mask_history(E):
    """T = 3 with a limit of 4 steps: truncations and auto-resets fall inside both rollouts.
    expert_mask[t] = nav_ref's mask of the state observed at step t (the env's table before
    the step), slot 0 of the second rollout included; the rows around [T, E] keep their fill;
    the env's own buffer holds the post-rollout masks."""
    T = 3
    tr = make(E, T, limit=4, expert_weight=1.0)
    tabs = tables(tr)
    pad = torch.full((T + 2, E), 0xEE, dtype=torch.uint8, device="cuda")
    tr.expert_mask = pad[1:T + 1]
    seen = []
    step = tr.env.step_a2c

    def recording_step(*a):
        step(*a)
        seen.append(tr.env.get_state().clone())

    tr.env.step_a2c = recording_step
    dones = 0
    for r in range(2):
        del seen[:]
        first = tr.env.get_state().clone()
        tr.step()
        torch.cuda.synchronize()
        observed = np.stack([masks_of(tr, tabs, tb) for tb in [first] + seen[:T - 1]])
        got = tr.expert_mask.cpu().numpy()
        assert np.array_equal(got, observed), (r, got, observed)
        assert (pad[0] == 0xEE).all() and (pad[T + 1] == 0xEE).all()
        own = tr.env.nav_outputs()["optimal_mask"].cpu().numpy()
        assert np.array_equal(own, masks_of(tr, tabs, seen[T - 1])), r
        dones += int(tr.dones.sum())
        assert (observed != 0).any()
    assert dones >= E  # every env ran into the 4-step limit inside the six steps


# ---- 6. one update's dout -----------------------------------------------------------------

@pytest.mark.parametrize("recurrent", [False, True], ids=["ff", "lstm"])
def test_update_dout_vs_fp64(recurrent):
    E, T, w = 16, 5, 0.5
    tr = make(E, T, recurrent=recurrent, expert_weight=w, pg_coefficient=0.25)
    tr.step()
    tr.step()
    torch.cuda.synchronize()
    out, actions = tr.out.cpu().numpy(), tr.actions.cpu().numpy()
    rets, mask = tr.returns.cpu().numpy(), tr.expert_mask.cpu().numpy().reshape(-1)
    A = tr.A
    ref = er.expert_loss_grad64(out, actions, rets, mask, A, tr.value_coefficient, tr.entropy_coefficient, 0.25,
                                np.float32(w))
    d = tr.dout.cpu().numpy().astype(np.float64)
    scale = np.abs(ref["dout"]).max()
    err = np.abs(d - ref["dout"]).max()
    print("EXPERTERR update dout (%s) worst %.3e bound %.3e" % ("lstm" if recurrent else "ff", err, 1e-5 * scale))
    assert np.isfinite(d).all() and err <= 1e-5 * scale
    e = tr.expert_stats.cpu().numpy()
    assert e[1] == ref["expert3"][1] and e[2] == ref["expert3"][2] and e[2] > 0
    assert abs(e[0] - ref["expert3"][0]) <= 1e-5 * ref["expert_mag"]
    assert e[3] == np.float32(w)
    assert (mask != 0).sum() == e[2]


# ---- 7. off = today's trainer ---------------------------------------------------------------

@pytest.mark.parametrize("recurrent", [False, True], ids=["ff", "lstm"])
def test_zero_weight_changes_nothing(recurrent):
    E, T = 4, 5
    runs = {}
    for w in (None, 0.0):
        tr = make(E, T, recurrent=recurrent, expert_weight=w)
        ms = [tr.step(sync=True) for _ in range(3)]
        raw = tr.step(sync=False)["raw"]
        torch.cuda.synchronize()
        runs[w] = (tr.params.clone(), tr.square_avg.clone(), ms, raw, tr)
    off, on = runs[None], runs[0.0]
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])
    assert all(set(m) == BASE_KEYS for m in off[2]) and off[3].numel() == 9
    assert not hasattr(off[4], "expert_mask") and not off[4].env.nav_info
    assert all(set(m) == BASE_KEYS | EXPERT_KEYS for m in on[2]) and on[3].numel() == 13
    assert torch.equal(on[3][:9], off[3])
    for a, b in zip(on[2], off[2]):
        for k in BASE_KEYS - {"fps"}:
            assert a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]), k
        assert a["expert_weight"] == 0.0 and 0.0 <= a["expert_agreement"] <= 1.0 and a["expert_loss"] > 0.0
    with pytest.raises(ValueError):
        make(E, T, pg_coefficient=0.5)


def test_metric_vector_with_nav_metrics():
    """nav sums first, then the three expert sums and the weight; evaluate() reports the
    agreement."""
    tr = make(4, 5, expert_weight=0.5, nav_metrics=True)
    m = tr.step()
    assert set(m) == BASE_KEYS | EXPERT_KEYS | {"success_rate", "spl"}
    raw = tr.step(sync=False)["raw"].cpu().numpy()
    assert raw.shape == (17,)
    assert np.array_equal(raw[9:13], tr.nav_stats.cpu().numpy())
    assert np.array_equal(raw[13:], tr.expert_stats.cpu().numpy())
    N = 20
    m = tr.step()
    want = tr.value_coefficient * m["value_loss"] + m["action_loss"] - tr.entropy_coefficient * m["entropy"] + \
        m["expert_weight"] * m["expert_loss"] * float(tr.expert_stats[2]) / N
    assert abs(m["loss"] - want) <= 1e-6 * max(abs(want), 1.0)
    res = tr.evaluate(episodes=6)
    assert 0.0 <= res["expert_agreement"] <= 1.0 and "spl" in res
    assert "expert_agreement" not in make(4, 5).evaluate(episodes=2)


# ---- 8. hipGraph ------------------------------------------------------------------------------

@pytest.mark.parametrize("recurrent", [False, True], ids=["ff", "lstm"])
def test_graph_anneals_as_eager(recurrent):
    """20 env-steps per update against an annealing horizon of 70: the weight changes at every
    update and reaches 0 at the fifth. A captured update froze its scalar arguments, so the
    sequence shows that the weight comes from device memory."""
    E, T, w0, horizon = 4, 5, 0.8, 70
    want = [float(er.anneal_weight(w0, k * E * T, horizon)) for k in range(5)]
    assert len(set(want)) == 5 and want[-1] == 0.0
    runs = {}
    for graph in (False, True):
        tr = make(E, T, recurrent=recurrent, expert_weight=w0, expert_anneal_steps=horizon, cuda_graph=graph)
        ws = [tr.step()["expert_weight"] for _ in range(5)]
        torch.cuda.synchronize()
        assert ws == want, (graph, ws, want)
        runs[graph] = (tr.params.clone(), tr.square_avg.clone(), tr.expert_mask.clone())
    for a, b in zip(runs[True], runs[False]):
        assert torch.equal(a, b)


# ---- 9. resume --------------------------------------------------------------------------------

@pytest.mark.parametrize("recurrent", [False, True], ids=["ff", "lstm"])
def test_resume_is_exact(recurrent):
    kw = dict(recurrent=recurrent, expert_weight=0.8, expert_anneal_steps=200, limit=4)
    a = make(4, 5, **kw)
    a.step()
    a.step()
    sd = a.state_dict()
    own = a.env.nav_outputs()["optimal_mask"].clone()
    a.step()
    a.step()
    b = make(4, 5, **kw)
    b.load_state_dict(sd)
    torch.cuda.synchronize()
    assert torch.equal(b.env.nav_outputs()["optimal_mask"], own)  # the restored states' masks
    b.step()
    mid = b.expert_mask.clone()
    b.step()
    torch.cuda.synchronize()
    assert torch.equal(b.params, a.params) and torch.equal(b.square_avg, a.square_avg)
    assert torch.equal(b.expert_mask, a.expert_mask) and torch.equal(mid[0], own)
    assert torch.equal(b.expert_stats, a.expert_stats)


# ---- 10. it learns ----------------------------------------------------------------------------

def learning_run(seed, updates, expert_weight, pg_coefficient, tasks=None):
    """16 envs x 20 steps, feed-forward 84 x 84, one 6 x 6 scene: per-update expert_agreement
    and the uniform-policy expectation mean(popcount(M) / A) over the labelled samples."""
    tr = make(16, 20, limit=30, n_scenes=1, env_seed=seed + 1, tasks=tasks, seed=seed, expert_weight=expert_weight,
              pg_coefficient=pg_coefficient)
    agree, uniform = [], []
    for _ in range(updates):
        agree.append(tr.step()["expert_agreement"])
        m = tr.expert_mask.cpu().numpy().reshape(-1).astype(np.int64) & ((1 << tr.A) - 1)
        bits = np.array([bin(v).count("1") for v in m[m != 0]], dtype=np.float64)
        uniform.append(bits.mean() / tr.A)
    return np.array(agree), np.array(uniform)


LEARN_UPDATES, LEARN_TASKS = 120, [(0, 7)]
# Recorded on the first GPU run (DESIGN.md "Expert loss from the navigation tables"): mean
# expert_agreement over updates 110..119, seeds 0 / 1 / 2 -> imitation 0.9944 / 0.9966 / 0.9912,
# A2C alone 0.3978 / 0.4000 / 0.3844: gaps 0.5966 / 0.5966 / 0.6069. The test asks for half the
# smallest: agreement over 3200 samples of 16 correlated envs moves by a few points per seed.
LEARN_MIN_GAP = 0.5 * 0.5966


def test_imitation_raises_agreement():
    """pg_coefficient = 0, expert_weight = 1 against the same trainer and seed with
    expert_weight = 0 (which reports the agreement but trains by A2C alone), one 6 x 6 scene
    with one goal, 120 updates of 16 envs x 20 steps (0.2 s a run): the agreement over the last
    ten updates lies at least LEARN_MIN_GAP above A2C's, and above what a uniform policy would
    score on the same masks."""
    im, uniform = learning_run(0, LEARN_UPDATES, 1.0, 0.0, tasks=LEARN_TASKS)
    rl, _ = learning_run(0, LEARN_UPDATES, 0.0, 1.0, tasks=LEARN_TASKS)
    a, b, u = im[-10:].mean(), rl[-10:].mean(), uniform[-10:].mean()
    print("EXPERT learns: imitation %.4f a2c %.4f gap %.4f (asked %.4f) uniform %.4f" % (a, b, a - b, LEARN_MIN_GAP, u))
    assert a - b >= LEARN_MIN_GAP
    assert a > u


def test_experiment_table_has_expert_columns(tmp_path):
    import json
    import os
    from vnav import train
    logs = []
    exp = train.make_trainer("thor-cached-auxiliary", expert_weight=1.0, pg_coefficient=0.0,
                             expert_anneal_steps=10 ** 6, env_kwargs=dict(grid=(6, 6), frame=(84, 84), goal=(3, 3, 0), num_envs=8),
                             save_dir=str(tmp_path), max_time_steps=8 * 20 * 3, saving_period=0, episode_log_interval=1,
                             logger=logs.append)
    exp.run()
    assert exp.trainer.expert and exp.trainer.pg_coefficient == 0.0
    rows = [l for l in logs if l.startswith("---")]
    assert rows and all("| " + k in r for r in rows for k in EXPERT_KEYS)
    last = json.loads(open(os.path.join(str(tmp_path), "metrics.jsonl")).read().strip().split("\n")[-1])
    assert EXPERT_KEYS <= set(last) and 0.0 < last["expert_weight"] <= 1.0
