"""A2CTrainer(geo_curriculum=...): the level moves inside the captured hipGraph exactly as it does
eagerly, a checkpoint resumes bit for bit, the evaluations leave the curriculum and the training
as they were, and the default trainer is unchanged. 84 x 84 policy, 4 envs, T = 5, one scene."""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

E, T, LIMIT = 4, 5, 6
# down just under up: every full window moves the level one way or the other (a rate k / n with
# n < 50 never lies strictly between), so the level changes whatever the untrained policy does
CUR = dict(level=3, mode=1, window=4, up=0.5, down=0.49, step=1, level_min=1)


def make(cur=CUR, graph=False, nav=False, seed=9):
    import vnav
    env = vnav.VectorEnv([vnav.synthetic_scene(0, grid=6)], E, seed=5, max_episode_steps=LIMIT)
    return vnav.A2CTrainer(env, num_steps=T, seed=seed, max_time_steps=1e6, cuda_graph=graph, nav_metrics=nav,
                           geo_curriculum=cur)


def snapshot(tr):
    s = dict(params=tr.params.clone(), square_avg=tr.square_avg.clone(), env=tr.env.get_state().clone(),
             returns=tr.env.get_episode_returns().clone(), sched=tr.sched.clone())
    if tr.geo_curriculum is not None:
        s["cur"] = tr.env.curriculum_state().clone()
        s["nav"] = tr.env.get_nav_state().clone()
    return s


def assert_same(a, b):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def same_metrics(xs, ys):
    for x, y in zip(xs, ys):
        assert set(x) == set(y)
        for k in x:
            if k != "fps":
                assert x[k] == y[k] or (x[k] != x[k] and y[k] != y[k]), k


def test_graph_equals_eager():
    a, b = make(), make(graph=True)
    gen = b.env.config_generation
    ma = [a.step() for _ in range(6)]
    mb = [b.step() for _ in range(6)]
    assert b._graph is not None and b.env.config_generation == gen  # one capture, never recaptured
    assert_same(snapshot(a), snapshot(b))
    same_metrics(ma, mb)
    levels = [m["curriculum_level"] for m in ma]
    assert len(set(levels)) > 1, levels  # the level moved under the captured graph
    st = a.env.curriculum_state().cpu().numpy()
    assert levels[-1] == float(st[0, 0]) and 1 <= st[0, 0] <= st[3, 0]
    assert a.env.error_flags() == 0 and b.env.error_flags() == 0


def test_checkpoint_resumes_bitwise():
    a, b, c = make(), make(), make()
    for _ in range(6):
        a.step()
    for _ in range(3):
        b.step()
    sd = b.state_dict()
    assert sd["env_curriculum"].shape == (4, 1) and sd["env_curriculum"].dtype == torch.int32
    c.load_state_dict(sd)
    for _ in range(3):
        c.step()
    assert_same(snapshot(a), snapshot(c))
    # a checkpoint without the curriculum state: a warning, and the configured level
    del sd["env_curriculum"]
    d = make(cur=dict(CUR, level=5))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        d.load_state_dict(sd)
    assert any("curriculum" in str(x.message) for x in w)
    assert d.env.curriculum_state().cpu().numpy()[:3, 0].tolist() == [5, 0, 0]


def test_evaluations_leave_the_curriculum():
    import vnav
    a, b = make(nav=True), make(nav=True)
    ma = [a.step() for _ in range(3)]
    before = snapshot(a)
    eps = vnav.EpisodeSet.sample(a.env, 3, buckets=((1, 3), (4, None)), seed=2)
    res = a.evaluate_episodes(eps, seed=5)
    assert res["episodes"] == len(eps)
    assert_same(before, snapshot(a))
    a.evaluate(episodes=4)  # runs on: the envs move, the curriculum state does not
    assert torch.equal(a.env.curriculum_state(), before["cur"])
    c = make(nav=True)
    mc = [c.step() for _ in range(3)]
    c.evaluate_episodes(eps, seed=5)
    mc += [c.step() for _ in range(2)]
    mb = [b.step() for _ in range(5)]
    assert_same(snapshot(b), snapshot(c))
    same_metrics(mb, mc)
    same_metrics(ma, mb[:3])


def test_default_trainer_is_unchanged():
    a = make(cur=None)
    m = a.step()
    assert "curriculum_level" not in m and a.geo_curriculum is None
    assert a.env.geo_curriculum is None and not a.env.nav_info
    assert "env_curriculum" not in a.state_dict()
    b = make()
    assert "curriculum_level" in b.step() and b.env.nav_info
