"""A2CTrainer.evaluate_episodes on the GPU: exact end to end with a constant-action policy (the
expected outcome of every episode is a CPU walk of the graph), every episode exactly once with a
real policy, and training left bitwise untouched."""
import numpy as np
import pytest
import torch

import episodes_ref as er
import nav_ref as nr

pytestmark = pytest.mark.gpu

E, T, LIMIT, ACTION = 5, 4, 12, 2
BUCKETS = ((1, 3), (4, 8), (9, None))
KEYS = ("episodes", "success_rate", "spl", "episode_length", "reward", "start_distance")


def _vnav():
    import vnav
    return vnav


def scenes():
    return [_vnav().synthetic_scene(k, grid=6) for k in range(2)]  # 84 x 84 frames, 92 states


def make(recurrent, graph=False, nav=True, limit=LIMIT, seed=9):
    vnav = _vnav()
    env = vnav.VectorEnv(scenes(), E, seed=5, max_episode_steps=limit)
    return vnav.A2CTrainer(env, num_steps=T, seed=seed, max_time_steps=4000, recurrent=recurrent, cuda_graph=graph,
                           nav_metrics=nav)


@pytest.fixture(scope="module")
def tables():
    graphs = [s.graph for s in scenes()]
    return graphs, [nr.geodesic(g) for g in graphs]


def constant_policy(tr, action):
    """All parameters zero, the head bias of `action` 1000: the policy takes it whatever it sees,
    sampled or greedy."""
    tr.params.zero_()
    _, b_off = tr.net.offsets["head"]
    tr.params[b_off + action] = 1000.0


def expected(tables_, eps):
    graphs, geos = tables_
    w = [er.walk_constant(graphs[k], geos[k], s, g, ACTION, LIMIT) for k, s, g in zip(eps.scene, eps.start, eps.goal)]
    return dict(success=np.array([x[0] for x in w], dtype=bool), length=np.array([x[1] for x in w], dtype=np.int32),
                spl=np.array([x[2] for x in w], dtype=np.float32),
                start_distance=np.array([geos[k][g, s] for k, s, g in zip(eps.scene, eps.start, eps.goal)],
                                        dtype=np.int32))


def outcomes(want):
    ok = want["success"]
    return (ok & (want["spl"] == 1)).any() and (ok & (want["spl"] < 1)).any() and (~ok).any()


def sampled_ref(tables_, seed, per_bucket=16):
    """EpisodeSet.sample restated on the CPU: (scene, start, goal, distance)."""
    sc, st, gl, ds = [], [], [], []
    for k, geo in enumerate(tables_[1]):
        for b, (lo, hi) in enumerate(BUCKETS):
            pairs, dist, total = er.sample_episodes(geo, lo, hi, per_bucket, seed, k * 65536 + b)
            assert total > 0
            sc += [k] * per_bucket
            st += pairs[:, 0].tolist()
            gl += pairs[:, 1].tolist()
            ds += dist.tolist()
    return [np.array(x, dtype=np.int32) for x in (sc, st, gl, ds)]


def check_exact(res, eps, want):
    per = res["per_episode"]
    M = len(eps)
    assert res["episodes"] == M and np.array_equal(per["index"], np.arange(M))
    assert np.array_equal(per["success"], want["success"])
    assert np.array_equal(per["length"], want["length"]) and per["length"].dtype == np.int32
    assert per["spl"].dtype == np.float32 and per["spl"].tobytes() == want["spl"].tobytes()
    assert np.array_equal(per["start_distance"], want["start_distance"])
    assert np.array_equal(per["start_distance"], eps.distance)
    assert np.isfinite(per["reward"]).all() and per["reward"].dtype == np.float32

    def means(sel):
        n = float(sel.sum())
        return dict(episodes=int(n), success_rate=want["success"][sel].sum() / n,
                    spl=want["spl"][sel].astype(np.float64).sum() / n, episode_length=want["length"][sel].sum() / n,
                    start_distance=want["start_distance"][sel].sum() / n,
                    reward=per["reward"][sel].astype(np.float64).sum() / n)
    for k, v in means(np.ones(M, dtype=bool)).items():
        assert res[k] == v, k
    assert len(res["buckets"]) == len(eps.buckets)
    for b, row in enumerate(res["buckets"]):
        sel = eps.bucket == b
        assert row["bucket"] == eps.buckets[b] and row["episodes"] == sel.sum()
        if sel.any():
            for k, v in means(sel).items():
                assert row[k] == v, (b, k)
        else:
            assert all(row[k] != row[k] for k in KEYS[1:])


@pytest.mark.parametrize("recurrent", [False, True], ids=["ff", "lstm"])
def test_constant_policy_is_exact(tables, recurrent):
    vnav = _vnav()
    graphs, geos = tables
    tr = make(recurrent)
    tr.step()  # episodes in flight when the evaluation starts
    constant_policy(tr, ACTION)
    # an explicit set of 4 (< E): on scene 0 a success with SPL 1, one with SPL < 1 and a
    # time-out at distance 1-3, on scene 1 a pair at distance >= 9
    g0, s0 = er.qualifying(geos[0], 1, 3)
    walks = [er.walk_constant(graphs[0], geos[0], s, g, ACTION, LIMIT) for g, s in zip(g0, s0)]
    i_one = next(i for i, w in enumerate(walks) if w[0] and w[1] == 1)  # one step: SPL 1
    i_slow = next(i for i, w in enumerate(walks) if w[0] and w[1] == 3 and geos[0][g0[i], s0[i]] == 1)
    i_out = next(i for i, w in enumerate(walks) if not w[0])
    g9, s9 = er.qualifying(geos[1], 9, None)
    explicit = vnav.EpisodeSet(scene=[0, 0, 1, 0], start=[s0[i_slow], s0[i_one], s9[5], s0[i_out]],
                               goal=[g0[i_slow], g0[i_one], g9[5], g0[i_out]], env=tr.env)
    want = expected(tables, explicit)
    assert want["success"].tolist() == [True, True, False, False] and want["spl"][0] == np.float32(1) / np.float32(3)
    assert explicit.bucket.tolist() == [0, 0, 2, 0] and len(explicit) < E
    # a sampled set of 16 per scene and bucket (96 > E), its seed chosen on the CPU so that all
    # three outcomes occur
    seed = next(s for s in range(100) if outcomes(expected(tables, vnav.EpisodeSet(
        *sampled_ref(tables, s)[:3], distance=sampled_ref(tables, s)[3]))))
    sampled = vnav.EpisodeSet.sample(tr.env, 16, buckets=BUCKETS, seed=seed)
    ref = sampled_ref(tables, seed)
    for k, w in zip(("scene", "start", "goal", "distance"), ref):
        assert np.array_equal(getattr(sampled, k), w) and getattr(sampled, k).dtype == np.int32, k
    assert len(sampled) == 96 and np.bincount(sampled.bucket).tolist() == [32, 32, 32]
    for eps in (explicit, sampled):
        want = expected(tables, eps)
        for policy in ("sample", "greedy"):
            check_exact(tr.evaluate_episodes(eps, policy=policy, seed=3), eps, want)
    # no farther pair is reached by the rotation: buckets 4-8 and >= 9 fail whole
    res = tr.evaluate_episodes(sampled, policy="greedy")
    assert res["buckets"][1]["success_rate"] == 0 and res["buckets"][2]["success_rate"] == 0
    assert res["buckets"][1]["episode_length"] == LIMIT and 0 < res["buckets"][0]["success_rate"] < 1
    # a shorter limit for the evaluation alone
    short = tr.evaluate_episodes(explicit, max_episode_steps=2)
    assert short["per_episode"]["length"].tolist() == [2, 1, 2, 2] and tr.env.max_episode_steps == LIMIT
    assert tr.env.error_flags() == 0


@pytest.mark.parametrize("recurrent", [False, True], ids=["ff", "lstm"])
def test_every_episode_exactly_once_with_a_real_policy(tables, recurrent):
    vnav = _vnav()
    tr = make(recurrent)
    eps = vnav.EpisodeSet.sample(tr.env, 7, buckets=BUCKETS, seed=1)  # 42 episodes, not a multiple of anything
    res = tr.evaluate_episodes(eps, policy="sample", seed=11)
    per = res["per_episode"]
    geos = tables[1]
    want_d = np.array([geos[k][g, s] for k, s, g in zip(eps.scene, eps.start, eps.goal)], dtype=np.int32)
    assert res["episodes"] == len(eps) == 42
    assert np.array_equal(per["start_distance"], want_d) and np.array_equal(want_d, eps.distance)
    ok, p, l = per["success"], per["length"], per["start_distance"]
    assert (p[~ok] == LIMIT).all() and (p[ok] >= l[ok]).all() and (p >= 1).all() and (p <= LIMIT).all()
    spl = np.where(ok, l.astype(np.float32) / np.maximum(p, l).astype(np.float32), np.float32(0)).astype(np.float32)
    assert per["spl"].tobytes() == spl.tobytes()
    again = tr.evaluate_episodes(eps, policy="sample", seed=11)
    for k in per:
        assert np.array_equal(per[k], again["per_episode"][k]) and per[k].dtype == again["per_episode"][k].dtype, k
    assert {k: res[k] for k in KEYS} == {k: again[k] for k in KEYS}
    assert tr.env.error_flags() == 0


def snapshot(tr):
    out = dict(params=tr.params, square_avg=tr.square_avg, env=tr.env.get_state(), ret=tr.env.get_episode_returns(),
               nav=tr.env.get_nav_state(), sched=tr.sched)
    if tr.recurrent:
        out.update({k: getattr(tr, k) for k in tr._RECURRENT_STATE})
    return {k: v.detach().clone() for k, v in out.items()}


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("recurrent", [False, True], ids=["ff", "lstm"])
def test_training_is_untouched(recurrent, graph):
    vnav = _vnav()
    a, b = make(recurrent, graph), make(recurrent, graph)
    ma = [a.step() for _ in range(2)]
    before = snapshot(a)
    gen = a.env.config_generation
    eps = vnav.EpisodeSet.sample(a.env, 3, buckets=BUCKETS, seed=2)
    for policy in ("sample", "greedy"):
        res = a.evaluate_episodes(eps, policy=policy, seed=5)
        assert res["episodes"] == len(eps) == 18
    after = snapshot(a)
    for k in before:
        assert torch.equal(before[k], after[k]), k
    assert a.env.episode_log is None and a.env.config_generation > gen  # a captured update is recaptured
    ma += [a.step() for _ in range(2)]
    mb = [b.step() for _ in range(4)]
    sa, sb = snapshot(a), snapshot(b)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    for x, y in zip(ma, mb):
        assert set(x) == set(y)
        for k in x:
            if k != "fps":
                assert x[k] == y[k] or (x[k] != x[k] and y[k] != y[k]), k
    assert sum(m["episodes"] for m in mb) >= 1


def test_refusals(tables):
    vnav = _vnav()
    tr = make(False)
    good = vnav.EpisodeSet(scene=[0], start=[1], goal=[5], env=tr.env)
    empty = vnav.EpisodeSet(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32),
                            distance=np.zeros(0, np.int32))
    outside = [vnav.EpisodeSet([0], [10**6], [5], distance=[3]), vnav.EpisodeSet([2], [1], [5], distance=[3]),
               vnav.EpisodeSet([0], [1], [-1], distance=[3]), vnav.EpisodeSet([0], [1], [5], distance=[30000]),
               vnav.EpisodeSet([0], [5], [5], distance=[0])]
    for bad in [empty] + outside:
        with pytest.raises(ValueError):
            tr.evaluate_episodes(bad)
    with pytest.raises(ValueError):
        tr.evaluate_episodes(good, policy="best")
    with pytest.raises(ValueError):
        tr.evaluate_episodes(good, max_episode_steps=0)
    with pytest.raises(ValueError):
        vnav.EpisodeSet([0], [10**6], [5], env=tr.env)
    assert tr.evaluate_episodes(good)["episodes"] == 1
    with pytest.raises(ValueError, match="nav_metrics"):
        make(False, nav=False).evaluate_episodes(good)
    with pytest.raises(ValueError, match="time limit"):
        make(False, limit=0).evaluate_episodes(good)
