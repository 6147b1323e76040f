"""CPU checks of the fixed-episode evaluation's restatement (tests/episodes_ref.py) and of the
pure helpers in vnav/episodes.py: pair totals pinned to independently counted figures, draws
inside their bucket, both ends of Q, the episode -> env assignment and the world slicing."""
import numpy as np
import pytest

import episodes_ref as er
import nav_ref
from vnav import episodes as ve
from vnav.scenes import synthetic_scene

BUCKETS = ((1, 3), (4, 8), (9, None))
# directed-BFS counts, made apart from the restatement
TOTALS = {
    ("a", 0): 224, ("a", 1): 238, ("a", 2): 0,
    ("b", 0): 1640, ("b", 1): 3972, ("b", 2): 2760,
    ("c", 0): 17, ("c", 1): 1,
    ("g12", 0): 7648, ("g12", 1): 27768,
}


@pytest.fixture(scope="module")
def geos():
    a, b, c = nav_ref.shared_scenes()
    return {"a": nav_ref.geodesic(a.graph), "b": nav_ref.geodesic(b.graph), "c": nav_ref.geodesic(c.graph),
            "g12": nav_ref.geodesic(synthetic_scene(0, grid=12).graph)}


def test_scene_sizes(geos):
    assert [len(geos[k]) for k in ("a", "b", "c", "g12")] == [22, 92, 7, 376]
    assert int((geos["c"] < 0).sum()) == 24


@pytest.mark.parametrize("key", sorted(TOTALS))
def test_pair_totals(geos, key):
    name, b = key
    g, s = er.qualifying(geos[name], *BUCKETS[b])
    assert len(g) == TOTALS[key]
    # ordered by g, then by s, without repeats
    flat = g.astype(np.int64) * len(geos[name]) + s
    assert (np.diff(flat) > 0).all()
    _, _, total = er.sample_episodes(geos[name], *BUCKETS[b], count=3, seed=1, salt=2)
    assert total == TOTALS[key]


def test_single_pair_bucket(geos):
    pairs, dist, total = er.sample_episodes(geos["c"], 4, 8, 9, seed=5, salt=0)
    assert total == 1 and (pairs == np.array([0, 4])).all() and (dist == 4).all()


def test_empty_bucket_writes_nothing(geos):
    pairs, dist, total = er.sample_episodes(geos["a"], 9, None, 5, seed=5, salt=0)
    assert total == 0 and (pairs == -1).all() and (dist == -1).all()


@pytest.mark.parametrize("name", ["a", "b", "c", "g12"])
def test_draws_lie_in_their_bucket(geos, name):
    geo = geos[name]
    for b, (lo, hi) in enumerate(BUCKETS):
        pairs, dist, total = er.sample_episodes(geo, lo, hi, 200, seed=11, salt=b)
        if total == 0:
            continue
        d = geo[pairs[:, 1], pairs[:, 0]]
        assert (d == dist).all() and (d >= lo).all() and (d <= (hi or 32767)).all()
        assert (pairs[:, 0] != pairs[:, 1]).all()


def test_index_hits_both_ends(geos):
    geo = geos["b"]
    g, s = er.qualifying(geo, 4, 8)
    pairs, _, total = er.sample_episodes(geo, 4, 8, 2, seed=0, salt=0, u=[0, 2**64 - 1])
    assert er.index_of(0, total) == 0 and er.index_of(2**64 - 1, total) == total - 1
    assert tuple(pairs[0]) == (s[0], g[0]) and tuple(pairs[1]) == (s[-1], g[-1])
    # the largest total of the contract
    assert er.index_of(2**64 - 1, 2**28) == 2**28 - 1


def test_draws_depend_on_seed_and_salt(geos):
    geo = geos["b"]
    base = er.sample_episodes(geo, 1, 3, 64, seed=3, salt=7)[0]
    assert (er.sample_episodes(geo, 1, 3, 64, seed=3, salt=7)[0] == base).all()
    assert (er.sample_episodes(geo, 1, 3, 64, seed=3, salt=8)[0] != base).any()
    assert (er.sample_episodes(geo, 1, 3, 64, seed=4, salt=7)[0] != base).any()
    # seeds beyond 32 bits reach the key's high word
    assert (er.sample_episodes(geo, 1, 3, 64, seed=3 + 2**32, salt=7)[0] != base).any()


def test_draws_are_near_uniform(geos):
    """4096 draws over the 17 pairs of nav-c 1-3: every pair within 6 sigma of 4096 / 17."""
    pairs, _, total = er.sample_episodes(geos["c"], 1, 3, 4096, seed=9, salt=1)
    _, n = np.unique(pairs[:, 1] * 7 + pairs[:, 0], return_counts=True)
    mean = 4096 / total
    assert len(n) == total and np.abs(n - mean).max() < 6 * np.sqrt(mean)


ASSIGN_CASES = [
    ("M < E", [0, 0, 1], 8, 2),
    ("M = E", [0, 1, 0, 1, 1], 5, 2),
    ("M not a multiple of m", [0] * 7, 3, 1),
    ("three unequal scenes", [0] * 11 + [1] * 2 + [2] * 30, 9, 3),
    ("a scene without episodes", [0, 2, 2, 2], 4, 3),
    ("one env per scene", [0, 1, 1, 1, 2], 3, 3),
]


@pytest.mark.parametrize("name,scene,E,S", ASSIGN_CASES, ids=[c[0] for c in ASSIGN_CASES])
def test_assignment_places_every_episode_once(name, scene, E, S):
    scene = np.array(scene)
    rng = np.random.RandomState(len(scene))
    scene = scene[rng.permutation(len(scene))]  # the set's order is not by scene
    env_scenes, env, slot, want, slots = ve.assign_episodes(scene, E, S)
    ref = er.assign(scene, E, S)
    for x, y in zip((env_scenes, env, slot, want), ref[:4]):
        assert np.array_equal(x, y)
    assert slots == ref[4]
    M = len(scene)
    assert len(env_scenes) == E and len(set(zip(env.tolist(), slot.tolist()))) == M
    assert (env_scenes[env] == scene).all()  # on an env of its own scene
    assert want.sum() == M and want.max() == slots
    for e in range(E):  # slots 0..want-1 of every env, none skipped
        assert sorted(slot[env == e].tolist()) == list(range(want[e]))
    for k in np.unique(scene):
        assert (env_scenes == k).sum() >= 1
        # order kept: a scene's later episode never sits in an earlier slot
        assert (np.diff(slot[scene == k]) >= 0).all()


def test_assignment_is_proportional():
    scene = np.array([0] * 100 + [1] * 300)
    env_scenes, _, _, want, slots = ve.assign_episodes(scene, 8, 2)
    assert (env_scenes == 0).sum() == 2 and (env_scenes == 1).sum() == 6 and slots == 50


def test_assignment_refusals():
    with pytest.raises(ValueError):
        ve.assign_episodes(np.zeros(0, np.int64), 4, 2)
    with pytest.raises(ValueError):
        ve.assign_episodes(np.array([0, 1, 2]), 2, 3)


@pytest.mark.parametrize("M,world", [(10, 1), (10, 3), (2, 4), (16, 4), (0, 2)])
def test_world_slices_partition_the_set(M, world):
    parts = [ve.world_slice(M, r, world) for r in range(world)]
    assert sorted(np.concatenate(parts).tolist()) == list(range(M))
    for r, p in enumerate(parts):
        assert (p % world == r).all() and (np.diff(p) > 0).all()


def test_log_rule():
    log = er.EpisodeLogRef(2, [0, 1, 2])
    ones = np.ones(3)
    for t in range(3):
        log.step([1, 1, t != 1], ones, ones * 0.5, ones * 4, ones * (t + 1), ones * -t)
    assert log.count.tolist() == [3, 3, 2]
    assert log.written.T.tolist() == [[False, False], [True, False], [True, True]]
    assert log.length[:, 2].tolist() == [1, 3] and log.length[0, 1] == 1


def test_buckets_and_parse():
    assert ve.parse_buckets("1-3,4-8,9-") == BUCKETS
    assert ve.bucket_of([0, 1, 3, 4, 8, 9, 500, -1], BUCKETS).tolist() == [-1, 0, 0, 1, 1, 2, 2, -1]


def test_episode_set_round_trip(tmp_path):
    s = ve.EpisodeSet([0, 1, 1], [3, 4, 5], [6, 7, 8], distance=[2, 5, 12])
    assert s.bucket.tolist() == [0, 1, 2] and len(s) == 3
    path = str(tmp_path / "set.npz")
    s.save(path)
    t = ve.EpisodeSet.load(path)
    for k in ("scene", "start", "goal", "distance", "bucket"):
        assert np.array_equal(getattr(s, k), getattr(t, k)) and getattr(t, k).dtype == np.int32
    assert t.buckets == s.buckets
    with pytest.raises(ValueError):
        ve.EpisodeSet([0], [1], [2])  # no distances and no env to take them from


def test_constant_action_walk_counts():
    """Action 2 on synthetic_scene(0, grid=6), time limit 12: of the 1640 pairs at distance 1-3,
    276 reach the goal, 92 of them with SPL < 1; no farther pair does."""
    graph = synthetic_scene(0, grid=6).graph
    geo = nav_ref.geodesic(graph)
    ok = {b: [er.walk_constant(graph, geo, s, g, 2, 12) for g, s in zip(*er.qualifying(geo, *BUCKETS[b]))]
          for b in range(3)}
    near = [w for w in ok[0] if w[0]]
    assert len(ok[0]) == 1640 and len(near) == 276 and sum(1 for w in near if w[2] < 1) == 92
    assert not any(w[0] for w in ok[1] + ok[2])
