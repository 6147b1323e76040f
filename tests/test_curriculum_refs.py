"""The restatement of the geodesic curriculum (tests/curriculum_ref.py) against plain loops on the
nav tests' three scenes, and its draw against the pinned oracle's: with geo.T handed to the
unmodified VectorEnvOracle as its spd, both draw the same starts. CPU only."""
import numpy as np
import pytest

import curriculum_ref as cr
import nav_ref as nr
from oracle.envs import VectorEnvOracle


@pytest.fixture(scope="module")
def scenes():
    return nr.shared_scenes()


@pytest.fixture(scope="module")
def geos(scenes):
    return [nr.geodesic(s.graph) for s in scenes]


def test_tables_against_loops(geos):
    assert np.array_equal(geos[2], nr.TABLE_C.T)
    for geo in geos:
        n = len(geo)
        D = max(int(v) for row in geo for v in row)
        order, count, gotD = cr.tables(geo)
        assert gotD == D and order.shape == (n, n) and count.shape == (n, D + 2)
        assert order.dtype == np.int32 and count.dtype == np.int32
        for g in range(n):
            key = [min(max(int(geo[g][s]), -1), D) + 1 for s in range(n)]
            buckets = [[s for s in range(n) if key[s] == b] for b in range(D + 2)]  # ascending s
            assert [s for b in buckets for s in b] == list(order[g])
            run, want = 0, []
            for b in buckets:
                run += len(b)
                want.append(run)
            assert want == list(count[g]) and count[g][-1] == n
    assert [cr.scene_D(g) for g in geos][1:] == [17, 4]


def test_clamp_level():
    assert [cr.clamp_level(l, 1, 17) for l in (-3, 0, 1, 9, 17, 22)] == [1, 1, 1, 9, 17, 17]
    assert cr.clamp_level(1, 3, 17) == 3 and cr.clamp_level(1, 3, 2) == 2 and cr.clamp_level(5, 1, 0) == 0


@pytest.mark.parametrize("mode", [1, 2])
def test_draw_is_the_pinned_oracles(scenes, geos, mode):
    """The unmodified oracle ranks by spd[s][g] with threshold floor(c (maxd + offset) + 1):
    with spd = geo.T, c = 1 and offset = level - 1 - D that is the level, exactly."""
    E, seed = 9, 21
    own = [dict(graph=s.graph, spd=s.spd, rewards=s.rewards, geo=g) for s, g in zip(scenes, geos)]
    pinned = [dict(graph=s.graph, spd=np.ascontiguousarray(np.asarray(g).T).astype(np.int64), rewards=s.rewards)
              for s, g in zip(scenes, geos)]
    a = cr.GeoCurriculumOracle(own, E, seed)
    b = VectorEnvOracle(pinned, E, seed)
    Ds = [cr.scene_D(g) for g in geos]
    for level in (1, 2, 3, 5, 40):
        levels = [cr.clamp_level(level, 1, D) for D in Ds]
        a.set_geo_curriculum(mode, levels)
        b.set_curriculum(1.0, [mode] * 3, [float(l - 1 - D) for l, D in zip(levels, Ds)])
        far = 0
        for sc, geo in enumerate(geos):
            for g in range(len(geo)):
                for e in range(E):
                    for k in (0, 1, 7):
                        x, y = a._curriculum_start(e, k, sc, g), b._curriculum_start(e, k, sc, g)
                        assert x == y, (level, sc, g, e, k)
                        if x is not None:
                            d = int(geo[g][x])
                            assert d >= 1
                            far += d > levels[sc]
                            if mode == 1 and (geo[g] > 0).any() and ((geo[g] > 0) & (geo[g] <= levels[sc])).any():
                                assert d <= levels[sc]
        assert (far > 0) == (mode == 2 and level < 40) or mode == 1


def test_controller_rule():
    c = cr.Controller([17, 4], [0, 1, 1], level=3, window=4, up=0.75, down=0.25, step=2, level_min=2)
    assert c.state().tolist() == [[3, 3], [0, 0], [0, 0], [17, 4]]
    c.count([1, 1, 0], [0, 1, 0], [1, 1, 0])  # env 0 ran in scene 0 and moves to scene 1
    assert c.state().tolist() == [[3, 3], [1, 1], [1, 0], [17, 4]]
    c.advance()  # no window full
    assert c.state().tolist()[0] == [3, 3]
    for _ in range(3):
        c.count([1, 1, 1], [0, 0, 1], [1, 1, 0])
    # scene 0: 1 + env 2's three truncated ones; scene 1: 1 + 6, six of them successes
    assert c.state().tolist()[1:3] == [[4, 7], [1, 6]]
    c.advance()  # 1 / 4 <= down: 3 - 2 held at level_min; 6 / 7 >= up: 3 + 2 held at D
    assert c.state().tolist() == [[2, 4], [0, 0], [0, 0], [17, 4]]
    # 3 / 4 = 0.75 >= up raises, 1 / 4 <= down lowers, between holds; fp32 division
    for succ, done, want in ((3, 4, 5), (1, 4, 2), (2, 4, 3), (1, 3, 3)):
        c = cr.Controller([17], [0], level=3, window=3, up=0.75, down=0.25, step=2, level_min=2)
        c.done[0], c.succ[0] = done, succ
        c.advance()
        assert c.level[0] == want and c.done[0] == 0 and c.succ[0] == 0
    c = cr.Controller([17], [0], level=3, window=0)
    c.count([1], [0], [0])
    c.advance()
    assert c.state().tolist() == [[3], [0], [0], [17]]
