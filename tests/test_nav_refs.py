"""The numpy / scipy restatement of the navigation info (tests/nav_ref.py) against hand-worked
values, and the new entry points' presence in libvnav.so. CPU only."""
import ctypes

import numpy as np

import nav_ref as nr

NAV_SYMBOLS = ("vn_nav_enable", "vn_set_nav_buffers", "vn_nav_table", "vn_get_nav_state", "vn_set_nav_state",
               "vn_nav_episode_stats")


def test_hand_built_graph_table():
    geo = nr.geodesic(nr.GRAPH_C)
    assert geo.dtype == np.int16 and geo.shape == (7, 7)
    assert np.array_equal(geo.T, nr.TABLE_C)  # geo is [goal, state], the table [state, goal]


def test_maze_geodesic_equals_spd():
    s = nr.scene_a()
    assert s.n_states == 22
    assert np.array_equal(nr.geodesic(s.graph).T, s.spd)


def test_oriented_geodesic_exceeds_spd():
    """On the h5 convention (forward, backward, rot+1, rot-1) spd counts no rotation on the way:
    a sideways neighbour costs rotate, move, rotate = 3 actions where spd says 1."""
    s = nr.scene_b()
    assert s.n_states == 92
    geo = nr.geodesic(s.graph).T.astype(np.int64)  # [state, goal] like spd
    assert (geo >= s.spd).all()
    assert (geo > s.spd).any()
    assert geo.max() == 17 and s.spd.max() == 13


def test_mask_and_action():
    g, geo = nr.GRAPH_C, nr.geodesic(nr.GRAPH_C)
    # state 1, goal 0: the ring needs 3 actions, the back edge on action 3 one
    assert nr.distance_mask_action(g, geo, 1, 0) == (1, 1 << 3, 3)
    assert nr.distance_mask_action(g, geo, 0, 4) == (4, 1, 0)
    assert nr.distance_mask_action(g, geo, 3, 4) == (1, 1 << 1, 1)
    assert nr.distance_mask_action(g, geo, 2, 2) == (0, 0, -1)    # on the goal
    assert nr.distance_mask_action(g, geo, 4, 0) == (-1, 0, -1)   # no way back from the spur
    assert nr.distance_mask_action(g, geo, 0, 5) == (-1, 0, -1)   # the island
    # two optimal first actions: the open 5x5 corner to corner
    a = nr.scene_a()
    ga = nr.geodesic(a.graph)
    d, mask, act = nr.distance_mask_action(a.graph, ga, 0, a.n_states - 1)
    assert d == 8 and bin(mask).count("1") == 2 and act == (mask & -mask).bit_length() - 1


def test_spl_cases_by_hand():
    f = np.float32
    assert nr.spl_value(True, 0, 0) == f(1.0)              # l = 0
    assert nr.spl_value(True, 0, 7) == f(1.0)
    assert nr.spl_value(True, 5, 5) == f(1.0)              # p = l
    assert nr.spl_value(True, 3, 7) == f(3.0) / f(7.0)     # p > l: one fp32 division
    assert nr.spl_value(True, 3, 7).dtype == np.float32
    assert nr.spl_value(True, 5, 3) == f(1.0)              # max(p, l): never above 1
    assert nr.spl_value(False, 3, 7) == f(0.0)             # failure
    assert nr.spl_value(True, -1, 4) == f(0.0)             # unreachable start
    assert nr.spl_value(False, -1, 11) == f(0.0)


def test_step_outputs_and_record_by_hand():
    """Two envs on (c), goal 0: env 0 walks 1 -> 2 -> 3 -> 0 (p = l = 3), env 1 starts on the
    spur (unreachable) and is truncated at step 3; both are then reset."""
    graphs, geos = [nr.GRAPH_C], [nr.geodesic(nr.GRAPH_C)]
    z = np.zeros(2, dtype=np.int64)
    rec = nr.NavRecord(2)
    goal = np.array([0, 0])
    o = nr.nav_refresh(graphs, geos, z, np.array([1, 4]), goal, z, rec)
    assert o["distance_to_goal"].tolist() == [1, -1] and rec.start.tolist() == [1, -1]
    rec.start[0] = 3  # as if the episode had started at state 1 before the back edge existed
    no = np.zeros(2, bool)
    for t, st in enumerate(([2, 4], [3, 4]), 1):
        o = nr.nav_outputs(graphs, geos, z, np.array(st), goal, z + t, no, no, z + t, rec)
        assert not o["success"].any() and o["spl"].tolist() == [0.0, 0.0]
        assert o["start_distance"].tolist() == [3, -1]
    # step 3: env 0 reaches the goal, env 1 hits the limit; the table shows the new episodes
    o = nr.nav_outputs(graphs, geos, z, np.array([2, 3]), np.array([0, 4]), z, np.array([True, True]),
                       np.array([False, True]), z + 3, rec)
    assert o["success"].tolist() == [True, False]
    assert o["spl"].tolist() == [1.0, 0.0]
    assert o["start_distance"].tolist() == [3, -1]       # the finished episodes'
    assert o["distance_to_goal"].tolist() == [2, 1]      # the new episodes'
    assert rec.start.tolist() == [2, 1] and rec.offset.tolist() == [0, 0]


def test_mid_episode_offset():
    graphs, geos = [nr.GRAPH_C], [nr.geodesic(nr.GRAPH_C)]
    z = np.zeros(1, dtype=np.int64)
    rec = nr.NavRecord(1)
    nr.nav_refresh(graphs, geos, z, np.array([1]), np.array([4]), z + 5, rec, enable=True)
    assert rec.start.tolist() == [3] and rec.offset.tolist() == [5]
    o = nr.nav_outputs(graphs, geos, z, np.array([0]), np.array([2]), z, np.array([True]), np.array([False]),
                       z + 9, rec)
    assert o["spl"][0] == np.float32(3.0) / np.float32(4.0)  # p = 9 - 5


def test_library_exports_nav_symbols(built_lib):
    import torch  # noqa: F401  (shares torch's HIP runtime, as the product does)
    lib = ctypes.CDLL(built_lib)
    missing = [s for s in NAV_SYMBOLS if not hasattr(lib, s)]
    assert not missing, missing
    from vnav import _lib
    assert set(NAV_SYMBOLS) <= set(_lib.SIGNATURES)
    lib = _lib.load()
    assert lib.vn_nav_enable(None, 1) != 0  # NULL ctx is refused with a message, no device call
    assert "NULL" in _lib.last_error()
