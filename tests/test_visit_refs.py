"""tests/visit_ref.py against values worked out by hand and against independent loops, on tiny
cases: a done with a scene change at the auto-reset, a truncation, an env that re-enters a state,
auto-reset off, the clamps, N == 0 and a cell out of range, and the anneal at 0, mid-way and past
the end. CPU only."""
from collections import Counter

import numpy as np

import visit_ref as vr


def two_scene_state():
    vs = vr.VisitState([3, 2], 2)
    vr.visit_start(vs, [0, 1], [1, 0])
    return vs


def test_enable_counts_the_current_states():
    vs = two_scene_state()
    assert vs.C == 5 and vs.W == 1 and list(vs.cell_off) == [0, 3, 5]
    assert list(vs.count) == [0, 1, 0, 1, 0]
    assert list(vs.ep_scene) == [0, 1] and list(vs.ep_distinct) == [1, 1]
    assert vs.seen == [{1}, {0}]


def test_step_reentry_done_with_scene_change_and_truncation():
    vs = two_scene_state()
    # step 1: env 0 moves to state 2; env 1 is blocked and re-enters state 0
    cell, first, cov = vr.visit_step(vs, [0, 1], [2, 0], [0, 0], [2, 0])
    assert list(cell) == [2, 3] and list(first) == [1, 0] and list(cov) == [0, 0]
    assert list(vs.count) == [0, 1, 1, 2, 0] and list(vs.ep_distinct) == [2, 1]
    # step 2: env 0 finishes in scene 0 at terminal_state 1 and resets into scene 1, state 1;
    # env 1 is truncated at terminal_state 1 of scene 1 and resets into scene 1, state 0
    cell, first, cov = vr.visit_step(vs, [1, 1], [1, 0], [1, 1], [1, 1])
    assert list(cell) == [1, 4] and list(first) == [0, 1] and list(cov) == [2, 2]
    assert list(vs.count) == [0, 2, 1, 3, 2]
    assert list(vs.ep_scene) == [1, 1] and list(vs.ep_distinct) == [1, 1]
    assert vs.seen == [{1}, {0}]
    packed = vs.packed()
    assert packed.dtype == np.int32 and list(packed) == [0, 2, 1, 3, 2, 1, 1, 1, 1, 2, 1]
    assert list(vs.stats()) == [4, 8] and list(vs.stats(0)) == [2, 3] and list(vs.stats(1)) == [2, 5]


def test_autoreset_off_keeps_the_episode():
    vs = two_scene_state()
    cell, first, cov = vr.visit_step(vs, [0, 1], [2, 0], [1, 0], [2, 0], autoreset=False)
    assert list(cell) == [2, 3] and list(first) == [1, 0] and list(cov) == [2, 0]
    assert vs.seen[0] == {1, 2} and vs.ep_distinct[0] == 2 and vs.ep_scene[0] == 0
    # the finished env is stepped again (done again): counted into the same episode
    cell, first, cov = vr.visit_step(vs, [0, 1], [0, 1], [1, 0], [0, 1], autoreset=False)
    assert list(cell) == [0, 4] and list(first) == [1, 1] and list(cov) == [3, 0]
    # vn_reset's form starts it, for the masked env only
    vr.visit_start(vs, [1, 1], [1, 1], mask=[1, 0])
    assert vs.seen == [{1}, {0, 1}] and list(vs.ep_scene) == [1, 1] and list(vs.ep_distinct) == [1, 2]
    assert list(vs.count) == [1, 1, 1, 2, 2]


def test_set_state_form_and_clear_and_clamps():
    vs = two_scene_state()
    before = vs.count.copy()
    vr.visit_start(vs, [-4, 9], [7, -1], add=False)  # clamped: (0, 2) and (1, 0)
    assert np.array_equal(vs.count, before) and vs.seen == [{2}, {0}] and list(vs.ep_scene) == [0, 1]
    vr.visit_clear(vs, [0, 0], [0, 0])
    assert list(vs.count) == [2, 0, 0, 0, 0] and list(vs.ep_distinct) == [1, 1]
    vs.ep_scene[0] = 5  # a bad restored record is clamped like a bad state
    cell, _, _ = vr.visit_step(vs, [0, 0], [0, 0], [1, 0], [9, 0])
    assert cell[0] == 4


def test_random_walk_against_independent_counting():
    """Counts are the multiset of arrivals plus the episode starts; coverage is the size of the
    set of states between two starts."""
    rng = np.random.RandomState(0)
    ns, E, T = [4, 33, 2], 5, 60
    vs = vr.VisitState(ns, E)
    scene = rng.randint(0, 3, E)
    state = np.array([rng.randint(0, ns[k]) for k in scene])
    vr.visit_start(vs, scene, state)
    arrivals = Counter(zip(scene.tolist(), state.tolist()))
    episode = [{(int(k), int(s))} for k, s in zip(scene, state)]
    ep_scene = scene.copy()
    for _ in range(T):
        done = rng.rand(E) < 0.3
        term = np.array([rng.randint(0, ns[k]) for k in ep_scene])
        scene = np.where(done, rng.randint(0, 3, E), scene)
        state = np.array([rng.randint(0, ns[k]) for k in scene])
        cell, first, cov = vr.visit_step(vs, scene, state, done, term)
        for e in range(E):
            arrived = (int(ep_scene[e]), int(term[e])) if done[e] else (int(scene[e]), int(state[e]))
            arrivals[arrived] += 1
            assert cell[e] == vs.cell_off[arrived[0]] + arrived[1]
            assert bool(first[e]) == (arrived not in episode[e])
            episode[e].add(arrived)
            assert cov[e] == (len(episode[e]) if done[e] else 0)
            if done[e]:
                start = (int(scene[e]), int(state[e]))
                arrivals[start] += 1
                episode[e] = {start}
                ep_scene[e] = scene[e]
        assert list(vs.ep_distinct) == [len(s) for s in episode]
    want = np.zeros(vs.C, dtype=np.uint32)
    for (k, s), c in arrivals.items():
        want[vs.cell_off[k] + s] = c
    assert np.array_equal(vs.count, want)
    assert list(vs.stats()) == [int((want > 0).sum()), int(want.sum())] and int(want.sum()) > E * T


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def test_bonus_by_hand():
    count = np.array([0, 1, 4, 16], dtype=np.uint32)
    r = np.array([[1.0, -0.0, 0.5], [-0.0, 2.0, -1.0]], dtype=np.float32)
    cell = np.array([[2, -1, 3], [0, 4, 1]], dtype=np.int32)  # -1 and C = 4 are outside, count[0] == 0
    first = np.array([[0, 0, 1], [0, 1, 1]], dtype=np.uint8)
    out, st = vr.novelty_rewards32(r, cell, first, count, 0.5, 0.25)
    want = np.array([[1.25, 0.0, 0.5 + (0.125 + 0.25)], [0.0, 2.25, -1.0 + 0.75]], dtype=np.float32)
    assert out.dtype == np.float32 and np.array_equal(bits(out), bits(want))
    assert bits(out)[0, 1] == 0 and bits(out)[1, 0] == 0  # -0.0 + (+0.0) = +0.0
    assert st["firsts"] == 3.0 and st["added"] == 0.25 + 0.375 + 0.25 + 0.75 and st["inv"] == 0.5 + 0.25 + 1.0
    assert st["wc"] == np.float32(0.5)
    # one rounding per operation: 0.1 / sqrt(3) in float32, by a plain loop
    f = np.float32
    b = f(f(0.1) / f(np.sqrt(f(3.0))))
    out, _ = vr.novelty_rewards32([[0.3]], [[0]], [[1]], np.array([3], dtype=np.uint32), 0.1, 0.2)
    assert bits(out)[0, 0] == bits(f(f(0.3) + f(b + f(0.2))))
    # 2^24 + 1 and 2^32 - 1 round to float32 before the root
    out, _ = vr.novelty_rewards32([[0.0, 0.0]], [[0, 1]], [[0, 0]],
                                  np.array([2**24 + 1, 2**32 - 1], dtype=np.uint32), 1.0, 0.0)
    assert np.array_equal(bits(out), bits([[f(1.0) / f(4096.0), f(1.0) / f(65536.0)]]))


def test_bonus_anneal():
    count = np.array([4], dtype=np.uint32)
    args = ([[0.0]], [[0]], [[1]], count, 0.5, 0.25)
    out0, s0 = vr.novelty_rewards32(*args, steps=0, anneal_steps=1000)
    assert out0[0, 0] == np.float32(0.5) and s0["wc"] == np.float32(0.5)
    mid, s1 = vr.novelty_rewards32(*args, steps=250, anneal_steps=1000)
    assert s1["wc"] == np.float32(0.375) and mid[0, 0] == np.float32(0.375 / 2 + 0.1875)
    end, s2 = vr.novelty_rewards32(*args, steps=1500, anneal_steps=1000)
    assert s2["wc"] == 0 and bits(end)[0, 0] == 0 and s2["added"] == 0.0 and s2["firsts"] == 1.0
    off, s3 = vr.novelty_rewards32(*args, steps=1500, anneal_steps=0)
    assert s3["wc"] == np.float32(0.5) and off[0, 0] == np.float32(0.5)
    third = vr.anneal_weight(0.1, 1, 3)  # fp64 product rounded once
    assert third == np.float32(float(np.float32(0.1)) * (1.0 - 1.0 / 3.0))
