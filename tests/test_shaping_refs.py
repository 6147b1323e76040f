"""The restatements in tests/shaping_ref.py against what they must reduce to: the n-step returns of
oracle/a2c.py, the one-step target at lambda = 0, the telescoping sum of a potential-based shaping
term, the expert term's anneal, and the float32 form against exact rational arithmetic. CPU only."""
from fractions import Fraction

import numpy as np

from oracle import a2c as oa2c

import expert_ref as er
import nav_ref as nr
import shaping_ref as sr

EPS24 = 2.0 ** -24


def case(T, E, A, seed):
    rng = np.random.RandomState([11, T, E, A, seed])
    rewards = rng.randn(T, E).astype(np.float32)
    rewards[rng.rand(T, E) < 0.2] = np.float32(-0.0)
    dones = (rng.rand(T, E) < 0.15).astype(np.uint8)
    boot = np.full((E, 8), np.nan, dtype=np.float32)
    boot[:, A] = rng.randn(E).astype(np.float32)
    out = np.full((T * E, 8), np.nan, dtype=np.float32)
    out[:, A] = rng.randn(T * E).astype(np.float32)
    dist = rng.randint(-1, 13, size=(T, 2, E)).astype(np.int32)
    return rewards, dones, boot, out, dist


def test_n_step_form_is_the_oracles():
    for T, E, A in ((1, 1, 1), (20, 257, 4), (7, 3, 7)):
        rewards, dones, boot, out, dist = case(T, E, A, 0)
        want = oa2c.returns64(rewards, dones, boot, A, 0.99)
        for d, w in ((None, 0.5), (dist, 0.0), (None, 0.0)):
            got, M = sr.returns_ex64(rewards, dones, boot, None, d, A, 0.99, 1.0, w=w, gamma_phi=0.9)
            assert np.array_equal(got, want)
            assert M >= np.abs(want).max()


def test_lambda_zero_is_the_one_step_target():
    T, E, A = 9, 5, 4
    rewards, dones, boot, out, dist = case(T, E, A, 1)
    w, gp, g = np.float32(0.25), np.float32(0.99), float(np.float32(0.97))
    got, _ = sr.returns_ex64(rewards, dones, boot, out, dist, A, 0.97, 0.0, w=w, gamma_phi=gp)
    F, valid = sr.shaping_terms64(dist, w, gp)
    assert (~valid).any() and valid.any() and (F[~valid] == 0).all()
    V = out.astype(np.float64).reshape(T, E, 8)[:, :, A]
    Vn = np.concatenate([V[1:], boot[None, :, A].astype(np.float64)])
    want = rewards.astype(np.float64) + F + g * Vn * (1.0 - dones)
    assert np.abs(got - want).max() <= 4 * 2.0 ** -53 * np.abs(want).max()


def test_lambda_between_matches_the_direct_sum():
    """G_t = sum_k (gamma lambda)^k delta_{t+k} up to the first done, formed directly."""
    T, E, A = 6, 4, 2
    rewards, dones, boot, out, dist = case(T, E, A, 2)
    got, _ = sr.returns_ex64(rewards, dones, boot, out, None, A, 0.99, 0.95)
    g = float(np.float32(0.99))
    gl = float(np.float32(np.float32(0.99) * np.float32(0.95)))
    V = out.astype(np.float64).reshape(T, E, 8)[:, :, A]
    Vn = np.concatenate([V[1:], boot[None, :, A].astype(np.float64)])
    nd = 1.0 - dones
    delta = rewards.astype(np.float64) + g * Vn * nd - V
    for e in range(E):
        for t in range(T):
            G, c = 0.0, 1.0
            for k in range(t, T):
                G += c * delta[k, e]
                if dones[k, e]:
                    break
                c *= gl
            assert abs(got[t, e] - (G + V[t, e])) <= 1e-12 * (1 + abs(G))


def walk_episode(graph, start, goal, actions):
    """States after each action (a move off the graph keeps the state), until the goal."""
    s, out = start, []
    for a in actions:
        nxt = int(graph[s, a])
        s = s if nxt == -1 else nxt
        out.append(s)
        if s == goal:
            break
    return out


def test_shaping_telescopes_to_the_start_distance():
    """gamma_phi = 1 on an untruncated successful episode: sum_t F_t = w * start distance,
    whatever detours and blocked moves the path takes."""
    scene = nr.scene_a()
    graph, geo = scene.graph, nr.geodesic(scene.graph)
    rng = np.random.RandomState(4)
    n = len(graph)
    done_cases = 0
    for _ in range(40):
        goal, start = rng.randint(n), rng.randint(n)
        d0 = int(geo[goal, start])
        if d0 <= 0:
            continue
        # a random prefix (detours, blocked moves), then the optimal actions to the goal
        s, acts = start, []
        for a in rng.randint(0, 4, size=6):
            nxt = int(graph[s, a])
            if nxt == goal:
                continue
            acts.append(int(a))
            s = s if nxt == -1 else nxt
        while s != goal:
            a = nr.distance_mask_action(graph, geo, s, goal)[2]
            acts.append(a)
            s = int(graph[s, a])
        states = walk_episode(graph, start, goal, acts)
        assert states[-1] == goal and len(states) == len(acts)
        rec = sr.ProgressRecord(1)
        sr.progress_refresh([geo], [0], [start], [goal], rec)
        assert rec.dist[0] == d0
        dist = np.zeros((len(states), 2, 1), dtype=np.int32)
        prog = 0
        for t, st in enumerate(states):
            done = st == goal
            # after the terminal step the env already holds another episode: any state will do
            after_state = rng.randint(n) if done else st
            b, a, p = sr.progress_ref([geo], [0], [after_state], [goal], [done], [False], [st], rec)
            dist[t, 0, 0], dist[t, 1, 0] = b[0], a[0]
            prog += int(p[0])
        w = np.float32(0.3)
        F, valid = sr.shaping_terms64(dist, w, 1.0)
        assert valid.all() and prog == d0
        assert abs(F.sum() - float(w) * d0) <= 1e-12
        done_cases += 1
    assert done_cases >= 10


def test_truncation_and_unreachable_goal():
    """A truncated step measures the finished episode's goal at terminal_state, from the record,
    though the env has moved on; an unreachable goal gives progress 0 and an invalid pair."""
    geos = [nr.geodesic(nr.GRAPH_C), nr.geodesic(nr.scene_a().graph)]
    rec = sr.ProgressRecord(2)
    sr.progress_refresh(geos, [0, 0], [0, 4], [3, 0], rec)
    assert list(rec.dist) == [3, -1]
    # env 0 moves 0 -> 1 and is truncated, then reset into scene 1; env 1 stays unreachable
    b, a, p = sr.progress_ref(geos, [1, 0], [5, 4], [7, 0], [1, 0], [1, 0], [1, 4], rec)
    assert (list(b), list(a), list(p)) == ([3, -1], [2, -1], [1, 0])
    assert list(rec.scene) == [1, 0] and list(rec.goal) == [7, 0]
    assert rec.dist[0] == geos[1][7, 5]
    assert list(sr.shaping_stats(np.stack([b, a])[None])) == [3, 2, 1]


def test_anneal_is_the_expert_terms():
    assert sr.anneal_weight is er.anneal_weight
    for w0, steps, horizon in ((0.5, 0, 0), (0.5, 100, 1000), (0.3, 1000, 1000), (0.3, 5000, 1000), (1.0, 7, 3)):
        want = np.float32(np.float32(w0) * 1.0) if horizon <= 0 else \
            np.float32(float(np.float32(w0)) * max(0.0, 1.0 - steps / horizon))
        assert sr.anneal_weight(w0, steps, horizon) == want


def test_fma32_is_correctly_rounded():
    rng = np.random.RandomState(9)
    a = (rng.randn(4000) * 10.0 ** rng.randint(-3, 4, 4000)).astype(np.float32)
    b = (rng.randn(4000) * 10.0 ** rng.randint(-3, 4, 4000)).astype(np.float32)
    c = (rng.randn(4000) * 10.0 ** rng.randint(-3, 4, 4000)).astype(np.float32)
    c[:500] = -(a[:500] * b[:500])  # cancellation: the exact result is the product's rounding error
    got = sr.fma32(a, b, c)
    for i in range(len(a)):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = np.nextafter(got[i], np.float32(-np.inf))
        hi = np.nextafter(got[i], np.float32(np.inf))
        err = abs(Fraction(float(got[i])) - exact)
        assert err <= abs(Fraction(float(lo)) - exact) and err <= abs(Fraction(float(hi)) - exact), i


def test_float32_form_stays_within_the_stated_roundings():
    for T, E, A in ((20, 33, 4), (40, 7, 7)):
        rewards, dones, boot, out, dist = case(T, E, A, 3)
        for d, w, k in ((None, 0.0, sr.K_NSTEP), (dist, 0.5, sr.K_NSTEP_SHAPED)):
            ref, M = sr.returns_ex64(rewards, dones, boot, None, d, A, 0.99, 1.0, w=w, gamma_phi=0.99)
            got = sr.returns_ex32(rewards, dones, boot, d, A, 0.99, w=w, gamma_phi=0.99)
            assert got.dtype == np.float32
            assert np.abs(got.astype(np.float64) - ref).max() <= 2 * k * T * EPS24 * M
