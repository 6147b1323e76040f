"""tests/ppo_kl_ref.py on its own, no GPU: every decision case keeps the fp64 KL CLEARANCE away
from its limit (and that clearance is at least 100 times the bar the kernel's KL is held to), both
outcomes occur; the restated KL is ppo_ref's ppo_stats4[0] / n; the gate's restatement is sticky and
strict; the restated gated steps are the ungated restatements at flag 0 and the identity at flag 1."""
import numpy as np

import ppo_kl_ref as kref
import ppo_ref as ref


def test_every_decision_case_is_clear_of_its_limit():
    outcomes = set()
    cases = kref.decision_cases()
    assert len(cases) == len(kref.NS) * (1 + 2 * (len(kref.AS) - 1)) * len(kref.SCALES)  # none left out
    for n, A, scale, limit in cases:
        out, out_old, actions, k, mag, _ = kref.case(n, A, scale)
        limit = float(limit)
        assert limit >= 0.0
        assert abs(k - limit) >= kref.CLEARANCE * limit, (n, A, scale, limit, k)
        # the kernel's KL is held to 1e-5 of the terms' mean magnitude: the clearance is 100 bars wide
        assert abs(k - limit) >= 100.0 * 1e-5 * mag, (n, A, scale, limit, k, mag)
        g, k2 = kref.gate(out, out_old, actions, A, limit)
        outcomes.add((A > 1, g[0]))
        assert g == ([1, 0] if k > limit else [0, 1]) and k2[0] == k and k2[1] == (k if g[0] else 0.0)
    assert outcomes == {(True, 0), (True, 1), (False, 0)}  # one action: the KL is exactly 0, nothing stops


def test_kl_is_ppo_refs_statistic():
    for n, A, scale in kref.all_cases():
        out, out_old, actions, k, mag, _ = kref.case(n, A, scale)
        returns = np.zeros(n, np.float32)  # the KL sum reads neither the returns nor the value column
        r = ref.loss_grad(out, out_old, actions, returns, None, A)
        assert abs(k - r["ppo_stats4"][0] / n) <= 1e-15 * max(mag, 1e-300), (n, A, scale)
        assert abs(mag - k) <= 1e-12 * mag  # every term is >= 0: the magnitudes' mean is the KL itself
        assert (k == 0.0) == (A == 1)


def test_gate_is_sticky_and_strict():
    out, out_old, actions, k, _, _ = kref.case(65, 4, 1.0)
    assert kref.gate(out, out_old, actions, 4, 0.0, (1, 5), (0.25, 0.5)) == ([1, 5], [0.25, 0.5])
    assert kref.gate(out, out, actions, 4, 0.0) == ([0, 1], [0.0, 0.0])  # kl == limit passes
    assert kref.gate(out, out_old, actions, 4, k) == ([0, 1], [k, 0.0])
    g, k2 = kref.gate(out, out_old, actions, 4, 2.0 * k, (0, 1))
    assert g == [0, 2] and k2 == [k, 0.0]


def test_gated_steps_are_the_ungated_ones_or_the_identity():
    rng = np.random.RandomState(3)
    n = 257
    p, g = rng.randn(n).astype(np.float32), (0.01 * rng.randn(n)).astype(np.float32)
    m, v, sq = (0.01 * rng.randn(n)).astype(np.float32), (1e-4 * rng.rand(n)).astype(np.float32), \
        (1e-4 * rng.rand(n)).astype(np.float32)
    adam = dict(t=3, coef=0.375, lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-5)
    want = ref.adam_step(p, g, m, v, **adam)
    got = kref.adam_step_gated(p, g, m, v, skip=0, **adam)
    assert all(np.array_equal(x, y) for x, y in zip(got[:3], want[:3])) and got[3] == 4
    got = kref.adam_step_gated(p, g, m, v, skip=1, **adam)
    assert all(np.array_equal(x, y.astype(np.float64)) for x, y in zip(got[:3], (p, m, v))) and got[3] == 3
    rms = dict(coef=0.375, lr=7e-4, alpha=0.99, eps=1e-5)
    want = kref.rmsprop_step(p, g, sq, **rms)
    got = kref.rmsprop_step_gated(p, g, sq, skip=0, **rms)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.abs(want[0] - p).max() > 0 and np.abs(want[1] - sq).max() > 0
    # the RMSprop restatement against the formula written out for one element
    gi = float(g[5]) * 0.375
    si = 0.99 * float(sq[5]) + (1.0 - 0.99) * gi * gi
    assert want[1][5] == si and want[0][5] == float(p[5]) - 7e-4 * gi / (np.sqrt(si) + 1e-5)
    got = kref.rmsprop_step_gated(p, g, sq, skip=1, **rms)
    assert np.array_equal(got[0], p.astype(np.float64)) and np.array_equal(got[1], sq.astype(np.float64))
