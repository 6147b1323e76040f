"""The fp64 restatement of the PPO kernels (tests/ppo_ref.py) and its generated cases, on the CPU
alone: the restated gradient is the derivative of the restated loss, every sample of every case
is MARGIN clear of every decision boundary (no sample is left out of a comparison: the cap on
excluded samples is zero), and every branch of the loss is populated."""
import numpy as np
import pytest

import ppo_ref as ref


def _loss(out, out_old, actions, returns, stats2, A, value_clip):
    r = ref.loss_grad(out, out_old, actions, returns, stats2, A, value_clip=value_clip)
    n = out.shape[0]
    lv, pol, H = r["terms"][0].sum(), r["terms"][1].sum(), r["terms"][2].sum()
    return (ref.VC * lv + pol - ref.EC * H) / n


@pytest.mark.parametrize("value_clip", (0.0, ref.VALUE_CLIP))
def test_dout_is_the_derivative_of_the_loss(value_clip):
    n, A = 65, 4
    out, out_old, actions, returns, stats2, _ = ref.case(n, A, 1.0)
    out = out.astype(np.float64)
    got = ref.loss_grad(out, out_old, actions, returns, stats2, A, value_clip=value_clip)["dout"]
    h = 1e-6
    worst = 0.0
    for i in range(0, n, 7):
        for j in range(A + 1):
            up, dn = out.copy(), out.copy()
            up[i, j] += h
            dn[i, j] -= h
            num = (_loss(up, out_old, actions, returns, stats2, A, value_clip) -
                   _loss(dn, out_old, actions, returns, stats2, A, value_clip)) / (2 * h)
            worst = max(worst, abs(num - got[i, j]))
    assert worst <= 1e-8, worst
    assert (got[:, A + 1:] == 0).all()


def test_out_old_is_out_gives_a2c():
    """r = 1 everywhere: nothing clipped, kl = 0, and with no value clip the columns are A2C's."""
    n, A = 63, 4
    out, _, actions, returns, _, _ = ref.case(n, A, 1.0)
    r = ref.loss_grad(out, out, actions, returns, None, A, value_clip=0.0)
    assert r["ppo_stats4"][0] == 0.0 and r["ppo_stats4"][1] == 0.0 and r["ppo_stats4"][2] == n
    o = out.astype(np.float64)
    p, logp, H = ref.softmax_stats(o[:, :A])
    adv = returns.astype(np.float64) - o[:, A]
    ind = np.zeros((n, A))
    ind[np.arange(n), actions] = 1.0
    a2c = (-adv[:, None] * (ind - p) + ref.EC * p * (logp + H[:, None])) / n
    assert np.abs(r["dout"][:, :A] - a2c).max() <= 1e-15
    assert np.abs(r["dout"][:, A] - ref.VC * (-2.0 * adv) / n).max() <= 1e-15


@pytest.mark.parametrize("n,A,scale", ref.all_cases())
def test_cases_are_clear_of_every_boundary(n, A, scale):
    for normalize in (True, False):
        r = ref.case(n, A, scale, normalize)[5]
        assert set(r["margins"]) == {"r = 1 - c", "r = 1 + c", "s1 = s2", "|V - V_old| = cv", "e1^2 = e2^2"}
        for name, m in r["margins"].items():
            assert m.shape == (n,)
            assert (m >= ref.MARGIN).all(), (name, float(m.min()))  # every sample: none excluded
        # the surrogate's tie is a boundary only where the advantage is not zero
        out_of_range = ~r["branches"]["unclipped"]
        assert (np.abs(r["adv"][out_of_range]) > 0).all()


@pytest.mark.parametrize("n,A,scale", ref.all_cases())
def test_cases_populate_every_branch(n, A, scale):
    """One action gives r = 1 at every sample and one sample takes one branch, so every branch
    is asked of every case with n >= 63 and A >= 2; the value branches of every case with
    n >= 63."""
    r = ref.case(n, A, scale)[5]
    if n >= 63:
        assert r["branches"]["value clipped"].any() and r["branches"]["value unclipped"].any()
    if n >= 63 and A >= 2:
        for name, b in r["branches"].items():
            assert b.any(), name
    if A == 1:
        assert r["branches"]["unclipped"].all()


def test_adv_stats_and_adam_restatements():
    rng = np.random.RandomState(0)
    returns, out_old = rng.randn(257), rng.randn(257, 8)
    mean, rstd = ref.adv_stats(returns, out_old, 4, 1e-8)
    adv = returns - out_old[:, 4]
    assert abs(mean - adv.mean()) <= 1e-15 and abs(rstd - 1.0 / (adv.std() + 1e-8)) <= 1e-12 * rstd
    assert ref.adv_stats(returns[:1], out_old[:1], 4, 0.5)[1] == 2.0  # n = 1: std = 0
    # torch's Adam on the same numbers
    import torch
    p0, g = rng.randn(33), rng.randn(3, 33)
    tp = torch.nn.Parameter(torch.tensor(p0))
    opt = torch.optim.Adam([tp], lr=3e-4, betas=(0.9, 0.999), eps=1e-5)
    p, m, v = p0, np.zeros(33), np.zeros(33)
    for t in range(3):
        tp.grad = torch.tensor(g[t] * 0.5)
        opt.step()
        p, m, v, _ = ref.adam_step(p, g[t], m, v, t, 0.5, 3e-4, 0.9, 0.999, 1e-5)
        assert np.abs(tp.detach().numpy() - p).max() <= 1e-14
