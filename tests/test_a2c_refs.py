"""The float64 references of the A2C step / update kernels (oracle/a2c.py) on the CPU:
against the torch restatements of the same math at 1e-5, and the share of categorical draws
of the GPU tests' inputs (oracle/a2c_cases.py) that lie within DRAW_MARGIN of a CDF boundary
— those are left out of the exact comparison on the GPU and must stay under 0.1 %."""
import numpy as np
import pytest
import torch

from oracle import a2c as oa2c
from oracle import a2c_cases as cases
from oracle import philox


def _close(a, b, rtol, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    scale = max(np.abs(b).max(), 1e-30)
    err = np.abs(a - b).max() / scale
    assert err <= rtol, "%s: max err %.3g of scale %.3g" % (what, err, scale)


@pytest.mark.parametrize("T,E,A", [(1, 1, 1), (9, 37, 4), (20, 5, 7)])
def test_returns64_vs_torch(T, E, A):
    rng = np.random.RandomState(T * 100 + E)
    rewards = rng.randn(T, E).astype(np.float32)
    dones = rng.rand(T, E) < 0.15
    boot = rng.randn(E, 8).astype(np.float32)
    vext = torch.zeros(T + 1, E, dtype=torch.float64)
    vext[T] = torch.as_tensor(boot[:, A]).double()
    ref = oa2c.returns(torch.as_tensor(rewards).double(), torch.as_tensor(dones), vext, float(np.float32(0.99)))
    _close(oa2c.returns64(rewards, dones, boot, A, 0.99), ref.numpy(), 1e-5, "returns")


@pytest.mark.parametrize("n,A,scale", [(1, 1, 1.0), (64, 2, 1.0), (257, 4, 1.0), (257, 7, 30.0), (33, 4, 30.0)])
def test_loss_grad64_vs_autograd(n, A, scale):
    rng = np.random.RandomState(n + A)
    out = np.full((n, 8), np.nan, dtype=np.float32)
    out[:, :A] = (rng.randn(n, A) * scale).astype(np.float32)
    out[:, A] = rng.randn(n).astype(np.float32)
    actions = rng.randint(0, A, size=n)
    rets = rng.randn(n).astype(np.float32)
    dout, stats, mags = oa2c.loss_grad64(out, actions, rets, A, 0.5, 0.01)
    lg = torch.as_tensor(out[:, :A]).double().requires_grad_(True)
    v = torch.as_tensor(out[:, A]).double().requires_grad_(True)
    loss, parts = oa2c.loss(lg, v, torch.as_tensor(actions), torch.as_tensor(rets).double(),
                            float(np.float32(0.5)), float(np.float32(0.01)))
    loss.backward()
    _close(dout[:, :A], lg.grad.numpy(), 1e-5, "dlogits")
    _close(dout[:, A], v.grad.numpy(), 1e-5, "dvalue")
    assert np.all(dout[:, A + 1:] == 0.0)
    for k, name in enumerate(("value_loss", "action_loss", "entropy")):
        assert abs(stats[k] / n - parts[name].item()) <= 1e-5 * max(mags[k] / n, 1e-30), name
    assert abs(stats[3] - float(rets.astype(np.float64).sum())) <= 1e-12 * max(mags[3], 1.0)
    assert np.all(mags >= np.abs(stats))


def test_softmax_stats64_underflow():
    p, lp, H = oa2c.softmax_stats64(np.array([[0.0, -2000.0, 0.0]]))
    assert p[0, 1] == 0.0 and np.isfinite(H[0]) and abs(H[0] - np.log(2.0)) < 1e-15
    assert np.isfinite(lp).all()


def test_softmax_stats64_keeps_precision_when_saturated():
    """One action at probability 1 - s, s = e^-40 / (1 + e^-40): log p_0 = -log1p(e^-40) and
    H = p_0 log1p(e^-40) + p_1 (40 + log1p(e^-40)) to float64 precision, where log(1 + e^-40)
    would be exactly 0."""
    p, lp, H = oa2c.softmax_stats64(np.array([[3.0, -37.0]]))
    s = np.exp(-40.0)
    assert abs(lp[0, 0] + np.log1p(s)) <= 1e-15 * s and lp[0, 0] < 0.0
    want = np.log1p(s) / (1.0 + s) + s / (1.0 + s) * (40.0 + np.log1p(s))
    assert abs(H[0] - want) <= 1e-14 * want
    assert abs(p.sum() - 1.0) < 1e-15


@pytest.mark.parametrize("max_norm", [0.5, 1e9, 0.0, -1.0])
def test_grad_norm64_and_rmsprop64_vs_torch(max_norm):
    rng = np.random.RandomState(3)
    P = 1001
    p0 = rng.randn(P).astype(np.float32)
    sq0 = (rng.rand(P) * 1e-3).astype(np.float32)
    g = rng.randn(P).astype(np.float32)
    g[::50] = 0.0
    sq0[::50] = 0.0
    scale = 0.5
    norm, coef = oa2c.grad_norm64(g, scale, max_norm)
    assert abs(norm - np.sqrt(((g.astype(np.float64) * 0.5) ** 2).sum())) <= 1e-12 * norm
    if max_norm <= 0.0 or max_norm == 1e9:
        assert coef == 1.0
    else:
        assert coef < 1.0
    pn, sn = oa2c.rmsprop64(p0, g, sq0, coef, scale, 7e-4, 0.99, 1e-5)
    if max_norm > 0.0:  # torch's clip_grad_norm_ has no "off": compare where it applies
        pr, sr = [torch.as_tensor(p0).double()], [torch.as_tensor(sq0).double()]
        tn = oa2c.clip_and_rmsprop(pr, [torch.as_tensor(g).double() * scale], sr, float(np.float32(7e-4)),
                                   max_norm=float(np.float32(max_norm)), alpha=float(np.float32(0.99)),
                                   eps=float(np.float32(1e-5)))
        assert abs(tn.item() - norm) <= 1e-5 * norm
        _close(pn - p0, pr[0].numpy() - p0, 1e-5, "parameter step")
        _close(sn, sr[0].numpy(), 1e-5, "square_avg")
    assert np.array_equal(pn[::50], p0[::50].astype(np.float64)) and np.all(sn[::50] == 0.0)


def test_schedule64_and_step_post64():
    st, lr = oa2c.schedule64([40, 500, 7], 7e-4, 1000.0, 80, 20)
    assert st.tolist() == [60, 580, 40] and lr == np.float32(7e-4 * 0.5)
    assert oa2c.schedule64([0, 2000, 0], 7e-4, 1000.0, 80, 20)[1] == np.float32(0.0)
    assert oa2c.schedule64([0, 2000, 0], 7e-4, 0.0, 80, 20)[1] == np.float32(7e-4)
    lra, m, stats = oa2c.step_post64([2, 0, 3], [0.5, -0.25, 1.0], [0, 1, 1], [9.0, 2.5, -1.0], [4, 7, 3], 4)
    assert lra.tolist() == [[0, 0, 1, 0, 0.5], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]]
    assert m.tolist() == [1.0, 0.0, 0.0] and stats.tolist() == [2.0, 1.5, 10.0]


def test_categorical_draw64_is_the_inverse_cdf():
    """Against a scalar restatement of sample_action (first j with u < c_j, else A - 1), the
    Philox words laid out as the kernel lays them: (i, ctr_lo, ctr_hi, STREAM_POLICY)."""
    rng = np.random.RandomState(0)
    n, A, seed, ctr = 200, 5, 0x1234567890ABCDEF, cases.COUNTER_BASE + 3
    logits = rng.randn(n, 8) * 2.0
    act, dist = oa2c.categorical_draw64(logits, A, seed, ctr, np.arange(n))
    k0, k1 = philox.seed_key(seed)
    for i in range(n):
        r = philox.philox4x32_10(i, ctr & 0xFFFFFFFF, ctr >> 32, 3, k0, k1)[0]
        u = float(int(r) >> 8) / 16777216.0
        z = np.exp(logits[i, :A] - logits[i, :A].max())
        p = z / z.sum()
        a, c, gaps = A - 1, 0.0, []
        for j in range(A - 1):
            c += p[j]
            gaps.append(abs(u - c))
        c = 0.0
        for j in range(A - 1):
            c += p[j]
            if u < c:
                a = j
                break
        assert act[i] == a and abs(dist[i] - min(gaps)) < 1e-12
    assert np.isinf(oa2c.categorical_draw64(logits, 1, seed, ctr, np.arange(n))[1]).all()
    assert (oa2c.categorical_draw64(logits, 1, seed, ctr, np.arange(n))[0] == 0).all()


@pytest.mark.parametrize("E,A", cases.STEP_CASES)
def test_step_draws_stay_clear_of_cdf_boundaries(E, A):
    """Every (seed, counter, E, A, step) the fused-step GPU tests draw with: the share of
    draws within DRAW_MARGIN of a boundary is at most 0.1 %."""
    near = total = 0
    for t in range(cases.STEP_K):
        out = cases.step_policy_out(E, A, t)
        assert np.isnan(out[:, A + 1:]).all() and np.isfinite(out[:, :A + 1]).all()
        _, dist = oa2c.categorical_draw64(out, A, cases.STEP_SEED, cases.COUNTER_BASE + t, np.arange(E))
        near += int((dist < cases.DRAW_MARGIN).sum())
        total += E
    assert near <= cases.MAX_EXCLUDED_SHARE * total, (near, total)


@pytest.mark.parametrize("E", cases.HEADS_CASES)
def test_heads_draws_stay_clear_of_cdf_boundaries(E):
    """The in-step heads' draws (a handful): none within HEADS_CPU_MARGIN of a boundary of
    the fp64 heads' distribution, so none within DRAW_MARGIN of the fp32 heads' one."""
    w, b, h = cases.heads_inputs(E)
    logits = h.astype(np.float64) @ w.astype(np.float64).T + b.astype(np.float64)
    _, dist = oa2c.categorical_draw64(logits, cases.HEADS_A, cases.HEADS_SEED, cases.COUNTER_BASE, np.arange(E))
    assert (dist >= cases.HEADS_CPU_MARGIN).all(), dist.min()
