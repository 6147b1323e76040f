"""csrc/vn_ppo.hip against the fp64 restatement of tests/ppo_ref.py: vn_ppo_loss_grad at one lane,
a ragged wave, a second wave, a second block and a ragged last block, for 1, 4 and 7 actions at
logit scale 1 and 8 (dout within 1e-5 of its scale, the unused columns exactly 0, each statistic
within 1e-5 of the sum of its terms' magnitudes: the bars of tests/test_a2c_kernels_gpu.py);
vn_ppo_adv_stats (1e-6 relative, equal bits over two runs, n = 1); vn_adam_step_dev over three
steps on float32 state, eager and inside a captured graph replayed three times; every VN_EINVAL
refusal writes nothing. The cases keep every sample 1e-4 clear of every decision boundary
(tests/test_ppo_refs.py), so no sample is left out."""
import ctypes

import numpy as np
import pytest
import torch

import ppo_ref as ref
from test_a2c_kernels_gpu import EPS24, NAN, VN_EINVAL, _l, full, host, report, same_bits, within, within_scale
from test_a2c_kernels_gpu import dev as _dev

pytestmark = pytest.mark.gpu

CF, I64 = ctypes.c_float, ctypes.c_int64


def dev(a):
    """A device copy (the shared cases are read-only arrays: torch wants a writable source)."""
    return _dev(np.array(a))


def _loss_grad(case, out_is_old=False, normalize=True, value_clip=ref.VALUE_CLIP):
    _lib, lib, st = _l()
    P = _lib.ptr
    out, out_old, actions, returns, stats2, _ = case
    n = out.shape[0]
    o_d = dev(out)
    old_d = o_d if out_is_old else dev(out_old)
    a_d, r_d = dev(actions), dev(returns)
    s2_d = dev(stats2) if normalize else None
    dout, stats, pstats = full((n, 8), NAN), full(4, NAN), full(4, NAN)

    def call(A):
        _lib.check(lib.vn_ppo_loss_grad(P(o_d), P(old_d), P(a_d), P(r_d), P(s2_d), n, A, CF(ref.CLIP), CF(value_clip),
                                        CF(ref.VC), CF(ref.EC), P(dout), P(stats), P(pstats), st), "vn_ppo_loss_grad")
        return host(dout).copy(), host(stats).copy(), host(pstats).copy()

    return call


@pytest.mark.parametrize("scale", ref.SCALES)
@pytest.mark.parametrize("A", ref.AS)
@pytest.mark.parametrize("n", ref.NS)
def test_loss_grad_vs_fp64(n, A, scale):
    for normalize in (True, False):
        case = ref.case(n, A, scale, normalize)
        r = case[5]
        call = _loss_grad(case, normalize=normalize)
        d, s4, p4 = call(A)
        tag = "ppo_loss_grad n=%d A=%d x%d norm=%d" % (n, A, int(scale), normalize)
        within_scale(tag + " dout", d[:, :A + 1], r["dout"][:, :A + 1], 1e-5)
        assert same_bits(d[:, A + 1:], np.zeros((n, 7 - A), dtype=np.float32))
        mags = np.abs(r["terms"]).sum(axis=1)
        want = np.concatenate([r["stats4"], r["ppo_stats4"]])
        within(tag + " stats", np.concatenate([s4, p4]), want, 1e-5 * mags)
        # the flags are sums of exact 0 / 1: every sample took the reference's branch
        assert p4[1] == r["ppo_stats4"][1] and p4[3] == r["ppo_stats4"][3]
        # zeroed by the call itself: the second call's values are within the bound, not doubled
        d2, s4b, p4b = call(A)
        within(tag + " stats, 2nd call", np.concatenate([s4b, p4b]), want, 1e-5 * mags)
        assert same_bits(d2, d)


@pytest.mark.parametrize("A", ref.AS)
@pytest.mark.parametrize("n", ref.NS)
def test_loss_grad_value_clip_off_is_the_a2c_value_column(n, A):
    case = ref.case(n, A, 1.0)
    out, out_old, actions, returns, stats2, _ = case
    r = ref.loss_grad(out, out_old, actions, returns, stats2, A, value_clip=0.0)
    d, s4, p4 = _loss_grad(case, value_clip=0.0)(A)
    within_scale("ppo_loss_grad n=%d A=%d cv=0 dout" % (n, A), d[:, :A + 1], r["dout"][:, :A + 1], 1e-5)
    within("ppo_loss_grad n=%d A=%d cv=0 value loss" % (n, A), s4[0], r["stats4"][0], 1e-5 * r["terms"][0].sum())
    assert p4[3] == 0.0


@pytest.mark.parametrize("A", ref.AS)
@pytest.mark.parametrize("n", ref.NS)
def test_loss_grad_out_old_is_out(n, A):
    """r is exactly 1: nothing clipped, the kl sum exactly 0, the ratio sum exactly n, and the
    columns are vn_a2c_loss_grad's on the same inputs."""
    _lib, lib, st = _l()
    P = _lib.ptr
    case = ref.case(n, A, 8.0)
    out, _, actions, returns = case[:4]
    d, s4, p4 = _loss_grad(case, out_is_old=True, normalize=False, value_clip=0.0)(A)
    assert p4[0] == 0.0 and p4[1] == 0.0 and p4[2] == float(n) and p4[3] == 0.0
    dout, stats = full((n, 8), NAN), full(4, NAN)
    o_d, a_d, r_d = dev(out), dev(actions), dev(returns)
    _lib.check(lib.vn_a2c_loss_grad(P(o_d), P(a_d), P(r_d), n, A, CF(ref.VC), CF(ref.EC), P(dout), P(stats), st),
               "vn_a2c_loss_grad")
    a2c = host(dout)
    # the same fp32 expression in both kernels, up to how the compiler contracts its three
    # products and sums: a few roundings of 2^-24 of the column's scale
    within_scale("ppo out_old=out vs a2c n=%d A=%d" % (n, A), d[:, :A + 1], a2c[:, :A + 1].astype(np.float64), 1e-6)
    r = ref.loss_grad(out, out, actions, returns, None, A, value_clip=0.0)
    within_scale("ppo out_old=out vs fp64 n=%d A=%d" % (n, A), d[:, :A + 1], r["dout"][:, :A + 1], 1e-5)


@pytest.mark.parametrize("n", ref.NS + (4099,))
def test_adv_stats_vs_fp64(n):
    """4099 rows: every thread of the one workgroup strides."""
    _lib, lib, st = _l()
    P = _lib.ptr
    A = 4
    rng = np.random.RandomState([11, n])
    returns = (3.0 + 2.0 * rng.randn(n)).astype(np.float32)
    out_old = rng.randn(n, 8).astype(np.float32)
    r_d, o_d = dev(returns), dev(out_old)
    runs = []
    for _ in range(2):
        s2 = full(2, NAN)
        _lib.check(lib.vn_ppo_adv_stats(P(r_d), P(o_d), n, A, CF(ref.ADV_EPS), P(s2), st), "vn_ppo_adv_stats")
        runs.append(host(s2).copy())
    assert same_bits(runs[0], runs[1])
    # the kernel forms adv in fp32 (one rounding of returns - V, as the loss kernel does)
    adv32 = (returns - out_old[:, A]).astype(np.float32)
    want = ref.adv_stats(adv32, np.zeros((n, 8)), A, np.float32(ref.ADV_EPS))
    got = runs[0].astype(np.float64)
    if n == 1:  # std = 0: the mean is the sample, rstd = 1 / eps
        assert same_bits(runs[0][0], adv32[0]) and same_bits(runs[0][1], np.float32(1.0 / np.float64(np.float32(ref.ADV_EPS))))
        return
    rel = np.abs(got - want) / np.abs(want)
    report("adv_stats n=%d (relative)" % n, rel.max(), 1e-6)
    assert (rel <= 1e-6).all(), (got, want)


def _adam_case(n, steps=3):
    rng = np.random.RandomState([12, n])
    p0 = rng.randn(n).astype(np.float32)
    gs = [(rng.randn(n) * 0.01).astype(np.float32) for _ in range(steps)]
    return p0, gs


ADAM = dict(scale=0.5, coef=0.75, lr=3e-4, b1=0.9, b2=0.999, eps=1e-5)


def _adam_call(lib, _lib, st, p, g, m, v, n, scalars, lr_d, step_d):
    P = _lib.ptr
    _lib.check(lib.vn_adam_step_dev(P(p), P(g), P(m), P(v), I64(n), CF(ADAM["scale"]), P(scalars), P(lr_d), P(step_d),
                                    CF(ADAM["b1"]), CF(ADAM["b2"]), CF(ADAM["eps"]), st), "vn_adam_step_dev")


def _adam_check(tag, it, p_in, m_in, v_in, g, p_out, m_out, v_out):
    b1, b2 = float(np.float32(ADAM["b1"])), float(np.float32(ADAM["b2"]))
    pr, mr, vr, step_ref = ref.adam_step(p_in, g, m_in, v_in, it, np.float32(ADAM["coef"]) * np.float32(ADAM["scale"]),
                                         np.float32(ADAM["lr"]), b1, b2, np.float32(ADAM["eps"]))
    em = np.abs(m_out - mr).max() / np.abs(mr).max()
    ev = np.abs(v_out - vr).max() / np.abs(vr).max()
    bound = 1e-5 * np.abs(step_ref).max() + EPS24 * np.abs(p_in).max()
    ep = np.abs((p_out.astype(np.float64) - p_in.astype(np.float64)) + step_ref).max()
    report("%s step %d moments (of scale)" % (tag, it), max(em, ev), 1e-6)
    report("%s step %d parameter step (of its bound)" % (tag, it), ep / bound, 1.0)
    assert em <= 1e-6 and ev <= 1e-6, (tag, it, em, ev)
    assert ep <= bound, (tag, it, ep, bound)


@pytest.mark.parametrize("n", [1, 257, 131072 + 5, 524288 + 5])
def test_adam_vs_fp64(n):
    """Three steps, each from the kernel's own float32 state. adam_kernel's grid is capped at
    2048 blocks of 256 as rmsprop_kernel's: 524288 + 5 runs its stride loop."""
    _lib, lib, st = _l()
    p0, gs = _adam_case(n)
    p, m, v = dev(p0), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    scalars = dev(np.array([2.0, ADAM["coef"]], dtype=np.float32))
    lr_d = dev(np.array([ADAM["lr"]], dtype=np.float32))
    step_d = torch.zeros(1, dtype=torch.int64, device="cuda")
    for it, g in enumerate(gs):
        p_in, m_in, v_in = host(p).copy(), host(m).copy(), host(v).copy()
        _adam_call(lib, _lib, st, p, dev(g), m, v, n, scalars, lr_d, step_d)
        assert int(step_d) == it + 1
        _adam_check("adam n=%d" % n, it, p_in, m_in, v_in, g, host(p), host(m), host(v))


def test_adam_in_a_captured_graph():
    """One captured step replayed three times: lr and the step count are read on the device, so
    every replay takes its own bias corrections and the learning rate written between them."""
    _lib, lib, _ = _l()
    n = 257
    p0, gs = _adam_case(n)
    p, m, v = dev(p0), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    g_d = torch.zeros(n, device="cuda")
    scalars = dev(np.array([2.0, ADAM["coef"]], dtype=np.float32))
    lr_d = dev(np.array([ADAM["lr"]], dtype=np.float32))
    step_d = torch.zeros(1, dtype=torch.int64, device="cuda")
    # the same three steps eagerly, for the bits
    pe, me, ve, se = dev(p0), torch.zeros_like(m), torch.zeros_like(v), torch.zeros_like(step_d)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # the capture stream is the current one inside
        _adam_call(lib, _lib, _lib.stream_ptr(torch.device("cuda", 0)), p, g_d, m, v, n, scalars, lr_d, step_d)
    assert int(step_d) == 0 and same_bits(host(p), p0)  # capture ran nothing
    for it, g in enumerate(gs):
        lr = np.float32(ADAM["lr"] * (1.0 - 0.25 * it))
        lr_d.copy_(dev(np.array([lr], dtype=np.float32)))
        g_d.copy_(dev(g))
        p_in, m_in, v_in = host(p).copy(), host(m).copy(), host(v).copy()
        graph.replay()
        torch.cuda.synchronize()
        assert int(step_d) == it + 1
        _adam_call(lib, _lib, _lib.stream_ptr(torch.device("cuda", 0)), pe, g_d, me, ve, n, scalars, lr_d, se)
        assert same_bits(host(p), host(pe)) and same_bits(host(m), host(me)) and same_bits(host(v), host(ve))
        b1, b2 = float(np.float32(ADAM["b1"])), float(np.float32(ADAM["b2"]))
        _, _, _, step_ref = ref.adam_step(p_in, g, m_in, v_in, it, np.float32(ADAM["coef"]) * np.float32(ADAM["scale"]),
                                          lr, b1, b2, np.float32(ADAM["eps"]))
        bound = 1e-5 * np.abs(step_ref).max() + EPS24 * np.abs(p_in).max()
        assert np.abs((host(p).astype(np.float64) - p_in) + step_ref).max() <= bound, it


def test_refusals_write_nothing():
    _lib, lib, st = _l()
    P = _lib.ptr
    n, A = 65, 4
    out, out_old, actions, returns, stats2, _ = ref.case(n, A, 1.0)
    o, oo, a, r, s2 = dev(out), dev(out_old), dev(actions), dev(returns), dev(stats2)
    dout, stats, pstats = full((n, 8), NAN), full(4, NAN), full(4, NAN)
    good = dict(out=o, out_old=oo, actions=a, returns=r, s2=s2, n=n, A=A, clip=0.2, dout=dout, stats=stats,
                pstats=pstats)

    def loss(**kw):
        g = dict(good, **kw)
        return lib.vn_ppo_loss_grad(P(g["out"]), P(g["out_old"]), P(g["actions"]), P(g["returns"]), P(g["s2"]), g["n"],
                                    g["A"], CF(g["clip"]), CF(0.2), CF(0.5), CF(0.01), P(g["dout"]), P(g["stats"]),
                                    P(g["pstats"]), st)

    bad = [dict(out=None), dict(out_old=None), dict(actions=None), dict(returns=None), dict(dout=None),
           dict(stats=None), dict(pstats=None), dict(n=0), dict(n=-3), dict(A=0), dict(A=8), dict(clip=0.0),
           dict(clip=-0.2), dict(clip=NAN)]
    for kw in bad:
        assert loss(**kw) == VN_EINVAL, kw
    torch.cuda.synchronize()
    for t in (dout, stats, pstats):
        assert torch.isnan(t).all()
    assert loss(s2=None) == 0  # the statistics may be NULL

    s_out = full(2, NAN)

    def adv(returns=r, out_old=oo, n=n, A=A, eps=1e-8, out=s_out):
        return lib.vn_ppo_adv_stats(P(returns), P(out_old), n, A, CF(eps), P(out), st)

    for kw in (dict(returns=None), dict(out_old=None), dict(out=None), dict(n=0), dict(n=-1), dict(A=0), dict(A=8),
               dict(eps=0.0), dict(eps=-1e-8), dict(eps=NAN)):
        assert adv(**kw) == VN_EINVAL, kw
    torch.cuda.synchronize()
    assert torch.isnan(s_out).all()

    p, g, m, v = full(n, NAN), full(n, NAN), full(n, NAN), full(n, NAN)
    scalars, lr_d = full(2, NAN), full(1, NAN)
    step_d = torch.full((1,), 7, dtype=torch.int64, device="cuda")
    base = dict(p=p, g=g, m=m, v=v, n=n, scalars=scalars, lr=lr_d, step=step_d)

    def adam(**kw):
        q = dict(base, **kw)
        return lib.vn_adam_step_dev(P(q["p"]), P(q["g"]), P(q["m"]), P(q["v"]), I64(q["n"]), CF(1.0), P(q["scalars"]),
                                    P(q["lr"]), P(q["step"]), CF(0.9), CF(0.999), CF(1e-5), st)

    for kw in (dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(scalars=None), dict(lr=None),
               dict(step=None), dict(n=0), dict(n=-1)):
        assert adam(**kw) == VN_EINVAL, kw
    torch.cuda.synchronize()
    assert int(step_d) == 7
    for t in (p, m, v):
        assert torch.isnan(t).all()
