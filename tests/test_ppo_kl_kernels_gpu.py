"""csrc/vn_ppo_kl.hip on the device. vn_ppo_kl_gate against the fp64 restatement of
tests/ppo_kl_ref.py at one lane, the wave edge, the block edge and a second and third stride, for 1,
4 and 7 actions at logit scale 1 and 8: the KL within 1e-5 of the mean of its terms' magnitudes (the
bar tests/test_ppo_kernels_gpu.py holds ppo_stats4[0] to), equal bits over two runs, the
reference's decision at a limit below and a limit above the KL, and exactly the buffers of each
outcome; two passes count two steps, a set flag is sticky, out_old = out and one action give a KL
of exactly 0 that a limit of 0 lets pass, every refusal writes nothing. vn_adam_step_gated and
vn_rmsprop_step_gated over three steps between guard words: at flag 0 the bits of vn_adam_step_dev /
vn_rmsprop_step_dev on copies, at flag 1 nothing written, Adam's step count included."""
import ctypes

import numpy as np
import pytest
import torch

import ppo_kl_ref as kref
from test_a2c_kernels_gpu import NAN, VN_EINVAL, _l, full, host, report, same_bits
from test_a2c_kernels_gpu import dev as _dev

pytestmark = pytest.mark.gpu

CF, I64 = ctypes.c_float, ctypes.c_int64
CANARY_I, CANARY_F = 77, -3.5


def dev(a):
    return _dev(np.array(a))


def i32(values):
    return torch.tensor(values, dtype=torch.int32, device="cuda")


def f32(values):
    return torch.tensor(values, dtype=torch.float32, device="cuda")


def gate_call(o, oo, a, n, A, limit, gate, kl2):
    _lib, lib, st = _l()
    P = _lib.ptr
    return lib.vn_ppo_kl_gate(P(o), P(oo), P(a), n, A, CF(limit), P(gate), P(kl2), st)


@pytest.mark.parametrize("scale", kref.SCALES)
@pytest.mark.parametrize("A", kref.AS)
@pytest.mark.parametrize("n", kref.NS)
def test_gate_vs_fp64(n, A, scale):
    out, out_old, actions, k64, mag, limits = kref.case(n, A, scale)
    o, oo, a = dev(out), dev(out_old), dev(actions)
    seen = []
    for limit in limits:
        want_gate, want_kl = kref.gate(out, out_old, actions, A, float(limit))
        for _ in range(2):
            gate, kl2 = i32([0, 0]), f32([NAN, CANARY_F])
            assert gate_call(o, oo, a, n, A, limit, gate, kl2) == 0
            g, k = host(gate).copy(), host(kl2).copy()
            seen.append(k[0])
            err = abs(float(k[0]) - k64)
            report("kl_gate n=%d A=%d x%d limit %.3e" % (n, A, int(scale), limit), err, 1e-5 * mag)
            assert err <= 1e-5 * mag, (k[0], k64, mag)
            assert g.tolist() == want_gate, (g, want_gate, k[0], limit)
            if want_gate[0]:  # stopped: no step counted, the KL kept
                assert g.tolist() == [1, 0] and same_bits(k[1], k[0]) and want_kl[1] == k64
            else:  # passed: one step counted, the second word untouched
                assert g.tolist() == [0, 1] and same_bits(k[1], np.float32(CANARY_F))
    assert all(same_bits(x, seen[0]) for x in seen)  # the same bits on every run, whatever the limit
    if A == 1:
        assert seen[0] == 0.0


def test_two_passes_count_two_steps_and_a_set_flag_is_sticky():
    n, A = 1025, 4
    out, out_old, actions, k64, _, limits = kref.case(n, A, 1.0)
    o, oo, a = dev(out), dev(out_old), dev(actions)
    gate, kl2 = i32([0, 0]), f32([NAN, CANARY_F])
    for _ in range(2):
        assert gate_call(o, oo, a, n, A, limits[1], gate, kl2) == 0
    assert host(gate).tolist() == [0, 2] and same_bits(host(kl2)[1], np.float32(CANARY_F))
    # a stop after two allowed steps keeps their count; then the flag is sticky, whatever the limit
    assert gate_call(o, oo, a, n, A, limits[0], gate, kl2) == 0
    stopped = host(kl2).copy()
    assert host(gate).tolist() == [1, 2] and same_bits(stopped[1], stopped[0]) and stopped[0] > 0
    gate, kl2 = i32([1, CANARY_I]), f32([CANARY_F, 2 * CANARY_F])
    for limit in (limits[0], limits[1], np.float32(1e30)):
        assert gate_call(o, oo, a, n, A, limit, gate, kl2) == 0
    assert host(gate).tolist() == [1, CANARY_I]
    assert same_bits(host(kl2), np.array([CANARY_F, 2 * CANARY_F], np.float32))
    gate = i32([-5, CANARY_I])  # any non-zero word is a set flag
    assert gate_call(o, oo, a, n, A, limits[1], gate, kl2) == 0
    assert host(gate).tolist() == [-5, CANARY_I] and same_bits(host(kl2), np.array([CANARY_F, 2 * CANARY_F], np.float32))


@pytest.mark.parametrize("n", [1, 65, 2049])
def test_exact_zero_passes_a_limit_of_zero(n):
    """out_old is out: every d is exactly 0. One action: logp is exactly 0 on both sides. The check
    is strict, so a KL of 0 passes a limit of 0."""
    for A, scale, alias in ((4, 8.0, True), (7, 1.0, True), (1, 8.0, False)):
        out, out_old, actions = kref.case(n, A, scale)[:3]
        o, a = dev(out), dev(actions)
        oo = o if alias else dev(out_old)
        gate, kl2 = i32([0, 0]), f32([NAN, CANARY_F])
        assert gate_call(o, oo, a, n, A, 0.0, gate, kl2) == 0
        assert host(gate).tolist() == [0, 1]
        assert same_bits(host(kl2), np.array([0.0, CANARY_F], np.float32))


def test_gate_refusals_write_nothing():
    n, A = 65, 4
    out, out_old, actions = kref.case(n, A, 1.0)[:3]
    o, oo, a = dev(out), dev(out_old), dev(actions)
    gate, kl2 = i32([0, CANARY_I]), f32([CANARY_F, 2 * CANARY_F])
    good = dict(o=o, oo=oo, a=a, n=n, A=A, limit=0.01, gate=gate, kl2=kl2)
    for kw in (dict(o=None), dict(oo=None), dict(a=None), dict(gate=None), dict(kl2=None), dict(n=0), dict(n=-4),
               dict(A=0), dict(A=8), dict(limit=-1e-9), dict(limit=-1.0), dict(limit=NAN)):
        q = dict(good, **kw)
        assert gate_call(q["o"], q["oo"], q["a"], q["n"], q["A"], q["limit"], q["gate"], q["kl2"]) == VN_EINVAL, kw
    torch.cuda.synchronize()
    assert host(gate).tolist() == [0, CANARY_I]
    assert same_bits(host(kl2), np.array([CANARY_F, 2 * CANARY_F], np.float32))
    assert gate_call(o, oo, a, n, A, 0.0, gate, kl2) == 0  # a limit of 0 is a limit


# ---- the gated optimiser steps ---------------------------------------------------------

GUARD = 8  # guard words on either side of every buffer
ADAM = dict(scale=0.5, coef=0.75, lr=3e-4, b1=0.9, b2=0.999, eps=1e-5)
RMS = dict(scale=0.5, coef=0.75, lr=7e-4, alpha=0.99, eps=1e-5)


def guarded(values):
    """A device buffer with GUARD canary words before and after the values; (whole, inner view)."""
    whole = torch.full((values.size + 2 * GUARD,), CANARY_F, dtype=torch.float32, device="cuda")
    whole[GUARD:GUARD + values.size] = dev(values)
    return whole, whole[GUARD:GUARD + values.size]


def guards_intact(whole):
    h = host(whole)
    want = np.full(GUARD, CANARY_F, np.float32)
    return same_bits(h[:GUARD], want) and same_bits(h[-GUARD:], want)


def _step_case(n, steps=3):
    rng = np.random.RandomState([13, n])
    p0 = rng.randn(n).astype(np.float32)
    gs = [(rng.randn(n) * 0.01).astype(np.float32) for _ in range(steps)]
    return p0, gs


@pytest.mark.parametrize("n", kref.STEP_NS)
def test_adam_gated(n):
    """70001 elements: more than one block, a ragged last one. Three steps at flag 0 beside
    vn_adam_step_dev on copies, then three at flag 1 on what they left."""
    _lib, lib, st = _l()
    P = _lib.ptr
    p0, gs = _step_case(n)
    zero = np.zeros(n, np.float32)
    (pw, p), (mw, m), (vw, v) = guarded(p0), guarded(zero), guarded(zero)
    pe, me, ve = dev(p0), dev(zero), dev(zero)
    scalars, lr_d = f32([2.0, ADAM["coef"]]), f32([ADAM["lr"]])
    step_d = torch.zeros(1, dtype=torch.int64, device="cuda")
    step_e = torch.zeros(1, dtype=torch.int64, device="cuda")
    flag = i32([0, CANARY_I])  # the trainer hands the gate's own buffer: word 0 is the flag

    def gated(g):
        _lib.check(lib.vn_adam_step_gated(P(p), P(g), P(m), P(v), I64(n), CF(ADAM["scale"]), P(scalars), P(lr_d),
                                          P(step_d), CF(ADAM["b1"]), CF(ADAM["b2"]), CF(ADAM["eps"]), P(flag), st),
                   "vn_adam_step_gated")

    for it, g in enumerate(gs):
        g_d = dev(g)
        gated(g_d)
        _lib.check(lib.vn_adam_step_dev(P(pe), P(g_d), P(me), P(ve), I64(n), CF(ADAM["scale"]), P(scalars), P(lr_d),
                                        P(step_e), CF(ADAM["b1"]), CF(ADAM["b2"]), CF(ADAM["eps"]), st),
                   "vn_adam_step_dev")
        assert int(step_d) == it + 1 == int(step_e)
        for x, y in ((p, pe), (m, me), (v, ve)):
            assert same_bits(host(x), host(y)), it
    assert not same_bits(host(p), p0)
    before = [host(x).copy() for x in (pw, mw, vw)]
    flag[0] = 1
    for g in gs:
        gated(dev(g))
    torch.cuda.synchronize()
    assert int(step_d) == len(gs)
    for x, y in zip((pw, mw, vw), before):
        assert same_bits(host(x), y)
    assert all(guards_intact(w) for w in (pw, mw, vw)) and host(flag).tolist() == [1, CANARY_I]


@pytest.mark.parametrize("n", kref.STEP_NS)
def test_rmsprop_gated(n):
    _lib, lib, st = _l()
    P = _lib.ptr
    p0, gs = _step_case(n)
    zero = np.zeros(n, np.float32)
    (pw, p), (sw, s) = guarded(p0), guarded(zero)
    pe, se = dev(p0), dev(zero)
    scalars, lr_d = f32([2.0, RMS["coef"]]), f32([RMS["lr"]])
    flag = i32([0, CANARY_I])

    def gated(g):
        _lib.check(lib.vn_rmsprop_step_gated(P(p), P(g), P(s), I64(n), CF(RMS["scale"]), P(scalars), P(lr_d),
                                             CF(RMS["alpha"]), CF(RMS["eps"]), P(flag), st), "vn_rmsprop_step_gated")

    for it, g in enumerate(gs):
        g_d = dev(g)
        gated(g_d)
        _lib.check(lib.vn_rmsprop_step_dev(P(pe), P(g_d), P(se), I64(n), CF(RMS["scale"]), P(scalars), P(lr_d),
                                           CF(RMS["alpha"]), CF(RMS["eps"]), st), "vn_rmsprop_step_dev")
        assert same_bits(host(p), host(pe)) and same_bits(host(s), host(se)), it
    assert not same_bits(host(p), p0)
    before = [host(x).copy() for x in (pw, sw)]
    flag[0] = 1
    for g in gs:
        gated(dev(g))
    torch.cuda.synchronize()
    for x, y in zip((pw, sw), before):
        assert same_bits(host(x), y)
    assert guards_intact(pw) and guards_intact(sw) and host(flag).tolist() == [1, CANARY_I]


def test_gated_step_refusals_write_nothing():
    _lib, lib, st = _l()
    P = _lib.ptr
    n = 65
    p, g, m, v = full(n, NAN), full(n, NAN), full(n, NAN), full(n, NAN)
    scalars, lr_d, flag = full(2, NAN), full(1, NAN), i32([0, 0])
    step_d = torch.full((1,), 7, dtype=torch.int64, device="cuda")
    base = dict(p=p, g=g, m=m, v=v, n=n, scalars=scalars, lr=lr_d, step=step_d, flag=flag)

    def adam(**kw):
        q = dict(base, **kw)
        return lib.vn_adam_step_gated(P(q["p"]), P(q["g"]), P(q["m"]), P(q["v"]), I64(q["n"]), CF(1.0), P(q["scalars"]),
                                      P(q["lr"]), P(q["step"]), CF(0.9), CF(0.999), CF(1e-5), P(q["flag"]), st)

    def rms(**kw):
        q = dict(base, **kw)
        return lib.vn_rmsprop_step_gated(P(q["p"]), P(q["g"]), P(q["m"]), I64(q["n"]), CF(1.0), P(q["scalars"]),
                                         P(q["lr"]), CF(0.99), CF(1e-5), P(q["flag"]), st)

    for kw in (dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(scalars=None), dict(lr=None),
               dict(step=None), dict(flag=None), dict(n=0), dict(n=-1)):
        assert adam(**kw) == VN_EINVAL, kw
    for kw in (dict(p=None), dict(g=None), dict(m=None), dict(scalars=None), dict(lr=None), dict(flag=None),
               dict(n=0), dict(n=-1)):
        assert rms(**kw) == VN_EINVAL, kw
    torch.cuda.synchronize()
    assert int(step_d) == 7
    for t in (p, m, v):
        assert torch.isnan(t).all()
