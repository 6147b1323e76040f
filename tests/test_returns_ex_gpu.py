"""vn_a2c_returns_ex (csrc/vn_shaping.hip) on the GPU: bit for bit vn_a2c_returns where nothing is
shaped and lambda = 1 (rewards of -0.0 included), both recurrences against the float64 restatement
of tests/shaping_ref.py within 2 k T 2^-24 M (k = the fp32 roundings per step the kernel's comment
states, M = the largest magnitude among r', V, G and R of the float64 run; the form of
test_returns_vs_fp64's 4 T 2^-24 max|R|, derived and not tuned), the weight's anneal read from the
device, the integer statistics exactly, and every refused call writing nothing. The shapes are
test_returns_vs_fp64's: one lane, a second workgroup, several."""
import ctypes

import numpy as np
import pytest
import torch

import shaping_ref as sr

pytestmark = pytest.mark.gpu

NAN = float("nan")
EPS24 = 2.0 ** -24
VN_EINVAL = -1
CF, I64 = ctypes.c_float, ctypes.c_int64
SHAPES = [(1, 1), (20, 257), (40, 1000)]
GAMMA, GAMMA_PHI, W = 0.99, 0.99, 0.5


def _l():
    from vnav import _lib
    return _lib, _lib.load(), _lib.stream_ptr(torch.device("cuda", 0))


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def case(T, E, A):
    rng = np.random.RandomState([21, T, E, A])
    rewards = rng.randn(T, E).astype(np.float32)
    rewards[rng.rand(T, E) < 0.25] = np.float32(-0.0)
    rewards[rng.rand(T, E) < 0.1] = np.float32(0.0)
    dones = (rng.rand(T, E) < 0.15).astype(np.uint8)
    boot = np.full((E, 8), np.nan, dtype=np.float32)
    boot[:, A] = rng.randn(E).astype(np.float32)
    out = np.full((T * E, 8), np.nan, dtype=np.float32)
    out[:, A] = rng.randn(T * E).astype(np.float32)
    dist = rng.randint(-1, 13, size=(T, 2, E)).astype(np.int32)  # -1: the goal is unreachable
    return rewards, dones, boot, out, dist


def call(c, T, E, A, lam, w, dist=True, out=True, steps=None, anneal=0, gamma_phi=GAMMA_PHI, returns=None,
         stats=None, rewards=True, expect=0):
    """One vn_a2c_returns_ex on the case `c`; returns (returns [T, E] host, stats3 host)."""
    _lib, lib, st = _l()
    P = _lib.ptr
    rw, dn, bt, ot, ds = (dev(x) for x in c)
    R = torch.full((T * E,), NAN, dtype=torch.float32, device="cuda") if returns is None else returns
    S = torch.full((3,), -7, dtype=torch.int64, device="cuda") if stats is None else stats
    sd = None if steps is None else dev(np.array([steps], dtype=np.int64))
    rc = lib.vn_a2c_returns_ex(P(rw) if rewards else None, P(dn), P(bt), P(ot) if out else None,
                               P(ds) if dist else None, T, E, A, CF(GAMMA), CF(lam), CF(w), CF(gamma_phi),
                               P(sd), I64(anneal), P(R), P(S), st)
    torch.cuda.synchronize()
    assert rc == expect, (rc, _lib.last_error())
    R = R.cpu().numpy()
    return (R.reshape(T, E) if expect == 0 else R), S.cpu().numpy()


def plain(c, T, E, A):
    _lib, lib, st = _l()
    P = _lib.ptr
    rw, dn, bt = dev(c[0]), dev(c[1]), dev(c[2])
    R = torch.full((T * E,), NAN, dtype=torch.float32, device="cuda")
    _lib.check(lib.vn_a2c_returns(P(rw), P(dn), P(bt), T, E, A, CF(GAMMA), P(R), st), "returns")
    return R.cpu().numpy().reshape(T, E)


@pytest.mark.parametrize("A", [1, 4, 7])
@pytest.mark.parametrize("T,E", SHAPES)
def test_unshaped_n_step_is_vn_a2c_returns_by_bits(T, E, A):
    c = case(T, E, A)
    assert (np.signbit(c[0]) & (c[0] == 0)).any() or T * E == 1
    want = plain(c, T, E, A)
    for kw in (dict(dist=False, w=W), dict(dist=True, w=0.0), dict(dist=False, w=0.0, out=False),
               dict(dist=True, w=W, steps=10, anneal=10)):  # annealed to exactly 0
        got, stats = call(c, T, E, A, 1.0, **kw)
        assert got.view(np.uint32).tobytes() == want.view(np.uint32).tobytes(), kw
        if kw["dist"]:
            assert list(stats) == list(sr.shaping_stats(c[4]))
        else:
            assert list(stats) == [0, 0, 0]


@pytest.mark.parametrize("lam", [1.0, 0.95, 0.0])
@pytest.mark.parametrize("A", [1, 4, 7])
@pytest.mark.parametrize("T,E", SHAPES)
def test_shaped_returns_vs_fp64(T, E, A, lam):
    c = case(T, E, A)
    got, stats = call(c, T, E, A, lam, W)
    ref, M = sr.returns_ex64(c[0], c[1], c[2], c[3], c[4], A, GAMMA, lam, w=W, gamma_phi=GAMMA_PHI)
    k = sr.K_NSTEP_SHAPED if lam == 1.0 else sr.K_GAE_SHAPED
    bound = 2 * k * T * EPS24 * M
    assert np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - ref).max()
    print("SHAPEERR T=%d E=%d A=%d lambda=%g worst %.3e bound %.3e" % (T, E, A, lam, err, bound))
    assert err <= bound
    assert list(stats) == list(sr.shaping_stats(c[4]))
    if T * E > 1:  # the shaping term is really in there
        base, _ = sr.returns_ex64(c[0], c[1], c[2], c[3], None, A, GAMMA, lam)
        assert np.abs(ref - base).max() > 100 * bound


@pytest.mark.parametrize("lam", [0.95, 0.0])
def test_unshaped_gae_vs_fp64(lam):
    T, E, A = 20, 257, 4
    c = case(T, E, A)
    for kw in (dict(dist=False, w=W), dict(dist=True, w=0.0)):
        got, _ = call(c, T, E, A, lam, **kw)
        ref, M = sr.returns_ex64(c[0], c[1], c[2], c[3], None, A, GAMMA, lam)
        assert np.abs(got.astype(np.float64) - ref).max() <= 2 * sr.K_GAE * T * EPS24 * M


def test_n_step_form_matches_the_float32_restatement():
    """The lambda = 1 form in the kernel's stated order, operation for operation."""
    T, E, A = 20, 257, 4
    c = case(T, E, A)
    got, _ = call(c, T, E, A, 1.0, W)
    want = sr.returns_ex32(c[0], c[1], c[2], c[4], A, GAMMA, w=W, gamma_phi=GAMMA_PHI)
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("steps", [0, 2500, 10000, 25000])
def test_anneal_is_read_on_the_device(steps):
    """Before, inside, at the end of and past the horizon; the weight the expert term's rule gives."""
    T, E, A, horizon = 20, 257, 4, 10000
    c = case(T, E, A)
    w = sr.anneal_weight(W, steps, horizon)
    assert (w == 0) == (steps >= horizon)
    for lam, k in ((1.0, sr.K_NSTEP_SHAPED), (0.95, sr.K_GAE_SHAPED)):
        got, _ = call(c, T, E, A, lam, W, steps=steps, anneal=horizon)
        ref, M = sr.returns_ex64(c[0], c[1], c[2], c[3], c[4], A, GAMMA, lam, w=w, gamma_phi=GAMMA_PHI)
        assert np.abs(got.astype(np.float64) - ref).max() <= 2 * k * T * EPS24 * M
    if 0 < steps < horizon:  # not the constant weight's result
        full, _ = sr.returns_ex64(c[0], c[1], c[2], c[3], c[4], A, GAMMA, 1.0, w=W, gamma_phi=GAMMA_PHI)
        got, _ = call(c, T, E, A, 1.0, W, steps=steps, anneal=horizon)
        assert np.abs(got - full).max() > 0.1


def test_stats_are_exact_integers():
    """Sums far past 2^24 stay exact: int64 atomics."""
    T, E, A = 40, 1000, 4
    c = list(case(T, E, A))
    c[4] = np.random.RandomState(5).randint(-1, 16384, size=(T, 2, E)).astype(np.int32)
    _, stats = call(c, T, E, A, 1.0, 0.0)
    want = sr.shaping_stats(c[4])
    assert want[0] > 2 ** 27 and want[2] > 0
    assert stats.dtype == np.int64 and list(stats) == list(want)


def test_refusals_write_nothing():
    T, E, A = 20, 257, 4
    c = case(T, E, A)

    def refused(**kw):
        args = dict(T=T, E=E, A=A, lam=1.0, w=W)
        args.update(kw)
        R = torch.full((T * E,), NAN, dtype=torch.float32, device="cuda")
        S = torch.full((3,), -7, dtype=torch.int64, device="cuda")
        got, stats = call(c, args.pop("T"), args.pop("E"), args.pop("A"), args.pop("lam"), args.pop("w"),
                          returns=R, stats=S, expect=VN_EINVAL, **args)
        assert np.isnan(R.cpu().numpy()).all() and (S.cpu().numpy() == -7).all(), kw

    refused(rewards=False)
    refused(T=0)
    refused(E=0)
    refused(T=-1)
    refused(A=0)
    refused(A=8)
    refused(lam=-0.01)
    refused(lam=1.01)
    refused(lam=NAN)
    refused(lam=0.95, out=False)  # the values are read when lambda != 1
    refused(anneal=100)           # anneal_steps > 0 without steps_dev
    _lib, lib, st = _l()
    P = _lib.ptr
    rw, dn, bt, ot, ds = (dev(x) for x in c)
    R = torch.full((T * E,), NAN, dtype=torch.float32, device="cuda")
    S = torch.full((3,), -7, dtype=torch.int64, device="cuda")
    for a in ((P(rw), None, P(bt), P(R), P(S)), (P(rw), P(dn), None, P(R), P(S)), (P(rw), P(dn), P(bt), None, P(S)),
              (P(rw), P(dn), P(bt), P(R), None)):
        rc = lib.vn_a2c_returns_ex(a[0], a[1], a[2], P(ot), P(ds), T, E, A, CF(GAMMA), CF(1.0), CF(W), CF(1.0), None,
                                   I64(0), a[3], a[4], st)
        assert rc == VN_EINVAL
    torch.cuda.synchronize()
    assert np.isnan(R.cpu().numpy()).all() and (S.cpu().numpy() == -7).all()
