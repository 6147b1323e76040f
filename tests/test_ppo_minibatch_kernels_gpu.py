"""csrc/vn_ppo_minibatch.hip and vn_ppo_loss_grad_acc against tests/ppo_minibatch_ref.py:
vn_ppo_env_permutation equals numpy's stable argsort of the reference keys exactly, from one lane
across a wave, a workgroup and the counting kernel's LDS tile (1024 keys) to 32768 envs, in two
epochs, under a counter base whose high word is live, with whole keys and with 3-bit keys that
force ties; vn_ppo_minibatch_gather equals fancy indexing bitwise on every minibatch of four
splits, row widths 5 (A = 4) and 8 (A = 7) included, leaves everything past T Eb untouched and takes
NULL LSTM buffers; the accumulating loss-gradient entry adds where the existing one clears."""
import ctypes

import numpy as np
import pytest
import torch

import ppo_minibatch_ref as ref
import ppo_ref

pytestmark = pytest.mark.gpu

SEED = 9 * 1000003 + 1
CTR = 2 ** 32 + 5  # the high counter word is live (oracle/a2c_cases.py does the same)
TILE = 1024
CF = ctypes.c_float


def _l():
    from vnav import _lib
    return _lib, _lib.load(), _lib.stream_ptr(torch.device("cuda", 0))


def dev(a):
    return torch.as_tensor(np.array(a)).cuda()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8)


@pytest.mark.parametrize("E", [1, 2, 5, 63, 64, 65, 257, TILE - 1, TILE, TILE + 1, 1030, 4099, 32768])
def test_permutation_is_the_stable_argsort(E):
    _lib, lib, st = _l()
    assert _lib.PPO_PERM_TILE == TILE
    ctr = dev(np.array([CTR], dtype=np.int64))
    for k in (0, 3):
        for key_bits in (32, 3):
            perm = torch.full((E + 8,), -7, dtype=torch.int32, device="cuda")
            _lib.check(lib.vn_ppo_env_permutation(SEED, _lib.ptr(ctr), k, E, key_bits, _lib.ptr(perm), st),
                       "vn_ppo_env_permutation")
            got = perm.cpu().numpy()
            want = ref.permutation(SEED, CTR, k, E, key_bits)
            assert np.array_equal(got[:E], want), (E, k, key_bits)
            assert (got[E:] == -7).all()
    # the counter is read on the device: another value in the same buffer, another permutation
    if E >= 63:
        ctr.fill_(7)
        perm = torch.zeros(E, dtype=torch.int32, device="cuda")
        _lib.check(lib.vn_ppo_env_permutation(SEED, _lib.ptr(ctr), 0, E, 32, _lib.ptr(perm), st), "perm")
        assert np.array_equal(perm.cpu().numpy(), ref.permutation(SEED, 7, 0, E))
        assert not np.array_equal(perm.cpu().numpy(), ref.permutation(SEED, CTR, 0, E))


def test_permutation_refusals_write_nothing():
    _lib, lib, st = _l()
    ctr = dev(np.array([CTR], dtype=np.int64))
    perm = torch.full((8,), -7, dtype=torch.int32, device="cuda")
    P = _lib.ptr
    for args in ((None, 0, 8, 32, P(perm)), (P(ctr), 0, 8, 32, None), (P(ctr), -1, 8, 32, P(perm)),
                 (P(ctr), 0, 0, 32, P(perm)), (P(ctr), 0, 8, 0, P(perm)), (P(ctr), 0, 8, 33, P(perm)),
                 (P(ctr), 2 ** 29, 8, 32, P(perm))):
        assert lib.vn_ppo_env_permutation(SEED, args[0], args[1], args[2], args[3], args[4], st) != 0
    torch.cuda.synchronize()
    assert (perm.cpu().numpy() == -7).all()


def _rollout(T, E, A, seed):
    rng = np.random.RandomState(seed)
    return dict(rows_img=rng.randint(0, 1 << 20, T * E).astype(np.int32),
                rows_goal=rng.randint(0, 1 << 20, T * E).astype(np.int32),
                actions=rng.randint(0, A, T * E).astype(np.int32), returns=rng.randn(T * E).astype(np.float32),
                out_old=rng.randn(T * E, ref.OUT_LD).astype(np.float32), dones=rng.rand(T * E) < 0.3,
                masks=(rng.rand(T * E) < 0.7).astype(np.float32), lra=rng.randn(T * E, A + 1).astype(np.float32),
                h0=rng.randn(E, 512).astype(np.float32), c0=rng.randn(E, 512).astype(np.float32),
                goal_delta=(-E * rng.randint(0, T, T * E)).astype(np.int32))


LSTM = ("masks", "lra", "h0", "c0")
SENTINEL = 0x5A


@pytest.mark.parametrize("E,M,T,A", [(5, 2, 6, 4), (18, 4, 3, 7), (65, 3, 3, 4), (1030, 4, 2, 4)])
@pytest.mark.parametrize("lstm", [True, False])
def test_gather_is_fancy_indexing_bitwise(E, M, T, A, lstm):
    _lib, lib, st = _l()
    src = _rollout(T, E, A, seed=E + M)
    if not lstm:
        src = {k: v for k, v in src.items() if k not in LSTM and k != "goal_delta"}
    src_d = {k: dev(v) for k, v in src.items()}
    perm = ref.permutation(SEED, CTR, 1, E)
    perm_d = dev(perm)
    lo = ref.bounds(E, M)
    cap_e = max(np.diff(lo))
    # destinations sized for the largest minibatch, every byte a sentinel
    dst_d = {}
    for k, v in src.items():
        rows = cap_e if k in ("h0", "c0") else T * cap_e
        dst_d[k] = torch.empty((rows,) + v.shape[1:], dtype=src_d[k].dtype, device="cuda")
    s = _lib.PpoRollout(**{k: v.data_ptr() for k, v in src_d.items()})
    d = _lib.PpoRollout(**{k: v.data_ptr() for k, v in dst_d.items()})
    for m in range(M):
        eb = lo[m + 1] - lo[m]
        for v in dst_d.values():
            v.view(torch.uint8).fill_(SENTINEL)
        _lib.check(lib.vn_ppo_minibatch_gather(ctypes.byref(s), ctypes.byref(d), _lib.ptr(perm_d[lo[m]:]), eb, T, E, A,
                                               st), "vn_ppo_minibatch_gather")
        want = ref.gather(src, perm[lo[m]:lo[m + 1]], T, E)
        for k, w in want.items():
            got = dst_d[k].cpu().numpy()
            n = eb if k in ("h0", "c0") else T * eb
            assert np.array_equal(bits(got[:n]), bits(w.reshape(got[:n].shape))), (k, m)
            assert (bits(got[n:]) == SENTINEL).all(), (k, m)
    for k, v in src.items():  # the source is read only
        assert np.array_equal(bits(src_d[k].cpu().numpy()), bits(v)), k


def test_gather_refusals_and_bad_env_indices():
    _lib, lib, st = _l()
    T, E, A = 2, 5, 4
    src = _rollout(T, E, A, seed=1)
    src_d = {k: dev(v) for k, v in src.items()}
    dst_d = {k: torch.full_like(v, 0).view(torch.uint8).fill_(SENTINEL).view(v.dtype).view(v.shape)
             for k, v in src_d.items()}
    envs = dev(np.array([3, -1, 7, 1, 5], dtype=np.int32))
    ptrs = lambda t, drop=(): _lib.PpoRollout(**{k: v.data_ptr() for k, v in t.items() if k not in drop})  # noqa: E731
    s, d, P = ptrs(src_d), ptrs(dst_d), _lib.ptr
    g = lambda a, b, e, n, t=T: lib.vn_ppo_minibatch_gather(a, b, e, n, t, E, A, st)  # noqa: E731
    by = ctypes.byref
    assert g(None, by(d), P(envs), 2) != 0 and g(by(s), None, P(envs), 2) != 0 and g(by(s), by(d), None, 2) != 0
    assert g(by(s), by(d), P(envs), 0) != 0 and g(by(s), by(d), P(envs), E + 1) != 0
    assert g(by(s), by(d), P(envs), 2, 0) != 0
    assert g(by(s), by(ptrs(dst_d, ("returns",))), P(envs), 2) != 0  # a missing buffer
    assert g(by(s), by(ptrs(dst_d, ("lra",))), P(envs), 2) != 0  # some of the LSTM buffers only
    assert g(by(ptrs(src_d, LSTM)), by(d), P(envs), 2) != 0  # a destination without its source
    assert g(by(ptrs(src_d, ("goal_delta",))), by(d), P(envs), 2) != 0
    assert lib.vn_ppo_minibatch_gather(by(s), by(d), P(envs), 2, T, E, 8, st) != 0
    torch.cuda.synchronize()
    for k, v in dst_d.items():
        assert (bits(v.cpu().numpy()) == SENTINEL).all(), k
    # an env index outside [0, E) reads and writes nothing; its neighbours are gathered
    _lib.check(g(by(s), by(d), P(envs), 5), "vn_ppo_minibatch_gather")
    got = dst_d["returns"].cpu().numpy()
    ok = [0, 3]  # envs 3 and 1
    for t in range(T):
        for j in range(5):
            i = t * 5 + j
            if j in ok:
                assert got[i] == src["returns"][t * E + [3, -1, 7, 1, 5][j]]
            else:
                assert (bits(got[i:i + 1]) == SENTINEL).all()


def test_loss_grad_acc_adds_where_loss_grad_clears():
    _lib, lib, st = _l()
    P = _lib.ptr
    A = 4
    out, out_old, actions, returns, stats2, r = ppo_ref.case(257, A, 1.0)
    n, cut = out.shape[0], 100
    o, oo, a, R, s2 = dev(out), dev(out_old), dev(actions), dev(returns), dev(stats2)

    def call(fn, lo, hi, dout, stats, pstats):
        _lib.check(fn(P(o[lo:]), P(oo[lo:]), P(a[lo:]), P(R[lo:]), P(s2), hi - lo, A, CF(ppo_ref.CLIP),
                      CF(ppo_ref.VALUE_CLIP), CF(ppo_ref.VC), CF(ppo_ref.EC), P(dout), P(stats), P(pstats), st), "call")

    parts = []
    for lo, hi in ((0, cut), (cut, n)):
        dout = torch.zeros((hi - lo, 8), device="cuda")
        stats, pstats = torch.full((4,), 3.0, device="cuda"), torch.full((4,), 3.0, device="cuda")
        call(lib.vn_ppo_loss_grad, lo, hi, dout, stats, pstats)  # clears the 3.0
        parts.append((dout.clone(), stats.double().cpu().numpy(), pstats.double().cpu().numpy()))
    stats, pstats = torch.full((4,), 1.0, device="cuda"), torch.full((4,), 2.0, device="cuda")
    for (lo, hi), (dout_want, _, _) in zip(((0, cut), (cut, n)), parts):
        dout = torch.zeros((hi - lo, 8), device="cuda")
        call(lib.vn_ppo_loss_grad_acc, lo, hi, dout, stats, pstats)
        assert torch.equal(dout.view(torch.int32), dout_want.view(torch.int32))  # the mean over its own samples
    mags = np.abs(r["terms"]).sum(axis=1)
    got4, gotp = stats.double().cpu().numpy(), pstats.double().cpu().numpy()
    assert (np.abs(got4 - 1.0 - parts[0][1] - parts[1][1]) <= 1e-5 * (mags[:4] + 1.0)).all()
    assert (np.abs(gotp - 2.0 - parts[0][2] - parts[1][2]) <= 1e-5 * (mags[4:] + 2.0)).all()
    # and against fp64 over all n samples: the sums do not depend on the split
    assert (np.abs(got4 - 1.0 - r["stats4"]) <= 1e-5 * (mags[:4] + 1.0)).all()
    assert (np.abs(gotp - 2.0 - r["ppo_stats4"]) <= 1e-5 * (mags[4:] + 2.0)).all()
