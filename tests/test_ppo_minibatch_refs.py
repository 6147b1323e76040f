"""The PPO minibatch split on the CPU: the numpy restatement of tests/ppo_minibatch_ref.py on its
own (the bounds cover the envs in sizes that differ by at most one, the permutation is one and
keeps ties in env order, every env is equally likely at every position, the gather is plain
indexing), and the library declares and exports the new entry points. No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import ppo_minibatch_ref as ref
from conftest import PKG, REPO

SEED = 9 * 1000003 + 1  # vdist.rank_seed(9, 0), the GPU trainer tests' key: chosen once
NEW_SYMBOLS = ("vn_ppo_env_permutation", "vn_ppo_minibatch_gather", "vn_ppo_loss_grad_acc")


@pytest.mark.parametrize("E", [1, 5, 18, 65])
def test_bounds_cover_the_envs_evenly(E):
    for M in range(1, E + 1):
        lo = ref.bounds(E, M)
        assert len(lo) == M + 1 and lo[0] == 0 and lo[-1] == E
        sizes = np.diff(lo)
        assert (sizes >= 1).all() and sizes.max() - sizes.min() <= 1 and sizes.sum() == E
        assert sizes.max() == -(-E // M)


@pytest.mark.parametrize("E", [1, 2, 5, 64, 65, 1030])
@pytest.mark.parametrize("key_bits", [32, 3])
def test_permutation_is_a_permutation(E, key_bits):
    ctr = 2 ** 32 + 5
    for k in (0, 3):
        p = ref.permutation(SEED, ctr, k, E, key_bits)
        assert p.dtype == np.int32 and sorted(p.tolist()) == list(range(E))
        key = ref.keys(SEED, ctr, k, E, key_bits)
        assert key.dtype == np.uint32 and int(key.max()) < 2 ** key_bits
        pairs = list(zip(key[p].tolist(), p.tolist()))
        assert pairs == sorted(pairs)  # by key, ties by env index
        if key_bits == 3 and E > 8:
            assert len(set(key.tolist())) < E  # ties were forced
    if E > 1 and key_bits == 32:
        a, b = ref.permutation(SEED, ctr, 0, E), ref.permutation(SEED, ctr, 1, E)
        c, d = ref.permutation(SEED, ctr + 1, 0, E), ref.permutation(SEED + 1, ctr, 0, E)
        if E > 5:  # (at E = 2 two draws agree half the time)
            assert not np.array_equal(a, b) and not np.array_equal(a, c) and not np.array_equal(a, d)
        # the high counter word is live
        assert not np.array_equal(ref.keys(SEED, 5, 0, E), ref.keys(SEED, ctr, 0, E))


def test_every_env_is_equally_likely_at_every_position():
    """4000 counters at E = 8: each (env, position) count is Binomial(4000, 1/8), mean 500, standard
    deviation sqrt(4000 * 1/8 * 7/8) = 20.9; every one of the 64 lies within 5 of them."""
    E, n = 8, 4000
    count = np.zeros((E, E), dtype=np.int64)
    for ctr in range(n):
        p = ref.permutation(SEED, ctr * 20, 0, E)  # the counter base advances by num_steps per update
        count[p, np.arange(E)] += 1
    sd = np.sqrt(n * (1 / E) * (1 - 1 / E))
    worst = np.abs(count - n / E).max() / sd
    print("PPOMB position counts: worst %.2f standard deviations from %d" % (worst, n // E))
    assert worst <= 5.0
    assert (count.sum(axis=0) == n).all() and (count.sum(axis=1) == n).all()


def test_gather_is_plain_indexing():
    T, E, A = 3, 5, 4
    rng = np.random.RandomState(0)
    src = dict(rows_img=rng.randint(0, 99, T * E).astype(np.int32), returns=rng.randn(T * E).astype(np.float32),
               out_old=rng.randn(T * E, ref.OUT_LD).astype(np.float32), lra=rng.randn(T, E, A + 1).astype(np.float32),
               dones=rng.rand(T, E) < 0.3, h0=rng.randn(E, 512).astype(np.float32),
               goal_delta=(-E * rng.randint(0, 3, (T, E))).astype(np.int32))
    envs = [4, 0, 2]
    got = ref.gather(src, envs, T, E)
    for t in range(T):
        for j, e in enumerate(envs):
            i = t * len(envs) + j
            assert got["rows_img"][i] == src["rows_img"][t * E + e]
            assert got["returns"][i] == src["returns"][t * E + e]
            assert np.array_equal(got["out_old"][i], src["out_old"][t * E + e])
            assert np.array_equal(got["lra"][i], src["lra"][t, e])
            assert got["dones"][i] == src["dones"][t, e]
            assert got["goal_delta"][i] == src["goal_delta"][t, e] // E * len(envs)
    assert np.array_equal(got["h0"], src["h0"][envs])
    assert got["out_old"].shape == (T * 3, ref.OUT_LD) and got["lra"].shape == (T * 3, A + 1)
    assert got["dones"].shape == (T * 3,) and got["dones"].dtype == src["dones"].dtype


def test_stream_id_and_tile_are_the_librarys():
    text = open(os.path.join(PKG, "csrc", "vn_common.h")).read()
    assert re.search(r"STREAM_PPO\s*=\s*%d\b" % ref.STREAM_PPO, text)
    ids = [int(v) for v in re.findall(r"STREAM_[A-Z]+\s*=\s*(\d+)", text)]
    assert len(ids) == len(set(ids)) == ref.STREAM_PPO + 1
    from vnav import _lib
    header = open(os.path.join(REPO, "include", "vnav.h")).read()
    assert re.search(r"#define\s+VN_PPO_PERM_TILE\s+%d\b" % _lib.PPO_PERM_TILE, header)


def test_new_entry_points_are_declared_and_exported(built_lib):
    import torch  # noqa: F401  (shares torch's HIP runtime, as the product does)
    from test_lib_abi import declared_symbols
    from vnav import _lib
    syms = declared_symbols()
    lib = ctypes.CDLL(built_lib)
    for s in NEW_SYMBOLS:
        assert s in syms and s in _lib.SIGNATURES and hasattr(lib, s), s
    # the accumulating entry takes the clearing entry's arguments
    assert _lib.SIGNATURES["vn_ppo_loss_grad_acc"] == _lib.SIGNATURES["vn_ppo_loss_grad"]
    fields = [f for f, _ in _lib.PpoRollout._fields_]
    body = re.search(r"typedef struct vn_ppo_rollout \{(.*?)\} vn_ppo_rollout;", open(
        os.path.join(REPO, "include", "vnav.h")).read(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\*\s*([a-z0-9_]+)\s*;", body) == fields
    # the refusals need no device: nothing is launched
    load = _lib.load()
    assert load.vn_ppo_env_permutation(1, None, 0, 4, 32, None, None) != 0
    assert "vn_ppo_env_permutation" in _lib.last_error()
    assert load.vn_ppo_minibatch_gather(None, None, None, 1, 1, 1, 4, None) != 0
    assert "vn_ppo_minibatch_gather" in _lib.last_error()
