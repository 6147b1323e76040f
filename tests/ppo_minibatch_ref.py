"""numpy restatement of the PPO minibatch split (include/vnav.h, vn_ppo_env_permutation and
vn_ppo_minibatch_gather; DESIGN.md "PPO minibatches"). Built on oracle.philox; shared by
test_ppo_minibatch_refs.py (CPU) and the GPU tests."""
import numpy as np

from oracle import philox

STREAM_PPO = 7
OUT_LD = 8


def keys(seed, ctr, k, E, key_bits=32):
    """uint32 [E]: the key of env e in epoch k under counter base ``ctr`` = the first word of
    Philox4x32-10 (k E + e, ctr_lo, ctr_hi, STREAM_PPO), masked to its low key_bits bits."""
    k0, k1 = philox.seed_key(seed)
    ctr = int(ctr) & 0xFFFFFFFFFFFFFFFF
    first = (int(k) * int(E) + np.arange(E, dtype=np.uint64)) & np.uint64(0xFFFFFFFF)
    x = philox.philox4x32_10(first, ctr & 0xFFFFFFFF, ctr >> 32, STREAM_PPO, k0, k1)[0]
    return (np.asarray(x, dtype=np.uint64) & np.uint64((1 << int(key_bits)) - 1)).astype(np.uint32)


def permutation(seed, ctr, k, E, key_bits=32):
    """int32 [E]: the stable argsort of the keys, ties by env index."""
    return np.argsort(keys(seed, ctr, k, E, key_bits), kind="stable").astype(np.int32)


def bounds(E, M):
    """lo_0..lo_M, lo_m = floor(m E / M): minibatch m holds perm[lo_m:lo_{m+1}]."""
    return [m * int(E) // int(M) for m in range(int(M) + 1)]


def gather(src, envs, T, E):
    """The compact [T, len(envs)] form of every buffer of ``src`` (name -> array whose leading
    T * E rows are time-major, row t E + e; "h0" / "c0": [E, 512], row e; "goal_delta": scaled by
    len(envs) / E): plain fancy indexing, bits untouched."""
    envs = np.asarray(envs, dtype=np.int64)
    rows = (np.arange(T, dtype=np.int64)[:, None] * E + envs[None, :]).reshape(-1)
    out = {}
    for name, v in src.items():
        v = np.asarray(v)
        if name in ("h0", "c0"):
            out[name] = v[envs].copy()
        elif name == "goal_delta":
            out[name] = (v.reshape(T * E)[rows] // E * len(envs)).astype(v.dtype)
        else:
            out[name] = v.reshape(T * E, -1)[rows].reshape((len(rows),) + _tail(v, T * E))
    return out


def _tail(v, n):
    """The per-row shape of an array holding n rows."""
    per = v.size // n
    return () if per == 1 else (per,)
