"""Deterministic inputs of the A2C step tests (TEST INFRASTRUCTURE ONLY — see oracle/__init__.py).

tests/test_a2c_kernels_gpu.py feeds these to the kernels; tests/test_a2c_refs.py checks on
the CPU that the categorical draws they lead to stay clear of the CDF boundaries (a draw
within DRAW_MARGIN of a boundary may legitimately fall on either side in fp32 and is left
out of the exact comparison; the seeds below keep that share under MAX_EXCLUDED_SHARE).
numpy only: nothing here needs the GPU.
"""
import numpy as np

DRAW_MARGIN = 1e-5           # fp32 CDF error is a few 1e-7 per term: more than ten times that
MAX_EXCLUDED_SHARE = 1e-3    # expected share 2e-5 * (A - 1) <= 1.2e-4

COUNTER_BASE = 2 ** 32 + 5   # device counter base: the high Philox counter word is non-zero

# vn_step_a2c against the references: (E, A) x STEP_K steps, counter = COUNTER_BASE + t
STEP_SEED = 0x5EED0A2C00000007  # policy sampling key (both key words non-zero)
STEP_ENV_SEED = 4711            # the env's own reset streams
STEP_K = 30
STEP_MAX_EPISODE_STEPS = 7
STEP_CASES = [(5, 4), (301, 4), (2500, 4), (301, 1), (301, 3), (301, 7)]
STEP_REWARDS = (1.0, -0.0625, -0.25)  # goal, step, collision: dyadic, every fp32 sum is exact

# the in-step heads (MODE_STEP_HEADS): E envs, one step, A = 4
HEADS_SEED = 0xA2C0000000000011
HEADS_CASES = [1, 5, 16]
HEADS_A = 4
HEADS_CPU_MARGIN = 1e-4  # the CPU check sees fp64 logits, the GPU draw fp32 ones: 10x DRAW_MARGIN


def step_policy_out(E, A, t):
    """policy_out [E][8] of step t: logits N(0,1) * 3 in columns < A, a value in column A,
    NaN in the columns > A (never read)."""
    rng = np.random.RandomState([1234, E, A, t])
    out = np.full((E, 8), np.nan, dtype=np.float32)
    out[:, :A] = (rng.randn(E, A) * 3.0).astype(np.float32)
    out[:, A] = rng.randn(E).astype(np.float32)
    return out


def heads_inputs(E, A=HEADS_A):
    """(W [A+1][512], b [A+1], h [E][512]) float32: the policy heads' parameters and the
    LSTM outputs they read (h in (-1, 1) as an LSTM emits)."""
    rng = np.random.RandomState([4321, E, A])
    w = (rng.uniform(-1.0, 1.0, size=(A + 1, 512)) * 0.25).astype(np.float32)
    b = (rng.randn(A + 1) * 0.5).astype(np.float32)
    h = rng.uniform(-1.0, 1.0, size=(E, 512)).astype(np.float32)
    return w, b, h
