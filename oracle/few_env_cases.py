"""Case tables and inputs of the few-env policy tests (TEST INFRASTRUCTURE ONLY — see
oracle/__init__.py).

tests/test_few_env_gpu.py runs these through the kernels of csrc/vn_skinny.h (n <=
SKINNY_ROWS samples: skinny_kernel for conv_merge and the heads, conv34_small_kernel, the fused
LSTM step / BPTT step), the float-frame conv1 / conv2-gradient paths and action counts other
than 4; tests/test_few_env_cases.py checks on the CPU that the tables hold what they claim
(both sides of every row-instance switch, an odd pixel count for odd n, a non-zero last LDS
chunk of conv_merge's K at 300x400, the three placed resets, float frames off the k/255
grid). numpy only: nothing here needs the GPU.

The three frame geometries are template instantiations of the kernels, so they are the
smallest shapes these kernels exist at; the batch sizes are the smallest that sit on either
side of each switch.
"""
import numpy as np

GEOMETRIES = ((84, 84), (174, 174), (300, 400))
GEO_IDS = {(84, 84): "84x84", (174, 174): "174x174", (300, 400): "300x400"}

# csrc/vn_skinny.h: M <= kSkinnyRows runs the VALU path, instantiated for MR = 4, 8, 16 rows
SKINNY_ROWS = 16
ROW_INSTANCES = (4, 8, 16)
C34_ROWS = 2       # kC34Rows: output pixels per conv34_small_kernel workgroup
SK_KB_MAX = 24     # kSkKB


def trunk_sizes(h, w):
    o1 = ((h - 7) // 4 + 1, (w - 7) // 4 + 1)
    o2 = ((o1[0] - 4) // 2 + 1, (o1[1] - 4) // 2 + 1)
    o3 = ((o2[0] - 4) // 2 + 1, (o2[1] - 4) // 2 + 1)
    return o1, o2, o3


def fcin(hw):
    """K of the conv_merge product: 32 channels x conv_base's output map."""
    o3 = trunk_sizes(*hw)[2]
    return 32 * o3[0] * o3[1]


def row_instance(n):
    """The MR a call of n rows runs at (launch_skinny), None past SKINNY_ROWS (tensor-core path)."""
    for mr in ROW_INSTANCES:
        if n <= mr:
            return mr
    return None


def skinny_kb(K, lpc):
    """launch_skinny_lpc: the B f4 registers per lane chosen for K at LPC lanes per column."""
    if K <= 4 * lpc * 4:
        return 4
    if K <= 4 * lpc * 8:
        return 8
    return 6 if lpc == 128 else SK_KB_MAX


def skinny_kc(mr, lpc, kb):
    """skinny_kc<MR, LPC, KB>: the LDS chunk length in values (A staged [MR][kc], <= 128 KiB)."""
    if mr * kb * 4 * lpc * 4 <= 128 * 1024:
        return kb * 4 * lpc
    return (128 * 1024 // (mr * 4)) // (4 * lpc) * (4 * lpc)


def conv_merge_chunks(hw, n):
    """(chunk length, full chunks, remainder) of conv_merge's K for a call of n <= 16 rows
    (N = 512 >= 256: LPC = 128)."""
    K, mr = fcin(hw), row_instance(n)
    kc = skinny_kc(mr, 128, skinny_kb(K, 128))
    return kc, K // kc, K % kc


# ---- A: trunk + heads on u8 frames: (geometry, n, num_actions) -----------------------------
TRUNK_N = {(84, 84): (1, 4, 5, 8, 9, 16, 17), (174, 174): (1, 5, 8, 9, 16, 17), (300, 400): (1, 4, 5, 9, 16, 17)}
ACTION_COUNTS = (1, 3, 7)   # besides 4, at 84x84 n = 5 and n = 17
TRUNK_CASES = []
for _hw in GEOMETRIES:
    for _n in TRUNK_N[_hw]:
        if _hw == (84, 84) and _n in (5, 17):
            TRUNK_CASES += [(_hw, _n, _a) for _a in ACTION_COUNTS]
        else:
            TRUNK_CASES.append((_hw, _n, 4))
TRUNK_IDS = ["%s-n%d-A%d" % (GEO_IDS[hw], n, a) for hw, n, a in TRUNK_CASES]

# ---- B: guard rows: (geometry, n), store capacity n + 2, act_offset 1 -----------------------
GUARD_CASES = [((84, 84), 5), ((174, 174), 5), ((174, 174), 16), ((300, 400), 5)]
GUARD_IDS = ["%s-n%d" % (GEO_IDS[hw], n) for hw, n in GUARD_CASES]
GUARD_BITS = 0x7FC5A5A5  # a quiet NaN with a payload (as int32)

# ---- C: float frames ------------------------------------------------------------------------
FLOAT_N = (3, 17)
FLOAT_CASES = [(hw, n) for hw in GEOMETRIES for n in FLOAT_N]
FLOAT_IDS = ["%s-n%d" % (GEO_IDS[hw], n) for hw, n in FLOAT_CASES]
FLOAT_U8_N = 3   # the frames_to_float(u8) check, one per geometry

# ---- D: recurrent core: (E, T, A, null_args, extra_envs) --------------------------------------
LSTM_CASES = ([(E, T, 4, False, 0) for E, T in ((1, 1), (1, 3), (4, 3), (8, 2), (9, 3), (16, 1), (17, 1), (17, 3))]
              + [(5, 3, A, False, 0) for A in ACTION_COUNTS]
              + [(4, 3, 4, True, 0), (17, 3, 4, True, 0)]
              + [(9, 3, 4, False, 4), (17, 3, 4, False, 17)])
LSTM_IDS = ["E%d-T%d-A%d%s%s" % (E, T, A, "-null" if nul else "", "-extra%d" % x if x else "")
            for E, T, A, nul, x in LSTM_CASES]
XCAT_PAD = {1: 2, 3: 0, 7: 0, 4: 3}  # zero columns between lra and h in xcat, by action count


def _rng(*key):
    return np.random.RandomState([20240607] + [int(k) for k in key])


def weight_seed(hw, n, A):
    """torch seed of a case's N(0, 0.01) weight noise (the init itself is seeded by the policy)."""
    return 1000 * hw[0] + 10 * n + A


def u8_frames(hw, n, key=0):
    """(image, goal) uint8 [n, H, W, 3]."""
    rng = _rng(1, hw[0], hw[1], n, key)
    shape = (n, hw[0], hw[1], 3)
    return rng.randint(0, 256, size=shape).astype(np.uint8), rng.randint(0, 256, size=shape).astype(np.uint8)


def float_frames(hw, n):
    """(image, goal) float32 [n, 3, H, W] uniform in [0, 1): not the k/255 grid of scaled u8
    frames, so a path that quantised its input shows."""
    rng = _rng(2, hw[0], hw[1], n)
    shape = (n, 3, hw[0], hw[1])
    return rng.random_sample(shape).astype(np.float32), rng.random_sample(shape).astype(np.float32)


def loss_inputs(n, A, key=0):
    """(actions int32 [n], returns float32 [n]) of the A2C loss."""
    rng = _rng(3, n, A, key)
    return rng.randint(0, A, size=n).astype(np.int32), rng.randn(n).astype(np.float32)


def out_cotangent(n, A):
    """dL/d(logits | value) float32 [n, A + 1] of the linear loss of the float-frame cases."""
    return _rng(4, n, A).randn(n, A + 1).astype(np.float32)


def lstm_masks(E, T):
    """float32 [T, E], placed: env 0 is reset at t = 0, env E - 1 at t = T - 1, env E // 2 at
    t = 1 where T >= 3; one env alone is reset at t = 1 only; every other entry is 1."""
    m = np.ones((T, E), dtype=np.float32)
    for t, e in lstm_resets(E, T):
        m[t, e] = 0.0
    return m


def lstm_resets(E, T):
    if E == 1:
        return [(1, 0)] if T >= 2 else []
    out = [(0, 0), (T - 1, E - 1)]
    if T >= 3:
        out.append((1, E // 2))
    return out
