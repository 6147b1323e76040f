"""Case tables of the UNREAL head tests and the launch rules they rest on (TEST
INFRASTRUCTURE ONLY — see oracle/__init__.py).

pc_forward_impl / pc_backward_impl / rp_forward_impl / rp_backward_impl (csrc/vn_policy.hip)
choose their kernels from the row count alone: splitk_count (split below 128 tiles, about 512
workgroups, chunks of >= 2 K tiles, the slabs within sk_cap) and the two lines after it, the
slab count of launch_wgrad / launch_wgrad6, the lanes per output G of launch_splitk_epilogue /
launch_wgrad_reduce, and colsum's block count. This module restates those rules with the
constants as they stand in the source and gives, per (arch, n) or (geometry, R), the regime of
each product; tests/test_unreal_head_cases.py checks on the CPU that the tables below hold a
case on each side of every switch, tests/test_unreal_head_regimes_gpu.py runs them against
float64. numpy only: nothing here needs the GPU.
"""
import numpy as np

from .few_env_cases import GEO_IDS, fcin

# ---- constants of csrc/vn_policy.hip / vn_unreal.h -----------------------------------------
SK_TILES = 128          # splitk_count: no split from this many tiles on
SK_WORKGROUPS = 512     # ... the workgroup count a split aims at
BK = 32
SK_CAP = 4 << 20        # kSplitKFloats: the policy's split-K scratch, in floats
SLAB = 24 << 20         # slab_floats: the weight-gradient slabs of a workspace
WGRAD_WORKGROUPS = 2048
WGRAD_ROWS = 256        # reduction rows per slab
REDUCE_FLAT = 65536     # M * N from which the reduces run one thread per output
COLSUM_BLOCKS = 512     # kColsumBlocks
PC_MAP, PC_A1, PC_P, PC_C1, PC_C2 = 9, 20, 42, 64, 8
PC_BASE = PC_MAP * PC_MAP * 32
PC_IMG = 2              # images per work item of the parity-class kernel on the 9x9 map


def _cdiv(a, b):
    return (a + b - 1) // b


def splitk_chunk(M, N, K, BM, BN):
    """(slabs, kchunk) of a launch_gemm_x6_sk / launch_gemm_sk product (1 slab = the unsplit kernel
    with its own epilogue, kchunk = K): splitk_count, then kchunk and the recomputed count."""
    tiles = _cdiv(M, BM) * _cdiv(N, BN)
    if tiles >= SK_TILES or K < 4 * BK:
        return 1, K
    splits = min(_cdiv(SK_WORKGROUPS, tiles), K // (2 * BK))
    while splits > 1 and splits * M * N > SK_CAP:
        splits -= 1
    splits = max(splits, 1)
    if splits <= 1:
        return 1, K
    kchunk = _cdiv(_cdiv(K, splits), BK) * BK
    return _cdiv(K, kchunk), kchunk


def splitk(M, N, K, BM, BN):
    """Slabs of a launch_gemm_x6_sk / launch_gemm_sk product (see splitk_chunk)."""
    return splitk_chunk(M, N, K, BM, BN)[0]


def wgrad_chunk(M, KP, P, BM, BN, bias):
    """(slabs, kchunk) of launch_wgrad / launch_wgrad6 over P reduction rows (1 slab = the direct
    EpiWgrad epilogue, else EpiSlab + launch_wgrad_reduce)."""
    N = KP + (1 if bias else 0)
    tiles = _cdiv(M, BM) * _cdiv(N, BN)
    splits = max(1, min(_cdiv(WGRAD_WORKGROUPS, tiles), _cdiv(P, WGRAD_ROWS)))
    while splits * M * N > SLAB and splits > 1:
        splits //= 2
    kchunk = _cdiv(_cdiv(P, splits), BK) * BK
    return _cdiv(P, kchunk), kchunk


def wgrad_slabs(M, KP, P, BM, BN, bias):
    """Slabs of launch_wgrad / launch_wgrad6 over P reduction rows (see wgrad_chunk)."""
    return wgrad_chunk(M, KP, P, BM, BN, bias)[0]


def reduce_lanes(M, N, splits):
    """G of launch_splitk_epilogue / launch_wgrad_reduce: lanes per output (about 8 slabs each)."""
    G = 1
    if M * N < REDUCE_FLAT:
        while G < 64 and G * 8 < splits:
            G *= 2
    return G


def colsum_blocks(rows, cols):
    return max(1, min(COLSUM_BLOCKS, _cdiv(rows, 256 // cols)))


def pc_regime(arch, n):
    """The regime of every product of pixel control at n rows ("goal": BigGoalHouseModel's two
    deconv layers, "bighouse": BigHouseModel's one)."""
    P0 = n * PC_MAP * PC_MAP
    r = {"fwd_splits": splitk(n, PC_BASE, 512, 64, 64),                    # pc_base forward
         "dh_splits": splitk(n, 512, PC_BASE, 64, 64),                     # dh = dpcb x W (EpiAcc)
         "pcw_slabs": wgrad_slabs(PC_BASE, 512, n, 128, 128, True)}        # pc_base dW | db
    if arch == "bighouse":  # 32 -> 8 channels: the generic per-class products, no parity-class kernel
        K1, side = 16 * PC_C2, PC_A1
        r["items"], r["half_item"] = 0, False
        r["b1_blocks"] = colsum_blocks(n * side * side, PC_C2)
    else:
        K1, side = 16 * PC_C1, PC_P
        P1 = n * PC_A1 * PC_A1
        # the first deconv (32 -> 64) on the persistent parity-class kernel: work items of IMG images
        r["items"], r["half_item"] = _cdiv(n, PC_IMG), n % PC_IMG == 1
        r["w2_slabs"] = wgrad_slabs(PC_C1, 16 * PC_C2, P1, 64, 128, False)
        r["b2_blocks"] = colsum_blocks(n * side * side, PC_C2)
        r["b1_blocks"] = colsum_blocks(P1, PC_C1)
    r["w1_slabs"] = wgrad_slabs(32, K1, P0, 32, 128, False)
    r["dpcb_splits"] = splitk(P0, 32, K1, 128, 32)
    r["dpcb_G"] = reduce_lanes(P0, 32, r["dpcb_splits"]) if r["dpcb_splits"] > 1 else 0
    r["pcw_G"] = reduce_lanes(PC_BASE, 513, r["pcw_slabs"]) if r["pcw_slabs"] > 1 else 0
    return r


def rp_k(arch, hw):
    return 3 * (32 * 7 * 7 if arch == "bighouse" else fcin(hw))


def rp_regime(arch, hw, R):
    K = rp_k(arch, hw)
    s = splitk(R, 3, K, 64, 16)
    w = wgrad_slabs(3, K, R, 32, 64, True)
    return {"K": K, "row_tiles": _cdiv(R, 64), "fwd_splits": s, "fwd_G": reduce_lanes(R, 3, s) if s > 1 else 0,
            "w_slabs": w, "w_G": reduce_lanes(3, K + 1, w) if w > 1 else 0}


# ---- pixel control, BigGoalHouseModel heads (frame geometry plays no part: 174x174), A = 4 ----
PC_N = (1, 3, 4, 84, 192, 193, 200, 201, 256, 257, 336, 960, 961)
# accumulate: 0 at even positions, 1 at odd — but both values on each side of the dh switch
PC_CASES = [("goal", n, 4, i % 2) for i, n in enumerate(PC_N)] + [("goal", 960, 4, 0), ("goal", 961, 4, 1)]
# other action counts: the combine / dq / block-diagonal mask kernels and the head layout
PC_A_CASES = [("goal", n, A, i % 2) for n in (5, 201) for i, A in enumerate((1, 2, 7))]
# the trainer's calling form (q = NULL forward, dq = NULL backward on dL/dp2 written into p2)
PC_TRAINER_N = (5, 336)
# BigHouseModel heads (84x84 frames), a1 = NULL
BH_CASES = ([("bighouse", n, 4, i % 2) for i, n in enumerate((1, 3, 4, 200, 201, 257))]
            + [("bighouse", 5, 1, 0), ("bighouse", 5, 7, 1)])
PC_DETERMINISM_N = (4, 336)


def pc_id(c):
    return "%s-n%d-A%d-acc%d" % c


# ---- reward prediction: (arch, geometry, R) ---------------------------------------------------
RP_R = (1, 64, 65, 72, 256, 257, 288)
RP_CASES = ([("goal", hw, R) for hw in ((174, 174), (300, 400)) for R in RP_R]
            + [("goal", (84, 84), R) for R in (1, 65, 257)] + [("bighouse", (84, 84), R) for R in (1, 65, 257)])
RP_NULL_DX_R = 65
RP_DETERMINISM_R = 288


def rp_id(c):
    return "%s-%s-R%d" % (c[0], GEO_IDS[c[1]], c[2])


def regime_table():
    """The regimes of every case, as text rows (DESIGN.md holds a copy)."""
    rows = []
    for arch, n, A, acc in PC_CASES + PC_A_CASES + BH_CASES:
        r = pc_regime(arch, n)
        rows.append("pc %-8s n=%-4d A=%d acc=%d  fwd %d  W2 %s  W1 %d  dpcb %d (G %d)  pc_base dW %d (G %d)  dh %d  "
                    "items %d%s" % (arch, n, A, acc, r["fwd_splits"], r.get("w2_slabs", "-"), r["w1_slabs"],
                                    r["dpcb_splits"], r["dpcb_G"], r["pcw_slabs"], r["pcw_G"], r["dh_splits"],
                                    r["items"], " (half)" if r["half_item"] else ""))
    for arch, hw, R in RP_CASES:
        r = rp_regime(arch, hw, R)
        rows.append("rp %-8s %-8s R=%-4d K=%-6d row tiles %d  fwd %d (G %d)  dW %d (G %d)"
                    % (arch, GEO_IDS[hw], R, r["K"], r["row_tiles"], r["fwd_splits"], r["fwd_G"], r["w_slabs"],
                       r["w_G"]))
    return rows


def _rng(*key):
    return np.random.RandomState([20250311] + [int(k) for k in key])


def pc_inputs(n, A, side):
    """h [n, 512] in [-0.5, 1.5), dq [n, side, side, A] (NHWC), dh0 [n, 512] float32."""
    rng = _rng(1, n, A, side)
    return ((rng.random_sample((n, 512)) * 2.0 - 0.5).astype(np.float32),
            rng.standard_normal((n, side, side, A)).astype(np.float32),
            rng.standard_normal((n, 512)).astype(np.float32))


def rp_inputs(R, K):
    """x [R, K] (three frames' conv_base maps, NHWC each), dout [R, 4] with column 3 (the padding
    logit) set to 3.0: it must not reach any gradient."""
    rng = _rng(2, R, K)
    x = (rng.standard_normal((R, K)) * 0.1).astype(np.float32)
    dout = rng.standard_normal((R, 4)).astype(np.float32)
    dout[:, 3] = 3.0
    return x, dout
