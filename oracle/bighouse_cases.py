"""Case tables of the BigHouse trunk regime tests and the launch rules they rest on (TEST
INFRASTRUCTURE ONLY — see oracle/__init__.py).

forward_bignet / backward_bignet (csrc/vn_policy.hip) choose their kernels from the row count n
alone, through the launch helpers whose rules oracle/unreal_head_cases.py restates (splitk_count
and the two lines after it, the slab count of launch_wgrad / launch_wgrad6, the lanes per output
of launch_splitk_epilogue / launch_wgrad_reduce). trunk_regime(n, A) feeds them BigHouseModel's
shapes (84x84 frames: 20x20x32 -> 9x9x64 -> 7x7x32 -> 512 -> A + 1) and gives, per product, the
slab count, the reduce / epilogue lanes, the kchunk with the length of the last slab, and the row
remainder against the product's tile. SWITCHES names every switch in n with the two cases of
CASE_N that stand nearest to it on either side; tests/test_bighouse_cases.py checks on the CPU
that the regimes on the two sides are those of the last n before and the first n past the switch
and that every n of CASE_N is named by some switch. tests/test_bighouse_regimes_gpu.py runs the
cases against float64. numpy only: nothing here needs the GPU.

conv_merge's forward (K = 1568 = 49 K tiles of 32) walks more slab counts than its two 32-long
last slabs: 17 slabs of 96 up to n = 192, 13 of 128 up to n = 320, then 10 of 160 (last 128), 7
of 224 (the one even split), 6 of 288 (last 128) and 5 of 320 (last 288) before the unsplit
kernel at n = 961; CASE_N holds the first n of each.

Not covered: above n = 7936 the weight-gradient slab cap (SLAB = 24 M floats) halves
conv_merge's slab count (32 slabs of 512 x 1569 no longer fit); a case there needs an 8k-row
float64 oracle.
"""
import math

import numpy as np

from .unreal_head_cases import BK, REDUCE_FLAT, SK_TILES, SLAB, reduce_lanes, splitk_chunk, wgrad_chunk  # noqa: F401

HW = (84, 84)
O1, O2, O3 = 20, 9, 7                 # conv1 k8 s4, conv2 k4 s2, conv3 k3 s1 output sides
FCIN = 32 * O3 * O3                   # conv_merge's K: 1568
MERGE_TAIL = FCIN - 32                # the features of the 32-long last K slab start here

# product -> (BM, BN) of its launch (csrc/vn_policy.hip forward_bignet / backward_bignet)
TILES = {"conv1_fwd": (128, 32), "conv2_fwd": (64, 64), "conv3_fwd": (128, 32), "merge_fwd": (64, 64),
         "heads_fwd": (64, 16), "heads_dgrad": (64, 64), "heads_wgrad": (32, 64), "merge_dgrad": (64, 64),
         "merge_wgrad": (128, 128), "conv3_wgrad": (32, 64), "conv3_dgrad": (64, 64), "conv2_wgrad": (64, 128),
         "conv1_wgrad": (32, 64)}


def _split(M, N, K, tile, rows):
    slabs, kchunk = splitk_chunk(M, N, K, *tile)
    return {"slabs": slabs, "lanes": reduce_lanes(M, N, slabs) if slabs > 1 else 0, "kchunk": kchunk,
            "last": K - (slabs - 1) * kchunk, "rem": rows % tile[0]}


def _wgrad(M, KP, P, tile):
    slabs, kchunk = wgrad_chunk(M, KP, P, tile[0], tile[1], True)
    return {"slabs": slabs, "lanes": reduce_lanes(M, KP + 1, slabs) if slabs > 1 else 0, "kchunk": kchunk,
            "last": P - (slabs - 1) * kchunk, "rem": P % BK}


def trunk_regime(n, A=4):
    """The regime of every product of forward_bignet / backward_bignet at n rows and A actions:
    {product: {slabs, lanes, kchunk, last, rem}}. slabs = 1: the unsplit kernel / the direct
    EpiWgrad epilogue (lanes 0: no reduce launch). kchunk / last: the slab length along the
    reduction and that of the last slab (K or P when unsplit). rem: the rows left over against
    the product's row tile (forward and input-gradient products), the reduction rows left over
    against the K tile of 32 (weight gradients); merge_dgrad also carries col_rem, its N = 1568
    against the 64-wide column tile."""
    P1, P2, P3 = n * O1 * O1, n * O2 * O2, n * O3 * O3
    r = {
        # forward: conv1 .. conv3 are launch_gemm_x6 (never split), conv_merge and the heads split K
        "conv1_fwd": {"slabs": 1, "lanes": 0, "kchunk": 192, "last": 192, "rem": P1 % TILES["conv1_fwd"][0]},
        "conv2_fwd": {"slabs": 1, "lanes": 0, "kchunk": 512, "last": 512, "rem": P2 % TILES["conv2_fwd"][0]},
        "conv3_fwd": {"slabs": 1, "lanes": 0, "kchunk": 576, "last": 576, "rem": P3 % TILES["conv3_fwd"][0]},
        "merge_fwd": _split(n, 512, FCIN, TILES["merge_fwd"], n),
        "heads_fwd": _split(n, A + 1, 512, TILES["heads_fwd"], n),
        # backward: the input gradients are unsplit, the weight gradients split the reduction rows
        "heads_dgrad": {"slabs": 1, "lanes": 0, "kchunk": A + 1, "last": A + 1, "rem": n % TILES["heads_dgrad"][0]},
        "heads_wgrad": _wgrad(A + 1, 512, n, TILES["heads_wgrad"]),
        "merge_dgrad": {"slabs": 1, "lanes": 0, "kchunk": 512, "last": 512, "rem": n % TILES["merge_dgrad"][0],
                        "col_rem": FCIN % TILES["merge_dgrad"][1]},
        "merge_wgrad": _wgrad(512, FCIN, n, TILES["merge_wgrad"]),
        "conv3_wgrad": _wgrad(32, 576, P3, TILES["conv3_wgrad"]),
        "conv3_dgrad": {"slabs": 1, "lanes": 0, "kchunk": 288, "last": 288, "rem": P2 % TILES["conv3_dgrad"][0]},
        "conv2_wgrad": _wgrad(64, 512, P2, TILES["conv2_wgrad"]),
        "conv1_wgrad": _wgrad(32, 192, P1, TILES["conv1_wgrad"]),
    }
    return r


# ---- the cases ----------------------------------------------------------------------------------
# the smallest set with a case next to every switch below, on either side
CASE_N = (1, 3, 5, 6, 26, 42, 65, 127, 128, 193, 257, 321, 449, 641, 769, 961)
PROD_N = 961  # the smallest n at which conv_merge's forward is unsplit: 15 row tiles + 1 row

# (what switches, product, key, first n past the switch, nearest case below, nearest case above)
SWITCHES = (
    ("one row -> more (one row: M = 1 in every tile, conv1's weight gradient at its fewest slabs, 2)",
     "merge_fwd", "rows>1", 2, 1, 3),
    ("conv2 weight gradient: direct EpiWgrad -> slabs", "conv2_wgrad", "slabs", 4, 3, 5),
    ("conv3 weight gradient: direct EpiWgrad -> slabs", "conv3_wgrad", "slabs", 6, 5, 6),
    ("conv1 weight gradient: reduce lanes 1 -> 2", "conv1_wgrad", "lanes", 6, 5, 6),
    ("conv2 weight gradient: reduce lanes 1 -> 2", "conv2_wgrad", "lanes", 26, 6, 26),
    ("conv3 weight gradient: reduce lanes 1 -> 2", "conv3_wgrad", "lanes", 42, 26, 42),
    ("a second 64-row tile of n (conv_merge, heads, their input gradients)", "merge_fwd", "row_tiles", 65, 42, 65),
    ("conv_merge forward: epilogue lanes 4 -> 1 (M N = 65536)", "merge_fwd", "lanes", 128, 127, 128),
    ("conv1 weight gradient: reduce lanes 32 -> 64 (their cap)", "conv1_wgrad", "lanes", 164, 128, 193),
    ("conv_merge forward: 17 slabs of 96 -> 13 of 128", "merge_fwd", "slabs", 193, 128, 193),
    ("heads weight gradient: direct EpiWgrad -> 2 slabs", "heads_wgrad", "slabs", 257, 193, 257),
    ("conv_merge weight gradient: direct EpiWgrad -> 2 slabs", "merge_wgrad", "slabs", 257, 193, 257),
    ("conv_merge forward: 13 slabs of 128 -> 10 of 160", "merge_fwd", "slabs", 321, 257, 321),
    ("conv_merge forward: 10 slabs -> 7 of 224 (even)", "merge_fwd", "slabs", 449, 321, 449),
    ("conv_merge forward: 7 slabs -> 6 of 288", "merge_fwd", "slabs", 641, 449, 641),
    ("conv_merge forward: 6 slabs -> 5 of 320", "merge_fwd", "slabs", 769, 641, 769),
    ("conv_merge forward: 5 slabs -> unsplit, 64-wide K tile", "merge_fwd", "slabs", 961, 769, 961),
)


def regime_value(n, product, key, A=4):
    if key == "row_tiles":
        return -(-n // TILES[product][0])
    if key == "rows>1":
        return n > 1
    return trunk_regime(n, A)[product][key]


def uncovered(ns):
    """The switches of SWITCHES that the case list ns leaves without a side: the nearest n of ns
    on either side must sit in the regime of the last n before / the first n past the switch."""
    ns = sorted(ns)
    out = []
    for what, product, key, at, _, _ in SWITCHES:
        below = [n for n in ns if n < at]
        above = [n for n in ns if n >= at]
        lo_v, hi_v = regime_value(at - 1, product, key), regime_value(at, product, key)
        if not below or not above or regime_value(below[-1], product, key) != lo_v or \
                regime_value(above[0], product, key) != hi_v:
            out.append(what)
    return out


ACTION_COUNTS = (1, 3, 7)                       # besides 4
ACTION_CASES = [(n, A) for n in (5, 65) for A in ACTION_COUNTS]
ROWS_N = (26, 257)                              # frames gathered by row from an arena
# arena sizes: fewer rows than samples, so some rows repeat, but most samples see a frame of their
# own. The elementwise bound on logits and values has a floor of 1e-6 of the tensor's scale, the
# largest |value| among the distinct frames, while float32 rounding is set by the terms of the sum
# (sum |w f| ~ 0.15 here, 5 to 14 times the values): with a dozen distinct frames the scale of the
# values fell to 0.0104, the floor to one float32 ulp of the terms, and a plain float32 forward on
# the CPU came to 0.77 of the bound (2.4e-6 of scale) on such an arena.
ARENA_ROWS = {26: 20, 257: 200}
FLOAT_N = (3, 65, 257)
FLOAT_U8_N = 3
GUARD_N = (5, 65)
COTANGENT_N = (42, 193)                         # dz5_in + dx3_extra
DETERMINISM_N = (128, PROD_N)
EXPOSURE_N = 6                                  # the case of the CPU fault-exposure test


def regime_table(ns=CASE_N, A=4):
    """The regimes of the cases as text rows (DESIGN.md holds a copy)."""
    rows = []
    for n in ns:
        r = trunk_regime(n, A)
        f = r["merge_fwd"]
        rows.append("n=%-4d conv_merge fwd %2d x %-3d (last %3d, lanes %d)  heads fwd %d  dW heads %d merge %d  "
                    "conv3 %3d (lanes %2d)  conv2 %3d (lanes %2d)  conv1 %3d (lanes %2d)  rows left: conv1 %3d conv2 %2d "
                    "conv3 %3d n %2d" % (n, f["slabs"], f["kchunk"], f["last"], f["lanes"], r["heads_fwd"]["slabs"],
                                         r["heads_wgrad"]["slabs"], r["merge_wgrad"]["slabs"],
                                         r["conv3_wgrad"]["slabs"], r["conv3_wgrad"]["lanes"],
                                         r["conv2_wgrad"]["slabs"], r["conv2_wgrad"]["lanes"],
                                         r["conv1_wgrad"]["slabs"], r["conv1_wgrad"]["lanes"], r["conv1_fwd"]["rem"],
                                         r["conv2_fwd"]["rem"], r["conv3_fwd"]["rem"], f["rem"]))
    return rows


# ---- seeded inputs ------------------------------------------------------------------------------
def _rng(*key):
    return np.random.RandomState([20250611] + [int(k) for k in key])


def weight_seed(n, A, key=0):
    """Seed of a case's parameters (init_state) and of their N(0, 0.01) noise."""
    return 100000 * key + 10 * n + A


LAYER_SHAPES = (("conv_base.0.0", 32, 8, 3), ("conv_base.0.2", 64, 4, 32), ("conv_base.0.4", 32, 3, 64))


def init_state(seed, A=4):
    """PolicyNet(arch="bighouse").init_params(seed) in the reference's names and shapes, restated
    so that it runs without the GPU: bias 0, W ~ U(+-1/sqrt(fan_in)) drawn layer by layer from one
    torch CPU generator into [Cout][ky][kx][Cin] / [512][7][7][32] rows (the flat layout), then
    permuted as PolicyNet.to_reference does. The GPU test asserts it equals init_params bit for
    bit."""
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)

    def draw(co, k):
        d = 1.0 / math.sqrt(k)
        return torch.empty(co, k, dtype=torch.float32).uniform_(-d, d, generator=g)
    sd = {}
    for name, co, kk, ci in LAYER_SHAPES:
        sd[name + ".weight"] = draw(co, kk * kk * ci).reshape(co, kk, kk, ci).permute(0, 3, 1, 2).contiguous()
        sd[name + ".bias"] = torch.zeros(co)
    sd["conv_merge.0.1.weight"] = draw(512, FCIN).reshape(512, O3, O3, 32).permute(0, 3, 1, 2).reshape(512, -1).contiguous()
    sd["conv_merge.0.1.bias"] = torch.zeros(512)
    head = draw(A + 1, 512)
    sd["policy_logits.0.weight"], sd["policy_logits.0.bias"] = head[:A].clone(), torch.zeros(A)
    sd["critic.0.weight"], sd["critic.0.bias"] = head[A:A + 1].clone(), torch.zeros(1)
    return sd


def seeded_state(n, A=4, key=0):
    """A case's parameters by reference name: init_state + N(0, 0.01) on every tensor (biases
    included), float32."""
    import torch
    seed = weight_seed(n, A, key)
    sd = init_state(seed, A)
    g = torch.Generator(device="cpu").manual_seed(seed + 1)
    return {k: v + 0.01 * torch.randn(v.shape, generator=g, dtype=torch.float32) for k, v in sd.items()}


def u8_frames(n, key=0):
    """image uint8 [n, 84, 84, 3]."""
    return _rng(1, n, key).randint(0, 256, size=(n,) + HW + (3,)).astype(np.uint8)


def float_frames(n):
    """image float32 [n, 3, 84, 84] uniform in [0, 1): not the k/255 grid of scaled u8 frames, so
    a path that quantised its input shows."""
    return _rng(2, n).random_sample((n, 3) + HW).astype(np.float32)


def arena_rows(n):
    """(arena uint8 [R, 84, 84, 3], rows int32 [n]) with R = ARENA_ROWS[n] < n, so some rows
    repeat; the last arena row is used (by the last sample among others), row 0 by sample 0."""
    R = ARENA_ROWS[n]
    rng = _rng(3, n)
    arena = rng.randint(0, 256, size=(R,) + HW + (3,)).astype(np.uint8)
    rows = rng.randint(0, R, size=n).astype(np.int32)
    rows[0], rows[n // 2], rows[n - 1] = 0, R - 1, R - 1
    return arena, rows


def trunk_cotangents(n):
    """(dz5 float32 [n, 512], dx3 float32 [n, 7, 7, 32] NHWC): a cotangent of conv_merge's
    features and a gradient to add at conv_base's output (reward prediction's place). The dz5 a
    caller hands backward_bignet is dL/dZ5, already masked by the features' ReLU (as
    vn_lstm_backward writes it): the test multiplies this draw by the GPU's mask first."""
    rng = _rng(4, n)
    return rng.standard_normal((n, 512)).astype(np.float32), rng.standard_normal((n, O3, O3, 32)).astype(np.float32)
