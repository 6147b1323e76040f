"""Case tables of the goal trunk's regime tests and the launch rules they rest on (TEST
INFRASTRUCTURE ONLY — see oracle/__init__.py).

forward_impl / backward_impl of csrc/vn_policy.hip (arch 0, the default network) choose their
kernels from the frame geometry and the row count n alone. The products on the generic helpers
follow the rules oracle/unreal_head_cases.py restates (splitk_count and the two lines after it,
the slab count of launch_wgrad / launch_wgrad6, the lanes per output of launch_splitk_epilogue /
launch_wgrad_reduce); the persistent kernels launch min(items, resident_blocks(...)) workgroups
over work items whose count the band structs fix (Conv1X3Band, Conv1WgBand, Conv2FwdBand,
Conv2DgBand, ParityDg, WgSpec — restated below with their constants as they stand in the source).
trunk_regime(hw, n, A) gives, per product, the slabs, the reduce / epilogue lanes, the kchunk with
the length of the last slab, the row and column remainders against the product's tile, and for the
persistent kernels the item count, the images packed per item, whether the last item is part
filled, and whether the x6 weight gradients take the two-stage slab reduce. SWITCHES[hw] names
every switch in n between 18 rows and the geometry's cap; CASES[hw] is a smallest set of n with a
case in the right regime on each side of every switch (the first n past a switch wherever one n can
serve); EDGE_CASES adds the two n around each two-stage reduce's first use. tests/test_goal_trunk_cases.py
checks that on the CPU, tests/test_goal_trunk_regimes_gpu.py runs the cases against float64. numpy
only: nothing here needs the GPU.

resident_blocks is a device query, so a table cannot know where a persistent grid wraps. It knows
two bounds: with items <= the CU count every workgroup takes one item at most (may_wrap False),
and with items > CUs x (2048 / threads per workgroup) some workgroup takes two whatever the
occupancy (must_wrap True). The table uses NOMINAL_CUS; the GPU test asserts both against
multi_processor_count before it runs. The two-stage reduce of launch_conv_wgrad_x6 starts at
bx = min(items, resident_blocks / G) >= 2 kParts = 64 workgroups: from 64 items on, given at least
64 G resident workgroups, which the GPU test asserts the same way (one workgroup of 512 threads
per CU: 256 / G).

Not covered (tests/test_prod_oracle_gpu.py stands on the far side where it reaches):
- Float frames above 17 rows: the regime cases run u8 frames, dense and row-gathered; float frames
  take the im2col conv1 forward and weight gradient and the four-class conv2 input gradient, held
  to fp64 at n = 3 and 17 only (tests/test_few_env_gpu.py).
- The goal-runs path (vn_goal_runs: frame lists and goal deltas through every frame-level kernel);
  tests/test_goal_runs_gpu.py compares it with the plain path, not with fp64.
- Certain wraps beyond the caps: at 84x84 the parity input gradient (n > 4096), conv3's weight
  gradient (n > 1536); at 174x174 conv2's forward (n > 1024), conv2's input gradient (n > 512), the
  parity input gradient (n > 2048) and conv3's weight gradient (n > 512); at 300x400 every kernel
  but conv2's forward and weight gradient (conv1's from n = 54, conv3's weight gradient from 61,
  conv2's input gradient from 103, the parity bands from 513).
  The n = 4096 and n = 512 tests wrap these at the occupancy the device really gives.
- The heads' and conv_merge's weight gradients on 4 and 5 slabs (n = 769, 1025 at 84x84): more of
  the 3-slab form, whose key here is min(slabs, 3).
- 174x174 above n = 260 and 300x400 above n = 40 up to the n = 512 tests: conv_merge's forward
  unsplit from n = 961 at 174x174 is run at 84x84 only.
"""
import functools

import numpy as np

from . import few_env_cases as fc
from .few_env_cases import GEO_IDS, GEOMETRIES, fcin, loss_inputs, trunk_sizes, u8_frames, weight_seed  # noqa: F401
from .unreal_head_cases import BK, REDUCE_FLAT, SK_CAP, SK_TILES, SLAB, reduce_lanes, splitk_chunk, wgrad_chunk  # noqa: F401

FIRST_N = fc.SKINNY_ROWS + 2            # 18: the first n the few-env tests leave (they end at 17)
CAPS = {(84, 84): 1030, (174, 174): 260, (300, 400): 40}
NOMINAL_CUS = 256                       # MI355X; the GPU test asserts the bounds against the device's count
KPARTS = 32                             # kParts of launch_conv_wgrad_x6
LDS_MAX = 160 * 1024


def _cdiv(a, b):
    return (a + b - 1) // b


# ---- the band structs of the persistent kernels, restated -------------------------------------
def conv1_fwd_bands(hw):
    """Conv1X3Band<H, W>::NB: bands per frame of conv1_fwd_x3r_kernel (256 threads)."""
    H, W = hw
    rs = _cdiv(W * 3, 4) * 4
    oh = (H - 7) // 4 + 1
    br = oh
    while br > 1 and min(4 * br + 4, H) * rs * 2 + 11 * 3 * 64 * 16 > 80 * 1024:
        br -= 1
    return _cdiv(oh, br)


CONV1_WG_RSQ = {(84, 84): 296, (174, 174): 888, (300, 400): 1464}   # Conv1WgQ<H, W>::RSQ


def conv1_wgrad_bands(hw):
    """Conv1WgBand<H, W>::NB: bands per frame of conv1_wgrad_x3_kernel (256 threads)."""
    H = hw[0]
    oh = (H - 7) // 4 + 1
    br = oh
    while br > 1 and min(4 * br + 3, H) * CONV1_WG_RSQ[hw] * 2 > 56 * 1024:
        br -= 1
    return _cdiv(oh, br)


def conv2_fwd_bands(hw):
    """Conv2FwdBand<...>::NB (conv2_fwd_x6_kernel, 512 threads); 174x174 streams whole frames
    through conv2_fwd_ring2_kernel (256 threads) above 16 rows: one item per frame."""
    (ih, iw), (oh, ow), _ = trunk_sizes(*hw)
    if (ih, iw, oh, ow) == (42, 42, 20, 20):
        return 1
    tiled = (ih, iw, oh, ow) == (20, 20, 9, 9)
    rsp = 680 if tiled else 2 * ((iw + 1) // 2) * 32
    br = oh
    while br > 1 and 3 * min(2 * br + 2, ih) * rsp * 2 + 4 * _cdiv(br * ow, 16) * 16 * 36 * 4 > LDS_MAX:
        br -= 1
    return _cdiv(oh, br)


def conv2_dgrad_bands(hw):
    """Bands per frame of conv2's input gradient: 1 on even conv1 maps (conv2_dgrad_x6_kernel, a
    whole frame per item), Conv2DgBand<...>::NB on odd ones (300x400: conv2_dgrad_band_x6_kernel)."""
    (ih, iw), (oh, ow), _ = trunk_sizes(*hw)
    if ih % 2 == 0 and iw % 2 == 0:
        return 1
    by = 16
    while by > 2 and 3 * ((by // 2 + 3) * ((iw + 1) // 2) + 16) * 32 * 2 + by * iw * 4 > 80 * 1024:
        by -= 2
    return _cdiv(ih, by)


def conv2_dgrad_threads(hw):
    (ih, iw), _, _ = trunk_sizes(*hw)
    if ih % 2 or iw % 2:
        return 256
    rows = _cdiv((ih // 2) * (iw // 2), 16) * 16 + iw // 2 + 1   # conv2_dgrad_x6_rows
    return 256 if 3 * rows * 32 * 2 + ih * iw * 4 <= 64 * 1024 else 512


def parity_dgrad(hw):
    """(IMG, bands per image) of conv3's input gradient: ParityDg<OH3, OW3, CH / 2, CW / 2, 64, 64, 2>
    ::IMG images per item where the planes fit (launch_parity_dgrad_x6), else bands of class rows
    (parity_dgrad_band_x6_kernel, 300x400), one image per item. 512 threads."""
    _, (h, w), (oh, ow) = trunk_sizes(*hw)
    yc, xc = min(h, 2 * (oh - 1) + 4) // 2, min(w, 2 * (ow - 1) + 4) // 2
    npc, kc = yc * xc, 64

    def rows(img):
        return _cdiv(img * npc, 16) * 16 + xc + 1
    img = (2 if 3 * rows(2) * kc * 2 <= LDS_MAX else 1) if npc >= 64 else 64 // npc
    if 3 * rows(img) * kc * 2 <= LDS_MAX:
        return img, 1
    bmax = next(b for b in range(yc, 0, -1) if 3 * (_cdiv(b * xc, 16) * 16 + xc + 1) * kc * 2 <= 150 * 1024)
    nb = _cdiv(yc, bmax)
    by = _cdiv(yc, nb)
    return 1, _cdiv(yc, by)


def _wgspec(ih, iw, oh, ow, co, br, img):
    """WgSpec<...>: (fits, NB) at 32 channels per input group."""
    kp = img * br * ow
    xr = min(2 * br + 2, ih)
    lds = 3 * ((kp + 1) * (co + 16) + (img * xr * iw + 1) * 40) * 2
    return oh % br == 0 and lds <= LDS_MAX, oh // br


def conv3_wgrad_spec(hw):
    """(IMG, NB, G) of Conv3Wg: whole maps packed to >= 32 reduction pixels, else bands of one row,
    two images per item."""
    _, (ih, iw), (oh, ow) = trunk_sizes(*hw)
    img = 1 if oh * ow >= 32 else 32 // (oh * ow)
    fits, nb = _wgspec(ih, iw, oh, ow, 64, oh, img)
    if fits:
        return img, nb, 2
    fits, nb = _wgspec(ih, iw, oh, ow, 64, 1, 2)
    assert fits
    return 2, nb, 2


def conv2_wgrad_spec(hw):
    """(IMG, NB, G) of Conv2Wg over the 2n frames."""
    (ih, iw), (oh, ow), _ = trunk_sizes(*hw)
    fits, nb = _wgspec(ih, iw, oh, ow, 32, 4 if oh % 4 == 0 and oh > 9 else oh, 1)
    if fits:
        return 1, nb, 1
    fits, nb = _wgspec(ih, iw, oh, ow, 32, 1, 1)
    assert fits
    return 1, nb, 1


def _persistent(items, threads, img=1, n=0, G=0):
    r = {"items": items, "threads": threads, "img": img, "part_item": bool(img > 1 and n % img),
         "may_wrap": items > NOMINAL_CUS // max(G, 1), "must_wrap": items > NOMINAL_CUS * (2048 // threads) // max(G, 1)}
    if G:  # an x6 weight gradient: bx = min(items, resident / G) slabs, two-stage from 2 kParts on
        r["two_stage"] = items >= 2 * KPARTS
        r["short_parts"] = items < KPARTS   # the one-stage reduce reads fewer than kParts live slabs
    return r


# ---- the regime of every product ------------------------------------------------------------
def _split(M, N, K, tile, big=False):
    slabs, kchunk = (1, K) if big else splitk_chunk(M, N, K, *tile)
    return {"slabs": slabs, "lanes": reduce_lanes(M, N, slabs) if slabs > 1 else 0, "kchunk": kchunk,
            "last": K - (slabs - 1) * kchunk, "rem": M % tile[0], "col_rem": N % tile[1], "row_tiles": _cdiv(M, tile[0]),
            "tile": tile[0]}


def _wgrad(M, KP, P, tile):
    slabs, kchunk = wgrad_chunk(M, KP, P, tile[0], tile[1], True)
    return {"slabs": slabs, "slabs3": min(slabs, 3), "lanes": reduce_lanes(M, KP + 1, slabs) if slabs > 1 else 0,
            "kchunk": kchunk, "last": P - (slabs - 1) * kchunk, "rem": P % BK}


def trunk_regime(hw, n, A=4):
    """The regime of every product of forward_impl / backward_impl at geometry hw, n > 16 rows of u8
    frames and A actions: {product: {...}}.

    Split products (launch_gemm_x6_sk / launch_gemm_sk / the unsplit launches): slabs (1: the unsplit
    kernel with its own epilogue), lanes (epilogue lanes per output, 0 unsplit), kchunk and last (the
    slab length along K and that of the last slab), rem / col_rem (rows and columns left over against
    the tile), row_tiles, tile (the row tile: conv_merge's input gradient moves to 128).
    Weight gradients on launch_wgrad / launch_wgrad6: slabs (1: the direct EpiWgrad epilogue), slabs3
    = min(slabs, 3), lanes of launch_wgrad_reduce, kchunk / last along the reduction rows, rem against
    the K tile of 32.
    Persistent kernels: items, threads, img (images per item), part_item (the last item part filled),
    may_wrap / must_wrap (see the module text), and for the x6 weight gradients two_stage and
    short_parts."""
    (o1h, o1w), (o2h, o2w), (o3h, o3w) = trunk_sizes(*hw)
    K5, n9, frames = fcin(hw), n * o3h * o3w, 2 * n
    big = K5 >= 1024 and n >= 256
    c3 = conv3_wgrad_spec(hw)
    c2 = conv2_wgrad_spec(hw)
    pimg, pnb = parity_dgrad(hw)
    return {
        "conv1_fwd": _persistent(frames * conv1_fwd_bands(hw), 256),
        "conv2_fwd": _persistent(frames * conv2_fwd_bands(hw), 256 if hw == (174, 174) else 512),
        "conv3_fwd": _split(n9, 64, 1024, (128, 64) if o3h * o3w >= 64 else (64, 64)),
        "conv4_fwd": _split(n9, 32, 64, (128, 32), big=True),
        "merge_fwd": _split(n, 512, K5, (64, 64)),
        "heads_fwd": _split(n, A + 1, 512, (64, 16)),
        "heads_dgrad": _split(n, 512, A + 1, (64, 64), big=True),
        "heads_wgrad": _wgrad(A + 1, 512, n, (32, 64)),
        "merge_dgrad": _split(n, K5, 512, (128, 128) if big else (64, 64), big=big),
        "merge_wgrad": _wgrad(512, K5, n, (128, 128)),
        "conv4_dgrad": _split(n9, 64, 32, (64, 64), big=True),
        "conv4_wgrad": _wgrad(32, 64, n9, (32, 64)),
        "conv3_wgrad": _persistent(_cdiv(n, c3[0]) * c3[1], 512, c3[0], n, c3[2]),
        "conv3_dgrad": _persistent(_cdiv(n, pimg) * pnb, 512, pimg, n),
        "conv2_wgrad": _persistent(_cdiv(frames, c2[0]) * c2[1], 512, c2[0], frames, c2[2]),
        "conv2_dgrad": _persistent(frames * conv2_dgrad_bands(hw), conv2_dgrad_threads(hw)),
        "conv1_wgrad": _persistent(frames * conv1_wgrad_bands(hw), 256),
    }


PERSISTENT = ("conv1_fwd", "conv2_fwd", "conv3_wgrad", "conv3_dgrad", "conv2_wgrad", "conv2_dgrad", "conv1_wgrad")


def regime_value(hw, n, product, key, A=4):
    return trunk_regime(hw, n, A)[product][key]


# ---- the switches ---------------------------------------------------------------------------
# (what switches, product, key): the places follow from trunk_regime by a scan of n (switch_points)
_KEYS = (
    ("conv3 forward: slabs x kchunk", "conv3_fwd", "kchunk"),
    ("conv3 forward: epilogue lanes", "conv3_fwd", "lanes"),
    ("conv_merge forward: slabs x kchunk (unsplit: the 64-wide K tile)", "merge_fwd", "kchunk"),
    ("conv_merge forward: epilogue lanes", "merge_fwd", "lanes"),
    ("conv_merge input gradient: slabs x kchunk", "merge_dgrad", "kchunk"),
    ("conv_merge input gradient: 64 x 64 -> 128 x 128 tiles", "merge_dgrad", "tile"),
    ("heads weight gradient: direct EpiWgrad -> 2 slabs -> 3", "heads_wgrad", "slabs3"),
    ("conv_merge weight gradient: direct EpiWgrad -> 2 slabs -> 3", "merge_wgrad", "slabs3"),
    ("conv4 weight gradient: direct EpiWgrad -> slabs", "conv4_wgrad", "slabs3"),
    ("conv4 weight gradient: reduce lanes", "conv4_wgrad", "lanes"),
    ("conv2 weight gradient: two-stage slab reduce", "conv2_wgrad", "two_stage"),
    ("conv3 weight gradient: two-stage slab reduce", "conv3_wgrad", "two_stage"),
    ("conv2 weight gradient: one stage over fewer than kParts slabs", "conv2_wgrad", "short_parts"),
    ("conv3 weight gradient: one stage over fewer than kParts slabs", "conv3_wgrad", "short_parts"),
    ("a second 64-row tile of n (conv_merge, heads, their input gradients)", "heads_dgrad", "row_tiles>1"),
) + tuple(("%s: items > CUs (a wrap is possible)" % p, p, "may_wrap") for p in PERSISTENT) \
  + tuple(("%s: items > CUs x 2048 / threads (a wrap is certain)" % p, p, "must_wrap") for p in PERSISTENT)


@functools.lru_cache(maxsize=None)
def _regime4(hw, n):
    return trunk_regime(hw, n)


def _value(hw, n, product, key):
    if key == "row_tiles>1":
        return n > 64
    v = _regime4(hw, n)[product][key]
    if key == "slabs3" and product == "conv4_wgrad":
        return min(v, 2)    # direct or slabs: their count grows with n at every step
    return v


def switch_points(hw):
    """[(what, product, key, at)]: every n in FIRST_N + 1 .. cap at which a key of _KEYS changes."""
    out = []
    for what, product, key in _KEYS:
        prev = _value(hw, FIRST_N, product, key)
        for n in range(FIRST_N + 1, CAPS[hw] + 1):
            v = _value(hw, n, product, key)
            if v != prev:
                out.append((what, product, key, n))
                prev = v
    return sorted(out, key=lambda s: (s[3], s[1], s[2]))


def _runs(hw, product, key, at):
    """([lo0, at - 1], [at, hi1]): the runs of n around the switch over which the key keeps the value
    of the last n before / the first n past it."""
    a, b = _value(hw, at - 1, product, key), _value(hw, at, product, key)
    lo0 = at - 1
    while lo0 - 1 >= FIRST_N and _value(hw, lo0 - 1, product, key) == a:
        lo0 -= 1
    hi1 = at
    while hi1 + 1 <= CAPS[hw] and _value(hw, hi1 + 1, product, key) == b:
        hi1 += 1
    return (lo0, at - 1), (at, hi1)


@functools.lru_cache(maxsize=None)
def switches(hw):
    """SWITCHES[hw]: (what, product, key, at, run below, run above)."""
    return tuple(s + _runs(hw, *s[1:]) for s in switch_points(hw))


def smallest_case_set(hw):
    """A smallest set of n with one in the run below and one in the run above every switch: the
    intervals stabbed from the top, each by its left end (so the first n past a switch wherever a
    switch's upper run is the one that forces a case)."""
    iv = []
    for s in switches(hw):
        iv += [s[4], s[5]]
    chosen = []
    for lo, hi in sorted(iv, key=lambda r: -r[0]):
        if not any(lo <= c <= hi for c in chosen):
            chosen.append(lo)
    return tuple(sorted(chosen))


SWITCHES = {hw: switches(hw) for hw in GEOMETRIES}


def uncovered(hw, ns):
    """The switches that the case list ns leaves without a case on one side."""
    out = []
    for what, product, key, at, below, above in switches(hw):
        if not any(below[0] <= n <= below[1] for n in ns) or not any(above[0] <= n <= above[1] for n in ns):
            out.append("%s at %d" % (what, at))
    return out


# ---- the cases --------------------------------------------------------------------------------
# smallest_case_set(hw) at 84x84 and 174x174 (tests/test_goal_trunk_cases.py asserts it). The packing
# tails fall out of them: conv3's weight gradient packs 3 images at 84x84 (18, 363, 726 fill the last
# item, the others do not, on both the one-stage and the two-stage reduce), the parity input gradient
# packs 4 there (every n mod 4 occurs) and 2 at 174x174 (even and odd n).
CASES = {
    (84, 84): (18, 29, 242, 363, 520, 605, 726, 1025),
    (174, 174): (18, 26, 51, 74, 102, 116, 135, 193, 257),
    # 300x400, two cases: 18 (the first tensor-core n; conv_merge's input gradient on 64 x 64 tiles, never
    # split) and SECOND_300
    (300, 400): (18, 37),
}
# 300x400's second case, one n of 30..40 by the item counts: conv3's weight gradient packs 2 images per item
# (bands of one row: 17 items per pair), so an odd n leaves the last 17 items half filled; 37 also sits past
# conv3's last forward switch in range (4 slabs of 256 from n = 34) and leaves 3 rows of 14467 in conv3's last
# 128-row tile. conv2's forward and weight gradient (72 n items) wrap for certain from n = 15; no other kernel
# does below n = 54, and no n above 16 rows keeps every grid within the CU count (72 n <= 256 ends at n = 3).
# Its conv3 forward regimes between them (7 x 160 from n = 21, 6 x 192 from 24, 5 x 224 from 28) are left
# without a case, so the four switches of UNCOVERED_300 lack a side: the same kernel instance runs those chunk
# lengths at 174x174 (n = 102, 116, 135).
SECOND_300 = 37
UNCOVERED_300 = ("conv3 forward: slabs x kchunk at 21", "conv3 forward: slabs x kchunk at 24",
                 "conv3 forward: slabs x kchunk at 28", "conv3 forward: slabs x kchunk at 34")
TRUNK_CASES = [(hw, n) for hw in GEOMETRIES for n in CASES[hw]]
TRUNK_IDS = ["%s-n%d" % (GEO_IDS[hw], n) for hw, n in TRUNK_CASES]

# persistent kernels: the case above 16 rows at which no grid can wrap (every kernel's items <= CUs); the
# cases at which a wrap is certain are the must_wrap switches' upper sides
NO_WRAP_N = {(84, 84): 18, (174, 174): 18}
ACTION_COUNTS = (1, 3, 7)                        # besides 4
ACTION_N = (29, 257)                             # below 65 rows; the heads' weight gradient on 2 slabs
ACTION_CASES = [((84, 84), n, A) for n in ACTION_N for A in ACTION_COUNTS]
ACTION_IDS = ["84x84-n%d-A%d" % (n, A) for _, n, A in ACTION_CASES]
ROWS_CASES = [((84, 84), 242), ((174, 174), 74), ((300, 400), 18)]   # frames gathered by row from an arena
ROWS_IDS = ["%s-n%d" % (GEO_IDS[hw], n) for hw, n in ROWS_CASES]
GUARD_CASES = [((84, 84), 18), ((84, 84), 242), ((174, 174), 18), ((300, 400), 18)]   # 242: both x6 reduces two-stage
GUARD_IDS = ["%s-n%d" % (GEO_IDS[hw], n) for hw, n in GUARD_CASES]
GUARD_BITS = fc.GUARD_BITS
# besides the smallest lists: the first n of each two-stage slab reduce within the caps (exactly 2 kParts = 64
# slabs, 2 per part) with the n before it (the one-stage reduce at its most slabs). 189 | 190 is also the
# packing tail at its edge: 63 full items of 3 images against 63 and one image.
EDGE_CASES = [((84, 84), 31), ((84, 84), 32), ((84, 84), 189), ((84, 84), 190), ((174, 174), 63), ((174, 174), 64)]
EDGE_IDS = ["%s-n%d" % (GEO_IDS[hw], n) for hw, n in EDGE_CASES]


def regime_table(hw, ns=None, A=4):
    """The regimes of the cases as text rows (DESIGN.md holds a copy)."""
    rows = []
    for n in (ns or CASES[hw]):
        r = trunk_regime(hw, n, A)
        c3, cm, dg, w4 = r["conv3_fwd"], r["merge_fwd"], r["merge_dgrad"], r["conv4_wgrad"]
        rows.append("n=%-4d conv3 %2dx%-4d (last %3d, lanes %d)  merge fwd %2dx%-5d (last %4d, lanes %d)  dgrad %dx%-3d tile %3d  "
                    "dW heads %d merge %d conv4 %3d (lanes %2d)  items: c1f %4d c2f %4d c3w %3d%s%s pdg %3d%s c2w %4d%s c2d %4d "
                    "c1w %4d" % (n, c3["slabs"], c3["kchunk"], c3["last"], c3["lanes"], cm["slabs"], cm["kchunk"], cm["last"],
                                 cm["lanes"], dg["slabs"], dg["kchunk"], dg["tile"], r["heads_wgrad"]["slabs"],
                                 r["merge_wgrad"]["slabs"], w4["slabs"], w4["lanes"], r["conv1_fwd"]["items"],
                                 r["conv2_fwd"]["items"], r["conv3_wgrad"]["items"],
                                 "*" if r["conv3_wgrad"]["part_item"] else "", "+" if r["conv3_wgrad"]["two_stage"] else "",
                                 r["conv3_dgrad"]["items"], "*" if r["conv3_dgrad"]["part_item"] else "",
                                 r["conv2_wgrad"]["items"], "+" if r["conv2_wgrad"]["two_stage"] else "",
                                 r["conv2_dgrad"]["items"], r["conv1_wgrad"]["items"]))
    return rows


# ---- seeded inputs (frames, loss inputs and weight seeds are few_env_cases') ------------------------
def _rng(*key):
    return np.random.RandomState([20250927] + [int(k) for k in key])


def arena_rows(hw, n):
    """(arena uint8 [R, H, W, 3], image rows int32 [n], goal rows int32 [n]) with R = max(6, 3n / 4)
    rows for 2n frames, so rows repeat within and between the two lists; the last arena row is
    used by the last sample's goal, row 0 by sample 0's image."""
    R = max(6, 3 * n // 4)
    rng = _rng(1, hw[0], hw[1], n)
    arena = rng.randint(0, 256, size=(R,) + tuple(hw) + (3,)).astype(np.uint8)
    ri = rng.randint(0, R, size=n).astype(np.int32)
    rg = rng.randint(0, R, size=n).astype(np.int32)
    ri[0], rg[n - 1] = 0, R - 1
    return arena, ri, rg
