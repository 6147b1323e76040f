"""Case tables of the aux deconv head regime tests and the launch rules they rest on (TEST
INFRASTRUCTURE ONLY — see oracle/__init__.py).

aux_forward_impl / aux_forward_loss_impl / aux_backward_impl (csrc/vn_policy.hip) and the kernels
of csrc/vn_aux.h choose their work split from the frame geometry (constexpr) and the sample count
n: samples per item and bands per sample, persistent grids min(items, resident workgroups), the
512 cap of the second layer's backward with its finish kernel (64 lanes over the partials), the
packed items of the first layer's weight gradient with launch_conv_wgrad_x6's two-stage reduce
from 64 slabs. This module restates those rules with the constants as they stand in the source
and gives, per (geometry, n), the regime of each kernel; tests/test_aux_head_cases.py checks on
the CPU that the table below holds a case on each side of every switch and that the checks see
planted faults, tests/test_aux_head_regimes_gpu.py runs the cases against float64.

resident_blocks is an occupancy query at run time. wg_bound restates an upper bound: per CU at
most min(2048 / threads, floor(160 KiB / LDS bytes)) workgroups. The second argument of
__launch_bounds__ is left out of it: it is the occupancy the compiler must make possible (a cap on
registers), not a ceiling, and a kernel that needs fewer registers runs more workgroups than it
asks for. A case whose items exceed the bound has a workgroup on its second item whatever the
query returns; a case whose items do not exceed the CU count runs one item per workgroup (the
query returns at least 1 per CU).

numpy only at import; reference() and the inputs' consumers import torch when called.
"""
import numpy as np

from .few_env_cases import GEO_IDS
from .policy import trunk_sizes

GEOMETRIES = ((84, 84), (174, 174), (300, 400))
CUS = 256          # the CU count the tables are computed for (MI355X); the GPU test asserts <=
MIN_CUS = 65       # ... and >=: 65 partials / 64 slabs need that many resident workgroups

# ---- constants of csrc/vn_aux.h / csrc/vn_policy.hip -----------------------------------------
AUX_C1, AUX_C2, AUX_CELL = 48, 8, 4       # kAuxC1, kAuxC2, kAuxCell
AUX_LOSS_BLOCKS = 2048                    # kAuxLossBlocks (x 256 threads)
AUX2_THREADS, AUX2_PST, AUX2_PX = 512, 52, 4   # kAux2Threads, kAux2Pst, kAux2Px
AUX2_WFL = 4 * 4 * AUX_C1 * AUX_C2        # kAux2Wfl
AUX2_STAGE = 96 * 1024                    # aux2_spi: staging budget of the whole-map form
AUX2_SPI_MAX = 8
AUX2_BAND_STAGE = 150 * 1024              # aux2_byc: LDS of a band
AUX2_BAND_PRE = 11                        # ... and its prefetch registers (f4 per thread)
AUXB_THREADS, AUXB_DS = 512, 9            # kAuxBThreads, kAuxBDs
AUXB_PART = 7 * 4 * 64 + AUX_C1 + AUX_C2  # kAuxBPart
AUXB_STAGE = 80 * 1024                    # auxb_fits / auxb_bya
AUXB_RED = 7 * 4 * 64 * 4 + 64 * 4        # ... and the reduction area they must hold
COLSUM_BLOCKS = 512                       # kColsumBlocks: the backward's grid cap
FINISH_LANES = 64                         # aux_backward2_finish_kernel: lanes over the partials
DX4_PP, DX4_TG = 36, 2                    # AuxDx4::PP, TG
WG_PARTS = 32                             # launch_conv_wgrad_x6: kParts; two stages from 2 kParts slabs
LDS_CU = 160 * 1024
THREADS_CU = 2048


def _cdiv(a, b):
    return (a + b - 1) // b


def maps(hw):
    """(IH, IW), (AH, AW), (PH, PW): conv_base's map, the first and the second deconv's output."""
    ih, iw = trunk_sizes(*hw)[2]
    ah, aw = 2 * ih + 2, 2 * iw + 2
    return (ih, iw), (ah, aw), (2 * ah + 2, 2 * aw + 2)


# ---- second layer forward: aux_deconv2_kernel / aux_deconv2_band_kernel ------------------------
def aux2_spi(ah, aw):
    per = (ah * aw + 1) * AUX2_PST * 4
    return min(AUX2_STAGE // per, AUX2_SPI_MAX) if per * 2 <= AUX2_STAGE else 1


def aux2_lds(ah, aw):
    return aux2_spi(ah, aw) * (ah * aw + 1) * AUX2_PST * 4 + AUX2_WFL * 4


def aux2_fits(ah, aw):
    return aux2_lds(ah, aw) <= LDS_CU


def aux2b_lds(aw, byc):
    return ((byc + 1) * aw + 1) * AUX2_PST * 4 + AUX2_WFL * 4


def aux2_byc(aw, pw):
    xb = _cdiv(pw // 2, AUX2_PX)
    b = 128 // xb
    while b > 0 and (aux2b_lds(aw, b) > AUX2_BAND_STAGE or _cdiv((b + 1) * aw * 12, AUX2_THREADS) > AUX2_BAND_PRE):
        b -= 1
    return b


# ---- second layer backward: aux_backward2_kernel -------------------------------------------------
def auxb_lds(ph, pw):
    return ph * pw * AUXB_DS * 4


def auxb_fits(ah, aw, ph, pw):
    return (ah * aw) % 16 == 0 and AUXB_RED <= auxb_lds(ph, pw) <= AUXB_STAGE


def auxb_band_lds(pw, bya):
    return (2 * bya + 2) * pw * AUXB_DS * 4


def auxb_bya(ah, aw, pw):
    for b in range(ah, 0, -1):
        if (b * aw) % 128 == 0 and AUXB_RED <= auxb_band_lds(pw, b) <= AUXB_STAGE:
            return b
    return 0


# ---- dX4: AuxDx4 -----------------------------------------------------------------------------------
def dx4_lds(iw, by):
    tp = _cdiv(by * (iw + 1), 16) * 16
    return 12 * (tp + iw + 2) * AUX_C1 * 2 + 2 * DX4_TG * 4 * 16 * DX4_PP * 4


def dx4_by(ih, iw):
    by = ih
    while by > 1 and dx4_lds(iw, by) > LDS_CU:
        by -= 1
    return by


# ---- first layer forward: ParityDg<IH, IW, IH + 1, IW + 1, 32, 48, 1> ---------------------------
def parity_rows(npc, xc, img):
    return _cdiv(img * npc, 16) * 16 + xc + 1


def parity_img(ih, iw):
    npc, xc = (ih + 1) * (iw + 1), iw + 1
    if npc >= 64:
        return 2 if 3 * parity_rows(npc, xc, 2) * 32 * 2 <= LDS_CU else 1
    return 64 // npc


def parity_lds(ih, iw):
    return 3 * parity_rows((ih + 1) * (iw + 1), iw + 1, parity_img(ih, iw)) * 32 * 2


# ---- first layer weight gradient: the Wa instance of WgSpec ------------------------------------
def wa_lds(ah, aw, ih, iw, br, img):
    xr = min(2 * br + 2, ah)
    kp = img * br * iw
    pz, px = 32 + 8, AUX_C1 + 8      # CX = 48: the plain k order
    return 3 * ((kp + 1) * pz + (img * xr * aw + 1) * px) * 2


def wa_spec(ah, aw, ih, iw):
    """(BR, IMG, NB, LDS) of Wa: whole maps packed to >= 32 reduction pixels an item, else bands
    of one X4 row, two images per item."""
    img = 1 if ih * iw >= 32 else 32 // (ih * iw)
    if wa_lds(ah, aw, ih, iw, ih, img) <= LDS_CU:
        return ih, img, 1, wa_lds(ah, aw, ih, iw, ih, img)
    return 1, 2, ih, wa_lds(ah, aw, ih, iw, 1, 2)


def wg_bound(threads, lds, cus=CUS, cap=None):
    """Upper bound on the workgroups of a persistent launch (see the module docstring)."""
    b = max(1, min(THREADS_CU // threads, LDS_CU // lds if lds else THREADS_CU)) * cus
    return min(b, cap) if cap else b


def geometry(hw):
    """Everything of a geometry that does not depend on n."""
    (ih, iw), (ah, aw), (ph, pw) = maps(hw)
    g = {"IH": ih, "IW": iw, "AH": ah, "AW": aw, "PH": ph, "PW": pw}
    g["fwd2_whole"] = aux2_fits(ah, aw)
    if g["fwd2_whole"]:
        g["fwd2_spi"], g["fwd2_bands"], g["fwd2_byc"], g["fwd2_lds"] = aux2_spi(ah, aw), 1, 0, aux2_lds(ah, aw)
    else:
        byc = aux2_byc(aw, pw)
        assert byc > 0, "no banded form: the generic products would run"
        g["fwd2_spi"], g["fwd2_bands"], g["fwd2_byc"], g["fwd2_lds"] = 1, _cdiv(ph // 2, byc), byc, aux2b_lds(aw, byc)
    if auxb_fits(ah, aw, ph, pw):
        g["bwd2_bya"], g["bwd2_bands"], g["bwd2_last"], g["bwd2_lds"] = ah, 1, ah, auxb_lds(ph, pw)
    else:
        bya = auxb_bya(ah, aw, pw)
        assert bya > 0, "no banded form: the generic products would run"
        nb = _cdiv(ah, bya)
        g["bwd2_bya"], g["bwd2_bands"], g["bwd2_last"], g["bwd2_lds"] = bya, nb, ah - (nb - 1) * bya, auxb_band_lds(pw, bya)
    by = dx4_by(ih, iw)
    g["dx4_by"], g["dx4_bands"], g["dx4_lds"] = by, _cdiv(ih, by), dx4_lds(iw, by)
    assert g["dx4_lds"] <= LDS_CU
    g["l1_img"], g["l1_lds"] = parity_img(ih, iw), parity_lds(ih, iw)
    assert g["l1_lds"] <= LDS_CU
    g["wa_br"], g["wa_img"], g["wa_bands"], g["wa_lds"] = wa_spec(ah, aw, ih, iw)
    assert g["wa_lds"] <= LDS_CU and ih % g["wa_br"] == 0
    return g


def _persistent(items, bound, cus):
    return {"items": items, "bound": bound, "second_pass": items > bound, "one_pass": items <= min(cus, MIN_CUS)}


def aux_regime(hw, n, cus=CUS):
    """Per kernel: items, the upper bound on workgroups, whether a second pass is certain
    (second_pass) or impossible (one_pass: items within the fewest resident workgroups), the tail
    of the last item; for the backward the bound on the partials the finish kernel sums and their
    count per lane; for the first layer's weight gradient the slab bound and the reduce form."""
    g = geometry(hw)
    r = {}
    k = _persistent(_cdiv(n, g["l1_img"]), wg_bound(256, g["l1_lds"], cus), cus)
    k["tail"] = n % g["l1_img"] or g["l1_img"]
    r["layer1"] = k
    k = _persistent(_cdiv(n, g["fwd2_spi"]) * g["fwd2_bands"], wg_bound(AUX2_THREADS, g["fwd2_lds"], cus), cus)
    k["tail"] = n % g["fwd2_spi"] or g["fwd2_spi"]
    r["fwd2"] = k
    total = n * g["PH"] * g["PW"]
    blocks = min(AUX_LOSS_BLOCKS, _cdiv(total, 256))
    r["loss"] = {"items": _cdiv(total, 256), "bound": AUX_LOSS_BLOCKS, "second_pass": total > blocks * 256,
                 "one_pass": total <= blocks * 256}
    k = _persistent(n * g["bwd2_bands"], wg_bound(AUXB_THREADS, g["bwd2_lds"], cus, COLSUM_BLOCKS), cus)
    k["partials"] = min(k["items"], k["bound"])            # = the count itself while items <= MIN_CUS
    k["per_lane"] = _cdiv(k["partials"], FINISH_LANES)
    r["bwd2"] = k
    k = _persistent(_cdiv(n, g["wa_img"]) * g["wa_bands"], wg_bound(512, g["wa_lds"], cus), cus)
    k["tail"] = n % g["wa_img"] or g["wa_img"]
    k["slabs"] = min(k["items"], k["bound"])
    # bx >= 2 kParts: every device of MIN_CUS or more CUs holds 64 workgroups
    k["reduce"] = "two-stage" if k["items"] >= 2 * WG_PARTS else "one-stage"
    r["dw1"] = k
    r["dx4"] = _persistent(n * g["dx4_bands"], wg_bound(512, g["dx4_lds"], cus), cus)
    return r


# ---- the cases ----------------------------------------------------------------------------------
# per geometry: every n named by a switch of SWITCHES, nothing else
CASE_N = {
    (84, 84): (1, 6, 7, 8, 9, 64, 65, 189, 190, 512, 513, 1536, 1537, 1792, 1797),
    (174, 174): (1, 63, 64, 65, 256, 257, 512, 513),
    (300, 400): (1, 2, 3, 6, 7, 12, 13, 30, 31, 42, 43, 51, 52, 102, 103),
}
CASES = [(hw, n) for hw in GEOMETRIES for n in CASE_N[hw]]

# (geometry, what switches, kernel, key, the first n past the switch): the cases at - 1 and at
# stand in CASE_N. key "second_pass": at - 1 is the last n whose items fit the bound.
SWITCHES = (
    ((84, 84), "one sample -> more", "fwd2", "n>1", 2),
    ((84, 84), "forward: a ragged item of 6 -> a whole one of SPI = 7", "fwd2", "tail", 7),
    ((84, 84), "forward: one item -> a second, of one sample", "fwd2", "items", 8),
    ((84, 84), "weight gradient: items of IMG = 3 whole (6) -> a ragged third (7)", "dw1", "tail", 7),
    ((84, 84), "weight gradient: a ragged item of 2 (8) -> whole items (9)", "dw1", "tail", 9),
    ((84, 84), "finish kernel: one partial a lane -> a second on lane 0", "bwd2", "per_lane", 65),
    ((84, 84), "weight gradient: 63 slabs in one stage -> 64 in two", "dw1", "reduce", 190),
    ((84, 84), "backward and dX4: the 512 workgroup cap, a second item", "bwd2", "second_pass", 513),
    ((84, 84), "dX4: a second item", "dx4", "second_pass", 513),
    ((84, 84), "forward: a second item per workgroup (1797: 257 items, the last of 5)", "fwd2", "second_pass", 1793),
    ((84, 84), "loss kernel alone: grid-stride past 2048 x 256 pixels", "loss", "second_pass", 1619),
    ((84, 84), "weight gradient: a second item per workgroup (513 items of 3)", "dw1", "second_pass", 1537),
    ((174, 174), "one sample -> more", "fwd2", "n>1", 2),
    ((174, 174), "weight gradient: 63 slabs in one stage -> 64 in two", "dw1", "reduce", 64),
    ((174, 174), "finish kernel: one partial a lane -> a second on lane 0", "bwd2", "per_lane", 65),
    ((174, 174), "forward: a second item per workgroup", "fwd2", "second_pass", 257),
    ((174, 174), "dX4: a second item per workgroup", "dx4", "second_pass", 257),
    ((174, 174), "weight gradient: a second item per workgroup", "dw1", "second_pass", 257),
    ((174, 174), "loss kernel alone: grid-stride", "loss", "second_pass", 298),
    ((174, 174), "backward: the 512 workgroup cap, a second item", "bwd2", "second_pass", 513),
    ((300, 400), "one sample -> more", "fwd2", "n>1", 2),
    ((300, 400), "weight gradient: half an item of IMG = 2 -> whole", "dw1", "tail", 2),
    ((300, 400), "weight gradient: whole -> half an item", "dw1", "tail", 3),
    ((300, 400), "weight gradient: 51 slabs in one stage -> 68 in two", "dw1", "reduce", 7),
    ((300, 400), "finish kernel: 60 partials -> 65, a second on lane 0", "bwd2", "per_lane", 13),
    ((300, 400), "weight gradient: a second item per workgroup (17 bands x 16 pairs)", "dw1", "second_pass", 31),
    ((300, 400), "dX4 (6 bands a sample): a second item per workgroup", "dx4", "second_pass", 43),
    ((300, 400), "forward (5 bands a sample): a second item per workgroup", "fwd2", "second_pass", 52),
    ((300, 400), "loss kernel alone: grid-stride", "loss", "second_pass", 73),
    ((300, 400), "backward (5 bands a sample): the 512 workgroup cap, a second item", "bwd2", "second_pass", 103),
)
# the forward's second pass at 84x84 runs at 1797 = 256 x 7 + 5: the last item ragged as well
ABOVE = {((84, 84), "fwd2", "second_pass", 1793): 1797}
# switches whose two sides need not be the nearest n: vn_aux_loss_grad's grid-stride loop is one
# thread a pixel with no state carried between passes, and its switch falls between cases that
# other kernels place; a case on each side is held
LOOSE = {((84, 84), "loss"), ((174, 174), "loss"), ((300, 400), "loss")}

CAPACITY_N = {(84, 84): 9, (174, 174): 65, (300, 400): 7}       # act_capacity = n + 3
GENERIC_N = {(84, 84): 190, (174, 174): 65, (300, 400): 13}     # the VN_*_GENERIC forms
REPEAT_N = {(84, 84): (1, 513), (174, 174): (1, 257), (300, 400): (1, 31)}  # bitwise repeatable
BITS_HW = (174, 174)       # the bit test of the reduce forms: one sample an item in every kernel
BITS_N = (63, 64, 65)
WEIGHT = 0.1


def regime_value(hw, n, kernel, key):
    if key == "n>1":
        return n > 1
    return aux_regime(hw, n)[kernel][key]


def uncovered(cases=CASE_N):
    """The switches that the case lists leave without a side: at - 1 and at (or the n a switch
    names in its place) are cases with nothing between them; a LOOSE switch holds some case in
    the regime of either side."""
    out = []
    for hw, what, kernel, key, at in SWITCHES:
        ns = sorted(cases[hw])
        lo_v, hi_v = regime_value(hw, at - 1, kernel, key), regime_value(hw, at, kernel, key)
        below, above = [n for n in ns if n < at], [n for n in ns if n >= at]
        ok = lo_v != hi_v and bool(below) and bool(above)
        if ok and key == "n>1":
            ok = below[-1] == 1
        elif ok and (hw, kernel) in LOOSE and key == "second_pass":
            ok = regime_value(hw, below[-1], kernel, key) == lo_v and regime_value(hw, above[0], kernel, key) == hi_v
        elif ok:
            ok = below[-1] == at - 1 and above[0] == ABOVE.get((hw, kernel, key, at), at) and \
                regime_value(hw, above[0], kernel, key) == hi_v
        if not ok:
            out.append((GEO_IDS[hw], what))
    return out


def case_id(c):
    return "%s-n%d" % (GEO_IDS[c[0]], c[1])


def regime_table():
    """The regimes of the cases as text rows: items / bound per kernel, * where a second pass is certain."""
    rows = []
    for hw, n in CASES:
        r = aux_regime(hw, n)

        def f(k):
            return "%d/%d%s" % (r[k]["items"], r[k]["bound"], "*" if r[k]["second_pass"] else "")
        rows.append("%-8s n=%-4d layer1 %s (tail %d)  fwd2 %s (tail %d)  loss %s  bwd2 %s (partials <= %d, %d a lane)  "
                    "dW1 %s (tail %d, %s)  dX4 %s" % (GEO_IDS[hw], n, f("layer1"), r["layer1"]["tail"], f("fwd2"),
                                                      r["fwd2"]["tail"], f("loss"), f("bwd2"), r["bwd2"]["partials"],
                                                      r["bwd2"]["per_lane"], f("dw1"), r["dw1"]["tail"],
                                                      r["dw1"]["reduce"], f("dx4")))
    return rows


# ---- seeded inputs ------------------------------------------------------------------------------
HEADS = (("deconv_depth", 1, 0), ("deconv_mask", 3, 1), ("deconv_mask_goal", 3, 4))  # name, C, first channel


def _rng(*key):
    return np.random.RandomState([20250917] + [int(k) for k in key])


def table_rows(n):
    """R of the target table: != n, and small enough that rows repeat."""
    R = n // 2 + 2
    return R + 1 if R == n else R


def inputs(hw, n):
    """x4 float32 [n, IH, IW, 32] (NHWC) >= 0 with about half zeros, as behind a ReLU; table
    float32 [R, PH, PW, 4] in [0, 1) (depth, seg 0..2); image_rows, goal_rows int32 [n] out of
    order with repeats, image_rows[i] != goal_rows[i] for every i."""
    (ih, iw), _, (ph, pw) = maps(hw)
    rng = _rng(1, hw[0], hw[1], n)
    x4 = np.maximum(rng.standard_normal((n, ih, iw, 32)), 0.0).astype(np.float32)
    R = table_rows(n)
    table = rng.random_sample((R, ph, pw, 4)).astype(np.float32)
    image_rows = rng.randint(0, R, size=n).astype(np.int32)
    image_rows[-1] = R - 1                                     # the table's last row is read
    goal_rows = ((image_rows + 1 + rng.randint(0, R - 1, size=n)) % R).astype(np.int32)
    return {"x4": x4, "table": table, "image_rows": image_rows, "goal_rows": goal_rows}


def seeded_state(hw, seed=5):
    """The heads' parameters by reference name, float32: init_weights' distributions (U(+-1 /
    sqrt(fan_in)), ConvTranspose2d's fan_in = out channels x 16) with the biases moved off zero
    (U(+-0.05)). For the CPU tests: the GPU test takes PolicyNet.init_params."""
    rng = _rng(2, hw[0], hw[1], seed)
    sd = {}
    for name, c, _ in HEADS:
        for i, shape, d in ((1, (32, 16, 4, 4), 1.0 / 16.0), (3, (16, c, 4, 4), 1.0 / np.sqrt(16.0 * c))):
            sd["%s.0.%d.weight" % (name, i)] = rng.uniform(-d, d, size=shape).astype(np.float32)
            sd["%s.0.%d.bias" % (name, i)] = rng.uniform(-0.05, 0.05, size=shape[1]).astype(np.float32)
    return sd


PARAM_NAMES = tuple("%s.0.%d.%s" % (name, i, kind) for name, _, _ in HEADS for i in (1, 3)
                    for kind in ("weight", "bias"))


# ---- the float64 (or float32) restatement of the heads, their loss and their backward -----------
def forward(sd, inp, masks=None, dtype=None):
    """The heads on inp["x4"]: {"pre": [3 x (n, 16, AH, AW)], "a1" [n, AH, AW, 48] (after the
    ReLU, or under the given 0/1 masks [3 x (n, 16, AH, AW)]), "pred" [n, PH, PW, 8] (channel 7 = 0)}
    as tensors of dtype (float64), with the graph kept for backward()."""
    import torch
    import torch.nn.functional as F
    dtype = dtype or torch.float64
    P = {k: torch.as_tensor(np.asarray(v)).to(dtype).requires_grad_() for k, v in sd.items() if k in PARAM_NAMES}
    x = torch.as_tensor(inp["x4"]).to(dtype).permute(0, 3, 1, 2).contiguous().requires_grad_()
    pre, act, out = [], [], []
    for h, (name, c, _) in enumerate(HEADS):
        z = F.conv_transpose2d(x, P[name + ".0.1.weight"], P[name + ".0.1.bias"], stride=2)
        m = (z.detach() > 0).to(dtype) if masks is None else torch.as_tensor(masks[h]).to(dtype)
        a = z * m
        a.retain_grad()
        pre.append(z)
        act.append(a)
        out.append(F.conv_transpose2d(a, P[name + ".0.3.weight"], P[name + ".0.3.bias"], stride=2))
    n, _, ph, pw = out[0].shape
    pred = torch.cat(out + [torch.zeros((n, 1, ph, pw), dtype=dtype)], dim=1).permute(0, 2, 3, 1)
    return {"params": P, "x": x, "pre": pre, "act": act, "pred": pred,
            "a1": torch.cat([a.detach() for a in act], dim=1).permute(0, 2, 3, 1)}


def targets(inp, goal_from=None):
    """[n, PH, PW, 8] float64: depth, seg of the image row, seg of the goal row, 0."""
    t = inp["table"].astype(np.float64)
    ti, tg = t[inp["image_rows"]], t[inp["goal_rows"] if goal_from is None else inp[goal_from]]
    return np.concatenate([ti, tg[..., 1:], np.zeros_like(ti[..., :1])], axis=-1)


def loss_grad(pred, inp, weight=WEIGHT, goal_from=None):
    """(dpred [n, PH, PW, 8], stats [3]) of the per-head MSE x weight: dP = weight 2 (P - t) /
    numel(head), stats[h] = sum (P - t)^2, in the dtype of pred (numpy)."""
    pred = np.asarray(pred)
    d = pred - targets(inp, goal_from).astype(pred.dtype)
    d[..., 7] = 0
    n, ph, pw, _ = d.shape
    dp = np.zeros_like(d)
    stats = np.zeros(3, dtype=pred.dtype)
    for h, (_, c, o) in enumerate(HEADS):
        dp[..., o:o + c] = d[..., o:o + c] * pred.dtype.type(2.0 * weight / (c * n * ph * pw))
        stats[h] = (d[..., o:o + c] ** 2).sum(dtype=pred.dtype)
    return dp, stats


def backward(fwd, dpred, samples=None):
    """Gradients of sum(pred x dpred) (dpred [n, PH, PW, 8] given, as aux_backward takes it): {"dx4"
    [n, IH, IW, 32], "da1" [n, AH, AW, 48] (under the masks), reference parameter names}. samples:
    a 0/1 vector [n]: the parameter gradients sum over those samples only."""
    import torch
    dp = torch.as_tensor(np.asarray(dpred)).to(fwd["pred"].dtype)
    if samples is not None:
        dp = dp * torch.as_tensor(np.asarray(samples)).to(dp.dtype).view(-1, 1, 1, 1)
    names = list(fwd["params"])
    for t in [fwd["x"]] + fwd["act"] + [fwd["params"][k] for k in names]:
        t.grad = None
    (fwd["pred"] * dp).sum().backward(retain_graph=True)
    out = {k: fwd["params"][k].grad.numpy().copy() for k in names}
    out["dx4"] = fwd["x"].grad.permute(0, 2, 3, 1).numpy().copy()
    da = [a.grad * (a.detach() != 0).to(a.dtype) for a in fwd["act"]]
    out["da1"] = torch.cat(da, dim=1).permute(0, 2, 3, 1).numpy().copy()
    return out


def reference(sd, inp, masks=None, weight=WEIGHT, dtype=None):
    """forward + loss_grad + backward: everything the GPU test compares, as numpy arrays."""
    fwd = forward(sd, inp, masks, dtype)
    pred = fwd["pred"].detach().numpy()
    dpred, stats = loss_grad(pred, inp, weight)
    out = backward(fwd, dpred)
    out.update(pred=pred, dpred=dpred, stats=stats, a1=fwd["a1"].numpy(), pre=[z.detach().numpy() for z in fwd["pre"]])
    return out


# ---- the checks (shared by the GPU test and the CPU test of their sensitivity) -------------------
TOL = {"pred": 1e-5, "dpred": 1e-5, "dpred_fused": 1e-5, "stats": 1e-5, "stats_fused": 1e-5, "dx4": 1e-4}
TOL.update({k: 1e-4 for k in PARAM_NAMES})


def err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def errors(got, ref):
    """{tensor: error}: of the tensor's scale (stats: relative, per head) for every tensor of TOL
    that got holds; the fused forms are compared with the reference's dpred / stats."""
    out = {}
    for k in TOL:
        if k not in got:
            continue
        want = ref[k.replace("_fused", "")]
        if k.startswith("stats"):
            g, w = np.asarray(got[k], dtype=np.float64)[:3], np.asarray(want, dtype=np.float64)
            out[k] = float(np.abs(g / w - 1.0).max())
        else:
            out[k] = err(got[k], want)
    return out


def misses(errs):
    return {k: "%.3g" % e for k, e in errs.items() if not e <= TOL[k]}
