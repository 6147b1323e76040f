"""The conditions the cases of tests/test_aux_head_regimes_gpu.py rest on, checked on the CPU
from the launch rules restated in oracle/aux_head_cases.py: the restated constants stand in the
source as restated, every switch has a case on each side, every "second pass" claim holds under
the upper bound on resident workgroups, and the checks of the GPU test see each of seven planted
faults by at least ten times their tolerance on the case built for it (a float64 restatement of
the heads with one fault at a time). A changed threshold fails here and names the case to move."""
import os
import re

import numpy as np
import pytest

from oracle import aux_head_cases as ac
from oracle.few_env_cases import GEO_IDS

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "a2cat-vn-pytorch_amd", "csrc")
G84, G174, G300 = ac.GEOMETRIES


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return re.sub(r"\s+", " ", f.read())


def test_tables_hold_what_the_issue_sets():
    issue = {G84: (1, 6, 7, 8, 9, 64, 65, 189, 190, 512, 513, 1792, 1797),
             G174: (1, 63, 64, 65, 256, 257, 512, 513),
             G300: (1, 2, 3, 42, 43, 51, 52, 102, 103)}
    for hw, ns in issue.items():
        assert set(ns) <= set(ac.CASE_N[hw]), GEO_IDS[hw]
        assert list(ac.CASE_N[hw]) == sorted(set(ac.CASE_N[hw]))
    # the restated rules add, at 300x400: 6 / 7 (51 -> 68 weight-gradient slabs: the two-stage
    # reduce), 12 / 13 (60 -> 65 partials: the finish kernel's second round), 30 / 31 (the weight
    # gradient's second pass: 17 bands x 16 pairs = 272 items)
    assert set(ac.CASE_N[G300]) - set(issue[G300]) == {6, 7, 12, 13, 30, 31}
    # and at 84x84 1536 / 1537 (the weight gradient's second pass: 513 items of 3 samples)
    assert set(ac.CASE_N[G84]) - set(issue[G84]) == {1536, 1537} and ac.CASE_N[G174] == issue[G174]
    ids = [ac.case_id(c) for c in ac.CASES]
    assert len(ids) == len(set(ids)) == sum(len(v) for v in ac.CASE_N.values())
    for hw in ac.GEOMETRIES:
        ns = ac.CASE_N[hw]
        assert ac.CAPACITY_N[hw] in ns and ac.GENERIC_N[hw] in ns and set(ac.REPEAT_N[hw]) <= set(ns)
        first = ac.REPEAT_N[hw][1]   # the geometry's first size with a certain second pass
        assert [n for n in ns if any(k["second_pass"] for k in ac.aux_regime(hw, n).values())][0] == first
    assert set(ac.BITS_N) <= set(ac.CASE_N[ac.BITS_HW]) and ac.WEIGHT == 0.1
    assert len(ac.regime_table()) == len(ac.CASES)


def test_restated_geometry():
    """The per-geometry constants the issue names, from the restated constexpr functions."""
    g = {hw: ac.geometry(hw) for hw in ac.GEOMETRIES}
    assert [(v["IH"], v["IW"], v["AH"], v["AW"], v["PH"], v["PW"]) for v in g.values()] == \
        [(3, 3, 8, 8, 18, 18), (9, 9, 20, 20, 42, 42), (17, 23, 36, 48, 74, 98)]
    assert [(v["fwd2_whole"], v["fwd2_spi"], v["fwd2_byc"], v["fwd2_bands"]) for v in g.values()] == \
        [(True, 7, 0, 1), (True, 1, 0, 1), (False, 1, 8, 5)]
    assert [(v["bwd2_bya"], v["bwd2_bands"], v["bwd2_last"]) for v in g.values()] == [(8, 1, 8), (20, 1, 20), (8, 5, 4)]
    assert [(v["dx4_by"], v["dx4_bands"]) for v in g.values()] == [(3, 1), (9, 1), (3, 6)]
    assert [v["l1_img"] for v in g.values()] == [4, 2, 1]
    assert [(v["wa_img"], v["wa_bands"]) for v in g.values()] == [(3, 1), (1, 1), (2, 17)]
    # each kernel's LDS bytes
    assert [v["fwd2_lds"] for v in g.values()] == [119216, 107984, 114640]
    assert [v["bwd2_lds"] for v in g.values()] == [11664, 63504, 63504]
    assert [v["dx4_lds"] for v in g.values()] == [61056, 160128, 157824]
    assert [v["l1_lds"] for v in g.values()] == [13248, 42048, 87744]
    assert [v["wa_lds"] for v in g.values()] == [71568, 154416, 140640]
    assert all(v[k] <= ac.LDS_CU for v in g.values() for k in v if k.endswith("_lds"))
    assert ac.AUXB_PART == 1848 and ac.COLSUM_BLOCKS == 512


def test_restated_constants_stand_in_the_source():
    aux, pol = _source("vn_aux.h"), _source("vn_policy.hip")
    for text in ("constexpr int kAuxC1 = %d;" % ac.AUX_C1, "constexpr int kAuxC2 = %d;" % ac.AUX_C2,
                 "constexpr int kAuxCell = %d;" % ac.AUX_CELL, "constexpr int kAuxLossBlocks = %d;" % ac.AUX_LOSS_BLOCKS,
                 "constexpr int kAux2Threads = %d;" % ac.AUX2_THREADS, "constexpr int kAux2Pst = %d;" % ac.AUX2_PST,
                 "constexpr int kAux2Px = %d;" % ac.AUX2_PX, "constexpr int kAux2Wfl = 4 * 4 * kAuxC1 * kAuxC2;",
                 "constexpr int per = (AH * AW + 1) * kAux2Pst * 4;",
                 "return per * 2 <= 96 * 1024 ? (96 * 1024 / per < 8 ? 96 * 1024 / per : 8) : 1;",
                 "return (size_t)aux2_spi<AH, AW>() * (AH * AW + 1) * kAux2Pst * 4 + kAux2Wfl * 4;",
                 "return aux2_lds<AH, AW>() <= 160 * 1024;",
                 "return (size_t)((byc + 1) * aw + 1) * kAux2Pst * 4 + kAux2Wfl * 4; }",
                 "int b = 128 / XB;",
                 "(aux2b_lds(AW, b) > 150 * 1024 || ((b + 1) * AW * 12 + kAux2Threads - 1) / kAux2Threads > 11)",
                 "constexpr int kAuxBThreads = %d;" % ac.AUXB_THREADS, "constexpr int kAuxBDs = %d;" % ac.AUXB_DS,
                 "constexpr int kAuxBPart = 7 * 4 * 64 + kAuxC1 + kAuxC2;",
                 "return (size_t)PH * PW * kAuxBDs * 4;",
                 "return (AH * AW) % 16 == 0 && auxb_lds<PH, PW>() <= 80 * 1024 && auxb_lds<PH, PW>() >= 7 * 4 * 64 * 4 + 64 * 4;",
                 "return (size_t)(2 * bya + 2) * pw * kAuxBDs * 4; }",
                 "if ((b * AW) % 128 == 0 && auxb_band_lds(PW, b) <= 80 * 1024 && auxb_band_lds(PW, b) >= 7 * 4 * 64 * 4 + 64 * 4)",
                 "__launch_bounds__(kAux2Threads) void aux_deconv2_kernel", "__launch_bounds__(kAux2Threads) void aux_deconv2_band_kernel",
                 "__launch_bounds__(kAuxBThreads, 4) void aux_backward2_kernel",
                 "for (int b = lane; b < nblk; b += 64) s += part[(int64_t)b * kAuxBPart + src];",
                 "for (int s0 = blockIdx.x * SPI; s0 < n; s0 += gridDim.x * SPI)",
                 "const int NPPC = (y0 + rows == AH ? 2 * rows + 2 : 2 * rows) * PW;"):
        assert text in aux, text
    for text in ("constexpr int kColsumBlocks = %d;" % ac.COLSUM_BLOCKS, "constexpr int kParts = %d;" % ac.WG_PARTS,
                 "if (bx >= 2 * kParts) {", "const int items = (n + S::IMG - 1) / S::IMG * S::NB;",
                 "int bx = std::max(1, std::min(items, resident_blocks(kfn, 512, S::LDS) / S::G));",
                 "static constexpr int PP = %d;" % ac.DX4_PP, "static constexpr int TG = %d;" % ac.DX4_TG,
                 "static constexpr int tp_of(int by) { return (by * XC + 15) / 16 * 16; }",
                 "static constexpr int nr_of(int by) { return tp_of(by) + XC + 1; }",
                 "return (size_t)12 * nr_of(by) * C * 2 + (size_t)2 * TG * 4 * 16 * PP * 4; }",
                 "while (by > 1 && lds_of(by) > 160 * 1024) --by;",
                 "static constexpr int rows(int img) { return (img * NPC + 15) / 16 * 16 + XC + 1; }",
                 "static constexpr int IMG = NPC >= 64 ? ((size_t)3 * rows(2) * KC * 2 <= 160 * 1024 ? 2 : 1) : 64 / NPC;",
                 "static constexpr size_t LDS = (size_t)3 * NR * KC * 2;", "static constexpr int NT = 256 * WPC;",
                 "static constexpr int XR = 2 * BR + 2 < IH ? 2 * BR + 2 : IH;", "static constexpr int KP = IMG * BR * OW",
                 "static constexpr int PZ = CO + (KPERM ? 16 : 8), PX = CX + 8;",
                 "static constexpr int RZ = KP + 1, RX = IMG * NPX + 1;",
                 "static constexpr size_t LDS = (size_t)3 * (RZ * PZ + RX * PX) * 2;",
                 "using WaWhole = WgSpec<AH, AW, IH, IW, 32, 1, IH, (IH * IW >= 32 ? 1 : 32 / (IH * IW)), kAuxC1, false>;",
                 "WgSpec<AH, AW, IH, IW, 32, 1, 1, 2, kAuxC1, false>>;",
                 "using S = ParityDg<IH, IW, OH / 2, OW / 2, 32, kPc ? 64 : 48, kPc ? 2 : 1>;",
                 "const int blocks = std::min((n + SPI - 1) / SPI, resident_blocks(kfn, kAux2Threads, lds));",
                 "const int items = n * ((PH / 2 + BYC - 1) / BYC);",
                 "const int blocks = std::min(n, std::min(resident_blocks(kfn, kAuxBThreads, lds), kColsumBlocks));",
                 "const int items = n * ((AH + BYA - 1) / BYA);",
                 "const int blocks = std::min(items, std::min(resident_blocks(kfn, kAuxBThreads, lds), kColsumBlocks));",
                 "const int blocks = std::min(n * Dx::NB, resident_blocks(kfn, 512, Dx::LDS));",
                 "const int blocks = std::min(items, resident_blocks(kfn, S::NT, S::LDS));",
                 "const unsigned blocks = (unsigned)std::min<int64_t>(kAuxLossBlocks, (total + 255) / 256);",
                 "__launch_bounds__(512, 1) void aux_dx4_x6_kernel", "__launch_bounds__(512, 1) void conv_wgrad_x6_kernel"):
        assert text in pol, text
    # the single-stage and the two-stage sums as the bit test restates them
    assert "for (int z = 0; z < splits; ++z) s += slab[((int64_t)z * M + row) * N + col];" in pol
    assert "for (int z = blockIdx.y; z < nslab; z += gridDim.y) s += slab[(int64_t)z * n + i];" in _source("vn_conv1.h")


def test_every_switch_has_a_case_on_each_side():
    assert ac.uncovered() == []
    # the check notices a case taken away or moved
    for hw, n in ((G84, 190), (G84, 8), (G174, 64), (G174, 513), (G300, 7), (G300, 43), (G300, 102)):
        fewer = dict(ac.CASE_N)
        fewer[hw] = tuple(m for m in ac.CASE_N[hw] if m != n)
        assert ac.uncovered(fewer), (GEO_IDS[hw], n)
    # and every case is there for a switch
    for hw in ac.GEOMETRIES:
        named = {1}
        for g, what, kernel, key, at in ac.SWITCHES:
            if g == hw and not ((g, kernel) in ac.LOOSE and key == "second_pass") and key != "n>1":
                named |= {at - 1, ac.ABOVE.get((g, kernel, key, at), at)}
        assert named == set(ac.CASE_N[hw]), (GEO_IDS[hw], sorted(named ^ set(ac.CASE_N[hw])))


def test_switches_sit_where_the_restated_rules_put_them():
    r = {c: ac.aux_regime(*c) for c in ac.CASES}
    # 84x84: SPI 7 and the weight gradient's IMG 3
    assert [r[G84, n]["fwd2"]["tail"] for n in (1, 6, 7, 8, 9)] == [1, 6, 7, 1, 2]
    assert [r[G84, n]["fwd2"]["items"] for n in (7, 8, 1792, 1797)] == [1, 2, 256, 257]
    assert [r[G84, n]["dw1"]["tail"] for n in (6, 7, 8, 9)] == [3, 1, 2, 3]
    assert [r[G84, n]["layer1"]["tail"] for n in (1, 6, 7, 8, 9)] == [1, 2, 3, 4, 1]
    assert (r[G84, 189]["dw1"]["items"], r[G84, 190]["dw1"]["items"]) == (63, 64)
    assert (r[G84, 189]["dw1"]["reduce"], r[G84, 190]["dw1"]["reduce"]) == ("one-stage", "two-stage")
    assert r[G84, 1797]["fwd2"]["tail"] == 5 and r[G84, 1797]["fwd2"]["second_pass"] and not r[G84, 1792]["fwd2"]["second_pass"]
    # 174x174: one sample an item everywhere but the first layer
    assert (r[G174, 63]["dw1"]["reduce"], r[G174, 64]["dw1"]["reduce"]) == ("one-stage", "two-stage")
    for k in ("fwd2", "dx4", "dw1"):
        assert not r[G174, 256][k]["second_pass"] and r[G174, 257][k]["second_pass"], k
    # 300x400: bands
    assert [r[G300, n]["dw1"]["items"] for n in (1, 2, 3, 6, 7, 30, 31)] == [17, 17, 34, 51, 68, 255, 272]
    assert (r[G300, 6]["dw1"]["reduce"], r[G300, 7]["dw1"]["reduce"]) == ("one-stage", "two-stage")
    assert [r[G300, n]["dw1"]["tail"] for n in (1, 2, 3)] == [1, 2, 1]
    assert (r[G300, 42]["dx4"]["items"], r[G300, 43]["dx4"]["items"]) == (252, 258)
    assert (r[G300, 51]["fwd2"]["items"], r[G300, 52]["fwd2"]["items"]) == (255, 260)
    assert (r[G300, 102]["bwd2"]["items"], r[G300, 103]["bwd2"]["items"]) == (510, 515)
    assert (r[G300, 12]["bwd2"]["partials"], r[G300, 13]["bwd2"]["partials"]) == (60, 65)
    # every geometry: the finish kernel's lanes and the backward's grid cap
    for hw, lo, hi in ((G84, 64, 65), (G174, 64, 65), (G300, 12, 13)):
        assert (r[hw, lo]["bwd2"]["per_lane"], r[hw, hi]["bwd2"]["per_lane"]) == (1, 2)
        assert r[hw, lo]["bwd2"]["one_pass"] and r[hw, hi]["bwd2"]["one_pass"]   # partials = items on any device
    for hw, lo, hi in ((G84, 512, 513), (G174, 512, 513), (G300, 102, 103)):
        assert not r[hw, lo]["bwd2"]["second_pass"] and r[hw, hi]["bwd2"]["second_pass"]
        assert r[hw, hi]["bwd2"]["bound"] == r[hw, hi]["bwd2"]["partials"] == ac.COLSUM_BLOCKS
    # the first layer's second pass is out of reach of a quick case (84x84: n > 8192, 174x174:
    # n > 1536, 300x400: n > 256 samples of 36x48x48 maps): tests/test_parity_dgrad_gpu.py holds
    # that kernel's grid-stride loop to the generic products
    assert not any(v["layer1"]["second_pass"] for v in r.values())
    assert [ac.aux_regime(hw, n)["layer1"]["second_pass"] for hw, n in ((G84, 8193), (G174, 1537), (G300, 257))] == [True] * 3


def test_second_pass_claims_hold_under_the_upper_bound():
    """items > bound, the bound no smaller on any part of up to CUS CUs, and no smaller than the
    bound that also takes __launch_bounds__' second argument as a ceiling."""
    floors = {"layer1": (256, "l1_lds", 2), "fwd2": (512, "fwd2_lds", None), "bwd2": (512, "bwd2_lds", 4),
              "dw1": (512, "wa_lds", 1), "dx4": (512, "dx4_lds", 1)}
    claims = 0
    for hw, n in ac.CASES:
        g, r = ac.geometry(hw), ac.aux_regime(hw, n)
        for k, (threads, lds, floor) in floors.items():
            per_cu = min(ac.THREADS_CU // threads, ac.LDS_CU // g[lds])
            assert per_cu >= 1
            bound = min(per_cu * ac.CUS, ac.COLSUM_BLOCKS) if k == "bwd2" else per_cu * ac.CUS
            assert r[k]["bound"] == bound, (k, hw, n)
            assert r[k]["second_pass"] == (r[k]["items"] > bound)
            for cus in (64, 128, 255):
                assert ac.aux_regime(hw, n, cus)[k]["bound"] <= bound
            if floor is not None:
                assert min(per_cu, floor) * ac.CUS <= per_cu * ac.CUS
            claims += r[k]["second_pass"]
        assert r["loss"]["second_pass"] == (n * g["PH"] * g["PW"] > ac.AUX_LOSS_BLOCKS * 256)
    assert claims >= 20


def test_inputs_are_what_the_issue_sets():
    for hw, n in ((G84, 1), (G84, 9), (G174, 65), (G300, 3)):
        a, b = ac.inputs(hw, n), ac.inputs(hw, n)
        assert all((a[k] == b[k]).all() for k in a)
        (ih, iw), _, (ph, pw) = ac.maps(hw)
        R = ac.table_rows(n)
        assert a["x4"].shape == (n, ih, iw, 32) and a["x4"].dtype == np.float32 and (a["x4"] >= 0).all()
        assert 0.4 < (a["x4"] == 0).mean() < 0.6
        assert a["table"].shape == (R, ph, pw, 4) and R != n and a["table"].dtype == np.float32
        for k in ("image_rows", "goal_rows"):
            assert a[k].dtype == np.int32 and a[k].shape == (n,) and 0 <= a[k].min() and a[k].max() < R
        assert a["image_rows"].max() == R - 1 and (a["image_rows"] != a["goal_rows"]).all()
        if n >= 9:
            assert len(set(a["image_rows"])) < n and (np.diff(a["image_rows"]) < 0).any()
    sd = ac.seeded_state(G84)
    assert set(sd) == set(ac.PARAM_NAMES) and all(np.abs(sd[k]).min() > 0 for k in sd if k.endswith("bias"))


# ---- sensitivity: one planted fault at a time, on the case built for it ------------------------
_REF = {}


def _ref(hw, n):
    """(sd, inputs, forward graph, float64 reference): computed once per case, never changed."""
    if (hw, n) not in _REF:
        sd, inp = ac.seeded_state(hw), ac.inputs(hw, n)
        fwd = ac.forward(sd, inp)
        pred = fwd["pred"].detach().numpy()
        dpred, stats = ac.loss_grad(pred, inp)
        ref = ac.backward(fwd, dpred)
        ref.update(pred=pred, dpred=dpred, stats=stats)
        _REF[hw, n] = (sd, inp, fwd, ref)
    return _REF[hw, n]


def _seen(got, ref, keys):
    """The smallest multiple of its tolerance by which the checks see got on the tensors keys."""
    errs = ac.errors(got, ref)
    assert set(keys) <= set(errs)
    return min(errs[k] / ac.TOL[k] for k in keys), errs


def _layer2(which=("weight", "bias")):
    return [k for k in ac.PARAM_NAMES if ".0.3." in k and k.rsplit(".", 1)[1] in which]


def _with_loss(pred, inp, goal_from=None):
    dpred, stats = ac.loss_grad(pred, inp, goal_from=goal_from)
    return {"pred": pred, "dpred": dpred, "dpred_fused": dpred, "stats": stats, "stats_fused": stats}


def test_fault_ragged_item_from_the_previous_items_maps():
    """84x84 n = 8: the second item holds one sample; it is computed from the maps the first item
    left in that slot (sample 0's)."""
    hw, n = G84, 8
    assert ac.aux_regime(hw, n)["fwd2"]["tail"] == 1 and ac.geometry(hw)["fwd2_spi"] == 7
    _, inp, _, ref = _ref(hw, n)
    pred = ref["pred"].copy()
    pred[7] = ref["pred"][0]
    seen, errs = _seen(_with_loss(pred, inp), ref, ("pred", "dpred", "dpred_fused"))
    assert seen >= 10, errs
    # the scalar the suite had: the per-head mean squared error at 1e-5
    print("ragged item: pred %.3g dpred %.3g stats %.3g" % (errs["pred"], errs["dpred"], errs["stats"]))


def test_fault_items_past_the_first_grid_pass_skipped():
    """174x174 n = 257: the forward never writes sample 256; 84x84 n = 513: the backward never
    adds sample 512 (parameter gradients without it, its dX4 unwritten)."""
    hw, n = G174, 257
    assert ac.aux_regime(hw, n)["fwd2"]["second_pass"]
    _, inp, _, ref = _ref(hw, n)
    pred = ref["pred"].copy()
    pred[256:] = 0.0
    seen, errs = _seen(_with_loss(pred, inp), ref, ("pred", "dpred", "dpred_fused"))
    assert seen >= 10, errs
    hw, n = G84, 513
    assert ac.aux_regime(hw, n)["bwd2"]["second_pass"]
    _, inp, fwd, ref = _ref(hw, n)
    got = ac.backward(fwd, ref["dpred"], samples=np.arange(n) < 512)
    keys = _layer2() + [k for k in ac.PARAM_NAMES if k.endswith(".0.1.bias")]
    seen, errs = _seen(got, ref, keys)
    assert seen >= 10, {k: errs[k] for k in keys}
    got["dx4"][512:] = 0.0
    assert _seen(got, ref, ("dx4",))[0] >= 10


@pytest.mark.parametrize("hw", ac.GEOMETRIES, ids=[GEO_IDS[hw] for hw in ac.GEOMETRIES])
def test_fault_last_row_and_column_taps_lost(hw):
    """The last output row and column of the second transposed conv take one tap row / column
    (ky = 3 from A1's last row): lost, the bias alone is left there."""
    sd, inp, _, ref = _ref(hw, 1)
    pred = ref["pred"].copy()
    b2 = np.concatenate([sd["%s.0.3.bias" % name] for name, _, _ in ac.HEADS]).astype(np.float64)
    pred[:, -1, :, :7] = b2
    pred[:, :, -1, :7] = b2
    seen, errs = _seen(_with_loss(pred, inp), ref, ("pred", "dpred", "dpred_fused"))
    assert seen >= 10, errs
    print("%s border taps: pred %.3g dpred %.3g, the scalar statistics %.3g" % (GEO_IDS[hw], errs["pred"], errs["dpred"],
                                                                              errs["stats"]))


def test_fault_band_seam_rows_counted_twice_in_db2():
    """300x400: bands of 8 A1 rows stage 18 dP rows and count the first 16 (the last band all of
    its 10); counting every staged row adds rows 16, 17, 32, 33, 48, 49, 64, 65 a second time."""
    hw, n = G300, 2
    g = ac.geometry(hw)
    assert (g["bwd2_bya"], g["bwd2_bands"], g["bwd2_last"]) == (8, 5, 4)
    _, inp, _, ref = _ref(hw, n)
    seams = [2 * g["bwd2_bya"] * b + d for b in range(1, g["bwd2_bands"]) for d in (0, 1)]
    assert seams == [16, 17, 32, 33, 48, 49, 64, 65] and seams[-1] < g["PH"]
    extra = ref["dpred"][:, seams].sum(axis=(0, 1, 2))
    got = {k: v.copy() for k, v in ref.items() if k in ac.PARAM_NAMES}
    for name, c, o in ac.HEADS:
        got[name + ".0.3.bias"] += extra[o:o + c]
    keys = _layer2(("bias",))
    seen, errs = _seen(got, ref, keys)
    assert seen >= 10, {k: errs[k] for k in keys}


@pytest.mark.parametrize("hw,n", [(G84, 65), (G174, 65), (G300, 13)], ids=["84x84", "174x174", "300x400"])
def test_fault_partial_sum_stops_after_64_partials(hw, n):
    r, g = ac.aux_regime(hw, n)["bwd2"], ac.geometry(hw)
    assert r["partials"] == 65 and r["per_lane"] == 2
    _, inp, fwd, ref = _ref(hw, n)
    keys = _layer2() + [k for k in ac.PARAM_NAMES if k.endswith(".0.1.bias")]
    if g["bwd2_bands"] == 1:
        got = ac.backward(fwd, ref["dpred"], samples=np.arange(n) < 64)
    else:   # partial 64 is the last band of the last sample: its dP rows and its A1 rows
        assert (n * g["bwd2_bands"], g["bwd2_last"]) == (65, 4)
        full = ac.backward(fwd, ref["dpred"])
        dp = np.zeros_like(ref["dpred"])
        y0 = g["AH"] - g["bwd2_last"]
        dp[-1, 2 * y0:] = ref["dpred"][-1, 2 * y0:]      # the rows that band's windows read and db2 counts
        band = ac.backward(fwd, dp)
        # of those rows' effect the band owns what reaches A1 rows >= y0 (dW2, db1) and all of db2
        # (rows 2 y0 .. are counted by the last band alone)
        a1 = fwd["a1"].numpy()
        keep = np.zeros_like(a1)
        keep[-1, y0:] = 1.0
        got = {k: full[k].copy() for k in ac.PARAM_NAMES}
        for h, (name, c, o) in enumerate(ac.HEADS):
            got[name + ".0.3.bias"] -= band[name + ".0.3.bias"]
            got[name + ".0.1.bias"] -= (band["da1"] * keep)[..., 16 * h:16 * h + 16].sum(axis=(0, 1, 2))
        keys = _layer2(("bias",)) + [k for k in ac.PARAM_NAMES if k.endswith(".0.1.bias")]
    seen, errs = _seen(got, ref, keys)
    assert seen >= 10, {k: errs[k] for k in keys}


@pytest.mark.parametrize("hw,n,kept", [(G84, 7, 6), (G84, 8, 6), (G300, 3, 2)], ids=["84x84-n7", "84x84-n8", "300x400-n3"])
def test_fault_weight_gradient_half_item_dropped(hw, n, kept):
    r, g = ac.aux_regime(hw, n)["dw1"], ac.geometry(hw)
    assert r["tail"] == n - kept < g["wa_img"]
    _, inp, fwd, ref = _ref(hw, n)
    got = ac.backward(fwd, ref["dpred"], samples=np.arange(n) < kept)
    keys = [k for k in ac.PARAM_NAMES if k.endswith(".0.1.weight")]
    seen, errs = _seen(got, ref, keys)
    assert seen >= 10, {k: errs[k] for k in keys}


@pytest.mark.parametrize("hw,n", [(G84, 9), (G300, 2)], ids=["84x84-n9", "300x400-n2"])
def test_fault_goal_targets_read_from_image_rows(hw, n):
    _, inp, _, ref = _ref(hw, n)
    assert (inp["image_rows"] != inp["goal_rows"]).all()
    got = _with_loss(ref["pred"], inp, goal_from="image_rows")
    seen, errs = _seen(got, ref, ("dpred", "dpred_fused"))
    assert seen >= 10, errs
    assert errs["pred"] == 0.0
    print("goal rows: dpred %.3g, the scalar statistics %.3g" % (errs["dpred"], errs["stats"]))


@pytest.mark.parametrize("hw,n", [(G84, 65), (G174, 9), (G300, 2)], ids=["84x84", "174x174", "300x400"])
def test_float32_arithmetic_stays_under_half_of_every_bar(hw, n):
    """A plain float32 forward / loss / backward on the CPU against float64 (with float64's
    masks: no tie flips between them): were it within a factor of two of a bar, the inputs would
    have collapsed that tensor's scale."""
    import torch
    sd, inp = ac.seeded_state(hw), ac.inputs(hw, n)
    ref = ac.reference(sd, inp)
    masks = [z > 0 for z in ref["pre"]]
    f32 = ac.reference(sd, inp, masks=masks, dtype=torch.float32)
    f32.update(dpred_fused=f32["dpred"], stats_fused=f32["stats"])
    errs = ac.errors(f32, ref)
    assert set(errs) == set(ac.TOL)
    print("%s n=%d float32 floor: %s" % (GEO_IDS[hw], n, {k: "%.2g" % e for k, e in errs.items()}))
    assert all(e <= 0.5 * ac.TOL[k] for k, e in errs.items()), errs
