"""The conditions the cases of tests/test_lstm_regimes_gpu.py rest on, checked on the CPU from the
launch rules restated in oracle/unreal_head_cases.py, fed the recurrent core's shapes by
oracle/lstm_regime_cases.py: the table is those rules and holds the values derived from the launch
code, the switch list found from the launch code's inequalities equals a scan of every E in 18..1030,
the case list covers every value of every key and every case is needed, the calling forms sit where
they are said to, and the inputs are reproducible with their resets placed.

The seeded inputs are shown to expose the faults these regimes can hide. The core is restated in
float64 with its backward written out (checked against autograd through torch's float64 nn.LSTM), and
each fault is restated in it on the inputs of the case named: the last gates slab dropped, the last dh
slab dropped, the mask taken as 1 in the dh epilogue, the last part-filled dW_cat slab dropped, b_hh's
gradient left unwritten, dh_extra given to the rows e >= S as well. Each moves the tensors named by
at least 100 times the bar the GPU test holds them to (1e-5 of scale for h and c, 1e-4 for dz5 and
the gradients). A condition on the inputs: a seed that fails it is replaced, the factor stays."""
import math

import numpy as np
import pytest
import torch

from oracle import a2c as oa2c
from oracle import few_env_cases as fc
from oracle import lstm_regime_cases as lc
from oracle import unreal_head_cases as uc

FACTOR = 100
BAR_STATE, BAR_GRAD = 1e-5, 1e-4
LSTM_GRADS = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")


def _r(E, T, A=4):
    return lc.lstm_regime(E, T, A)


# ---- the table ------------------------------------------------------------------------------------
def test_regimes_are_the_restated_launch_rules():
    """lstm_regime is splitk_chunk / wgrad_chunk / reduce_lanes of oracle/unreal_head_cases.py on the core's
    shapes, nothing of its own."""
    assert [lc.layout(A) for A in (1, 3, 4, 7)] == [(514, 516, 1028), (516, 516, 1028), (517, 520, 1032), (520, 520, 1032)]
    assert {A: lc.layout(A)[1] - lc.layout(A)[0] for A in fc.XCAT_PAD} == fc.XCAT_PAD
    for E, T, A in [(E, T, 4) for E, T in lc.CASES] + [c[:3] for c in lc.VARIANT_CASES] + [(17, 3, 4), (2048, 3, 4)]:
        r, N, xcat = _r(E, T, A), T * E, lc.layout(A)[2]
        assert (r["gates"]["slabs"], r["gates"]["kchunk"]) == uc.splitk_chunk(E, 2048, xcat, 128, 128)
        assert (r["dh"]["slabs"], r["dh"]["kchunk"]) == uc.splitk_chunk(E, 512, 2048, 64, 64)
        assert (r["dz5"]["slabs"], r["dz5"]["kchunk"]) == uc.splitk_chunk(N, 512, 2048, 128, 128)
        assert (r["headf"]["slabs"], r["headf"]["kchunk"]) == uc.splitk_chunk(N, A + 1, 512, 64, 16)
        assert N >= 4673 or (r["headf"]["slabs"], r["headf"]["kchunk"], r["headf"]["lanes"]) == (8, 64, 1)  # 74 row tiles
        assert (r["wcat"]["slabs"], r["wcat"]["kchunk"]) == uc.wgrad_chunk(2048, xcat, N, 128, 128, True)
        assert (r["headw"]["slabs"], r["headw"]["kchunk"]) == uc.wgrad_chunk(A + 1, 512, N, 32, 64, True)
        for p, (M, Ncols) in (("gates", (E, 2048)), ("dh", (E, 512)), ("dz5", (N, 512)), ("headf", (N, A + 1)),
                              ("wcat", (2048, xcat + 1)), ("headw", (A + 1, 513))):
            v = r[p]
            assert v["lanes"] == (uc.reduce_lanes(M, Ncols, v["slabs"]) if v["slabs"] > 1 else 0)
            assert 0 < v["last"] <= v["kchunk"] and (v["slabs"] == 1 or v["kchunk"] % uc.BK == 0), (E, T, A, p, v)
        for p, rows in (("gates", E), ("dh", E), ("dz5", N), ("headf", N)):
            bm = lc.TILE[p][0]
            assert (r[p]["row_tiles"], r[p]["rem"]) == (-(-rows // bm), rows % bm)


def test_values_derived_from_the_launch_code():
    g = {E: _r(E, 1)["gates"] for E in (18, 31, 32, 186, 187, 192, 227, 228, 292, 293, 341, 342, 409, 410, 512, 513,
                                        682, 683, 896, 897)}
    assert [g[E]["slabs"] for E in (18, 186, 187, 227, 228, 292, 293, 341, 342, 409, 410, 512, 513, 682, 683, 896, 897)] == \
        [11, 11, 9, 9, 7, 7, 6, 6, 5, 5, 4, 4, 3, 3, 2, 2, 1]
    assert (g[192]["slabs"], g[192]["kchunk"], g[192]["last"]) == (9, 128, 8) and g[192]["last"] < uc.BK
    assert [g[E]["lanes"] for E in (18, 31, 32)] == [2, 2, 1]
    # from E = 187 the slab count is set by sk_cap (splits E 2048 > 4 << 20), not by the 512-workgroup target:
    # 16 splits (the K / 64 bound) still fit at 128 envs, 10 at 187
    assert 16 * 128 * 2048 <= uc.SK_CAP < 11 * 187 * 2048 and 10 * 187 * 2048 <= uc.SK_CAP
    assert -(-(-(-1032 // 10)) // 32) * 32 == 128 and -(-1032 // 128) == 9
    # bench.py's c5 leg: 512 envs
    assert (g[512]["slabs"], _r(512, 1)["dh"]["slabs"]) == (4, 8)
    d = {E: _r(E, 1)["dh"] for E in (18, 127, 128, 129, 192, 193, 257, 321, 385, 449, 577, 641, 769, 960, 961)}
    assert [(d[E]["slabs"], d[E]["lanes"]) for E in (18, 127, 128)] == [(32, 4), (32, 4), (32, 1)]
    assert [d[E]["slabs"] for E in (129, 193, 257, 321, 385, 449, 577, 641, 769, 960, 961)] == [22, 16, 13, 11, 10, 8, 7, 6, 5, 5, 1]
    assert min(E for E in range(18, 1031) if _r(E, 1)["dh"]["slabs"] == 1) == 961
    # dz5 over T E rows: 32 slabs down to 2, 4 lanes or 1, unsplit only from 3969 rows
    z = {_r(E, T)["dz5"]["slabs"] for T in lc.STEPS for E in range(18, 1031)}
    assert max(z) == 32 and min(z) == 2
    assert {_r(E, T)["dz5"]["lanes"] for T in lc.STEPS for E in range(18, 1031)} == {4, 1}
    assert _r(1323, 3)["dz5"]["slabs"] == 1 and _r(3968, 1)["dz5"]["slabs"] == 2 and _r(3969, 1)["dz5"]["slabs"] == 1
    # dW_cat: direct to 256 rows, 2..11 slabs, and from 2817 rows the slab bound halves 12..15 slabs to 6..7
    w = {n: _r(n, 1)["wcat"]["slabs"] for n in (18, 256, 257, 2816, 2817, 3072, 3075, 6144)}
    assert w == {18: 1, 256: 1, 257: 2, 2816: 11, 2817: 6, 3072: 6, 3075: 6, 6144: 7}
    assert 11 * 2048 * 1033 <= uc.SLAB < 12 * 2048 * 1033
    assert {_r(E, T)["wcat"]["slabs"] for T in lc.STEPS for E in range(18, 1031)} == set(range(1, 12))
    # the heads' weight gradient: 1..13 slabs, 1 or 2 reduce lanes
    assert {_r(E, T)["headw"]["slabs"] for T in lc.STEPS for E in range(18, 1031)} == set(range(1, 14))
    assert {_r(E, T)["headw"]["lanes"] for T in lc.STEPS for E in range(18, 1031)} == {0, 1, 2}
    # what the existing float64 cases run: E = 17 (gates 11 slabs, 2 lanes), 1024 and 2048 at T = 3
    assert (_r(17, 3)["gates"]["slabs"], _r(17, 3)["gates"]["lanes"]) == (11, 2)
    assert [(_r(E, 3)["gates"]["slabs"], _r(E, 3)["dh"]["slabs"], _r(E, 3)["wcat"]["slabs"]) for E in (1024, 2048)] == \
        [(1, 1, 6), (1, 1, 7)]


def test_switch_list_equals_a_scan():
    for T in lc.STEPS:
        assert lc.SWITCHES[T] == lc.switches(T) == lc.scan_switches(T)
        assert all(lc.FIRST_E < e <= lc.LAST_E and changed for e, changed in lc.SWITCHES[T])
    at = {p: [e for e, ch in lc.SWITCHES[1] if p in ch] for p in ("gates", "dh")}
    # gates: the lanes at 32, a second and a third row tile at 129 and 257, the sk_cap steps, unsplit at 897
    assert at["gates"] == [32, 129, 187, 228, 257, 293, 342, 410, 513, 683, 897]
    assert at["dh"] == [65, 128, 129, 193, 257, 321, 385, 449, 577, 641, 769, 961]
    assert at["gates"] == [e for e, ch in lc.SWITCHES[3] if "gates" in ch]      # the per-step products do not depend on T
    assert [e for e, ch in lc.SWITCHES[3] if "wcat" in ch] == [86, 171, 257, 342, 427, 513, 598, 683, 769, 854, 939]
    assert sum(len(ch) for T in lc.STEPS for _, ch in lc.SWITCHES[T]) > 40
    assert lc.form(18, 1)["headf"] == lc.form(1030, 3)["headf"] == (8, 1)


def test_cover_and_case_cap():
    cases = lc.CASES
    assert len(cases) == len(set(cases)) <= lc.MAX_CASES and cases == sorted(cases)
    assert all(lc.FIRST_E <= E <= lc.LAST_E and T in lc.STEPS for E, T in cases)
    assert lc.uncovered(cases) == []
    for c in cases:  # every case is needed: without it a key loses a value
        assert lc.uncovered([x for x in cases if x != c]), c
    assert cases == lc.greedy_cover() and lc.FAULT_GATES_SLAB in cases
    keys = lc.all_keys()
    # dh is observed only where a step t - 1 reads it: its keys count for T >= 2 alone, and every value they take
    # in 18..1030 (the same at every T: dh's shape is E x 512) is held by a case with a BPTT hop
    assert not any(k.startswith("dh ") for E in (18, 256, 1025) for k, _ in lc.cover_keys(E, 1))
    seen = set().union(*(lc.cover_keys(E, T) for E, T in cases if T >= 2))
    for E in range(lc.FIRST_E, lc.LAST_E + 1):
        d = _r(E, 1)["dh"]
        assert {("dh slabs", d["slabs"]), ("dh lanes", d["lanes"]),
                ("dh split, row tiles, remainder", (d["slabs"] > 1, min(d["row_tiles"], 3), d["rem"] != 0))} <= seen, E
    assert {v for k, v in keys if k == "gates slabs"} == {11, 9, 7, 6, 5, 4, 3, 2, 1}
    assert {v for k, v in keys if k == "dh slabs"} == {32, 22, 16, 13, 11, 10, 8, 7, 6, 5, 1}
    assert {v for k, v in keys if k == "gates last slab < BK"} == {False, True}
    assert {v for k, v in keys if k == "wcat split, last slab part filled, its length no multiple of 32"} == \
        {(False, False, False), (False, True, True), (True, False, False), (True, True, False), (True, True, True)}
    assert {v for k, v in keys if k == "dh split, row tiles, remainder"} == \
        {(True, n, rem) for n in (1, 2, 3) for rem in (False, True)} | {(False, 3, False), (False, 3, True)}
    # the largest case has 3075 rows
    assert max(E * T for E, T in cases) == 3075


def test_calling_forms_sit_where_they_are_said_to():
    v = lc.VARIANT_CASES
    assert len(lc.VARIANT_IDS) == len(set(lc.VARIANT_IDS)) == len(v) == 9
    assert all(E > fc.SKINNY_ROWS + 1 for E, T, A, nul, x in v)
    assert [(E, T, A) for E, T, A, nul, x in v if A != 4] == [(40, 3, 1), (40, 3, 3), (40, 3, 7), (192, 3, 1)]
    # A = 1 and 3: xcat 1028, a K tail of 4 against BK = 32 instead of 8; A = 7 fills the heads' 8 output columns
    assert [_r(40, 3, A)["gates"]["last"] for A in (1, 3, 7)] == [68, 68, 72] and 1028 % 32 == 4 and 1032 % 32 == 8
    # where A = 4 has the short last slab, A = 1 has 9 slabs of 128 as well, the last of 4 k-columns
    E, T, A = lc.SHORT_SLAB_E, 3, lc.SHORT_SLAB_A
    assert 190 <= E <= 227 and (_r(E, T, 4)["gates"]["slabs"], _r(E, T, 4)["gates"]["last"]) == (9, 8)
    assert (_r(E, T, A)["gates"]["slabs"], _r(E, T, A)["gates"]["kchunk"], _r(E, T, A)["gates"]["last"]) == (9, 128, 4)
    assert {(E, T) for E, T, A, nul, x in v if nul} == {(18, 3), (300, 3)}
    assert {(E, x, T) for E, T, A, nul, x in v if x} == {(40, 5, 3), (300, 16, 3)}
    assert all(x < E for E, T, A, nul, x in v)
    r = _r(130, 2)
    assert (130, 2, 4, False, 0) in v and (r["dh"]["slabs"], r["dh"]["row_tiles"], r["dh"]["rem"]) == (22, 3, 2)
    assert lc.FAULT_EXTRA in v and all(c in lc.CASES for c in (lc.FAULT_GATES_SLAB, lc.FAULT_DH_SLAB, lc.FAULT_DH_MASK,
                                                                 lc.FAULT_WCAT_SLAB, lc.FAULT_DB2))
    assert len(lc.regime_table()) == len(lc.CASES) + len(v)
    # the whole-update cases: 136 envs x 4 steps has gates on two row tiles with 8 rows in the second, dh on 22
    # slabs over three row tiles and dW_cat on 3 slabs over 544 rows; 20 envs keep every product in its first form
    # with dW_cat on the direct epilogue (80 and 120 rows)
    assert lc.TRAINER_CASES == [(20, 4), (136, 4), (20, 6)]
    r = _r(136, 4)
    assert (r["gates"]["slabs"], r["gates"]["row_tiles"], r["gates"]["rem"]) == (11, 2, 8)
    assert (r["dh"]["slabs"], r["dh"]["row_tiles"], r["dh"]["rem"]) == (22, 3, 8)
    assert (r["wcat"]["slabs"], r["wcat"]["kchunk"], r["wcat"]["last"], 136 * 4) == (3, 192, 160, 544)
    for T, rows in ((4, 80), (6, 120)):
        r = _r(20, T)
        assert (r["gates"]["slabs"], r["gates"]["lanes"], r["dh"]["slabs"], r["dh"]["lanes"]) == (11, 2, 32, 4)
        assert (r["dz5"]["slabs"], r["dz5"]["lanes"], r["wcat"]["slabs"], r["wcat"]["last"], r["headw"]["slabs"]) == (32, 4, 1, rows, 1)


def test_inputs_are_reproducible_and_masks_placed():
    for E, T, A, S in [(E, T, 4, 0) for E, T in lc.CASES[:4]] + [(E, T, A, x) for E, T, A, nul, x in lc.VARIANT_CASES]:
        a, b = lc.inputs(E, T, A, S), lc.inputs(E, T, A, S)
        N = T * E
        for k in a:
            assert (a[k] is None and b[k] is None) or (a[k].tobytes() == b[k].tobytes() and a[k].dtype == b[k].dtype), k
        assert a["x5"].shape == (N, 512) and a["x5"].min() == 0.0 and a["lra"].shape == (T, E, A + 1)
        assert a["h0"].shape == a["c0"].shape == (E, 512) and a["rets"].shape == (N,)
        assert a["actions"].dtype == np.int32 and a["actions"].min() >= 0 and a["actions"].max() < A
        assert (a["dh_extra"] is None) == (S == 0) and (S == 0 or a["dh_extra"].shape == (T, S, 512))
        assert all(a[k].dtype == np.float32 for k in ("x5", "lra", "masks", "h0", "c0", "rets"))
        m = a["masks"]
        assert m.shape == (T, E) and set(np.unique(m)) == {0.0, 1.0} and np.array_equal(m, lc.masks(E, T))
        assert np.all(m <= fc.lstm_masks(E, T)) and all(m[t, e] == 0 for t, e in lc.resets(E, T))
        assert np.array_equal(a["lra"], a["lra"] * m[..., None])
        assert np.all(a["lra"][..., :A].sum(2) == m)   # one-hot where the env runs on
        if T >= 2:  # a zero of the dh epilogue's mask (t >= 1) in dh's first and in its last 64-row tile
            tiles = -(-E // 64)
            assert (m[1:, :64] == 0).any() and (m[1:, 64 * (tiles - 1):] == 0).any()
    for E, T in lc.CASES:
        m = lc.masks(E, T)
        assert 0.02 <= 1.0 - m.mean() <= 0.2, (E, T)
        if T >= 2:
            assert (m[1:, :64] == 0).any() and (m[1:, 64 * (-(-E // 64) - 1):] == 0).any()


# ---- the core in float64, its backward written out -------------------------------------------------
def _params(A, seed):
    """Parameters of the law the GPU test draws: init_params (xavier-uniform W_ih, orthogonal W_hh, zero
    biases, heads U(+-1/sqrt(512))) plus N(0, 0.01) on every tensor. The same law, not the same values:
    the GPU test's come from PolicyNet.init_params(3) over the flat buffer, which needs the library. The
    fault checks are conditions on the inputs, so they run for each draw of lc.WEIGHT_SEEDS."""
    lin = lc.layout(A)[0]
    g = torch.Generator().manual_seed(seed)
    wih, whh, wh = torch.empty(2048, lin), torch.empty(2048, 512), torch.empty(A + 1, 512)
    torch.nn.init.xavier_uniform_(wih, generator=g)
    torch.nn.init.orthogonal_(whh, generator=g)
    wh.uniform_(-1.0 / math.sqrt(512), 1.0 / math.sqrt(512), generator=g)
    p = {"weight_ih": wih, "weight_hh": whh, "bias_ih": torch.zeros(2048), "bias_hh": torch.zeros(2048), "head_w": wh,
         "head_b": torch.zeros(A + 1)}
    return {k: (v + torch.randn(v.shape, generator=g) * 0.01).double() for k, v in p.items()}


def _core(p, inp, A, S=0, fault=None, cut=None):
    """The core on one case's inputs in float64, as csrc/vn_policy.hip lays it out: xcat = [x5 | lra | 0 | m
    h_prev] against W_cat = [W_ih | 0 | W_hh] for the gates, dh_{t-1} = m_t (dgates_t x W_hh) per step, dz5
    and dW_cat over all rows. fault: None or one of
      "gates_slab"  the gates without the k-columns from cut on (the last K slab of the split product)
      "dh_slab"     dh without the gate columns from cut on (the last K slab of dgates x W_hh)
      "dh_mask"     dh with the mask taken as 1
      "wcat_slab"   dW_cat and the bias gradients without the rows from cut on (the last slab of the rows)
      "db2"         b_hh's gradient left at zero
      "extra_rows"  dh_extra row e mod S added to every env, not to the first S alone"""
    T, E = inp["masks"].shape
    lin, xoff, xcat_w = lc.layout(A)
    d = lambda k: torch.as_tensor(inp[k]).double()  # noqa: E731
    x5, lra, m = d("x5").view(T, E, 512), d("lra"), d("masks")
    wcat = torch.zeros(2048, xcat_w, dtype=torch.float64)
    wcat[:, :lin], wcat[:, xoff:] = p["weight_ih"], p["weight_hh"]
    bias = p["bias_ih"] + p["bias_hh"]
    h, c = d("h0"), d("c0")
    xs, acts, cs, hs, cps = [], [], [], [], []
    for t in range(T):
        mt = m[t][:, None]
        xc = torch.cat((x5[t], lra[t], torch.zeros(E, xoff - lin, dtype=torch.float64), h * mt), 1)
        k = cut if fault == "gates_slab" else xcat_w
        z = xc[:, :k] @ wcat[:, :k].t() + bias
        i, f, g, o = torch.sigmoid(z[:, :512]), torch.sigmoid(z[:, 512:1024]), torch.tanh(z[:, 1024:1536]), torch.sigmoid(z[:, 1536:])
        cp = c * mt
        c = f * cp + i * g
        h = o * torch.tanh(c)
        xs.append(xc), acts.append((i, f, g, o)), cs.append(c), hs.append(h), cps.append(cp)
    y = torch.cat(hs).clone().requires_grad_()
    out = y @ p["head_w"].t() + p["head_b"]
    loss, _ = oa2c.loss(out[:, :A], out[:, A], torch.as_tensor(inp["actions"]).long(), d("rets"))
    dout, = torch.autograd.grad(loss, out, retain_graph=True)
    dhh = (dout @ p["head_w"]).view(T, E, 512).clone()
    if S:
        dhx = d("dh_extra")
        if fault == "extra_rows":
            dhh += dhx[:, torch.arange(E) % S]
        else:
            dhh[:, :S] += dhx
    res = {"h": torch.stack(hs), "c": torch.stack(cs), "head_w": dout.t() @ y.detach(), "head_b": dout.sum(0)}
    dgs = [None] * T
    dh_next = dc_next = torch.zeros(E, 512, dtype=torch.float64)
    for t in range(T - 1, -1, -1):
        i, f, g, o = acts[t]
        tc = torch.tanh(cs[t])
        dh = dhh[t] + dh_next
        dc = dc_next + dh * o * (1 - tc * tc)
        dg = torch.cat((dc * g * i * (1 - i), dc * cps[t] * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)), 1)
        dgs[t] = dg
        mt = m[t][:, None]
        dc_next = dc * f * mt
        k = cut if fault == "dh_slab" else 2048
        dh_next = dg[:, :k] @ p["weight_hh"][:k]
        if fault != "dh_mask":
            dh_next = dh_next * mt
    dg, xc = torch.cat(dgs), torch.cat(xs)
    res["dz5"] = (dg @ p["weight_ih"][:, :512]) * (x5.reshape(-1, 512) > 0)
    rows = cut if fault == "wcat_slab" else T * E
    dw = dg[:rows].t() @ xc[:rows]
    res["weight_ih"], res["weight_hh"], res["pad"] = dw[:, :lin], dw[:, xoff:], dw[:, lin:xoff]
    res["bias_ih"] = dg[:rows].sum(0)
    res["bias_hh"] = torch.zeros(2048, dtype=torch.float64) if fault == "db2" else res["bias_ih"].clone()
    return res


def _moved(a, b):
    return float((a - b).abs().max() / a.abs().max())


def _moved_steps(a, b):
    """h / c [T, E, 512]: the least over the steps of the change against that step's own scale."""
    return min(_moved(a[t], b[t]) for t in range(a.shape[0]))


def _assert_moved(good, bad, names, what):
    for k in names:
        bar = BAR_STATE if k in ("h", "c") else BAR_GRAD
        mv = _moved_steps(good[k], bad[k]) if k in ("h", "c") else _moved(good[k], bad[k])
        assert mv >= FACTOR * bar, "%s: %s moves by %.3g of scale, under %d x %g" % (what, k, mv, FACTOR, bar)


@pytest.fixture(scope="module", params=lc.WEIGHT_SEEDS, ids=["weights%d" % s for s in lc.WEIGHT_SEEDS])
def params4(request):
    return _params(4, request.param)


def test_written_out_backward_is_autograd_through_nn_lstm(params4):
    """The restatement with no fault against torch's float64 nn.LSTM under the MaskedRNN convention and
    autograd, as oracle/trunk_checks.py lstm_core_check builds its reference, at the (40, 5) case."""
    E, T, A, _, S = lc.FAULT_EXTRA
    inp, p = lc.inputs(E, T, A, S), params4
    got = _core(p, inp, A, S)
    lstm = torch.nn.LSTM(512 + A + 1, 512, batch_first=True).double()
    for k in LSTM_GRADS:
        getattr(lstm, k + "_l0").data.copy_(p[k])
    head = torch.nn.Linear(512, A + 1).double()
    head.weight.data.copy_(p["head_w"]), head.bias.data.copy_(p["head_b"])
    xf = torch.as_tensor(inp["x5"]).double().view(T, E, 512).requires_grad_()
    x = torch.cat((xf, torch.as_tensor(inp["lra"]).double()), 2)
    m = torch.as_tensor(inp["masks"]).double()
    h, c = torch.as_tensor(inp["h0"]).double()[None], torch.as_tensor(inp["c0"]).double()[None]
    ys, cs = [], []
    for t in range(T):
        y, (h, c) = lstm(x[t][:, None], (h * m[t][None, :, None], c * m[t][None, :, None]))
        ys.append(y[:, 0]), cs.append(c[0])
    y = torch.cat(ys)
    out = head(y)
    loss, _ = oa2c.loss(out[:, :A], out[:, A], torch.as_tensor(inp["actions"]).long(), torch.as_tensor(inp["rets"]).double())
    (loss + (y.view(T, E, 512)[:, :S] * torch.as_tensor(inp["dh_extra"]).double()).sum()).backward()
    assert _moved(torch.stack(ys).detach(), got["h"]) < 1e-12 and _moved(torch.stack(cs).detach(), got["c"]) < 1e-12
    assert _moved((xf.grad * (xf > 0)).reshape(-1, 512), got["dz5"]) < 1e-12
    for k in LSTM_GRADS:
        assert _moved(getattr(lstm, k + "_l0").grad, got[k]) < 1e-12, k
    assert _moved(head.weight.grad, got["head_w"]) < 1e-12 and _moved(head.bias.grad, got["head_b"]) < 1e-12
    assert not got["pad"].any()


def test_inputs_expose_a_dropped_gates_slab(params4):
    """1. (192, 1): gates on 9 slabs of 128, the last holds 8 k-columns (W_hh's last 8): h and c move."""
    E, T = lc.FAULT_GATES_SLAB
    g = _r(E, T)["gates"]
    assert (g["slabs"], g["kchunk"], g["last"]) == (9, 128, 8)
    inp = lc.inputs(E, T)
    good, bad = _core(params4, inp, 4), _core(params4, inp, 4, fault="gates_slab", cut=8 * 128)
    _assert_moved(good, bad, ("h", "c"), "last gates slab dropped")


def test_inputs_expose_a_dropped_dh_slab_and_a_mask_of_one(params4):
    """2. the last dh slab dropped at a T = 3 case; 3. the mask taken as 1 in the dh epilogue: dW_cat (both
    halves), b_ih and dz5 move."""
    E, T = lc.FAULT_DH_SLAB
    d = _r(E, T)["dh"]
    assert T == 3 and d["slabs"] > 1
    inp = lc.inputs(E, T)
    good = _core(params4, inp, 4)
    bad = _core(params4, inp, 4, fault="dh_slab", cut=(d["slabs"] - 1) * d["kchunk"])
    _assert_moved(good, bad, ("weight_ih", "weight_hh", "bias_ih", "dz5"), "last dh slab dropped")
    E, T = lc.FAULT_DH_MASK
    assert T == 3 and _r(E, T)["dh"]["slabs"] > 1
    inp = lc.inputs(E, T)
    good, bad = _core(params4, inp, 4), _core(params4, inp, 4, fault="dh_mask")
    _assert_moved(good, bad, ("weight_ih", "weight_hh", "bias_ih", "dz5"), "dh mask taken as 1")


def test_inputs_expose_a_dropped_wcat_slab_and_an_unwritten_b_hh(params4):
    """4. the last, part-filled dW_cat slab dropped where its length is no multiple of 32: W_ih's, W_hh's and
    both biases' gradients move; 5. b_hh's gradient left unwritten on the reduce's db2 path."""
    E, T = lc.FAULT_WCAT_SLAB
    w = _r(E, T)["wcat"]
    assert w["slabs"] > 1 and w["last"] < w["kchunk"] and w["last"] % 32 != 0
    inp = lc.inputs(E, T)
    good = _core(params4, inp, 4)
    bad = _core(params4, inp, 4, fault="wcat_slab", cut=(w["slabs"] - 1) * w["kchunk"])
    _assert_moved(good, bad, LSTM_GRADS, "last dW_cat slab dropped")
    E, T = lc.FAULT_DB2
    assert _r(E, T)["wcat"]["slabs"] > 1
    inp = lc.inputs(E, T)
    good, bad = _core(params4, inp, 4), _core(params4, inp, 4, fault="db2")
    _assert_moved(good, bad, ("bias_hh",), "b_hh's gradient unwritten")
    assert _moved(good["bias_hh"], good["bias_ih"]) == 0.0


def test_inputs_expose_dh_extra_on_every_row(params4):
    """6. (40, 5): the rows e >= S given dh_extra as well: every gradient of the LSTM and dz5 move."""
    E, T, A, _, S = lc.FAULT_EXTRA
    assert (E, S) == (40, 5)
    inp = lc.inputs(E, T, A, S)
    good, bad = _core(params4, inp, A, S), _core(params4, inp, A, S, fault="extra_rows")
    _assert_moved(good, bad, LSTM_GRADS + ("dz5",), "dh_extra on the rows e >= S")
