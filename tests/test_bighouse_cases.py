"""The conditions the cases of tests/test_bighouse_regimes_gpu.py rest on, checked on the CPU from
the launch rules restated in oracle/unreal_head_cases.py fed BigHouseModel's shapes
(oracle/bighouse_cases.py trunk_regime): every switch in n has a case on each side, and every n of
the case list is the nearest case to some switch, so removing one fails here and a changed
threshold names the case to move. The seeded inputs are shown to expose the faults the cases exist
for: the fp64 oracle with conv_merge's last K slab dropped, with conv3's border row and column
missing from dL/dX2, and with the last sample missing from conv1's weight gradient moves the
affected tensors by at least ten times their tolerance."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import a2c as oa2c
from oracle import bighouse_cases as bc
from oracle import few_env_cases as fc
from oracle import unreal_head_cases as uc
from oracle.policy import BigHouseOracle, frames_to_float
from oracle.trunk_checks import BIGHOUSE_NAMES, BIGHOUSE_PAIRS, _bighouse_forward_masked, _ties_only


def _r(n, A=4):
    return bc.trunk_regime(n, A)


def test_tables_hold_what_the_issue_sets():
    issue = {1, 3, 5, 6, 26, 42, 65, 127, 128, 193, 257, 961}
    assert issue <= set(bc.CASE_N) and list(bc.CASE_N) == sorted(set(bc.CASE_N))
    # the four more: the first n of each slab count of conv_merge's forward between 13 and unsplit
    assert set(bc.CASE_N) - issue == {321, 449, 641, 769}
    assert bc.PROD_N == 961 and bc.ACTION_CASES == [(n, A) for n in (5, 65) for A in (1, 3, 7)]
    assert bc.ROWS_N == (26, 257) and bc.FLOAT_N == (3, 65, 257) and bc.GUARD_N == (5, 65)
    assert bc.COTANGENT_N == (42, 193) and bc.DETERMINISM_N == (128, 961)
    for ns in (bc.ROWS_N, bc.FLOAT_N, bc.GUARD_N, bc.COTANGENT_N, bc.DETERMINISM_N, [n for n, A in bc.ACTION_CASES]):
        assert set(ns) <= set(bc.CASE_N)
    assert len(bc.regime_table()) == len(bc.CASE_N)


def test_regimes_are_the_restated_launch_rules():
    """trunk_regime is splitk / wgrad_slabs / reduce_lanes of oracle/unreal_head_cases.py on
    BigHouseModel's shapes, nothing of its own."""
    assert bc.FCIN == 1568 == 49 * uc.BK and bc.MERGE_TAIL == 1536
    for n in bc.CASE_N + (2, 4, 64, 192, 256, 320, 960, 4096):
        for A in (1, 4, 7):
            r = _r(n, A)
            assert r["merge_fwd"]["slabs"] == uc.splitk(n, 512, 1568, 64, 64)
            assert r["heads_fwd"]["slabs"] == uc.splitk(n, A + 1, 512, 64, 16)
            assert r["heads_wgrad"]["slabs"] == uc.wgrad_slabs(A + 1, 512, n, 32, 64, True)
            assert r["merge_wgrad"]["slabs"] == uc.wgrad_slabs(512, 1568, n, 128, 128, True)
            assert r["conv3_wgrad"]["slabs"] == uc.wgrad_slabs(32, 576, 49 * n, 32, 64, True)
            assert r["conv2_wgrad"]["slabs"] == uc.wgrad_slabs(64, 512, 81 * n, 64, 128, True)
            assert r["conv1_wgrad"]["slabs"] == uc.wgrad_slabs(32, 192, 400 * n, 32, 64, True)
            for p, v in r.items():
                assert 0 < v["last"] <= v["kchunk"] and (v["lanes"] > 0) == (v["slabs"] > 1), (n, p, v)
                if v["slabs"] > 1:
                    assert v["kchunk"] % uc.BK == 0
            assert r["conv1_wgrad"]["lanes"] == uc.reduce_lanes(32, 193, r["conv1_wgrad"]["slabs"])
            assert r["merge_dgrad"]["col_rem"] == 32  # N = 1568 = 24.5 column tiles


def test_every_switch_has_a_case_on_each_side_and_every_case_is_needed():
    assert bc.uncovered(bc.CASE_N) == []
    named = set()
    for what, product, key, at, lo, hi in bc.SWITCHES:
        below = [n for n in bc.CASE_N if n < at]
        above = [n for n in bc.CASE_N if n >= at]
        assert (below[-1], above[0]) == (lo, hi), what  # the nearest cases are the ones named
        a, b = bc.regime_value(at - 1, product, key), bc.regime_value(at, product, key)
        assert a != b, what  # the switch is where the table puts it
        assert bc.regime_value(lo, product, key) == a and bc.regime_value(hi, product, key) == b, what
        named |= {lo, hi}
    # every case is the nearest one to some switch on one of its sides: without it that side moves
    # further off, next to another switch, or is lost (the assertion on the named pair fails)
    assert named == set(bc.CASE_N)
    alone = [n for n in bc.CASE_N if bc.uncovered([m for m in bc.CASE_N if m != n])]
    assert alone == [1, 6, 321, 449, 641, 769, 961]  # the only case of a side: a regime no other case runs
    # 3 and 5 separate conv2's switch (3 | 4) from conv3's and conv1's (5 | 6): 3 is the last n with
    # conv2's weight gradient direct, 5 the only case with conv2's in slabs and conv3's direct
    assert [(_r(n)["conv2_wgrad"]["slabs"] > 1, _r(n)["conv3_wgrad"]["slabs"] > 1) for n in (3, 5, 6)] == \
        [(False, False), (True, False), (True, True)]


def test_switches_by_value():
    """The regime table of the issue, by value (DESIGN.md holds bc.regime_table())."""
    f = {n: _r(n)["merge_fwd"] for n in bc.CASE_N + (192, 256, 320, 448, 640, 768, 960)}
    # conv_merge forward: slabs x kchunk (last slab), per regime, with the last n of each
    want = {1: (17, 96, 32), 128: (17, 96, 32), 192: (17, 96, 32), 193: (13, 128, 32), 257: (13, 128, 32),
            320: (13, 128, 32), 321: (10, 160, 128), 448: (10, 160, 128), 449: (7, 224, 224), 640: (7, 224, 224),
            641: (6, 288, 128), 768: (6, 288, 128), 769: (5, 320, 288), 960: (5, 320, 288), 961: (1, 1568, 1568)}
    for n, w in want.items():
        assert (f[n]["slabs"], f[n]["kchunk"], f[n]["last"]) == w, n
    assert (f[127]["lanes"], f[128]["lanes"], f[961]["lanes"]) == (4, 1, 0) and 128 * 512 == uc.REDUCE_FLAT
    assert -(-961 // 64) * 8 == uc.SK_TILES and -(-960 // 64) * 8 < uc.SK_TILES
    # kchunk 96 and 128 leave a 32-long last slab at K = 1568; the unsplit form ends in half a 64-wide K tile
    assert 1568 - 16 * 96 == 32 and 1568 - 12 * 128 == 32 and 1568 % 64 == 32
    # 961: 15 row tiles + 1 row
    assert f[961]["rem"] == 1 and 961 // 64 == 15
    # heads forward: 8 slabs of 64 at every n, one epilogue lane
    for n in bc.CASE_N + (4096,):
        for A in (1, 3, 4, 7):
            h = _r(n, A)["heads_fwd"]
            assert (h["slabs"], h["kchunk"], h["last"], h["lanes"]) == (8, 64, 64, 1), (n, A)
    # heads and conv_merge weight gradients: direct up to 256 rows, 2 slabs from 257 (last slab: 1 row of 160)
    for p in ("heads_wgrad", "merge_wgrad"):
        assert [_r(n)[p]["slabs"] for n in (1, 193, 256, 257, 961)] == [1, 1, 1, 2, 4], p
        assert (_r(257)[p]["kchunk"], _r(257)[p]["last"]) == (160, 97)
    for A in bc.ACTION_COUNTS:
        assert _r(65, A)["heads_wgrad"]["slabs"] == 1
    # conv3 (P = 49 n): direct up to 5, lanes 1 -> 2 at 42, up to 32
    c = {n: _r(n)["conv3_wgrad"] for n in bc.CASE_N + (41,)}
    assert [c[n]["slabs"] for n in (1, 3, 5, 6)] == [1, 1, 1, 2]
    assert [c[n]["lanes"] for n in (6, 26, 41, 42, 961)] == [1, 1, 1, 2, 32]
    # conv2 (P = 81 n): direct up to 3, lanes 1 -> 2 at 26, up to 64
    c = {n: _r(n)["conv2_wgrad"] for n in bc.CASE_N + (4, 25)}
    assert [c[n]["slabs"] for n in (1, 3, 4, 5)] == [1, 1, 2, 2]
    assert [c[n]["lanes"] for n in (5, 6, 25, 26, 961)] == [1, 1, 1, 2, 64]
    # conv1 (P = 400 n): never direct, lanes 1 -> 2 at 6, 64 from 164
    c = {n: _r(n)["conv1_wgrad"] for n in bc.CASE_N + (2, 163, 164)}
    assert [c[n]["slabs"] for n in (1, 2, 3)] == [2, 4, 5]
    assert [c[n]["lanes"] for n in (1, 5, 6, 128, 163, 164, 193)] == [1, 1, 2, 32, 32, 64, 64]
    # every lane count of the reduces is run by some case
    lanes = {_r(n)[p]["lanes"] for n in bc.CASE_N for p in ("conv1_wgrad", "conv2_wgrad", "conv3_wgrad")}
    assert lanes == {0, 1, 2, 4, 8, 16, 32, 64}
    # ragged tiles: 128 fills every row tile, every other case leaves rows over somewhere; weight-gradient
    # reductions end inside a K tile
    full = _r(128)
    assert all(full[p]["rem"] == 0 for p in full)
    for n in bc.CASE_N:
        if n != 128:
            r = _r(n)
            assert r["merge_fwd"]["rem"] == n % 64 != 0
            assert any(r[p]["rem"] for p in ("conv1_fwd", "conv2_fwd", "conv3_fwd"))
    assert any(_r(n)["conv3_wgrad"]["rem"] for n in bc.CASE_N) and any(_r(n)["conv2_wgrad"]["rem"] for n in bc.CASE_N)
    # the switch left out: the slab cap halves conv_merge's weight-gradient slabs past n = 7936
    assert _r(7936)["merge_wgrad"]["slabs"] == 31 and _r(7937)["merge_wgrad"]["slabs"] == 16
    assert 32 * 512 * 1569 > uc.SLAB >= 31 * 512 * 1569


def test_inputs_are_reproducible_and_placed():
    a, b = bc.seeded_state(5, 3), bc.seeded_state(5, 3)
    assert set(a) == {k + "." + kind for k in BIGHOUSE_NAMES for kind in ("weight", "bias")}
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert a["policy_logits.0.weight"].shape == (3, 512) and a["conv_merge.0.1.weight"].shape == (512, 1568)
    init = bc.init_state(bc.weight_seed(5, 3), 3)
    assert not init["conv_base.0.2.bias"].any() and a["conv_base.0.2.bias"].any()  # the noise reaches the biases
    d = float((a["conv_base.0.4.weight"] - init["conv_base.0.4.weight"]).std())
    assert 0.009 < d < 0.011
    assert np.array_equal(bc.u8_frames(3), bc.u8_frames(3)) and not np.array_equal(bc.u8_frames(3), bc.u8_frames(3, 1))
    for n in bc.ROWS_N:
        arena, rows = bc.arena_rows(n)
        R = arena.shape[0]
        assert R == bc.ARENA_ROWS[n] < n and rows.dtype == np.int32 and rows.min() == 0 and rows.max() == R - 1
        assert rows[n - 1] == R - 1 and len(set(rows.tolist())) < n  # the last arena row is used; rows repeat
        assert rows[0] == 0 and len(set(rows.tolist())) > R // 2  # most samples see a frame of their own
    for n in bc.COTANGENT_N:
        dz5, dx3 = bc.trunk_cotangents(n)
        assert dz5.shape == (n, 512) and dx3.shape == (n, 7, 7, 32) and dz5.dtype == dx3.dtype == np.float32


def test_float_frames_are_off_the_u8_grid():
    for n in bc.FLOAT_N:
        f = bc.float_frames(n)
        assert f.dtype == np.float32 and f.shape == (n, 3, 84, 84) and 0.0 <= f.min() and f.max() < 1.0
        k = np.rint(f.astype(np.float64) * 255.0)
        off = np.abs(f - (k / 255.0).astype(np.float32)) > 1e-4
        assert off.mean() > 0.9  # nearly every value is far from a multiple of 1/255, as few_env_cases.float_frames
    g = fc.float_frames((84, 84), 3)[0]
    assert g.shape == bc.float_frames(3).shape


def _exposure_case():
    n, A = bc.EXPOSURE_N, 4
    ref = BigHouseOracle(A).load_reference(bc.seeded_state(n, A)).double()
    image = frames_to_float(torch.as_tensor(bc.u8_frames(n))).double()
    actions, rets = (torch.as_tensor(v) for v in fc.loss_inputs(n, A))
    return n, A, ref, image, actions.long(), rets.double()


def _moved(a, b):
    return float((a - b).abs().max() / a.abs().max())


def test_masked_forward_with_own_signs_equals_forward():
    n, A, ref, image, _, _ = _exposure_case()
    with torch.no_grad():
        z1 = ref.conv1(image)
        z2 = ref.conv2(torch.relu(z1))
        z3 = ref.conv3(torch.relu(z2))
        z5 = ref.fc(torch.relu(z3).flatten(1))
        masks = {"m1": (z1 > 0).double(), "m2": (z2 > 0).double(), "m3": (z3 > 0).double(), "m5": (z5 > 0).double()}
        x3, f, pre = _bighouse_forward_masked(ref, image, masks)
        assert torch.equal(f, ref.features(image)) and torch.equal(x3, torch.relu(z3))
        assert _ties_only(masks, pre, BIGHOUSE_PAIRS) == {"m1": 0, "m2": 0, "m3": 0, "m5": 0}
        masks["m3"][0, 0, 0, 0] = 1 - masks["m3"][0, 0, 0, 0]  # a flipped bit that is no tie is refused
        with pytest.raises(AssertionError):
            _ties_only(masks, pre, BIGHOUSE_PAIRS)


def test_inputs_expose_the_faults_the_cases_exist_for():
    """The fp64 oracle of one case (n = 6, u8 frames, the A2C loss), whole and with a part
    removed; each removal moves a tensor the GPU test checks by >= 10 x its tolerance. A condition
    on the seeded inputs: a seed that fails it is replaced, the factor stays."""
    n, A, ref, image, actions, rets = _exposure_case()
    W1, W2, W3 = ref.conv1.weight, ref.conv2.weight, ref.conv3.weight
    z1 = ref.conv1(image)
    z2 = ref.conv2(torch.relu(z1))
    x2 = torch.relu(z2)
    z3 = ref.conv3(x2)
    x3 = torch.relu(z3)
    x5 = torch.relu(ref.fc(x3.flatten(1)))
    loss, _ = oa2c.loss(ref.policy_logits(x5), ref.critic(x5).view(-1), actions, rets)
    g1, gx2, g3 = torch.autograd.grad(loss, (z1, x2, z3), retain_graph=True)

    # 1. a split-K reduce that drops conv_merge's last slab: K indices 1536..1567 of the kernels' NHWC
    #    rows [7][7][32] are the 32 channels of pixel (6, 6)
    assert bc.MERGE_TAIL == (6 * 7 + 6) * 32
    cut = x3.detach().clone()
    cut[:, :, 6, 6] = 0.0
    with torch.no_grad():
        moved = _moved(x5.detach(), torch.relu(ref.fc(cut.flatten(1))))
    assert moved >= 10 * 1e-5, "X5 moves by %.3g of scale" % moved

    # 2. a stride-1 input gradient that loses conv3's border taps: dL/dX2 without the outputs of row 0
    #    and column 0, seen in the weight gradients of conv2 and conv1 behind it
    full = F.conv_transpose2d(g3, W3.detach())
    assert _moved(gx2, full) <= 1e-12
    g3c = g3.clone()
    g3c[:, :, 0, :] = 0.0
    g3c[:, :, :, 0] = 0.0
    part = F.conv_transpose2d(g3c, W3.detach())
    for w, name in ((W2, "conv2"), (W1, "conv1")):
        a, = torch.autograd.grad(x2, w, grad_outputs=full, retain_graph=True)
        b, = torch.autograd.grad(x2, w, grad_outputs=part, retain_graph=True)
        assert _moved(a, b) >= 10 * 1e-4, "%s weight gradient moves by %.3g of scale" % (name, _moved(a, b))

    # 3. a weight-gradient reduce that stops one slab short: conv1's dW without the last sample's rows
    a, = torch.autograd.grad(z1, W1, grad_outputs=g1, retain_graph=True)
    g1c = g1.clone()
    g1c[n - 1] = 0.0
    b, = torch.autograd.grad(z1, W1, grad_outputs=g1c, retain_graph=True)
    assert _moved(a, b) >= 10 * 1e-4, "conv1 weight gradient moves by %.3g of scale" % _moved(a, b)
