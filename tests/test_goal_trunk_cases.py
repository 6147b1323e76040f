"""The conditions the cases of tests/test_goal_trunk_regimes_gpu.py rest on, checked on the CPU from
the launch rules restated in oracle/unreal_head_cases.py and the band structs restated in
oracle/goal_trunk_cases.py, fed the goal trunk's shapes at its three geometries: the table reproduces
the switch points derived from the launch code, every switch has a case in the right regime on each
side, every case is needed (without it some switch loses a side) and the list is a smallest one.
The seeded inputs are shown to expose the faults these regimes can hide: the fp64 oracle with the
last K slab of conv3's forward dropped, with conv_merge's K tail dropped, with the ragged column tile
of conv_merge's input gradient dropped, with the last image of a part-filled packed item missing from
conv3's weight gradient and with a slab reduce that stops one slab short moves the affected tensor
by more than ten times its bar."""
import numpy as np
import pytest
import torch

from oracle import a2c as oa2c
from oracle import few_env_cases as fc
from oracle import goal_trunk_cases as gc
from oracle import unreal_head_cases as uc
from oracle.policy import GoalNetOracle, frames_to_float

G84, G174, G300 = (84, 84), (174, 174), (300, 400)


def _r(hw, n, A=4):
    return gc.trunk_regime(hw, n, A)


def _at(hw, product, key):
    return [s[3] for s in gc.SWITCHES[hw] if s[1] == product and s[2] == key]


def test_geometry_constants():
    assert [fc.trunk_sizes(*hw) for hw in gc.GEOMETRIES] == [((20, 20), (9, 9), (3, 3)), ((42, 42), (20, 20), (9, 9)),
                                                              ((74, 99), (36, 48), (17, 23))]
    assert [fc.fcin(hw) for hw in gc.GEOMETRIES] == [288, 2592, 12512]
    assert gc.CAPS == {G84: 1030, G174: 260, G300: 40} and gc.FIRST_N == 18
    # images per item and bands per image of the persistent kernels, from the band structs
    assert [gc.conv3_wgrad_spec(hw) for hw in gc.GEOMETRIES] == [(3, 1, 2), (1, 1, 2), (2, 17, 2)]
    assert [gc.conv2_wgrad_spec(hw) for hw in gc.GEOMETRIES] == [(1, 1, 1), (1, 5, 1), (1, 36, 1)]
    assert [gc.parity_dgrad(hw) for hw in gc.GEOMETRIES] == [(4, 1), (2, 1), (1, 2)]   # ParityDg::IMG = 4 on the 4x4 class map
    assert [gc.conv1_fwd_bands(hw) for hw in gc.GEOMETRIES] == [1, 5, 19]              # 174x174: bands of 9, 9, 9, 9, 6 rows
    assert [gc.conv2_fwd_bands(hw) for hw in gc.GEOMETRIES] == [1, 1, 36]
    assert [gc.conv2_dgrad_bands(hw) for hw in gc.GEOMETRIES] == [1, 1, 10]            # 74 rows in bands of 8
    assert [gc.conv2_dgrad_threads(hw) for hw in gc.GEOMETRIES] == [256, 512, 256]


def test_regimes_are_the_restated_launch_rules():
    """trunk_regime is splitk_chunk / wgrad_chunk / reduce_lanes of oracle/unreal_head_cases.py on the
    goal trunk's shapes, nothing of its own."""
    for hw in gc.GEOMETRIES:
        (o3h, o3w), K5 = fc.trunk_sizes(*hw)[2], fc.fcin(hw)
        bm3 = 128 if o3h * o3w >= 64 else 64
        for n in gc.CASES[hw] + (64, 65, 255, 256):
            for A in (1, 4, 7):
                r, n9 = _r(hw, n, A), n * o3h * o3w
                assert (r["conv3_fwd"]["slabs"], r["conv3_fwd"]["kchunk"]) == uc.splitk_chunk(n9, 64, 1024, bm3, 64)
                assert (r["merge_fwd"]["slabs"], r["merge_fwd"]["kchunk"]) == uc.splitk_chunk(n, 512, K5, 64, 64)
                assert r["heads_fwd"]["slabs"] == uc.splitk(n, A + 1, 512, 64, 16) == 8
                big = K5 >= 1024 and n >= 256
                want = (1, 512) if big else uc.splitk_chunk(n, K5, 512, 64, 64)
                assert (r["merge_dgrad"]["slabs"], r["merge_dgrad"]["kchunk"]) == want
                assert r["merge_dgrad"]["tile"] == (128 if big else 64)
                assert r["heads_wgrad"]["slabs"] == uc.wgrad_slabs(A + 1, 512, n, 32, 64, True)
                assert r["merge_wgrad"]["slabs"] == uc.wgrad_slabs(512, K5, n, 128, 128, True)
                assert r["conv4_wgrad"]["slabs"] == uc.wgrad_slabs(32, 64, n9, 32, 64, True)
                assert r["conv4_wgrad"]["lanes"] == (uc.reduce_lanes(32, 65, r["conv4_wgrad"]["slabs"])
                                                     if r["conv4_wgrad"]["slabs"] > 1 else 0)
                for p, v in r.items():
                    if p in gc.PERSISTENT:
                        assert v["items"] > 0 and 2048 % v["threads"] == 0
                        continue
                    assert 0 < v["last"] <= v["kchunk"] and (v["lanes"] > 0) == (v["slabs"] > 1), (hw, n, p, v)
                    if v["slabs"] > 1:
                        assert v["kchunk"] % uc.BK == 0
        # the ragged column tile of conv_merge's input gradient: N = 4.5 / 40.5 / 195.5 tiles of 64
        assert _r(hw, 18)["merge_dgrad"]["col_rem"] == 32
    assert [fc.fcin(hw) / 64 for hw in gc.GEOMETRIES] == [4.5, 40.5, 195.5] and 2592 / 128 == 20.25


def test_switch_points_are_those_derived_from_the_launch_code():
    """The switch tables of DESIGN.md ("The goal trunk at every launch regime above 16 rows"), by
    value: the first n of each new regime."""
    # 84x84
    assert _at(G84, "conv3_fwd", "kchunk") == [242, 363, 520, 605, 726, 904]
    c3 = {n: _r(G84, n)["conv3_fwd"] for n in (18, 241, 242, 363, 520, 605, 726, 903, 904)}
    assert [(c3[n]["slabs"], c3[n]["kchunk"]) for n in (18, 241, 242, 363, 520, 605, 726, 903, 904)] == \
        [(16, 64), (16, 64), (11, 96), (8, 128), (7, 160), (6, 192), (5, 224), (5, 224), (1, 1024)]
    assert _at(G84, "merge_fwd", "kchunk") == [961]
    assert [(_r(G84, n)["merge_fwd"]["slabs"], _r(G84, n)["merge_fwd"]["kchunk"]) for n in (18, 960, 961)] == \
        [(3, 96), (3, 96), (1, 288)]
    assert 288 % 64 == 32  # the unsplit form's 64-wide K tile ends in half a tile
    assert _at(G84, "merge_dgrad", "kchunk") == [897] and _at(G84, "merge_dgrad", "tile") == []
    assert [(_r(G84, n)["merge_dgrad"]["slabs"], _r(G84, n)["merge_dgrad"]["kchunk"]) for n in (896, 897, 1280, 1281)] == \
        [(8, 64), (6, 96), (6, 96), (4, 128)]
    for p in ("heads_wgrad", "merge_wgrad"):
        assert _at(G84, p, "slabs3") == [257, 513]
        assert [_r(G84, n)[p]["slabs"] for n in (18, 256, 257, 512, 513)] == [1, 1, 2, 2, 3]
    assert _at(G84, "conv4_wgrad", "slabs3") == [29] and _at(G84, "conv4_wgrad", "lanes") == [29, 228, 456, 911]
    assert [_r(G84, n)["conv4_wgrad"]["lanes"] for n in (28, 29, 227, 228, 455, 456, 910, 911)] == [0, 1, 1, 2, 2, 4, 4, 8]
    assert _at(G84, "conv2_wgrad", "two_stage") == [32] and _at(G84, "conv3_wgrad", "two_stage") == [190]
    assert _at(G84, "heads_dgrad", "row_tiles>1") == [65]
    assert _at(G84, "conv3_fwd", "lanes") == [114, 904] and 114 * 9 * 64 >= uc.REDUCE_FLAT > 113 * 9 * 64
    # packing tails: 190 leaves a part-filled item of 3, 189 does not
    assert _r(G84, 190)["conv3_wgrad"]["part_item"] and not _r(G84, 189)["conv3_wgrad"]["part_item"]
    assert _r(G84, 190)["conv3_wgrad"]["items"] == 64 and _r(G84, 189)["conv3_wgrad"]["items"] == 63
    # 174x174
    assert _at(G174, "conv3_fwd", "kchunk") == [51, 74, 102, 116, 135, 162, 201]
    assert [(_r(G174, n)["conv3_fwd"]["slabs"], _r(G174, n)["conv3_fwd"]["kchunk"])
            for n in (18, 50, 51, 74, 102, 116, 135, 162, 200, 201)] == \
        [(16, 64), (16, 64), (11, 96), (8, 128), (7, 160), (6, 192), (5, 224), (4, 256), (4, 256), (1, 1024)]
    assert 16 * 81 * 51 * 64 > uc.SK_CAP >= 16 * 81 * 50 * 64  # 51: the sk_cap clamp of splitk_count, not the tile count
    assert _at(G174, "merge_fwd", "kchunk") == [129, 193, 257]
    assert [(_r(G174, n)["merge_fwd"]["slabs"], _r(G174, n)["merge_fwd"]["kchunk"]) for n in (18, 129, 193, 257)] == \
        [(27, 96), (21, 128), (14, 192), (12, 224)]
    assert uc.splitk_chunk(961, 512, 2592, 64, 64) == (1, 2592)
    assert _at(G174, "merge_dgrad", "kchunk") == [65, 129, 193] and _at(G174, "merge_dgrad", "tile") == [256]
    assert [(_r(G174, n)["merge_dgrad"]["slabs"], _r(G174, n)["merge_dgrad"]["kchunk"], _r(G174, n)["merge_dgrad"]["tile"])
            for n in (18, 65, 129, 193, 255, 256)] == \
        [(8, 64, 64), (6, 96, 64), (4, 128, 64), (1, 512, 64), (1, 512, 64), (1, 512, 128)]
    assert _at(G174, "conv4_wgrad", "lanes") == [26, 51, 102, 203]
    assert _at(G174, "conv3_wgrad", "two_stage") == [64] and _at(G174, "conv2_wgrad", "two_stage") == []
    assert _r(G174, 18)["conv2_wgrad"]["two_stage"]  # 10 n items: two-stage from n = 7 on
    assert _at(G174, "heads_wgrad", "slabs3") == _at(G174, "merge_wgrad", "slabs3") == [257]
    assert _at(G174, "merge_fwd", "lanes") == [128]
    # 300x400: conv_merge's input gradient is never split, on 64 x 64 tiles below 256 rows
    for n in (18, 37, 255):
        d = _r(G300, n)["merge_dgrad"]
        assert (d["slabs"], d["tile"], d["col_rem"]) == (1, 64, 32)
    assert _r(G300, 256)["merge_dgrad"]["tile"] == 128
    assert _at(G300, "conv3_fwd", "kchunk") == [21, 24, 28, 34]


def test_persistent_item_counts():
    """Items as a function of n, and the no-wrap / certain-wrap cases."""
    for n in (18, 37, 257):
        f = 2 * n
        assert {p: _r(G84, n)[p]["items"] for p in gc.PERSISTENT} == {
            "conv1_fwd": f, "conv2_fwd": f, "conv3_wgrad": -(-n // 3), "conv3_dgrad": -(-n // 4), "conv2_wgrad": f,
            "conv2_dgrad": f, "conv1_wgrad": f}
        assert {p: _r(G174, n)[p]["items"] for p in gc.PERSISTENT} == {
            "conv1_fwd": 5 * f, "conv2_fwd": f, "conv3_wgrad": n, "conv3_dgrad": -(-n // 2), "conv2_wgrad": 5 * f,
            "conv2_dgrad": f, "conv1_wgrad": 6 * f}
        assert {p: _r(G300, n)[p]["items"] for p in gc.PERSISTENT} == {
            "conv1_fwd": 19 * f, "conv2_fwd": 36 * f, "conv3_wgrad": 17 * -(-n // 2), "conv3_dgrad": 2 * n,
            "conv2_wgrad": 36 * f, "conv2_dgrad": 10 * f, "conv1_wgrad": 19 * f}
    for hw, n in gc.NO_WRAP_N.items():
        assert n in gc.CASES[hw] and not any(_r(hw, n)[p]["may_wrap"] for p in gc.PERSISTENT)
    # a certain wrap within the caps, and the case that runs it
    certain = {hw: {p: min(n for n in gc.CASES[hw] if _r(hw, n)[p]["must_wrap"]) for p in gc.PERSISTENT
                    if any(_r(hw, n)[p]["must_wrap"] for n in gc.CASES[hw])} for hw in gc.GEOMETRIES}
    assert certain == {G84: {"conv1_fwd": 1025, "conv1_wgrad": 1025, "conv2_dgrad": 1025, "conv2_fwd": 520, "conv2_wgrad": 520},
                       G174: {"conv1_fwd": 257, "conv1_wgrad": 193, "conv2_wgrad": 116},
                       G300: {"conv2_fwd": 18, "conv2_wgrad": 18}}
    # beyond the caps (the module's "Not covered"): the first n of a certain wrap
    assert not _r(G84, 4096)["conv3_dgrad"]["must_wrap"] and _r(G84, 4097)["conv3_dgrad"]["must_wrap"]
    assert not _r(G84, 1536)["conv3_wgrad"]["must_wrap"] and _r(G84, 1537)["conv3_wgrad"]["must_wrap"]
    assert _r(G174, 1025)["conv2_fwd"]["must_wrap"] and _r(G174, 513)["conv2_dgrad"]["must_wrap"]
    assert _r(G174, 2049)["conv3_dgrad"]["must_wrap"] and _r(G174, 513)["conv3_wgrad"]["must_wrap"]
    assert [min(n for n in range(1, 600) if _r(G300, n)[p]["must_wrap"]) for p in
            ("conv1_fwd", "conv3_wgrad", "conv2_dgrad", "conv3_dgrad")] == [54, 61, 103, 513]
    # one item per workgroup and fewer than kParts live slabs in the one-stage reduce
    assert _r(G84, 18)["conv3_wgrad"]["short_parts"] and _r(G84, 29)["conv3_wgrad"]["short_parts"]
    assert _r(G174, 18)["conv3_wgrad"]["short_parts"] and not _r(G174, 51)["conv3_wgrad"]["two_stage"]


@pytest.mark.parametrize("hw", (G84, G174), ids=("84x84", "174x174"))
def test_every_switch_has_a_case_on_each_side_and_every_case_is_needed(hw):
    cases = gc.CASES[hw]
    assert list(cases) == sorted(set(cases)) and cases[0] == gc.FIRST_N and cases[-1] <= gc.CAPS[hw]
    assert gc.uncovered(hw, cases) == []
    named = set()
    for what, product, key, at, below, above in gc.SWITCHES[hw]:
        a, b = gc._value(hw, at - 1, product, key), gc._value(hw, at, product, key)
        assert a != b and below[1] == at - 1 and above[0] == at, what
        lo = [n for n in cases if below[0] <= n <= below[1]]
        hi = [n for n in cases if above[0] <= n <= above[1]]
        assert lo and hi, what
        # the two sides are the regimes of the last n before and the first n past the switch
        assert all(gc._value(hw, n, product, key) == a for n in lo) and all(gc._value(hw, n, product, key) == b for n in hi)
        named |= {lo[-1], hi[0]}
    assert named == set(cases)
    # every case is needed: without it some switch loses a side
    for n in cases:
        assert gc.uncovered(hw, [m for m in cases if m != n]), n
    # and the list is a smallest one: the interval-stabbing count
    assert cases == gc.smallest_case_set(hw)
    # both packing tails occur among the cases
    img3, img_p = gc.conv3_wgrad_spec(hw)[0], gc.parity_dgrad(hw)[0]
    assert {n % img_p for n in cases} == set(range(img_p))
    if img3 > 1:
        for two in (False, True):
            assert {bool(n % img3) for n in cases if _r(hw, n)["conv3_wgrad"]["two_stage"] == two} == {False, True}


def test_300x400_cases_and_what_they_leave():
    assert gc.CASES[G300] == (18, gc.SECOND_300) and 30 <= gc.SECOND_300 <= 40
    assert tuple(gc.uncovered(G300, gc.CASES[G300])) == gc.UNCOVERED_300
    r = _r(G300, gc.SECOND_300)
    assert r["conv3_wgrad"]["part_item"] and r["conv3_fwd"]["kchunk"] == 256 and r["conv3_fwd"]["rem"] == 3
    # the chunk lengths it leaves are run by the same <128, 64> instance at 174x174
    assert {_r(G174, n)["conv3_fwd"]["kchunk"] for n in gc.CASES[G174]} >= {160, 192, 224}


def test_other_case_lists():
    assert gc.ACTION_CASES == [(G84, n, A) for n in (29, 257) for A in (1, 3, 7)]
    assert _r(G84, 257, 1)["heads_wgrad"]["slabs"] == 2 and _r(G84, 29, 7)["heads_wgrad"]["slabs"] == 1
    assert [hw for hw, _ in gc.ROWS_CASES] == list(gc.GEOMETRIES) and gc.ROWS_CASES[2] == (G300, 18)
    assert all(n in gc.CASES[hw] for hw, n in gc.ROWS_CASES + gc.GUARD_CASES)
    assert {(hw, n) for hw, n in gc.GUARD_CASES if n == 18} == {(hw, 18) for hw in gc.GEOMETRIES}
    two = [n for hw, n in gc.GUARD_CASES if hw == G84 and n != 18]
    assert len(two) == 1 and _r(G84, two[0])["conv3_wgrad"]["two_stage"] and _r(G84, two[0])["conv2_wgrad"]["two_stage"]
    for hw in gc.GEOMETRIES:
        assert len(gc.regime_table(hw)) == len(gc.CASES[hw])
    # the edges of the two-stage reduce: 63 (62 at 84x84's conv2) and exactly 64 slabs
    edge = [(hw, n, p) for hw, n in gc.EDGE_CASES for p in ("conv2_wgrad", "conv3_wgrad")
            if n + 1 in _at(hw, p, "two_stage") or n in _at(hw, p, "two_stage")]
    assert edge == [(G84, 31, "conv2_wgrad"), (G84, 32, "conv2_wgrad"), (G84, 189, "conv3_wgrad"),
                    (G84, 190, "conv3_wgrad"), (G174, 63, "conv3_wgrad"), (G174, 64, "conv3_wgrad")]
    assert [_r(hw, n)[p]["items"] for hw, n, p in edge] == [62, 64, 63, 64, 63, 64]
    assert [_r(hw, n)[p]["two_stage"] for hw, n, p in edge] == [False, True] * 3


def test_inputs_are_reproducible_and_placed():
    for hw, n in gc.ROWS_CASES[:2]:
        arena, ri, rg = gc.arena_rows(hw, n)
        arena2, ri2, rg2 = gc.arena_rows(hw, n)
        assert np.array_equal(arena, arena2) and np.array_equal(ri, ri2) and np.array_equal(rg, rg2)
        R = arena.shape[0]
        assert arena.shape == (R,) + hw + (3,) and arena.dtype == np.uint8 and R < n
        assert ri.dtype == rg.dtype == np.int32 and ri[0] == 0 and rg[n - 1] == R - 1
        assert len(set(ri.tolist())) < n and len(set(rg.tolist())) < n   # rows repeat
        assert set(ri.tolist()) & set(rg.tolist())                       # and are shared between the two lists
        assert 0 <= min(ri.min(), rg.min()) and max(ri.max(), rg.max()) == R - 1


# ---- the faults these regimes can hide, in float64 ----------------------------------------------------
def _oracle_case(hw, n, A=4):
    """The fp64 oracle of one case with parameters of the law the GPU test draws (U(+-1/sqrt(fan_in)) +
    N(0, 0.01) on every tensor), the case's seeded frames and loss inputs."""
    torch.manual_seed(fc.weight_seed(hw, n, A))
    ref = GoalNetOracle(hw, 3, A)
    with torch.no_grad():
        for p in ref.parameters():
            p.add_(torch.randn_like(p) * 0.01)
    ref = ref.double()
    img, gl = (frames_to_float(torch.as_tensor(f)).double() for f in fc.u8_frames(hw, n))
    actions, rets = (torch.as_tensor(v) for v in fc.loss_inputs(n, A))
    return ref, img, gl, actions.long(), rets.double()


def _trunk(ref, img, gl):
    x2 = torch.cat([torch.relu(ref.conv2(torch.relu(ref.conv1(x)))) for x in (img, gl)], 1)
    z3 = ref.conv3(x2)
    x3 = torch.relu(z3)
    z4 = ref.conv4(x3)
    x4 = torch.relu(z4)
    x5 = torch.relu(ref.fc(x4.flatten(1)))
    return x2, z3, x3, z4, x4, x5


def _moved(a, b):
    return float((a - b).abs().max() / a.abs().max())


def test_inputs_expose_the_faults_at_84():
    """n = 29 at 84x84 (the smallest case with n mod 3 != 0; conv3 forward 16 x 64, conv_merge forward
    3 x 96, conv4's weight gradient on 2 slabs of 160 rows). A condition on the seeded inputs: a seed
    that fails it is replaced, the factor stays."""
    hw, n, A = G84, 29, 4
    r = _r(hw, n)
    ref, img, gl, actions, rets = _oracle_case(hw, n, A)
    x2, z3, x3, z4, x4, x5 = _trunk(ref, img, gl)
    loss, _ = oa2c.loss(ref.policy_logits(x5), ref.critic(x5).view(-1), actions, rets)
    g3, g4, gx4 = torch.autograd.grad(loss, (z3, z4, x4), retain_graph=True)

    # 1. conv3's forward without its last K slab: K runs [ky][kx][64 channels], the last 64 are tap (3, 3)
    assert (r["conv3_fwd"]["slabs"], r["conv3_fwd"]["last"]) == (16, 64)
    with torch.no_grad():
        w = ref.conv3.weight.clone()
        w[:, :, 3, 3] = 0.0
        cut = torch.relu(torch.nn.functional.conv2d(x2, w, ref.conv3.bias, stride=2))
        m = _moved(x3, cut)
    assert m > 10 * 1e-5, "X3 moves by %.3g of scale" % m

    # 2. conv_merge's forward without the K tail: the unsplit form's 64-wide K tile forced on the split
    #    product's chunks of 96 loses the last half tile, the 32 channels of pixel (2, 2)
    assert r["merge_fwd"]["kchunk"] == 96 and 288 % 64 == 32
    with torch.no_grad():
        cut = x4.clone()
        cut[:, :, 2, 2] = 0.0
        m = _moved(x5, torch.relu(ref.fc(cut.flatten(1))))
    assert m > 10 * 1e-5, "X5 moves by %.3g of scale" % m

    # 3. conv_merge's input gradient without its ragged column tile (columns 256..287 of the kernels' NHWC
    #    rows: pixel (2, 2)), seen in conv4's weight gradient behind it
    assert r["merge_dgrad"]["col_rem"] == 32
    a, = torch.autograd.grad(z4, ref.conv4.weight, grad_outputs=g4, retain_graph=True)
    g4c = g4.clone()
    g4c[:, :, 2, 2] = 0.0
    b, = torch.autograd.grad(z4, ref.conv4.weight, grad_outputs=g4c, retain_graph=True)
    assert _moved(a, b) > 10 * 1e-4, "conv4 weight gradient moves by %.3g of scale" % _moved(a, b)

    # 4. conv3's weight gradient without the last image of its part-filled item (3 images per item, 29 = 9 x 3 + 2)
    assert r["conv3_wgrad"]["part_item"] and r["conv3_wgrad"]["img"] == 3 and r["conv3_wgrad"]["items"] == 10
    a, = torch.autograd.grad(z3, ref.conv3.weight, grad_outputs=g3, retain_graph=True)
    g3c = g3.clone()
    g3c[n - 1] = 0.0
    b, = torch.autograd.grad(z3, ref.conv3.weight, grad_outputs=g3c, retain_graph=True)
    assert _moved(a, b) > 10 * 1e-4, "conv3 weight gradient moves by %.3g of scale" % _moved(a, b)

    # 5. a slab reduce that stops one slab short: conv3's x6 slabs are its items (the last one: images 27, 28) ...
    g3c = g3.clone()
    g3c[27:] = 0.0
    b, = torch.autograd.grad(z3, ref.conv3.weight, grad_outputs=g3c, retain_graph=True)
    assert _moved(a, b) > 10 * 1e-4, "conv3 weight gradient moves by %.3g of scale" % _moved(a, b)
    #    ... conv4's are kchunk rows of the [n 9][32] dZ4 rows (NHWC): 2 slabs of 160, the last holds rows 160..260
    w4 = r["conv4_wgrad"]
    assert (w4["slabs"], w4["kchunk"], w4["last"]) == (2, 160, 101)
    dz = g4.permute(0, 2, 3, 1).reshape(n * 9, 32)
    xr = x3.detach().permute(0, 2, 3, 1).reshape(n * 9, 64)
    full = dz.t() @ xr
    a, = torch.autograd.grad(z4, ref.conv4.weight, grad_outputs=g4, retain_graph=True)
    assert _moved(a.reshape(32, 64), full) < 1e-12
    short = dz[:160].t() @ xr[:160]
    assert _moved(full, short) > 10 * 1e-4, "conv4 weight gradient moves by %.3g of scale" % _moved(full, short)
    db, dbs = dz.sum(0), dz[:160].sum(0)
    assert _moved(db, dbs) > 10 * 1e-4


def test_inputs_expose_the_ragged_column_tile_at_174():
    """n = 18 at 174x174: conv_merge's input gradient has N = 2592 = 40.5 column tiles of 64; without the
    last half tile (pixel (8, 8) of the 9x9 map) conv4's weight gradient moves by more than ten bars."""
    hw, n, A = G174, 18, 4
    assert _r(hw, n)["merge_dgrad"]["col_rem"] == 32 and 2592 - 32 == (8 * 9 + 8) * 32
    ref, img, gl, actions, rets = _oracle_case(hw, n, A)
    x2, z3, x3, z4, x4, x5 = _trunk(ref, img, gl)
    loss, _ = oa2c.loss(ref.policy_logits(x5), ref.critic(x5).view(-1), actions, rets)
    g4, = torch.autograd.grad(loss, (z4,), retain_graph=True)
    a, = torch.autograd.grad(z4, ref.conv4.weight, grad_outputs=g4, retain_graph=True)
    g4c = g4.clone()
    g4c[:, :, 8, 8] = 0.0
    b, = torch.autograd.grad(z4, ref.conv4.weight, grad_outputs=g4c, retain_graph=True)
    assert _moved(a, b) > 10 * 1e-4, "conv4 weight gradient moves by %.3g of scale" % _moved(a, b)
    # conv3's forward without its last K slab (16 x 64 on the <128, 64> instance)
    assert (_r(hw, n)["conv3_fwd"]["slabs"], _r(hw, n)["conv3_fwd"]["last"]) == (16, 64)
    with torch.no_grad():
        w = ref.conv3.weight.clone()
        w[:, :, 3, 3] = 0.0
        m = _moved(x3, torch.relu(torch.nn.functional.conv2d(x2, w, ref.conv3.bias, stride=2)))
    assert m > 10 * 1e-5, "X3 moves by %.3g of scale" % m
