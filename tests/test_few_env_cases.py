"""The conditions the cases of tests/test_few_env_gpu.py rest on, checked on the CPU from the
same formulas as the code (csrc/vn_skinny.h: the row instances of launch_skinny, skinny_kc
and the register counts of launch_skinny_lpc; the trunk geometry), and the fp64 oracle's
masked forward against its plain one."""
import numpy as np
import pytest
import torch

from oracle import few_env_cases as fc
from oracle.policy import GoalNetOracle, trunk_sizes


def test_tables_hold_what_the_issue_sets():
    assert len(fc.TRUNK_CASES) == len(set(fc.TRUNK_CASES)) == 5 + 6 + 6 + 6
    for hw, n, A in fc.TRUNK_CASES:
        want = fc.ACTION_COUNTS if (hw == (84, 84) and n in (5, 17)) else (4,)
        assert A in want
    assert {(E, T) for E, T, A, nul, x in fc.LSTM_CASES if A == 4 and not nul and not x} == \
        {(1, 1), (1, 3), (4, 3), (8, 2), (9, 3), (16, 1), (17, 1), (17, 3)}
    assert {(E, T, A) for E, T, A, nul, x in fc.LSTM_CASES if A != 4} == {(5, 3, 1), (5, 3, 3), (5, 3, 7)}
    assert {(E, T) for E, T, A, nul, x in fc.LSTM_CASES if nul} == {(4, 3), (17, 3)}
    assert {(E, x, T) for E, T, A, nul, x in fc.LSTM_CASES if x} == {(9, 4, 3), (17, 17, 3)}
    assert len(fc.LSTM_IDS) == len(set(fc.LSTM_IDS)) and len(fc.TRUNK_IDS) == len(set(fc.TRUNK_IDS))


@pytest.mark.parametrize("hw", fc.GEOMETRIES, ids=[fc.GEO_IDS[hw] for hw in fc.GEOMETRIES])
def test_n_lists_sit_on_both_sides_of_every_row_switch(hw):
    """launch_skinny switches at M <= 4, <= 8, <= 16, and the callers leave the VALU path past
    16: every instance (and the tensor-core path) is run, and every switch has a case at its
    last row count or the first of the next instance. 174x174 has no n = 4 and 300x400 no n = 8
    in the issue's table; 5 / 9 then stand on the far side of those switches and 1 / 5 on the
    near side."""
    ns = fc.TRUNK_N[hw]
    assert {fc.row_instance(n) for n in ns} == {4, 8, 16, None}
    for lo in fc.ROW_INSTANCES:  # the switch between lo and lo + 1 rows
        near = [n for n in ns if fc.row_instance(n) == lo]
        far = [n for n in ns if n > lo]
        assert near and far
        assert max(near) == lo or min(far) == lo + 1
    assert 16 in ns and 17 in ns  # the 16 | 17 switch to the tensor-core path: both sides exactly
    if hw == (84, 84):
        assert {4, 5, 8, 9} <= set(ns)


@pytest.mark.parametrize("hw", fc.GEOMETRIES, ids=[fc.GEO_IDS[hw] for hw in fc.GEOMETRIES])
def test_odd_n_gives_an_odd_pixel_count(hw):
    """conv34_small_kernel takes C34_ROWS = 2 output pixels per workgroup: an odd number of
    pixels leaves the last workgroup one live row."""
    o3 = trunk_sizes(*hw)[2]
    assert fc.trunk_sizes(*hw) == trunk_sizes(*hw)
    assert o3[0] * o3[1] == {(84, 84): 9, (174, 174): 81, (300, 400): 391}[hw]
    odd = [n for n in fc.TRUNK_N[hw] if n % 2]
    assert odd
    for n in odd:
        assert (n * o3[0] * o3[1]) % fc.C34_ROWS == 1
    assert any(n <= fc.SKINNY_ROWS for n in odd)


def test_conv_merge_k_at_300x400_leaves_a_last_chunk_for_every_row_instance():
    assert fc.fcin((84, 84)) == 288 and fc.fcin((174, 174)) == 2592 and fc.fcin((300, 400)) == 12512
    seen = set()
    for n in fc.TRUNK_N[(300, 400)]:
        if n > fc.SKINNY_ROWS:
            continue
        kc, full, rem = fc.conv_merge_chunks((300, 400), n)
        assert kc * fc.row_instance(n) * 4 <= 128 * 1024 and kc % 512 == 0
        assert full >= 2 and rem == 224, (n, kc, full, rem)  # several chunks + a 224-value remainder
        seen.add(fc.row_instance(n))
    assert seen == {4, 8, 16}
    # the other geometries: one chunk (84x84: 288 values, KB = 4) / two (174x174: 2592, KB = 8)
    assert fc.conv_merge_chunks((84, 84), 4) == (2048, 0, 288)
    assert fc.conv_merge_chunks((174, 174), 4)[1:] == (0, 2592)
    assert fc.conv_merge_chunks((174, 174), 16) == (2048, 1, 544)


def test_placed_masks_contain_the_resets():
    for E, T, A, nul, x in fc.LSTM_CASES:
        m = fc.lstm_masks(E, T)
        assert m.shape == (T, E) and set(np.unique(m)) <= {0.0, 1.0}
        if E == 1:
            assert (m[:, 0] == 0).nonzero()[0].tolist() == ([1] if T >= 2 else [])
            continue
        assert m[0, 0] == 0 and m[T - 1, E - 1] == 0
        want = 2
        if T >= 3:
            assert m[1, E // 2] == 0
            want = 3
        assert int((m == 0).sum()) == want
    assert any(T >= 3 and E > 1 for E, T, A, nul, x in fc.LSTM_CASES)


def test_xcat_pad_widths():
    for A, pad in fc.XCAT_PAD.items():
        lin = 512 + A + 1
        assert (lin + 3) // 4 * 4 - lin == pad
    assert [fc.XCAT_PAD[A] for A in fc.ACTION_COUNTS] == [2, 0, 0]


def test_float_frames_are_off_the_u8_grid():
    for hw, n in fc.FLOAT_CASES:
        for f in fc.float_frames(hw, n):
            assert f.dtype == np.float32 and f.shape == (n, 3) + hw and 0.0 <= f.min() and f.max() < 1.0
            k = np.rint(f.astype(np.float64) * 255.0)
            off = np.abs(f - (k / 255.0).astype(np.float32)) > 1e-4
            assert off.mean() > 0.9  # nearly every value is far from a multiple of 1/255


@pytest.mark.parametrize("hw", fc.GEOMETRIES, ids=[fc.GEO_IDS[hw] for hw in fc.GEOMETRIES])
def test_masked_forward_with_own_signs_equals_forward(hw):
    """GoalNetOracle.forward_masked fed the signs of its own pre-activations is forward."""
    torch.manual_seed(11)
    ref = GoalNetOracle(hw, 3, 3).double()
    img, gl = (torch.as_tensor(f).double() for f in fc.float_frames(hw, 3))
    with torch.no_grad():
        logits, value = ref(img, gl)
        z1 = [ref.conv1(v) for v in (img, gl)]
        z2 = [ref.conv2(torch.relu(z)) for z in z1]
        z3 = ref.conv3(torch.cat([torch.relu(z) for z in z2], 1))
        z4 = ref.conv4(torch.relu(z3))
        z5 = ref.fc(torch.relu(z4).flatten(1))
        masks = {"m1i": z1[0] > 0, "m1g": z1[1] > 0, "m2i": z2[0] > 0, "m2g": z2[1] > 0, "m3": z3 > 0, "m4": z4 > 0,
                 "m5": z5 > 0}
        masks = {k: v.double() for k, v in masks.items()}
        ml, mv, x4, pre = ref.forward_masked(img, gl, masks)
    for a, b in ((ml, logits), (mv, value), (pre["z5"], z5), (x4, torch.relu(z4))):
        assert float((a - b).abs().max()) <= 1e-12 * max(float(b.abs().max()), 1.0)
