"""tests/resize_ref.py (the project's statement of the ingest resize) against scipy and against
the reference's recorded skimage outputs, CPU only.

(a) its Gaussian stage equals scipy.ndimage.gaussian_filter on uint8, mode="mirror", bit for bit;
(b) its bytes against tests/golden/resize.npz (skimage.transform.resize, anti_aliasing=True,
    recorded by tests/golden/gen_resize_goldens.py);
(c) against the cached env's own 100 -> 84 frames in ingest.npz;
(d) the inputs exercise both branches of the tie rule.
The bounds of (b): a stored byte is round(255 x), so it lies within 0.5 of 255 x wherever the
filtered bytes agree with the recording installation's; on flat regions those may differ by one
between installations (DESIGN.md "Scene ingest"), which moves an output by at most 1."""
import numpy as np
import pytest
from scipy import ndimage

import resize_ref as rr

RAND_SHAPES = ((17, 23), (59, 79), (12, 80), (21, 21))
FLAT_SHAPES = ((11, 10), (40, 13), (17, 36), (7, 5))
SIGMA_PAIRS = ((1.2857, 1.2857), (0.3621, 0.5), (2.0, 0.7))


def frame_kinds():
    """flat, piecewise-flat and random 40x36x3 frames, [N, 40, 36, 3] uint8."""
    rng = np.random.RandomState(7)
    flat = np.array([0, 1, 77, 128, 192, 254, 255], dtype=np.uint8)[:, None, None, None] \
        * np.ones((1, 40, 36, 3), dtype=np.uint8)
    piece = rng.randint(0, 256, size=(4, 8, 6, 3)).astype(np.uint8).repeat(5, axis=1).repeat(6, axis=2)
    rand = rng.randint(0, 256, size=(4, 40, 36, 3)).astype(np.uint8)
    return {"flat": flat, "piecewise": piece, "random": rand}


def scipy_gaussian(frames, sr, sc):
    return np.stack([ndimage.gaussian_filter(f, (sr, sc, 0), mode="mirror") for f in frames])


@pytest.mark.parametrize("sigmas", SIGMA_PAIRS)
def test_gaussian_stage_equals_scipy(sigmas):
    taps_rc = (rr.taps_sigma(sigmas[0])[1], rr.taps_sigma(sigmas[1])[1])
    for kind, frames in frame_kinds().items():
        got = rr.gaussian_u8(frames, taps_rc=taps_rc)
        want = scipy_gaussian(frames, *sigmas)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (kind, int((got != want).sum()))


@pytest.mark.parametrize("n", (1, 2, 3, 5))
def test_gaussian_mirror_beyond_one_reflection(n):
    """Extents smaller than the radius: sigma = 2 gives R = 8 (5 -> 1 rows: the mirror period
    is 8; n = 3 reflects four times; n = 1 reads sample 0 everywhere), on either axis."""
    rng = np.random.RandomState(n)
    R, w = rr.taps_sigma(2.0)
    assert R == 8 and rr.taps(5, 1)[:2] == (2.0, 8)
    x = rng.randint(0, 256, size=(3, n, 9, 3)).astype(np.uint8)
    assert np.array_equal(rr.gaussian_u8(x, taps_rc=(w, None)), scipy_gaussian(x, 2.0, 0))
    xt = np.ascontiguousarray(x.transpose(0, 2, 1, 3))
    assert np.array_equal(rr.gaussian_u8(xt, taps_rc=(None, w)), scipy_gaussian(xt, 0, 2.0))
    assert np.array_equal(rr.gaussian_u8(x, taps_rc=(w, w)), scipy_gaussian(x, 2.0, 2.0))


def test_mirror_index():
    assert rr.mirror(np.arange(-9, 14), 5).tolist() == [1, 0, 1, 2, 3, 4, 3, 2, 1, 0, 1, 2, 3, 4, 3, 2, 1, 0, 1, 2,
                                                        3, 4, 3]
    assert rr.mirror(np.arange(-3, 4), 1).tolist() == [0] * 7
    assert rr.mirror(np.arange(-3, 5), 2).tolist() == [1, 0, 1, 0, 1, 0, 1, 0]


def test_taps_follow_the_shapes():
    assert rr.taps(100, 84)[:2] == ((100 / 84 - 1) / 2, 0) and rr.taps(100, 84)[2].tolist() == [1.0]
    assert rr.taps(40, 40) == (0.0, 0, None)
    s, R, w = rr.taps(300, 84)
    assert R == 5 and len(w) == 11 and abs(w.sum() - 1) < 1e-15 and np.array_equal(w, w[::-1])
    assert rr.taps(1600, 100)[1] == 30  # a factor of 16


@pytest.mark.parametrize("hw", RAND_SHAPES)
def test_random_frames_against_reference(golden, hw):
    d = golden("resize.npz")
    want = 255.0 * d["rand_out_%dx%d" % hw]
    got = rr.resize(d["rand_in"], hw)
    err = np.abs(got.astype(np.float64) - want).max()
    print("random %s: max |byte - 255 ref| = 0.5 + %.3g" % (hw, err - 0.5))
    assert err <= 0.5 + 1e-9, err


@pytest.mark.parametrize("hw", FLAT_SHAPES)
def test_flat_frames_against_reference(golden, hw):
    d = golden("resize.npz")
    want = 255.0 * d["flat_out_%dx%d" % hw]
    got = rr.resize(d["flat_in"], hw)
    err = np.abs(got.astype(np.float64) - want)
    above = int((err > 0.5 + 1e-9).sum())
    print("flat %s: max %.6g, %d of %d outputs above 0.5 (%.4f %%)" % (hw, err.max(), above, err.size,
                                                                        100.0 * above / err.size))
    assert err.max() <= 1.5, err.max()
    assert above <= 0.01 * err.size, (above, err.size)


def test_cached_env_frames_against_reference(golden):
    """The cached env's own _preprocess_frame outputs at 100 -> 84 (ingest.npz, float32)."""
    d = golden("ingest.npz")
    got = rr.resize(d["r_frames"][d["r_pick"]], (84, 84))
    err = np.abs(got.astype(np.float64) - 255.0 * d["r_expected"].astype(np.float64)).max()
    print("cached env 100 -> 84: max |byte - 255 ref| = %.6g" % err)
    assert err <= 0.5 + 1e-4, err


def test_inputs_exercise_both_tie_branches(golden):
    d = golden("resize.npz")
    even = odd = 0
    for frames, shapes in ((d["rand_in"], RAND_SHAPES), (d["flat_in"], FLAT_SHAPES)):
        for hw in shapes:
            S, D = rr.bilinear_sd(rr.gaussian_u8(frames, out_hw=hw), hw)
            e, o = rr.tie_counts(S, D)
            even, odd = even + e, odd + o
    print("exact ties: %d with an even quotient, %d with an odd one" % (even, odd))
    assert even >= 1 and odd >= 1
    # the rule itself on hand-made quotients: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, above / below a tie
    S = np.array([1, 3, 5, 7, 11, 9], dtype=np.int64)
    assert rr.round_half_even(S, 2).tolist() == [0, 2, 2, 4, 6, 4]
    assert rr.round_half_even(np.array([5, 7, 249 * 4 + 2]), 4).tolist() == [1, 2, 250]
