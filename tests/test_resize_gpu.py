"""vn_resize_frames on the GPU, bit for bit against tests/resize_ref.py (the project's numpy
statement of the ingest resize): through the C ABI via ctypes, with guard bytes round the
destination, and through vnav.scenes.resize_frames."""
import ctypes

import numpy as np
import pytest
import torch

import resize_ref as rr
from test_resize_refs import FLAT_SHAPES, RAND_SHAPES

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5


def _dptr(w):
    return None if w is None else np.ascontiguousarray(w).ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def call_cabi(src_t, n, h, w, c, oh, ow, tr, rr_, tc, rc, dst_t):
    from vnav import _lib
    return _lib.load().vn_resize_frames(_lib.ptr(src_t), n, h, w, c, oh, ow, _dptr(tr), rr_, _dptr(tc), rc,
                                        _lib.ptr(dst_t), _lib.stream_ptr(torch.device("cuda", 0)))


def resize_cabi(frames, hw, src_offset=0):
    """vn_resize_frames on frames [N,H,W,C] with resize_ref's taps; the source starts src_offset
    bytes into its allocation, the destination GUARD bytes into one filled with FILL. Returns
    the output after checking that the guards on both sides are untouched."""
    frames = np.ascontiguousarray(frames, dtype=np.uint8)
    n, h, w, c = frames.shape
    oh, ow = hw
    buf = torch.zeros(frames.size + src_offset, dtype=torch.uint8, device="cuda")
    src = buf[src_offset:]
    src.copy_(torch.from_numpy(frames.reshape(-1)))
    out_bytes = n * oh * ow * c
    guarded = torch.full((out_bytes + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")
    dst = guarded[GUARD:GUARD + out_bytes]
    _, r_r, t_r = rr.taps(h, oh)
    _, r_c, t_c = rr.taps(w, ow)
    rc = call_cabi(src, n, h, w, c, oh, ow, t_r, r_r, t_c, r_c, dst)
    torch.cuda.synchronize()
    from vnav import _lib
    assert rc == 0, _lib.last_error()
    g = guarded.cpu().numpy()
    assert (g[:GUARD] == FILL).all() and (g[GUARD + out_bytes:] == FILL).all(), "guard bytes overwritten"
    return g[GUARD:GUARD + out_bytes].reshape(n, oh, ow, c)


def check_both(frames, hw, **kw):
    from vnav import scenes
    want = rr.resize(frames, hw)
    got = resize_cabi(frames, hw)
    assert np.array_equal(got, want), ("C ABI", frames.shape, hw, int((got != want).sum()))
    got = scenes.resize_frames(frames, hw, **kw)
    assert got.dtype == np.uint8 and np.array_equal(got, want), ("resize_frames", frames.shape, hw)
    return want


@pytest.mark.parametrize("hw", RAND_SHAPES)
def test_random_golden_shapes(golden, hw):
    check_both(golden("resize.npz")["rand_in"], hw)


@pytest.mark.parametrize("hw", FLAT_SHAPES)
def test_flat_golden_shapes(golden, hw):
    check_both(golden("resize.npz")["flat_in"], hw)


def test_radius_zero_on_both_axes(golden):
    """100 -> 84: sigma = 0.095, R = 0, the one tap 1.0 on each axis."""
    assert rr.taps(100, 84)[1] == 0 and rr.taps(100, 84)[2] is not None
    check_both(golden("ingest.npz")["r_frames"][:2], (84, 84))


def test_axis_unchanged_and_copy():
    rng = np.random.RandomState(0)
    x = rng.randint(0, 256, size=(2, 40, 36, 3)).astype(np.uint8)
    assert rr.taps(40, 40)[2] is None
    check_both(x, (40, 13))  # rows pass skipped
    check_both(x, (11, 36))  # columns pass skipped
    assert np.array_equal(check_both(x, (40, 36)), x)  # the plain copy


def test_one_channel_odd_sizes():
    x = np.random.RandomState(1).randint(0, 256, size=(3, 31, 45, 1)).astype(np.uint8)
    check_both(x, (9, 14))


@pytest.mark.parametrize("shape,hw", (((5, 7), (1, 1)), ((1, 9), (1, 4))))
def test_extents_below_the_radius(shape, hw):
    for c in (1, 3):
        x = np.random.RandomState(2).randint(0, 256, size=(2,) + shape + (c,)).astype(np.uint8)
        check_both(x, hw)


def test_frame_counts_and_ragged_chunks():
    x = np.random.RandomState(3).randint(0, 256, size=(5, 23, 30, 3)).astype(np.uint8)
    check_both(x[:1], (10, 11))
    check_both(x, (10, 11), chunk_frames=2)  # chunks of 2, 2, 1


@pytest.mark.parametrize("shape,hw", (((300, 400), (84, 84)), ((300, 300), (174, 174))))
def test_real_frame_sizes(shape, hw):
    """The cached-THOR dump sizes: several bands of output rows per frame, R = 5 / 8 and R = 1."""
    rng = np.random.RandomState(4)
    x = rng.randint(0, 256, size=(2,) + shape + (3,)).astype(np.uint8)
    x[1, :, : shape[1] // 2] = rng.randint(0, 256, size=(1, 1, 3))  # a flat half
    check_both(x, hw)


def test_source_at_odd_byte_offset():
    x = np.random.RandomState(5).randint(0, 256, size=(2, 33, 50, 3)).astype(np.uint8)
    got = resize_cabi(x, (12, 17), src_offset=1)
    assert np.array_equal(got, rr.resize(x, (12, 17)))


def test_two_runs_are_bitwise_equal():
    x = np.random.RandomState(6).randint(0, 256, size=(3, 60, 80, 3)).astype(np.uint8)
    assert np.array_equal(resize_cabi(x, (17, 23)), resize_cabi(x, (17, 23)))


def test_refusals_write_nothing():
    from vnav import _lib
    h, w = 12, 10
    src = torch.zeros(2 * h * w * 3, dtype=torch.uint8, device="cuda")
    dst = torch.full((2 * h * w * 4,), FILL, dtype=torch.uint8, device="cuda")
    big = np.full(2 * 33 + 1, 1.0 / 67)
    one = np.array([1.0])
    cases = {  # the caps are VN_RESIZE_MAX_RADIUS = 32 and VN_RESIZE_MAX_ROW_BYTES = 24576 (include/vnav.h)
        "upsampled rows": (src, 2, h, w, 3, h + 1, w, one, 0, one, 0, dst),
        "upsampled columns": (src, 2, h, w, 3, h, w + 1, one, 0, one, 0, dst),
        "two channels": (src, 2, h, w, 2, 6, 5, one, 0, one, 0, dst),
        "four channels": (src, 1, h, w, 4, 6, 5, one, 0, one, 0, dst),
        "no frames": (src, 0, h, w, 3, 6, 5, one, 0, one, 0, dst),
        "negative count": (src, -1, h, w, 3, 6, 5, one, 0, one, 0, dst),
        "zero height": (src, 2, 0, w, 3, 6, 5, one, 0, one, 0, dst),
        "zero width": (src, 2, h, 0, 3, 6, 5, one, 0, one, 0, dst),
        "zero output height": (src, 2, h, w, 3, 0, 5, one, 0, one, 0, dst),
        "negative output width": (src, 2, h, w, 3, 6, -5, one, 0, one, 0, dst),
        "zero channels": (src, 2, h, w, 0, 6, 5, one, 0, one, 0, dst),
        "rows radius above the cap": (src, 2, h, w, 3, 6, 5, big, 33, one, 0, dst),
        "columns radius above the cap": (src, 2, h, w, 3, 6, 5, one, 0, big, 33, dst),
        "negative radius": (src, 2, h, w, 3, 6, 5, one, -1, one, 0, dst),
        "radius without taps": (src, 2, h, w, 3, 6, 5, None, 2, one, 0, dst),
        "row wider than the cap": (src, 1, 1, 24577, 1, 1, 5, one, 0, one, 0, dst),
        "NULL source": (None, 2, h, w, 3, 6, 5, one, 0, one, 0, dst),
        "NULL destination": (src, 2, h, w, 3, 6, 5, one, 0, one, 0, None),
    }
    for name, args in cases.items():
        assert call_cabi(*args) != 0, name
        assert "vn_resize_frames" in _lib.last_error(), name
    torch.cuda.synchronize()
    assert bool((dst == FILL).all()), "a refused call wrote to the destination"


def test_radius_cap_covers_a_factor_of_16():
    """16x per axis is R = 30, inside the cap of 32: 64 x 48 -> 4 x 3, and 17x (R = 32) on rows."""
    x = np.random.RandomState(8).randint(0, 256, size=(1, 64, 48, 3)).astype(np.uint8)
    assert rr.taps(64, 4)[1] == 30
    check_both(x, (4, 3))
    y = np.random.RandomState(9).randint(0, 256, size=(1, 34, 6, 1)).astype(np.uint8)
    assert rr.taps(34, 2)[1] == 32
    check_both(y, (2, 6))


def test_resize_frames_rejects_upsampling_and_bad_shapes():
    from vnav import VnavError, scenes
    x = np.zeros((1, 8, 8, 3), dtype=np.uint8)
    with pytest.raises(VnavError):
        scenes.resize_frames(x, (9, 8))
    with pytest.raises(ValueError):
        scenes.resize_frames(x[0], (4, 4))
    assert scenes.resize_frames(x[:0], (4, 4)).shape == (0, 4, 4, 3)
    for n, no in ((300, 84), (100, 84), (40, 40)):
        mine, ref = scenes.resize_taps(n, no), rr.taps(n, no)
        assert mine[:2] == ref[:2] and (mine[2] is None) == (ref[2] is None)
        assert mine[2] is None or np.array_equal(mine[2], ref[2])
