"""The frame resize of the scene ingest, stated in numpy (DESIGN.md "Scene ingest: resize on
the device"). This is the project's own statement of what vn_resize_frames computes; it calls
neither scipy nor scikit-image. tests/test_resize_refs.py holds it to both on the CPU, the GPU
tests hold the kernel to it bit for bit.

  1. Gaussian on the uint8 image, rows axis then columns axis, each axis's fp64 result floored
     back to uint8 (scipy.ndimage.gaussian_filter on a uint8 array, mode="mirror");
  2. bilinear sampling at r = (i + 0.5) H / Ho - 0.5, c = (j + 0.5) W / Wo - 0.5;
  3. the byte round(255 x), defined in integers: S / D to nearest, ties to even.
"""
import numpy as np


def taps_sigma(sigma):
    """(R, w) of one axis: w is None when the axis is skipped (sigma <= 1e-15), else the 2R+1
    normalised fp64 weights."""
    if sigma <= 1e-15:
        return 0, None
    R = int(4.0 * sigma + 0.5)
    k = np.arange(-R, R + 1)
    w = np.exp(-0.5 / (sigma * sigma) * k ** 2)
    return R, w / w.sum()


def taps(n, no):
    """(sigma, R, w): the axis's Gaussian for n -> no samples."""
    sigma = max(0.0, (n / no - 1) / 2)
    return (sigma,) + taps_sigma(sigma)


def mirror(i, n):
    """Mirror without repeating the edge sample: period 2 (n - 1), any number of reflections."""
    i = np.asarray(i, dtype=np.int64)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    m = np.mod(i, p)
    return np.where(m < n, m, p - m)


def filter_axis(x, axis, w):
    """One pass of the symmetric correlation along `axis` of a uint8 array, floored to uint8:
    acc = x[i] w[R]; acc += (x[i+j] + x[i-j]) w[j+R] for j = -R..-1, fp64, every product and
    sum rounded on its own."""
    R = (len(w) - 1) // 2
    n = x.shape[axis]
    xf = np.moveaxis(x, axis, 0).astype(np.float64)
    i = np.arange(n)
    acc = xf * w[R]
    for j in range(-R, 0):
        acc = acc + (xf[mirror(i + j, n)] + xf[mirror(i - j, n)]) * w[j + R]
    return np.moveaxis(np.floor(acc).astype(np.uint8), 0, axis)


def gaussian_u8(frames, out_hw=None, taps_rc=None):
    """Stage 1 on [..., H, W, C] uint8 frames: rows pass, floor, columns pass, floor. Give
    out_hw (the taps follow from the shapes) or taps_rc = (w_rows or None, w_cols or None)."""
    H, W = frames.shape[-3], frames.shape[-2]
    if taps_rc is None:
        taps_rc = (taps(H, out_hw[0])[2], taps(W, out_hw[1])[2])
    g = np.ascontiguousarray(frames, dtype=np.uint8)
    if taps_rc[0] is not None:
        g = filter_axis(g, g.ndim - 3, taps_rc[0])
    if taps_rc[1] is not None:
        g = filter_axis(g, g.ndim - 2, taps_rc[1])
    return g


def _axis(n, no):
    d = 2 * no
    num = (2 * np.arange(no, dtype=np.int64) + 1) * n - no
    i0 = num // d
    frac = num - i0 * d
    i1 = np.minimum(i0 + (frac > 0), n - 1)
    return i0, i1, frac, d


def bilinear_sd(g, out_hw):
    """Stage 2 in integers: (S, D) with the sampled value of 255 x exactly S / D."""
    H, W = g.shape[-3], g.shape[-2]
    r0, r1, nr, Dr = _axis(H, out_hw[0])
    c0, c1, nc, Dc = _axis(W, out_hw[1])
    gi = g.astype(np.int64)
    nr = nr[:, None, None]
    nc = nc[None, :, None]
    top, bot = gi[..., r0, :, :], gi[..., r1, :, :]
    S = ((Dc - nc) * (Dr - nr) * top[..., c0, :] + nc * (Dr - nr) * top[..., c1, :]
         + (Dc - nc) * nr * bot[..., c0, :] + nc * nr * bot[..., c1, :])
    return S, int(Dr * Dc)


def round_half_even(S, D):
    q = S // D
    twice = 2 * (S - q * D)
    return (q + ((twice > D) | ((twice == D) & (q % 2 == 1)))).astype(np.uint8)


def tie_counts(S, D):
    """(exact ties with an even quotient, with an odd quotient) among the outputs."""
    q = S // D
    tie = 2 * (S - q * D) == D
    return int((tie & (q % 2 == 0)).sum()), int((tie & (q % 2 == 1)).sum())


def resize(frames, out_hw):
    """[..., H, W, C] uint8 -> [..., Ho, Wo, C] uint8, Ho <= H and Wo <= W."""
    frames = np.asarray(frames)
    H, W = frames.shape[-3], frames.shape[-2]
    out_hw = (int(out_hw[0]), int(out_hw[1]))
    if out_hw[0] > H or out_hw[1] > W:
        raise ValueError("upsampling is not defined here")
    S, D = bilinear_sd(gaussian_u8(frames, out_hw=out_hw), out_hw)
    return round_half_even(S, D)
