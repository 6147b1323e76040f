"""Golden vectors for the scene ingest's frame resize, from the REFERENCE's own call.

Run ONLY in the build container, with the interpreter that has scikit-image:
    /opt/conda/bin/python3.9 tests/golden/gen_resize_goldens.py

The reference's cached env resizes every frame it emits with
skimage.transform.resize(frame, image_size, anti_aliasing=True)
(environments/gym_ai2thor/envs/cached.py:62-64). This script makes that call on synthetic
uint8 frames and records inputs and float64 outputs in resize.npz:

  rand_in   3 random 60x80x3 frames          -> (17, 23), (59, 79), (12, 80), (21, 21)
  flat_in   8 piecewise-flat 40x36x3 frames (blocks of 5x6 pixels) followed by the constant
            frames 0, 5, ..., 255            -> (11, 10), (40, 13), (17, 36), (7, 5)
  <set>_out_<Ho>x<Wo>   float64 [N, Ho, Wo, 3] in [0, 1]
"""
import os

import numpy as np
from skimage.transform import resize

HERE = os.path.dirname(os.path.abspath(__file__))
RAND_SHAPES = ((17, 23), (59, 79), (12, 80), (21, 21))
FLAT_SHAPES = ((11, 10), (40, 13), (17, 36), (7, 5))


def inputs():
    rng = np.random.RandomState(2024)
    rand = rng.randint(0, 256, size=(3, 60, 80, 3)).astype(np.uint8)
    blocks = rng.randint(0, 256, size=(8, 8, 6, 3)).astype(np.uint8)
    piecewise = blocks.repeat(5, axis=1).repeat(6, axis=2)
    const = np.arange(0, 256, 5, dtype=np.uint8)[:, None, None, None].repeat(40, 1).repeat(36, 2).repeat(3, 3)
    return rand, np.concatenate([piecewise, const])


def main():
    rand, flat = inputs()
    out = {"rand_in": rand, "flat_in": flat}
    for name, frames, shapes in (("rand", rand, RAND_SHAPES), ("flat", flat, FLAT_SHAPES)):
        for hw in shapes:
            res = np.stack([resize(f, hw, anti_aliasing=True) for f in frames])
            assert res.dtype == np.float64 and res.shape == (len(frames),) + hw + (3,)
            out["%s_out_%dx%d" % (name, hw[0], hw[1])] = res
    path = os.path.join(HERE, "resize.npz")
    np.savez_compressed(path, **out)
    print({k: v.shape for k, v in out.items()}, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
