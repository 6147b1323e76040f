"""Float observations (obs_format="f32_chw", vn_step_f32), the parts that need no GPU: the
scalar conversion of csrc/vn_unit_float.h compiled for the host and checked for all 256 byte
values, and the argument check of obs_format."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import PKG

MAIN = r"""
#include <stdio.h>
#include <string.h>
#include "vn_unit_float.h"
int main() {
  for (int b = 0; b < 256; ++b) {
    const float f = vn::unit_from_u8((uint8_t)b);
    uint32_t u;
    memcpy(&u, &f, 4);
    printf("%u\n", u);
  }
  return 0;
}
"""


def test_unit_float_is_the_fp32_division_for_every_byte(tmp_path):
    """float(u8) / 255.0f bit for bit (np.float32(u) / np.float32(255)) for u = 0..255, from the
    header the kernel uses, built as a stand-alone host program."""
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = tmp_path / "unit_float_main.cpp"
    src.write_text(MAIN)
    exe = tmp_path / "unit_float_main"
    subprocess.run([cxx, "-O2", "-std=c++17", "-I", os.path.join(PKG, "csrc"), str(src), "-o", str(exe), "-lm"],
                   check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    got = np.array([int(x) for x in out], dtype=np.uint32)
    u = np.arange(256, dtype=np.float32)
    want = (u / np.float32(255)).view(np.uint32)
    assert got.shape == want.shape
    assert np.array_equal(got, want), np.nonzero(got != want)[0]
    # the multiplication the header replaces is not that division (126 of 256 differ): the
    # test would notice a header that fell back to it
    recip = (u * (np.float32(1) / np.float32(255))).view(np.uint32)
    assert int((recip != want).sum()) == 126


def test_unknown_obs_format_is_refused_before_any_gpu_use():
    import vnav
    from vnav import envs
    assert envs.OBS_FORMATS == ("u8_hwc", "f32_chw")
    for bad in ("f32_hwc", "float", None, "U8_HWC"):
        with pytest.raises(ValueError):
            vnav.VectorEnv([], 4, obs_format=bad)
        with pytest.raises(ValueError):
            vnav.make("CachedThor-v0", [], 4, obs_format=bad)
