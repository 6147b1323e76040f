"""The five-frame observation in one launch (vn_set_aux_arena, vn_step_aux, vn_observe_aux,
VectorEnv(aux_format=...)), the parts that need no GPU: the C ABI is declared, exported and
bound, its argument checks answer without a device, and VectorEnv refuses a bad aux_format
before it touches the GPU."""
import ctypes

import pytest

from test_lib_abi import declared_symbols

NEW = ("vn_set_aux_arena", "vn_step_aux", "vn_observe_aux")


def test_entry_points_declared_exported_and_bound(built_lib):
    import torch  # noqa: F401  (shares torch's HIP runtime, as the product does)
    from vnav import _lib
    syms = declared_symbols()
    lib = ctypes.CDLL(built_lib)
    for s in NEW:
        assert s in syms, s
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES, s
    bound = _lib.load()
    for s in NEW:
        assert getattr(bound, s).argtypes == _lib.SIGNATURES[s][1]


def test_obs_set_matches_the_header():
    """vn_obs_set: five pointers and one int32 format, in the header's order."""
    import re

    from conftest import REPO
    from vnav import _lib
    text = open(REPO + "/include/vnav.h").read()
    body = re.search(r"typedef struct vn_obs_set \{(.*?)\} vn_obs_set;", text, flags=re.S).group(1)
    fields = re.findall(r"(\w+);", body)
    assert fields == [f[0] for f in _lib.ObsSet._fields_]
    assert fields == ["image", "goal", "depth", "segmentation", "goal_segmentation", "format"]
    assert ctypes.sizeof(_lib.ObsSet) == 5 * ctypes.sizeof(ctypes.c_void_p) + 8
    assert re.search(r"VN_OBS_U8_HWC = 0", text) and re.search(r"VN_OBS_F32_CHW = 1", text)
    assert (_lib.OBS_U8_HWC, _lib.OBS_F32_CHW) == (0, 1)


def test_null_context_is_refused_with_a_message(built_lib):
    from vnav import _lib
    lib = _lib.load()
    o = _lib.ObsSet()
    assert lib.vn_step_aux(None, None, ctypes.byref(o), None, None, None, None) == -1
    assert "vn_step_aux" in _lib.last_error() and "NULL" in _lib.last_error()
    assert lib.vn_observe_aux(None, ctypes.byref(o), None, None) == -1
    assert "vn_observe_aux" in _lib.last_error()
    assert lib.vn_set_aux_arena(None, None, 1, None, 3) == -1
    assert "vn_set_aux_arena" in _lib.last_error()


def test_aux_format_is_checked_before_any_gpu_use():
    import vnav
    from vnav import envs
    assert envs.AUX_KEYS == ("depth", "segmentation", "goal_segmentation")
    for kw in (dict(aux_format="f32_chw"), dict(aux_format="f32_chw", obs_format="u8_hwc"),
               dict(aux_format="f32_hwc", obs_format="f32_chw"), dict(aux_format="U8_HWC"), dict(aux_format=1)):
        with pytest.raises(ValueError):
            vnav.VectorEnv([], 4, aux_observations=True, **kw)
        with pytest.raises(ValueError):
            vnav.make("AuxiliaryGraph-v0", [], 4, **kw)
    # the accepted spellings get past the format checks (and stop at the empty scene list)
    for kw in (dict(), dict(aux_format=None), dict(aux_format="u8_hwc"), dict(aux_format="u8_hwc", obs_format="f32_chw"),
               dict(aux_format="f32_chw", obs_format="f32_chw")):
        with pytest.raises(ValueError, match="at least one scene"):
            vnav.VectorEnv([], 4, aux_observations=True, **kw)
