"""CPU suite for the colour entry points of the homography and the fused map: names, argument checks made before any device
call, the three places a C symbol has to appear in, and the shape of golden G24."""
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

NAMES = ("correct_perspective_color_image", "unwarp_perspective_fused_color_image")
SYMBOLS = ("dcp_perspective_color_image", "dcp_unwarp_fused_color_image")


def test_both_functions_are_importable_and_public():
    from discorpy_amd.util import utility as util
    for name in NAMES:
        assert callable(getattr(util, name)) and name in util.__all__, name


@pytest.mark.parametrize("ncoef", [0, 7, 9])
def test_a_wrong_length_list_coef_is_refused_before_any_device_call(monkeypatch, ncoef):
    """post.correct_perspective_image's own check and message (reference postprocessing.py:486-487), on 3-D and 2-D input."""
    from discorpy_amd import _ffi as F
    from discorpy_amd.post import postprocessing as pp
    from discorpy_amd.util import utility as util

    def no_device(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(F, "require_device", no_device)
    monkeypatch.setattr(F, "lib", no_device)
    coef = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0][:ncoef]
    with pytest.raises(ValueError) as want:
        pp.correct_perspective_image(np.zeros((6, 7), np.float32), coef)
    for img in (np.zeros((6, 7, 3), np.float32), np.zeros((6, 7), np.float32), np.zeros((6, 7, 3), np.uint8)):
        with pytest.raises(ValueError) as got:
            util.correct_perspective_color_image(img, coef)
        assert str(got.value) == str(want.value)
        with pytest.raises(ValueError) as got:
            util.unwarp_perspective_fused_color_image(img, 3.0, 3.0, [1.0, 1e-3], coef)
        assert str(got.value) == str(want.value)


def test_a_3d_array_still_fails_in_the_post_function():
    """post.correct_perspective_image itself is unchanged: (height, width) = mat.shape, as in the reference."""
    from discorpy_amd.post import postprocessing as pp
    with pytest.raises(ValueError):
        pp.correct_perspective_image(np.zeros((6, 7, 3), np.float32), [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])


@pytest.mark.parametrize("symbol", SYMBOLS)
def test_each_new_symbol_is_declared_exported_and_prototyped(symbol):
    from discorpy_amd import _ffi as F
    header = open(os.path.join(ROOT, "include", "discorpy_hip.h")).read()
    assert re.search(r"^int %s\(" % symbol, header, re.M), "not declared in include/discorpy_hip.h"
    exports = open(os.path.join(ROOT, "discorpy_amd", "csrc", "exports.map")).read()
    assert re.search(r"^\s*%s;" % symbol, exports, re.M), "not named in csrc/exports.map"
    protos = [v for k, v in vars(F).items() if isinstance(v, dict) and symbol in v]
    assert len(protos) == 1, "no prototype in _ffi.py"
    restype, argtypes = protos[0][symbol]
    declared = re.search(r"^int %s\((.*?)\);" % symbol, header, re.M | re.S).group(1)
    assert len(argtypes) == declared.count(",") + 1, "prototype and declaration disagree on the number of arguments"


def test_golden_g24_holds_arrays_only():
    path = os.path.join(GOLDEN, "g24_colour_homography40x56x3.npz")
    assert os.path.getsize(path) < 1048576
    with np.load(path, allow_pickle=False) as z:          # (an object array would need pickle and fail here)
        assert len(z.files) >= 14
        for name in z.files:
            a = z[name]
            assert isinstance(a, np.ndarray) and a.dtype.kind in "fiu", (name, a.dtype)
        assert tuple(z["shape"]) == (40, 56, 3) and z["rgb_f32"].dtype == np.float32 and z["rgb_u8"].dtype == np.uint8
        for tag, dt in (("f32", np.float32), ("u8", np.uint8)):
            for order in (1, 0, 3):
                for kind in ("persp", "fused"):
                    a = z["%s_%s_o%d" % (kind, tag, order)]
                    assert a.shape == (40, 56, 3) and a.dtype == dt, (kind, tag, order)
