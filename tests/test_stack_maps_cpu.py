"""CPU suite for the frames of one calibration under the homography and the fused map (post.correct_perspective_images,
post.unwarp_perspective_fused_images, dcp_remap_frames_typed): names, the checks made before any device call, the three places the
C symbol has to appear in, and every argument check of the entry point through the library loaded without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NAMES = ("correct_perspective_images", "unwarp_perspective_fused_images")
SYMBOL = "dcp_remap_frames_typed"
IDENTITY = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
F32, U16 = 0, 4
MAP_RADIAL, MAP_PERSP, MAP_FUSED = 0, 1, 2


def test_both_functions_are_importable_and_public():
    from discorpy_amd.post import postprocessing as pp
    for name in NAMES:
        assert callable(getattr(pp, name)) and name in pp.__all__, name


def _no_device(monkeypatch):
    from discorpy_amd import _ffi as F

    def no_device(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(F, "require_device", no_device)
    monkeypatch.setattr(F, "lib", no_device)


@pytest.mark.parametrize("ncoef", [0, 7, 9])
def test_a_wrong_length_list_coef_is_refused_before_any_device_call(monkeypatch, ncoef):
    """post.correct_perspective_image's own check and message (reference postprocessing.py:486-487), on an array and on a list."""
    from discorpy_amd.post import postprocessing as pp
    _no_device(monkeypatch)
    coef = (IDENTITY + [0.0])[:ncoef]
    with pytest.raises(ValueError) as want:
        pp.correct_perspective_image(np.zeros((6, 7), np.float32), coef)
    assert str(want.value) == "!!! Eight coefficients are required !!!"
    for mats in (np.zeros((3, 6, 7), np.float32), [np.zeros((6, 7), np.float32)] * 2, np.zeros((3, 6, 7), np.uint16)):
        with pytest.raises(ValueError) as got:
            pp.correct_perspective_images(mats, coef)
        assert str(got.value) == str(want.value)
        with pytest.raises(ValueError) as got:
            pp.unwarp_perspective_fused_images(mats, 3.0, 3.0, [1.0, 1e-3], coef)
        assert str(got.value) == str(want.value)


@pytest.mark.parametrize("shape", [(6, 7), (2, 3, 6, 7)])
def test_an_array_of_the_wrong_rank_is_refused_as_unwarp_images_backward_refuses_it(monkeypatch, shape):
    from discorpy_amd.post import postprocessing as pp
    _no_device(monkeypatch)
    mats = np.zeros(shape, np.float32)
    with pytest.raises(ValueError) as want:
        pp.unwarp_images_backward(mats, 3.0, 3.0, [1.0])
    with pytest.raises(ValueError) as got:
        pp.correct_perspective_images(mats, IDENTITY)
    assert str(got.value) == str(want.value)
    with pytest.raises(ValueError) as got:
        pp.unwarp_perspective_fused_images(mats, 3.0, 3.0, [1.0], IDENTITY)
    assert str(got.value) == str(want.value)


def test_an_empty_sequence_gives_an_empty_list_without_a_device(monkeypatch):
    from discorpy_amd.post import postprocessing as pp
    _no_device(monkeypatch)
    assert pp.correct_perspective_images([], IDENTITY) == []
    assert pp.unwarp_perspective_fused_images([], 3.0, 3.0, [1.0], IDENTITY) == []


def test_a_3d_array_still_fails_in_the_single_frame_function():
    """post.correct_perspective_image itself is unchanged: (height, width) = mat.shape, as in the reference."""
    from discorpy_amd.post import postprocessing as pp
    with pytest.raises(ValueError):
        pp.correct_perspective_image(np.zeros((3, 6, 7), np.float32), IDENTITY)


def test_the_symbol_is_declared_exported_and_prototyped():
    from discorpy_amd import _ffi as F
    header = open(os.path.join(ROOT, "include", "discorpy_hip.h")).read()
    assert re.search(r"^int %s\(" % SYMBOL, header, re.M), "not declared in include/discorpy_hip.h"
    exports = open(os.path.join(ROOT, "discorpy_amd", "csrc", "exports.map")).read()
    assert re.search(r"^\s*%s;" % SYMBOL, exports, re.M), "not named in csrc/exports.map"
    restype, argtypes = F.SIGNATURES[SYMBOL]
    declared = re.search(r"^int %s\((.*?)\);" % SYMBOL, header, re.M | re.S).group(1)
    assert len(argtypes) == declared.count(",") + 1 == 19, "prototype and declaration disagree on the number of arguments"
    # the comment above the declaration cites what the call stands for in the reference
    comment = header[:header.index("int %s(" % SYMBOL)].rsplit("/*", 1)[1]
    assert "postprocessing.py:444-459" in comment and ":486-492" in comment and "demo_05.py:127,147" in comment


def _call(L, **kw):
    """dcp_remap_frames_typed on two 4 x 5 float32 host frames under the identity homography, with the arguments in `kw` replaced."""
    buf = np.zeros(64, np.float32)
    one = (C.c_double * 8)(*IDENTITY)
    fact = (C.c_double * 2)(1.0, 0.0)
    a = dict(src=buf.ctypes.data, dst=buf.ctypes.data + 160, dtype=F32, map_kind=MAP_PERSP, nframes=2, height=4, width=5, frame_stride=20,
             row_stride=5, xcenter=2.0, ycenter=2.0, list_fact=fact, nfact=2, list_coef=one, order=1, blend_mode=0, mem_kind=0, device=-1,
             stream=None)
    a.update(kw)
    return L.dcp_remap_frames_typed(*[a[k] for k in ("src", "dst", "dtype", "map_kind", "nframes", "height", "width", "frame_stride", "row_stride",
                                                     "xcenter", "ycenter", "list_fact", "nfact", "list_coef", "order", "blend_mode", "mem_kind",
                                                     "device", "stream")])


BAD = [
    (dict(src=None), "null frame pointer"),
    (dict(dst=None), "null frame pointer"),
    (dict(list_coef=None), "null homography pointer"),
    (dict(map_kind=MAP_FUSED, list_fact=None), "null coefficient pointer"),
    (dict(nframes=-1), "nframes < 0"),
    (dict(height=0), "frames must be non-empty"),
    (dict(width=0), "frames must be non-empty"),
    (dict(row_stride=4), "row stride 4 overlaps rows of width 5"),
    (dict(frame_stride=19), "frame stride 19 overlaps frames"),
    (dict(dtype=11), "unknown element type 11"),
    (dict(dtype=-1), "unknown element type -1"),
    (dict(map_kind=3), "unknown map_kind 3"),
    (dict(map_kind=-1), "unknown map_kind -1"),
    (dict(mem_kind=7), "unknown mem_kind 7"),
    (dict(order=2), "order 2 outside [0, 1]"),
    (dict(order=-1), "order -1 outside [0, 1]"),
    (dict(nfact=-1), "nfact = -1 outside [0, 32]"),
    (dict(nfact=33), "nfact = 33 outside [0, 32]"),
    (dict(map_kind=MAP_FUSED, nfact=33), "nfact = 33 outside [0, 32]"),
    (dict(blend_mode=9), "unknown blend_mode 9"),
]


@pytest.mark.parametrize("kw, message", BAD, ids=["%s" % "-".join("%s=%s" % (k, v) for k, v in b[0].items()) for b in BAD])
def test_each_argument_check_answers_before_any_device_call(kw, message):
    """DCP_ERR_INVALID_ARG and a message, from the library loaded on a box without a device (the checks come before the first HIP call:
    with a device call in front of them this test would see DCP_ERR_HIP / DCP_ERR_NO_DEVICE instead)."""
    from discorpy_amd import _ffi as F
    L = F.lib()
    assert _call(L, **kw) == F.ERR_INVALID_ARG, F.last_error()
    assert message in F.last_error(), F.last_error()


def test_the_radial_map_is_sent_to_the_stack_entry_points():
    from discorpy_amd import _ffi as F
    L = F.lib()
    assert _call(L, map_kind=MAP_RADIAL) == F.ERR_INVALID_ARG
    assert "dcp_unwarp_stack_rows_f32" in F.last_error() and "dcp_unwarp_stack_rows_typed" in F.last_error(), F.last_error()


@pytest.mark.parametrize("kind", [MAP_PERSP, MAP_FUSED])
def test_no_frames_is_ok_whatever_the_pointers_are(kind):
    from discorpy_amd import _ffi as F
    L = F.lib()
    assert _call(L, nframes=0, map_kind=kind) == F.OK
    assert _call(L, nframes=0, map_kind=kind, src=None, dst=None, mem_kind=F.MEM_DEVICE, dtype=U16) == F.OK
    # fewer than two frames: the distance to a next frame does not matter
    assert _call(L, nframes=0, frame_stride=0, map_kind=kind) == F.OK
    # ... but an argument that is wrong stays wrong
    assert _call(L, nframes=0, map_kind=kind, order=4) == F.ERR_INVALID_ARG
