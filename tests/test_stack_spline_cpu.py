"""CPU suite for stacks of frames at spline orders 2..5 in one call (post.unwarp_images_backward, post.correct_perspective_images,
post.unwarp_perspective_fused_images -> dcp_remap_frames_spline): the three places the C symbol has to appear in, every argument
check of the entry point through the library loaded without a device, and the routing of the three post functions (recorded with a
stand-in for the library, no device): what goes to the entry point and what stays frame by frame."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

SYMBOL = "dcp_remap_frames_spline"
IDENTITY = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
COEF = [0.98, -0.01, 3.0, 0.012, 0.97, 2.0, -1e-5, 2e-5]
RADIAL = (9.5, 6.25, [1.0, 1e-3, 2e-5])
F32, F64, U16, BOOL = 0, 1, 4, 10
MAP_RADIAL, MAP_PERSP, MAP_FUSED = 0, 1, 2
SCIPY_SUM = 0x100
ARGS = ("src", "dst", "dtype", "map_kind", "nframes", "height", "width", "frame_stride", "row_stride", "xcenter", "ycenter", "list_fact",
        "nfact", "list_coef", "order", "mode", "mem_kind", "device", "stream")


def test_the_symbol_is_declared_exported_and_prototyped():
    from discorpy_amd import _ffi as F
    header = open(os.path.join(ROOT, "include", "discorpy_hip.h")).read()
    assert re.search(r"^int %s\(" % SYMBOL, header, re.M), "not declared in include/discorpy_hip.h"
    exports = open(os.path.join(ROOT, "discorpy_amd", "csrc", "exports.map")).read()
    assert re.search(r"^\s*%s;" % SYMBOL, exports, re.M), "not named in csrc/exports.map"
    restype, argtypes = F.SIGNATURES[SYMBOL]
    declared = re.search(r"^int %s\((.*?)\);" % SYMBOL, header, re.M | re.S).group(1)
    assert len(argtypes) == declared.count(",") + 1 == len(ARGS), "prototype and declaration disagree on the number of arguments"
    # the arguments of the order 0 / 1 entry point, with mode in place of blend_mode
    sibling = re.search(r"^int dcp_remap_frames_typed\((.*?)\);", header, re.M | re.S).group(1)
    assert " ".join(declared.split()) == " ".join(sibling.replace("blend_mode", "mode").split())
    assert argtypes == F.SIGNATURES["dcp_remap_frames_typed"][1]
    # the comment above the declaration cites what the call stands for in the reference
    comment = header[:header.index("int %s(" % SYMBOL)].rsplit("/*", 1)[1]
    assert "postprocessing.py:111-148" in comment and "demo_07.py:25,60" in comment and "demo_05.py:127,147" in comment


def test_the_lab_option_is_not_in_the_header():
    header = open(os.path.join(ROOT, "include", "discorpy_hip.h")).read()
    assert "spline_frames\"" not in header and "x_spline_frames" not in header


def _call(L, **kw):
    """dcp_remap_frames_spline on two 4 x 5 float32 host frames under the radial map at order 3, with the arguments in `kw` replaced."""
    buf = np.zeros(64, np.float32)
    one = (C.c_double * 8)(*IDENTITY)
    fact = (C.c_double * 2)(1.0, 0.0)
    a = dict(src=buf.ctypes.data, dst=buf.ctypes.data + 160, dtype=F32, map_kind=MAP_RADIAL, nframes=2, height=4, width=5, frame_stride=20,
             row_stride=5, xcenter=2.0, ycenter=2.0, list_fact=fact, nfact=2, list_coef=one, order=3, mode=0, mem_kind=0, device=-1,
             stream=None)
    a.update(kw)
    return L.dcp_remap_frames_spline(*[a[k] for k in ARGS])


BAD = [
    (dict(order=1), "spline order 1 outside [2, 5]"),
    (dict(order=6), "spline order 6 outside [2, 5]"),
    (dict(order=-1), "spline order -1 outside [2, 5]"),
    (dict(mode=8), "unknown boundary mode 8"),
    (dict(mode=8 | SCIPY_SUM), "unknown boundary mode"),
    (dict(mode=-1), "unknown boundary mode"),
    (dict(mem_kind=0x101), "unknown mem_kind 257"),
    (dict(dtype=11), "unknown element type 11"),
    (dict(dtype=-1), "unknown element type -1"),
    (dict(src=None), "null"),
    (dict(dst=None), "null"),
    (dict(list_fact=None), "null coefficient pointer"),
    (dict(map_kind=MAP_PERSP, list_coef=None), "null homography pointer"),
    (dict(map_kind=MAP_FUSED, list_coef=None), "null homography pointer"),
    (dict(map_kind=MAP_FUSED, list_fact=None), "null coefficient pointer"),
    (dict(nframes=-1), "nframes < 0"),
    (dict(height=0), "non-empty"),
    (dict(width=0), "non-empty"),
    (dict(row_stride=4), "row stride 4 overlaps rows of width 5"),
    (dict(frame_stride=19), "frame stride 19 overlaps frames"),
    (dict(map_kind=3), "unknown map_kind 3"),
    (dict(map_kind=-1), "unknown map_kind -1"),
    (dict(nfact=-1), "nfact = -1 outside [0, 32]"),
    (dict(nfact=33), "nfact = 33 outside [0, 32]"),
]


@pytest.mark.parametrize("kw, message", BAD, ids=["%s" % "-".join("%s=%s" % (k, v) for k, v in b[0].items()) for b in BAD])
def test_each_argument_check_answers_before_any_device_call(kw, message):
    """DCP_ERR_INVALID_ARG and a message, from the library loaded on a box without a device (the checks come before the first HIP call:
    with a device call in front of them this test would see DCP_ERR_HIP / DCP_ERR_NO_DEVICE instead)."""
    from discorpy_amd import _ffi as F
    L = F.lib()
    assert _call(L, **kw) == F.ERR_INVALID_ARG, F.last_error()
    assert message in F.last_error(), F.last_error()


@pytest.mark.parametrize("kind", [MAP_RADIAL, MAP_PERSP, MAP_FUSED])
def test_no_frames_is_ok_whatever_the_pointers_are(kind):
    from discorpy_amd import _ffi as F
    L = F.lib()
    assert _call(L, nframes=0, map_kind=kind) == F.OK
    assert _call(L, nframes=0, map_kind=kind, src=None, dst=None, mem_kind=F.MEM_DEVICE, dtype=U16, mode=4 | SCIPY_SUM, order=5) == F.OK
    # fewer than two frames: the distance to a next frame does not matter
    assert _call(L, nframes=0, frame_stride=0, map_kind=kind) == F.OK
    # ... but an argument that is wrong stays wrong
    assert _call(L, nframes=0, map_kind=kind, order=1) == F.ERR_INVALID_ARG
    assert _call(L, nframes=0, map_kind=kind, mode=9) == F.ERR_INVALID_ARG


def test_arguments_the_map_does_not_use_may_be_null():
    """The radial map ignores the homography, the homography the polynomial: refused for neither (what is left to fail without a
    device is the device itself)."""
    from discorpy_amd import _ffi as F
    L = F.lib()
    assert _call(L, nframes=0, map_kind=MAP_RADIAL, list_coef=None) == F.OK
    assert _call(L, nframes=0, map_kind=MAP_PERSP, list_fact=None, nfact=40) == F.OK


@pytest.mark.parametrize("value", [-1, 17, 100])
def test_the_lab_option_refuses_values_outside_0_16(value):
    from discorpy_amd import _ffi as F
    L = F.lib()
    before = C.c_int(-7)
    assert L.dcp_get_option(b"x_spline_frames", C.byref(before)) == F.OK and before.value in (2, 4, 8, 16)
    assert L.dcp_set_option(b"x_spline_frames", value) == F.ERR_INVALID_ARG
    assert L.dcp_set_option(b"spline_frames", 4) == F.ERR_INVALID_ARG              # a lab switch: only with its prefix
    after = C.c_int(-7)
    assert L.dcp_get_option(b"x_spline_frames", C.byref(after)) == F.OK and after.value == before.value
    for ok in (0, 1, 16, before.value):
        assert L.dcp_set_option(b"x_spline_frames", ok) == F.OK
        assert L.dcp_get_option(b"x_spline_frames", C.byref(after)) == F.OK and after.value == ok


# ---- routing

class _Recorder:
    """Stands in for the loaded library: every entry point is recorded and reports success; nothing reaches a device."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("dcp_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


@pytest.fixture
def recorder(monkeypatch):
    """The library replaced by a recorder, and the one-place switch answering yes for every map and spline order: what is checked
    with it is what a stack needs to reach the entry point once the switch lets it (the switch's own table has its test below)."""
    from discorpy_amd import _ffi as F
    from discorpy_amd.post import postprocessing as pp
    rec = _Recorder()
    monkeypatch.setattr(F, "lib", lambda: rec)
    monkeypatch.setattr(F, "require_device", lambda: None)
    monkeypatch.setattr(pp, "_stack_spline_one_call", lambda kind, order, host: 2 <= order <= 5)
    return rec


def test_the_switch_keeps_the_cases_that_measured_slower_on_the_route(monkeypatch):
    """Radial: every spline order; homography: orders 2 and 3; fused map: none (tools/time_batch.py --order on the MI355X)."""
    from discorpy_amd import _ffi as F
    from discorpy_amd.post import postprocessing as pp
    table = {(kind, order): pp._stack_spline_one_call(kind, order, host) for kind in (MAP_RADIAL, MAP_PERSP, MAP_FUSED) for order in range(0, 7)
             for host in (True, False)}
    assert {k for k, v in table.items() if v} == {(MAP_RADIAL, 2), (MAP_RADIAL, 3), (MAP_RADIAL, 4), (MAP_RADIAL, 5), (MAP_PERSP, 2), (MAP_PERSP, 3)}
    rec = _Recorder()
    monkeypatch.setattr(F, "lib", lambda: rec)
    monkeypatch.setattr(F, "require_device", lambda: None)
    mats = np.zeros((3, 6, 7), np.float32)
    for order in (2, 3, 4, 5):
        for kind, fn in _three(pp, mats, order=order):
            names = _run(rec, fn)[1]
            assert (names == [SYMBOL]) == table[kind, order], (kind, order, names)
            assert len(names) == (1 if table[kind, order] else 3), (kind, order, names)


def _three(pp, mats, **kw):
    """The three stack functions on `mats` with keyword arguments `kw`, and the map kind each hands to the entry point."""
    return [(MAP_RADIAL, lambda: pp.unwarp_images_backward(mats, *RADIAL, **kw)),
            (MAP_PERSP, lambda: pp.correct_perspective_images(mats, COEF, **kw)),
            (MAP_FUSED, lambda: pp.unwarp_perspective_fused_images(mats, *RADIAL, COEF, **kw))]


def _run(rec, fn):
    del rec.calls[:]
    res = fn()
    return res, [n for n, _ in rec.calls], [a for n, a in rec.calls if n == SYMBOL]


@pytest.mark.parametrize("dtype", ["float32", "uint8", "uint16", "int16", "float64", "bool", "int64"])
@pytest.mark.parametrize("order", [2, 3, 4, 5])
def test_a_numpy_stack_at_a_spline_order_makes_one_call_of_the_entry_point(recorder, dtype, order):
    from discorpy_amd import _ffi as F
    from discorpy_amd.post import postprocessing as pp
    mats = np.zeros((3, 6, 7), dtype)
    for kind, fn in _three(pp, mats, order=order, mode="mirror", blend="scipy"):
        res, names, calls = _run(recorder, fn)
        assert names == [SYMBOL], (kind, names)
        a = dict(zip(ARGS, calls[0]))
        assert (a["src"], a["dtype"], a["map_kind"], a["nframes"], a["height"], a["width"], a["frame_stride"], a["row_stride"]) == \
               (mats.ctypes.data, F.DTYPE_BY_NAME[dtype], kind, 3, 6, 7, 42, 7)
        assert (a["order"], a["mode"], a["mem_kind"]) == (order, 5 | SCIPY_SUM, F.MEM_HOST)
        assert isinstance(res, np.ndarray) and res.shape == mats.shape and res.dtype == mats.dtype and a["dst"] == res.ctypes.data
        if kind != MAP_PERSP:
            assert (a["xcenter"], a["ycenter"], a["nfact"]) == (RADIAL[0], RADIAL[1], 3)
    # the default sum: the mode's code alone
    _, _, calls = _run(recorder, lambda: pp.unwarp_images_backward(mats, *RADIAL, order=order, mode="nearest"))
    assert dict(zip(ARGS, calls[0]))["mode"] == 4


def test_out_as_a_3d_array_is_filled_and_returned(recorder):
    from discorpy_amd.post import postprocessing as pp
    mats = np.zeros((2, 6, 7), np.float32)
    for kind, fn in _three(pp, mats, order=3, out=None):
        out = np.empty_like(mats)
        args = {MAP_RADIAL: (pp.unwarp_images_backward, RADIAL), MAP_PERSP: (pp.correct_perspective_images, (COEF,)),
                MAP_FUSED: (pp.unwarp_perspective_fused_images, RADIAL + (COEF,))}[kind]
        res, names, calls = _run(recorder, lambda: args[0](mats, *args[1], order=3, out=out))
        assert res is out and names == [SYMBOL] and dict(zip(ARGS, calls[0]))["dst"] == out.ctypes.data


def test_frames_read_in_place_from_a_wider_buffer(recorder):
    from discorpy_amd.post import postprocessing as pp
    buf = np.zeros((4, 8, 10), np.uint16)
    for view, fs, rs in ((buf[:3, :6, :7], 80, 10), (buf[::2, :, :7], 160, 10), (buf[:, :6, :], 80, 10), (buf[1:2, :6, :7], 80, 10)):
        for kind, fn in _three(pp, view, order=3):
            _, names, calls = _run(recorder, fn)
            a = dict(zip(ARGS, calls[0]))
            assert names == [SYMBOL] and (a["src"], a["frame_stride"], a["row_stride"]) == (view.ctypes.data, fs, rs), (kind, names)


def test_what_stays_frame_by_frame(recorder):
    """Sequences of 2-D arrays, per-frame calibrations, complex input, column-strided and overlapping views, a list as `out`: the
    single-frame entry points, once per frame (twice for complex under the homography: real and imaginary part; the
    other two functions refuse complex frames as they always have), and never the new one."""
    from discorpy_amd.post import postprocessing as pp
    f32 = np.zeros((3, 6, 7), np.float32)
    single = {MAP_RADIAL: "dcp_unwarp_image_spline_f32", MAP_PERSP: "dcp_perspective_image_spline_f32", MAP_FUSED: "dcp_unwarp_fused_spline_f32"}
    typed = {MAP_RADIAL: "dcp_unwarp_image_typed", MAP_PERSP: "dcp_perspective_image_typed", MAP_FUSED: "dcp_unwarp_fused_typed"}
    for kind, fn in _three(pp, [f32[i] for i in range(3)], order=3):
        assert _run(recorder, fn)[1] == [single[kind]] * 3, kind
    for kind, fn in _three(pp, f32[:, :, ::2], order=3):                          # column stride 2
        assert _run(recorder, fn)[1] == [single[kind]] * 3, kind
    overlapping = np.lib.stride_tricks.as_strided(np.zeros(100, np.float32), (3, 6, 7), (28, 28, 4))
    for kind, fn in _three(pp, overlapping, order=3):
        assert _run(recorder, fn)[1] == [single[kind]] * 3, kind
    for kind, fn in _three(pp, f32.astype(np.complex64), order=3):
        if kind != MAP_PERSP:                                                      # (as before: only the homography's function splits complex frames)
            with pytest.raises(NotImplementedError):
                fn()
            assert SYMBOL not in [n for n, _ in recorder.calls]
        else:
            assert _run(recorder, fn)[1] == [single[kind]] * 6, kind
    for kind, fn in _three(pp, f32.astype(np.uint8), order=3, out=[np.zeros((6, 7), np.uint8) for _ in range(3)]):
        assert _run(recorder, fn)[1] == [typed[kind]] * 3, kind
    # per-frame calibrations (radial map only)
    assert _run(recorder, lambda: pp.unwarp_images_backward(f32, [9.5, 9.0, 8.5], 6.25, RADIAL[2], order=3))[1] == [single[MAP_RADIAL]] * 3
    assert _run(recorder, lambda: pp.unwarp_images_backward(f32, 9.5, [6.25, 6.0, 5.75], RADIAL[2], order=3))[1] == [single[MAP_RADIAL]] * 3
    assert _run(recorder, lambda: pp.unwarp_images_backward(f32, 9.5, 6.25, [RADIAL[2]] * 3, order=3))[1] == [single[MAP_RADIAL]] * 3
    # more coefficients than the library takes: the single-frame call, which refuses them itself
    assert _run(recorder, lambda: pp.unwarp_images_backward(f32, 9.5, 6.25, [1.0] + [0.0] * 32, order=3))[1] == [single[MAP_RADIAL]] * 3


def test_orders_0_and_1_do_not_reach_the_entry_point(recorder):
    from discorpy_amd.post import postprocessing as pp
    mats = np.zeros((3, 6, 7), np.float32)
    for order in (0, 1):
        for kind, fn in _three(pp, mats, order=order):
            names = _run(recorder, fn)[1]
            assert names and SYMBOL not in names, (order, kind, names)


def test_an_empty_stack_is_returned_without_a_call(recorder):
    from discorpy_amd.post import postprocessing as pp
    mats = np.zeros((0, 6, 7), np.float32)
    for kind, fn in _three(pp, mats, order=3):
        res, names, _ = _run(recorder, fn)
        assert res is mats and names == [], kind


def test_the_one_place_switch_sends_a_case_back_to_the_route(recorder, monkeypatch):
    from discorpy_amd import _ffi as F
    from discorpy_amd.post import postprocessing as pp
    mats = np.zeros((3, 6, 7), np.float32)
    seen = []

    def only_order_3(kind, order, host):
        seen.append((kind, order, host))
        return order == 3
    monkeypatch.setattr(pp, "_stack_spline_one_call", only_order_3)
    for kind, fn in _three(pp, mats, order=5):
        assert SYMBOL not in _run(recorder, fn)[1], kind
    for kind, fn in _three(pp, mats, order=3):
        assert _run(recorder, fn)[1] == [SYMBOL], kind
    assert seen == [(k, o, True) for o in (5, 3) for k in (MAP_RADIAL, MAP_PERSP, MAP_FUSED)]
