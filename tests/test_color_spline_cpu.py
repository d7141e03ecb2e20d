"""CPU suite for colour images at spline orders 2..5 in one call: the three places each new C symbol has to appear in, golden G25
(the reference's util.unwarp_color_image_backward at orders 2..5) against the oracle, the routing of the three util functions
(recorded with a stand-in for the library, no device), and the argument check made before any device call."""
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, golden

SYMBOLS = ("dcp_unwarp_color_image_spline", "dcp_perspective_color_image_spline", "dcp_unwarp_fused_color_image_spline")
SIBLINGS = {"dcp_unwarp_color_image_spline": "dcp_unwarp_color_image", "dcp_perspective_color_image_spline": "dcp_perspective_color_image",
            "dcp_unwarp_fused_color_image_spline": "dcp_unwarp_fused_color_image"}
MODES = ("reflect", "grid-mirror", "constant", "grid-constant", "nearest", "mirror", "grid-wrap", "wrap")
G25 = "g25_colour_spline40x56x3"
COEF = [0.98, -0.01, 3.0, 0.012, 0.97, 2.0, -1e-5, 2e-5]
RADIAL = (9.5, 6.25, [1.0, 1e-3, 2e-5])


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
    # the arguments of the order 0 / 1 entry point, with boundary_mode in place of blend_mode
    sibling = re.search(r"^int %s\((.*?)\);" % SIBLINGS[symbol], header, re.M | re.S).group(1)
    assert " ".join(declared.split()) == " ".join(sibling.replace("blend_mode", "boundary_mode").split())
    assert argtypes == protos[0][SIBLINGS[symbol]][1]


def test_golden_g25_holds_arrays_only():
    path = os.path.join(GOLDEN, G25 + ".npz")
    assert os.path.getsize(path) < 1048576
    with np.load(path, allow_pickle=False) as z:          # (an object array would need pickle and fail here)
        names = set(z.files)
        for name in z.files:
            a = z[name]
            assert isinstance(a, np.ndarray) and a.dtype.kind in "fiu", (name, a.dtype)
        assert tuple(z["shape"]) == (40, 56, 3) and int(z["seed"]) == 2510
        assert z["rgb_f32"].dtype == np.float32 and z["rgb_f32"].shape == (40, 56, 3)
        assert z["rgb_u8"].dtype == np.uint8 and z["rgb_u8"].shape == (40, 56, 3)
        assert (float(z["xcenter"]), float(z["ycenter"]), list(z["list_fact"])) == (27.4, 19.1, [1.0, 0.004, 2e-5])
        want = {"seed", "shape", "xcenter", "ycenter", "list_fact", "rgb_f32", "rgb_u8", "f32_o3_reflect_pad_4_edge"}
        for order in (2, 3, 4, 5):
            for mode in ("reflect", "nearest", "grid_wrap"):
                a = z["f32_o%d_%s" % (order, mode)]
                assert a.shape == (40, 56, 3) and a.dtype == np.float32, (order, mode)
                want.add("f32_o%d_%s" % (order, mode))
        for mode in MODES:
            a = z["u8_o3_%s" % mode.replace("-", "_")]
            assert a.shape == (40, 56, 3) and a.dtype == np.uint8, mode
            want.add("u8_o3_%s" % mode.replace("-", "_"))
        a = z["f32_o3_reflect_pad_4_edge"]
        assert a.shape == (48, 64, 3) and a.dtype == np.float32
        assert names == want
    # the inputs are the seed's
    rng = np.random.default_rng(2510)
    g = golden(G25)
    assert np.array_equal(g["rgb_f32"], rng.random((40, 56, 3), dtype=np.float32))
    assert np.array_equal(g["rgb_u8"], rng.integers(0, 255, (40, 56, 3), endpoint=True).astype(np.uint8))


def test_the_oracle_per_channel_equals_golden_g25(orc):
    g = golden(G25)
    xc, yc, fact = float(g["xcenter"]), float(g["ycenter"]), list(g["list_fact"])
    for c in range(3):
        plane = np.ascontiguousarray(g["rgb_f32"][:, :, c])
        for order in (2, 3, 4, 5):
            for mode in ("reflect", "nearest", "grid-wrap"):
                want = g["f32_o%d_%s" % (order, mode.replace("-", "_"))][:, :, c]
                assert np.array_equal(orc.unwarp_image_backward(plane, xc, yc, fact, order=order, mode=mode), want), (c, order, mode)
        plane = np.ascontiguousarray(g["rgb_u8"][:, :, c])
        for mode in MODES:
            want = g["u8_o3_%s" % mode.replace("-", "_")][:, :, c]
            assert np.array_equal(orc.unwarp_image_backward(plane, xc, yc, fact, order=3, mode=mode), want), (c, mode)
        padded = np.pad(g["rgb_f32"][:, :, c], 4, mode="edge")
        assert np.array_equal(orc.unwarp_image_backward(padded, xc + 4, yc + 4, fact, order=3, mode="reflect"),
                              g["f32_o3_reflect_pad_4_edge"][:, :, c]), c


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

    def named(self, suffix="_spline"):
        return [(n, a) for n, a in self.calls if n.endswith(suffix)]


@pytest.fixture
def recorder(monkeypatch):
    from discorpy_amd import _ffi as F
    rec = _Recorder()
    monkeypatch.setattr(F, "lib", lambda: rec)
    monkeypatch.setattr(F, "require_device", lambda: None)
    return rec


def _calls(rec, fn):
    del rec.calls[:]
    fn()
    return rec.named()


def _util_calls(util, img, **kw):
    """The three util functions on `img` with keyword arguments `kw`, and the C symbol each is expected to call."""
    return [("dcp_unwarp_color_image_spline", lambda: util.unwarp_color_image_backward(img, *RADIAL, **kw)),
            ("dcp_perspective_color_image_spline", lambda: util.correct_perspective_color_image(img, COEF, **kw)),
            ("dcp_unwarp_fused_color_image_spline", lambda: util.unwarp_perspective_fused_color_image(img, *RADIAL, COEF, **kw))]


def test_a_numpy_image_at_order_3_makes_one_call_of_the_matching_symbol(recorder):
    from discorpy_amd import _ffi as F
    from discorpy_amd.util import utility as util
    img = np.random.default_rng(1).random((12, 20, 3), dtype=np.float32)
    for symbol, fn in _util_calls(util, img, order=3):
        got = _calls(recorder, fn)
        assert [n for n, _ in got] == [symbol], (symbol, recorder.calls)
        assert [n for n, _ in recorder.calls] == [symbol], "another entry point was called as well"
        args = got[0][1]
        # src, dst, dtype, height, width, channels, row stride, pixel stride
        assert args[0] == img.ctypes.data and args[2:8] == (F.DTYPE_F32, 12, 20, 3, 60, 3), args
        # ..., order, boundary_mode, mem_kind, device, stream
        assert args[-5] == 3 and args[-4] == 0 and args[-3] == F.MEM_HOST, args
    # a view of a wider buffer goes in place: pixel stride 4, row stride 80
    rgba = np.random.default_rng(2).random((12, 20, 4), dtype=np.float32)
    for symbol, fn in _util_calls(util, rgba[:, :, :3], order=2, mode="mirror"):
        args = _calls(recorder, fn)[0][1]
        assert args[0] == rgba.ctypes.data and args[5:8] == (3, 80, 4) and args[-5] == 2 and args[-4] == MODES.index("mirror"), (symbol, args)


@pytest.mark.parametrize("blend, bit", [(None, 0), ("scipy", 0x100), ("SciPy", 0x100), ("exact", 0x100), ("f64lerp", 0)])
def test_the_scipy_sum_bit_is_set_only_for_the_scipy_blend(recorder, blend, bit):
    from discorpy_amd.util import utility as util
    img = np.zeros((12, 20, 3), np.uint8)
    for mode in ("reflect", "nearest", "wrap"):
        for symbol, fn in _util_calls(util, img, order=3, mode=mode, blend=blend):
            got = _calls(recorder, fn)
            assert len(got) == 1 and got[0][0] == symbol and got[0][1][-4] == (MODES.index(mode) | bit), (symbol, mode, blend, got)


def test_orders_2_to_5_and_one_to_four_channels_take_the_one_call_route(recorder):
    from discorpy_amd.util import utility as util
    for order in (2, 3, 4, 5):
        for channels in (1, 2, 3, 4):
            img = np.zeros((12, 20, channels), np.float32)
            for symbol, fn in _util_calls(util, img, order=order):
                got = _calls(recorder, fn)
                assert [n for n, _ in got] == [symbol] and got[0][1][5] == channels and got[0][1][-5] == order, (order, channels, symbol)


def test_five_channels_orders_0_and_1_and_map_index_make_no_such_call(recorder):
    from discorpy_amd.util import utility as util
    five = np.zeros((12, 20, 5), np.float32)
    for symbol, fn in _util_calls(util, five, order=3):
        assert _calls(recorder, fn) == [], symbol
        assert recorder.calls, "the plane-by-plane route made no call at all"
    rgb = np.zeros((12, 20, 3), np.float32)
    for order in (0, 1):
        for symbol, fn in _util_calls(util, rgb, order=order):
            assert _calls(recorder, fn) == [], (symbol, order)
    ymap, xmap = np.mgrid[0:12, 0:20].astype(np.float32).reshape(2, -1, 1)
    assert _calls(recorder, lambda: util.correct_perspective_color_image(rgb, COEF, order=3, map_index=(ymap, xmap))) == []
    assert len([n for n, _ in recorder.calls if n.startswith("dcp_remap_coords")]) == 3          # one per plane
    # a 2-D image is the single-plane function's
    for symbol, fn in _util_calls(util, rgb[:, :, 0], order=3):
        assert _calls(recorder, fn) == [], symbol


def test_complex_input_is_split_and_padding_happens_before_the_call(recorder):
    from discorpy_amd.util import utility as util
    z = np.zeros((12, 20, 3), np.complex64)
    for symbol, fn in _util_calls(util, z, order=3):
        got = _calls(recorder, fn)
        assert [n for n, _ in got] == [symbol, symbol], (symbol, got)            # real and imaginary parts
    rgb = np.zeros((12, 20, 3), np.float32)
    got = _calls(recorder, lambda: util.unwarp_color_image_backward(rgb, *RADIAL, order=3, pad=4, pad_mode="edge"))
    assert len(got) == 1 and got[0][1][3:6] == (20, 28, 3) and got[0][1][8:10] == (RADIAL[0] + 4, RADIAL[1] + 4), got


@pytest.mark.parametrize("ncoef", [0, 7, 9])
def test_a_wrong_length_list_coef_is_refused_before_any_device_call(monkeypatch, ncoef):
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
    assert "Eight coefficients" in str(want.value)
    for order in (2, 3, 5):
        for img in (np.zeros((6, 7, 3), np.float32), np.zeros((6, 7, 4), np.uint8)):
            with pytest.raises(ValueError) as got:
                util.correct_perspective_color_image(img, coef, order=order)
            assert str(got.value) == str(want.value)
            with pytest.raises(ValueError) as got:
                util.unwarp_perspective_fused_color_image(img, 3.0, 3.0, [1.0, 1e-3], coef, order=order)
            assert str(got.value) == str(want.value)
