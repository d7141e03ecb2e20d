"""CPU suite for the cross-point route of discorpy_amd.prep.linepattern (get_tilted_profiles, sliding_window_slope,
locate_subpixel_point, get_local_extrema_points, get_cross_points_hor_lines / get_cross_points_ver_lines; dcp_local_extrema_rows,
dcp_window_slope_rows, dcp_tilted_profiles_2d): the names, signatures and defaults are the reference's; the entry points are exported,
declared and bound and refuse what they do not take before any device work; the wrappers raise for what they do not take before they
ask for a device (this machine has none: reaching the device would raise something else); and the NumPy restatements of the kernels'
arithmetic (tests/helpers/peaks_reference.py) are held to NumPy itself and to the reference's recorded results, golden G27
(tools/gen_golden.py): the pairwise mean bit for bit, the integer positions exactly, the closed forms within 4 e_sub / 4 e_slope."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT, golden

from discorpy_amd import _ffi as F

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import peaks_reference as PR  # noqa: E402

INV, UNS = F.ERR_INVALID_ARG, F.ERR_UNSUPPORTED
P = inspect.Parameter


@pytest.fixture(scope="module")
def lp():
    from discorpy_amd.prep import linepattern
    return linepattern


@pytest.fixture(scope="module")
def g27():
    g = golden("g27_cross_points")
    for v in g.values():
        v.setflags(write=False)
    return g


def test_names_and_signatures_are_the_references(lp):
    assert set(lp.__all__) == {"gaussian_filter", "convert_chessboard_to_linepattern", "get_tilted_profile"}
    assert lp.CROSS_POINTS == ["get_tilted_profiles", "sliding_window_slope", "locate_subpixel_point", "get_local_extrema_points",
                               "get_cross_points_hor_lines", "get_cross_points_ver_lines"]
    for name in lp.CROSS_POINTS:
        assert callable(getattr(lp, name)), name

    def params(fn):
        return [(p.name, p.default, p.kind) for p in inspect.signature(fn).parameters.values()]
    K, V = P.POSITIONAL_OR_KEYWORD, P.VAR_KEYWORD
    assert params(lp.locate_subpixel_point) == [("list_point", P.empty, K), ("option", "min", K)]
    assert params(lp.sliding_window_slope) == [("list_data", P.empty, K), ("size", 3, K), ("norm", True, K)]
    assert params(lp.get_local_extrema_points) == [("list_data", P.empty, K), ("option", "min", K), ("radius", 7, K), ("sensitive", 0.1, K),
                                                   ("denoise", True, K), ("norm", True, K), ("subpixel", True, K), ("select_peaks", False, K),
                                                   ("kwargs", P.empty, V)]
    for fn, a, b in ((lp.get_cross_points_hor_lines, "slope_ver", "dist_ver"), (lp.get_cross_points_ver_lines, "slope_hor", "dist_hor")):
        assert params(fn) == [("mat", P.empty, K), (a, P.empty, K), (b, P.empty, K), ("ratio", 0.3, K), ("norm", True, K), ("offset", 0, K),
                              ("bgr", "bright", K), ("radius", 11, K), ("sensitive", 0.1, K), ("denoise", True, K), ("subpixel", True, K),
                              ("chessboard", False, K), ("select_peaks", False, K), ("kwargs", P.empty, V)]
    assert list(inspect.signature(lp.get_tilted_profiles).parameters) == ["mat", "indices", "angle_deg", "direction"]
    assert list(inspect.signature(lp.get_tilted_profile).parameters) == ["mat", "index", "angle_deg", "direction"]
    for word in ("closed form", "collinear", "select_peaks", "CROSS_POINTS"):
        assert word in lp.__doc__, word


def test_symbols_are_exported_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "discorpy_hip.h")).read()
    exports = open(os.path.join(ROOT, "discorpy_amd", "csrc", "exports.map")).read()
    for symbol, nargs in (("dcp_local_extrema_rows", 12), ("dcp_window_slope_rows", 10), ("dcp_tilted_profiles_2d", 16)):
        assert hasattr(F.lib(), symbol)
        assert re.search(r"^int %s\(const void\* src, " % symbol, header, re.M), symbol
        assert re.search(r"^\s*%s;" % symbol, exports, re.M), symbol
        restype, argtypes = F.SIGNATURES[symbol]
        assert restype is F.C.c_int and len(argtypes) == nargs, symbol


ROWS = np.zeros((4, 40), np.float32)
SENTINEL = 0xA5
OUT = np.full(4 * 40 * 8, SENTINEL, np.uint8)
F32, F64, U16 = (F.DTYPE_BY_NAME[n] for n in ("float32", "float64", "uint16"))


def extrema(**o):
    a = dict(src=ROWS.ctypes.data, dst=OUT.ctypes.data, nrows=4, length=40, stride=40, dtype=F32, radius=5, sensitive=0.1, subpixel=1,
             mem_kind=F.MEM_HOST, device=-1, stream=None)
    a.update(o)
    return F.lib().dcp_local_extrema_rows(*a.values())


def slope(**o):
    a = dict(src=ROWS.ctypes.data, dst=OUT.ctypes.data, nrows=4, length=40, stride=40, dtype=F32, size=3, mem_kind=F.MEM_HOST, device=-1, stream=None)
    a.update(o)
    return F.lib().dcp_window_slope_rows(*a.values())


# 65536 rows of one sample and a destination of that shape: a refusal for the number of rows comes behind the overlap check
MANY = np.zeros((65536, 1), np.float32)
OUT_MANY = np.full(65536 * 4, SENTINEL, np.uint8)

COORD = np.zeros((2, 40))
BAND = np.array([0, 1], np.int32), np.array([2, 2], np.int32)
_i32 = F.C.POINTER(F.C.c_int32)


def profiles(**o):
    a = dict(src=ROWS.ctypes.data, dst=OUT.ctypes.data, height=4, width=40, stride=40, dtype=F32, direction=0, nprofiles=2, length=40,
             yc=COORD.ctypes.data, xc=COORD.ctypes.data, lo=BAND[0], n=BAND[1], mem_kind=F.MEM_HOST, device=-1, stream=None)
    a.update(o)
    for k in ("lo", "n"):
        a[k] = None if a[k] is None else a[k].ctypes.data_as(_i32)
    return F.lib().dcp_tilted_profiles_2d(*a.values())


REFUSALS = [
    (extrema, dict(src=None), INV, "null src / dst"),
    (extrema, dict(dst=None), INV, "null src / dst"),
    (extrema, dict(nrows=0), INV, "height and width must be at least 1"),
    (extrema, dict(stride=39), INV, "src_row_stride 39 is below the width 40"),
    (extrema, dict(dtype=U16), UNS, "profiles are float32 or float64"),
    (extrema, dict(dtype=99), INV, "unknown dtype 99"),
    (extrema, dict(radius=-1), INV, "radius must be at least 0"),
    (extrema, dict(radius=129), UNS, "radius above 128"),
    (extrema, dict(subpixel=2), INV, "subpixel must be 0 or 1"),
    (extrema, dict(radius=0), INV, "subpixel needs a radius of at least 1"),
    (extrema, dict(sensitive=float("nan")), INV, "sensitive is NaN"),
    (extrema, dict(mem_kind=7), INV, "mem_kind"),
    (extrema, dict(dst=ROWS.ctypes.data + 8), INV, "src and dst overlap"),
    (slope, dict(size=4), INV, "size must be odd and at least 3"),
    (slope, dict(size=1), INV, "size must be odd and at least 3"),
    (slope, dict(dtype=U16), UNS, "profiles are float32 or float64"),
    (slope, dict(dst=None), INV, "null src / dst"),
    (slope, dict(length=0), INV, "height and width must be at least 1"),
    (slope, dict(src=MANY.ctypes.data, dst=OUT_MANY.ctypes.data, nrows=65536, length=1, stride=1), UNS, "more than 65535 rows"),
    (profiles, dict(dtype=U16), UNS, "profiles are float32 or float64"),
    (profiles, dict(dst=None), INV, "null dst / coordinate / band pointer"),
    (profiles, dict(yc=None), INV, "null dst / coordinate / band pointer"),
    (profiles, dict(lo=None), INV, "null dst / coordinate / band pointer"),
    (profiles, dict(direction=2), INV, "direction must be 0"),
    (profiles, dict(nprofiles=0), INV, "nprofiles and length must be at least 1"),
    (profiles, dict(nprofiles=70000), UNS, "more than 65535 profiles"),
    (profiles, dict(lo=np.array([0, 3], np.int32)), INV, "band 1: [3, 3 + 2) leaves the image"),
    (profiles, dict(n=np.array([2, 0], np.int32)), INV, "band 1"),
    (profiles, dict(lo=np.array([-1, 0], np.int32)), INV, "band 0"),
    (profiles, dict(direction=1, lo=np.array([0, 39], np.int32)), INV, "band 1: [39, 39 + 2) leaves the image"),
    (profiles, dict(dst=ROWS.ctypes.data), INV, "src and dst overlap"),
]


@pytest.mark.parametrize("fn,override,code,fragment", REFUSALS, ids=["%s-%s" % (c[0].__name__, "-".join(c[1])) for c in REFUSALS])
def test_entry_points_refuse_before_any_device_work(fn, override, code, fragment):
    OUT[:] = SENTINEL
    assert fn(**override) == code
    assert fragment in F.last_error(), F.last_error()
    assert (OUT == SENTINEL).all() and (OUT_MANY == SENTINEL).all()


def test_wrappers_refuse_before_any_device_work(lp):
    img = np.zeros((40, 60), np.float32)
    row = np.arange(600.0)
    with pytest.raises(NotImplementedError, match="select_peaks"):
        lp.get_local_extrema_points(row, select_peaks=True)
    with pytest.raises(NotImplementedError, match="select_peaks"):
        lp.get_cross_points_hor_lines(img, 0.01, 10.0, select_peaks=True)
    with pytest.raises(NotImplementedError, match="select_peaks"):
        lp.get_cross_points_ver_lines(img, 0.01, 10.0, select_peaks=True)
    with pytest.raises(NotImplementedError, match="radius above 128"):
        lp.get_local_extrema_points(row, radius=129)
    with pytest.raises(TypeError, match="Complex type not supported"):
        lp.get_local_extrema_points(row.astype(np.complex64))
    with pytest.raises(TypeError, match="Complex type not supported"):
        lp.sliding_window_slope(row.astype(np.complex128))
    with pytest.raises(TypeError, match="Complex type not supported"):
        lp.get_cross_points_hor_lines(img.astype(np.complex64), 0.01, 10.0)
    with pytest.raises(TypeError, match="Complex type not supported"):
        lp.get_tilted_profiles(img.astype(np.complex64), [3], 1.0, "horizontal")
    with pytest.raises(ValueError, match="Data size must be larger than 2"):
        lp.sliding_window_slope(np.zeros(2))
    with pytest.raises(ValueError, match="1D array or an"):
        lp.get_local_extrema_points(np.zeros((2, 3, 4)))
    with pytest.raises(ValueError, match="direction must be"):
        lp.get_tilted_profiles(img, [3], 1.0, "diagonal")
    with pytest.raises(ValueError, match="Input must be a 2D array"):
        lp.get_tilted_profiles(np.zeros(7, np.float32), [3], 1.0, "horizontal")
    with pytest.raises(ValueError, match=r"Input index is out of possible range: \[2, 39\]"):
        lp.get_tilted_profiles(img, [5, 1], 1.0, "horizontal")
    with pytest.raises(ValueError, match=r"Input index is out of possible range"):
        lp.get_tilted_profiles(img, [5, 60], 1.0, "vertical")
    with pytest.raises(ValueError, match="around 90-degree"):
        lp.get_tilted_profiles(img, [5], 90.0, "vertical")


def test_locate_subpixel_point_is_the_closed_form(lp):
    assert lp.locate_subpixel_point([3.0, 1.0, 2.0]) == PR.subpixel_offset(3.0, 1.0, 2.0) == 3.5 / 3.0        # a = 1.5, b = -3.5
    assert lp.locate_subpixel_point([2.0, 2.0, 2.0]) == 0 and lp.locate_subpixel_point([3.0, 2.0, 1.0]) == 2       # flat, collinear: the argmin
    assert lp.locate_subpixel_point([1.0, 2.0, 0.5], option="max") == PR.subpixel_offset(-1.0, -2.0, -0.5)
    assert abs(lp.locate_subpixel_point([5.0, 1.0, 2.0, 6.0, 9.0]) - (-np.polyfit(np.arange(5), [5.0, 1.0, 2.0, 6.0, 9.0], 2)[1]
                                                                     / (2 * np.polyfit(np.arange(5), [5.0, 1.0, 2.0, 6.0, 9.0], 2)[0]))) < 1e-12


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_pairwise_mean_is_numpys_bit_for_bit(dtype):
    """Every radius 1..128, sorted data whose partial sums round at every step (magnitudes over twelve decades, both signs)."""
    rng = np.random.default_rng(5)
    for radius in range(1, 129):
        for _ in range(6):
            a = np.sort((rng.standard_normal(2 * radius + 1) * 10.0 ** rng.integers(-6, 6, 2 * radius + 1)).astype(dtype))
            tail = a[-radius:]
            want = np.mean(tail)
            got = PR.tail_mean(tail)
            assert got.dtype == want.dtype == np.dtype(dtype) and got == want, (radius, got, want)


def test_restated_search_gives_the_fixtures_integer_positions(g27):
    n = int(g27["pk_count"])
    assert n >= 100
    seen = 0
    for k in range(n):
        row, radius = g27["pk%d_row" % k], int(np.clip(g27["pk_radius"][k], 1, len(g27["pk%d_row" % k]) // 4))
        sens = np.float64(g27["pk_sensitive"][k]) if g27["pk_promotes"][k] else float(g27["pk_sensitive"][k])
        got = PR.local_minima(row, radius, sens)
        assert np.array_equal(got, g27["pk%d_int" % k]), (k, radius, got, g27["pk%d_int" % k])
        seen += len(got)
    assert seen > 300
    lengths = {len(g27["pk%d_row" % k]) for k in range(n)}
    assert {1, 2, 3, 4, 5, 8, 255, 256, 257, 513} <= lengths and {1, 5, 11, 63, 128} <= set(g27["pk_radius"].tolist())


def test_closed_forms_lie_within_the_fixtures_error_of_the_reference(g27):
    e_sub, e_slope = float(g27["e_sub"]), float(g27["e_slope"])
    assert 0 < e_sub < 1e-9 and 0 < e_slope < 1e-12
    worst = 0.0
    for k in range(int(g27["pk_count"])):
        row, ints, subs, curved = (g27["pk%d_%s" % (k, s)] for s in ("row", "int", "sub", "curved"))
        if curved.any():
            worst = max(worst, np.abs(PR.refine(row, ints)[curved] - subs[curved]).max())
    print("closed-form sub-pixel positions: largest deviation from the reference %.3g (e_sub %.3g)" % (worst, e_sub))
    assert worst <= 4 * e_sub
    worst = 0.0
    for k in range(int(g27["sl_count"])):
        row = g27["sl%d_row" % k]
        for size in (3, 5):
            raw = g27["sl%d_s%d" % (k, size)]
            got = PR.window_slope(row, size)
            worst = max(worst, np.abs(got - raw).max() / np.abs(raw).max())
            nmean = np.mean(got)
            normed = g27["sl%d_s%d_norm" % (k, size)]
            # (normalised: the slopes and the mean they are divided by each carry at most 4 e_slope)
            assert np.abs(got / nmean - normed).max() <= 8 * e_slope * np.abs(normed).max()
    print("closed-form slopes: largest relative deviation from the reference %.3g (e_slope %.3g)" % (worst, e_slope))
    assert worst <= 4 * e_slope
