"""CPU suite for calculate_threshold's GPU steps: dcp_sort_plane_2d and dcp_zoom_cubic_nearest_1d are exported, declared and bound and
refuse what they say they refuse before any device work (host buffers, no GPU visible); discorpy_amd.prep.threshold and .complete carry
the reference's names and signatures (golden G31 records them); and tests/helpers/sorted_zoom_reference.py, the written-down form of what
the two kernels must do, is held against NumPy's sort and against scipy.ndimage.zoom itself."""
import inspect
import os
import re
import sys

import numpy as np
import pytest
import scipy.ndimage as ndi

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import sorted_zoom_reference as szr  # noqa: E402

from discorpy_amd import _ffi as F  # noqa: E402
from discorpy_amd.prep import complete, pointgrid, preprocessing, threshold  # noqa: E402

G31 = np.load(os.path.join(ROOT, "tests", "golden", "g31_prep_rest.npz"))
INV, UNS = F.ERR_INVALID_ARG, F.ERR_UNSUPPORTED
H, W = 8, 10
SRC = np.zeros(H * (W + 4) * 8, np.uint8)
DST = np.full(H * W * 8, 7, np.uint8)
U16 = F.DTYPE_BY_NAME["uint16"]
CALLS = {
    "dcp_sort_plane_2d": (dict(src=SRC.ctypes.data, dst=DST.ctypes.data, height=H, width=W, stride=W, dtype=U16, mem_kind=F.MEM_HOST, device=-1,
                               stream=None), "src dst height width stride dtype mem_kind device stream".split()),
    "dcp_zoom_cubic_nearest_1d": (dict(src=SRC.ctypes.data, n=H * W, dst=DST.ctypes.data, out_n=W, dtype=U16, mem_kind=F.MEM_HOST, device=-1,
                                       stream=None), "src n dst out_n dtype mem_kind device stream".split()),
}


def call(name, override):
    valid, order = CALLS[name]
    args = dict(valid, **override)
    return getattr(F.lib(), name)(*[args[k] for k in order])


@pytest.mark.parametrize("symbol,head,nargs", [
    ("dcp_sort_plane_2d", r"const void\* src, void\* dst, int height, int width, long src_row_stride, int dtype, int mem_kind", 9),
    ("dcp_zoom_cubic_nearest_1d", r"const void\* src, int64_t n, void\* dst, int64_t out_n, int dtype, int mem_kind", 8)])
def test_symbols_are_exported_declared_and_bound(symbol, head, nargs):
    assert hasattr(F.lib(), symbol)
    header = open(os.path.join(ROOT, "include", "discorpy_hip.h")).read()
    assert re.search(r"^int %s\(%s" % (symbol, head), header, re.M)
    exports = open(os.path.join(ROOT, "discorpy_amd", "csrc", "exports.map")).read()
    assert re.search(r"^\s*%s;" % symbol, exports, re.M), "not named in csrc/exports.map"
    restype, argtypes = F.SIGNATURES[symbol]
    assert restype is F.C.c_int and len(argtypes) == nargs
    makefile = open(os.path.join(ROOT, "discorpy_amd", "csrc", "Makefile")).read()
    assert "api_sort.o" in makefile and "sort_kernels.o" in makefile


REFUSALS = (
    [("dcp_sort_plane_2d",) + c for c in [
        (dict(height=0), INV, "height"), (dict(width=0), INV, "width"), (dict(height=-1), INV, "height"), (dict(stride=W - 1), INV, "src_row_stride"),
        (dict(mem_kind=7), INV, "mem_kind"), (dict(mem_kind=F.MEM_DEVICE_UNORDERED), INV, "mem_kind"), (dict(src=None), INV, "src"),
        (dict(dst=None), INV, "dst"), (dict(dst=SRC.ctypes.data), INV, "overlap"), (dict(dtype=99), INV, "dtype"), (dict(dtype=-1), INV, "dtype"),
        (dict(dtype=F.DTYPE_BY_NAME["bool"]), UNS, "dtype"),
        (dict(height=65536, width=32768, stride=32768), UNS, "height * width"),
        # 2^30 float64 keys twice: 16 GiB of key buffers (a destination address far enough away not to overlap; nothing is touched)
        (dict(height=32768, width=32768, stride=32768, dtype=F.DTYPE_BY_NAME["float64"], dst=SRC.ctypes.data + (1 << 40)), UNS, "2 GiB")]]
    + [("dcp_zoom_cubic_nearest_1d",) + c for c in [
        (dict(n=0), INV, "at least 1"), (dict(n=-4), INV, "at least 1"), (dict(out_n=0), INV, "out_n"), (dict(out_n=-1), INV, "out_n"),
        (dict(n=1 << 31), UNS, "2^31 - 1"), (dict(out_n=1 << 31), UNS, "2^31 - 1"),
        (dict(mem_kind=7), INV, "mem_kind"), (dict(mem_kind=7, n=0), INV, "mem_kind"), (dict(src=None), INV, "src"), (dict(dst=None), INV, "dst"),
        (dict(dst=SRC.ctypes.data + 2), INV, "overlap"), (dict(dtype=99), INV, "dtype"), (dict(dtype=-1, n=0), INV, "dtype"),
        (dict(dtype=F.DTYPE_BY_NAME["bool"]), UNS, "dtype")]])


@pytest.mark.parametrize("name,override,rc,fragment", REFUSALS,
                         ids=["%s-%s" % (c[0][4:], "-".join("%s=%s" % (k, v if k not in ("src", "dst") else "x") for k, v in sorted(c[1].items())))
                              for c in REFUSALS])
def test_entry_points_refuse(name, override, rc, fragment):
    got = call(name, override)
    assert (got, fragment in F.last_error()) == (rc, True), (got, F.last_error())
    assert (DST == 7).all()          # nothing was written


def test_lab_option_round_trips_under_its_prefixed_name_only():
    assert F.get_option("x_sort_skip") == 1
    F.set_option("x_sort_skip", 0)
    assert F.get_option("x_sort_skip") == 0
    F.set_option("x_sort_skip", 1)
    with pytest.raises(ValueError, match="unknown option"):
        F.set_option("sort_skip", 0)


def test_the_keys_moved_to_a_shared_header():
    csrc = os.path.join(ROOT, "discorpy_amd", "csrc")
    for user in ("median_kernels.hip", "sort_kernels.hip"):
        text = open(os.path.join(csrc, user)).read()
        assert '#include "order_keys.h"' in text and "struct MedianKey" not in text and "median_key(U u)" not in text
    shared = open(os.path.join(csrc, "order_keys.h")).read()
    assert "struct MedianKey" in shared and "median_key(U u)" in shared and "median_elem(" in shared


def test_window_and_horizon_of_the_helper_are_the_kernels():
    text = open(os.path.join(ROOT, "discorpy_amd", "csrc", "sort_kernels.hip")).read()
    m = re.search(r"constexpr int kZoomPad = (\d+), kZoomWindow = (\d+), kZoomHorizon = (\d+),", text)
    assert m and tuple(int(g) for g in m.groups()) == (szr.PAD, szr.WINDOW, szr.HORIZON)
    assert abs(szr.POLE) ** szr.WINDOW < 2.0 ** -121          # the bound the header states


# --------------------------------------------------------------------------- names and signatures

def recorded(kind="public"):
    names = [str(n) for n in G31["%s_names" % kind]]
    return dict(zip(names, (str(s) for s in G31["signatures" if kind == "public" else "private_signatures"])))


def test_complete_has_exactly_the_references_public_names_and_signatures():
    want = recorded()
    got = sorted(n for n, f in inspect.getmembers(complete, inspect.isfunction) if not n.startswith("_"))
    assert got == sorted(want) == sorted(complete.__all__)
    for name, sig in want.items():
        assert str(inspect.signature(getattr(complete, name))) == sig, name


def test_new_functions_have_the_references_signatures():
    want = recorded()
    assert str(inspect.signature(threshold.calculate_threshold)) == want["calculate_threshold"]
    for name in pointgrid.__all__:
        assert str(inspect.signature(getattr(pointgrid, name))) == want[name], name
    for name, sig in recorded("private").items():
        assert str(inspect.signature(getattr(pointgrid, name))) == sig, name
    assert threshold.__all__ == ["sort_values", "zoom_sorted", "calculate_threshold"]


def test_preprocessing_keeps_refusing_what_complete_offers():
    for name in ("calculate_threshold", "make_parabola_mask", "rotate_points", "remove_subset_points", "group_dots_hor_lines_based_polyfit"):
        assert not hasattr(preprocessing, name) and hasattr(complete, name)
    assert complete.get_points_dot_pattern is not preprocessing.get_points_dot_pattern
    assert complete.binarization is preprocessing.binarization
    import discorpy_amd.prep as prep
    assert prep.threshold is threshold and prep.pointgrid is pointgrid and prep.complete is complete


def test_inputs_are_refused_before_any_device_work():
    with pytest.raises(TypeError, match="Complex type not supported"):
        threshold.calculate_threshold(np.zeros((4, 4), np.complex64))
    with pytest.raises(RuntimeError, match="data type not supported"):
        threshold.calculate_threshold(np.zeros((4, 4), np.float16))
    with pytest.raises(NotImplementedError, match="bool"):
        threshold.calculate_threshold(np.zeros((4, 4), bool))
    with pytest.raises(ValueError, match="2-D"):
        threshold.calculate_threshold(np.zeros(16, np.float32))
    with pytest.raises(ValueError, match="2-D"):
        threshold.calculate_threshold(np.zeros((2, 2, 4), np.float32))
    with pytest.raises(TypeError, match="Complex type not supported"):
        threshold.sort_values(np.zeros((4, 4), np.complex128))
    with pytest.raises(NotImplementedError, match="bool"):
        threshold.zoom_sorted(np.zeros(4, bool), 2)
    with pytest.raises(ValueError, match="at least one"):
        threshold.zoom_sorted(np.zeros(4, np.float32), 0)


def test_host_half_of_the_formula_equals_the_recorded_thresholds():
    """The trim, the fit and the closing formulas on scipy's own sorted and zoomed profile: G31's values within 1e-9."""
    for i, want in enumerate(G31["thres_value"]):
        img = G31["thres_img%d" % i]
        profile = ndi.zoom(np.sort(img, axis=None), 1.0 * max(img.shape) / img.size, mode="nearest")
        got = threshold._threshold_of_profile(profile, str(G31["thres_bgr"][i]), float(G31["thres_snr"][i]))
        assert abs(got - want) <= 1e-9 * max(abs(want), 1.0), (i, got, want)
    # the constant middle half: the fitted slope is 0 to rounding, the threshold the plateau's value
    assert abs(G31["thres_value"][-1] - np.median(G31["thres_img%d" % (len(G31["thres_value"]) - 1)])) < 1e-6


# --------------------------------------------------------------------------- the helper against NumPy and scipy

DTYPES = ["float32", "float64", "uint8", "int8", "uint16", "int16", "uint32", "int32", "uint64", "int64"]


@pytest.mark.parametrize("dtype", DTYPES)
def test_sort_reference_equals_np_sort(dtype):
    rng = np.random.default_rng(11)
    dt = np.dtype(dtype)
    if dt.kind == "f":
        a = (rng.standard_normal(5000) * 10.0 ** rng.integers(-30, 30, 5000)).astype(dt)
        u = "u%d" % dt.itemsize
        a[:40] = np.array([0.0, -0.0, np.inf, -np.inf, np.finfo(dt).tiny / 4, -np.finfo(dt).tiny / 4, np.nan, -np.nan] * 5, dt)
        a[40] = np.array([np.array(np.nan, dt).view(u) | 5], u).view(dt)[0]          # another payload
        a[41] = -a[40]
    else:
        info = np.iinfo(dt)
        a = rng.integers(info.min, info.max, 5000, dtype=dt, endpoint=True)
        a[:2] = info.min, info.max
    a = rng.permutation(a)
    got, want = szr.sort_reference(a), np.sort(a, axis=None)
    assert got.dtype == want.dtype and np.array_equal(got, want, equal_nan=dt.kind == "f")
    if dt.kind == "f":          # what NumPy leaves open: zeros by sign, every NaN positive and last
        zeros = got[got == 0]
        assert np.signbit(zeros).tolist() == sorted(np.signbit(zeros).tolist(), reverse=True)
        nans = got[np.isnan(got)]
        assert len(nans) == 12 and not np.signbit(nans).any() and np.isnan(got[-12:]).all()


def window_ulps(a, got, want):
    """The largest |got - want| in float64 ulps of the largest magnitude in the output point's window of the source."""
    n, m = len(a), len(got)
    zoom = (n - 1) / (m - 1) if m > 1 else 1.0
    first = np.floor(np.arange(m) * zoom + szr.PAD).astype(np.int64) - 1
    lo = np.clip(first - szr.WINDOW - szr.PAD, 0, n - 1)
    hi = np.clip(first + 3 + szr.WINDOW - szr.PAD, 0, n - 1)
    mag = np.array([np.abs(a[l:h + 1]).max() for l, h in zip(lo, hi)])
    ulp = np.spacing(np.where(mag > 0, mag, np.finfo(np.float64).tiny))
    return float((np.abs(got.astype(np.float64) - want.astype(np.float64)) / ulp).max())


# float64: the distance of the restatement from scipy.ndimage.zoom measured where this was written (x86-64, scipy 1.15.3) over LENGTHS on
# zoom_case's lines and on rough unsorted lines: 4.0 ulps of the window's largest magnitude at most; one more for another libm.
F64_ULPS = 4.0 + 1.0


@pytest.mark.parametrize("n,out_n", szr.LENGTHS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_zoom_reference_against_scipy(dtype, n, out_n):
    """float32 and integers equal scipy.ndimage.zoom.  float64 does not: already the whole-line restatement (window=None) of the
    prefilter differs from scipy's spline_filter1d by up to 2 ulps per coefficient on this build of scipy (operation orders and fused
    forms tried, none matched), which the four taps carry into the result; the interpolation itself, on scipy's own coefficients,
    equals scipy's.  Measured: at most 4.0 ulps of the window's largest magnitude, with and without the window."""
    a = szr.zoom_case(n, dtype)
    want = ndi.zoom(a, out_n / n, order=3, mode="nearest")
    assert want.shape == (out_n,) == (szr.zoom_length(n, out_n / n),)
    got = szr.zoom_reference(a, out_n)
    assert got.dtype == want.dtype
    if dtype == "float64":
        whole = szr.zoom_reference(a, out_n, window=None)
        print("float64 %d -> %d: %.3f ulps windowed, %.3f whole line, %.3f between the two"
              % (n, out_n, window_ulps(a, got, want), window_ulps(a, whole, want), window_ulps(a, got, whole)))
        assert window_ulps(a, got, want) <= F64_ULPS
        assert window_ulps(a, got, whole) <= 1.0          # the window itself: no more than a last-bit flicker
    else:
        assert np.array_equal(got, want)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_zoom_reference_on_rough_lines(dtype):
    """Unsorted lines whose neighbours differ by orders of magnitude: the window's start-up error is measured against local magnitude."""
    rng = np.random.default_rng(5)
    for n, out_n in szr.LENGTHS:
        a = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)).astype(dtype)
        want = ndi.zoom(a, out_n / n, order=3, mode="nearest")
        got = szr.zoom_reference(a, out_n)
        if dtype == "float32":
            assert np.array_equal(got, want), (n, out_n)
        else:
            assert window_ulps(a, got, want) <= F64_ULPS, (n, out_n)


def test_the_threshold_mode_of_the_timing_tool_answers_help():
    import subprocess
    tool = os.path.join(ROOT, "tools", "time_binarize.py")
    res = subprocess.run([sys.executable, tool, "--threshold", "--help"], capture_output=True, text=True)
    assert res.returncode == 0 and "calculate_threshold" in res.stdout and "torch.sort" in res.stdout
    res = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True)
    assert res.returncode == 0 and "--threshold" in res.stdout and "salt-and-pepper" in res.stdout
