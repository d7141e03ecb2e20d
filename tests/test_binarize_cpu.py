"""CPU suite for the binarization of dot images: the six new entry points are exported, declared and bound and refuse what they say they
refuse before any device work (the buffers are host memory, no GPU is visible to these cases); discorpy_amd.prep.preprocessing offers
the functions with the reference's and scikit-image's signatures and raises what it says it raises without a device; the tile table of
the GPU tests is the kernels'; and the scipy / NumPy composite of tests/helpers/binarize_reference.py is a yardstick at all: scipy's
"reflect" equals "ignore what lies outside" for the cross, and np.histogram equals a plain search of its own edges on inputs where its
raw estimate is off by one for many elements."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import binarize_reference as bref  # noqa: E402
import label_cases as cases  # noqa: E402

from discorpy_amd import _ffi as F  # noqa: E402

INV, UNS = F.ERR_INVALID_ARG, F.ERR_UNSUPPORTED
H, W = 8, 10
SRC = np.zeros(H * (W + 4) * 8, np.uint8)
DST = np.zeros(H * W * 8, np.uint8)
EDGES = np.linspace(0, 1, 9)
COUNTS = np.full(8, -7, np.int64)
MINMAX = np.full(2, -7.0)
BAD = F.C.c_int64(-7)
U16, F64 = F.DTYPE_BY_NAME["uint16"], F.DTYPE_BY_NAME["float64"]

COMMON = dict(src=SRC.ctypes.data, dst=DST.ctypes.data, height=H, width=W, stride=W, dtype=U16, mem_kind=F.MEM_HOST, device=-1, stream=None)
CALLS = {
    "dcp_abs_2d": (COMMON, "src dst height width stride dtype mem_kind device stream".split()),
    "dcp_minmax_2d": (dict(COMMON, minmax=MINMAX.ctypes.data_as(F.C.POINTER(F.C.c_double)), bad=F.C.byref(BAD)),
                      "src height width stride dtype minmax bad mem_kind device stream".split()),
    "dcp_histogram_2d": (dict(COMMON, dtype=F64, edges=EDGES.ctypes.data, nbins=8, first=0, counts=COUNTS.ctypes.data),
                         "src height width stride dtype edges nbins first counts mem_kind device stream".split()),
    "dcp_threshold_2d": (dict(COMMON, thres=0.5, count=None), "src dst height width stride dtype thres count mem_kind device stream".split()),
    "dcp_clear_border_2d": (dict(COMMON, connectivity=8, invert=0),
                            "src dst height width stride dtype connectivity invert mem_kind device stream".split()),
    "dcp_morph_cross_2d": (dict(COMMON, op=2), "src dst height width stride op mem_kind device stream".split()),
}


def call(name, override):
    valid, order = CALLS[name]
    args = dict(valid, **override)
    return getattr(F.lib(), name)(*[args[k] for k in order])


@pytest.mark.parametrize("symbol,head,nargs", [
    ("dcp_abs_2d", r"const void\* src, void\* dst, int height, int width, long src_row_stride, int dtype, int mem_kind", 9),
    ("dcp_minmax_2d", r"const void\* src, int height, int width, long src_row_stride, int dtype, double\* minmax_out, int64_t\* nonfinite_out", 10),
    ("dcp_histogram_2d", r"const void\* src, int height, int width, long src_row_stride, int dtype, const void\* edges, int nbins, int64_t first", 12),
    ("dcp_threshold_2d", r"const void\* src, uint8_t\* dst, int height, int width, long src_row_stride, int dtype, double thres, int64_t\* count", 11),
    ("dcp_clear_border_2d", r"const void\* src, uint8_t\* dst, int height, int width, long src_row_stride, int dtype, int connectivity, int invert", 11),
    ("dcp_morph_cross_2d", r"const uint8_t\* src, uint8_t\* dst, int height, int width, long src_row_stride, int op, int mem_kind", 9)])
def test_symbols_are_exported_declared_and_bound(symbol, head, nargs):
    assert hasattr(F.lib(), symbol)
    header = open(os.path.join(ROOT, "include", "discorpy_hip.h")).read()
    assert re.search(r"^int %s\(%s" % (symbol, head), header, re.M)
    exports = open(os.path.join(ROOT, "discorpy_amd", "csrc", "exports.map")).read()
    assert re.search(r"^\s*%s;" % symbol, exports, re.M), "not named in csrc/exports.map"
    restype, argtypes = F.SIGNATURES[symbol]
    assert restype is F.C.c_int and len(argtypes) == nargs and F.C.c_long in argtypes
    makefile = open(os.path.join(ROOT, "discorpy_amd", "csrc", "Makefile")).read()
    assert "api_binarize.o" in makefile and "binarize_kernels.o" in makefile


SHARED = [
    (dict(height=0), INV, "height"),
    (dict(width=0), INV, "width"),
    (dict(height=-1), INV, "height"),
    (dict(stride=W - 1), INV, "src_row_stride"),
    (dict(mem_kind=7), INV, "mem_kind"),
    (dict(mem_kind=F.MEM_DEVICE_UNORDERED), INV, "mem_kind"),
    (dict(src=None), INV, "src"),
    (dict(height=65536, width=32768, stride=32768), UNS, "height * width"),
]
TYPED = [(dict(dtype=99), INV, "dtype"), (dict(dtype=-1), INV, "dtype")]
WITH_DST = [(dict(dst=None), INV, "dst"), (dict(dst=SRC.ctypes.data), INV, "overlap")]
REDUCED = [(dict(dtype=F.DTYPE_BY_NAME[n]), UNS, "dtype") for n in ("int32", "uint32", "int64", "uint64", "bool")]
REFUSALS = (
    [("dcp_abs_2d",) + c for c in SHARED + TYPED + WITH_DST]
    + [("dcp_minmax_2d",) + c for c in SHARED + TYPED + REDUCED + [(dict(minmax=None), INV, "minmax_out"), (dict(bad=None), INV, "nonfinite_out")]]
    + [("dcp_histogram_2d",) + c for c in SHARED + TYPED + REDUCED + [
        (dict(counts=None), INV, "counts_out"), (dict(nbins=0), INV, "nbins"), (dict(nbins=-3), INV, "nbins"), (dict(nbins=65537), UNS, "nbins"),
        (dict(edges=None), INV, "edges"), (dict(dtype=U16), INV, "edges")]]
    + [("dcp_threshold_2d",) + c for c in SHARED + TYPED + WITH_DST]
    + [("dcp_clear_border_2d",) + c for c in SHARED + TYPED + WITH_DST + [
        (dict(connectivity=6), INV, "connectivity"), (dict(connectivity=0), INV, "connectivity"), (dict(invert=2), INV, "invert"),
        (dict(invert=-1), INV, "invert")]]
    + [("dcp_morph_cross_2d",) + c for c in SHARED + WITH_DST + [(dict(op=3), INV, "op"), (dict(op=-1), INV, "op")]])


@pytest.mark.parametrize("name,override,rc,fragment", REFUSALS,
                         ids=["%s-%s" % (c[0][4:-3], "-".join("%s=%s" % (k, v if k not in ("src", "dst", "minmax", "bad", "counts", "edges") else "x")
                                                               for k, v in sorted(c[1].items()))) for c in REFUSALS])
def test_entry_points_refuse(name, override, rc, fragment):
    got = call(name, override)
    assert (got, fragment in F.last_error()) == (rc, True), (got, F.last_error())
    assert BAD.value == -7 and (COUNTS == -7).all() and (MINMAX == -7.0).all()          # nothing was written


def test_lab_options_round_trip_under_their_prefixed_names_only():
    for key in ("x_hist_lds", "x_morph_fused"):
        assert F.get_option(key) == 1
        F.set_option(key, 0)
        assert F.get_option(key) == 0
        F.set_option(key, 1)
        with pytest.raises(ValueError, match="unknown option"):
            F.set_option(key[2:], 0)


def test_tile_table_of_the_gpu_tests_is_the_kernels():
    text = open(os.path.join(ROOT, "discorpy_amd", "csrc", "dcp_internal.h")).read()
    m = re.search(r"constexpr int kMorphTW = (\d+), kMorphTH = (\d+);", text)
    assert m, "kMorphTW / kMorphTH are not named constants of dcp_internal.h"
    assert (int(m.group(2)), int(m.group(1))) == (bref.TILE["TH"], bref.TILE["TW"]) == (cases.TH, cases.TW)
    assert bref.SHAPES == cases.SHAPES
    m = re.search(r"constexpr int kHistLdsMaxBins = (\d+);", text)
    assert m and int(m.group(1)) == bref.HIST_LDS_MAX_BINS
    assert 256 < bref.HIST_LDS_MAX_BINS < 65536          # 8-bit counts stay below the switch, 16-bit ones can stand on both sides
    # LARGE and MEDIUM are the labelling tests'; what LARGE promises about minmax_kernel's and histogram_kernel's grid, from the constants
    assert (bref.LARGE, bref.MEDIUM) == (cases.LARGE, cases.MEDIUM)
    found = {}
    for name, source in (("kLabelScanChunk", "dcp_internal.h"), ("kReduceMaxBlocks", "dcp_internal.h"), ("kLabelBlock", "label_kernels.hip"),
                         ("kBinBlock", "binarize_kernels.hip")):
        m = re.search(r"^constexpr int %s = (\d+);" % name, open(os.path.join(ROOT, "discorpy_amd", "csrc", source)).read(), re.M)
        assert m, "%s is not a named constant of %s" % (name, source)
        found[name] = int(m.group(1))
    held = cases.large_conditions(bref.LARGE, found["kLabelScanChunk"], found["kLabelBlock"], found["kReduceMaxBlocks"], found["kBinBlock"])
    assert len(held) == 8 and all(held.values()), [k for k, v in held.items() if not v]
    cap, block, n = found["kReduceMaxBlocks"], found["kBinBlock"], bref.LARGE[0] * bref.LARGE[1]
    assert (cap, block) == (bref.REDUCE_MAX_BLOCKS, bref.BIN_BLOCK)
    assert re.search(r"const int64_t want = \(n \+ kBinBlock \* 8 - 1\) / \(kBinBlock \* 8\);", open(os.path.join(ROOT, "discorpy_amd", "csrc",
                                                                                                          "binarize_kernels.hip")).read())
    rounds = -(-n // (cap * block))
    assert rounds == 10 and (cap - 1) * block + (rounds - 1) * cap * block >= n          # the last workgroup walks one round fewer
    assert 0 < n - (rounds - 1) * cap * block < cap * block and (n - (rounds - 1) * cap * block) % block != 0          # and one is cut short


# ---------------------------------------------------------------------------------------------- the yardstick

def test_scipys_reflect_equals_ignoring_what_lies_outside_for_the_cross():
    rng = np.random.default_rng(11)
    for _ in range(200):
        h, w = rng.integers(1, 12, 2)
        m = (rng.random((h, w)) < rng.random()).astype(np.uint8)
        for op, fn in ((0, bref.erosion), (1, bref.dilation), (2, bref.opening)):
            assert np.array_equal(fn(m), bref.pad_and_ignore(m, op)), (op, m)
    grey = rng.integers(0, 256, (9, 13)).astype(np.uint8)
    for op, fn in ((0, bref.erosion), (1, bref.dilation), (2, bref.opening)):
        assert np.array_equal(fn(grey), bref.pad_and_ignore(grey, op))


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("nbins", [512, 256])
def test_np_histogram_is_a_search_of_its_edges_and_not_its_raw_estimate(dtype, nbins):
    a = bref.edge_hugging(dtype, bref.SHAPES[-1], nbins)
    counts, edges = np.histogram(a, nbins)
    by_search, own_edges = bref.histogram_by_search(a, nbins)
    assert edges.dtype == a.dtype and np.array_equal(edges, own_edges)
    assert np.array_equal(counts, by_search) and counts.sum() == a.size
    assert int((bref.raw_estimate(a, edges) != bref.final_bins(a, edges)).sum()) >= 32


def test_every_stage_of_the_reference_route_changes_the_plane():
    for dtype in ("float32", "float64", "uint16"):
        for bright in (False, True):
            st = bref.binarization_stages(bref.dot_image(dtype, bright))
            assert (not np.array_equal(st["binary"], st["inverted"])) == bright
            for before, after in (("inverted", "cleared"), ("cleared", "opened"), ("opened", "filled")):
                assert not np.array_equal(st[before], st[after]), (dtype, bright, before)
            assert len(bref.points(st["filled"])) > 100


# ---------------------------------------------------------------------------------------------- the Python functions

P = inspect.Parameter


def _sig(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]


def test_signatures_are_the_references_and_scikit_images():
    from discorpy_amd.prep import preprocessing as prep
    # discorpy/prep/preprocessing.py:161, :194, :216
    assert _sig(prep.binarization) == [("mat", P.empty), ("ratio", 0.3), ("thres", None), ("denoise", True)]
    assert _sig(prep._select_roi) == [("mat", P.empty), ("ratio", P.empty), ("square", False)]
    assert _sig(prep._invert_dots_contrast) == [("mat", P.empty)]
    # skimage.filters.threshold_otsu(image=None, nbins=256, ...), segmentation.clear_border(labels, ...), morphology.opening(image, footprint=None, ...)
    assert _sig(prep.threshold_otsu) == [("image", P.empty), ("nbins", 256)]
    assert _sig(prep.clear_border) == [("mat", P.empty)]
    assert _sig(prep.opening) == [("mat", P.empty), ("footprint", None)]
    assert prep.BINARIZATION == ["threshold_otsu", "clear_border", "opening", "binarization"]
    assert all(callable(getattr(prep, name)) for name in prep.BINARIZATION)
    assert prep.__all__ == ["normalization", "median_filter"]
    rest = prep.__doc__.split("out of scope")[0].split("The rest of the reference's module")[1]
    assert "regionprops" in rest and "Radon" in rest and "Otsu" not in rest and "clear_border" not in rest
    assert "UNVERIFIED" in prep.__doc__ and "UNVERIFIED" in open(os.path.join(ROOT, "DESIGN.md")).read()


def test_select_roi_is_a_view_with_the_references_bounds():
    from discorpy_amd.prep import preprocessing as prep
    a = np.arange(300 * 420, dtype=np.float32).reshape(300, 420)
    roi = prep._select_roi(a, 0.3)
    assert np.shares_memory(roi, a) and not roi.flags.owndata and np.array_equal(roi, a[105:195, 147:273]) and np.array_equal(roi, bref.select_roi(a, 0.3))
    assert prep._select_roi(a, 5.0).shape == a.shape and prep._select_roi(a, 0.0).shape == prep._select_roi(a, 0.05).shape
    sq = prep._select_roi(a, 0.5, square=True)
    assert sq.shape == (150, 150) and sq[0, 0] == a[75, 135]


def test_errors_are_raised_before_any_device_call():
    from discorpy_amd.prep import preprocessing as prep
    a = np.ones((4, 4), np.float32)
    for dt in (np.complex64, np.complex128):
        for fn in (prep.threshold_otsu, prep.clear_border, prep.opening, prep.binarization):
            with pytest.raises(TypeError, match="Complex type not supported"):
                fn(np.zeros((4, 4), dt))
    for dt in (np.int32, np.uint32, np.int64, np.uint64, np.bool_):
        with pytest.raises(NotImplementedError, match="8- / 16-bit"):
            prep.threshold_otsu(np.ones((4, 4), dt))
        with pytest.raises(NotImplementedError, match="8- / 16-bit"):
            prep.binarization(np.ones((4, 4), dt))
    for bad in (0, -1):
        with pytest.raises(ValueError, match="`bins` must be positive"):
            prep.threshold_otsu(a, bad)
    with pytest.raises(TypeError):
        prep.threshold_otsu(a, 2.5)
    for bad in (np.ones((3, 3)), np.eye(3), np.ones((5, 5)), [[0, 1, 0], [1, 1, 1], [0, 0, 0]], np.ones(3)):
        with pytest.raises(NotImplementedError, match="footprint"):
            prep.opening(a, bad)
    with pytest.raises(ValueError, match="expected a 2-D array"):
        prep.binarization(np.ones((2, 3, 4), np.float32))
    with pytest.raises(ValueError, match="empty"):
        prep.threshold_otsu(np.zeros((0, 4), np.float32))


def test_empty_images_need_no_device():
    from discorpy_amd.prep import preprocessing as prep
    for shape in ((0, 5), (3, 0)):
        out = prep.binarization(np.zeros(shape, np.float32))
        assert out.shape == shape and out.dtype == np.int16
        for fn in (prep.clear_border, prep.opening):
            got = fn(np.zeros(shape, np.uint16))
            assert got.shape == shape and got.dtype == np.uint16
        assert prep._invert_dots_contrast(np.zeros(shape, np.float32)).shape == shape


def test_a_given_threshold_reduces_to_the_double_numpy_compares_with():
    from discorpy_amd.prep import preprocessing as prep
    assert prep._thres_double(0.1, "float32") == float(np.float32(0.1)) != 0.1          # a Python float is weak
    assert prep._thres_double(np.float64(0.1), "float32") == 0.1                        # a NumPy float64 promotes the comparison
    assert prep._thres_double(np.float32(0.1), "float64") == float(np.float32(0.1))
    assert prep._thres_double(0.1, "float64") == 0.1 and prep._thres_double(0.1, "uint16") == 0.1 and prep._thres_double(7, "int16") == 7.0
    img = np.array([[np.float32(0.1)]], np.float32)
    for thres in (0.1, np.float64(0.1), np.float32(0.1)):
        assert bool((img > thres)[0, 0]) == (float(img[0, 0]) > prep._thres_double(thres, "float32"))


def test_get_points_dot_pattern_still_raises_its_old_message():
    from discorpy_amd.prep import preprocessing as prep
    with pytest.raises(NotImplementedError) as info:
        prep.get_points_dot_pattern(np.zeros((4, 4), np.float32))
    assert str(info.value) == ("binarize=True rests on scikit-image's Otsu threshold (threshold_otsu), clear_border and opening, "
                               "which are not implemented here: binarize the image first and pass binarize=False")
    assert "binarization(mat" in prep.get_points_dot_pattern.__doc__
