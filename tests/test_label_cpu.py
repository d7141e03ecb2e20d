"""CPU suite for labelling, dot measurements and hole filling: dcp_label_2d, dcp_label_measures_2d and dcp_fill_holes_2d are exported,
declared and bound; every argument they refuse is refused with its code and a message that names the argument before any device work
(the buffers are host memory, no GPU is visible to these cases); discorpy_amd.prep.preprocessing offers the functions with the
reference's (and scipy's) signatures and raises what it says it raises without a device; the tile table of the GPU tests is the
kernels'."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import dots_reference as dref  # noqa: E402
import label_cases as cases  # noqa: E402

from discorpy_amd import _ffi as F  # noqa: E402

INV, UNS = F.ERR_INVALID_ARG, F.ERR_UNSUPPORTED
H, W = 8, 10
SRC = np.zeros(H * (W + 4) * 8, np.uint8)
DST = np.zeros(H * W * 8, np.uint8)
NUM = F.C.c_int(-7)
SUMS = np.zeros((5, 4), np.int64)
BOXES = np.zeros((5, 4), np.int32)
U16 = F.DTYPE_BY_NAME["uint16"]

LABEL = dict(src=SRC.ctypes.data, dst=DST.ctypes.data, height=H, width=W, stride=W, dtype=U16, connectivity=4, num=F.C.byref(NUM),
             mem_kind=F.MEM_HOST, device=-1, stream=None)
LABEL_ORDER = "src dst height width stride dtype connectivity num mem_kind device stream".split()
FILL = dict(src=SRC.ctypes.data, dst=DST.ctypes.data, height=H, width=W, stride=W, dtype=U16, mem_kind=F.MEM_HOST, device=-1, stream=None)
FILL_ORDER = "src dst height width stride dtype mem_kind device stream".split()
MEAS = dict(weights=SRC.ctypes.data, labels=DST.ctypes.data, height=H, width=W, wstride=W, lstride=W, dtype=U16, num_labels=5,
            sums=SUMS.ctypes.data, boxes=BOXES.ctypes.data, mem_kind=F.MEM_HOST, device=-1, stream=None)
MEAS_ORDER = "weights labels height width wstride lstride dtype num_labels sums boxes mem_kind device stream".split()


def call(name, valid, order, override):
    args = dict(valid, **override)
    return getattr(F.lib(), name)(*[args[k] for k in order])


@pytest.mark.parametrize("symbol,head,nargs", [
    ("dcp_label_2d", r"const void\* src, int32_t\* dst, int height, int width, long src_row_stride, int dtype, int connectivity", 11),
    ("dcp_label_measures_2d", r"const void\* weights, const int32_t\* labels, int height, int width, long weights_row_stride", 13),
    ("dcp_fill_holes_2d", r"const void\* src, uint8_t\* dst, int height, int width, long src_row_stride, int dtype, int mem_kind", 9)])
def test_symbols_are_exported_declared_and_bound(symbol, head, nargs):
    assert hasattr(F.lib(), symbol)
    header = open(os.path.join(ROOT, "include", "discorpy_hip.h")).read()
    assert re.search(r"^int %s\(%s" % (symbol, head), header, re.M)
    assert "SYNCHRONISES `stream` BEFORE IT RETURNS" in header
    exports = open(os.path.join(ROOT, "discorpy_amd", "csrc", "exports.map")).read()
    assert re.search(r"^\s*%s;" % symbol, exports, re.M), "not named in csrc/exports.map"
    restype, argtypes = F.SIGNATURES[symbol]
    assert restype is F.C.c_int and len(argtypes) == nargs and argtypes[4] is F.C.c_long
    makefile = open(os.path.join(ROOT, "discorpy_amd", "csrc", "Makefile")).read()
    assert "api_label.o" in makefile and "label_kernels.o" in makefile


SHARED = [
    (dict(height=0), INV, "height"),
    (dict(width=0), INV, "width"),
    (dict(height=-1), INV, "height"),
    (dict(stride=W - 1), INV, "src_row_stride"),
    (dict(dtype=99), INV, "dtype"),
    (dict(dtype=-1), INV, "dtype"),
    (dict(mem_kind=7), INV, "mem_kind"),
    (dict(mem_kind=F.MEM_DEVICE_UNORDERED), INV, "mem_kind"),
    (dict(src=None), INV, "src"),
    (dict(dst=None), INV, "dst"),
    (dict(dst=SRC.ctypes.data), INV, "overlap"),
    (dict(stride=W + 4, dst=SRC.ctypes.data + 2 * ((H - 1) * (W + 4) + W - 1)), INV, "overlap"),     # the last source element is the first of dst
    (dict(height=65536, width=32768, stride=32768), UNS, "height * width"),
    (dict(height=2, width=1073741824, stride=1073741824), UNS, "height * width"),
]
LABEL_CASES = SHARED + [(dict(connectivity=6), INV, "connectivity"), (dict(connectivity=0), INV, "connectivity"),
                        (dict(connectivity=-8), INV, "connectivity"), (dict(num=None), INV, "num_labels_out")]
MEAS_CASES = [
    (dict(height=0), INV, "height"),
    (dict(width=-2), INV, "width"),
    (dict(labels=None), INV, "labels"),
    (dict(sums=None), INV, "sums"),
    (dict(boxes=None), INV, "boxes"),
    (dict(lstride=W - 1), INV, "labels_row_stride"),
    (dict(wstride=W - 1), INV, "weights_row_stride"),
    (dict(dtype=99), INV, "dtype"),
    (dict(dtype=-1), INV, "dtype"),
    (dict(mem_kind=7), INV, "mem_kind"),
    (dict(num_labels=-1), INV, "num_labels"),
    (dict(dtype=F.DTYPE_BY_NAME["float32"]), UNS, "dtype"),
    (dict(dtype=F.DTYPE_BY_NAME["float64"]), UNS, "dtype"),
    (dict(dtype=F.DTYPE_BY_NAME["int32"]), UNS, "dtype"),
    (dict(dtype=F.DTYPE_BY_NAME["uint64"]), UNS, "dtype"),
    (dict(height=65536, width=32768, wstride=32768, lstride=32768), UNS, "height * width"),
    (dict(height=1 << 17, width=1 << 13, wstride=1 << 13, lstride=1 << 13), UNS, "max(height, width)"),   # 2^30 x 2^17 x 2^16 = 2^63
    (dict(weights=None, height=1 << 13, width=1 << 17, lstride=1 << 17), UNS, "max(height, width)"),
]


def _ids(table):
    return ["-".join("%s=%s" % (k, v if k not in ("src", "dst", "num", "weights", "labels", "sums", "boxes") else "x") for k, v in sorted(c[0].items()))
            for c in table]


@pytest.mark.parametrize("override,rc,fragment", LABEL_CASES, ids=_ids(LABEL_CASES))
def test_label_refuses(override, rc, fragment):
    got = call("dcp_label_2d", LABEL, LABEL_ORDER, override)
    assert (got, fragment in F.last_error()) == (rc, True), (got, F.last_error())
    assert NUM.value == -7                                    # nothing was written


@pytest.mark.parametrize("override,rc,fragment", SHARED, ids=_ids(SHARED))
def test_fill_holes_refuses(override, rc, fragment):
    if override.get("dst") == SRC.ctypes.data + 2 * ((H - 1) * (W + 4) + W - 1):
        override = dict(override, dst=SRC.ctypes.data + 2 * ((H - 1) * (W + 4) + W) - 1)          # dst is bytes: its first one on the source's last
    got = call("dcp_fill_holes_2d", FILL, FILL_ORDER, override)
    assert (got, fragment in F.last_error()) == (rc, True), (got, F.last_error())


@pytest.mark.parametrize("override,rc,fragment", MEAS_CASES, ids=_ids(MEAS_CASES))
def test_measures_refuse(override, rc, fragment):
    got = call("dcp_label_measures_2d", MEAS, MEAS_ORDER, override)
    assert (got, fragment in F.last_error()) == (rc, True), (got, F.last_error())


def test_largest_frame_the_measures_take_passes_the_checks():
    """2^17 x (2^13 - 1): height * width * max * 65536 = 2^63 - 2^50.  Null weights and no label to measure: the call returns before
    any transfer (DCP_OK), or fails in the device layer where no GPU is visible -- but not in the argument checks."""
    got = call("dcp_label_measures_2d", MEAS, MEAS_ORDER, dict(weights=None, height=1 << 17, width=(1 << 13) - 1, lstride=1 << 13, num_labels=0))
    assert got in (F.OK, F.ERR_HIP, F.ERR_NO_DEVICE), (got, F.last_error())


def test_buffers_that_touch_but_do_not_overlap_pass_the_checks():
    got = call("dcp_label_2d", LABEL, LABEL_ORDER, dict(stride=W + 4, dst=SRC.ctypes.data + 2 * ((H - 1) * (W + 4) + W)))
    assert got in (F.OK, F.ERR_HIP, F.ERR_NO_DEVICE), (got, F.last_error())


def test_lab_option_round_trips_under_its_prefixed_name_only():
    assert F.get_option("x_label_lds") == 1
    F.set_option("x_label_lds", 0)
    assert F.get_option("x_label_lds") == 0
    F.set_option("x_label_lds", 1)
    with pytest.raises(ValueError, match="unknown option"):
        F.set_option("label_lds", 0)


def kernel_constants():
    """kLabelScanChunk and kReduceMaxBlocks of dcp_internal.h, kLabelBlock and kBinBlock of the two kernel files."""
    csrc = os.path.join(ROOT, "discorpy_amd", "csrc")
    found = {}
    for name, source in (("kLabelScanChunk", "dcp_internal.h"), ("kReduceMaxBlocks", "dcp_internal.h"), ("kLabelBlock", "label_kernels.hip"),
                         ("kBinBlock", "binarize_kernels.hip")):
        m = re.search(r"^constexpr int %s = (\d+);" % name, open(os.path.join(csrc, source)).read(), re.M)
        assert m, "%s is not a named constant of %s" % (name, source)
        found[name] = int(m.group(1))
    return found


def test_tile_table_of_the_gpu_tests_is_the_kernels():
    text = open(os.path.join(ROOT, "discorpy_amd", "csrc", "dcp_internal.h")).read()
    m = re.search(r"constexpr int kLabelTW = (\d+), kLabelTH = (\d+);", text)
    assert m, "kLabelTW / kLabelTH are not named constants of dcp_internal.h"
    assert (int(m.group(2)), int(m.group(1))) == (cases.TILE["TH"], cases.TILE["TW"])
    th, tw = cases.TH, cases.TW
    assert cases.SHAPES == [(1, 1), (1, 2 * tw + 3), (2 * th + 3, 1), (th, tw), (th + 1, tw + 1), (2 * th + 5, 3 * tw + 7)]
    assert cases.BIG == cases.SHAPES[-1] and cases.MEDIUM == (5 * th + 3, 4 * tw + 5) == (163, 517)
    # LARGE turns the loops of label_scan_kernel, minmax_kernel and histogram_kernel that the shapes above never turn
    const = kernel_constants()
    assert const == {"kLabelScanChunk": 4096, "kLabelBlock": 256, "kReduceMaxBlocks": 1024, "kBinBlock": 256}, "a constant moved: derive LARGE again"
    args = (const["kLabelScanChunk"], const["kLabelBlock"], const["kReduceMaxBlocks"], const["kBinBlock"])
    held = cases.large_conditions(cases.LARGE, *args)
    assert len(held) == 8 and all(held.values()), [k for k, v in held.items() if not v]
    n = cases.LARGE[0] * cases.LARGE[1]
    assert (n, -(-n // const["kLabelScanChunk"])) == (2540209, 621)
    # the conditions tell: each of these frames misses what is named and nothing else (with these constants three scan rounds and the
    # capped grid both begin above 2^21 pixels)
    scan, cap = "three scan rounds, two of them full", "the cap of the reduce grid is reached"
    for shape, missed in (((601, 4099), ["ragged tile, wider than a wave"]), ((600, 4095), ["no row and no plane of whole quads"]),
                          ((601, 2303), [scan, cap]), ((745, 4223), ["the partial scan round crosses a wave"]),
                          ((807, 4223), ["the last reduce round is ragged between workgroups"]),
                          ((601, 16511), ["float64 sums of 16-bit weights are exact"]), ((4099, 4223), ["below 2^24 pixels"])):
        got = cases.large_conditions(shape, *args)
        assert [k for k, v in got.items() if not v] == missed, (shape, missed)
    assert not cases.large_conditions(cases.BIG, *args)[scan] and not cases.large_conditions(cases.BIG, *args)[cap]


# ---------------------------------------------------------------------------------------------- the Python functions

P = inspect.Parameter


def _sig(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]


def test_signatures_are_the_references_and_scipys():
    from discorpy_amd.prep import preprocessing as prep
    # discorpy/prep/preprocessing.py:251, :332, :422, :966
    assert _sig(prep.check_num_dots) == [("mat", P.empty)]
    assert _sig(prep.select_dots_based_size) == [("mat", P.empty), ("dot_size", P.empty), ("ratio", 0.3)]
    assert _sig(prep.select_dots_based_distance) == [("mat", P.empty), ("dot_dist", P.empty), ("ratio", 0.3)]
    assert _sig(prep.get_points_dot_pattern) == [("mat", P.empty), ("binarize", True), ("ratio", 0.3), ("thres", None)]
    # scipy.ndimage, with the first argument under this package's name for an image
    from scipy import ndimage as ndi
    for name in ("label", "sum_labels", "center_of_mass", "find_objects", "binary_fill_holes"):
        ours, theirs = _sig(getattr(prep, name)), _sig(getattr(ndi, name))
        assert [p[0] for p in ours[1:]] == [p[0] for p in theirs[1:len(ours)]] and [p[1] for p in ours] == [p[1] for p in theirs[:len(ours)]], name
    assert set(prep.DOT_PATTERN) == {"label", "sum_labels", "center_of_mass", "find_objects", "binary_fill_holes", "check_num_dots",
                                     "get_points_dot_pattern", "select_dots_based_size", "select_dots_based_distance"}
    assert all(callable(getattr(prep, name)) for name in prep.DOT_PATTERN)
    assert "labelling" not in prep.__doc__.split("out of scope")[0].split("The rest of the reference's module")[1]


def test_structures_other_than_the_cross_and_the_block_raise():
    from discorpy_amd.prep import preprocessing as prep
    a = np.ones((4, 4), np.uint8)
    for bad in ([[1, 1, 0], [1, 1, 1], [0, 1, 1]], np.eye(3), np.zeros((3, 3))):
        with pytest.raises(NotImplementedError, match="structure"):
            prep.label(a, bad)
    with pytest.raises(ValueError, match="structure dimensions must be equal to 3"):
        prep.label(a, np.ones((5, 5)))
    with pytest.raises(RuntimeError, match="structure and input must have equal rank"):
        prep.label(a, np.ones(3))
    assert prep._connectivity(None) == 4 and prep._connectivity(cases.CROSS.astype(np.float64)) == 4 and prep._connectivity(np.full((3, 3), 7)) == 8


@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
def test_complex_input_raises_scipys_error(dt):
    from discorpy_amd.prep import preprocessing as prep
    with pytest.raises(TypeError, match="Complex type not supported"):
        prep.label(np.zeros((4, 4), dt))
    with pytest.raises(TypeError, match="Complex type not supported"):
        prep.binary_fill_holes(np.zeros((4, 4), dt))


@pytest.mark.parametrize("dt", [np.float32, np.float64, np.int32, np.uint32, np.int64, np.uint64])
def test_float_and_wide_integer_weights_raise(dt):
    from discorpy_amd.prep import preprocessing as prep
    labels = np.ones((4, 4), np.int32)
    for fn in (prep.sum_labels, prep.center_of_mass):
        with pytest.raises(NotImplementedError, match="8- / 16-bit"):
            fn(np.ones((4, 4), dt), labels, 1)


def test_binarize_raises_and_names_what_is_missing():
    from discorpy_amd.prep import preprocessing as prep
    for kw in ({}, {"binarize": True}):
        with pytest.raises(NotImplementedError) as info:
            prep.get_points_dot_pattern(np.zeros((4, 4), np.float32), **kw)
        assert all(word in str(info.value) for word in ("scikit-image", "Otsu", "clear_border", "opening"))


@pytest.mark.parametrize("values", [(0.0, 0.5), (0.0, 2.0), (1.0, 1.0), (0.0, 0.0), (-1.0, 1.0), (0.0, 0.5, 1.0), (0.0, np.nan, 1.0)],
                         ids=lambda v: "_".join(str(x) for x in v))
def test_non_binary_input_raises_the_references_error(values):
    from discorpy_amd.prep import preprocessing as prep
    a = np.resize(np.array(values, np.float32), (5, 6))
    with pytest.raises(ValueError) as info:
        prep.get_points_dot_pattern(a, binarize=False)
    assert str(info.value) == dref.BINARY_ERROR == "Input not a binary image, e.i. maximum_value=1 and minimum value=0!!!"


def test_empty_images_and_label_tables_need_no_device():
    from discorpy_amd.prep import preprocessing as prep
    lab, num = prep.label(np.zeros((0, 5), np.uint8))
    assert lab.shape == (0, 5) and lab.dtype == np.int32 and num == 0
    assert prep.binary_fill_holes(np.zeros((3, 0), np.float32)).dtype == np.bool_
    zero = np.zeros((4, 4), np.int32)
    assert prep.find_objects(zero) == [] and prep.find_objects(zero, 3) == [None, None, None]
    assert prep.center_of_mass(np.zeros((4, 4), np.uint8), zero, []) == []
    assert prep.sum_labels(np.zeros((4, 4), np.uint8), zero, []).shape == (0,)


@pytest.mark.parametrize("dtype,value", [(np.int64, (1 << 32) + 1), (np.int64, 1 << 31), (np.int64, -(1 << 31) - 1), (np.uint32, (1 << 31) + 5),
                                         (np.uint64, 1 << 40)], ids=lambda v: str(getattr(v, "__name__", v)))
def test_labels_that_would_wrap_in_int32_are_refused(dtype, value):
    """(2^32 + 1 cast to int32 is 1: the huge label would be measured as label 1.)"""
    from discorpy_amd.prep import preprocessing as prep
    labels = np.ones((4, 4), dtype)
    labels[2, 3] = value
    mat = np.ones((4, 4), np.uint8)
    for call in (lambda: prep.sum_labels(mat, labels, 1), lambda: prep.center_of_mass(mat, labels, [1]), lambda: prep.find_objects(labels, 1)):
        with pytest.raises(NotImplementedError, match="int32 range"):
            call()
    with pytest.raises(TypeError, match="labels must be integers"):
        prep.sum_labels(mat, np.ones((4, 4), np.float32), 1)
