"""CPU suite for the rest of the dot-pattern route, discorpy_amd.prep.dotpattern (radon_padded, calc_size_distance, select_dots_based_ratio,
calc_hor_slope / calc_ver_slope, the grouping of dots into lines and the residual filter; dcp_radon_padded_2d, dcp_nearest_sq_dists,
dcp_box_moments_2d): the names, signatures and defaults are the reference's and reachable from prep.preprocessing; the three entry
points are declared, exported and bound and refuse what they do not take before any device work (this machine has no device: reaching
one would answer something else); the point-list paths of the four host functions return golden G29's lines (tools/gen_golden.py: what
the reference returned); the axis lengths from exact integer sums agree with the float-moment helper (tests/helpers/
regionprops_reference.py) on every box of G29; the padded restatement of the Radon transform (tests/helpers/radon_padded_reference.py,
the oracle of tests/test_dot_grid_gpu.py) is held to facts checked by hand and to the circle-free core of radon_reference; and the
documents say what is here, what is not, and what is UNVERIFIED."""
import inspect
import os
import re
import sys

import numpy as np
import pytest
from scipy import ndimage as ndi

from conftest import ROOT, golden

from discorpy_amd import _ffi as F

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import radon_padded_reference as RP  # noqa: E402
import radon_reference as RR  # noqa: E402
import regionprops_reference as RG  # noqa: E402

INV, UNS = F.ERR_INVALID_ARG, F.ERR_UNSUPPORTED
P = inspect.Parameter
K = P.POSITIONAL_OR_KEYWORD
DOT_GRID = ["radon_padded", "calc_size_distance", "select_dots_based_ratio", "calc_hor_slope", "calc_ver_slope", "group_dots_hor_lines",
            "group_dots_ver_lines", "remove_residual_dots_hor", "remove_residual_dots_ver"]


@pytest.fixture(scope="module")
def prep():
    from discorpy_amd.prep import preprocessing
    return preprocessing


@pytest.fixture(scope="module")
def dp():
    from discorpy_amd.prep import dotpattern
    return dotpattern


@pytest.fixture(scope="module")
def g29():
    return golden("g29_dot_grid")


def params(fn):
    return [(p.name, p.default, p.kind) for p in inspect.signature(fn).parameters.values()]


def test_names_signatures_and_defaults_are_the_references(prep, dp):
    import discorpy_amd.prep as package
    assert package.dotpattern is dp
    assert prep.DOT_GRID == DOT_GRID and list(dp.__all__) == DOT_GRID
    for name in DOT_GRID:
        assert callable(getattr(prep, name)) and getattr(prep, name) is getattr(dp, name), name
    assert params(prep.radon_padded) == [("image", P.empty, K), ("theta", None, K)]
    for fn in (prep.calc_size_distance, prep.select_dots_based_ratio, prep.calc_hor_slope, prep.calc_ver_slope):
        assert params(fn) == [("mat", P.empty, K), ("ratio", 0.3, K)], fn.__name__
    assert params(prep.group_dots_hor_lines) == [("mat", P.empty, K), ("slope", P.empty, K), ("dot_dist", P.empty, K), ("ratio", 0.3, K),
                                                 ("num_dot_miss", 6, K), ("accepted_ratio", 0.65, K)]
    assert params(prep.group_dots_ver_lines) == [("mat", P.empty, K), ("slope", P.empty, K), ("dot_dist", P.empty, K), ("ratio", 0.3, K),
                                                 ("num_dot_miss", 6, K), ("accepted_ratio", 0.75, K)]
    for fn in (prep.remove_residual_dots_hor, prep.remove_residual_dots_ver):
        assert params(fn) == [("list_lines", P.empty, K), ("slope", P.empty, K), ("residual", 2.5, K)], fn.__name__
    # what was there stays what it was
    assert params(prep.select_dots_based_distance) == [("mat", P.empty, K), ("dot_dist", P.empty, K), ("ratio", 0.3, K)]
    for name in ("calculate_threshold", "make_parabola_mask", "rotate_points", "remove_subset_points", "group_dots_hor_lines_based_polyfit"):
        assert not hasattr(prep, name), name


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "discorpy_hip.h")).read()
    exports = open(os.path.join(ROOT, "discorpy_amd", "csrc", "exports.map")).read()
    makefile = open(os.path.join(ROOT, "discorpy_amd", "csrc", "Makefile")).read()
    for name, first, nargs in (("dcp_radon_padded_2d", r"const void\* src, double\* dst, int height, int width, ", 11),
                               ("dcp_nearest_sq_dists", r"const double\* points, double\* dst, int npoints, ", 6),
                               ("dcp_box_moments_2d", r"const void\* src, int height, int width, long src_row_stride, int dtype, const int32_t\* boxes, ", 11)):
        assert hasattr(F.lib(), name), name
        assert re.search(r"^int %s\(%s" % (name, first), header, re.M), name
        assert re.search(r"^\s*%s;" % name, exports, re.M), name
        restype, argtypes = F.SIGNATURES[name]
        assert restype is F.C.c_int and len(argtypes) == nargs, name
    assert "dotgrid_kernels.o" in makefile and "api_dotgrid.o" in makefile
    assert len(F.SIGNATURES["dcp_radon_2d"][1]) == 10


# --------------------------------------------------------------------------- refusals, on host buffers; no case reaches a device call

SENTINEL = 0xA5
H, W, NANG = 9, 12, 3
SIDE = RP.padded_side(H, W)
SRC = np.zeros((H, W), np.float32)
SINO = np.full(SIDE * NANG * 8, SENTINEL, np.uint8)
TABLE = RP.angle_table([0.0, 45.0, 90.0], SIDE)
NPTS = 5
PTS = np.arange(2.0 * NPTS).reshape(NPTS, 2)
DIST = np.full(NPTS * 4 * 8, SENTINEL, np.uint8)
MASK = np.zeros((H, W), np.uint8)
NBOX = 2
BOXES = np.array([[0, 3, 0, 4], [2, 8, 5, 11]], np.int32)
SUMS = np.full(NBOX * 6 * 8, SENTINEL, np.uint8)
F32, F64, U8, U16, I32, BOOL = (F.DTYPE_BY_NAME[n] for n in ("float32", "float64", "uint8", "uint16", "int32", "bool"))
_dp = F.C.POINTER(F.C.c_double)


def bad_table(value):
    t = TABLE.copy()
    t[1, 2] = value
    return t


def bad_points(value):
    p = PTS.copy()
    p[3, 1] = value
    return p


def boxes_with(row):
    b = BOXES.copy()
    b[1] = row
    return b


def radon_padded_abi(**o):
    a = dict(src=SRC.ctypes.data, dst=SINO.ctypes.data, height=H, width=W, stride=W, dtype=F32, nangles=NANG, table=TABLE, mem_kind=F.MEM_HOST,
             device=-1, stream=None)
    a.update(o)
    keep = a["table"]
    a["table"] = None if keep is None else keep.ctypes.data_as(_dp)
    return F.lib().dcp_radon_padded_2d(*a.values())


def nearest_abi(**o):
    a = dict(points=PTS, dst=DIST.ctypes.data, npoints=NPTS, mem_kind=F.MEM_HOST, device=-1, stream=None)
    a.update(o)
    keep = a["points"]
    a["points"] = None if keep is None else (keep if isinstance(keep, int) else keep.ctypes.data)
    return F.lib().dcp_nearest_sq_dists(*a.values())


def box_abi(**o):
    a = dict(src=MASK.ctypes.data, height=H, width=W, stride=W, dtype=U8, boxes=BOXES, nboxes=NBOX, sums=SUMS.ctypes.data, mem_kind=F.MEM_HOST,
             device=-1, stream=None)
    a.update(o)
    keep = a["boxes"]
    a["boxes"] = None if keep is None else keep.ctypes.data
    return F.lib().dcp_box_moments_2d(*a.values())


REFUSALS = [
    (radon_padded_abi, dict(src=None), INV, "null src / dst"),
    (radon_padded_abi, dict(dst=None), INV, "null dst / table pointer"),
    (radon_padded_abi, dict(table=None), INV, "null dst / table pointer"),
    (radon_padded_abi, dict(height=0), INV, "height and width must be at least 1"),
    (radon_padded_abi, dict(width=-2), INV, "height and width must be at least 1"),
    (radon_padded_abi, dict(nangles=0), INV, "nangles must be at least 1"),
    (radon_padded_abi, dict(nangles=65536), UNS, "more than 65535 angles"),
    (radon_padded_abi, dict(height=23171), UNS, "padded side above 32768"),
    (radon_padded_abi, dict(width=40000, stride=40000), UNS, "padded side above 32768"),
    (radon_padded_abi, dict(stride=W - 1), INV, "src_row_stride 11 is below the width 12"),
    (radon_padded_abi, dict(dtype=U16), UNS, "float32 or float64"),
    (radon_padded_abi, dict(dtype=BOOL), UNS, "float32 or float64"),
    (radon_padded_abi, dict(dtype=99), INV, "unknown dtype 99"),
    (radon_padded_abi, dict(mem_kind=7), INV, "mem_kind"),
    (radon_padded_abi, dict(dst=SRC.ctypes.data + 8), INV, "src and dst overlap"),
    (radon_padded_abi, dict(dst=SRC.ctypes.data - 8), INV, "src and dst overlap"),
    (radon_padded_abi, dict(table=bad_table(np.nan)), INV, "table entry 6 (angle 1) is not finite"),
    (radon_padded_abi, dict(table=bad_table(-np.inf)), INV, "table entry 6 (angle 1) is not finite"),
    (nearest_abi, dict(points=None), INV, "null src / dst"),
    (nearest_abi, dict(dst=None), INV, "null dst pointer"),
    (nearest_abi, dict(npoints=0), INV, "npoints must be at least 1"),
    (nearest_abi, dict(npoints=-4), INV, "npoints must be at least 1"),
    (nearest_abi, dict(npoints=(1 << 20) + 1), UNS, "more than 1048576 points"),
    (nearest_abi, dict(mem_kind=9), INV, "mem_kind"),
    (nearest_abi, dict(dst=PTS.ctypes.data + 16), INV, "points and dst overlap"),
    (nearest_abi, dict(points=DIST.ctypes.data + 8), INV, "points and dst overlap"),
    (nearest_abi, dict(points=bad_points(np.nan)), INV, "coordinate 1 of point 3 is not finite"),
    (nearest_abi, dict(points=bad_points(np.inf)), INV, "coordinate 1 of point 3 is not finite"),
    (box_abi, dict(src=None), INV, "null src / dst"),
    (box_abi, dict(boxes=None), INV, "null boxes / sums pointer"),
    (box_abi, dict(sums=None), INV, "null boxes / sums pointer"),
    (box_abi, dict(height=0), INV, "height and width must be at least 1"),
    (box_abi, dict(width=-1), INV, "height and width must be at least 1"),
    (box_abi, dict(width=32769, stride=32769), UNS, "above 32768"),
    (box_abi, dict(stride=W - 2), INV, "src_row_stride 10 is below the width 12"),
    (box_abi, dict(dtype=F32), UNS, "bool and 8- / 16-bit integers only"),
    (box_abi, dict(dtype=I32), UNS, "bool and 8- / 16-bit integers only"),
    (box_abi, dict(dtype=-1), INV, "unknown dtype -1"),
    (box_abi, dict(mem_kind=3), INV, "mem_kind"),
    (box_abi, dict(nboxes=-1), INV, "nboxes must not be negative"),
    (box_abi, dict(sums=MASK.ctypes.data + 4), INV, "src and sums overlap"),
    (box_abi, dict(boxes=boxes_with([2, 9, 5, 11])), INV, "box 1 (rows 2..9, columns 5..11) lies outside the 9 x 12 plane"),
    (box_abi, dict(boxes=boxes_with([2, 8, 5, 12])), INV, "box 1 (rows 2..8, columns 5..12) lies outside"),
    (box_abi, dict(boxes=boxes_with([-1, 8, 5, 11])), INV, "box 1 (rows -1..8, columns 5..11) lies outside"),
    (box_abi, dict(boxes=boxes_with([2, 8, -3, 11])), INV, "box 1 (rows 2..8, columns -3..11) lies outside"),
]


@pytest.mark.parametrize("call,override,code,fragment", REFUSALS,
                         ids=["%s-%s-%d" % (c[0].__name__, "-".join(c[1]), i) for i, c in enumerate(REFUSALS)])
def test_entry_points_refuse_before_any_device_work(call, override, code, fragment):
    for out in (SINO, DIST, SUMS):
        out[:] = SENTINEL
    assert call(**override) == code
    assert fragment in F.last_error(), F.last_error()
    for out in (SINO, DIST, SUMS):
        assert (out == SENTINEL).all()


def test_no_box_is_no_work():
    SUMS[:] = SENTINEL
    assert box_abi(nboxes=0, boxes=None, sums=None) == F.OK
    assert (SUMS == SENTINEL).all()


def test_wrappers_refuse_before_any_device_work(prep, dp):
    img = np.zeros((40, 60), np.float32)
    with pytest.raises(TypeError, match="Complex type not supported"):
        prep.radon_padded(img.astype(np.complex64))
    for dt in (np.uint8, np.int16, np.int64, np.bool_):
        with pytest.raises(NotImplementedError, match="float32 and float64 only"):
            prep.radon_padded(img.astype(dt))
    with pytest.raises(RuntimeError, match="data type not supported"):
        prep.radon_padded(img.astype(np.float16))
    for bad in (np.zeros(7, np.float32), np.zeros((2, 3, 4), np.float32)):
        with pytest.raises(ValueError, match="must be 2-D"):
            prep.radon_padded(bad)
    with pytest.raises(ValueError, match="must not be empty"):
        prep.radon_padded(np.zeros((0, 5), np.float32))
    with pytest.raises(ValueError, match="1D sequence"):
        prep.radon_padded(img, theta=np.zeros((2, 2)))
    with pytest.raises(ValueError, match="theta must be finite"):
        prep.radon_padded(img, theta=[0.0, np.nan])
    with pytest.raises(NotImplementedError, match="more than 65535 angles"):
        prep.radon_padded(img, theta=np.zeros(65536))
    empty = prep.radon_padded(img, theta=[])                  # no angle: nothing for a device to do
    assert isinstance(empty, np.ndarray) and empty.shape == (85, 0) and empty.dtype == np.float64
    with pytest.raises(ValueError, match="not a binary image"):
        prep.select_dots_based_ratio(np.array([[0, 2], [1, 0]]))
    with pytest.raises(ValueError, match="must be finite"):
        dp._nearest_sq(np.array([[0.0, 1.0], [np.nan, 2.0]]))
    with pytest.raises(ValueError, match="must be finite"):
        dp._nearest_sq(np.array([[0.0, np.inf]]))
    assert dp._nearest_sq(np.zeros((0, 2))).shape == (0, 4)
    assert dp._box_moments(np.zeros((4, 4), np.uint8), np.zeros((0, 4), np.int32)).shape == (0, 6)
    with pytest.raises(NotImplementedError, match="bool and 8- / 16-bit"):
        dp._box_moments(np.zeros((4, 4), np.float32), BOXES)
    with pytest.raises(NotImplementedError, match="binarize=True"):      # it keeps raising
        prep.get_points_dot_pattern(np.zeros((4, 4)))


# --------------------------------------------------------------------------- golden G29

def lines_of(g, key):
    pts, lens = g[key + "_pts"], g[key + "_len"]
    return np.split(pts, np.cumsum(lens)[:-1])


def same_lines(got, want):
    return len(got) == len(want) and all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(got, want))


def test_g29_loads_and_sits_on_no_tie_and_no_threshold(g29):
    names = [str(n) for n in g29["case_names"]]
    assert names == ["a_90", "a_60", "b_90", "b_60"]
    assert g29["img_a"].shape == (200, 260) and g29["img_b"].shape == (360, 300) and g29["img_a"].dtype == np.uint8
    assert float(g29["select_ratio"]) == 0.3
    for key in ("a", "b"):
        assert set(np.unique(g29["img_" + key])) == {0, 1}
        print("%s: least |val - ratio| / ratio %.3g over %d dots" % (key, g29["margin_" + key], len(g29["vals_" + key])))
        assert g29["margin_" + key] > 1e-6
        assert {"merged", "ellipse_kept", "ellipse_dropped", "neighbour", "crowded_dot", "bar", "block", "pair", "border"} == {str(m) for m in g29["mark_names_" + key]}
    for name in names:
        print("%-5s size %.1f dist %.4f slopes %+.6f %+.6f gaps %.3g %.3g lines %d / %d" % (
            name, g29["size_" + name], g29["dist_" + name], g29["slope_hor_" + name], g29["slope_ver_" + name], g29["gap_hor_" + name],
            g29["gap_ver_" + name], len(g29["hor_" + name + "_len"]), len(g29["ver_" + name + "_len"])))
        assert g29["gap_hor_" + name] > 1e-9 and g29["gap_ver_" + name] > 1e-9, name
        assert len(g29["hor_" + name + "_len"]) >= 8 and len(g29["ver_" + name + "_len"]) >= 8
    assert abs(g29["slope_hor_a_90"] - np.tan(np.deg2rad(2.0))) < 2e-3 and abs(g29["slope_ver_a_90"] + np.tan(np.deg2rad(2.0))) < 2e-3
    assert abs(g29["slope_hor_b_90"] + np.tan(np.deg2rad(1.5))) < 2e-3 and abs(g29["slope_ver_b_90"] - np.tan(np.deg2rad(1.5))) < 2e-3
    assert abs(g29["dist_a_90"] - 20.0) < 0.2 and abs(g29["dist_b_90"] - 24.0) < 0.2
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g29_dot_grid.npz")) <= 1 << 20


@pytest.mark.parametrize("name", ["a_90", "a_60", "b_90", "b_60"])
def test_point_lists_are_grouped_and_filtered_as_the_reference_does(prep, g29, name):
    points = g29["points_" + name]
    slope_hor, slope_ver, dist = g29["slope_hor_" + name], g29["slope_ver_" + name], g29["dist_" + name]
    hor = prep.group_dots_hor_lines(points, slope_hor, dist)
    ver = prep.group_dots_ver_lines(points, slope_ver, dist)
    assert same_lines(hor, lines_of(g29, "hor_" + name)) and same_lines(ver, lines_of(g29, "ver_" + name))
    assert same_lines(prep.remove_residual_dots_hor(hor, slope_hor), lines_of(g29, "hor2_" + name))
    assert same_lines(prep.remove_residual_dots_ver(ver, slope_ver), lines_of(g29, "ver2_" + name))
    # a tighter residual drops dots
    tight = prep.remove_residual_dots_hor(hor, slope_hor, residual=0.05)
    assert sum(len(line) for line in tight) < sum(len(line) for line in hor)
    # a list of lists and Python floats are taken as well
    assert same_lines(prep.group_dots_hor_lines(points.tolist(), float(slope_hor), float(dist)), hor)


def test_grouping_messages_and_small_inputs(prep):
    with pytest.raises(ValueError, match="Input is empty!!!"):
        prep.group_dots_hor_lines(np.zeros((0, 2)), 0.0, 10.0)
    with pytest.raises(ValueError, match="Input is empty!!!"):
        prep.group_dots_ver_lines(np.zeros((0, 2)), 0.0, 10.0)
    with pytest.raises(ValueError, match="No dots left"):
        prep.remove_residual_dots_hor([np.array([[0.0, 0.0], [5.0, 10.0], [0.0, 20.0], [7.0, 30.0]])], 0.0, residual=1e-3)
    with pytest.raises(ValueError, match="No dots left"):
        prep.remove_residual_dots_ver([], 0.0)
    with pytest.raises(ValueError):                               # no line at all: NumPy's own error for the maximum of nothing
        prep.group_dots_hor_lines(np.array([[0.0, 0.0]]), 0.0, 10.0)
    # two rows of a 10-pixel lattice, shuffled; integer input keeps its type
    pts = np.array([[y, x] for y in (0, 10) for x in range(0, 60, 10)])
    rng = np.random.default_rng(3)
    hor = prep.group_dots_hor_lines(pts[rng.permutation(len(pts))], 0.0, 10.0)
    assert [line.tolist() for line in hor] == [[[0, x] for x in range(0, 60, 10)], [[10, x] for x in range(0, 60, 10)]]
    assert hor[0].dtype == pts.dtype
    ver = prep.group_dots_ver_lines(pts[rng.permutation(len(pts))], 0.0, 10.0, accepted_ratio=0.5)
    assert [line.tolist() for line in ver] == [[[0, x], [10, x]] for x in range(0, 60, 10)]
    # a missing dot is bridged up to num_dot_miss pitches, not beyond
    gap = np.array([[0.0, 0.0], [0.0, 10.0], [0.0, 50.0], [0.0, 60.0]])
    assert [len(line) for line in prep.group_dots_hor_lines(gap, 0.0, 10.0)] == [4]
    assert [len(line) for line in prep.group_dots_hor_lines(gap, 0.0, 10.0, num_dot_miss=3)] == [2, 2]


def box_sums(sub):
    ys, xs = np.nonzero(sub)
    ys, xs = ys.astype(np.int64), xs.astype(np.int64)
    return [len(ys), ys.sum(), xs.sum(), (ys * ys).sum(), (xs * ys).sum(), (xs * xs).sum()]


@pytest.mark.parametrize("key", ["a", "b"])
def test_axis_lengths_from_integer_sums_agree_with_float_moments(dp, g29, key):
    img = g29["img_" + key]
    ratio = float(g29["select_ratio"])
    labels, num = ndi.label(img)
    kept = np.zeros(img.shape, np.uint8)
    vals, worst = [], 0.0
    for box in ndi.find_objects(labels):
        sub = img[box]
        if min(sub.shape) < 2:
            continue
        major, minor = dp._axis_lengths(box_sums(sub))
        want_major, want_minor = RG.axis_lengths(sub)
        worst = max(worst, abs(major - want_major) / want_major, abs(minor - want_minor) / want_minor)
        val = dp._axes_ratio_value(box_sums(sub))
        vals.append(val)
        assert (val < ratio) == (abs(want_major / want_minor - 1.0) < ratio)
        if val < ratio:
            kept[box] = sub
    print("%s: %d boxes, lengths within %.3g relative" % (key, len(vals), worst))
    assert worst <= 1e-9
    assert np.abs(np.array(vals) - g29["vals_" + key]).max() <= 1e-9
    assert np.array_equal(kept, g29["kept_ratio_" + key])          # the reference's own mask
    marks = {str(m): tuple(p) for m, p in zip(g29["mark_names_" + key], g29["marks_" + key])}
    want = dict(merged=0, ellipse_kept=1, ellipse_dropped=0, neighbour=1, crowded_dot=1, bar=0, block=1, pair=0)
    assert {m: int(kept[marks[m]]) for m in want} == want


def test_axis_lengths_of_shapes_known_by_hand(dp):
    # a 2 x 2 block: both central moments 1 / 4, both lengths 2; an n x 1 bar has a minor axis of 0: inf, and no warning
    assert dp._axis_lengths(box_sums(np.ones((2, 2)))) == (2.0, 2.0) and dp._axes_ratio_value(box_sums(np.ones((2, 2)))) == 0.0
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert dp._axes_ratio_value(box_sums(np.ones((1, 7)))) == float("inf")
        assert dp._axes_ratio_value(box_sums(np.eye(5))) == float("inf")
    # a w x h rectangle: variances (w^2 - 1) / 12 and (h^2 - 1) / 12
    major, minor = dp._axis_lengths(box_sums(np.ones((5, 11))))
    assert major == 4.0 * np.sqrt(10.0) and minor == 4.0 * np.sqrt(2.0)
    # sums as large as a 32768-wide box gives them stay exact: a full 3 x 32768 box
    n, w = 3 * 32768, 32768
    sx, sxx = 3 * (w * (w - 1) // 2), 3 * ((w - 1) * w * (2 * w - 1) // 6)
    major, minor = dp._axis_lengths([n, n, sx, 5 * w, sx, sxx])
    assert abs(major - 4.0 * np.sqrt((w * w - 1) / 12.0)) <= 1e-9 * major and abs(minor - 4.0 * np.sqrt(2.0 / 3.0)) <= 1e-9


# --------------------------------------------------------------------------- the padded restatement of the Radon transform

def test_padded_side_and_corner(dp):
    assert [RP.padded_side(*s) for s in ((1, 1), (1, 2), (3, 5), (64, 64), (40, 97), (23170, 5))] == [2, 3, 8, 91, 138, 32768]
    square, (py, px) = RP.pad_square(np.ones((3, 5)))
    assert square.shape == (8, 8) and (py, px) == (3, 2) and square.sum() == 15 and square[3:6, 2:7].all()
    for s in ((1, 1), (2, 1), (63, 65), (600, 600), (2048, 2047), (23170, 1)):
        assert dp._padded_side(*s) == RP.padded_side(*s)
    assert RP.padded_side(23171, 1) > 32768


@pytest.mark.parametrize("shape", [(1, 1), (1, 2), (2, 1), (3, 5), (5, 3), (40, 97), (64, 64)])
def test_padded_restatement_at_0_and_90_degree_is_row_and_column_sums(shape):
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    img = rng.integers(-9, 10, shape).astype(np.float32)
    square, (py, px) = RP.pad_square(img)
    side = square.shape[0]
    got = RP.radon(img, [0.0, 90.0])
    assert got.shape == (side, 2) and got.dtype == np.float64
    # 0 degree is the identity: exactly the column sums of the square
    assert np.array_equal(got[:, 0], square.sum(0)) and np.array_equal(got[px:px + shape[1], 0], img.astype(np.float64).sum(0))
    # 90 degree: cos is 6e-17, not 0, so the samples sit 1e-14 off the lattice; the projection is the row sums, bottom row first,
    # to that accuracy (turned about (c0, c0): row y lands on column 2 c0 - y)
    c0 = side // 2
    rows = square.sum(1)
    want = np.zeros(side)
    for y in range(side):
        if 0 <= 2 * c0 - y < side:
            want[2 * c0 - y] = rows[y]
    assert np.abs(got[:, 1] - want).max() <= 1e-11 * max(1.0, np.abs(img).sum())


@pytest.mark.parametrize("shape", [(3, 5), (40, 97), (65, 63)])
def test_padded_restatement_is_the_circle_free_core_of_radon_reference(shape):
    """radon_reference transforms a square inside its inscribed circle, about its own centre.  The padded square of an image, set into
    a square twice its side so that the two centres coincide, lies inside that circle whole; the big square's sinogram, cut to the
    padded square's columns, is then the padded sinogram -- the same samples, the big one adding exact zeros before and after."""
    rng = np.random.default_rng(7)
    img = rng.random(shape)
    square, _ = RP.pad_square(img)
    side = square.shape[0]
    first = side - side // 2                                   # the padded centre (side // 2) on the big centre (2 side) // 2 = side
    big = np.zeros((2 * side, 2 * side))
    big[first:first + side, first:first + side] = square
    theta = [0.0, 90.0, 45.0, -30.0, 17.3]
    want = RR.radon(big, theta)[first:first + side]
    got = RP.radon(img, theta)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_corners_survive_without_the_circle():
    img = np.zeros((64, 64), np.float32)
    img[0, 0] = img[0, -1] = img[-1, 0] = img[-1, -1] = 1.0
    assert RR.radon(img, [45.0]).sum() == 0.0                     # the circle drops them
    assert RP.radon(img, [45.0]).sum() > 3.0


# --------------------------------------------------------------------------- documents

def test_documents_say_what_is_here_and_what_is_not(prep, dp):
    doc = prep.__doc__
    rest = doc.split("The rest of the reference's module")[1].split("out of scope")[0]
    assert "regionprops" in rest and "Radon" in rest and "dotpattern" in rest
    for word in ("labelling", "Otsu", "clear_border"):
        assert word not in rest, word
    for word in ("Radon-based angle search", "scikit-image", "out of scope", "UNVERIFIED", "DOT_GRID"):
        assert word in doc, word
    out = dp.__doc__.split("Out of scope")[1]
    for word in ("calculate_threshold", "parabola", "rotate_points", "remove_subset_points", "polyfit", "binarize=True", "proc"):
        assert word in out, word
    for word in ("UNVERIFIED", "dcp_radon_padded_2d", "dcp_nearest_sq_dists", "dcp_box_moments_2d", "per box, not per", "regionprops_reference",
                 "radon_padded_reference"):
        assert word in dp.__doc__, word
    assert "UNVERIFIED" in prep.radon_padded.__doc__ and "UNVERIFIED" in prep.select_dots_based_ratio.__doc__
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design.split("Dot grid")[1]
    for word in ("UNVERIFIED", "dcp_radon_padded_2d", "dcp_nearest_sq_dists", "dcp_box_moments_2d", "per box"):
        assert word in section, word
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "calc_hor_slope" in readme and "select_dots_based_ratio" in readme and "time_label.py --dotgrid" in readme
    assert "needs scikit-image and is not here" not in readme
    for helper in ("radon_padded_reference.py", "regionprops_reference.py"):
        assert "UNVERIFIED" in open(os.path.join(ROOT, "tests", "helpers", helper)).read()
