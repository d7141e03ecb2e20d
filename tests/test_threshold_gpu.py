"""GPU suite for discorpy_amd.prep.threshold and .complete (csrc/sort_kernels.hip).

The sort is held to np.sort(a, axis=None) by == (NaNs equal), on the smallest shapes at which each mechanism can fail: one element, one
short row, less than a tile, several 4096-key tiles with a ragged last one (257 x 263) and a row-strided view of it; 70 000 elements of
three values put one bin across many tiles and waves, which an unstable scatter does not survive past the first digit.  The zoom is
held to tests/helpers/sorted_zoom_reference.py by == for every type and to scipy under the rule of tests/test_threshold_cpu.py (==
for float32 and integers, F64_ULPS for float64).  calculate_threshold is held to golden G31 and, for float32 and integers, by == to the
reference's formula on scipy's own sorted and zoomed profile."""
import os
import sys

import numpy as np
import pytest
import scipy.ndimage as ndi

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import sorted_zoom_reference as szr  # noqa: E402
from test_threshold_cpu import DTYPES, F64_ULPS, G31, window_ulps  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 7), (37, 53), (257, 263)]


@pytest.fixture(scope="module")
def thr(hip):
    from discorpy_amd.prep import threshold
    return threshold


@pytest.fixture(scope="module")
def complete(hip):
    from discorpy_amd.prep import complete
    return complete


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def unsigned_view(dt):
    return np.dtype("u%d" % np.dtype(dt).itemsize)


def plane(kind, dtype, shape, seed=0):
    """A plane of ``dtype`` for one of the data kinds of the sort tests."""
    dt, n = np.dtype(dtype), shape[0] * shape[1]
    rng = np.random.default_rng(seed + 17 * n)
    u = unsigned_view(dt)
    top = 8 * (dt.itemsize - 1)
    if kind == "random":          # every bit pattern (floats: NaNs of both signs, infinities and denormals among them)
        a = rng.integers(0, np.iinfo(u).max, n, dtype=u, endpoint=True).view(dt)
    elif kind == "equal":
        a = np.full(n, 3, u).view(dt) if dt.kind != "f" else np.full(n, -2.5, dt)
    elif kind in ("two", "three"):
        values = np.array([-7.25, 3.5, 1e-3], dt) if dt.kind == "f" else np.array([200, 3, 77], u).view(dt)
        a = values[rng.integers(0, 2 if kind == "two" else 3, n)]
    elif kind in ("ascending", "descending"):
        a = np.sort(rng.integers(0, np.iinfo(u).max, n, dtype=u, endpoint=True).view(dt))
        if dt.kind == "f":
            a = np.sort(a[~np.isnan(a)])
            a = np.resize(a, n) if len(a) else np.zeros(n, dt)
            a = np.sort(a)
        a = a[::-1].copy() if kind == "descending" else a
    elif kind == "low_byte":          # keys that differ in their lowest byte only (floats: positive, so keys keep the bytes' order)
        a = (np.full(n, 0x3f << top if dt.itemsize > 1 else 0, u) | rng.integers(0, 255, n, dtype=u, endpoint=True)).view(dt)
    elif kind == "high_byte":         # ... and in their highest only
        a = (np.full(n, 0x55 if dt.itemsize > 1 else 0, u) | (rng.integers(0, 255, n, dtype=u, endpoint=True) << u.type(top))).view(dt)
    elif kind == "special":
        tiny = np.finfo(dt).tiny
        pool = np.array([0.0, -0.0, np.inf, -np.inf, tiny / 2, -tiny / 2, tiny / 1024, np.nan, -np.nan, 1.0, -1.0, np.finfo(dt).max], dt)
        a = pool[rng.integers(0, len(pool), n)]
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(a).reshape(shape)


KINDS = ["random", "equal", "two", "ascending", "descending", "low_byte", "high_byte"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_sort_equals_np_sort(thr, dtype, kind):
    for shape in SHAPES:
        a = plane(kind, dtype, shape)
        got = thr.sort_values(a)
        assert same(got, np.sort(a, axis=None)), (shape, kind)
        assert got.tobytes() == szr.sort_reference(a).tobytes(), (shape, kind)          # also what NumPy leaves open


@pytest.mark.parametrize("dtype", DTYPES)
def test_sort_of_a_row_strided_view(thr, dtype):
    big = plane("random", dtype, (257, 263 + 11), seed=3)
    view = big[:, 4:-7]
    assert not view.flags.c_contiguous
    assert same(thr.sort_values(view), np.sort(view, axis=None))


@pytest.mark.parametrize("dtype", DTYPES)
def test_sort_of_three_values_across_many_tiles_is_stable_through_every_digit(thr, dtype):
    a = plane("three", dtype, (250, 280))          # 70 000 elements: 18 tiles, every bin of a pass spans all of them
    assert same(thr.sort_values(a), np.sort(a, axis=None))
    # and with a second digit that must keep the first one's order: the three values times 256 low bytes
    u = unsigned_view(dtype)
    if u.itemsize > 1:
        rng = np.random.default_rng(8)
        b = ((a.view(u) & u.type(~np.uint64(0xff) & np.uint64(np.iinfo(u).max))) | rng.integers(0, 255, a.shape, dtype=u, endpoint=True)).view(a.dtype)
        if a.dtype.kind == "f":
            b = np.where(np.isnan(b), a, b)
        assert same(thr.sort_values(b), np.sort(b, axis=None))


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_sort_of_zeros_infinities_denormals_and_nans_of_both_signs(thr, dtype):
    for shape in SHAPES[1:]:
        a = plane("special", dtype, shape)
        got = thr.sort_values(a)
        assert same(got, np.sort(a, axis=None))
        assert got.tobytes() == szr.sort_reference(a).tobytes()
    assert np.isnan(got[-1]) and not np.signbit(got[np.isnan(got)]).any() and np.signbit(a[np.isnan(a)]).any()


@pytest.mark.parametrize("dtype", ["uint32", "float64"])
def test_sort_with_every_pass_forced_equals_the_skipping_sort(thr, hip, dtype):
    a = plane("random", dtype, (257, 263), seed=5)
    low = plane("low_byte", dtype, (257, 263), seed=5)          # all passes but one are skipped by default
    assert hip.get_option("x_sort_skip") == 1
    with_skip = [thr.sort_values(a), thr.sort_values(low)]
    hip.set_option("x_sort_skip", 0)
    try:
        without = [thr.sort_values(a), thr.sort_values(low)]
        assert "skip=0" in hip.last_kernel()
    finally:
        hip.set_option("x_sort_skip", 1)
    for got, forced, src in zip(with_skip, without, (a, low)):
        assert got.tobytes() == forced.tobytes() and same(got, np.sort(src, axis=None))


@pytest.mark.parametrize("dtype", ["float32", "uint16", "int64"])
def test_sort_of_a_tensor_equals_the_sort_of_the_array(thr, dtype):
    import torch
    a = plane("random", dtype, (257, 263), seed=9)
    if dtype == "uint16":
        a = (a >> 1).astype(np.int16)          # (a type torch moves as it is)
    t = torch.from_numpy(a).to("cuda")
    got = thr.sort_values(t)
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.shape == (a.size,)
    assert same(got.cpu().numpy(), np.sort(a, axis=None))
    view = t[:, 5:-3]
    assert same(thr.sort_values(view).cpu().numpy(), np.sort(a[:, 5:-3], axis=None))


# --------------------------------------------------------------------------- zoom

@pytest.mark.parametrize("dtype", DTYPES)
def test_zoom_equals_the_restatement_and_scipy(thr, dtype):
    for n, out_n in szr.LENGTHS:
        a = szr.zoom_case(n, dtype)
        got = thr.zoom_sorted(a, out_n)
        want = szr.zoom_reference(a, out_n)
        assert got.dtype == want.dtype and got.shape == want.shape
        assert np.array_equal(got, want), (n, out_n, np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
        scipy_out = ndi.zoom(a, out_n / n, order=3, mode="nearest")
        if dtype == "float64":
            assert window_ulps(a, got, scipy_out) <= F64_ULPS, (n, out_n)
        else:
            assert np.array_equal(got, scipy_out), (n, out_n)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_zoom_of_rough_unsorted_lines(thr, dtype):
    rng = np.random.default_rng(5)
    for n, out_n in szr.LENGTHS:
        a = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)).astype(dtype)
        got = thr.zoom_sorted(a, out_n)
        assert np.array_equal(got, szr.zoom_reference(a, out_n)), (n, out_n)


def test_zoom_of_a_tensor(thr):
    import torch
    a = szr.zoom_case(1961, "float32")
    got = thr.zoom_sorted(torch.from_numpy(a).to("cuda"), 53)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), ndi.zoom(a, 53 / 1961, order=3, mode="nearest"))


# --------------------------------------------------------------------------- calculate_threshold

def formula_on_scipy(thr, img, bgr, snr):
    profile = ndi.zoom(np.sort(img, axis=None), 1.0 * max(img.shape) / img.size, mode="nearest")
    return thr._threshold_of_profile(profile, bgr, snr)


@pytest.mark.parametrize("i", range(len(G31["thres_value"])))
def test_calculate_threshold_equals_the_references(thr, i):
    img, bgr, snr, want = G31["thres_img%d" % i], str(G31["thres_bgr"][i]), float(G31["thres_snr"][i]), float(G31["thres_value"][i])
    got = thr.calculate_threshold(img, bgr=bgr, snr=snr)
    assert isinstance(got, float)
    assert abs(got - want) <= (1e-9 * abs(want) if want != 0 else 1e-9), (got, want)
    if img.dtype != np.float64:
        assert got == formula_on_scipy(thr, img, bgr, snr)
    import torch
    if img.dtype != np.uint16:
        assert thr.calculate_threshold(torch.from_numpy(img).to("cuda"), bgr=bgr, snr=snr) == got


def test_calculate_threshold_of_views_rows_and_columns(thr):
    rng = np.random.default_rng(21)
    big = (rng.random((70, 90)) * 200).astype(np.float32)
    view = big[3:-2, 6:-11]
    assert thr.calculate_threshold(view) == thr.calculate_threshold(np.ascontiguousarray(view)) == formula_on_scipy(thr, view, "bright", 2.0)
    import torch
    assert thr.calculate_threshold(torch.from_numpy(big).to("cuda")[3:-2, 6:-11]) == thr.calculate_threshold(view)
    row = (rng.random((1, 157)) * 1000).astype(np.uint16)
    assert thr.calculate_threshold(row, bgr="dark") == formula_on_scipy(thr, row, "dark", 2.0)
    assert thr.calculate_threshold(row.T.copy(), bgr="dark") == formula_on_scipy(thr, row.T, "dark", 2.0)


# --------------------------------------------------------------------------- complete

def smoke_dots():
    """The 50-dot image of smoke()."""
    yy, xx = np.mgrid[0:70, 0:150]
    dots = (((yy % 14 - 7) ** 2 + (xx % 14 - 7) ** 2) <= 16).astype(np.uint8)
    return (0.1 + 0.7 * dots + 0.01 * np.random.default_rng(0).random(dots.shape)).astype(np.float32)


def test_get_points_dot_pattern_binarizes_by_default(complete):
    from discorpy_amd.prep import preprocessing
    grey = smoke_dots()
    want = preprocessing.get_points_dot_pattern(preprocessing.binarization(grey), binarize=False)
    got = complete.get_points_dot_pattern(grey)
    assert isinstance(got, np.ndarray) and got.shape == want.shape == (50, 2) and np.array_equal(got, want)
    assert np.array_equal(complete.get_points_dot_pattern(grey, True, 0.3, 0.45),
                          preprocessing.get_points_dot_pattern(preprocessing.binarization(grey, thres=0.45), binarize=False))
    import torch
    assert np.array_equal(complete.get_points_dot_pattern(torch.from_numpy(grey).to("cuda")), want)
    with pytest.raises(NotImplementedError, match="binarize=True"):
        preprocessing.get_points_dot_pattern(grey)          # the module underneath keeps refusing


ROWS, COLS, PITCH, BARREL, SLOPE = 15, 17, 36.0, 2e-6, 0.02


def fisheye_dot_image():
    """A 600 x 700 image of bright dots of radius 4 with an edge two pixels wide (so that Otsu's criterion has its maximum between dots
    and background, not on a plateau that starts at the top of the noise) on a 15 x 17 grid, pulled towards (300, 350) by
    1 / (1 + BARREL r^2) and turned by SLOPE."""
    yy, xx = np.meshgrid((np.arange(ROWS) - ROWS // 2) * PITCH, (np.arange(COLS) - COLS // 2) * PITCH, indexing="ij")
    pull = 1.0 / (1.0 + BARREL * (yy ** 2 + xx ** 2))
    y, x = yy * pull, xx * pull
    a = np.arctan(SLOPE)
    cy, cx = y * np.cos(a) + x * np.sin(a) + 300.0, -y * np.sin(a) + x * np.cos(a) + 350.0
    py, px = np.mgrid[0:600, 0:700]
    img = np.zeros((600, 700), np.float32)
    for y0, x0 in zip(cy.ravel(), cx.ravel()):
        ys, xs = int(y0) - 8, int(x0) - 8
        r = np.sqrt((py[ys:ys + 17, xs:xs + 17] - y0) ** 2 + (px[ys:ys + 17, xs:xs + 17] - x0) ** 2)
        img[ys:ys + 17, xs:xs + 17] = np.clip((4.0 - r) / 2.0 + 0.5, 0.0, 1.0)
    return (0.1 + 0.7 * img + 0.02 * np.random.default_rng(4).random(img.shape)).astype(np.float32)


def test_fisheye_dot_pattern_route_returns_the_whole_grid(complete):
    """The steps of the reference's examples/fisheye_calibration_dot_pattern.py between the image and proc, through complete."""
    prep = complete
    img = fisheye_dot_image()
    height, width = img.shape
    mat1 = prep.binarization(img, ratio=0.3)
    dot_size, dist_dot = prep.calc_size_distance(mat1, ratio=0.3)
    slope_hor = prep.calc_hor_slope(mat1, ratio=0.3)
    slope_ver = prep.calc_ver_slope(mat1, ratio=0.3)
    print("dot size %.2f distance %.3f slopes %.5f %.5f" % (dot_size, dist_dot, slope_hor, slope_ver))
    assert abs(slope_hor - SLOPE) < 0.01 and abs(slope_ver + SLOPE) < 0.01          # (x = -slope y: the grid is turned, not sheared)
    points = prep.get_points_dot_pattern(mat1, binarize=False)
    assert len(points) == ROWS * COLS
    mask = dict(hor_curviness=0.1, ver_curviness=0.1, hor_margin=(20, 20), ver_margin=(20, 20))
    points_hor = prep.remove_points_using_parabola_mask(points, height, width, **mask)
    points_ver = prep.remove_points_using_parabola_mask(np.copy(points), height, width, **mask)
    assert len(points_hor) == ROWS * COLS
    hor = prep.group_dots_hor_lines_based_polyfit(points_hor, slope_hor, dist_dot, ratio=0.1, num_dot_miss=3, accepted_ratio=0.65, order=2)
    ver = prep.group_dots_ver_lines_based_polyfit(points_ver, slope_ver, dist_dot, ratio=0.1, num_dot_miss=3, accepted_ratio=0.65, order=2)
    hor = prep.remove_residual_dots_hor(hor, slope_hor, 2.0)
    ver = prep.remove_residual_dots_ver(ver, slope_ver, 2.0)
    assert [len(line) for line in hor] == [COLS] * ROWS
    assert [len(line) for line in ver] == [ROWS] * COLS
    # the same points from the grey image in one call
    assert np.array_equal(prep.get_points_dot_pattern(img), points)
