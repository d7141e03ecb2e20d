"""GPU suite for the rest of the dot-pattern route (discorpy_amd.prep.dotpattern; csrc/dotgrid_kernels.hip through dcp_radon_padded_2d,
dcp_nearest_sq_dists and dcp_box_moments_2d).  Everything is compared exactly:

* radon_padded against the NumPy restatement tests/helpers/radon_padded_reference.py (held to facts checked by hand in
  tests/test_dot_grid_cpu.py), bit for bit: rectangles 1 x 1 .. 65 x 63 and 40 x 97 (padded sides on both sides of a wave's 64 columns,
  both parities), the axis angles, 45, -30 and a 0.05 degree ladder, float32 and float64, arrays and tensors, a strided ROI in a sea of
  NaN, NaN and infinities inside, the four corners the circle would have dropped, two calls;
* dcp_nearest_sq_dists against ``np.sort(d2, axis=1)[:, :4]`` of NumPy's own d2, bit for bit: N on both sides of the wave (64) and of
  the LDS tile (256), several tiles (1025, 5000), coincident points, an integer lattice (all ties), coordinates near 1e4;
* dcp_box_moments_2d against NumPy's int64 sums: boxes 1 x 1 .. 70 x 70 and widths around the wave, overlapping boxes, boxes on the
  plane's edges, empty boxes, a strided view, every measured element type, one box and 300;
* every case of golden G29 (tools/gen_golden.py: what the reference's own functions returned): calc_size_distance, both slopes and the
  masks of select_dots_based_ratio / _size / _distance ``==`` the recording, from arrays and from tensors, and the image paths of the
  grouping functions; select_dots_based_distance also against its NumPy loop of before the rerouting."""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, golden

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import radon_padded_reference as RP  # noqa: E402

pytestmark = pytest.mark.gpu

LADDER = np.arange(-1.0, 1.05, 0.05)
ANGLES = np.concatenate([[0.0, 90.0, 180.0, 45.0, -30.0], LADDER, 90.0 + LADDER[::4]])
SHAPES = [(1, 1), (1, 2), (2, 1), (3, 5), (5, 3), (63, 65), (64, 64), (65, 63), (40, 97)]


@pytest.fixture(scope="module")
def prep(hip):
    from discorpy_amd.prep import preprocessing
    return preprocessing


@pytest.fixture(scope="module")
def dp(hip):
    from discorpy_amd.prep import dotpattern
    return dotpattern


@pytest.fixture(scope="module")
def g29():
    return golden("g29_dot_grid")


def plane(shape, dtype, seed=0):
    rng = np.random.default_rng(1000 * shape[0] + shape[1] + seed)
    return ((rng.random(shape) - 0.3) * 10.0 ** rng.integers(-3, 4, shape)).astype(dtype)


@functools.lru_cache(maxsize=None)
def oracle(shape, dtype, seed=0):
    """(the plane, its padded sinogram at ANGLES): computed once, shared, read-only."""
    img = plane(shape, dtype, seed)
    want = RP.radon(img, ANGLES)
    img.setflags(write=False)
    want.setflags(write=False)
    return img, want


def same_bits(got, want):
    return got.shape == want.shape and got.dtype == want.dtype == np.float64 and np.array_equal(got.view(np.uint64), want.view(np.uint64))


# --------------------------------------------------------------------------- radon_padded

@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_radon_padded_rectangles_every_angle(prep, shape, dtype):
    img, want = oracle(shape, dtype)
    got = prep.radon_padded(img, ANGLES)
    assert isinstance(got, np.ndarray) and got.shape == (RP.padded_side(*shape), len(ANGLES)) and same_bits(got, want)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape", [(3, 5), (65, 63), (40, 97)], ids=["3x5", "65x63", "40x97"])
def test_radon_padded_from_a_tensor(prep, shape, dtype):
    import torch
    img, want = oracle(shape, dtype)
    got = prep.radon_padded(torch.from_numpy(np.array(img)).to("cuda:0"), ANGLES)
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.float64 and same_bits(got.cpu().numpy(), want)


@pytest.mark.parametrize("kind", ["numpy", "torch"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_radon_padded_reads_a_strided_roi_in_place_and_nothing_around_it(prep, dtype, kind):
    img, want = oracle((40, 97), dtype)
    sea = np.full((52, 120), np.nan, dtype)
    sea[5:45, 11:108] = img
    if kind == "torch":
        import torch
        view = torch.from_numpy(sea).to("cuda:0")[5:45, 11:108]
        assert not view.is_contiguous()
        got = prep.radon_padded(view, ANGLES).cpu().numpy()
    else:
        view = sea[5:45, 11:108]
        assert not view.flags.c_contiguous
        got = prep.radon_padded(view, ANGLES)
    assert same_bits(got, want) and np.isfinite(got).all()


def test_radon_padded_nan_and_inf_inside_reach_the_result(prep):
    img = np.array(oracle((63, 65), "float32")[0])
    img[0, 0], img[31, 40], img[62, 64] = np.nan, np.inf, -np.inf          # a corner included: inside the rectangle everything counts
    theta = [0.0, 45.0, 90.0, -30.0]
    got, want = prep.radon_padded(img, theta), RP.radon(img, theta)
    assert same_bits(got, want)
    assert np.isnan(got).any() and np.isinf(got).any() and np.isfinite(got).any()


def test_radon_padded_keeps_the_corners_the_circle_drops(prep):
    img = np.zeros((64, 64), np.float32)
    img[0, 0] = img[0, -1] = img[-1, 0] = img[-1, -1] = 1.0
    got = prep.radon_padded(img, [45.0, 0.0])
    assert same_bits(got, RP.radon(img, [45.0, 0.0])) and got[:, 0].sum() > 3.0 and got[:, 1].sum() == 4.0
    from discorpy_amd.prep import linepattern as lp
    assert lp.radon(img, [45.0]).sum() == 0.0


def test_radon_padded_default_theta_and_two_calls(prep):
    img = np.array(oracle((5, 3), "float64")[0])
    got = prep.radon_padded(img)
    assert got.shape == (8, 180) and same_bits(got, RP.radon(img, np.arange(180)))
    big, _ = oracle((65, 63), "float32")
    assert same_bits(prep.radon_padded(big, ANGLES), prep.radon_padded(big, ANGLES))


# --------------------------------------------------------------------------- nearest squared distances

def points_of(kind, n):
    rng = np.random.default_rng(n)
    if kind == "random":
        return rng.random((n, 2)) * 500.0
    if kind == "far":                                      # coordinates near 1e4 with fractions: the differences round
        return 1e4 + rng.random((n, 2)) * 300.0 + rng.integers(0, 3, (n, 2)) / 3.0
    if kind == "lattice":                                  # an exact integer lattice: every distance is a tie of four or eight
        side = int(np.ceil(np.sqrt(n)))
        y, x = np.divmod(rng.permutation(side * side)[:n], side)
        return np.stack([y, x], axis=1).astype(np.float64) * 7.0
    pts = rng.random((n, 2)) * 50.0                        # coincident: every point three times at least
    return pts[rng.integers(0, max(n // 3, 1), n)]


def nearest_want(pts):
    y, x = pts[:, 0], pts[:, 1]
    d2 = (y[:, None] - y[None, :]) * (y[:, None] - y[None, :]) + (x[:, None] - x[None, :]) * (x[:, None] - x[None, :])
    want = np.full((len(pts), 4), np.inf)
    k = min(4, len(pts))
    want[:, :k] = np.sort(d2, axis=1)[:, :k]
    return want


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 63, 64, 65, 257, 1025, 5000])
def test_nearest_sq_dists_are_numpys(dp, n):
    pts = points_of("random", n)
    got = dp._nearest_sq(pts)
    assert same_bits(got, nearest_want(pts))
    assert (got[:, 0] == 0.0).all() and np.array_equal(np.sort(got, axis=1), got)
    # the reference's own expression, row by row, for a few points
    for i in (0, n // 2, n - 1):
        ref = np.sort(np.sqrt((pts[i][0] - pts[:, 0]) ** 2 + (pts[i][1] - pts[:, 1]) ** 2))[:4]
        assert np.array_equal(np.sqrt(got[i])[:len(ref)], ref)


@pytest.mark.parametrize("n", [5, 64, 257, 1025])
@pytest.mark.parametrize("kind", ["coincident", "lattice", "far"])
def test_nearest_sq_dists_ties_and_large_coordinates(dp, kind, n):
    pts = points_of(kind, n)
    got = dp._nearest_sq(pts)
    assert same_bits(got, nearest_want(pts))
    if kind == "coincident" and n >= 64:
        assert (got[:, 1] == 0.0).any()
    assert same_bits(dp._nearest_sq(pts), got)             # two calls


# --------------------------------------------------------------------------- box moments

MEASURED = ["bool", "uint8", "int8", "uint16", "int16"]


def moments_want(mask, boxes):
    out = np.zeros((len(boxes), 6), np.int64)
    for k, (y0, y1, x0, x1) in enumerate(boxes):
        if y1 < y0 or x1 < x0:
            continue
        ys, xs = np.nonzero(mask[y0:y1 + 1, x0:x1 + 1])
        ys, xs = ys.astype(np.int64), xs.astype(np.int64)
        out[k] = [len(ys), ys.sum(), xs.sum(), (ys * ys).sum(), (xs * ys).sum(), (xs * xs).sum()]
    return out


def mask_of(shape, dtype, seed=0):
    rng = np.random.default_rng(seed)
    on = rng.random(shape) < 0.45
    if dtype == "bool":
        return on
    info = np.iinfo(dtype)
    values = rng.integers(info.min, int(info.max) + 1, shape)           # any nonzero value is set, a negative one and 256 included
    values[values == 0] = 1
    if info.bits == 16:
        values[::3, ::2] = 256                                            # low byte zero: still set
    return np.where(on, values, 0).astype(dtype)


BOXES = np.array([[0, 0, 0, 0], [5, 5, 3, 150], [7, 149, 9, 9], [10, 11, 20, 21], [0, 99, 0, 62], [30, 60, 40, 103], [30, 61, 39, 103],
                  [20, 89, 100, 169], [50, 119, 90, 159], [0, 149, 0, 179], [149, 149, 179, 179], [0, 0, 170, 179], [140, 149, 0, 5],
                  [150, -1, 180, -1], [9, 8, 3, 50], [3, 50, 9, 8]], np.int32)


@pytest.mark.parametrize("kind", ["numpy", "torch"])
@pytest.mark.parametrize("dtype", MEASURED)
def test_box_moments_are_numpys_sums(dp, dtype, kind):
    mask = mask_of((150, 180), dtype, seed=1)
    want = moments_want(mask, BOXES)
    if kind == "torch":
        import torch
        # (a tensor of the same bits as int16 where torch has no 16-bit unsigned type to move: an element is set by its bits)
        got = dp._box_moments(torch.from_numpy(mask.view(np.int16) if dtype == "uint16" else mask).to("cuda:0"), BOXES)
    else:
        got = dp._box_moments(mask, BOXES)
    assert isinstance(got, np.ndarray) and got.dtype == np.int64 and np.array_equal(got, want)
    assert want[4, 0] > 2000 and (want[-3:] == 0).all()


@pytest.mark.parametrize("kind", ["numpy", "torch"])
def test_box_moments_of_a_strided_view_one_box_and_300(dp, kind):
    base = mask_of((120, 400), "uint8", seed=2)
    view = base[7:107, 13:350]
    rng = np.random.default_rng(5)
    y0, x0 = rng.integers(0, 90, 300), rng.integers(0, 300, 300)
    boxes = np.stack([y0, y0 + rng.integers(0, 10, 300), x0, x0 + rng.integers(0, 37, 300)], axis=1).astype(np.int32)
    arg = view
    if kind == "torch":
        import torch
        arg = torch.from_numpy(base).to("cuda:0")[7:107, 13:350]
        assert not arg.is_contiguous()
    assert np.array_equal(dp._box_moments(arg, boxes), moments_want(view, boxes))
    assert np.array_equal(dp._box_moments(arg, boxes[17:18]), moments_want(view, boxes[17:18]))
    full = np.ones((70, 70), np.uint8)                          # a full 70 x 70 box: the closed forms
    got = dp._box_moments(full, [[0, 69, 0, 69]])[0]
    assert got.tolist() == [4900, 70 * 2415, 70 * 2415, 70 * 111895, 2415 * 2415, 70 * 111895]


# --------------------------------------------------------------------------- golden G29

CASES = ["a_90", "a_60", "b_90", "b_60"]


def as_kind(img, kind):
    if kind == "numpy":
        return img
    import torch
    return torch.from_numpy(img).to("cuda:0")


@pytest.mark.parametrize("kind", ["numpy", "torch"])
@pytest.mark.parametrize("name", CASES)
def test_g29_size_distance_and_slopes_are_the_references(prep, g29, name, kind):
    mat = as_kind(np.int16(g29["img_" + name[0]]), kind)
    roi = float(g29["roi_" + name])
    size, dist = prep.calc_size_distance(mat, roi)
    slope_hor, slope_ver = prep.calc_hor_slope(mat, roi), prep.calc_ver_slope(mat, roi)
    print("%s: size %r dist %r slopes %r %r" % (name, size, dist, slope_hor, slope_ver))
    assert g29["gap_hor_" + name] > 1e-9 and g29["gap_ver_" + name] > 1e-9
    assert size == g29["size_" + name] and dist == g29["dist_" + name]
    assert slope_hor == g29["slope_hor_" + name] and slope_ver == g29["slope_ver_" + name]


@pytest.mark.parametrize("kind", ["numpy", "torch"])
@pytest.mark.parametrize("key", ["a", "b"])
def test_g29_ratio_mask_is_the_references(prep, g29, key, kind):
    assert g29["margin_" + key] > 1e-6
    img = g29["img_" + key]
    for mat in (as_kind(np.int16(img), kind), as_kind(img, kind), as_kind(img.astype(np.float32), kind)):
        got = prep.select_dots_based_ratio(mat, float(g29["select_ratio"]))
        assert isinstance(got, np.ndarray) and got.dtype == np.int16 and np.array_equal(got, g29["kept_ratio_" + key])
    strict = prep.select_dots_based_ratio(img, 0.02) != 0          # a stricter ratio keeps fewer dots, all of them among the kept
    assert 0 < strict.sum() < (g29["kept_ratio_" + key] != 0).sum() and not (strict & (g29["kept_ratio_" + key] == 0)).any()


def distance_mask_before_rerouting(prep, mat, dot_dist, ratio=0.3):
    """select_dots_based_distance as it was before its distances came from dcp_nearest_sq_dists: the NumPy loop, restated."""
    mat = np.int16(mat)
    labels, num = prep.label(mat)
    sums, boxes = prep._measures(mat, labels, num, top=num)
    cents = np.asarray(prep._centroids(sums, np.arange(1, num + 1)))
    kept = np.zeros_like(mat)
    for i, box in enumerate(prep._slices(boxes, num)):
        dist = np.sort(np.sqrt((cents[i][0] - cents[:, 0]) ** 2 + (cents[i][1] - cents[:, 1]) ** 2))[1:4]
        if any((dist - (dist // dot_dist) * dot_dist) / dot_dist < ratio):
            kept[box] = mat[box]
    return kept


@pytest.mark.parametrize("kind", ["numpy", "torch"])
@pytest.mark.parametrize("name", CASES)
def test_g29_size_and_distance_masks_and_the_flow(prep, g29, name, kind):
    img = np.int16(g29["img_" + name[0]])
    size, dist = g29["size_" + name], g29["dist_" + name]
    kept_size = prep.select_dots_based_size(as_kind(img, kind), size)
    assert np.array_equal(kept_size, g29["kept_size_" + name])
    kept_dist = prep.select_dots_based_distance(as_kind(img, kind), dist)
    assert kept_dist.dtype == np.int16 and np.array_equal(kept_dist, g29["kept_dist_" + name])
    if kind == "numpy":
        assert np.array_equal(distance_mask_before_rerouting(prep, img, dist), kept_dist)
        tiny = img[:30, :50]                                          # two or three dots: rows of fewer than three neighbours
        for sub in (tiny, img[:25, :25]):
            if sub.max() == 1:
                assert np.array_equal(prep.select_dots_based_distance(sub, dist), distance_mask_before_rerouting(prep, sub, dist))
    # the flow of the reference's example_01 from the binary image on, images handed to the grouping functions
    mat1 = prep.select_dots_based_ratio(kept_size, float(g29["select_ratio"]))
    assert np.array_equal(mat1, g29["flow_" + name])
    slope_hor, slope_ver = g29["slope_hor_" + name], g29["slope_ver_" + name]
    hor = prep.group_dots_hor_lines(as_kind(mat1, kind), slope_hor, dist)
    ver = prep.group_dots_ver_lines(as_kind(mat1, kind), slope_ver, dist)
    hor2, ver2 = prep.remove_residual_dots_hor(hor, slope_hor), prep.remove_residual_dots_ver(ver, slope_ver)
    for got, key in ((hor, "hor_"), (ver, "ver_"), (hor2, "hor2_"), (ver2, "ver2_")):
        want = np.split(g29[key + name + "_pts"], np.cumsum(g29[key + name + "_len"])[:-1])
        assert len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want)), key
