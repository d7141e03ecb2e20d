"""GPU suite for the cross-point route of discorpy_amd.prep.linepattern (csrc/profile_kernels.hip: peak_rows_kernel, window_slope_kernel,
the band kernels of dcp_tilted_profiles_2d) against the reference's own results, golden G27 (tools/gen_golden.py), and against the
NumPy restatements of tests/helpers/peaks_reference.py, which tests/test_cross_points_cpu.py holds to NumPy and to that fixture.

* peak search: the integer positions equal the fixture's on every peak table (both float types, 1, 2 and 73 rows per call); the
  sub-pixel positions equal the closed form bit for bit and lie within 4 e_sub of the reference's polyfit (e_sub: the fixture's own
  distance between the two) wherever the triple is not flat
* window slope: bit-equal to the restatement
* tilted profiles: scipy.ndimage.map_coordinates on the reference's band, at what remap_coordinates is held to at order 3 (float32 on
  [0, 1) data within 1e-6; float64 rtol 1e-12, atol 1e-9); xlists / ylists are the reference's expressions bit for bit
* whole functions: the number of points equals the fixture's and no coordinate deviates by more than four times what was measured on
  an MI355X (CROSS_POINTS_MEASURED), at most 1e-6 pixel.  Every test prints its figure before it asserts."""
import functools
import os
import sys

import numpy as np
import pytest
from scipy import ndimage as ndi

from conftest import ROOT, golden

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import peaks_reference as PR  # noqa: E402

pytestmark = pytest.mark.gpu

# largest |coordinate - fixture| over the image cases by the type of the image, measured on an MI355X (test_whole_functions prints it)
CROSS_POINTS_MEASURED = {"float32": 2.02e-12, "float64": 5.68e-13}
CAP = 1e-6                   # pixel: a condition, far below anything a calibration resolves


def bound(dtype):
    return min(4 * CROSS_POINTS_MEASURED[dtype], CAP)


@functools.lru_cache(maxsize=None)
def G():
    g = golden("g27_cross_points")
    for v in g.values():
        v.setflags(write=False)
    return g


NTABLES = int(golden("g27_cross_points")["pk_count"])
CASES = [str(n) for n in golden("g27_cross_points")["case_names"]]


@pytest.fixture(scope="module")
def lp(hip):
    from discorpy_amd.prep import linepattern
    return linepattern


def table(k):
    g = G()
    sens = np.float64(g["pk_sensitive"][k]) if g["pk_promotes"][k] else float(g["pk_sensitive"][k])
    return g["pk%d_row" % k], int(g["pk_radius"][k]), sens


def clipped(radius, row):
    return int(np.clip(radius, 1, len(row) // 4))


def test_peak_tables_integer_positions(lp):
    """One row per call and two (the second is the row reversed, held to the restated search)."""
    g, points = G(), 0
    for k in range(NTABLES):
        row, radius, sens = table(k)
        want = g["pk%d_int" % k]
        one = lp.get_local_extrema_points(row, radius=radius, sensitive=sens, denoise=False, norm=False, subpixel=False)
        assert np.array_equal(one, want), (k, len(row), radius, one, want)
        assert one.dtype == (np.int64 if len(want) else np.float64)
        flipped = np.ascontiguousarray(row[::-1])
        two = lp.get_local_extrema_points(np.stack([row, flipped]), radius=radius, sensitive=sens, denoise=False, norm=False, subpixel=False)
        assert isinstance(two, list) and len(two) == 2 and np.array_equal(two[0], want), (k, two[0], want)
        assert np.array_equal(two[1], PR.local_minima(flipped, clipped(radius, row) if len(row) >= 4 else 0, sens)), k
        points += len(want)
    print("peak tables: %d tables, %d points" % (NTABLES, points))
    assert points > 300


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_peak_search_of_73_rows(lp, dtype):
    """73 rows of 513 samples at radius 11 (samples 11 .. 500: two steps of the row's workgroup) and at 128 (samples 128 .. 383: one
    step): row 0 against the fixture, rows 1, 36 and 72 (the same samples rotated) against the restated search.  Rows of up to five
    steps are in tests/test_peak_steps_gpu.py."""
    g = G()
    for k in range(NTABLES):
        row, radius, sens = table(k)
        if len(row) == 513 and row.dtype == np.dtype(dtype) and radius in (11, 128) and not g["pk_promotes"][k] and len(g["pk%d_int" % k]) > 2:
            rows = np.stack([np.roll(row, 7 * j) for j in range(73)])
            got = lp.get_local_extrema_points(rows, radius=radius, sensitive=sens, denoise=False, norm=False, subpixel=False)
            assert len(got) == 73 and np.array_equal(got[0], g["pk%d_int" % k])
            for j in (1, 36, 72):
                assert np.array_equal(got[j], PR.local_minima(rows[j], radius, sens)), (k, j)


def test_peak_tables_subpixel_positions(lp):
    g = G()
    e_sub, worst, compared = float(g["e_sub"]), 0.0, 0
    for k in range(NTABLES):
        row, radius, sens = table(k)
        ints, subs, curved = g["pk%d_int" % k], g["pk%d_sub" % k], g["pk%d_curved" % k]
        got = lp.get_local_extrema_points(row, radius=radius, sensitive=sens, denoise=False, norm=False, subpixel=True)
        assert got.dtype == np.float64 and len(got) == len(ints), k
        if len(ints) == 0:
            continue
        assert np.array_equal(got, PR.refine(row, ints)), (k, got, PR.refine(row, ints))          # the closed form, bit for bit
        if curved.any():
            worst = max(worst, float(np.abs(got[curved] - subs[curved]).max()))
            compared += int(curved.sum())
    print("sub-pixel positions: %d compared, largest deviation from the reference %.3g (e_sub %.3g)" % (compared, worst, e_sub))
    assert compared > 200 and worst <= 4 * e_sub


def test_rows_through_denoise_and_norm(lp):
    g = G()
    e_sub, radius = float(g["e_sub"]), int(g["dn_radius"])
    rows = [g["dn%d_row" % k] for k in range(int(g["dn_count"]))]
    worst = 0.0
    for k, row in enumerate(rows):
        ints = lp.get_local_extrema_points(row, radius=radius, subpixel=False)
        subs = lp.get_local_extrema_points(row, radius=radius, subpixel=True)
        assert np.array_equal(ints, g["dn%d_int" % k]), (k, ints, g["dn%d_int" % k])
        worst = max(worst, float(np.abs(subs - g["dn%d_sub" % k]).max()))
    both = lp.get_local_extrema_points(np.stack([rows[1], rows[1] + 1.0]), radius=radius, subpixel=False)       # a batch: (N, L), same dtype
    assert np.array_equal(both[0], g["dn1_int"])
    print("denoise + norm rows: largest sub-pixel deviation from the reference %.3g (e_sub %.3g)" % (worst, e_sub))
    assert worst <= 4 * e_sub


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_window_slope_equals_its_restatement(lp, dtype):
    rng = np.random.default_rng(9)
    for n, nrows in ((3, 1), (8, 2), (257, 5), (600, 73)):
        rows = (rng.standard_normal((nrows, n)) * 10.0 ** rng.integers(-3, 4, (nrows, n))).astype(dtype)
        for size in (3, 5, 7, 11):
            used = int(np.clip(size, 3, n))
            used += 1 - used % 2
            got = lp.sliding_window_slope(rows, size=size, norm=False)
            assert got.dtype == rows.dtype and got.shape == rows.shape
            for r in (0, nrows - 1):
                assert np.array_equal(got[r], PR.window_slope(rows[r], used)), (n, nrows, size, r)
            single = lp.sliding_window_slope(rows[0], size=size, norm=True)
            want = PR.window_slope(rows[0], used)
            assert np.array_equal(single, want / np.mean(want) if np.mean(want) != 0.0 else want)
    if dtype != "float64":          # (the fixture's rows are float64: cast to float32 they are other rows)
        return
    g = G()
    e_slope = float(g["e_slope"])
    for k in range(int(g["sl_count"])):
        for size in (3, 5):
            for suffix, norm in (("", False), ("_norm", True)):
                ref = g["sl%d_s%d%s" % (k, size, suffix)]
                got = lp.sliding_window_slope(g["sl%d_row" % k].astype(dtype), size=size, norm=norm)
                dev = float(np.abs(got - ref).max() / np.abs(ref).max())
                tol = (8 if norm else 4) * e_slope        # (normalised: the slopes and their mean each carry 4 e_slope)
                assert dev <= tol, (k, size, norm, dev)


def reference_line(height, width, index, angle_deg, direction):
    """xlist, ylist and the band of the reference's get_tilted_profile, in its own expressions."""
    angle = angle_deg * np.pi / 180.0
    if direction == "horizontal":
        rlist = np.linspace(0, np.floor(width / np.cos(angle)), width)
        xlist = rlist * np.cos(angle)
        ylist = rlist * np.sin(-angle)
        xlist = np.clip(xlist, 0, width - 1)
        ylist = np.clip(index + ylist, 0, height - 1)
        lo, hi = int(np.floor(np.amin(ylist))), int(np.ceil(np.amax(ylist))) + 1
        return xlist, ylist, (slice(lo, hi), slice(None)), (ylist - lo, xlist)
    rlist = np.linspace(0, np.floor(height / np.cos(angle)), height)
    ylist = rlist * np.cos(angle)
    xlist = rlist * np.sin(angle)
    xlist = np.clip(index + xlist, 0, width - 1)
    ylist = np.clip(ylist, 0, height - 1)
    lo, hi = int(np.floor(np.amin(xlist))), int(np.ceil(np.amax(xlist))) + 1
    return xlist, ylist, (slice(None), slice(lo, hi)), (ylist, xlist - lo)


@functools.lru_cache(maxsize=None)
def profile_image(name, dtype):
    if name == "random":
        return np.random.default_rng(17).random((96, 120)).astype(dtype)
    tall = G()["img_tall"].astype(np.float64)                      # 300 x 96: a prefiltered line of 324 samples
    return (tall / (tall.max() * 1.001)).astype(dtype)             # on [0, 1)


PROFILE_CASES = [(name, dtype, direction, angle) for name in ("random", "tall") for dtype in ("float32", "float64")
                 for direction in ("horizontal", "vertical") for angle in (3.0, -3.0, 0.0)]


@pytest.mark.parametrize("name,dtype,direction,angle", PROFILE_CASES, ids=["%s-%s-%s%+g" % c for c in PROFILE_CASES])
def test_tilted_profiles(lp, name, dtype, direction, angle):
    """First and last admissible index and one in between, in one call; a band of one row / column at angle 0."""
    mat = profile_image(name, dtype)
    height, width = mat.shape
    first, last = lp._calc_index_range(height, width, angle, direction)
    indices = [first, (first + last) // 2 + 0.25, last]
    xlists, ylists, profiles = lp.get_tilted_profiles(mat, indices, angle, direction)
    assert profiles.dtype == mat.dtype and profiles.shape == xlists.shape == ylists.shape == (3, width if direction == "horizontal" else height)
    worst = 0.0
    for p, index in enumerate(indices):
        xlist, ylist, band, coords = reference_line(height, width, index, angle, direction)
        assert np.array_equal(xlists[p], xlist) and np.array_equal(ylists[p], ylist)
        ref = ndi.map_coordinates(mat[band], coords, order=3, mode="nearest")
        worst = max(worst, float(np.abs(profiles[p].astype(np.float64) - ref).max()))
        if dtype == "float32":
            assert np.abs(profiles[p] - ref).max() <= 1e-6, (p, worst)
        else:
            assert np.allclose(profiles[p], ref, rtol=1e-12, atol=1e-9), (p, worst)
    print("tilted profiles %s %s %s %+g: largest deviation from scipy %.3g" % (name, dtype, direction, angle, worst))


def test_tilted_profiles_in_two_groups(lp):
    """300 profiles: more than the 256 whose band table travels in one copy, so the call runs two groups; every profile equals the one
    a call of its own gives, bit for bit, for NumPy and for tensor input."""
    torch = pytest.importorskip("torch")
    mat = profile_image("random", "float64")
    first, last = lp._calc_index_range(96, 120, 3.0, "horizontal")
    indices = np.linspace(first, last, 300)
    xlists, ylists, profiles = lp.get_tilted_profiles(mat, indices, 3.0, "horizontal")
    assert profiles.shape == (300, 120)
    for p in (0, 1, 255, 256, 257, 299):
        one = lp.get_tilted_profiles(mat, [indices[p]], 3.0, "horizontal")
        assert np.array_equal(one[2][0], profiles[p]) and np.array_equal(one[0][0], xlists[p]) and np.array_equal(one[1][0], ylists[p]), p
    dev = lp.get_tilted_profiles(torch.from_numpy(mat).to("cuda:0"), indices, 3.0, "horizontal")[2]
    assert isinstance(dev, torch.Tensor) and np.array_equal(dev.cpu().numpy(), profiles)


def image_case(name):
    g = G()
    flag, dtype, fn = name.split("_")
    mat = g["img_chess" if flag == "chess" else "img_line"].astype(dtype)
    if flag == "dark":
        mat = mat.max() - mat
    kw = dict(default={}, nonorm=dict(norm=False), nodenoise=dict(denoise=False), dark=dict(bgr="dark"), offset=dict(offset=9),
              chess=dict(chessboard=True))[flag]
    return mat, dtype, fn, float(g["slope"]), 24.0 if flag == "chess" else 20.0, kw, g["pts_" + name]


@pytest.mark.parametrize("name", CASES)
def test_whole_functions(lp, name):
    mat, dtype, fn, slope, dist, kw, ref = image_case(name)
    call = lp.get_cross_points_hor_lines if fn == "hor" else lp.get_cross_points_ver_lines
    got = call(mat, slope, dist, **kw)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64
    assert got.shape == ref.shape and len(ref) >= 50, (got.shape, ref.shape)
    dev = float(np.abs(got - ref).max())
    print("cross points %s: %d points, largest coordinate deviation from the reference %.3g pixel" % (name, len(ref), dev))
    assert dev <= bound(dtype)


@pytest.mark.parametrize("name", [n for n in CASES if n.split("_")[0] in ("default", "nonorm", "chess")])
def test_tensor_input_gives_the_same_points(lp, name):
    torch = pytest.importorskip("torch")
    mat, dtype, fn, slope, dist, kw, ref = image_case(name)
    call = lp.get_cross_points_hor_lines if fn == "hor" else lp.get_cross_points_ver_lines
    host = call(mat, slope, dist, **kw)
    got = call(torch.from_numpy(mat).to("cuda:0"), slope, dist, **kw)
    assert isinstance(got, np.ndarray) and got.shape == host.shape == ref.shape
    dev, dev_ref = float(np.abs(got - host).max()), float(np.abs(got - ref).max())
    print("cross points %s, tensor input: largest coordinate deviation from NumPy input %.3g pixel, from the reference %.3g" % (name, dev, dev_ref))
    assert dev <= bound(dtype) and dev_ref <= bound(dtype)


def test_bounds_checking_build_counts_no_tap_outside_its_slab():
    """libdiscorpy_hip_bounds.so (sites 40 - 42 of peak_rows_kernel: every window against the staged samples, every sorted-tail write
    against the wave's slab) in a process of its own: the peak tables of 513 samples at radii 1, 11 and 128, both types, give the
    fixture's positions and count nothing."""
    import subprocess
    lib = os.path.join(ROOT, "discorpy_amd", "lib", "libdiscorpy_hip_bounds.so")
    assert os.path.exists(lib), "build() makes the bounds-checking library; it is missing"
    code = """
import sys, numpy as np
sys.path.insert(0, %r)
from discorpy_amd import _ffi as F
from discorpy_amd.prep import linepattern as lp
F.require_device()
assert F.debug_bounds()[4] == 1
g = np.load(%r)
done = 0
for k in range(int(g["pk_count"])):
    row, radius = g["pk%%d_row" %% k], int(g["pk_radius"][k])
    if len(row) == 513 and radius in (1, 11, 128) and not g["pk_promotes"][k]:
        got = lp.get_local_extrema_points(row, radius=radius, sensitive=float(g["pk_sensitive"][k]), denoise=False, norm=False, subpixel=True)
        assert len(got) == len(g["pk%%d_int" %% k]), k
        done += 1
b = F.debug_bounds()
assert b[0] == 0 and b[4] == 1, b
print("bounds ok", done, b)
""" % (ROOT, os.path.join(ROOT, "tests", "golden", "g27_cross_points.npz"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT, env=dict(os.environ, DCP_LIB_PATH=lib))
    assert r.returncode == 0 and "bounds ok 12" in r.stdout, (r.stdout + r.stderr)[-3000:]
