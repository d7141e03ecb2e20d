"""GPU suite for the Fourier Gaussian filter's run logic and tap indexing (dcp_fourier_gauss_2d, csrc/fourier_kernels.hip), with tables
in which every tap counts.

With the Gaussian tables of prep._fourier_taps the taps at the ends of a run are below 2^-56 of the table: a window one or three
indices too short, a leftover loop that stops early or a reversed tap index passes tests/test_fourier_gauss_gpu.py at any tolerance.
Here the C ABI is driven with tables of small integers (tests/helpers/fourier_cases.py): kept taps are nonzero integers in [-8, 8],
dropped taps exact zeros, so the library derives exactly the radius the table was built with, and with integer images every product
and partial sum is an integer below 2^53 -- the float64 multiply-add chains are exact in any order and every comparison is
np.array_equal against an integer Toeplitz product (dense_exact).  Every test also checks the number of taps kept that the launcher
reports, 4 R + 1 (2 N - 1 once 2 R + 1 >= N).  tests/test_fourier_gauss_cpu.py asserts, without a GPU, that each case takes the
branches of fourier_runs, the leftovers and the workgroup columns its table claims.

The last tests run Gaussian tables at the geometry of the default call (R > pad, below / one / above on both axes, under two thirds of
the taps kept) against the reference restated on scipy.fftpack, at the tolerance of tests/test_fourier_gauss_gpu.py times the
case's OWN e_ref (helpers.truth), and print the ratio before they assert."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import fourier_cases as FC  # noqa: E402
from test_fourier_gauss_gpu import BCK_FACTOR, NORM_FACTOR, kept_taps, ratio, reference_filter  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = {"reflect": 5, "symmetric": 0, "edge": 4, "wrap": 7, "constant": 2}      # np.pad's mode -> DCP_MODE_*
TYPES = ("float32", "float64", "uint8", "int8", "uint16", "int16", "uint32", "int32", "int64", "uint64", "bool")


def filter_plane(hip, src, pad, mode, ty, tx, device=False):
    """dcp_fourier_gauss_2d on a 2-D array whose rows may be strided, from host memory or (device=True) from device memory on a
    stream of its own; returns (plane, ((kept, all) of axis 0, (kept, all) of axis 1))."""
    h, w = src.shape
    assert src.strides[1] == src.itemsize and src.strides[0] % src.itemsize == 0
    stride = src.strides[0] // src.itemsize
    dp = hip.C.POINTER(hip.C.c_double)
    tables = [np.ascontiguousarray(t, dtype=np.float64) for t in ty + tx]
    assert [t.size for t in tables] == [2 * (h + 2 * pad) - 1] * 2 + [2 * (w + 2 * pad) - 1] * 2
    taps = [t.ctypes.data_as(dp) for t in tables]
    code = hip.DTYPE_BY_NAME[src.dtype.name]
    out = np.full((h, w), np.nan)
    if device:
        span = (h - 1) * stride + w                     # the elements from the view's first to its last
        flat = np.lib.stride_tricks.as_strided(src, (span,), (src.itemsize,), writeable=False)
        d_src = hip.DeviceBuffer(span * src.itemsize).upload(flat)
        d_dst = hip.DeviceBuffer(out.nbytes).upload(out)
        stream = hip.Stream()
        hip.check(hip.lib().dcp_fourier_gauss_2d(d_src.ptr, d_dst.ptr, h, w, stride, code, pad, MODES[mode], *taps, hip.MEM_DEVICE, -1, stream.ptr))
        stream.synchronize()
        out = d_dst.download((h, w), np.float64)
    else:
        hip.check(hip.lib().dcp_fourier_gauss_2d(src.ctypes.data, out.ctypes.data, h, w, stride, code, pad, MODES[mode], *taps, hip.MEM_HOST, -1, None))
    return out, kept_taps(hip)


def expect_kept(kept, ny, ry, nx, rx):
    assert kept == ((FC.taps_kept(ny, ry), 2 * ny - 1), (FC.taps_kept(nx, rx), 2 * nx - 1)), (kept, ny, ry, nx, rx)


# --------------------------------------------------------------------------- identity: the conversion of every element type

def extremes(dtype):
    dt = np.dtype(dtype)
    if dt == np.bool_:
        return [True, False]
    if dt == np.float32:
        return [np.finfo(np.float32).max, np.float32(1e-45), -np.finfo(np.float32).max, np.float32(-3.25), np.finfo(np.float32).tiny]
    if dt == np.float64:
        return [0.1, 1.0 + 2.0 ** -52, 1e300, -1e-300, 5e-324, -(2.0 ** 53 + 2.0), 16777217.0]
    info = np.iinfo(dt)
    out = [info.max, info.min, info.max - 1]
    if dt == np.uint64:
        out += [2 ** 53 + 1, 2 ** 63, 2 ** 63 + 1025]
    if dt == np.int64:
        out += [-(2 ** 53 + 1), 2 ** 53 + 1, -(2 ** 63 - 1023)]
    if dt.itemsize == 4:
        out += [2 ** 24 + 1, 2 ** 31 - 1]
    return out


def identity_source(dtype, shape, seed):
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype)
    if dt == np.bool_:
        src = rng.random(shape) < 0.5
    elif dt.kind == "f":
        src = rng.uniform(-1000.0, 1000.0, shape).astype(dt)
    else:
        info = np.iinfo(dt)
        src = rng.integers(info.min, info.max, size=shape, endpoint=True, dtype=dt)
    h, w = shape
    spots = [(0, 0), (h - 1, w - 1), (0, w - 1), (h - 1, 0), (h // 2, 255), (h // 2, 256), (7, 3), (8, 252), (h - 1, 253), (3, 254)]
    for k, v in enumerate(extremes(dtype)):
        src[spots[k]] = v
        assert src[spots[k]] == dt.type(v)
    return src


@pytest.mark.parametrize("dtype", TYPES)
def test_identity_tables_convert_every_element_as_numpy_does(hip, dtype):
    """a(0) = 1 on both axes (R = 0, one tap of 2 N - 1): dst is src.astype(float64) bit for bit, at a type's limits, above 2^53,
    below 0, for denormal and largest finite floats.  19 x 261 padded by 3 has a second workgroup column in pass 1."""
    shape, pad = (19, 261), 3
    src = identity_source(dtype, shape, 77)
    ty, tx = FC.delta_table(shape[0] + 2 * pad, 0), FC.delta_table(shape[1] + 2 * pad, 0)
    got, kept = filter_plane(hip, src, pad, "reflect", ty, tx)
    expect_kept(kept, shape[0] + 2 * pad, 0, shape[1] + 2 * pad, 0)
    want = src.astype(np.float64)
    assert kept[0][0] == kept[1][0] == 1
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]


@pytest.mark.parametrize("dtype", ["int64", "float32", "uint16", "bool"])
def test_identity_tables_on_a_row_strided_view(hip, dtype):
    shape, pad = (19, 261), 3
    base = np.zeros((19, 271), dtype)
    base[:] = identity_source(dtype, (19, 271), 78)
    view = base[:, 3:-7]
    view[:] = identity_source(dtype, shape, 79)
    assert not view.flags.c_contiguous and view.shape == shape
    ty, tx = FC.delta_table(shape[0] + 2 * pad, 0), FC.delta_table(shape[1] + 2 * pad, 0)
    for mode in ("symmetric", "constant"):
        got, kept = filter_plane(hip, view, pad, mode, ty, tx)
        expect_kept(kept, shape[0] + 2 * pad, 0, shape[1] + 2 * pad, 0)
        assert np.array_equal(got, view.astype(np.float64)), mode


# --------------------------------------------------------------------------- one shifted tap per axis

def shifted(src, pad, mode, dy, dx):
    """m[j + pad - dy, i + pad - dx] of the padded plane m where that lies inside it, 0 elsewhere, for the cropped (j, i)."""
    m = np.pad(src, pad, mode=mode).astype(np.float64)
    jj = np.arange(src.shape[0]) + pad - dy
    ii = np.arange(src.shape[1]) + pad - dx
    inside = ((jj >= 0) & (jj < m.shape[0]))[:, None] & ((ii >= 0) & (ii < m.shape[1]))[None, :]
    return np.where(inside, m[np.clip(jj, 0, m.shape[0] - 1)][:, np.clip(ii, 0, m.shape[1] - 1)], 0.0)


def tap_offsets(n, r):
    return [r, -r, n - r, -(n - r), n - 1, -(n - 1), 1, -1]


def radius_of(n, d):
    return min(abs(d), n - abs(d))


SHIFT_SHAPES = [((8, 5), 23, 5, mode) for mode in MODES] + [((41, 37), 2, 5, "reflect"), ((41, 37), 2, 12, "wrap")]


@pytest.mark.parametrize("shape,pad,r,mode", SHIFT_SHAPES, ids=["%dx%d_p%d_r%d_%s" % (c[0] + c[1:]) for c in SHIFT_SHAPES])
def test_one_shifted_tap_per_axis_moves_the_padded_plane(hip, shape, pad, r, mode):
    """a_y(dy) = 1, a_x(dx) = 1 and nothing else, dy and dx each from {R, -R, N - R, -(N - R), N - 1, -(N - 1), 1, -1}: the result is
    the padded plane moved by (dy, dx), zero where that leaves the plane.  This pins the direction of the tap index per axis, every
    fold of a pad several sides deep, and both ends of each run.  With i in front of both taps the result is the negated shift, with
    i in front of one of them exact zeros: the pairing and the sign of the two planes in pass 2."""
    ny, nx = shape[0] + 2 * pad, shape[1] + 2 * pad
    src = FC.integer_image(shape, "uint16", 300 + pad)
    ys, xs = tap_offsets(ny, r), tap_offsets(nx, r)
    seen = 0
    for k in range(8):
        for turn in (0, 3):
            dy, dx = ys[k], xs[(k + turn) % 8]
            want = shifted(src, pad, mode, dy, dx)
            got, kept = filter_plane(hip, src, pad, mode, FC.delta_table(ny, dy), FC.delta_table(nx, dx))
            expect_kept(kept, ny, radius_of(ny, dy), nx, radius_of(nx, dx))
            assert np.array_equal(got, want), (dy, dx, np.argwhere(got != want)[:4])
            seen += bool(want.any())
            if turn == 0:
                both, _ = filter_plane(hip, src, pad, mode, FC.delta_table(ny, dy, True), FC.delta_table(nx, dx, True))
                assert np.array_equal(both, -want), ("i i", dy, dx)
                for iy, ix in ((True, False), (False, True)):
                    one, _ = filter_plane(hip, src, pad, mode, FC.delta_table(ny, dy, iy), FC.delta_table(nx, dx, ix))
                    assert not one.any(), ("i on one axis", iy, ix, dy, dx)
    # (8 x 5 padded by 23: only the shifts by 1 and by R stay on the plane, and under `constant` a shift by R = 5 columns shows zeros)
    assert seen >= (8 if shape == (41, 37) else 2 if mode == "constant" else 4), "too few shifts landed on the plane to compare anything"


# --------------------------------------------------------------------------- random integer tables

@pytest.mark.parametrize("case", [c for c in FC.CASES if not c.wide], ids=repr)
def test_integer_tables_equal_the_integer_product(hip, case):
    """The radii 0, 1, 7, 8, 9 (leftovers 0, 2 and 6 of a one-run window; below, one and above on both axes from R = 7), the turn to
    the whole axis for both parities of N, tables with only the near, only the wrapped, only the negative or only the positive taps,
    pad 0 and a pad under 7 with ragged sides (the last block reads the zeros behind the table), the constant mode."""
    src, ty, tx, want = FC.case_data(case.name)
    got, kept = filter_plane(hip, src, case.pad, case.mode, ty, tx)
    expect_kept(kept, case.n[0], case.r[0], case.n[1], case.r[1])
    assert np.array_equal(got, want), (case, np.argwhere(got != want)[:5], np.abs(got - want).max())
    assert np.abs(want).max() > 1000.0


def test_a_second_workgroup_column_in_both_passes(hip):
    """261 x 259 padded by 2 at R = 6: 263 padded columns in pass 1, 261 rows in pass 2.  Host memory, the same plane as a
    row-strided view, and device memory on a stream give the same bits, those of the integer product."""
    case = FC.WIDE
    src, ty, tx, want = FC.case_data(case.name)
    got, kept = filter_plane(hip, src, case.pad, case.mode, ty, tx)
    expect_kept(kept, case.n[0], case.r[0], case.n[1], case.r[1])
    assert np.array_equal(got, want), (np.argwhere(got != want)[:5], np.abs(got - want).max())
    base = FC.integer_image((case.shape[0], case.shape[1] + 10), case.dtype, 9)
    view = base[:, 3:-7]
    view[:] = src
    assert not view.flags.c_contiguous
    assert np.array_equal(filter_plane(hip, view, case.pad, case.mode, ty, tx)[0], want), "row-strided view"
    dev, kept = filter_plane(hip, src, case.pad, case.mode, ty, tx, device=True)
    expect_kept(kept, case.n[0], case.r[0], case.n[1], case.r[1])
    assert np.array_equal(dev, want), "device memory on a stream"
    assert np.array_equal(filter_plane(hip, view, case.pad, case.mode, ty, tx, device=True)[0], want), "a strided view in device memory"


def test_bounds_checking_build_counts_no_index_outside_with_integer_tables():
    """libdiscorpy_hip_bounds.so (sites 50 and 51: the taps of every step against their table, every folded source index and plane
    column against its side) in a process of its own: the radii on 41 x 45, the three turn cases, the wrapped-only table and
    261 x 259 give the integer product and count nothing."""
    lib = os.path.join(ROOT, "discorpy_amd", "lib", "libdiscorpy_hip_bounds.so")
    assert os.path.exists(lib), "build() makes the bounds-checking library; it is missing"
    code = """
import sys, numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
sys.path.insert(0, %r)
from discorpy_amd import _ffi as F
import fourier_cases as FC
import test_fourier_taps_gpu as T
F.require_device()
assert F.debug_bounds()[4] == 1
for case in FC.BOUNDS_CASES:
    src, ty, tx, want = FC.case_data(case.name)
    got, kept = T.filter_plane(F, src, case.pad, case.mode, ty, tx)
    T.expect_kept(kept, case.n[0], case.r[0], case.n[1], case.r[1])
    assert np.array_equal(got, want), case
b = F.debug_bounds()
assert b[0] == 0 and b[4] == 1, b
print("bounds ok", len(FC.BOUNDS_CASES), b)
""" % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "helpers"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT, env=dict(os.environ, DCP_LIB_PATH=lib))
    assert r.returncode == 0 and "bounds ok %d" % len(FC.BOUNDS_CASES) in r.stdout, (r.stdout + r.stderr)[-3000:]


# --------------------------------------------------------------------------- Gaussian tables at the workload's geometry

@functools.lru_cache(maxsize=None)
def gauss_reference(k):
    """(image, the reference's plane, its normalization, the case's own e_ref), computed once."""
    shape, pad, sigma, mode = FC.GAUSS[k]
    mat = FC.gauss_image(k)
    ref = reference_filter(mat, sigma, pad, mode)
    e_ref = FC.e_ref_of(ref, mat, sigma, pad, mode)
    norm = np.mean(ref) * mat / ref
    ref.setflags(write=False)
    norm.setflags(write=False)
    return mat, ref, norm, e_ref


@pytest.fixture(scope="module")
def prep(hip):
    from discorpy_amd.prep import preprocessing
    return preprocessing


@pytest.mark.parametrize("k", range(len(FC.GAUSS)), ids=["%dx%d_p%d_s%d_%s" % (c[0] + c[1:]) for c in FC.GAUSS])
def test_gaussian_tables_with_wrapped_truncated_windows_on_both_axes(prep, hip, k):
    """The default call's geometry (2000 x 2000: R = 305 > pad = 100, below / one / above per axis, 4 R + 1 of 2 N - 1 taps) at sides
    within 264: from NumPy and from a torch tensor, within BCK_FACTOR e_ref of the reference, e_ref measured for this case.
    normalization_fft at NORM_FACTOR where pad > 0; with pad 0 the background comes close to 0 at the plane's edge (the cyclic filter
    sees the opposite edge through the sign plane), so only the background is compared there."""
    torch = pytest.importorskip("torch")
    shape, pad, sigma, mode = FC.GAUSS[k]
    mat, ref, norm, e_ref = gauss_reference(k)
    got = prep._apply_fft_filter(mat, sigma, pad, mode)
    ky, kx = kept_taps(hip)
    r = ratio(got, ref, e_ref)
    print("%s pad %d sigma %g %-9s e_ref %.3g  background %.2f e_ref  taps %d of %d, %d of %d" % (shape, pad, sigma, mode, e_ref, r, ky[0], ky[1], kx[0], kx[1]))
    for ax, (kept, whole) in enumerate((ky, kx)):
        n = shape[ax] + 2 * pad
        radius = (kept - 1) // 4
        assert whole == 2 * n - 1 and kept % 4 == 1 and 3 * kept < 2 * whole and n <= 264, (ax, kept, whole)
        assert radius > pad and FC.geometry(shape[ax], pad, radius)["branches"] == {"below", "one", "above"}, (ax, radius)
    dev = prep._apply_fft_filter(torch.from_numpy(mat.copy()).to("cuda:0"), sigma, pad, mode)
    assert isinstance(dev, torch.Tensor) and dev.dtype == torch.float64
    assert got.dtype == np.float64 and got.shape == ref.shape and np.array_equal(dev.cpu().numpy(), got)
    assert r <= BCK_FACTOR, (shape, r)
    if pad > 0:
        res = prep.normalization_fft(mat, sigma, pad, mode)
        rn = ratio(res, norm, e_ref)
        print("%s normalization %.2f e_ref" % (shape, rn))
        assert res.dtype == np.float64 and rn <= NORM_FACTOR, (shape, rn)
