"""GPU suite for the Fourier Gaussian filter (discorpy_amd.prep.preprocessing._apply_fft_filter / normalization_fft; dcp_fourier_gauss_2d,
csrc/fourier_kernels.hip) against the reference's own outputs, golden G26 (tools/gen_golden.py).

Tolerance (set by the reference, not by the kernels): a background plane passes when max|gpu - ref| / max|ref| <= 8 e_ref, e_ref the
reference's distance from a long-double evaluation of the same formula, recorded per case in the fixture (0.8e-16 .. 1.6e-15): a
sequential float64 sum of N <= 264 products may lose about sqrt(N) units of roundoff where the FFT loses log2(N), a ratio of about 2,
and the remaining factor 4 is headroom for the order of the taps.  normalization_fft: the same with factor 16 (one more division and
the mean), on the scale of max|result|.  A wrong fold, a missed wrapped tap or a wrong sign for an odd side shows at 1e-3 or worse.
Every test prints the ratio it measured before it asserts.

The kernels' workgroup covers 256 padded columns x 8 rows in pass 1 and 256 rows x 8 columns in pass 2 (kFourierBlock of
csrc/fourier_kernels.hip, kFourierRows of csrc/dcp_internal.h): the tile-edge cases put each side of the padded and of the cropped plane
at one tile, one less and one more.  Those shapes are not in the fixture; they are compared with the reference's function restated
here on scipy.fftpack, with the largest e_ref of the fixture."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, golden

pytestmark = pytest.mark.gpu

TILE_LANES, TILE_ROWS = 256, 8
BCK_FACTOR, NORM_FACTOR = 8.0, 16.0


@functools.lru_cache(maxsize=None)
def G():
    g = golden("g26_fourier_gauss")
    for v in g.values():
        v.setflags(write=False)
    return g


NAMES = [str(n) for n in golden("g26_fourier_gauss")["names"]]


def case(name):
    g = G()
    k = NAMES.index(name)
    mat = g[name + "_in"]
    if name.startswith("view_"):
        mat = mat[:, 3:-7]
    return mat, float(g["sigma"][k]), int(g["pad"][k]), str(g["mode"][k]), g[name + "_bck"], g[name + "_norm"], float(g["e_ref"][k])


def ratio(got, ref, e_ref):
    return float(np.abs(np.asarray(got) - ref).max() / np.abs(ref).max() / e_ref)


@pytest.fixture(scope="module")
def prep(hip):
    from discorpy_amd.prep import preprocessing
    return preprocessing


def kept_taps(hip):
    """((kept, all) of axis 0, (kept, all) of axis 1) from the name of the kernels that ran last."""
    m = re.fullmatch(r"fourier_rows_kernel<block=256x8, taps=(\d+) of (\d+)> \+ fourier_cols_kernel<taps=(\d+) of (\d+)>", hip.last_kernel())
    assert m, hip.last_kernel()
    v = [int(x) for x in m.groups()]
    return (v[0], v[1]), (v[2], v[3])


@pytest.mark.parametrize("name", NAMES)
def test_background_and_normalization_against_the_reference(prep, hip, name):
    """Every case of the fixture from NumPy input: odd and even padded sides at the defaults and at the cross-point sigma, full and
    narrow support, pad 0, a pad of several folds under each mode, sides of 1 and 2, every element type, a row-strided view."""
    mat, sigma, pad, mode, bck, norm, e_ref = case(name)
    got = prep._apply_fft_filter(mat, sigma, pad, mode)
    ky, kx = kept_taps(hip)
    r = ratio(got, bck, e_ref)
    print("%-22s e_ref %.3g  background %.2f e_ref  taps %d of %d, %d of %d" % (name, e_ref, r, ky[0], ky[1], kx[0], kx[1]))
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == bck.shape
    assert ky[1] == 2 * (mat.shape[0] + 2 * pad) - 1 and kx[1] == 2 * (mat.shape[1] + 2 * pad) - 1
    res = prep.normalization_fft(mat, sigma, pad, mode)
    rn = ratio(res, norm, e_ref)
    print("%-22s normalization %.2f e_ref" % (name, rn))
    assert res.dtype == np.float64 and res.shape == norm.shape
    assert r <= BCK_FACTOR, (name, r)
    assert rn <= NORM_FACTOR, (name, rn)


def test_support_is_the_whole_table_or_far_less(prep, hip):
    """sigma 1 and 0.5: every tap is kept (but for the middle one of an even side, which cancels exactly) and the wrapped half is in
    use.  sigma 40 on 264 x 248: the window is cut off at 4e-3 of its peak at the ends of the axis, its transform has an algebraic
    tail and the bound keeps everything as well -- the support is NOT narrow there.  Where the window decays inside the axis the bound
    leaves |d| <= R and |d| >= N - R with R about 0.15 N (10 / sigma): sigma 10 on 237 x 252 keeps less than a third of the table,
    sigma 5 less than two thirds."""
    for name in ("full_50x61", "full_30x45", "narrow_64x48", "pad0_33x47"):
        mat, sigma, pad, mode = case(name)[:4]
        prep._apply_fft_filter(mat, sigma, pad, mode)
        ky, kx = kept_taps(hip)
        assert ky[0] >= ky[1] - 2 and kx[0] >= kx[1] - 2, (name, ky, kx)
    for name, most in (("s37x52_p100_s10", 1.0 / 3.0), ("s40x51_p100_s10", 1.0 / 3.0), ("s37x52_p100_s5", 2.0 / 3.0), ("s40x51_p100_s5", 2.0 / 3.0)):
        mat, sigma, pad, mode = case(name)[:4]
        prep._apply_fft_filter(mat, sigma, pad, mode)
        ky, kx = kept_taps(hip)
        assert ky[1] / 8 < ky[0] < most * ky[1] and kx[1] / 8 < kx[0] < most * kx[1] and ky[0] % 4 == 1 and kx[0] % 4 == 1, (name, ky, kx)


def reference_filter(mat, sigma, pad, mode):
    """discorpy/prep/preprocessing.py:102-128 restated (the reference module itself needs scikit-image to import)."""
    from scipy.fftpack import fft2, ifft2
    mat = np.pad(mat, ((pad, pad), (pad, pad)), mode=mode)
    (height, width) = mat.shape
    xcenter, ycenter = (width - 1.0) / 2.0, (height - 1.0) / 2.0
    y, x = np.ogrid[-ycenter:height - ycenter, -xcenter:width - xcenter]
    num = 2.0 * sigma * sigma
    window = np.exp(-(x * x / num + y * y / num))
    x, y = np.meshgrid(np.arange(0, width), np.arange(0, height))
    matsign = np.power(-1.0, x + y)
    mat = np.real(ifft2(fft2(mat * matsign) * window) * matsign)
    return mat[pad:height - pad, pad:width - pad]


def test_restated_reference_is_the_fixtures_reference():
    """The restatement the tile cases are checked against reproduces the fixture's planes bit for bit."""
    for name in ("s37x52_p100_s5", "full_30x45", "folds_8x5_wrap", "type_uint16"):
        mat, sigma, pad, mode, bck = case(name)[:5]
        assert np.array_equal(reference_filter(mat, sigma, pad, mode), bck), name


TILE_CASES = ([(axis, side, 0) for axis in (0, 1) for side in (TILE_LANES - 1, TILE_LANES, TILE_LANES + 1, TILE_ROWS - 1, TILE_ROWS, TILE_ROWS + 1)]
              + [(axis, side, 5) for axis in (0, 1) for side in (TILE_LANES - 11, TILE_LANES - 10, TILE_LANES - 9, TILE_LANES - 1, TILE_LANES,
                                                                  TILE_LANES + 1)])


@pytest.mark.parametrize("axis,side,pad", TILE_CASES, ids=["axis%d-side%d-pad%d" % c for c in TILE_CASES])
def test_tile_edges(prep, hip, axis, side, pad):
    """One side at a workgroup tile, one less and one more (256 lanes, 8 register rows; with pad 5 the PADDED side too: 246 + 10), the
    other side 17."""
    shape = (side, 17) if axis == 0 else (17, side)
    rng = np.random.default_rng(1000 * side + 10 * pad + axis)
    mat = rng.uniform(50.0, 250.0, shape).astype(np.float32)
    e_ref = float(G()["e_ref"].max())
    for mode in ("reflect", "constant"):
        ref = reference_filter(mat, 3, pad, mode)
        got = prep._apply_fft_filter(mat, 3, pad, mode)
        r = ratio(got, ref, e_ref)
        print("%s pad %d %-8s %.2f e_ref (e_ref %.3g)" % (shape, pad, mode, r, e_ref))
        assert got.shape == ref.shape and r <= BCK_FACTOR, (shape, pad, mode, r)


def test_every_memory_kind_and_a_strided_view_give_the_same_bits(prep, hip):
    torch = pytest.importorskip("torch")
    mat, sigma, pad, mode, bck, norm, e_ref = case("s40x51_p100_s10")
    host = prep._apply_fft_filter(mat, sigma, pad, mode)
    t = torch.from_numpy(mat.copy()).to("cuda:0")
    dev = prep._apply_fft_filter(t, sigma, pad, mode)
    assert isinstance(dev, torch.Tensor) and dev.dtype == torch.float64 and dev.device == t.device
    cai = hip.DeviceArray(mat.shape, mat.dtype).copy_from_host(mat)
    other = prep._apply_fft_filter(cai, sigma, pad, mode)
    assert isinstance(other, hip.DeviceArray) and other.dtype == np.float64 and other.shape == mat.shape
    torch.cuda.synchronize()
    assert ratio(host, bck, e_ref) <= BCK_FACTOR
    assert np.array_equal(dev.cpu().numpy(), host) and np.array_equal(other.copy_to_host(), host)
    # a view whose rows are strided, read in place: NumPy, tensor, and the C ABI with the view's own stride
    g = G()
    base = g["view_40x58_in"]
    view, ref = base[:, 3:-7], g["view_40x58_bck"]
    assert not view.flags.c_contiguous
    vh = prep._apply_fft_filter(view, 3, 9)
    vt = prep._apply_fft_filter(torch.from_numpy(base.copy()).to("cuda:0")[:, 3:-7], 3, 9)
    taps = prep._fourier_taps(40 + 18, 3) + prep._fourier_taps(48 + 18, 3)
    out = np.empty((40, 48), np.float64)
    hip.check(hip.lib().dcp_fourier_gauss_2d(view.ctypes.data, out.ctypes.data, 40, 48, 58, hip.DTYPE_BY_NAME["float32"], 9, 5,
                                             *[v.ctypes.data_as(hip.C.POINTER(hip.C.c_double)) for v in taps], hip.MEM_HOST, -1, None))
    assert ratio(vh, ref, float(g["e_ref"][NAMES.index("view_40x58")])) <= BCK_FACTOR
    assert np.array_equal(vt.cpu().numpy(), vh) and np.array_equal(out, vh)
    assert np.array_equal(prep._apply_fft_filter(np.ascontiguousarray(view), 3, 9), vh)


@pytest.mark.parametrize("name", ["type_float32", "type_uint16"])
def test_normalization_of_a_tensor(prep, hip, name):
    torch = pytest.importorskip("torch")
    mat, sigma, pad, mode, bck, norm, e_ref = case(name)
    t = torch.from_numpy(mat.copy()).to("cuda:0")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        res = prep.normalization_fft(t, sigma, pad, mode)
    stream.synchronize()
    assert isinstance(res, torch.Tensor) and res.dtype == torch.float64 and res.device == t.device
    r = ratio(res.cpu().numpy(), norm, e_ref)
    print("%-14s tensor normalization %.2f e_ref" % (name, r))
    assert r <= NORM_FACTOR, (name, r)
    host = prep.normalization_fft(mat, sigma, pad, mode)
    assert host.dtype == np.float64 and ratio(host, norm, e_ref) <= NORM_FACTOR


def test_interleaved_calls_give_the_bits_of_each_alone(prep, hip):
    """Two calls with different (n, sigma) interleaved, across an emptied and an overflowing table cache and a released workspace."""
    a = case("s37x52_p100_s10")[:4]
    b = case("s40x51_p100_s5")[:4]
    prep._fourier_taps_of.cache_clear()
    alone_a = prep._apply_fft_filter(*a)
    prep._fourier_taps_of.cache_clear()
    alone_b = prep._apply_fft_filter(*b)
    for _ in range(2):
        assert np.array_equal(prep._apply_fft_filter(*a), alone_a)
        assert np.array_equal(prep._apply_fft_filter(*b), alone_b)
    for n in range(3, 3 + 2 * prep._fourier_taps_of.cache_info().maxsize):       # push both calls' tables out of the cache
        prep._fourier_taps(n, 2.0)
    hip.release_scratch()
    assert np.array_equal(prep._apply_fft_filter(*b), alone_b)
    assert np.array_equal(prep._apply_fft_filter(*a), alone_a)


def test_bounds_checking_build_counts_no_index_outside_its_plane(hip):
    """The library built with -DDCP_DEBUG_BOUNDS checks, in both passes (sites 50 and 51), the run of taps every step reads against its
    table and every folded source index and plane column against its side: a process of its own runs the truncated and the full support,
    pads of several folds under each mode, sides of 1 and 2 and a side one more than a tile, and nothing may lie outside."""
    lib = os.path.join(ROOT, "discorpy_amd", "lib", "libdiscorpy_hip_bounds.so")
    assert os.path.exists(lib), "build() makes the bounds-checking library; it is missing"
    code = """
import sys, numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
from discorpy_amd import _ffi as F
from discorpy_amd.prep import preprocessing as prep
import test_fourier_gauss_gpu as T
F.require_device()
assert F.debug_bounds()[4] == 1
for name in T.NAMES:
    if name.startswith(("s37x52_", "s40x51_", "narrow_", "full_", "folds_", "tiny_", "pad0_", "view_")) or name == "type_bool":
        mat, sigma, pad, mode, bck, norm, e_ref = T.case(name)
        r = T.ratio(prep._apply_fft_filter(mat, sigma, pad, mode), bck, e_ref)
        assert r <= T.BCK_FACTOR, (name, r)
        if name == "s37x52_p100_s10":
            ky, kx = T.kept_taps(F)
            assert 3 * ky[0] < ky[1] and 3 * kx[0] < kx[1], (ky, kx)
rng = np.random.default_rng(5)
for shape in ((257, 17), (17, 257)):
    mat = rng.uniform(50.0, 250.0, shape).astype(np.float32)
    for mode in ("symmetric", "constant"):
        r = T.ratio(prep._apply_fft_filter(mat, 3, 5, mode), T.reference_filter(mat, 3, 5, mode), float(T.G()["e_ref"].max()))
        assert r <= T.BCK_FACTOR, (shape, mode, r)
b = F.debug_bounds()
assert b[0] == 0 and b[4] == 1, b
print("bounds ok", b)
""" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT, env=dict(os.environ, DCP_LIB_PATH=lib))
    assert r.returncode == 0 and "bounds ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
