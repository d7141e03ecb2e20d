"""GPU suite for the Gaussian filter (discorpy_amd.prep.linepattern.gaussian_filter; csrc/gauss_kernels.hip): every comparison is
np.array_equal against scipy.ndimage.gaussian_filter -- the kernels restate scipy's float64 operations one by one
(tests/helpers/gaussian_reference.py is the same restatement on the CPU), so there is no rounding to allow for.

gauss_lds_kernel's tile is 128 columns x 32 rows: (33, 129) is one more than a tile in each axis, (57, 153) the staged box of that tile
at sigma 3 (radius 12).  Every case runs three routes: the default one (x_gauss_lds = 1: the fused kernel up to radius 24 and 80 KiB
of LDS, where it measured no slower than the per-axis route, one gauss_axis_kernel launch per axis beyond), the fused kernel wherever its planes fit LDS
(x_gauss_lds = 2) and one gauss_axis_kernel launch per axis always (x_gauss_lds = 0).  A call with one axis skipped is one
gauss_axis_kernel launch on every route.

Data: standard normal scaled by 40 (plus 128 for unsigned types) clipped into the type's range, so that every float64 result lies
inside the type; int64 is scaled by 2^40 on top (values within +-2^53, where scipy's read through a double is exact)."""
import functools

import numpy as np
import pytest
from scipy import ndimage as ndi

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 7), (5, 5), (3, 40), (2, 300), (33, 129), (57, 153)]
SIGMAS = [0.5, 1, 3, 5.3, (3, 0), (0, 3), (1, 5.3)]
MODES = ["reflect", "nearest", "mirror", "wrap", "constant"]
CVAL = 1.5
SUBSET_SHAPES = [(3, 40), (33, 129), (57, 153)]
SUBSET_SIGMAS = [0.5, 3, (1, 5.3)]


@functools.lru_cache(maxsize=None)
def image(shape, dtype):
    rng = np.random.default_rng(1000 * shape[0] + shape[1])
    dt = np.dtype(dtype)
    a = rng.standard_normal(shape) * 40.0
    if dt.kind in "iu":
        info = np.iinfo(dt)
        a = np.clip(a + (128.0 if dt.kind == "u" else 0.0), info.min, info.max)
    a = a.astype(dt)
    if dt == np.int64:
        a = a << 40
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def want(shape, dtype, sigma, mode):
    out = ndi.gaussian_filter(image(shape, dtype), sigma, mode=mode, cval=CVAL)
    out.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def lp(hip):
    from discorpy_amd.prep import linepattern
    return linepattern


FUSED_MAX_RADIUS, FUSED_MAX_LDS = 24, 80 << 10          # kGaussFusedMaxRadius, kGaussFusedMaxLds of csrc/dcp_internal.h


def lds_bytes(ry, rx, itemsize):
    """The two LDS planes of gauss_lds_kernel's 128 x 32 tile, the second one starting at a multiple of 16 bytes."""
    box = (32 + 2 * ry) * (128 + 2 * rx) * itemsize
    return (box + 15) // 16 * 16 + 32 * (128 + 2 * rx) * itemsize


@pytest.fixture
def route(hip):
    """route(value, fn) runs fn under x_gauss_lds = value; the option is restored afterwards."""
    old = hip.get_option("x_gauss_lds")

    def run(value, fn):
        hip.set_option("x_gauss_lds", value)
        try:
            return fn()
        finally:
            hip.set_option("x_gauss_lds", old)
    yield run
    hip.set_option("x_gauss_lds", old)


def kernel_names(dtype, sigma):
    """What x_gauss_lds = 1 (the default), 2 and 0 run for a sigma of the grid: every box of the grid fits LDS."""
    name = np.dtype(dtype).name
    fused = "gauss_lds_kernel<%s, tile=128x32>" % name
    both = "gauss_axis_kernel<%s, axis=0> + gauss_axis_kernel<%s, axis=1>" % (name, name)
    sy, sx = (sigma, sigma) if np.ndim(sigma) == 0 else sigma
    if sy > 0 and sx > 0:
        ry, rx = int(4.0 * sy + 0.5), int(4.0 * sx + 0.5)
        default = max(ry, rx) <= FUSED_MAX_RADIUS and lds_bytes(ry, rx, np.dtype(dtype).itemsize) <= FUSED_MAX_LDS
        return {1: fused if default else both, 2: fused, 0: both}
    one = "gauss_axis_kernel<%s, axis=%d>" % (name, 0 if sy > 0 else 1)
    return {1: one, 2: one, 0: one}


def check_grid(lp, hip, route, shape, dtype, sigmas):
    a = image(shape, dtype)
    assert hip.get_option("x_gauss_lds") == 1
    for sigma in sigmas:
        names = kernel_names(dtype, sigma)
        for mode in MODES:
            ref = want(shape, dtype, sigma, mode)
            for value in (1, 2, 0):
                got = route(value, lambda: lp.gaussian_filter(a, sigma, mode=mode, cval=CVAL))
                assert hip.last_kernel() == names[value], (sigma, mode, value, hip.last_kernel())
                assert got.dtype == ref.dtype and got.shape == ref.shape
                assert np.array_equal(got, ref), (sigma, mode, "x_gauss_lds = %d" % value)


@pytest.mark.parametrize("dtype", ["float32", "uint8"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_whole_grid(lp, hip, route, shape, dtype):
    check_grid(lp, hip, route, shape, dtype, SIGMAS)


@pytest.mark.parametrize("dtype", ["float64", "int16", "uint16", "int32", "int64"])
@pytest.mark.parametrize("shape", SUBSET_SHAPES, ids=lambda s: "%dx%d" % s)
def test_other_element_types(lp, hip, route, shape, dtype):
    check_grid(lp, hip, route, shape, dtype, SUBSET_SIGMAS)


def test_default_route_on_both_sides_of_its_limits(hip):
    """What kernel_names() expects of x_gauss_lds = 1, spelt out: float32 takes the fused kernel at sigma 5.3 (radius 21, 72 080 bytes)
    and the per-axis route at sigma 8 (radius 32); float64 takes the fused kernel at sigma 0.5 and leaves it at sigma 3 (radius 12:
    107 008 bytes, one workgroup per CU)."""
    assert lds_bytes(21, 21, 4) == 72080 and lds_bytes(12, 12, 8) == 107008 and lds_bytes(12, 12, 4) == 34048 + 19456
    assert kernel_names("float32", 5.3)[1].startswith("gauss_lds_kernel") and kernel_names("float32", 8)[1].startswith("gauss_axis_kernel")
    assert kernel_names("float64", 0.5)[1].startswith("gauss_lds_kernel") and kernel_names("float64", 3)[1].startswith("gauss_axis_kernel")
    assert kernel_names("uint16", 6)[1].startswith("gauss_lds_kernel") and kernel_names("uint16", 6.2)[1].startswith("gauss_axis_kernel")


def test_nearest_as_the_reference_calls_it(lp, hip):
    """linepattern.py:592: ndi.gaussian_filter(mat, sigma, mode="nearest") with the default sigma of 3, and :659 ndi.gaussian_filter(mat, 3)."""
    a = image((57, 153), "float32")
    assert np.array_equal(lp.gaussian_filter(a, 3, mode="nearest"), ndi.gaussian_filter(a, 3, mode="nearest"))
    assert np.array_equal(lp.gaussian_filter(a, 3), ndi.gaussian_filter(a, 3))
    for alias in ("grid-mirror", "grid-constant", "grid-wrap"):
        assert np.array_equal(lp.gaussian_filter(a, 3, mode=alias, cval=CVAL), ndi.gaussian_filter(a, 3, mode=alias, cval=CVAL)), alias
    assert np.array_equal(lp.gaussian_filter(a, 2, truncate=2.5), ndi.gaussian_filter(a, 2, truncate=2.5))
    assert np.array_equal(lp.gaussian_filter(a, 2, radius=(3, 9)), ndi.gaussian_filter(a, 2, radius=(3, 9)))
    assert np.array_equal(lp.gaussian_filter(a, 0), a) and hip.last_kernel() == "gauss_copy"


def test_boxes_above_64_kib_and_above_the_lds_cap(lp, hip, route):
    """float32 at sigma 8 (radius 32): planes of 96 x 192 and 32 x 192 elements = 98 304 bytes, the dynamic-LDS route above 64 KiB.
    At sigma 14 (radius 56) they are 144 x 240 and 32 x 240 elements = 168 960 bytes, above the CU's 163 840: one launch per axis
    even under x_gauss_lds = 2.  float64 reaches the cap at sigma 10 (radius 40: 112 x 208 + 32 x 208 elements of 8 bytes = 239 616 bytes)."""
    fused, both = "gauss_lds_kernel<float32, tile=128x32>", "gauss_axis_kernel<float32, axis=0> + gauss_axis_kernel<float32, axis=1>"
    a = image((57, 153), "float32")
    for mode in MODES:
        for value, name in ((2, fused), (1, both)):
            got = route(value, lambda: lp.gaussian_filter(a, 8, mode=mode, cval=CVAL))
            assert hip.last_kernel() == name
            assert np.array_equal(got, want((57, 153), "float32", 8, mode)), (mode, value)
        got = route(2, lambda: lp.gaussian_filter(a, 14, mode=mode, cval=CVAL))
        assert hip.last_kernel() == both
        assert np.array_equal(got, want((57, 153), "float32", 14, mode)), mode
    d = image((33, 129), "float64")
    got = route(2, lambda: lp.gaussian_filter(d, 10, mode="mirror"))
    assert hip.last_kernel() == "gauss_axis_kernel<float64, axis=0> + gauss_axis_kernel<float64, axis=1>"
    assert np.array_equal(got, want((33, 129), "float64", 10, "mirror"))
    # the plane between the two launches came from the library's scratch: releasing it leaves the next call working
    hip.release_scratch()
    assert np.array_equal(lp.gaussian_filter(d, 10, mode="mirror"), want((33, 129), "float64", 10, "mirror"))


def test_row_strided_view_is_read_in_place(lp, hip, route):
    base = image((57, 153), "uint16")
    view = base[:, 3:-7]
    assert not view.flags.c_contiguous
    ref = ndi.gaussian_filter(view, 3, mode="mirror")
    assert np.array_equal(lp.gaussian_filter(view, 3, mode="mirror"), ref)
    assert np.array_equal(route(0, lambda: lp.gaussian_filter(view, 3, mode="mirror")), ref)
    # the same through the C ABI with the view's own stride: nothing was copied on the way
    w = lp._gaussian_weights(3)
    wp = w.ctypes.data_as(hip.C.POINTER(hip.C.c_double))
    out = np.empty((57, 143), np.uint16)
    hip.check(hip.lib().dcp_correlate_sym_2d(view.ctypes.data, out.ctypes.data, 57, 143, 153, hip.DTYPE_BY_NAME["uint16"], wp, 12, wp, 12, 5, 0.0,
                                             hip.MEM_HOST, -1, None))
    assert np.array_equal(out, ref)


def test_out_argument(lp):
    a = image((33, 129), "uint8")
    out = np.empty((33, 129), np.uint8)
    assert lp.gaussian_filter(a, 3, mode="wrap", out=out) is out
    assert np.array_equal(out, want((33, 129), "uint8", 3, "wrap"))
    with pytest.raises(ValueError, match="out must be"):
        lp.gaussian_filter(a, 3, out=np.empty((33, 129), np.uint16))
    with pytest.raises(ValueError, match="overlap"):
        b = np.zeros((33, 129), np.uint8)
        lp.gaussian_filter(b, 3, out=b)


def test_torch_tensor_on_the_current_stream(lp, hip, route):
    torch = pytest.importorskip("torch")
    a = image((57, 153), "float32")
    host = lp.gaussian_filter(a, (1, 5.3), mode="constant", cval=CVAL)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        t = torch.from_numpy(a.copy()).to("cuda:0", non_blocking=False)
        got = lp.gaussian_filter(t, (1, 5.3), mode="constant", cval=CVAL)
        one = route(2, lambda: lp.gaussian_filter(t, (1, 5.3), mode="constant", cval=CVAL))
        two = route(0, lambda: lp.gaussian_filter(t, (1, 5.3), mode="constant", cval=CVAL))
        view = lp.gaussian_filter(t[:, 3:-7], 3)                # a row-strided tensor view, in place
        tout = torch.empty((57, 153), dtype=torch.float32, device="cuda:0")
        assert lp.gaussian_filter(t, 3, mode="nearest", out=tout) is tout
    stream.synchronize()
    assert isinstance(got, torch.Tensor) and got.device == t.device and got.dtype == torch.float32
    assert np.array_equal(got.cpu().numpy(), host) and np.array_equal(host, want((57, 153), "float32", (1, 5.3), "constant"))
    assert np.array_equal(one.cpu().numpy(), host) and np.array_equal(two.cpu().numpy(), host)
    assert np.array_equal(view.cpu().numpy(), ndi.gaussian_filter(a[:, 3:-7], 3))
    assert np.array_equal(tout.cpu().numpy(), want((57, 153), "float32", 3, "nearest"))


def test_cuda_array_interface_array(lp, hip):
    a = image((33, 129), "int16")
    dev = hip.DeviceArray((33, 129), np.int16).copy_from_host(a)
    got = lp.gaussian_filter(dev, 3, mode="mirror")
    assert isinstance(got, hip.DeviceArray) and got.shape == (33, 129) and got.dtype == np.int16
    assert np.array_equal(got.copy_to_host(), want((33, 129), "int16", 3, "mirror"))


def test_bounds_checking_build_counts_no_tap_outside_its_plane(hip):
    """The library built with -DDCP_DEBUG_BOUNDS (build() makes it next to the product library) checks the span of every tap loop of
    gauss_lds_kernel against its LDS plane: a process of its own loads it and runs boxes below and above 64 KiB, tiles that reach
    over every edge, images smaller than the radius and constant mode, and no tap may lie outside."""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    lib = os.path.join(ROOT, "discorpy_amd", "lib", "libdiscorpy_hip_bounds.so")
    assert os.path.exists(lib), "build() makes the bounds-checking library; it is missing"
    code = """
import sys, numpy as np
sys.path.insert(0, %r)
from scipy import ndimage as ndi
from discorpy_amd import _ffi as F
from discorpy_amd.prep import linepattern as lp
F.require_device()
assert F.debug_bounds()[4] == 1
F.set_option("x_gauss_lds", 2)
rng = np.random.default_rng(2)
for shape, dtype, sigma in (((57, 153), "float32", 3), ((33, 129), "float64", (1, 5.3)), ((3, 40), "uint8", 5.3), ((70, 300), "float32", 8),
                            ((2, 300), "uint16", 3)):
    a = (rng.standard_normal(shape) * 40.0 + 128.0).clip(0, 255).astype(dtype)
    for mode in ("reflect", "constant", "mirror"):
        assert np.array_equal(lp.gaussian_filter(a, sigma, mode=mode, cval=1.5), ndi.gaussian_filter(a, sigma, mode=mode, cval=1.5)), (shape, mode)
        assert F.last_kernel().startswith("gauss_lds_kernel"), F.last_kernel()
b = F.debug_bounds()
assert b[0] == 0 and b[4] == 1, b
print("bounds ok", b)
""" % (ROOT,)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT, env=dict(os.environ, DCP_LIB_PATH=lib))
    assert r.returncode == 0 and "bounds ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
