"""GPU suite for the median filter (discorpy_amd.prep.preprocessing; csrc/median_kernels.hip): every comparison is np.array_equal
against scipy.ndimage.median_filter(a, size, mode="reflect") -- a median selects one input element, so there is no rounding to allow
for.  Every shape keeps size // 2 < 4 * side (or a side of 1): the range in which scipy 1.15.3 reflects correctly.

The kernel's tile is 64 columns x 16 / 8 / 4 rows (16 for every window below whose key box fits 64 KiB; (64, 64) / 101 takes the
dynamic-LDS route above 64 KiB); (33, 65) and (17, 65) are one more than the 16 x 64 tile in each axis.

The reference's normalization (discorpy/prep/preprocessing.py:66-73) is restated with scipy's filter: its module cannot be imported
without scikit-image."""
import functools

import numpy as np
import pytest
from scipy import ndimage as ndi

pytestmark = pytest.mark.gpu

PAIRS = [((1, 1), 51), ((1, 1), (2, 2)), ((7, 5), (2, 2)), ((33, 65), (2, 2)), ((17, 130), 3), ((40, 70), (9, 5)), ((40, 70), (4, 6)),
         ((9, 200), 15), ((26, 26), 51), ((50, 50), 51), ((25, 90), 51), ((60, 131), 51), ((64, 64), 101), ((70, 300), (1, 51)),
         ((300, 70), (51, 1)), ((17, 65), 3)]
ALL_DTYPES = ("float32", "float64", "uint8", "int8", "uint16", "int16", "uint32", "int32", "int64", "uint64", "bool")


def _seed(*key):
    """The same seed in every process (hash() of a string is not)."""
    return sum(ord(c) * (i + 1) for i, c in enumerate(repr(key))) % (1 << 31)


@functools.lru_cache(maxsize=None)
def image(shape, dtype, kind):
    """kind "ties": integers 0..8 (heavy ties); "normal": standard_normal (negative values) with a block of zeros, scaled into the
    range of an integer type; "wide": draws over the whole range of the type (64-bit integers: within +-2^53, where scipy, which
    reads them as doubles, is still exact).  Read-only: shared between tests."""
    rng = np.random.default_rng(_seed(shape, dtype, kind))
    dt = np.dtype(dtype)
    h, w = shape
    if kind == "ties":
        a = rng.integers(0, 9, size=shape).astype(dt)
    elif kind == "normal" or dt.kind == "f":
        a = rng.standard_normal(shape)
        if dt.kind in "iu":
            info = np.iinfo(dt)
            a = np.clip(a * 40.0 + (128.0 if dt.kind == "u" else 0.0), info.min, info.max)
        a = a.astype(dt)
        a[h // 4:h // 4 + max(h // 2, 1), w // 4:w // 4 + max(w // 2, 1)] = 0
    elif dt.kind == "b":
        a = rng.random(shape) < 0.5
    else:
        info = np.iinfo(dt)
        lo, hi = max(info.min, -(1 << 53)), min(info.max, 1 << 53)
        a = rng.integers(lo, hi, size=shape, endpoint=True, dtype=np.int64 if dt.kind == "i" else np.uint64).astype(dt)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def want(shape, dtype, kind, size):
    out = ndi.median_filter(image(shape, dtype, kind), size, mode="reflect")
    out.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def prep(hip):
    from discorpy_amd.prep import preprocessing
    return preprocessing


@pytest.fixture
def global_kernel(hip):
    """x_median_lds = 0 for the test, restored afterwards."""
    old = hip.get_option("x_median_lds")
    hip.set_option("x_median_lds", 0)
    try:
        yield hip
    finally:
        hip.set_option("x_median_lds", old)


def _id(v):
    return "x".join(str(s) for s in v) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("kind", ["ties", "normal"])
@pytest.mark.parametrize("dtype", ["float32", "uint8"])
@pytest.mark.parametrize("shape,size", PAIRS, ids=["%s-%s" % (_id(s), _id(k)) for s, k in PAIRS])
def test_shapes_and_sizes(prep, hip, shape, size, dtype, kind):
    a = image(shape, dtype, kind)
    got = prep.median_filter(a, size)
    assert hip.last_kernel().startswith("median_lds_kernel<bits=%d" % (a.itemsize * 8)), hip.last_kernel()
    assert got.dtype == a.dtype and got.shape == a.shape
    assert np.array_equal(got, want(shape, dtype, kind, size))


def test_dynamic_lds_above_64_kib_is_what_the_largest_window_takes(prep, hip):
    prep.median_filter(image((64, 64), "float32", "ties"), 101)
    assert hip.last_kernel() == "median_lds_kernel<bits=32, tile=64x16>"           # 116 x 164 keys of 4 bytes = 76096 bytes
    prep.median_filter(image((40, 70), "float64", "ties"), (9, 5))
    assert hip.last_kernel() == "median_lds_kernel<bits=64, tile=64x16>"


@pytest.mark.parametrize("dtype", ALL_DTYPES)
@pytest.mark.parametrize("shape,size", [((40, 70), (9, 5)), ((7, 5), (2, 2))], ids=["40x70-9x5", "7x5-2x2"])
def test_every_element_type(prep, shape, size, dtype):
    a = image(shape, dtype, "wide")
    got = prep.median_filter(a, size)
    assert got.dtype == a.dtype
    assert np.array_equal(got, want(shape, dtype, "wide", size))


def test_sixty_four_bit_integers_are_selected_exactly(prep):
    """Beyond 2^53 scipy (which reads the values as doubles) is not a reference any more: a brute-force selection is."""
    rng = np.random.default_rng(5)
    for dt in (np.int64, np.uint64):
        info = np.iinfo(dt)
        a = rng.integers(info.min, info.max, size=(9, 11), endpoint=True, dtype=dt)
        a[2, 3:6] = info.max - np.arange(3).astype(dt)            # neighbours that one double cannot tell apart
        a[5, 1:4] = info.min + np.arange(3).astype(dt)
        pad = np.pad(a, ((1, 1), (1, 1)), mode="symmetric")
        ref = np.array([[np.sort(pad[y:y + 3, x:x + 3], axis=None)[4] for x in range(11)] for y in range(9)], dtype=dt)
        assert np.array_equal(prep.median_filter(a, 3), ref)


@pytest.mark.parametrize("shape,size,dtype", [((40, 70), (9, 5), "float32"), ((40, 70), (9, 5), "uint8"), ((26, 26), 51, "float32"),
                                              ((26, 26), 51, "uint8")], ids=lambda v: _id(v))
def test_global_kernel_when_forced(prep, global_kernel, shape, size, dtype):
    for kind in ("ties", "normal"):
        got = prep.median_filter(image(shape, dtype, kind), size)
        assert global_kernel.last_kernel() == "median_global_kernel<bits=%d>" % (np.dtype(dtype).itemsize * 8)
        assert np.array_equal(got, want(shape, dtype, kind, size))


def test_global_kernel_when_no_box_fits(prep, hip):
    """float64 (40, 48) at 201: the smallest box, (4 + 200) x (64 + 200) keys of 8 bytes, is 430 KB."""
    assert hip.get_option("x_median_lds") == 1
    got = prep.median_filter(image((40, 48), "float64", "normal"), 201)
    assert hip.last_kernel() == "median_global_kernel<bits=64>"
    assert np.array_equal(got, want((40, 48), "float64", "normal", 201))


def test_row_strided_view_is_read_in_place(prep, hip):
    base = image((40, 80), "uint16", "wide")
    view = base[:, 3:-7]
    assert not view.flags.c_contiguous
    got = prep.median_filter(view, (9, 5))
    assert got.shape == (40, 70) and got.dtype == np.uint16
    assert np.array_equal(got, ndi.median_filter(view, (9, 5), mode="reflect"))
    # the same through the C ABI with the view's own stride: nothing was copied on the way
    out = np.empty((40, 70), np.uint16)
    hip.check(hip.lib().dcp_median_filter_2d(view.ctypes.data, out.ctypes.data, 40, 70, 80, hip.DTYPE_BY_NAME["uint16"], 9, 5,
                                             hip.MEM_HOST, -1, None))
    assert np.array_equal(out, got)


def test_torch_tensor_on_the_current_stream(prep, hip):
    torch = pytest.importorskip("torch")
    a = image((60, 131), "float32", "normal")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        t = torch.from_numpy(a.copy()).to("cuda:0", non_blocking=False)
        got = prep.median_filter(t, 51)
        view = prep.median_filter(t[:, 3:-7], (9, 5))           # a row-strided tensor view, in place
    stream.synchronize()
    assert isinstance(got, torch.Tensor) and got.device == t.device and got.dtype == torch.float32
    assert np.array_equal(got.cpu().numpy(), want((60, 131), "float32", "normal", 51))
    assert np.array_equal(view.cpu().numpy(), ndi.median_filter(a[:, 3:-7], (9, 5), mode="reflect"))


def test_out_argument(prep):
    torch = pytest.importorskip("torch")
    a = image((40, 70), "uint8", "normal")
    out = np.empty((40, 70), np.uint8)
    assert prep.median_filter(a, (4, 6), out=out) is out
    assert np.array_equal(out, want((40, 70), "uint8", "normal", (4, 6)))
    with pytest.raises(ValueError, match="out must be"):
        prep.median_filter(a, 3, out=np.empty((40, 70), np.uint16))
    with pytest.raises(ValueError, match="overlap"):
        b = np.zeros((40, 70), np.uint8)
        prep.median_filter(b, 3, out=b)
    t = torch.from_numpy(a.copy()).to("cuda:0")
    tout = torch.empty((40, 70), dtype=torch.uint8, device="cuda:0")
    assert prep.median_filter(t, (4, 6), out=tout) is tout
    torch.cuda.synchronize()
    assert np.array_equal(tout.cpu().numpy(), want((40, 70), "uint8", "normal", (4, 6)))


def test_cuda_array_interface_array(prep, hip):
    a = image((40, 70), "int16", "wide")
    dev = hip.DeviceArray((40, 70), np.int16).copy_from_host(a)
    got = prep.median_filter(dev, (9, 5))
    assert isinstance(got, hip.DeviceArray) and got.shape == (40, 70) and got.dtype == np.int16
    assert np.array_equal(got.copy_to_host(), want((40, 70), "int16", "wide", (9, 5)))


def reference_normalization(mat, size=51):
    """discorpy/prep/preprocessing.py:66-73 with scipy's filter."""
    mat_bck = ndi.median_filter(mat, size, mode="reflect")
    mean_val = np.mean(mat_bck)
    try:
        mat_cor = mean_val * mat / mat_bck
    except ZeroDivisionError:
        mat_bck[mat_bck == 0.0] = mean_val
        mat_cor = mean_val * mat / mat_bck
    return mat_cor


def test_normalization_of_host_arrays_is_the_reference_bit_for_bit(prep):
    a = image((60, 131), "float32", "normal")           # the block of zeros makes the background zero there: 0 / 0 and x / 0
    with np.errstate(all="ignore"):
        got, ref = prep.normalization(a), reference_normalization(a)
    assert got.dtype == ref.dtype == np.float32 and np.isnan(ref).any()
    assert np.array_equal(got, ref, equal_nan=True)
    u = image((40, 70), "uint16", "wide")
    with np.errstate(all="ignore"):
        got, ref = prep.normalization(u, 9), reference_normalization(u, 9)
    assert got.dtype == ref.dtype == np.float64
    assert np.array_equal(got, ref, equal_nan=True)


def test_normalization_of_a_device_tensor(prep):
    """The device path takes the mean in float64 and rounds it to float32, the reference sums n float32 values: they differ by at most
    the worst-case float32 summation bound n * 2^-24 (relative: the background of this image is positive, so nothing cancels in the
    sum), and the product and the quotient round once each on either side: rtol = (n + 2) * 2^-24."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(11)
    h, w = 60, 131
    a = (rng.random((h, w), dtype=np.float32) + 0.5) * np.linspace(1.0, 3.0, w, dtype=np.float32)
    t = torch.from_numpy(a).to("cuda:0")
    got = prep.normalization(t)
    bck = prep.median_filter(t, 51)
    torch.cuda.synchronize()
    assert isinstance(got, torch.Tensor) and got.dtype == torch.float32 and got.device == t.device
    ref_bck = ndi.median_filter(a, 51, mode="reflect")
    assert np.array_equal(bck.cpu().numpy(), ref_bck)
    ref = reference_normalization(a)
    ok = ref_bck != 0
    assert ok.all()
    rtol = (h * w + 2) * 2.0 ** -24
    err = np.abs(got.cpu().numpy().astype(np.float64) - ref.astype(np.float64))
    print("normalization, device float32 (60, 131) at 51: max relative error %.3g, bound %.3g" % ((err / np.abs(ref))[ok].max(), rtol))
    assert np.all(err[ok] <= rtol * np.abs(ref[ok].astype(np.float64)))
