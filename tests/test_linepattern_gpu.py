"""GPU suite for discorpy_amd.prep.linepattern beyond the Gaussian itself: convert_chessboard_to_linepattern and get_tilted_profile
against the reference's lines (discorpy/prep/linepattern.py:512-601) restated with scipy -- the reference's module cannot be imported
without scikit-image."""
import numpy as np
import pytest
from scipy import ndimage as ndi

pytestmark = pytest.mark.gpu

# largest deviation of the tensor path from the host path by result type, measured on an MI355X: see test_chessboard_of_a_device_tensor
TENSOR_PATH_MEASURED = {"float32": 1.35e-7, "float64": 1.24e-16}


def chessboard(dtype):
    """96 x 120, squares of 12 pixels under a smooth illumination gradient and a little noise."""
    rng = np.random.default_rng(3)
    yy, xx = np.mgrid[0:96, 0:120]
    board = ((yy // 12 + xx // 12) % 2).astype(np.float64)
    img = (0.2 + 0.6 * board) * np.linspace(0.8, 1.2, 120) + rng.normal(0.0, 0.01, (96, 120))
    dt = np.dtype(dtype)
    return img.astype(dt) if dt.kind == "f" else np.clip(img * 40000.0, 0, np.iinfo(dt).max).astype(dt)


def reference_convert(mat, smooth=True, bgr="bright", sigma=3):
    """linepattern.py:591-601 with scipy's filter."""
    if smooth is True:
        mat = ndi.gaussian_filter(mat, sigma, mode="nearest")
    mat_line = np.mean(np.abs(np.gradient(mat)), axis=0)
    if smooth is True:
        mat_line = np.pad(mat_line[4:-4, 4:-4], 4, mode="edge")
    else:
        mat_line = np.pad(mat_line[2:-2, 2:-2], 2, mode="edge")
    if bgr == "bright":
        mat_line = np.max(mat_line) - mat_line
    return mat_line / np.mean(np.abs(mat_line))


def reference_profile_inputs(shape, index, angle_deg, direction):
    """linepattern.py:541-564: (xlist, ylist, band slice, coordinates inside the band)."""
    height, width = shape
    angle = angle_deg * np.pi / 180.0
    if direction == "horizontal":
        rlist = np.linspace(0, np.floor(width / np.cos(angle)), width)
        xlist = np.clip(rlist * np.cos(angle), 0, width - 1)
        ylist = np.clip(index + rlist * np.sin(-angle), 0, height - 1)
        ymin, ymax = int(np.floor(np.amin(ylist))), int(np.ceil(np.amax(ylist))) + 1
        return xlist, ylist, (slice(ymin, ymax), slice(None)), (ylist - ymin, xlist)
    rlist = np.linspace(0, np.floor(height / np.cos(angle)), height)
    ylist = np.clip(rlist * np.cos(angle), 0, height - 1)
    xlist = np.clip(index + rlist * np.sin(angle), 0, width - 1)
    xmin, xmax = int(np.floor(np.amin(xlist))), int(np.ceil(np.amax(xlist))) + 1
    return xlist, ylist, (slice(None), slice(xmin, xmax)), (ylist, xlist - xmin)


@pytest.fixture(scope="module")
def lp(hip):
    from discorpy_amd.prep import linepattern
    return linepattern


@pytest.mark.parametrize("dtype", ["float32", "uint16", "float64"])
@pytest.mark.parametrize("bgr", ["bright", "dark"])
@pytest.mark.parametrize("smooth", [True, False])
def test_chessboard_of_a_host_array_is_the_reference_bit_for_bit(lp, smooth, bgr, dtype):
    mat = chessboard(dtype)
    got, ref = lp.convert_chessboard_to_linepattern(mat, smooth, bgr), reference_convert(mat, smooth, bgr)
    assert got.dtype == ref.dtype and got.shape == ref.shape == (96, 120)
    assert np.array_equal(got, ref)
    if smooth:
        assert np.array_equal(lp.convert_chessboard_to_linepattern(mat, bgr=bgr, sigma=2), reference_convert(mat, bgr=bgr, sigma=2))


@pytest.mark.parametrize("dtype", ["float32", "uint16"])
@pytest.mark.parametrize("bgr", ["bright", "dark"])
@pytest.mark.parametrize("smooth", [True, False])
def test_chessboard_of_a_device_tensor(lp, smooth, bgr, dtype):
    """The tensor path runs the reference's steps with torch on the device.  Its Gaussian is the same kernel (equal bits), gradient, crop
    and pad are exact or single roundings of the same operands; the mean that everything is divided by is a reduction in another order.
    Deviation = max |tensor - host| / max |host| over the image.  Measured on these eight images (MI355X): float32 results 0, 1.35e-7,
    1.03e-7, 0 (smooth bright, smooth dark, plain bright, plain dark), float64 results (uint16 input) 0, 0, 0, 1.24e-16 -- about one
    unit in the last place of the result type.  Allowed: four times the largest figure of the result type (TENSOR_PATH_MEASURED)."""
    torch = pytest.importorskip("torch")
    mat = chessboard(dtype)
    host = lp.convert_chessboard_to_linepattern(mat, smooth, bgr)
    t = torch.from_numpy(mat).to("cuda:0")
    got = lp.convert_chessboard_to_linepattern(t, smooth, bgr)
    torch.cuda.synchronize()
    assert isinstance(got, torch.Tensor) and got.device == t.device and tuple(got.shape) == (96, 120)
    assert str(got.dtype).replace("torch.", "") == host.dtype.name
    dev = np.max(np.abs(got.cpu().numpy().astype(np.float64) - host.astype(np.float64))) / np.max(np.abs(host))
    print("convert_chessboard_to_linepattern tensor path, %s smooth=%s bgr=%s: relative deviation %.3g" % (dtype, smooth, bgr, dev))
    assert dev <= 4 * TENSOR_PATH_MEASURED[host.dtype.name]


PROFILE_CASES = [(direction, angle) for direction in ("horizontal", "vertical") for angle in (3.0, -3.0, 0.0)]


@pytest.mark.parametrize("direction,angle", PROFILE_CASES, ids=["%s%+g" % c for c in PROFILE_CASES])
def test_tilted_profile(lp, orc, direction, angle):
    """First and last admissible index.  xlist / ylist are the reference's, bit for bit.  The profile is scipy's map_coordinates on the
    reference's band within what tests/test_gpu_parity.py allows remap_coordinates at order 3: float32 (image in [0, 1)) at most 2
    points different and none by more than 1e-6; uint16 equal to the oracle's map_coordinates (itself held to scipy on the CPU)."""
    rng = np.random.default_rng(17)
    f32 = rng.random((96, 120), dtype=np.float32)
    u16 = (f32 * 60000).astype(np.uint16)
    lo, hi = lp._calc_index_range(96, 120, angle, direction)
    assert 0 <= lo < hi
    for index in (lo, hi):
        xref, yref, band, coords = reference_profile_inputs((96, 120), index, angle, direction)
        xlist, ylist, profile = lp.get_tilted_profile(f32, index, angle, direction)
        assert np.array_equal(xlist, xref) and np.array_equal(ylist, yref)
        ref = ndi.map_coordinates(f32[band], coords, order=3, mode="nearest")
        assert profile.dtype == np.float32 and profile.shape == ref.shape == xlist.shape
        assert np.count_nonzero(profile != ref) <= 2 and np.max(np.abs(profile - ref)) <= 1e-6, (index, np.max(np.abs(profile - ref)))
        xlist, ylist, profile = lp.get_tilted_profile(u16, index, angle, direction)
        assert np.array_equal(xlist, xref) and np.array_equal(ylist, yref)
        assert profile.dtype == np.uint16
        assert np.array_equal(profile, orc.map_coordinates(np.ascontiguousarray(u16[band]), coords[0], coords[1], 3, "nearest")), index


def test_tilted_profile_of_a_device_tensor(lp):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(17)
    f32 = rng.random((96, 120), dtype=np.float32)
    t = torch.from_numpy(f32).to("cuda:0")
    for direction, index in (("horizontal", 40), ("vertical", 50)):
        xh, yh, ph = lp.get_tilted_profile(f32, index, 3.0, direction)
        xt, yt, pt = lp.get_tilted_profile(t, index, 3.0, direction)
        torch.cuda.synchronize()
        assert isinstance(pt, torch.Tensor) and np.array_equal(xt, xh) and np.array_equal(yt, yh)
        assert np.max(np.abs(pt.cpu().numpy() - ph)) <= 1e-6
