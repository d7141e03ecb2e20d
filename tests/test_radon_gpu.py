"""GPU suite for the Radon transform of discorpy_amd.prep.linepattern (csrc/radon_kernels.hip: radon_kernel, through dcp_radon_2d) against
the NumPy restatement of its definition, tests/helpers/radon_reference.py, which tests/test_radon_cpu.py holds to facts checked by hand.
Everything is compared bit for bit: the kernel and the restatement are the same sequence of IEEE operations.

* sides 1, 2, 3, 5 (both parities of the centre, a circle of one element), 63, 64, 65 (the edge of a wave) at the axis angles, 45, -30 and
  359.95 degree and the two fine grids of the slope search (around 0 and around 90 degree); 257 (five waves per angle, the last one
  partial) with 1, 3 and 61 angles; 180 angles by default.  float32 and float64, random data and small integers
* a strided view, non-square images (both parities of the excess on either axis), a tensor on a stream of its own, a device array
* NaN and infinities inside and outside the circle, an all-zero plane, two calls of the same input"""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import radon_reference as RR  # noqa: E402

pytestmark = pytest.mark.gpu

BASE = [0.0, 90.0, 180.0, 270.0, 45.0, -30.0, 359.95]
FINE_0 = np.arange(-1.0, 1.05, 0.05)                  # the reference's fine grid around a best coarse angle of 0 ...
FINE_90 = np.arange(90.0 - 1.0, 90.0 + 1.05, 0.05)    # ... and of 90 degree
ANGLES = np.concatenate([BASE, FINE_0, FINE_90])
COARSE_90 = 90.0 + np.arange(-30.0, 31.0)


@pytest.fixture(scope="module")
def lp(hip):
    from discorpy_amd.prep import linepattern
    return linepattern


@functools.lru_cache(maxsize=None)
def plane(side, dtype, kind, seed=0):
    rng = np.random.default_rng(1000 * side + seed)
    if kind == "integers":
        img = rng.integers(-4, 5, (side, side)).astype(dtype)
    else:
        img = ((rng.random((side, side)) - 0.3) * 10.0 ** rng.integers(-3, 4, (side, side))).astype(dtype)
    img.setflags(write=False)
    return img


def same_bits(got, want):
    return got.shape == want.shape and got.dtype == want.dtype == np.float64 and np.array_equal(got.view(np.uint64), want.view(np.uint64))


@pytest.mark.parametrize("kind", ["random", "integers"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("side", [1, 2, 3, 5, 63, 64, 65])
def test_small_sides_every_angle(lp, side, dtype, kind):
    img = plane(side, dtype, kind)
    got = lp.radon(img, ANGLES)
    assert isinstance(got, np.ndarray) and same_bits(got, RR.radon(img, ANGLES))


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("theta", [[17.3], [0.0, 45.0, 90.0], COARSE_90], ids=["1", "3", "61"])
def test_side_257(lp, theta, dtype):
    img = plane(257, dtype, "random")
    assert same_bits(lp.radon(img, theta), RR.radon(img, theta))


def test_default_theta_is_180_angles(lp):
    img = plane(64, "float32", "random", seed=1)
    got = lp.radon(img)
    assert got.shape == (64, 180) and same_bits(got, RR.radon(img, np.arange(180)))


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_strided_view_is_read_in_place(lp, dtype):
    a = plane(80, dtype, "random", seed=2)
    view = a[3:-5, 7:-1]
    assert view.shape == (72, 72) and not view.flags.c_contiguous
    assert same_bits(lp.radon(view, ANGLES), RR.radon(np.ascontiguousarray(view), ANGLES))


@pytest.mark.parametrize("shape,rows,cols", [((40, 43), slice(0, 40), slice(2, 42)), ((46, 40), slice(3, 43), slice(0, 40)),
                                             ((41, 40), slice(1, 41), slice(0, 40)), ((33, 35), slice(0, 33), slice(1, 34))])
def test_non_square_image_is_cropped_to_the_centred_square(lp, shape, rows, cols):
    img = np.random.default_rng(shape[0]).random(shape).astype(np.float32)
    got = lp.radon(img, BASE)
    assert same_bits(got, RR.radon(np.ascontiguousarray(img[rows, cols]), BASE))
    assert same_bits(got, RR.radon(img, BASE))


def test_tensor_on_its_own_stream(lp):
    import torch
    img = plane(65, "float32", "random", seed=3)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        t = torch.from_numpy(np.array(img)).to("cuda:0")
        got = lp.radon(t, ANGLES)
    stream.synchronize()
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (65, len(ANGLES))
    assert same_bits(got.cpu().numpy(), RR.radon(img, ANGLES))
    # a view of a tensor (the ROI of the slope search is one), and a non-square one
    big = torch.from_numpy(np.array(plane(80, "float64", "random", seed=2))).to("cuda:0")
    assert same_bits(lp.radon(big[3:-5, 7:-1], BASE).cpu().numpy(), RR.radon(plane(80, "float64", "random", seed=2)[3:-5, 7:-1], BASE))
    assert same_bits(lp.radon(big[:, 5:], BASE).cpu().numpy(), RR.radon(plane(80, "float64", "random", seed=2)[:, 5:], BASE))
    empty = lp.radon(t, [])
    assert isinstance(empty, torch.Tensor) and tuple(empty.shape) == (65, 0) and empty.dtype == torch.float64


def test_device_array(lp, hip):
    img = plane(63, "float64", "random", seed=4)
    dev = hip.DeviceArray(img.shape, img.dtype).copy_from_host(img)
    got = lp.radon(dev, ANGLES)
    assert isinstance(got, hip.DeviceArray) and got.shape == (63, len(ANGLES)) and got.dtype == np.float64
    hip.check(hip.lib().dcp_stream_synchronize(-1, None))
    assert same_bits(got.copy_to_host(), RR.radon(img, ANGLES))


def test_nan_and_infinities(lp):
    side, c0 = 33, 16
    clean = np.array(plane(side, "float32", "random", seed=5))
    y, x = np.mgrid[:side, :side]
    inside = (y - c0) ** 2 + (x - c0) ** 2 <= c0 ** 2
    want = RR.radon(clean, ANGLES)
    for value in (np.nan, np.inf, -np.inf):
        outside = clean.copy()
        outside[~inside] = value                               # never read: nothing changes
        assert same_bits(lp.radon(outside, ANGLES), want), value
        within = clean.copy()
        within[10, 20] = value
        got, ref = lp.radon(within, ANGLES), RR.radon(within, ANGLES)
        assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.isnan(ref).any() and not np.isnan(ref).all(), value
        assert np.array_equal(got, ref, equal_nan=True), value
        assert np.array_equal(got[~np.isnan(ref)].view(np.uint64), ref[~np.isnan(ref)].view(np.uint64)), value
    zeros = lp.radon(np.zeros((side, side), np.float64), ANGLES)
    assert zeros.shape == (side, len(ANGLES)) and not zeros.view(np.uint64).any()        # +0.0 everywhere


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_two_calls_give_the_same_bits(lp, dtype):
    img = plane(257, dtype, "random", seed=6)
    first, second = lp.radon(img, COARSE_90), lp.radon(img, COARSE_90)
    assert first is not second and same_bits(first, second)
