"""The NumPy restatement of scipy's Gaussian filter (tests/helpers/gaussian_reference.py: the arithmetic contract of
dcp_correlate_sym_2d) is np.array_equal to scipy.ndimage.gaussian_filter: six element types, seven shapes from 1 x 1 to 57 x 153,
sigma 0.5 / 1 / 3 / 5.3 and three pairs, the five boundary modes with cval = 1.5.  No GPU."""
import numpy as np
import pytest
from scipy import ndimage as ndi

from helpers import gaussian_reference as G

SHAPES = [(1, 1), (1, 7), (5, 5), (3, 40), (2, 300), (33, 129), (57, 153)]
SIGMAS = [0.5, 1, 3, 5.3, (3, 0), (0, 3), (1, 5.3)]
MODES = ["reflect", "nearest", "mirror", "wrap", "constant"]
DTYPES = ["float32", "float64", "uint8", "int16", "uint16", "int32"]


def image(shape, dtype):
    """Standard normal scaled by 40 (plus 128 for unsigned types), clipped into the type's range."""
    rng = np.random.default_rng(1000 * shape[0] + shape[1])
    dt = np.dtype(dtype)
    a = rng.standard_normal(shape) * 40.0
    if dt.kind in "iu":
        info = np.iinfo(dt)
        a = np.clip(a + (128.0 if dt.kind == "u" else 0.0), info.min, info.max)
    return a.astype(dt)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_restatement_equals_scipy(shape, dtype):
    a = image(shape, dtype)
    for sigma in SIGMAS:
        for mode in MODES:
            ref = ndi.gaussian_filter(a, sigma, mode=mode, cval=1.5)
            got = G.gaussian_filter(a, sigma, mode=mode, cval=1.5)
            assert got.dtype == ref.dtype and np.array_equal(got, ref), (sigma, mode)


def test_aliases_truncate_and_radius():
    a = image((33, 129), "float32")
    for alias, mode in G.ALIASES.items():
        assert np.array_equal(G.gaussian_filter(a, 3, mode=alias, cval=1.5), ndi.gaussian_filter(a, 3, mode=mode, cval=1.5))
    assert np.array_equal(G.gaussian_filter(a, 2, truncate=2.5), ndi.gaussian_filter(a, 2, truncate=2.5))
    assert np.array_equal(G.gaussian_filter(a, 2, radius=(3, 9)), ndi.gaussian_filter(a, 2, radius=(3, 9)))


def test_weights_are_scipys_and_symmetric_to_the_bit():
    for sigma in (0.5, 1, 3, 5.3, 10):
        w = G.gaussian_weights(sigma)
        r = len(w) // 2
        assert r == int(4.0 * sigma + 0.5) and w.dtype == np.float64
        assert w.tobytes() == w[::-1].tobytes()
        delta = np.zeros(4 * r + 1)
        delta[2 * r] = 1.0
        assert np.array_equal(ndi.gaussian_filter1d(delta, sigma)[r:3 * r + 1], w)


def test_extension_folds_any_number_of_times():
    p = np.arange(-9, 12)
    assert list(G.extend_index(p, 3, "reflect")) == [2, 1, 0, 0, 1, 2, 2, 1, 0, 0, 1, 2, 2, 1, 0, 0, 1, 2, 2, 1, 0]
    assert list(G.extend_index(p, 3, "mirror")) == [1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1]
    assert list(G.extend_index(p, 3, "wrap")) == [0, 1, 2] * 7
    assert list(G.extend_index(p, 1, "mirror")) == [0] * 21
    assert list(G.extend_index(np.arange(-2, 5), 3, "constant")) == [-1, -1, 0, 1, 2, -1, -1]
