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


# ------------------------------------------------------------------ the data of tests/test_gaussian_edges_gpu.py can see what it is there to see

PLATEAU_SHAPE, PLATEAU_BLOCK = (100, 300), (44, 50)
PLATEAU_SIGMAS = [3, (1, 5.3)]
INTEGER_DTYPES = ["uint8", "int8", "uint16", "int16", "uint32", "int32", "int64", "uint64"]
FLOOR = 32


def differing(a, b):
    return int((a != b).sum())


def test_fused_multiply_add_is_exact():
    """G.fma (error-free product and sum, the small terms added with rounding to odd) against fractions.Fraction: random operands,
    operands whose product cancels against the addend, and sums that fall half-way between two doubles."""
    from fractions import Fraction
    rng = np.random.default_rng(3)
    a, b, c = rng.standard_normal(1500), rng.standard_normal(1500) * 1e-3, rng.standard_normal(1500)
    c[:300] = -(a[:300] * b[:300])
    a[300:600] = rng.integers(1, 1 << 26, 300) * 2.0 + 1.0                 # a b has 54 bits: exactly half-way cases when c = 0 or a power of two
    b[300:600] = rng.integers(1, 1 << 26, 300) * 2.0 + 1.0
    c[300:450], c[450:600] = 0.0, 2.0 ** 60
    got = G.fma(a, b, c)
    for i in range(len(a)):
        assert got[i] == float(Fraction(a[i]) * Fraction(b[i]) + Fraction(c[i])), (i, a[i], b[i], c[i])
    assert differing(got, a * b + c) > 100                                  # and it is not the two-rounding form


def test_plateau_image_is_blocks_of_one_level_with_different_neighbours():
    for dtype in INTEGER_DTYPES + ["float32", "float64"]:
        a = G.plateau_image(PLATEAU_SHAPE, dtype, PLATEAU_BLOCK)
        levels = G.plateau_levels(dtype)
        assert a.dtype == np.dtype(dtype) and a.shape == PLATEAU_SHAPE and not a.flags.writeable
        cells = a.view("u%d" % a.itemsize)
        assert len(np.unique(levels.view(cells.dtype))) == 12 and len(np.unique(cells)) == 12
        for i in range(3):
            for k in range(6):
                blk = cells[44 * i:44 * i + 44, 50 * k:50 * k + 50]
                assert (blk == blk[0, 0]).all()
                if k:
                    assert blk[0, 0] != cells[44 * i, 50 * k - 1]
                if i:
                    assert blk[0, 0] != cells[44 * i - 1, 50 * k]
        if np.dtype(dtype).kind in "iu":
            info = np.iinfo(dtype)
            if np.dtype(dtype).itemsize < 8:
                assert list(levels[:6]) == [info.max, info.min, info.max // 2 + 1, 1 if info.min == 0 else -1, info.max - 1, info.max // 3]
    assert abs(G.plateau_levels("int64").astype(object)).max() <= 2 ** 62 and 2 ** 53 + 1 in G.plateau_levels("int64")
    u = G.plateau_levels("uint64").astype(object)
    assert u.max() == 2 ** 64 - 2 ** 16 and sum(1 for v in u if v > 2 ** 63 and int(float(v)) != v) >= 2      # the read through a double rounds
    assert np.signbit(G.plateau_levels("float32")[4]) and G.plateau_levels("float64")[3] == np.finfo(np.float64).max / 4


@pytest.mark.parametrize("sigma", PLATEAU_SIGMAS, ids=str)
@pytest.mark.parametrize("dtype", INTEGER_DTYPES)
def test_plateaus_see_every_wrong_arithmetic(dtype, sigma):
    """The condition under which the plateau cases of tests/test_gaussian_edges_gpu.py mean something, held on the CPU for every
    (integer type, mode, sigma) of that grid: scipy equals the restatement, and each wrong arithmetic of the restatement differs from
    scipy -- "reversed", "unpaired" and "fused" in at least 32 pixels (a floor that keeps the GPU test from going blind, not a
    measurement), "unrounded_between" and "round_half" somewhere, "cval_cast" somewhere under constant with cval = 1.5.

    Why: on the normal(0, 40) images of tests/test_gaussian_gpu.py (70 x 150, sigma 1 and 3) the three arithmetics change
        uint8, int8, uint16, int16, int32, uint32      reversed 0    unpaired 0    fused 0     pixels
        float32                                        reversed 0    unpaired 0    fused 0
        float64                                        7134-8559     7521-8151     5466-7272
    because an integer result truncates a float64 that lies far from an integer and a float32 one rounds a float64 far from a tie.

    Observed on the (100, 300) plateau image with blocks of 44 x 50, the smallest count over the types of a width and the five modes:
                                  reversed   unpaired   fused   unrounded_between   round_half   cval_cast (constant)
        sigma 3         8-bit         5412       4740    3312                4013        14274                    357
                        16/32-bit     7556       6776    5106                4650        15383                    325
                        64-bit       19026      17266   13148                  68          324                     50
        sigma (1, 5.3)  8-bit         1008       3508       0                1694        12172                    182
                        16/32-bit     1824       2160    1456                1570        12740                    126
                        64-bit       19918      18838   11938                  40          428                      2
    (cval_cast in uint64 lives on the one level below 2^52 that lies on an edge: 1.5 against 1 is lost in the ulp of the others.)
    "fused" at sigma (1, 5.3) is 0 for uint8 and int8 whatever the levels: over a constant line of any of the 256 values neither the pass
    of radius 4 nor the one of radius 21 changes its truncated result when its multiply-adds are fused, and only a constant line brings
    the sum close to an integer.  That case asserts this fact instead of the floor (all 256 levels), so that it is noticed should it
    stop being one; the same instantiations see "fused" at sigma 3, through the same tap loop."""
    a = G.plateau_image(PLATEAU_SHAPE, dtype, PLATEAU_BLOCK)
    blind = np.dtype(dtype).itemsize == 1 and sigma == (1, 5.3)
    for mode in MODES:
        ref = ndi.gaussian_filter(a, sigma, mode=mode, cval=1.5)
        assert np.array_equal(G.gaussian_filter(a, sigma, mode=mode, cval=1.5), ref), mode
        counts = {ar: differing(G.gaussian_filter(a, sigma, mode=mode, cval=1.5, arithmetic=ar), ref) for ar in G.ARITHMETICS[1:]}
        print(dtype, sigma, mode, counts)
        for ar in ("reversed", "unpaired") + (() if blind else ("fused",)):
            assert counts[ar] >= FLOOR, (mode, ar, counts)
        assert counts["unrounded_between"] >= 1 and counts["round_half"] >= 1, (mode, counts)
        if mode == "constant":
            assert counts["cval_cast"] >= 1, counts
        else:
            assert counts["cval_cast"] == 0
    if blind:
        info = np.iinfo(dtype)
        lines = np.arange(info.min, info.max + 1).astype(dtype).reshape(256, 1)         # 256 constant lines under "nearest"
        out = {}
        for ar in ("scipy", "fused", "reversed"):
            first = G.correlate_sym_1d(lines, G.gaussian_weights(1), 1, "nearest", arithmetic=ar)
            out[ar] = G.correlate_sym_1d(first, G.gaussian_weights(5.3), 1, "nearest", arithmetic=ar)
        assert differing(out["fused"], out["scipy"]) == 0 and differing(out["reversed"], out["scipy"]) > 20


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_restatement_equals_scipy_on_float_plateaus_to_the_byte(dtype):
    a = G.plateau_image(PLATEAU_SHAPE, dtype, PLATEAU_BLOCK)
    for sigma in PLATEAU_SIGMAS:
        for mode in MODES:
            ref = ndi.gaussian_filter(a, sigma, mode=mode, cval=1.5)
            assert ref.tobytes() == G.gaussian_filter(a, sigma, mode=mode, cval=1.5).tobytes(), (sigma, mode)
            assert np.isfinite(ref).all()
    ref = ndi.gaussian_filter(a, 3)
    assert np.signbit(ref[ref == 0]).any(), "no -0.0 comes out of the -0.0 plateau"
    if dtype == "float64":
        assert differing(G.gaussian_filter(a, 3, arithmetic="reversed"), ref) >= FLOOR


def kinds_of(out):
    tiny = np.finfo(out.dtype).tiny
    finite = np.isfinite(out)
    return {"nan": int(np.isnan(out).sum()), "+inf": int((out == np.inf).sum()), "-inf": int((out == -np.inf).sum()),
            "subnormal": int((finite & (out != 0) & (np.abs(out) < tiny)).sum()), "-0.0": int(((out == 0) & np.signbit(out)).sum()),
            "normal": int((finite & (np.abs(out) >= tiny)).sum())}


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_special_float_inputs_are_scipys_and_yield_every_kind_of_output(dtype):
    """The inputs of the special-value cases of tests/test_gaussian_edges_gpu.py: scipy and the restatement have NaN at the same
    positions and equal bytes everywhere else, and scipy alone returns at least one NaN, +inf, -inf, subnormal, -0.0 and finite
    normal value from G.special_image under every mode -- a condition on the inputs, so that the GPU cases compare what they name."""
    a = G.special_image(dtype)
    with np.errstate(all="ignore"):
        for mode in MODES:
            ref = ndi.gaussian_filter(a, 3, mode=mode, cval=1.5)
            assert G.same_but_for_nan_bits(G.gaussian_filter(a, 3, mode=mode, cval=1.5), ref), mode
            kinds = kinds_of(ref)
            assert min(kinds.values()) >= 1, (mode, kinds)
        zeros = np.full((40, 70), -0.0, dtype)
        ref = ndi.gaussian_filter(zeros, 3)
        assert G.same_but_for_nan_bits(G.gaussian_filter(zeros, 3), ref) and np.signbit(ref).all() and not ref.any()
        tiny = G.tiny_image(dtype)
        for mode in ("reflect", "constant"):
            ref = ndi.gaussian_filter(tiny, 3, mode=mode, cval=0.0)
            assert G.same_but_for_nan_bits(G.gaussian_filter(tiny, 3, mode=mode, cval=0.0), ref)
            assert kinds_of(ref)["subnormal"] == ref.size == 2800
        plain = image((40, 70), dtype)
        for cval in (np.inf, np.nan, -1e300, 1e40):
            ref = ndi.gaussian_filter(plain, 3, mode="constant", cval=cval)
            assert G.same_but_for_nan_bits(G.gaussian_filter(plain, 3, mode="constant", cval=cval), ref), cval
            assert not np.isfinite(ref[0, 0]) or dtype == "float64"
    assert not G.same_but_for_nan_bits(np.array([0.0, np.nan], dtype), np.array([-0.0, np.nan], dtype))
    assert G.same_but_for_nan_bits(np.array([-0.0, np.nan], dtype), np.array([-0.0, -np.nan], dtype))
