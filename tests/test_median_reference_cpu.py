"""CPU checks of the median filter's independent reference (tests/helpers/median_reference.py), the checker of
tests/test_median_tiles_gpu.py: it equals scipy where scipy reflects correctly, it equals a literal Python loop on the shapes where
the window folds many times over the image and on floats with infinities, subnormals, zeros of both signs and NaNs, and its
restatement of the launcher's tile choice, fed with the constants read from csrc/median_kernels.hip, reproduces the tables the GPU
tests expect kernel names from."""
import os
import re
import sys

import numpy as np
import pytest
from scipy import ndimage as ndi

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import median_reference as mr  # noqa: E402

# the pairs of test_median_gpu.py's PAIRS that take scipy well under a second here ((64, 64) at 101 is left out)
SCIPY_PAIRS = [((1, 1), 51), ((1, 1), (2, 2)), ((7, 5), (2, 2)), ((33, 65), (2, 2)), ((17, 130), 3), ((40, 70), (9, 5)), ((40, 70), (4, 6)),
               ((9, 200), 15), ((26, 26), 51), ((50, 50), 51), ((25, 90), 51), ((60, 131), 51), ((70, 300), (1, 51)),
               ((300, 70), (51, 1)), ((17, 65), 3)]
# test_median_tiles_gpu.py's shapes on which the window folds more than once
FOLDS = [((3, 40), 31), ((5, 7), 51), ((2, 3), 51), ((1, 5), (1, 51)), ((4, 1), (9, 1)), ((2, 2), 171), ((3, 3), (2, 2))]


def _seed(*key):
    """The same seed in every process (hash() of a string is not)."""
    return sum(ord(c) * (i + 1) for i, c in enumerate(repr(key))) % (1 << 31)


def _id(v):
    return "x".join(str(s) for s in v) if isinstance(v, tuple) else str(v)


def _draws(shape, dtype):
    """Distinct-ish values without NaNs or zeros: every correct selection returns the same bytes."""
    rng = np.random.default_rng(_seed(shape, dtype))
    dt = np.dtype(dtype)
    if dt.kind == "f":
        return rng.standard_normal(shape).astype(dt)
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max, size=shape, endpoint=True, dtype=dt)


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("dtype", ["float32", "uint8"])
@pytest.mark.parametrize("shape,size", SCIPY_PAIRS, ids=["%s-%s" % (_id(s), _id(k)) for s, k in SCIPY_PAIRS])
def test_reference_equals_scipy_where_scipy_reflects_correctly(shape, size, dtype):
    a = _draws(shape, dtype)
    assert same_bytes(mr.median_reference(a, size), ndi.median_filter(a, size, mode="reflect"))


@pytest.mark.parametrize("shape,size", [((40, 70), (9, 5)), ((7, 5), (2, 2)), ((22, 23), 171), ((14, 15), 111)],
                         ids=["40x70-9x5", "7x5-2x2", "22x23-171", "14x15-111"])
def test_reference_equals_scipy_on_every_width_of_float(shape, size):
    """The last two: the smallest frames on which scipy still reflects correctly at those sizes (size // 2 < 4 * side); they check
    the index rule over several folds, not a pixel count."""
    for dtype in ("float32", "float64"):
        a = _draws(shape, dtype)
        assert same_bytes(mr.median_reference(a, size), ndi.median_filter(a, size, mode="reflect")), dtype


@pytest.mark.parametrize("shape,size", [((3, 40), 31), ((5, 7), 51)], ids=["3x40-31", "5x7-51"])
def test_scipy_is_no_reference_beyond_four_sides(shape, size):
    """Why the GPU tests need this helper: the module docstring of prep/preprocessing.py names these as cases scipy gets wrong."""
    a = _draws(shape, "float32")
    assert not np.array_equal(mr.median_reference(a, size), ndi.median_filter(a, size, mode="reflect"))


@pytest.mark.parametrize("dtype", ["float32", "uint16", "float64", "int64", "bool"])
@pytest.mark.parametrize("shape,size", FOLDS, ids=["%s-%s" % (_id(s), _id(k)) for s, k in FOLDS])
def test_reference_equals_the_loop_where_the_window_folds_many_times(shape, size, dtype):
    a = _draws(shape, dtype) if dtype != "bool" else np.random.default_rng(_seed(shape, size)).random(shape) < 0.5
    assert same_bytes(mr.median_reference(a, size), mr.median_loop(a, size))


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_reference_equals_the_loop_on_special_floats(dtype):
    """Infinities, the largest finite values, subnormals, zeros of both signs, NaNs of both signs: the total order, bit for bit."""
    edge = mr.edge_image(dtype, (9, 12), _seed("edge", dtype))
    signs = set()
    for size in (3, (2, 2), (9, 5)):
        ref = mr.median_reference(edge, size)
        assert same_bytes(ref, mr.median_loop(edge, size)), size
        signs |= {bool(s) for s in np.signbit(ref[ref == 0])}
    assert signs == {False, True}                        # zeros of both signs come out: the byte comparison sees their order
    nans, mask = mr.nan_image(dtype, (21, 70), _seed("nan", dtype))
    part, pmask = nans[2:14, 5:35], mask[2:14, 5:35]     # holds the block of positive NaNs and a lone negative one
    assert pmask.sum() == 10
    for size in (3, (2, 2), (9, 5)):
        ref = mr.median_reference(part, size)
        assert same_bytes(ref, mr.median_loop(part, size)), size
    assert np.isnan(mr.median_reference(part, 3)).sum() >= 1     # the centre of the block: a NaN is selected, payload and all


def test_total_order_of_the_keys():
    for dtype in ("float32", "float64"):
        dt = np.dtype(dtype)
        info = np.finfo(dt)
        u = np.dtype("u%d" % dt.itemsize)
        top = dt.itemsize * 8 - 1
        expo = ((1 << (top - info.nmant)) - 1) << info.nmant
        pos_nans = np.array([expo | 1, expo | (1 << (info.nmant - 1)), expo | ((1 << info.nmant) - 1)], u)
        neg_nans = (pos_nans | u.type(1 << top))[::-1]
        finite = np.array([-np.inf, -info.max, -1.0, -info.smallest_subnormal, -0.0, 0.0, info.smallest_subnormal, 1.0, info.max, np.inf], dt)
        ordered = np.concatenate([neg_nans.view(dt), finite, pos_nans.view(dt)])
        keys, back = mr.total_order_keys(ordered)
        assert np.all(np.diff(keys.astype(object)) > 0), dtype
        assert back(keys).tobytes() == ordered.tobytes()


def test_sixty_four_bit_integers_stay_in_their_type():
    for dt in (np.int64, np.uint64):
        info = np.iinfo(dt)
        a = np.full((3, 5), info.max - 2, dt)
        a[1, :] = info.max - np.arange(5).astype(dt)     # neighbours that one double cannot tell apart
        ref = mr.median_reference(a, (1, 3))
        assert ref.dtype == a.dtype and same_bytes(ref, mr.median_loop(a, (1, 3)))
        assert ref[1, 2] == info.max - 2 and ref[1, 1] == info.max - 1


# ---------------------------------------------------------------------------------------------- the launcher's choice of a tile

def source_constants():
    """kMedianTW, the two LDS caps and the tile heights as csrc/median_kernels.hip states them."""
    text = open(os.path.join(ROOT, "discorpy_amd", "csrc", "median_kernels.hip")).read()
    tw = int(re.search(r"constexpr int kMedianTW = (\d+);", text).group(1))
    caps = re.search(r"kMedianLdsPlain = (\d+)u << (\d+), kMedianLdsMax = (\d+)u << (\d+);", text)
    plain, most = int(caps.group(1)) << int(caps.group(2)), int(caps.group(3)) << int(caps.group(4))
    heights = tuple(int(v) for v in re.search(r"for \(int th : \{([\d, ]+)\}\)", text).group(1).split(","))
    assert re.search(r"for \(size_t cap : \{kMedianLdsPlain, kMedianLdsMax\}\)\s*for \(int th :", text), "the chooser's loop order changed"
    return tw, (plain, most), heights


def test_helper_constants_are_the_sources():
    tw, caps, heights = source_constants()
    assert (tw, caps, heights) == (mr.TILE_WIDTH, (mr.LDS_PLAIN, mr.LDS_MAX), mr.TILE_HEIGHTS)


@pytest.mark.parametrize("key_bytes", [4, 8])
def test_chooser_table_follows_from_the_constants(key_bytes):
    tw, caps, heights = source_constants()

    def choice(s):
        return mr.tile_rows(s, s, key_bytes, caps, tw, heights)

    names = ["64 KiB", "160 KiB"]
    for th, cap, lo, hi in mr.CHOOSER_TABLE[key_bytes]:
        row = "%d-byte keys, %s: sizes %s-%s" % (key_bytes, "TH%d under %s" % (th, names[cap]) if th else "global kernel", lo, hi or "")
        for s in range(lo, (hi or lo + 400) + 1):
            assert choice(s) == (th, cap), "row moved: %s (size %d now takes %s)" % (row, s, choice(s))
    rows = mr.CHOOSER_TABLE[key_bytes]
    assert rows[0][2] == 1 and all(b[2] == a[3] + 1 for a, b in zip(rows, rows[1:]))          # the rows cover every size once
    # the GPU tests' sizes sit on both sides of every boundary and expect what the rows say
    edges = sorted({s for th, cap, lo, hi in rows for s in (lo, hi) if s not in (1, None)})
    assert [s for s, _ in mr.BOUNDARY_SIZES[key_bytes]] == edges
    for s, th in mr.BOUNDARY_SIZES[key_bytes]:
        assert choice(s)[0] == th, "size %d at %d-byte keys: tile height %d expected, %d chosen" % (s, key_bytes, th, choice(s)[0])
    s, nbytes = mr.LARGEST_BOX[key_bytes]
    assert mr.box_bytes(4, s, s, key_bytes, tw) == nbytes <= caps[1] == 163840 and choice(s) == (4, 1) and choice(s + 1) == (0, None)


def test_non_square_windows_take_the_tile_the_formula_gives():
    tw, caps, heights = source_constants()
    for key_bytes, (sy, sx), th, cap in mr.NONSQUARE:
        assert mr.tile_rows(sy, sx, key_bytes, caps, tw, heights) == (th, cap), (key_bytes, sy, sx)
    assert {(k, cap) for k, _, _, cap in mr.NONSQUARE} == {(4, 0), (4, 1), (8, 0), (8, 1)}
    assert mr.box_bytes(16, 301, 1, 8) == 161792 and mr.box_bytes(8, 100, 90, 4) == 65484 < 65536 < mr.box_bytes(16, 100, 90, 4)


def test_kernel_names():
    assert mr.kernel_name(32, 16) == "median_lds_kernel<bits=32, tile=64x16>"
    assert mr.kernel_name(64, 4) == "median_lds_kernel<bits=64, tile=64x4>"
    assert mr.kernel_name(8, 0) == "median_global_kernel<bits=8>"
    text = open(os.path.join(ROOT, "discorpy_amd", "csrc", "median_kernels.hip")).read()
    assert '"median_lds_kernel<bits=%d, tile=%dx%d>"' in text and '"median_global_kernel<bits=%d>"' in text
