"""GPU suite for the binarization kernels (csrc/binarize_kernels.hip) at the sizes and addresses where their loops turn that one
3 x 4-tile frame never turns (tests/test_binarize_gpu.py covers the tiles' own edges).  Every comparison is exact, as there.

LARGE (tests/helpers/label_cases.py; its conditions are asserted against the kernels' constants by tests/test_binarize_cpu.py) has
2 540 209 elements: minmax_kernel and histogram_kernel run at their cap of 1024 workgroups, a thread walks ten rounds, and the tenth
is ragged -- workgroups 0 to 705 read a whole block in it, workgroup 706 reads 177 elements, the others nothing.  minmax_final_kernel
folds 1024 triples in four rounds over four waves.  The float histogram runs at 1, 2 and 3 bins, at its documented LDS maximum (4096
bins of float64 edges) and on the far side of the switch; the threshold kernel writes into a dst that is not aligned to four bytes."""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import binarize_reference as bref  # noqa: E402
import label_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu

TH, TW, BIG, LARGE = bref.TH, bref.TW, bref.SHAPES[-1], bref.LARGE
SWITCH = bref.HIST_LDS_MAX_BINS
N = LARGE[0] * LARGE[1]
CAP, BLOCK = bref.REDUCE_MAX_BLOCKS, bref.BIN_BLOCK          # kReduceMaxBlocks, kBinBlock (pinned by tests/test_binarize_cpu.py)
LAST_ROUND = 9 * CAP * BLOCK                 # the first element that only the ragged tenth round reads
# flat indices from the launch geometry: the last element (workgroup 706, cut short), the first element of the last workgroup, one of
# the tenth round (workgroup 300, wave 2), the first element
PLANTS = (N - 1, (CAP - 1) * BLOCK, LAST_ROUND + 300 * BLOCK + 129, 0)
assert LAST_ROUND < PLANTS[2] < N and (N - LAST_ROUND) // BLOCK == 706 and (N - LAST_ROUND) % BLOCK == 177


@pytest.fixture(scope="module")
def prep(hip):
    from discorpy_amd.prep import preprocessing
    return preprocessing


def _option(hip, key, value):
    old = hip.get_option(key)
    hip.set_option(key, value)
    try:
        yield value
    finally:
        hip.set_option(key, old)


@pytest.fixture(params=[1, 0], ids=["hist_lds", "hist_global"])
def hist_lds(request, hip):
    yield from _option(hip, "x_hist_lds", request.param)


@pytest.fixture(params=[1, 0], ids=["fused", "two_launches"])
def fused(request, hip):
    yield from _option(hip, "x_morph_fused", request.param)


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _same_or_both_nan(a, b):
    return a == b or (np.isnan(a) and np.isnan(b))


# ---------------------------------------------------------------------------------------------- minimum, maximum, non-finite count

def narrow_plane(dtype, shape=LARGE, seed=40):
    """Values of a narrow range in the middle of the type's, so that one planted element is the only extreme."""
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype)
    if dt.kind == "f":
        return rng.uniform(2.0, 3.0, shape).astype(dt)
    mid = (int(np.iinfo(dt).max) + int(np.iinfo(dt).min)) // 2
    return rng.integers(mid - 20, mid + 21, shape).astype(dt)


def extremes_of(dtype):
    dt = np.dtype(dtype)
    return (dt.type(-1.0e30), dt.type(1.0e30)) if dt.kind == "f" else (np.iinfo(dt).min, np.iinfo(dt).max)


def check_minmax(prep, a, src=None):
    lo, hi, bad = prep._minmax(prep._rows_image(a if src is None else src))
    with np.errstate(all="ignore"):
        want_lo, want_hi = float(a.min()), float(a.max())
    assert bad == int((~np.isfinite(a.astype(np.float64))).sum()), bad
    assert _same_or_both_nan(lo, want_lo) and _same_or_both_nan(hi, want_hi), (lo, hi, want_lo, want_hi)


@pytest.mark.parametrize("dtype", bref.HIST_DTYPES)
def test_one_planted_extreme_in_every_region_of_the_capped_grid(prep, hip, dtype):
    a = narrow_plane(dtype)
    flat = a.reshape(-1)
    inner_lo, inner_hi = a.min(), a.max()
    check_minmax(prep, a)
    assert hip.last_kernel() == "minmax_kernel + minmax_final_kernel"
    for position in PLANTS:
        for value in extremes_of(dtype):
            keep = flat[position]
            flat[position] = value
            assert (a.min(), a.max()) in ((value, inner_hi), (inner_lo, value))
            check_minmax(prep, a)
            flat[position] = keep
    assert (a.min(), a.max()) == (inner_lo, inner_hi)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_non_finite_elements_are_counted_exactly_across_the_capped_grid(prep, dtype):
    a = narrow_plane(dtype, seed=41)
    flat = a.reshape(-1)
    rng = np.random.default_rng(42)
    where = np.unique(np.concatenate([rng.choice(N, 3001 - len(PLANTS), replace=False), PLANTS]))
    where = np.concatenate([where, np.setdiff1d(np.arange(N - 64, N - 1), where)[:3001 - len(where)]])
    assert len(np.unique(where)) == 3001 and all(p in where for p in PLANTS)
    kinds = np.array([np.inf, -np.inf], a.dtype)
    flat[where] = kinds[rng.integers(0, 2, len(where))]
    assert (a.min(), a.max()) == (-np.inf, np.inf)
    check_minmax(prep, a)                                      # infinities only: the extremes are theirs, the count is 3001
    flat[where] = np.array([np.nan, np.inf, -np.inf], a.dtype)[rng.integers(0, 3, len(where))]
    flat[list(PLANTS)] = (np.nan, np.inf, np.nan, -np.inf)
    assert int((~np.isfinite(a)).sum()) == 3001 and np.isnan(a.min())
    check_minmax(prep, a)
    lo, hi, bad = prep._minmax(prep._rows_image(a))
    assert bad == 3001 and np.isnan(lo) and np.isnan(hi)


@pytest.mark.parametrize("dtype", ["float32", "int16"])
def test_planted_extremes_of_a_strided_view_of_a_padded_plane(prep, dtype):
    import torch
    lo_v, hi_v = extremes_of(dtype)
    a = narrow_plane(dtype, seed=43)
    base = np.ascontiguousarray(np.pad(a, ((0, 0), (3, 5)), constant_values=hi_v))          # the padding would win either way
    base[:, :3] = lo_v
    view = base[:, 3:-5]
    assert not view.flags.c_contiguous and view.shape == LARGE
    t = torch.from_numpy(base).to("cuda:0")
    for position, value in ((PLANTS[0], hi_v), (PLANTS[1], lo_v), (PLANTS[2], hi_v), (PLANTS[3], lo_v)):
        y, x = divmod(position, LARGE[1])
        keep = view[y, x]
        view[y, x] = value
        t[y, x + 3] = float(value) if np.dtype(dtype).kind == "f" else int(value)
        check_minmax(prep, np.ascontiguousarray(view), view)              # the host's rows are packed on the way up
        check_minmax(prep, np.ascontiguousarray(view), t[:, 3:-5])        # the tensor's are read in place through its stride
        view[y, x] = keep
        t[y, x + 3] = float(keep) if np.dtype(dtype).kind == "f" else int(keep)


# ---------------------------------------------------------------------------------------------- histogram

LO, HI = -3.7, 11.3          # the range of bref.edge_hugging


@functools.lru_cache(maxsize=None)
def np_histogram(dtype, shape, nbins):
    counts, edges = np.histogram(bref.edge_hugging(dtype, shape, nbins), nbins)
    return counts, edges


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_histogram_of_a_large_plane_of_edge_hugging_values(prep, hip, hist_lds, dtype):
    dt = np.dtype(dtype)
    nbins = 512
    a = bref.edge_hugging(dtype, LARGE, nbins)
    want, want_edges = np_histogram(dtype, LARGE, nbins)
    edges = np.linspace(dt.type(LO), dt.type(HI), nbins + 1, dtype=dt)
    assert np.array_equal(want_edges, edges) and want_edges.dtype == dt
    got = prep._histogram(prep._rows_image(a), nbins, edges=edges)
    assert got.dtype == np.int64 and np.array_equal(got, want), int(np.abs(got - want).sum())
    assert got.sum() == N
    assert hip.last_kernel() == "histogram_kernel<edges, bins=512, %s>" % ("lds" if hist_lds else "global")
    # a flat plane whose only outlier is the last element: whole waves on one bin in all ten rounds, one lane of the last on another
    flat = np.full(LARGE, 2.5, dtype)
    flat[-1, -1] = 9.0
    want, edges = np.histogram(flat, nbins)
    got = prep._histogram(prep._rows_image(flat), nbins, edges=edges)
    assert np.array_equal(got, want) and got[0] == N - 1 and got[-1] == 1 and got.sum() == N


@pytest.mark.parametrize("dtype,span", [("uint16", 4096), ("uint16", 65536), ("int8", 256)])
def test_bincount_of_a_large_plane(prep, hip, hist_lds, dtype, span):
    info = np.iinfo(dtype)
    lo = int(info.min) + (int(info.max) - int(info.min) + 1 - span) // 2
    a = np.random.default_rng(44).integers(lo, lo + span, size=LARGE).astype(dtype)
    a.flat[0], a.flat[-1] = lo, lo + span - 1
    a[LARGE[0] // 2, : LARGE[1] // 2] = lo + span // 3          # a flat run: whole waves on one bin
    want = np.bincount(a.ravel().astype(np.int64) - lo, minlength=span)
    got = prep._histogram(prep._rows_image(a), span, first=lo)
    assert np.array_equal(got, want) and got.sum() == N
    assert hip.last_kernel() == "histogram_kernel<bincount, bins=%d, %s>" % (span, "lds" if hist_lds and span <= SWITCH else "global")
    flat = np.full(LARGE, lo + 5, dtype)
    flat[-1, -1] = lo + span - 1
    got = prep._histogram(prep._rows_image(flat), span, first=lo)
    assert got[5] == N - 1 and got[-1] == 1 and got.sum() == N


@pytest.mark.parametrize("nbins", [1, 2, 3, SWITCH - 1, SWITCH, SWITCH + 1, 65536])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_float_histogram_from_one_bin_to_both_sides_of_the_lds_switch(prep, hip, hist_lds, dtype, nbins):
    """edge_bin's search at 1, 2 and 3 edges' worth of bins (3 is no power of two); 4096 bins of float64 edges are the largest LDS layout
    the kernel documents (4097 * 8 + 4096 * 4 bytes); from 4097 bins the edges are searched in global memory."""
    dt = np.dtype(dtype)
    a = bref.edge_hugging(dtype, BIG, nbins)
    want, want_edges = np_histogram(dtype, BIG, nbins)
    edges = np.linspace(dt.type(LO), dt.type(HI), nbins + 1, dtype=dt)
    assert np.array_equal(want_edges, edges) and want_edges.dtype == dt
    got = prep._histogram(prep._rows_image(a), nbins, edges=edges)
    assert np.array_equal(got, want), int(np.abs(got - want).sum())
    assert got.sum() == a.size
    assert hip.last_kernel() == "histogram_kernel<edges, bins=%d, %s>" % (nbins, "lds" if hist_lds and nbins <= SWITCH else "global")
    if nbins in (3, SWITCH, SWITCH + 1):
        otsu, want_otsu = prep.threshold_otsu(a, nbins), bref.threshold_otsu(a, nbins)
        assert isinstance(otsu, np.generic) and _same_bits(otsu, want_otsu), (otsu, want_otsu)


# ---------------------------------------------------------------------------------------------- threshold

def threshold_source(dtype, shape, seed):
    """(plane, threshold): values over the whole range of the type (floats: [0, 1)) and the middle of that range."""
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype)
    if dt.kind == "b":
        return rng.random(shape) < 0.5, 0.5
    if dt.kind == "f":
        return rng.random(shape).astype(dt), 0.5
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max, size=shape, endpoint=True, dtype=dt), (float(info.max) + float(info.min)) / 2


@pytest.mark.parametrize("dtype", ["uint8", "float32", "float64"])
def test_threshold_into_a_dst_that_is_not_aligned_to_four_bytes(prep, hip, dtype):
    """dcp_threshold_2d with device pointers: dst lies 0 to 3 bytes past an aligned address inside a larger buffer of 0xAB.  Unaligned,
    the kernel stores byte by byte; whatever it does, the plane and the count are NumPy's and no byte outside the window changes."""
    import torch
    code, front = hip.DTYPE_BY_NAME[dtype], 16
    for k, shape in enumerate(((1, 1), (1, 3), (3, 5), (TH + 1, TW + 1), BIG)):
        a, thres = threshold_source(dtype, shape, 54 + k)
        want = (a > np.float64(thres)).astype(np.uint8)
        flat = want.ravel()
        assert a.size < 3 or list(flat[:4]) != list(flat[:4][::-1]), "the first four bytes read the same backwards"
        src = torch.from_numpy(a).to("cuda:0")
        n = a.size
        for off in (0, 1, 2, 3):
            buf = torch.full((front + n + 16,), 0xAB, dtype=torch.uint8, device="cuda:0")
            count = torch.zeros(1, dtype=torch.int64, device="cuda:0")
            assert buf.data_ptr() % 4 == 0
            torch.cuda.synchronize()
            hip.check(hip.lib().dcp_threshold_2d(src.data_ptr(), buf.data_ptr() + front + off, shape[0], shape[1], shape[1], code, thres,
                                                 count.data_ptr(), hip.MEM_DEVICE, src.device.index, None))
            torch.cuda.synchronize()
            host = buf.cpu().numpy()
            window = host[front + off:front + off + n].reshape(shape)
            assert np.array_equal(window, want), (shape, off, int((window != want).sum()))
            assert int(count.item()) == int(want.sum()), (shape, off)
            assert (host[:front + off] == 0xAB).all() and (host[front + off + n:] == 0xAB).all(), (shape, off)
        assert "threshold_kernel" in hip.last_kernel()


@pytest.mark.parametrize("dtype", cases.REAL_DTYPES)
def test_threshold_of_a_large_plane_of_every_type(prep, dtype):
    """About 2 500 workgroups add their counts to one 64-bit word."""
    a, thres = threshold_source(dtype, LARGE, 60)
    want = a > np.float64(thres)
    got, count = prep._threshold_plane(prep._rows_image(a), thres)
    assert got.dtype == np.uint8 and np.array_equal(got, want.astype(np.uint8))
    assert count == int(want.sum()) and 0.4 * N < count < 0.6 * N


# ---------------------------------------------------------------------------------------------- erosion, dilation, opening

OPS = ((0, bref.erosion), (1, bref.dilation), (2, bref.opening))


@functools.lru_cache(maxsize=None)
def morph_plane(kind):
    if kind == "mask":
        return bref.random_mask(LARGE, 0.5, 65)
    m = np.random.default_rng(66).integers(0, 256, LARGE).astype(np.uint8)          # grey values: minimum and maximum, not and / or
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def expected_morph(kind, op):
    return OPS[op][1](morph_plane(kind))


@pytest.mark.parametrize("kind", ["mask", "grey"])
def test_morphology_of_a_large_plane(prep, hip, fused, kind):
    m = morph_plane(kind)
    for op, _ in OPS:
        got, want = prep._morph_plane(prep._rows_image(m), op), expected_morph(kind, op)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (op, int((got != want).sum()))
    assert hip.last_kernel() == ("morph_cross_kernel<opening>" if fused else "morph_cross_kernel<erosion> + morph_cross_kernel<dilation>")


# ---------------------------------------------------------------------------------------------- the whole route

@pytest.mark.parametrize("bright", [False, True], ids=["dark_background", "bright_background"])
@pytest.mark.parametrize("dtype", ["float32", "uint16"])
def test_binarization_of_a_large_image_end_to_end(prep, dtype, bright):
    import torch
    tile = bref.dot_image(dtype, bright)
    reps = (-(-LARGE[0] // tile.shape[0]), -(-LARGE[1] // tile.shape[1]))
    img = np.ascontiguousarray(np.tile(tile, reps)[:LARGE[0], :LARGE[1]])
    assert img.shape == LARGE
    st = bref.binarization_stages(img, thres=None, denoise=True)
    # on the reference alone: every stage does something to this image
    assert (not np.array_equal(st["binary"], st["inverted"])) == bright
    for before, after in (("inverted", "cleared"), ("cleared", "opened"), ("opened", "filled")):
        assert not np.array_equal(st[before], st[after]), before
    want = st["filled"]
    got = prep.binarization(img, denoise=True)
    assert isinstance(got, np.ndarray) and got.dtype == np.int16 and np.array_equal(got, want), int((got != want).sum())
    t = prep.binarization(torch.from_numpy(img).to("cuda:0"), denoise=True)
    assert t.is_cuda and t.dtype == torch.int16 and np.array_equal(t.cpu().numpy(), want)
    pts = prep.get_points_dot_pattern(got, binarize=False)
    assert len(pts) > 4000 and np.array_equal(pts, bref.points(want))
