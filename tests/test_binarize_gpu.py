"""GPU suite for the binarization of dot images (discorpy_amd.prep.preprocessing; csrc/binarize_kernels.hip and dcp_clear_border_2d of
csrc/label_kernels.hip).  Every comparison is np.array_equal with the scipy / NumPy composite of tests/helpers/binarize_reference.py:
counts, 0 / 1 planes and selected elements are exact, so there is nothing to round.

The shapes come from the kernels' tiles (pinned to dcp_internal.h by tests/test_binarize_cpu.py): one pixel, a row and a column across
three tiles, one tile, one pixel more each way, 3 x 4 ragged tiles.  The lab options "x_label_lds", "x_hist_lds" and "x_morph_fused" run
both ways."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import binarize_reference as bref  # noqa: E402
import label_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu

TH, TW, SHAPES, BIG = bref.TH, bref.TW, bref.SHAPES, bref.SHAPES[-1]
SWITCH = bref.HIST_LDS_MAX_BINS


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


@pytest.fixture(params=[1, 0], ids=["lds", "global"])
def label_lds(request, hip):
    yield from _option(hip, "x_label_lds", request.param)


@pytest.fixture(params=[1, 0], ids=["hist_lds", "hist_global"])
def hist_lds(request, hip):
    yield from _option(hip, "x_hist_lds", request.param)


@pytest.fixture(params=[1, 0], ids=["fused", "two_launches"])
def fused(request, hip):
    yield from _option(hip, "x_morph_fused", request.param)


def _id(shape):
    return "%dx%d" % shape


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------------- histogram

LO, HI = -3.7, 11.3          # the range of bref.edge_hugging


@pytest.mark.parametrize("nbins", [512, 256])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_histogram_of_edge_hugging_values_equals_np_histogram(prep, hip, hist_lds, dtype, nbins):
    dt = np.dtype(dtype)
    lo, hi = dt.type(LO), dt.type(HI)
    edges = np.linspace(lo, hi, nbins + 1, dtype=dt)
    for shape in SHAPES:
        a = bref.edge_hugging(dtype, shape, nbins)
        want, want_edges = np.histogram(a, nbins, range=(lo, hi))
        assert np.array_equal(want_edges, edges) and want_edges.dtype == dt
        got = prep._histogram(prep._rows_image(a), nbins, edges=edges)
        assert got.dtype == np.int64 and np.array_equal(got, want), (shape, int(np.abs(got - want).sum()))
        assert got.sum() == a.size
    assert ("lds" if hist_lds else "global") in hip.last_kernel()
    a = bref.edge_hugging(dtype, BIG, nbins)
    assert np.array_equal(prep._histogram(prep._rows_image(a), nbins, edges=edges), np.histogram(a, nbins)[0])          # its own range
    # a strided view (a region of interest), read in place
    view = a[3:-5, 7:-9]
    assert not view.flags.c_contiguous
    assert np.array_equal(prep._histogram(prep._rows_image(view), nbins, edges=edges), np.histogram(view, nbins, range=(lo, hi))[0])
    # elements outside the edges and NaN are not counted
    b = a.copy()
    b[5, 5:9] = np.nan
    narrow = np.linspace(dt.type(-1.0), dt.type(5.0), nbins + 1, dtype=dt)
    want = np.histogram(b[~np.isnan(b)], nbins, range=(dt.type(-1.0), dt.type(5.0)))[0]
    got = prep._histogram(prep._rows_image(b), nbins, edges=narrow)
    assert np.array_equal(got, want) and 0 < got.sum() < b.size


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_histogram_of_a_flat_plane_with_one_outlier(prep, hist_lds, dtype):
    a = np.full(BIG, 2.5, dtype)
    a[5, 77] = 9.0
    for nbins in (512, 256):
        want, edges = np.histogram(a, nbins)
        got = prep._histogram(prep._rows_image(a), nbins, edges=edges)
        assert np.array_equal(got, want) and got[0] == a.size - 1 and got[-1] == 1


@pytest.mark.parametrize("dtype", ["uint8", "int8", "uint16", "int16"])
def test_bincount_on_both_sides_of_the_lds_switch(prep, hip, hist_lds, dtype):
    dt = np.dtype(dtype)
    info = np.iinfo(dt)
    rng = np.random.default_rng(31)
    spans = [info.max - info.min + 1] if dt.itemsize == 1 else [3000, SWITCH, SWITCH + 1, 65536]
    for span in spans:
        for shape in (BIG, (TH + 1, TW + 1), (1, 1)):
            lo = int(info.min) + (int(info.max) - int(info.min) + 1 - span) // 2
            a = rng.integers(lo, lo + span, size=shape).astype(dt)
            if a.size > 2:
                a.flat[0], a.flat[-1] = lo, lo + span - 1
            a[a.shape[0] // 2, : a.shape[1] // 2] = lo + span // 3          # a flat run: whole waves on one bin
            first, nbins = int(a.min()), int(a.max()) - int(a.min()) + 1
            want = np.bincount(a.ravel().astype(np.int64) - first, minlength=nbins)
            got = prep._histogram(prep._rows_image(a), nbins, first=first)
            assert np.array_equal(got, want) and got.sum() == a.size, (span, shape)
            if a.size > 2:
                assert ("lds" if hist_lds and nbins <= SWITCH else "global") in hip.last_kernel(), (nbins, hip.last_kernel())
    # values outside [first, first + nbins) are not counted
    a = rng.integers(max(info.min, -100), min(info.max, 100) + 1, size=BIG).astype(dt)
    sel = a.ravel().astype(np.int64)
    sel = sel[(sel >= 5) & (sel < 45)]
    assert np.array_equal(prep._histogram(prep._rows_image(a), 40, first=5), np.bincount(sel - 5, minlength=40))


# ---------------------------------------------------------------------------------------------- Otsu

def _scaled_dots(dtype):
    dt = np.dtype(dtype)
    img = bref.dot_image("float64")
    if dt.kind == "f":
        return bref.dot_image(dtype)
    info = np.iinfo(dt)
    return np.clip(np.abs(img) * (0.9 * info.max - info.min * (dt.kind == "i")) + info.min * (dt.kind == "i"), info.min, info.max).astype(dt)


@pytest.mark.parametrize("dtype", bref.HIST_DTYPES)
def test_threshold_otsu_equals_the_composite_bit_for_bit(prep, dtype):
    dt = np.dtype(dtype)
    img = _scaled_dots(dtype)
    two = np.where(bref.random_mask(BIG, 0.3, 5) != 0, dt.type(100), dt.type(3))
    two_far = np.where(bref.random_mask((TH + 1, TW + 1), 0.9, 6) != 0, dt.type(-7 if dt.kind != "u" else 250), dt.type(120))
    planes = [img, bref.select_roi(img, 0.3), np.full((TH, TW), 42, dt), np.full((1, 1), 5, dt), two, two_far]
    for a in planes:
        for nbins in (256, 512):
            want = bref.threshold_otsu(a, nbins)
            got = prep.threshold_otsu(a, nbins)
            assert isinstance(got, np.generic) and _same_bits(got, want), (a.shape, nbins, got, want)
    assert img.min() < bref.threshold_otsu(img) < img.max()
    import torch
    if dt.kind == "f" or hasattr(torch, dtype):
        t = torch.from_numpy(np.array(img)).to("cuda:0")
        assert _same_bits(prep.threshold_otsu(bref.select_roi(t, 0.3), 512), bref.threshold_otsu(bref.select_roi(img, 0.3), 512))


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_threshold_otsu_raises_numpys_error_for_a_non_finite_plane(prep, dtype, bad):
    a = np.array(bref.dot_image(dtype)[:TH + 1, :TW + 1])
    a[7, 9] = bad
    with pytest.raises(ValueError) as want:
        bref.threshold_otsu(a)
    with pytest.raises(ValueError) as got:
        prep.threshold_otsu(a)
    assert str(got.value) == str(want.value) and "is not finite" in str(got.value)


def test_threshold_otsu_raises_numpys_error_where_the_range_is_too_narrow(prep):
    a = (-300 + 1e-3 * np.random.default_rng(2).random((TH + 1, TW + 1))).astype(np.float32)
    with pytest.raises(ValueError) as want:
        bref.threshold_otsu(a)
    with pytest.raises(ValueError) as got:
        prep.threshold_otsu(a)
    assert str(got.value) == str(want.value) == "Too many bins for data range. Cannot create 256 finite-sized bins."
    assert _same_bits(prep.threshold_otsu(a, 8), bref.threshold_otsu(a, 8))


# ---------------------------------------------------------------------------------------------- abs, threshold, minimum / maximum

def _with_both_nans(a):
    a = np.array(a)
    if a.dtype.kind == "f":
        a[0, 0], a[0, 1], a[1, 0] = np.nan, np.copysign(np.nan, -1.0), -0.0
        assert np.signbit(a[0, 1]) and not np.signbit(a[0, 0])
    elif a.dtype.kind == "i":
        a[0, 0], a[0, 1] = np.iinfo(a.dtype).min, -1
    return a


@pytest.mark.parametrize("dtype", cases.REAL_DTYPES)
def test_abs_of_every_type(prep, dtype):
    for shape in ((TH + 1, TW + 1), BIG):
        a = _with_both_nans(cases.typed_image(dtype, shape, 91))
        for src in (a, a[:, 1:-2], a[:1, 1:2]):
            with np.errstate(all="ignore"):
                want = np.abs(src)
            got = prep._abs_plane(prep._rows_image(src))
            assert _same_bits(got, want), (dtype, shape)


@pytest.mark.parametrize("dtype", cases.REAL_DTYPES)
def test_threshold_of_every_type(prep, dtype):
    dt = np.dtype(dtype)
    a = _with_both_nans(cases.typed_image(dtype, BIG, 92))
    if dt.itemsize == 8 and dt.kind in "iu":
        # 64-bit values beyond 2^53 against a float threshold: NumPy rounds them to double, to nearest even
        a[2, :8] = np.array([2**53, 2**53 + 1, 2**53 + 2, 2**53 + 3, 2**62 + 1, 2**62 - 1, 2**53 - 1, 2**60], dt)
    values = [0.0, -0.0, 0.5, -1.5, 1.0, float(2**53), float(2**53 + 2), float(2**62), np.inf, -np.inf, np.nan]
    if dt.kind in "iu":
        values += [float(np.iinfo(dt).max), float(np.iinfo(dt).min), float(np.iinfo(dt).max) / 2]
    for src in (a, a[1:, 3:-1], a[:1, :1]):
        for thres in values:
            with np.errstate(all="ignore"):
                want = src > np.float64(thres)          # (a NumPy float64 scalar promotes the comparison to float64 for every type)
            got, count = prep._threshold_plane(prep._rows_image(src), thres)
            assert got.dtype == np.uint8 and np.array_equal(got, want.astype(np.uint8)), (dtype, thres, src.shape)
            assert count == int(want.sum())


@pytest.mark.parametrize("dtype", bref.HIST_DTYPES)
def test_minimum_maximum_and_non_finite_count(prep, dtype):
    dt = np.dtype(dtype)
    rough = cases.typed_image(dtype, BIG, 93)
    planes = [rough, rough[2:, 5:-3], rough[:1, :1], _scaled_dots(dtype)]
    if dt.kind == "f":
        finite = np.where(np.isfinite(rough), rough, dt.type(1.5))
        only_inf = np.where(np.isnan(rough), dt.type(-2.5), rough)
        zeros = np.where(bref.random_mask(BIG, 0.5, 3) != 0, dt.type(-0.0), dt.type(0.0))
        planes += [finite, only_inf, zeros, np.full((3, 5), np.inf, dt)]
    for a in planes:
        lo, hi, bad = prep._minmax(prep._rows_image(a))
        with np.errstate(all="ignore"):
            want_lo, want_hi = float(a.min()), float(a.max())
        assert bad == int((~np.isfinite(a.astype(np.float64))).sum())
        assert (lo == want_lo or (np.isnan(lo) and np.isnan(want_lo))) and (hi == want_hi or (np.isnan(hi) and np.isnan(want_hi))), (lo, hi, want_lo, want_hi)


# ---------------------------------------------------------------------------------------------- clear_border

@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_clear_border_patterns(prep, label_lds, shape):
    for name in cases.PATTERNS:
        m = cases.pattern(name, shape)
        assert np.array_equal(prep.clear_border(m), bref.clear_border(m)), name
        for conn in (4, 8):
            for invert in (False, True):
                got = prep._clear_border_plane(prep._rows_image(m), invert=invert, conn=conn)
                assert got.dtype == np.uint8 and np.array_equal(got, bref.clear_border(m, conn, invert)), (name, conn, invert)


def test_clear_border_of_empty_full_and_diagonally_touching_images(prep, hip, label_lds):
    assert not prep.clear_border(np.zeros(BIG, np.uint8)).any() and not prep.clear_border(np.ones(BIG, np.uint8)).any()
    m = np.zeros((TH + 9, TW + 9), np.uint8)
    m[0, 0] = m[1, 1] = m[2, 2] = 1          # touches the border only through the corner pixel's diagonal
    m[TH - 2:TH + 2, TW - 2:TW + 2] = 1      # an inner block across four tiles
    inner = np.zeros_like(m)
    inner[TH - 2:TH + 2, TW - 2:TW + 2] = 1
    with_tail = inner.copy()
    with_tail[1, 1] = with_tail[2, 2] = 1
    assert np.array_equal(prep.clear_border(m), inner) and np.array_equal(bref.clear_border(m), inner)
    four = prep._clear_border_plane(prep._rows_image(m), conn=4)
    assert np.array_equal(four, with_tail) and np.array_equal(bref.clear_border(m, 4), with_tail)
    assert "clear_border_kernel" in hip.last_kernel()


def test_clear_border_keeps_kind_and_dtype(prep):
    import torch
    m = bref.random_mask(BIG, 0.3, 8)
    want = bref.clear_border(m)
    assert want.any() and not np.array_equal(want, m)
    for dt in (np.float32, np.int16, np.bool_, np.float64):
        got = prep.clear_border(m.astype(dt))
        assert got.dtype == dt and np.array_equal(got, want.astype(dt))
    view = np.pad(m, ((0, 0), (2, 3)))[:, 2:-3]
    assert np.array_equal(prep.clear_border(view), want)
    t = torch.from_numpy(m.astype(np.float32)).to("cuda:0")
    got = prep.clear_border(t)
    assert got.is_cuda and got.dtype == torch.float32 and np.array_equal(got.cpu().numpy(), want.astype(np.float32))


# ---------------------------------------------------------------------------------------------- erosion, dilation, opening

OPS = ((0, bref.erosion), (1, bref.dilation), (2, bref.opening))


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_morphology_of_random_masks(prep, hip, fused, shape):
    planes = [bref.random_mask(shape, d, 60 + k) for k, d in enumerate((0.1, 0.5, 0.9))]
    planes.append(np.random.default_rng(64).integers(0, 256, shape).astype(np.uint8))          # grey values: minimum and maximum, not and / or
    for m in planes:
        for op, ref in OPS:
            got = prep._morph_plane(prep._rows_image(m), op)
            assert got.dtype == np.uint8 and np.array_equal(got, ref(m)), (op, int((got != ref(m)).sum()))
    assert hip.last_kernel() == ("morph_cross_kernel<opening>" if fused else "morph_cross_kernel<erosion> + morph_cross_kernel<dilation>")


def test_single_pixels_and_crosses_on_tile_and_image_corners(prep, fused):
    h, w = BIG
    m = np.zeros(BIG, np.uint8)
    centres = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (TH - 1, TW - 1), (TH, TW), (TH - 1, 2 * TW), (TH, 2 * TW - 1), (2 * TH, TW - 1),
               (2 * TH - 1, 3 * TW), (10, 0), (0, TW), (h - 1, 2 * TW - 1), (TH, w - 1)]
    for cy, cx in centres:
        for dy, dx in ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1)):
            if 0 <= cy + dy < h and 0 <= cx + dx < w:
                m[cy + dy, cx + dx] = 1
    singles = [(5, 5), (TH - 1, TW + 40), (TH, TW + 44), (2 * TH, 2 * TW), (2 * TH - 1, 2 * TW - 5), (h - 1, 200), (20, w - 1)]
    for y, x in singles:
        m[y, x] = 1
    view = np.pad(m, ((0, 0), (5, 2)), constant_values=1)[:, 5:-2]
    for src in (m, view):
        for op, ref in OPS:
            assert np.array_equal(prep._morph_plane(prep._rows_image(src), op), ref(m)), op
    opened = prep.opening(m)
    assert all(opened[c] == 1 for c in centres) and not any(opened[s] for s in singles) and opened.sum() < m.sum()


def test_opening_keeps_kind_and_dtype_and_takes_only_the_cross(prep, fused):
    import torch
    m = bref.random_mask(BIG, 0.8, 9)
    want = bref.opening(m)
    assert want.any() and not np.array_equal(want, m)
    for dt in (np.float32, np.int16, np.bool_, np.uint8, np.float64):
        for fp in (None, bref.CROSS, bref.CROSS.astype(np.uint8)):
            got = prep.opening(m.astype(dt), fp)
            assert got.dtype == dt and np.array_equal(got, want.astype(dt))
    with pytest.raises(ValueError, match="0 / 1"):
        prep.opening(m.astype(np.float32) * 0.5)
    for dt in (torch.float32, torch.uint8):
        got = prep.opening(torch.from_numpy(np.array(m)).to("cuda:0").to(dt))
        assert got.is_cuda and got.dtype == dt and np.array_equal(got.cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------- the whole route

@pytest.mark.parametrize("bright", [False, True], ids=["dark_background", "bright_background"])
@pytest.mark.parametrize("dtype", ["float32", "float64", "uint16"])
def test_binarization_end_to_end(prep, dtype, bright):
    import torch
    img = bref.dot_image(dtype, bright)
    assert 250 <= img.shape[0] <= 350 and 380 <= img.shape[1] <= 460
    mid = 0.5 if np.dtype(dtype).kind == "f" else 22000
    for denoise in (True, False):
        for thres in (None, mid, np.float64(mid) + 0.125):
            st = bref.binarization_stages(img, thres=thres, denoise=denoise)
            # on the reference alone: every stage does something to this image
            assert (not np.array_equal(st["binary"], st["inverted"])) == bright
            for before, after in (("inverted", "cleared"), ("cleared", "opened"), ("opened", "filled")):
                assert not np.array_equal(st[before], st[after]), (before, denoise, thres)
            want = st["filled"]
            got = prep.binarization(img, thres=thres, denoise=denoise)
            assert isinstance(got, np.ndarray) and got.dtype == np.int16 and np.array_equal(got, want), (denoise, thres, int((got != want).sum()))
            t = prep.binarization(torch.from_numpy(np.array(img)).to("cuda:0"), thres=thres, denoise=denoise)
            assert t.is_cuda and t.dtype == torch.int16 and np.array_equal(t.cpu().numpy(), want), (denoise, thres)
            pts = prep.get_points_dot_pattern(got, binarize=False)
            assert len(pts) > 100 and np.array_equal(pts, bref.points(want))
    assert np.array_equal(prep.binarization(img, ratio=0.6), bref.binarization_stages(img, ratio=0.6)["filled"])


def test_invert_dots_contrast_counts_on_the_gpu(prep):
    m = bref.random_mask(BIG, 0.7, 12).astype(np.float32)
    assert np.array_equal(prep._invert_dots_contrast(m), 1 - m)
    sparse = bref.random_mask(BIG, 0.2, 13).astype(np.float32)
    assert np.array_equal(prep._invert_dots_contrast(sparse), sparse)
    half = np.zeros((4, 6), np.float32)
    half[:2] = 1          # exactly half: the reference's ratio > 0.5 is false
    assert np.array_equal(prep._invert_dots_contrast(half), half)
