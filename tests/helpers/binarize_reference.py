"""The yardstick of the binarization tests: every step of the reference's ``binarization`` (discorpy/prep/preprocessing.py:216-248)
written with what NumPy and scipy define, since scikit-image is not installed.

    threshold_otsu(a, nbins)   np.histogram for floats, np.bincount per value for integers, then the published Otsu formula in float64
    clear_border(a)            ndi.label with the full 3 x 3 structure; every label with a pixel on the image border is dropped
    opening(a)                 ndi.grey_opening(a, footprint=cross, mode="reflect")

The conditions under which these ARE yardsticks are asserted by tests/test_binarize_cpu.py: for the cross, scipy's "reflect" equals
"ignore what lies outside" (``pad_and_ignore``), and np.histogram equals the plain search of its own edges (``histogram_by_search``)
although its raw estimate (``raw_estimate``) is off by one for many elements of the edge-hugging inputs.

The shapes come from the kernels' tiles (SHAPES), pinned to dcp_internal.h by tests/test_binarize_cpu.py; MEDIUM and LARGE are those of
tests/helpers/label_cases.py, where they are explained.
"""
import functools

import numpy as np
from scipy import ndimage as ndi

from label_cases import LARGE, MEDIUM  # noqa: F401

CROSS = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], bool)
BLOCK = np.ones((3, 3), bool)
TILE = {"TH": 32, "TW": 128}          # kMorphTH / kMorphTW (and kLabelTH / kLabelTW)
TH, TW = TILE["TH"], TILE["TW"]
HIST_LDS_MAX_BINS = 4096               # kHistLdsMaxBins
REDUCE_MAX_BLOCKS, BIN_BLOCK = 1024, 256          # kReduceMaxBlocks, kBinBlock: the grid of minmax_kernel / histogram_kernel
SHAPES = [(1, 1), (1, 2 * TW + 3), (2 * TH + 3, 1), (TH, TW), (TH + 1, TW + 1), (2 * TH + 5, 3 * TW + 7)]
HIST_DTYPES = ("float32", "float64", "uint8", "int8", "uint16", "int16")


# ---------------------------------------------------------------------------------------------- Otsu

def otsu_of_counts(counts, centres):
    c = counts.astype(np.float64)
    w1 = np.cumsum(c)
    w2 = np.cumsum(c[::-1])[::-1]
    m1 = np.cumsum(c * centres) / w1
    m2 = (np.cumsum((c * centres)[::-1]) / w2[::-1])[::-1]
    v = w1[:-1] * w2[1:] * (m1[:-1] - m2[1:]) ** 2
    return centres[np.argmax(v)]


def threshold_otsu(a, nbins=256):
    a = np.asarray(a)
    if a.dtype.kind == "f":
        counts, edges = np.histogram(a, nbins)          # raises for a NaN, an infinity and a range too narrow for the bins
        if a.min() == a.max():
            return a.min()
        return otsu_of_counts(counts, (edges[:-1] + edges[1:]) / 2)
    lo, hi = int(a.min()), int(a.max())
    if lo == hi:
        return a.min()
    counts = np.bincount(a.ravel().astype(np.int64) - lo, minlength=hi - lo + 1)
    return otsu_of_counts(counts, np.arange(lo, hi + 1))


def histogram_by_search(a, nbins):
    """Counts of ``a`` between np.linspace(min, max, nbins + 1) in a's own type: a search of the edges, the last bin closed."""
    a = np.asarray(a)
    edges = np.linspace(a.min(), a.max(), nbins + 1, dtype=a.dtype)
    idx = np.searchsorted(edges, a.ravel(), side="right") - 1
    idx[a.ravel() == edges[-1]] = nbins - 1
    return np.bincount(idx, minlength=nbins), edges


def final_bins(a, edges):
    idx = np.searchsorted(edges, a.ravel(), side="right") - 1
    idx[a.ravel() == edges[-1]] = len(edges) - 2
    return idx


def raw_estimate(a, edges):
    """np.histogram's first guess of every element's bin (numpy/lib/_histograms_impl.py, the f_indices block), before its two
    correction steps."""
    nbins = len(edges) - 1
    f = ((a.ravel() - edges[0]) / (edges[-1] - edges[0])) * nbins
    idx = f.astype(np.intp)
    idx[idx == nbins] -= 1
    return idx


@functools.lru_cache(maxsize=None)
def edge_hugging(dtype, shape, nbins, seed=0):
    """Values on every edge of np.linspace(lo, hi, nbins + 1) and one ulp either side of it, mixed with uniform ones; lo and hi are
    elements, so np.histogram's own edges are these."""
    dt = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    lo, hi = dt.type(-3.7), dt.type(11.3)
    edges = np.linspace(lo, hi, nbins + 1, dtype=dt)
    pool = np.concatenate([edges, np.nextafter(edges[1:], dt.type(-np.inf)), np.nextafter(edges[:-1], dt.type(np.inf)),
                           rng.uniform(lo, hi, nbins).astype(dt)])
    pool = pool[(pool >= lo) & (pool <= hi)]
    a = rng.choice(pool, size=shape).astype(dt)
    a.flat[0], a.flat[-1] = hi, lo
    if a.size > 2:
        a.flat[a.size // 2] = hi          # the closed last edge more than once
    a.setflags(write=False)
    return a


# ---------------------------------------------------------------------------------------------- border components, morphology

def clear_border(a, conn=8, invert=False):
    a = np.asarray(a)
    fg = (a == 0) if invert else (a != 0)
    lab, _ = ndi.label(fg, BLOCK if conn == 8 else CROSS)
    touching = np.unique(np.concatenate([lab[0], lab[-1], lab[:, 0], lab[:, -1]]))
    return (fg & ~np.isin(lab, touching[touching > 0])).astype(np.uint8)


def erosion(a):
    return ndi.grey_erosion(a, footprint=CROSS, mode="reflect")


def dilation(a):
    return ndi.grey_dilation(a, footprint=CROSS, mode="reflect")


def opening(a):
    return ndi.grey_opening(a, footprint=CROSS, mode="reflect")


def _cross_fold(a, fill, fold):
    p = np.pad(a, 1, constant_values=fill)
    return fold.reduce([p[1:-1, 1:-1], p[:-2, 1:-1], p[2:, 1:-1], p[1:-1, :-2], p[1:-1, 2:]])


def pad_and_ignore(a, op):
    """Erosion (0), dilation (1) or opening (2) by the cross over the in-image neighbours only (scikit-image's border rule)."""
    a = np.asarray(a, np.uint8)
    if op == 0:
        return _cross_fold(a, 255, np.minimum)
    if op == 1:
        return _cross_fold(a, 0, np.maximum)
    return _cross_fold(_cross_fold(a, 255, np.minimum), 0, np.maximum)


@functools.lru_cache(maxsize=None)
def random_mask(shape, density, seed):
    m = (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)
    m.setflags(write=False)
    return m


# ---------------------------------------------------------------------------------------------- the whole route

def select_roi(mat, ratio):
    height, width = mat.shape
    ratio = np.clip(ratio, 0.05, 1.0)
    dh, dw = int((height - ratio * height) / 2), int((width - ratio * width) / 2)
    return mat[dh:height - dh, dw:width - dw]


def binarization_stages(mat, ratio=0.3, thres=None, denoise=True):
    """The reference's binarization step by step: a dict of the planes after each stage ("filled" is its return value)."""
    mat = np.asarray(mat)
    if denoise:
        mat = ndi.median_filter(np.abs(mat), (2, 2))
    if thres is None:
        thres = threshold_otsu(select_roi(mat, ratio), nbins=512)
    out = {"thres": thres}
    out["binary"] = np.asarray(mat > thres, dtype=np.float32)
    m = out["binary"]
    if np.sum(m) / (m.shape[0] * m.shape[1]) > 0.5:
        m = np.max(m) - m
    out["inverted"] = m
    out["cleared"] = clear_border(m).astype(np.float32)
    out["opened"] = opening(out["cleared"])
    out["filled"] = np.int16(ndi.binary_fill_holes(out["opened"]))
    return out


def points(binary):
    """The reference's get_points_dot_pattern(binary, binarize=False)."""
    lab, num = ndi.label(binary)
    return np.asarray(ndi.center_of_mass(binary, lab, np.arange(1, num + 1)))


@functools.lru_cache(maxsize=None)
def dot_image(dtype, bright=False, shape=(300, 420), seed=7):
    """A grid of dots of radius 5 on a pitch of 22 over a gradient background, with salt-and-pepper noise; the grid is cut by the image
    border, and every third dot is a ring (its middle at background level).  ``bright``: dark dots on a bright background."""
    dt = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    h, w = shape
    y, x = np.mgrid[0:h, 0:w]
    r2 = ((y + 4) % 22 - 11) ** 2 + ((x + 9) % 22 - 11) ** 2
    ring = (((y + 4) // 22 + (x + 9) // 22) % 3 == 0)
    dots = (r2 <= 25) & ~(ring & (r2 <= 4))
    back = 0.15 + 0.04 * x / w + 0.02 * y / h
    img = np.where(dots, 0.8 + 0.05 * np.sin(x / 9.0), back)
    if bright:
        img = 1.0 - img
    noise = rng.random(shape)
    img = np.where(noise < 0.004, 1.0, np.where(noise > 0.996, 0.0, img))
    img = img + 0.01 * rng.standard_normal(shape)
    if dt.kind == "f":
        if dt == np.float64:
            img = np.where((noise > 0.5) & (noise < 0.51), -img, img)          # (negative values, so that abs matters)
        out = img.astype(dt)
    else:
        out = np.clip(img * 40000.0 + 2000.0, 0, np.iinfo(dt).max).astype(dt)
    out.setflags(write=False)
    return out
