"""Shapes and binary patterns for the labelling tests (tests/test_label_gpu.py), with scipy's results computed once per case.

TILE is label_tile_kernel's tile as the tests assume it; tests/test_label_cpu.py pins it to kLabelTH / kLabelTW of
discorpy_amd/csrc/dcp_internal.h.  Every shape is built from it: a single pixel, a row and a column that span three tiles, exactly one
tile, one pixel more each way (four tiles, three of them slivers), and a frame of 3 x 4 tiles with ragged edges.

MEDIUM and LARGE are for tests/test_label_scale_gpu.py and tests/test_binarize_scale_gpu.py.  MEDIUM is 6 x 5 ragged tiles: about 330
workgroups of pair threads under "x_label_lds" 0, small enough for the long chains of the adversarial patterns.  LARGE is the smallest
kind of frame at which the loops that SHAPES never turns do turn: label_scan_kernel walks three rounds of kLabelBlock block counts (the
carry between rounds, and the sums of earlier waves within one), minmax_kernel and histogram_kernel reach their cap of kReduceMaxBlocks
workgroups with a last round that is ragged between workgroups, and the sums of 16-bit weights stay below 2^53, where scipy's float64
accumulation is still exact.  tests/test_label_cpu.py and tests/test_binarize_cpu.py assert every one of these conditions against the
kernels' constants.
"""
import functools

import numpy as np

TILE = {"TH": 32, "TW": 128}
TH, TW = TILE["TH"], TILE["TW"]
SHAPES = [(1, 1), (1, 2 * TW + 3), (2 * TH + 3, 1), (TH, TW), (TH + 1, TW + 1), (2 * TH + 5, 3 * TW + 7)]
BIG = SHAPES[-1]
MEDIUM = (5 * TH + 3, 4 * TW + 5)
LARGE = (1103, 2303)
CROSS = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], bool)
BLOCK = np.ones((3, 3), bool)
STRUCTURES = {4: CROSS, 8: BLOCK}
DENSITIES = (0.3, 0.55, 0.6, 0.8)


def large_conditions(shape, scan_chunk, label_block, reduce_max_blocks, bin_block):
    """What makes ``shape`` a LARGE, as a dict of named conditions, given kLabelScanChunk, kLabelBlock, kReduceMaxBlocks and kBinBlock."""
    h, w = shape
    n = h * w
    nb = -(-n // scan_chunk)
    return {
        "ragged tile, wider than a wave": h % TH != 0 and w % TW > 64,
        "no row and no plane of whole quads": w % 4 != 0 and n % 4 != 0,
        "three scan rounds, two of them full": nb > 2 * label_block,
        "the partial scan round crosses a wave": nb % label_block > 64,
        "the cap of the reduce grid is reached": -(-n // (bin_block * 8)) > reduce_max_blocks,
        "the last reduce round is ragged between workgroups": n % (reduce_max_blocks * bin_block) >= bin_block,
        "float64 sums of 16-bit weights are exact": n * max(h, w) * 65535 < 2**53,
        "below 2^24 pixels": n < 2**24,
    }


def zeros(h, w):
    return np.zeros((h, w), np.uint8)


def ones(h, w):
    return np.ones((h, w), np.uint8)


def corners(h, w):
    m = zeros(h, w)
    m[0, 0] = m[0, w - 1] = m[h - 1, 0] = m[h - 1, w - 1] = 1
    return m


def checkerboard(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return ((y + x) % 2 == 0).astype(np.uint8)


def serpentine(h, w):
    """A one-pixel path through every second row, joined at alternating ends: one component whose chain is as long as the image."""
    m = zeros(h, w)
    m[0::2] = 1
    for k, y in enumerate(range(1, h, 2)):
        if y + 1 < h:
            m[y, w - 1 if k % 2 == 0 else 0] = 1
    return m


def _spiral(h, w, pitch):
    """A rectangular spiral walked inwards from (0, 0), `pitch` pixels between its turns."""
    m = zeros(h, w)
    top, left, bottom, right = 0, 0, h - 1, w - 1
    first = True
    while top <= bottom and left <= right:
        m[top, (left if first else max(left - pitch, 0)):right + 1] = 1
        m[top:bottom + 1, right] = 1
        if bottom - top >= pitch:
            m[bottom, left:right + 1] = 1
            if right - left >= pitch:
                m[top + pitch:bottom + 1, left] = 1
        top, left, bottom, right = top + pitch, left + pitch, bottom - pitch, right - pitch
        first = False
    return m


def double_spiral(h, w):
    a = _spiral(h, w, 4)
    return np.maximum(a, np.roll(np.roll(a, 2, axis=0), 2, axis=1) * (np.arange(h)[:, None] >= 2) * (np.arange(w)[None, :] >= 2)).astype(np.uint8)


def comb(h, w):
    """Teeth in every second column, joined along the LAST row only: the first pixel of the component and the pixels that merge it are
    a whole image apart."""
    m = zeros(h, w)
    m[:, 0::2] = 1
    m[h - 1, :] = 1
    return m


def comb_transposed(h, w):
    return np.ascontiguousarray(comb(w, h).T)


def diagonals(h, w):
    """Diagonal and anti-diagonal lines through the tiles' corners: (TH - 1, TW - 1)-(TH, TW) and (TH - 1, TW)-(TH, TW - 1) are pairs."""
    y, x = np.mgrid[0:h, 0:w]
    main = (x - y) % 8 == (TW - TH) % 8
    anti = (x + y) % 16 == (TW + TH - 1) % 16
    return (main | anti).astype(np.uint8)


def random_mask(h, w, density, seed):
    return (np.random.default_rng(seed).random((h, w)) < density).astype(np.uint8)


PATTERNS = {"zeros": zeros, "ones": ones, "corners": corners, "checkerboard": checkerboard, "serpentine": serpentine,
            "double_spiral": double_spiral, "comb": comb, "comb_transposed": comb_transposed, "diagonals": diagonals}
for _k, _d in enumerate(DENSITIES):
    PATTERNS["random_%g" % _d] = functools.partial(random_mask, density=_d, seed=4100 + _k)


@functools.lru_cache(maxsize=None)
def pattern(name, shape):
    m = PATTERNS[name](*shape)
    assert m.shape == shape and m.dtype == np.uint8
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def expected_labels(name, shape, conn):
    from scipy import ndimage as ndi
    lab, num = ndi.label(pattern(name, shape), STRUCTURES[conn])
    lab.setflags(write=False)
    return lab, num


# ---------------------------------------------------------------------------------------------- hole filling

def rings(h, w):
    """Square rings of side 7 on a pitch of 10, the first one touching the corner."""
    m = zeros(h, w)
    for y in range(0, h - 6, 10):
        for x in range(0, w - 6, 10):
            m[y:y + 7, x:x + 7] = 1
            m[y + 1:y + 6, x + 1:x + 6] = 0
    return m


def nested_rings(h, w):
    m = zeros(h, w)
    k = 0
    while 2 * k < min(h, w) - 2 * k:
        m[2 * k:h - 2 * k, 2 * k:w - 2 * k] = 1
        m[2 * k + 1:h - 2 * k - 1, 2 * k + 1:w - 2 * k - 1] = 0
        k += 1
    return m


def open_ring(h, w):
    """A ring along the frame's border with one pixel missing in its top row: its inside reaches the border through that pixel."""
    m = ones(h, w)
    m[1:h - 1, 1:w - 1] = 0
    m[0, w // 2] = 0
    return m


def diagonal_gap(h, w):
    """Regions of zeros shut in by pixels that touch only diagonally: diamond outlines (|dy| + |dx| = 4) and square rings with one
    corner pixel missing.  The zeros inside and outside are neighbours only across a diagonal, so under the 4-neighbour structure of the
    background they are separate components; rings with a corner pixel AND its neighbour missing are open."""
    m = rings(h, w)
    m[0::20, 0::10] = 0
    m[10::20, 0::10] = 0
    m[10::20, 1::10] = 0
    dy, dx = np.mgrid[-4:5, -4:5]
    diamond = np.abs(dy) + np.abs(dx) == 4
    for cy in range(14, h - 4, 30):
        for cx in range(24, w - 4, 30):
            m[cy - 5:cy + 6, cx - 5:cx + 6] = 0
            m[cy - 4:cy + 5, cx - 4:cx + 5][diamond] = 1          # (the window lies inside the frame: 4 <= cy < h - 4, cx likewise)
    return m


HOLE_PATTERNS = {"rings": rings, "nested_rings": nested_rings, "open_ring": open_ring, "diagonal_gap": diagonal_gap}
for _k, _d in enumerate(DENSITIES):
    HOLE_PATTERNS["random_%g" % _d] = functools.partial(random_mask, density=_d, seed=4200 + _k)


@functools.lru_cache(maxsize=None)
def hole_pattern(name, shape):
    m = HOLE_PATTERNS[name](*shape)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def expected_filled(name, shape):
    from scipy import ndimage as ndi
    res = ndi.binary_fill_holes(hole_pattern(name, shape))
    res.setflags(write=False)
    return res


# ---------------------------------------------------------------------------------------------- element types

REAL_DTYPES = ("bool", "uint8", "int8", "uint16", "int16", "uint32", "int32", "uint64", "int64", "float32", "float64")


def typed_image(dtype, shape, seed):
    """Nonzero where a 0.55-density mask is set; the nonzero values include ones whose low byte, low 16 and low 32 bits are all zero
    (a test of the element that looks at a part of it fails), negative ones, and for floats NaN, -0.0 (zero), a denormal and -inf."""
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype)
    mask = rng.random(shape) < 0.55
    if dt.kind == "b":
        return mask
    pick = rng.integers(0, 4, size=shape)
    if dt.kind == "f":
        info = np.finfo(dt)
        special = np.array([np.nan, info.smallest_subnormal, -np.inf, -1.5], dt)
        a = np.where(mask, special[pick], np.where(pick < 2, dt.type(-0.0), dt.type(0.0))).astype(dt)
        assert np.isnan(a).any() and (a == info.smallest_subnormal).any() and np.signbit(a[a == 0]).any()
        return a
    info = np.iinfo(dt)
    bits = dt.itemsize * 8
    first = 1 << (bits // 2) if bits >= 16 else 1          # every bit of the low half zero
    special = np.array([first, int(info.max), int(info.min) if dt.kind == "i" else 1 << (bits - 1), 1 << (bits - 1 if dt.kind == "u" else bits - 2)],
                       dtype=dt)
    return np.where(mask, special[pick], 0).astype(dt)
