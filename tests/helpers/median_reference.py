"""An independent reference for the 2-D median filter (discorpy_amd.prep.preprocessing.median_filter), written from the specification
in plain NumPy and not from the kernel:

* the window of pixel (y, x) is rows y - sy // 2 .. y - sy // 2 + sy - 1 and columns x - sx // 2 .. x - sx // 2 + sx - 1;
* an index i outside the image maps to m = i mod 2 n, then to 2 n - 1 - m where m >= n (scipy's "reflect", any number of folds);
* the result is the window's element of rank (sy * sx) // 2 (0-based, ascending).

Floats are ordered by the IEEE 754 total order: negative NaNs (by payload, descending) < -inf < ... < -0.0 < +0.0 < ... < +inf <
positive NaNs (by payload, ascending).  That order is the contract ``discorpy_amd/prep/preprocessing.py`` documents, and it defines the
result bit for bit, the sign of a zero and the payload of a NaN included.  It is implemented by sorting on a signed-integer view of the
bits.  Integers and bool sort in their plain order; 64-bit integers are selected in their own type, never through a double.

:func:`median_reference` is the reference of the GPU tests; :func:`median_loop`, a literal Python double loop with ``sorted()``, exists
only to check :func:`median_reference` on tiny inputs (``tests/test_median_reference_cpu.py``).

The module also restates the launcher's choice of a tile (``median_tile_rows`` of ``csrc/median_kernels.hip``) and holds the tables
the tests expect of it; the CPU test ties those tables to the constants in the source.
"""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view


def window_sizes(size):
    """(sy, sx) of an int or a pair."""
    if isinstance(size, (tuple, list)):
        return int(size[0]), int(size[1])
    return int(size), int(size)


def reflect_index(i, n):
    """The specification's index rule for integer arrays ``i`` and a side of ``n``."""
    m = np.mod(np.asarray(i, dtype=np.int64), 2 * n)           # numpy's mod of a positive divisor is never negative
    return np.where(m >= n, 2 * n - 1 - m, m)


def total_order_keys(a):
    """Signed integers whose plain order is the selection order of ``a``, and the function that takes them back."""
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "f":
        it = np.dtype("i%d" % a.dtype.itemsize)
        low = it.type(np.iinfo(it).max)                          # every bit but the sign

        def flip(i):
            return np.where(i < 0, i ^ low, i)                   # negative floats: the larger the magnitude, the lower
        return flip(a.view(it)), lambda k: np.ascontiguousarray(flip(k)).view(a.dtype)
    if a.dtype.itemsize == 1:                                    # numpy selects among 16-bit values several times faster
        return a.view(np.uint8 if a.dtype.kind == "b" else a.dtype).astype(np.int16), lambda k: k.astype(a.dtype)
    return a, lambda k: k


def window_of(a, y, x, size):
    """The (sy, sx) window of pixel (y, x), gathered by the index rule."""
    sy, sx = window_sizes(size)
    h, w = a.shape
    ry = reflect_index(np.arange(y - sy // 2, y - sy // 2 + sy), h)
    rx = reflect_index(np.arange(x - sx // 2, x - sx // 2 + sx), w)
    return a[np.ix_(ry, rx)]


def median_reference(a, size):
    a = np.asarray(a)
    assert a.ndim == 2 and a.size
    sy, sx = window_sizes(size)
    h, w = a.shape
    rank = (sy * sx) // 2
    keys, back = total_order_keys(a)
    ry = reflect_index(np.arange(-(sy // 2), h - sy // 2 + sy - 1), h)
    rx = reflect_index(np.arange(-(sx // 2), w - sx // 2 + sx - 1), w)
    padded = keys[np.ix_(ry, rx)]                                # (h + sy - 1, w + sx - 1)
    out = np.empty((h, w), keys.dtype)
    for y in range(h):
        taps = sliding_window_view(padded[y:y + sy], (sy, sx)).reshape(w, sy * sx)
        out[y] = np.partition(taps, rank, axis=1)[:, rank]
    return back(out)


def _loop_key(v, kind, bits):
    """Python's sort key of one element: integers as they are, floats by their bit pattern ``v`` in total order."""
    if kind != "f":
        return v
    return (1 << bits) - 1 - v if v >> (bits - 1) else v + (1 << (bits - 1))


def median_loop(a, size):
    """The specification, literally: a loop over pixels and taps and ``sorted()``.  Tiny inputs only."""
    a = np.ascontiguousarray(a)
    sy, sx = window_sizes(size)
    h, w = a.shape
    kind, bits = a.dtype.kind, a.dtype.itemsize * 8
    cells = a.view("u%d" % a.dtype.itemsize) if kind in "fb" else a            # floats are handled as their bit patterns
    out = np.empty_like(cells)
    for y in range(h):
        for x in range(w):
            taps = []
            for wy in range(sy):
                my = (y - sy // 2 + wy) % (2 * h)
                if my >= h:
                    my = 2 * h - 1 - my
                for wx in range(sx):
                    mx = (x - sx // 2 + wx) % (2 * w)
                    if mx >= w:
                        mx = 2 * w - 1 - mx
                    taps.append(int(cells[my, mx]))
            out[y, x] = sorted(taps, key=lambda v: _loop_key(v, kind, bits))[(sy * sx) // 2]
    return out.view(a.dtype)


# ---------------------------------------------------------------------------------------------- the launcher's choice of a tile

TILE_WIDTH, TILE_HEIGHTS = 64, (16, 8, 4)
LDS_PLAIN, LDS_MAX = 64 << 10, 160 << 10


def box_bytes(th, sy, sx, key_bytes, tile_width=TILE_WIDTH):
    return (th + sy - 1) * (tile_width + sx - 1) * key_bytes


def tile_rows(sy, sx, key_bytes, caps=(LDS_PLAIN, LDS_MAX), tile_width=TILE_WIDTH, heights=TILE_HEIGHTS):
    """(tile height, index of the cap) of a window, (0, None) where no box fits: the chooser, restated."""
    for c, cap in enumerate(caps):
        for th in heights:
            if box_bytes(th, sy, sx, key_bytes, tile_width) <= cap:
                return th, c
    return 0, None


# key bytes -> (tile height, cap index, first and last square size); the last row is the global kernel, unbounded above
CHOOSER_TABLE = {
    4: [(16, 0, 1, 91), (8, 0, 92, 96), (4, 0, 97, 98), (16, 1, 99, 164), (8, 1, 165, 169), (4, 1, 170, 171), (0, None, 172, None)],
    8: [(16, 0, 1, 54), (8, 0, 55, 59), (4, 0, 60, 62), (16, 1, 63, 106), (8, 1, 107, 110), (4, 1, 111, 113), (0, None, 114, None)],
}
# key bytes -> (square size, tile height) on both sides of every boundary
BOUNDARY_SIZES = {
    4: [(91, 16), (92, 8), (96, 8), (97, 4), (98, 4), (99, 16), (164, 16), (165, 8), (169, 8), (170, 4), (171, 4), (172, 0)],
    8: [(54, 16), (55, 8), (59, 8), (60, 4), (62, 4), (63, 16), (106, 16), (107, 8), (110, 8), (111, 4), (113, 4), (114, 0)],
}
LARGEST_BOX = {4: (171, 162864), 8: (113, 163328)}               # the largest launches: square size, bytes (174 x 234 x 4, 116 x 176 x 8)
# key bytes, window, tile height, cap index: one non-square window per cap chosen so that the 16-row box misses the cap and the
# 8-row box fits it ((100, 90) at 4 bytes: 115 x 153 x 4 = 70 380 > 65 536 >= 107 x 153 x 4 = 65 484), and the wide and the tall
# line, (1, 301) with a 16 x 364 box and (301, 1) with a 316 x 64 box (8-byte keys: 161 792 bytes)
NONSQUARE = [(4, (100, 90), 8, 0), (4, (150, 190), 8, 1), (8, (60, 50), 8, 0), (8, (100, 120), 8, 1),
             (4, (1, 301), 16, 0), (4, (301, 1), 16, 1), (8, (1, 301), 16, 0), (8, (301, 1), 16, 1)]


def kernel_name(bits, th):
    """What ``last_kernel()`` reports for an element of ``bits`` bits on a tile of ``th`` rows (0: the global kernel)."""
    return "median_lds_kernel<bits=%d, tile=64x%d>" % (bits, th) if th else "median_global_kernel<bits=%d>" % bits


# ---------------------------------------------------------------------------------------------- float images for the edge cases

def edge_image(dtype, shape, seed):
    """Two fifths zeros, half of them -0.0, three tenths each negative and positive values from {inf, the largest finite value, 1,
    the smallest subnormal} and normal draws: the element of the median rank is a zero in many windows, with zeros of both signs on
    either side of it."""
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype)
    info = np.finfo(dt)
    special = np.array([np.inf, info.max, 1.0, info.smallest_subnormal], dt)
    mag = np.where(rng.random(shape) < 0.6, special[rng.integers(0, 4, size=shape)], np.abs(rng.standard_normal(shape)).astype(dt))
    u = rng.random(shape)
    a = np.where(u < 0.3, -mag, np.where(u < 0.6, mag, np.where(u < 0.8, dt.type(-0.0), dt.type(0.0)))).astype(dt)
    a.setflags(write=False)
    return a


def nan_image(dtype, shape, seed):
    """Normal draws with a few NaNs of either sign and different payloads (a signalling one among them): six lone ones, and one
    3 x 3 block per sign, so that a window of 3 there holds nothing else.  Returns the image and the mask of the NaNs."""
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype)
    h, w = shape
    assert h >= 20 and w >= 60
    a = rng.standard_normal(shape).astype(dt)
    cells = a.view("u%d" % dt.itemsize)
    bits, mant = dt.itemsize * 8, np.finfo(dt).nmant
    expo = ((1 << (bits - 1 - mant)) - 1) << mant                # all exponent bits
    quiet = 1 << (mant - 1)

    def nan(negative, payload, signalling=False):
        return (1 << (bits - 1) if negative else 0) | expo | (0 if signalling else quiet) | payload

    for k, (y, x) in enumerate([(0, 0), (2, 30), (10, w - 1), (h - 1, 17), (h - 2, w - 2), (9, 40)]):
        cells[y, x] = nan(k % 2 == 1, 1 + 37 * k, signalling=k == 5)
    for negative, (y, x) in ((False, (5, 10)), (True, (14, 50))):
        for j in range(9):
            cells[y + j // 3, x + j % 3] = nan(negative, 3 + 5 * j)
    mask = np.isnan(a)
    assert mask.sum() == 24
    a.setflags(write=False)
    return a, mask
