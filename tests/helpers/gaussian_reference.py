"""scipy.ndimage.gaussian_filter for 2-D input restated in NumPy, operation by operation: the arithmetic contract of
dcp_correlate_sym_2d ("The Gaussian filter").  tests/test_gaussian_reference_cpu.py holds it np.array_equal to scipy; the
GPU kernels are held to scipy directly, so this file is the written-down form of what they must do, checked on the CPU.

    weights      x = arange(-r, r + 1); phi = exp(-0.5 / sigma^2 * x^2); phi / phi.sum(), r = int(truncate * sigma + 0.5)
    one element  tmp = e[i] w[r]; for j = -r .. -1: tmp += (e[i + j] + e[i - j]) w[r + j]      (float64, one rounding per operation)
    extension    reflect / mirror / nearest / wrap fold the index (any number of folds); constant is the double cval
    axes         axis 0, then axis 1 on the first result cast to the element type; sigma <= 1e-15 skips an axis
    cast         floats round to nearest, integers truncate toward zero (NumPy's astype from float64 is the same C cast)

For the tests only: `arithmetic=` runs a pass that is wrong on purpose (reversed, unpaired, fused, ...), plateau_image / special_image /
tiny_image are the inputs on which tests/test_gaussian_edges_gpu.py can tell such a pass from scipy's, and fma is an exact float64
fused multiply-add.
"""
import numpy as np

ALIASES = {"grid-mirror": "reflect", "grid-constant": "constant", "grid-wrap": "wrap"}


def gaussian_weights(sigma, truncate=4.0, radius=None):
    if radius is None:
        radius = int(truncate * float(sigma) + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return phi / phi.sum()


def extend_index(p, n, mode):
    """Index into a line of length n for every integer position in `p`; -1 where the value is cval."""
    p = np.asarray(p, dtype=np.int64)
    mode = ALIASES.get(mode, mode)
    if mode == "reflect":
        q = np.mod(p, 2 * n)
        return np.where(q >= n, 2 * n - 1 - q, q)
    if mode == "mirror":
        if n == 1:
            return np.zeros_like(p)
        q = np.mod(p, 2 * n - 2)
        return np.where(q >= n, 2 * n - 2 - q, q)
    if mode == "nearest":
        return np.clip(p, 0, n - 1)
    if mode == "wrap":
        return np.mod(p, n)
    if mode == "constant":
        return np.where((p < 0) | (p >= n), -1, p)
    raise RuntimeError("boundary mode not supported")


ARITHMETICS = ("scipy", "reversed", "unpaired", "fused", "unrounded_between", "round_half", "cval_cast")


def _two_sum(a, b):
    """s = fl(a + b) and t with s + t = a + b exactly (Knuth)."""
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _two_prod(a, b):
    """p = fl(a b) and e with p + e = a b exactly (Veltkamp's split, Dekker's product; no overflow or underflow in the tests' range)."""
    p = a * b
    ca, cb = a * 134217729.0, b * 134217729.0
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def fma(a, b, c):
    """a b + c with one rounding, on float64 arrays, exactly: the product as an unevaluated sum uh + ul, th + tl = c + uh, the two small
    terms added with rounding to odd, one last rounding to nearest (Boldo and Melquiond, "Emulation of a FMA and correctly rounded sums:
    proved algorithms using rounding to odd", IEEE TC 57, 2008).  tests/test_gaussian_reference_cpu.py holds it to fractions.Fraction.
    Finite values away from overflow and underflow only."""
    a, b, c = (np.asarray(v, dtype=np.float64) for v in np.broadcast_arrays(a, b, c))
    uh, ul = _two_prod(a, b)
    th, tl = _two_sum(c, uh)
    v, err = _two_sum(tl, ul)
    even = (v.view(np.uint64) & np.uint64(1)) == 0
    v = np.where((err != 0) & even, np.nextafter(v, np.where(err > 0, np.inf, -np.inf)), v)      # round to odd
    return th + v


# Six more levels per integer type, found by a search over constant lines (a plateau's interior) for levels at which the truncated
# result of the passes of sigma 3 and of sigma (1, 5.3) changes under "reversed", "unpaired" and "fused": with the six named levels alone
# some (type, sigma, arithmetic) see nothing, a level either shows a one-ulp change or it does not.  For the 8-bit types no level at all
# shows "fused" at sigma (1, 5.3) (tests/test_gaussian_reference_cpu.py checks all 256).
MORE_LEVELS = {
    "uint8": [27, 163, 54, 39, 43, 47],
    "int8": [-108, -87, -54, 87, -27, -122],
    "uint16": [32541, 65082, 64968, 32484, 26416, 16242],
    "int16": [32541, -32541, 8121, 26585, -32484, -29593],
    "uint32": [434519403, 230724423, 3726567831, 486872233, 186376111, 3126623294],
    "int32": [2060386726, 1626005720, 1936906773, -323798383, 360876303, -193667495],
    "int64": [-2203650119737176907, -3262758332606638782, -3286900868073324966, -2180633645834942208, 3526837276008996343,
              -2116580484071553576],
    "uint64": [12148249315451622450, 6353043963895336320, 15065414286368001976, 12345, 5743875428958567893,
               13748466189571005410],
}


def plateau_levels(dtype):
    """The levels of plateau_image: six named ones (even block-rows), then six more (odd block-rows).
    Integers: max, min, max // 2 + 1, 1 (unsigned) or -1 (signed), max - 1, max // 3, then MORE_LEVELS; int64 stays within +-2^62 with
    2^53 + 1 among the levels, uint64 at most 2^64 - 2^16 with levels above 2^63 whose low bits are set (the read through a double
    rounds).  Floats: 1/3, -1/3, 1e-3, max / 4, -0.0, 1.0 and 3, -2/3, 1e-30, -max / 8, 0.1, -1e5 (not order-sensitive by truncation:
    they put the same tiles to work, and a float64 result shows any change of the sum anyway)."""
    dt = np.dtype(dtype)
    if dt.kind == "f":
        big = float(np.finfo(dt).max)
        return np.array([1.0 / 3.0, -1.0 / 3.0, 1e-3, big / 4, -0.0, 1.0, 3.0, -2.0 / 3.0, 1e-30, -big / 8, 0.1, -1e5]).astype(dt)
    if dt == np.int64:
        named = [2 ** 62, -2 ** 62, 2 ** 53 + 1, -1, 2 ** 62 - 2 ** 9 - 1, 2 ** 62 // 3]
    elif dt == np.uint64:
        named = [2 ** 64 - 2 ** 16, 0, 2 ** 63 + 2 ** 11 + 1, 1, 2 ** 64 - 2 ** 16 - 2 ** 10 - 1, 2 ** 64 // 3]
    else:
        lo, hi = int(np.iinfo(dt).min), int(np.iinfo(dt).max)
        named = [hi, lo, hi // 2 + 1, 1 if dt.kind == "u" else -1, hi - 1, hi // 3]
    levels = named + MORE_LEVELS[dt.name]
    assert len(set(levels)) == 12
    return np.array(levels, dtype=dt)


def plateau_image(shape, dtype, block):
    """Blocks of `block` = (rows, columns), each of one level, neighbours of different levels: the block at block-row i and
    block-column k has level 6 (i mod 2) + (k + 3 i) mod 6 of plateau_levels(dtype).  Inside a plateau wider than the window the float64
    sum of a pass lies within a few ulp of the level L, so an integer type's truncation toward zero turns a one-ulp change of the sum
    into L against L - 1: these images see the order of the additions, the pairing and a fused multiply-add, which normal data does
    not ("The Gaussian filter").  Read-only."""
    levels = plateau_levels(dtype)
    y, x = np.mgrid[0:shape[0], 0:shape[1]]
    i, k = y // block[0], x // block[1]
    a = levels[6 * (i % 2) + (k + 3 * i) % 6]
    a.setflags(write=False)
    return a


def special_image(dtype, shape=(40, 70)):
    """Standard-normal float data with what a window of radius 12 must carry through unharmed: a 28 x 28 block of -0.0 (rows 0..27,
    columns 0..27: the windows of rows 12..15, columns 12..15 hold nothing else), a 28 x 28 block of the 1999 smallest subnormals next
    to it (columns 28..55), a 2 x 2 block of the type's maximum (rows 33..34, columns 52..53; in float64 lo + hi overflows there), +inf
    at (39, 0), -inf at (39, 35) -- 35 columns apart, so windows hold one, the other or neither -- and one NaN at (39, 69)."""
    dt = np.dtype(dtype)
    assert dt.kind == "f" and tuple(shape) == (40, 70)
    rng = np.random.default_rng(40070 + dt.itemsize)
    a = rng.standard_normal(shape).astype(dt)
    a[0:28, 0:28] = -0.0
    a[0:28, 28:56] = rng.integers(1, 2000, size=(28, 28)).astype(dt) * np.finfo(dt).smallest_subnormal
    a[33:35, 52:54] = np.finfo(dt).max
    a[39, 0], a[39, 35], a[39, 69] = np.inf, -np.inf, np.nan
    a.setflags(write=False)
    return a


def tiny_image(dtype, shape=(40, 70)):
    """1e-42 (float32) or 1e-310 (float64) everywhere, with a few negative subnormals: every output is subnormal."""
    dt = np.dtype(dtype)
    a = np.full(shape, 1e-42 if dt == np.float32 else 1e-310, dt)
    a[3, 5], a[20, 33], a[39, 69], a[17, 0] = -a[0, 0], -3 * a[0, 0], -np.finfo(dt).smallest_subnormal, -a[0, 0] / 2
    a.setflags(write=False)
    return a


def same_but_for_nan_bits(a, b):
    """NaN at the same positions and equal bytes everywhere else (-0.0 is not +0.0).  Sign and payload of a NaN are not compared."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind != "f":
        return a.tobytes() == b.tobytes()
    na, nb = np.isnan(a), np.isnan(b)
    cells = "u%d" % a.itemsize
    return bool(np.array_equal(na, nb)) and a.view(cells)[~na].tobytes() == b.view(cells)[~nb].tobytes()


def correlate_sym_1d(a, w, axis, mode="reflect", cval=0.0, arithmetic="scipy", out_dtype=None):
    """One pass along `axis` of the 2-D array `a` with the 2 r + 1 symmetric weights `w`; the result has a's dtype (or `out_dtype`).

    `arithmetic` other than "scipy" is a deliberately wrong pass for the tests (tests/test_gaussian_reference_cpu.py holds each one
    to be visible on the data the GPU suite uses): "reversed" sums the taps from j = -1 down to -r, "unpaired" adds lo w and hi w
    separately, "fused" does each tmp += s w as one fused multiply-add, "round_half" rounds an integer result to nearest instead of
    truncating it, "cval_cast" casts cval to the element type.  ("unrounded_between" is gaussian_filter's.)"""
    assert arithmetic in ARITHMETICS
    out_dtype = a.dtype if out_dtype is None else np.dtype(out_dtype)
    r = len(w) // 2
    n = a.shape[axis]
    idx = extend_index(np.arange(-r, n + r), n, mode)
    e = np.take(a.astype(np.float64), np.maximum(idx, 0), axis=axis)
    outside = idx < 0
    if outside.any():
        with np.errstate(invalid="ignore"):
            fill = float(np.float64(cval).astype(a.dtype)) if arithmetic == "cval_cast" else float(cval)
        if axis == 0:
            e[outside, :] = fill
        else:
            e[:, outside] = fill
    e = np.moveaxis(e, axis, 0)                       # (n + 2 r, other)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        tmp = e[r:r + n] * w[r]
        for j in (range(-1, -r - 1, -1) if arithmetic == "reversed" else range(-r, 0)):
            lo, hi = e[r + j:r + j + n], e[r - j:r - j + n]
            if arithmetic == "unpaired":
                tmp += lo * w[r + j]
                tmp += hi * w[r + j]
            elif arithmetic == "fused":
                tmp = fma(lo + hi, w[r + j], tmp)
            else:
                tmp += (lo + hi) * w[r + j]
        if arithmetic == "round_half" and out_dtype.kind in "iu":
            tmp = np.rint(tmp)
        return np.moveaxis(tmp, 0, axis).astype(out_dtype)


def gaussian_filter(a, sigma, mode="reflect", cval=0.0, truncate=4.0, radius=None, arithmetic="scipy"):
    """`arithmetic` = "unrounded_between" keeps the result of the first pass in float64 instead of rounding it to the element type;
    the other names are correlate_sym_1d's."""
    a = np.asarray(a)
    sigmas = (sigma, sigma) if np.ndim(sigma) == 0 else tuple(sigma)
    radii = (radius, radius) if radius is None or np.ndim(radius) == 0 else tuple(radius)
    between = np.float64 if arithmetic == "unrounded_between" else a.dtype
    out = a.copy()
    for axis in (0, 1):
        if sigmas[axis] > 1e-15:
            out = correlate_sym_1d(out, gaussian_weights(sigmas[axis], truncate, radii[axis]), axis, mode, cval, arithmetic,
                                   out_dtype=between if axis == 0 and sigmas[1] > 1e-15 else a.dtype)
    return out
