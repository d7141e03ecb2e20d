"""scipy.ndimage.gaussian_filter for 2-D input restated in NumPy, operation by operation: the arithmetic contract of
dcp_correlate_sym_2d ("The Gaussian filter").  tests/test_gaussian_reference_cpu.py holds it np.array_equal to scipy; the
GPU kernels are held to scipy directly, so this file is the written-down form of what they must do, checked on the CPU.

    weights      x = arange(-r, r + 1); phi = exp(-0.5 / sigma^2 * x^2); phi / phi.sum(), r = int(truncate * sigma + 0.5)
    one element  tmp = e[i] w[r]; for j = -r .. -1: tmp += (e[i + j] + e[i - j]) w[r + j]      (float64, one rounding per operation)
    extension    reflect / mirror / nearest / wrap fold the index (any number of folds); constant is the double cval
    axes         axis 0, then axis 1 on the first result cast to the element type; sigma <= 1e-15 skips an axis
    cast         floats round to nearest, integers truncate toward zero (NumPy's astype from float64 is the same C cast)
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


def correlate_sym_1d(a, w, axis, mode="reflect", cval=0.0):
    """One pass along `axis` of the 2-D array `a` with the 2 r + 1 symmetric weights `w`; the result has a's dtype."""
    r = len(w) // 2
    n = a.shape[axis]
    idx = extend_index(np.arange(-r, n + r), n, mode)
    e = np.take(a.astype(np.float64), np.maximum(idx, 0), axis=axis)
    outside = idx < 0
    if outside.any():
        if axis == 0:
            e[outside, :] = float(cval)
        else:
            e[:, outside] = float(cval)
    e = np.moveaxis(e, axis, 0)                       # (n + 2 r, other)
    tmp = e[r:r + n] * w[r]
    for j in range(-r, 0):
        tmp += (e[r + j:r + j + n] + e[r - j:r - j + n]) * w[r + j]
    with np.errstate(invalid="ignore"):
        return np.moveaxis(tmp, 0, axis).astype(a.dtype)


def gaussian_filter(a, sigma, mode="reflect", cval=0.0, truncate=4.0, radius=None):
    a = np.asarray(a)
    sigmas = (sigma, sigma) if np.ndim(sigma) == 0 else tuple(sigma)
    radii = (radius, radius) if radius is None or np.ndim(radius) == 0 else tuple(radius)
    out = a.copy()
    for axis in (0, 1):
        if sigmas[axis] > 1e-15:
            out = correlate_sym_1d(out, gaussian_weights(sigmas[axis], truncate, radii[axis]), axis, mode, cval)
    return out
