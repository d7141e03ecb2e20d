"""The two definitions behind ``discorpy_amd.prep.threshold`` restated in NumPy, operation by operation: the arithmetic contracts of
dcp_sort_plane_2d and dcp_zoom_cubic_nearest_1d ("Sort and windowed zoom").  tests/test_threshold_cpu.py holds
zoom_reference against scipy.ndimage.zoom itself; the GPU kernels are held to this file by ``==``.

    sort     every element becomes an unsigned integer whose order is the order of the values (unsigned as it is, signed with the sign
             bit flipped, floats as u ^ (sign ? ~0 : signbit) after a NaN has lost its sign bit, so NaNs of either sign are the largest
             keys); the keys are sorted and turned back.  -0.0 comes before +0.0, NaNs come last in the order of their payloads, and a
             negative NaN comes out positive with its payload kept.

    zoom     scipy.ndimage.zoom(src, out_n / n, order=3, mode="nearest") of a 1-D array, scipy 1.15:
               line      the n samples extended by 12 copies of the edge value per side (an index clamp), N = n + 24, as doubles, each
                         multiplied by the gain (1 - z)(1 - 1 / z), z = sqrt(3) - 2
               causal    c[0] = s z / (1 - z^N z^N) + x[0], s = x[0] + z^N x[N - 1] + sum_{i >= 1} z^i (x[i] + z^N x[N - 1 - i]) with z^i
                         by repeated multiplication and z^N = pow(z, N) (scipy runs the sum to N - 1 and reads its own partial sum
                         where i = N - 1 wants x[0]; here it stops after HORIZON terms); c[i] = x[i] + z c[i - 1]
               anti      c[N - 1] *= z / (z - 1); c[i] = z (c[i + 1] - c[i])
               sample    at cc = j zoom + 12, zoom = (n - 1) / (out_n - 1) (1 for out_n = 1): taps floor(cc) - 1 .. + 2, scipy's cubic
                         weights in scipy's expressions, t = 0; t += c w per tap in ascending order
               store     floats by a cast, integers rounded half away from zero and clamped (unsigned: t > 0 ? t + 0.5 : 0)
             WINDOW: an output point does not need the whole line.  Its causal recursion starts WINDOW samples in front of its first
             tap from c = x (or from scipy's initial value where that reaches the line's start), its anticausal recursion WINDOW
             samples behind its last tap from 0 (or from scipy's value at the line's end).  A start-up error decays by |z| per sample:
             |z|^64 is about 2^-121 of the window's magnitude, far below one float64 rounding of the coefficients.
"""
import math

import numpy as np

PAD = 12
WINDOW = 64          # samples in front of the first and behind the last tap
HORIZON = 128        # terms of the causal initial sum (all of them for N - 1 <= HORIZON)
POLE = math.sqrt(3.0) - 2.0


# ------------------------------------------------------------------ sort

def sort_keys(a):
    """Order-preserving unsigned keys of the flattened array (see the module's text)."""
    a = np.ascontiguousarray(a).reshape(-1)
    bits = a.dtype.itemsize * 8
    u = a.view("u%d" % a.dtype.itemsize)
    sign = u.dtype.type(1 << (bits - 1))
    if a.dtype.kind == "u":
        return u.copy()
    if a.dtype.kind == "i":
        return u ^ sign
    assert a.dtype.kind == "f"
    u = np.where(np.isnan(a), u & ~sign, u)
    return np.where(u & sign != 0, ~u, u ^ sign)


def sort_elements(keys, dtype):
    dtype = np.dtype(dtype)
    bits = dtype.itemsize * 8
    sign = keys.dtype.type(1 << (bits - 1))
    if dtype.kind == "u":
        return keys.view(dtype)
    if dtype.kind == "i":
        return (keys ^ sign).view(dtype)
    return np.where(keys & sign != 0, keys ^ sign, ~keys).view(dtype)


def sort_reference(a):
    """What dcp_sort_plane_2d writes for the plane ``a``, bit for bit."""
    a = np.asarray(a)
    return sort_elements(np.sort(sort_keys(a)), a.dtype)


# ------------------------------------------------------------------ zoom

def zoom_length(n, zoom):
    """The output length scipy.ndimage.zoom computes for a line of n samples."""
    return int(round(n * zoom))


def _store(t, dtype):
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        return t.astype(dtype)
    info = np.iinfo(dtype)
    if dtype.kind == "u":
        th = np.where(t > 0, t + 0.5, 0.0)
    else:
        th = np.where(t > 0, t + 0.5, t - 0.5)
    th = np.where(th > float(info.max), float(info.max), th)
    th = np.where(th < float(info.min), float(info.min), th)
    if dtype.itemsize == 8:          # the clamp's double is 2^63 / 2^64: out of the C cast's range (the tests stay below)
        return np.trunc(th).astype(np.longdouble).astype(dtype)
    return np.trunc(th).astype(dtype)


def zoom_reference(src, out_n, window=WINDOW, horizon=HORIZON):
    """What dcp_zoom_cubic_nearest_1d writes: see the module's text.  ``window=None``: the whole line for every point, scipy's own way."""
    src = np.ascontiguousarray(src).reshape(-1)
    n, out_n = int(src.shape[0]), int(out_n)
    assert n >= 1 and out_n >= 1
    N = n + 2 * PAD
    if window is None:
        window = horizon = N
    z = POLE
    gain = (1.0 - z) * (1.0 - 1.0 / z)
    z_n = z ** N          # (Python's float power is the C library's pow, as scipy's is)
    line = src.astype(np.float64)

    def x(i):          # the gained sample at extended index i (an array of indices)
        return line[np.clip(i - PAD, 0, n - 1)] * gain

    zoom = (n - 1) / (out_n - 1) if out_n > 1 else 1.0
    cc = np.arange(out_n, dtype=np.float64) * zoom + float(PAD)
    fl = np.floor(cc)
    s = fl.astype(np.int64) - 1          # first tap
    lo = np.maximum(s - window, 0)
    hi = np.minimum(s + 3 + window, N - 1)
    span = int((hi - s).max()) + 1
    causal = np.zeros((span, out_n))          # causal[k] = c+[s + k]

    # the initial value at the line's start, for the points whose window reaches it
    first = lo == 0
    zero = np.zeros(out_n, dtype=np.int64)
    x0 = x(zero)
    acc = x0 + z_n * x(zero + N - 1)
    z_i = z
    for i in range(1, min(N - 1, horizon) + 1):
        far = acc if N - 1 - i == 0 else x(zero + N - 1 - i)
        acc = acc + z_i * (x(zero + i) + z_n * far)
        z_i *= z
    start = acc * (z / (1.0 - z_n * z_n)) + x0
    t = np.where(first, start, 0.0)
    # causal recursion, every point in step: sample lo + k at step k
    steps = int((hi - lo).max()) + 1
    for k in range(steps):
        i = lo + k
        live = i <= hi
        new = np.where(first & (k == 0), start, x(np.minimum(i, N - 1)) + z * t)
        t = np.where(live, new, t)
        slot = i - s
        put = live & (slot >= 0)
        causal[slot[put], np.nonzero(put)[0]] = t[put]
    # anticausal recursion from hi down to s
    last = hi == N - 1
    c = np.zeros((4, out_n))
    t = np.zeros(out_n)
    for k in range(span - 1, -1, -1):
        i = s + k
        live = i <= hi
        cp = causal[k]
        new = np.where(last & (i == N - 1), cp * (z / (z - 1.0)), z * (t - cp))
        t = np.where(live, new, t)
        if k < 4:
            c[k] = t
    y = cc - fl
    zz = 1.0 - y
    w1 = (y * y * (y - 2.0) * 3.0 + 4.0) / 6.0
    w2 = (zz * zz * (zz - 2.0) * 3.0 + 4.0) / 6.0
    w0 = zz * zz * zz / 6.0
    w3 = 1.0 - w0 - w1 - w2
    tt = np.zeros(out_n)
    for k, w in enumerate((w0, w1, w2, w3)):
        tt = tt + c[k] * w
    return _store(tt, src.dtype)


# n -> out_n pairs of the tests: one sample, whole-line windows, either side of the 12-sample extension, windows that just stop touching
# the ends, long lines, and zoom 1
LENGTHS = [(1, 1), (2, 2), (5, 3), (13, 13), (24, 7), (25, 7), (130, 9), (1961, 53), (67591, 263), (263, 263)]


def zoom_case(n, dtype, seed=0):
    """A sorted line of n samples of ``dtype`` with plateaus, steps and both signs where the type has them."""
    rng = np.random.default_rng(1000 + seed + n)
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        v = rng.standard_normal(n) * 100.0
        v[rng.random(n) < 0.2] = 3.25
        return np.sort(v.astype(dtype))
    info = np.iinfo(dtype)
    lo, hi = max(info.min, -(2 ** 40)), min(info.max, 2 ** 40)
    return np.sort(rng.integers(lo, hi, n, dtype=np.int64, endpoint=True).astype(dtype))
