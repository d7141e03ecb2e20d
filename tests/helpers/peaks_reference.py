"""NumPy restatements of what csrc/profile_kernels.hip computes, operation by operation (no GPU, no reference needed).

* :func:`pairwise_sum` / :func:`tail_mean`   NumPy's own ``np.add.reduce`` / ``np.mean`` over at most 128 contiguous elements, spelled
  out: below 8 terms a running sum from 0, else eight interleaved accumulators, their fixed tree, then the remaining terms
* :func:`local_minima`   the search loop of ``get_local_extrema_points`` with that mean; every operation in the row's type
* :func:`subpixel_offset` / :func:`refine`   the parabola through three samples in closed form, float64
* :func:`window_slope`   the closed form of ``sliding_window_slope`` before its normalisation
"""
import numpy as np


def pairwise_sum(a):
    """``np.add.reduce(a)`` for a contiguous 1-D float array of at most 128 elements, one rounded addition at a time."""
    a = np.asarray(a)
    n, T = len(a), a.dtype.type
    assert n <= 128
    if n < 8:
        res = T(0)
        for v in a:
            res = T(res + v)
        return res
    r = [a[j] for j in range(8)]
    i = 8
    while i < n - (n % 8):
        for j in range(8):
            r[j] = T(r[j] + a[i + j])
        i += 8
    res = T(T(T(r[0] + r[1]) + T(r[2] + r[3])) + T(T(r[4] + r[5]) + T(r[6] + r[7])))
    while i < n:
        res = T(res + a[i])
        i += 1
    return res


def tail_mean(sorted_tail):
    """``np.mean`` of it: the pairwise sum, then one division by the count, in the array's type."""
    T = np.asarray(sorted_tail).dtype.type
    return T(pairwise_sum(sorted_tail) / T(len(sorted_tail)))


def local_minima(row, radius, sensitive):
    """Integer positions of the minima search (``linepattern.py:254-262`` of the reference) on a float32 / float64 row."""
    row = np.asarray(row)
    T = row.dtype.type
    num_point = len(row)
    points = []
    with np.errstate(all="ignore"):
        for i in range(radius, num_point - radius - 1):
            window = row[i - radius:i + radius + 1]
            if np.isnan(window).any():
                continue
            val = row[i]
            if not (T(window.min() - val) == 0.0):
                continue
            top = np.sort(window, kind="stable")[-radius:]        # ([-0:] is the whole window: a radius of 0)
            nmean = tail_mean(top)
            num2 = np.abs(T(T(val - nmean) / nmean)) if nmean != 0 else T(0)
            if num2 > sensitive:
                points.append(i)
    return np.asarray(points, dtype=np.int64)


def subpixel_offset(d0, d1, d2):
    """Position in [0, 3) of the minimum of the parabola through (0, d0), (1, d1), (2, d2); the argmin where there is none."""
    d0, d1, d2 = np.float64(d0), np.float64(d1), np.float64(d2)
    with np.errstate(all="ignore"):
        a = (d0 - 2.0 * d1 + d2) / 2.0
        b = (-3.0 * d0 + 4.0 * d1 - d2) / 2.0
        off = np.float64(np.argmin([d0, d1, d2]))
        if a != 0.0:
            num = -b / (2.0 * a)
            if num >= 0.0 and num < 3.0:
                off = num
    return off


def refine(row, points):
    """Sub-pixel positions of integer ``points`` of ``row``: ``i - 1 + subpixel_offset(row[i - 1 : i + 2])``, float64."""
    return np.asarray([np.float64(i - 1) + subpixel_offset(row[i - 1], row[i], row[i + 1]) for i in points], dtype=np.float64)


def window_slope(row, size):
    """``|slope|`` of the least-squares line through the ``size`` (odd) samples around every sample of the edge-padded row: products
    and sum in float64 (k ascending, from 0.0), the quotient rounded to the row's type, then the absolute value."""
    row = np.asarray(row)
    r = size // 2
    padded = np.pad(row, (r, r), "edge").astype(np.float64)
    den = np.float64(sum(float(k * k) for k in range(-r, r + 1)))
    acc = np.zeros(len(row))
    for k in range(size):
        acc = acc + np.float64(k - r) * padded[k:k + len(row)]
    return np.abs((acc / den).astype(row.dtype))
