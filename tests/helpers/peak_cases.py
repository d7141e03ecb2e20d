"""Seeded rows for the peak search of csrc/profile_kernels.hip (peak_rows_kernel), shared by tests/test_peak_rows_cpu.py and
tests/test_peak_steps_gpu.py.  Every builder returns ``(row, radius, sensitive)`` tuples; the rows are read-only.  They are shaped
by the kernel, not by the data it usually sees: a row's workgroup walks it in steps of ``TILE`` samples from ``lo = radius`` to
``hi = L - radius - 1``, stages ``radius`` more samples on both sides of a step, lists the step's candidates by ballot, rank-sorts
every candidate's window in a wave and takes NumPy's pairwise mean of its ``radius`` largest elements.

* :func:`step_rows`      1 to 5 steps whose last one holds 1 or 256 samples, minima on the first and the last sample of every step
* :func:`crowded_rows`   every sample a candidate, every sample a point
* :func:`ladder_rows`    full-mantissa tails of every length at which the pairwise sum takes another path, thresholds that are the
  restated ``num2`` values themselves, so that one ulp of the mean moves a point in or out
* :func:`special_rows`   infinities, signed zeros, subnormals, NaN at the window's edge, a mean of exactly 0
"""
import functools
import math

import numpy as np

import peaks_reference as PR

TILE = 256
DTYPES = ("float32", "float64")


def search_range(length, radius):
    """(lo, hi): the samples ``range(lo, hi)`` are searched."""
    return radius, length - radius - 1


def frozen(row):
    row = np.ascontiguousarray(row)
    row.setflags(write=False)
    return row


# --------------------------------------------------------------------------- step rows

STEP_RADII = (1, 11, 128)
STEP_SPANS = (256, 257, 512, 513, 769, 1025)          # hi - lo: 1, 2, 2, 3, 4, 5 steps, the last of 256, 1, 256, 1, 1, 1 samples
STEP_COUNT = {256: 1, 257: 2, 512: 2, 513: 3, 769: 4, 1025: 5}
STEP_SENSITIVE = 0.1


def step_length(radius, span):
    return span + 2 * radius + 1


def constructed_row(radius, span, dtype, decoys=True):
    """(row, expected positions): a background of 5.0 and minima of 1.0 on the first and the last searched sample and on the last
    sample of every step but the last, the first sample of the next and the one after it.  A planted sample is a point iff nothing
    within ``radius`` samples of it is lower and the ``radius`` largest samples of its window are background (their mean is 5.0,
    ``num2`` is 0.8 or 0.9; at a radius of 1 the middle one of three minima has itself as its mean and is no point), so

    * a 0.5 exactly ``radius`` samples before the last sample of step 0 takes that minimum away, the minima behind it stay;
    * a 0.5 ``radius + 1`` samples before the last sample of step 1 takes nothing away;
    * both are lower than everything around them and are points themselves;
    * ``decoys``: 0.25 on ``lo - 1`` and on ``hi``, outside the searched range, are never points and take away every minimum and
      every 0.5 within ``radius`` samples of them (the minima on ``lo`` and ``hi - 1`` always).
    The two 0.5 are planted where the row has two step boundaries; the expected positions are written out here, rule by rule."""
    length = step_length(radius, span)
    lo, hi = search_range(length, radius)
    row = np.full(length, 5.0)
    firsts = [lo + TILE * k for k in range(1, STEP_COUNT[span])]           # the first sample of steps 1, 2, ...
    assert all(lo < f < hi for f in firsts) and lo + TILE * STEP_COUNT[span] >= hi
    minima = {lo, hi - 1}
    for f in firsts:
        minima |= {p for p in (f - 1, f, f + 1) if p < hi}
    expected = set(minima)
    lower = []                                        # (position, value) of everything below the minima
    if len(firsts) >= 2:
        kills, spares = firsts[0] - 1 - radius, firsts[1] - 1 - (radius + 1)
        assert lo <= kills and kills not in minima and spares not in minima
        lower += [(kills, 0.5), (spares, 0.5)]
        expected |= {kills, spares}
    if decoys:
        lower += [(lo - 1, 0.25), (hi, 0.25)]
    for q, value in lower:
        expected -= {p for p in expected if abs(p - q) <= radius and (1.0 if p in minima else 0.5) > value}
    if radius == 1:                                   # the middle of three minima: its window is flat, its mean its own value, num2 is 0
        expected -= {f for f in firsts if f + 1 < hi}
    for p in minima:
        row[p] = 1.0
    for q, value in lower:
        row[q] = value
    return frozen(row.astype(dtype)), np.asarray(sorted(expected), np.int64)


@functools.lru_cache(maxsize=None)
def step_rows(dtype):
    """Per (radius, span): (a) small integers, (b) cosine plus noise, (c) the constructed row and (d) the constructed row without its
    decoys (there the minima on ``lo`` and ``hi - 1`` are points)."""
    rng = np.random.default_rng(2751)
    out = []
    for radius in STEP_RADII:
        for span in STEP_SPANS:
            length = step_length(radius, span)
            x = np.arange(length)
            out.append((frozen(rng.integers(1, 4, length).astype(dtype)), radius, STEP_SENSITIVE))
            out.append((frozen((2.0 + np.cos(x * 2 * np.pi / 37.3) + 0.05 * rng.standard_normal(length)).astype(dtype)), radius, STEP_SENSITIVE))
            out.append((constructed_row(radius, span, dtype)[0], radius, STEP_SENSITIVE))
            out.append((constructed_row(radius, span, dtype, decoys=False)[0], radius, STEP_SENSITIVE))
    return out


def constructed_cases(dtype):
    """((row, radius, sensitive), expected positions) of every constructed row."""
    return [((row, radius, STEP_SENSITIVE), expected) for radius in STEP_RADII for span in STEP_SPANS for decoys in (True, False)
            for row, expected in [constructed_row(radius, span, dtype, decoys)]]


# --------------------------------------------------------------------------- crowded rows

CROWDED_LENGTH = 1300
CROWDED_RADII = (1, 128)


@functools.lru_cache(maxsize=None)
def crowded_rows(dtype):
    """A constant row and a row of two levels (blocks of 3.0 and 2.0, 1 to 9 samples long): every sample of the first and most of
    the second are candidates, 256 of them in a step.  ``sensitive = 0.1`` accepts none of the constant row (``num2`` is exactly 0),
    ``sensitive = -1.0`` accepts every candidate."""
    rng = np.random.default_rng(2752)
    flat = frozen(np.full(CROWDED_LENGTH, 3.0, dtype))
    levels = np.empty(0)
    while len(levels) < CROWDED_LENGTH:
        levels = np.concatenate([levels, np.full(rng.integers(1, 10), 3.0 if len(levels) == 0 or levels[-1] == 2.0 else 2.0)])
    levels = frozen(levels[:CROWDED_LENGTH].astype(dtype))
    return [(row, radius, sensitive) for radius in CROWDED_RADII for row in (flat, levels) for sensitive in (0.1, -1.0)]


# --------------------------------------------------------------------------- mean ladder

LADDER_RADII = (2, 3, 7, 8, 9, 15, 16, 17, 23, 24, 25, 63, 64, 65, 127, 128)
LADDER_K = 24
LADDER_RANKS = (6, 12, 18)                            # the thresholds: the 6th, 12th and 18th smallest num2 of the row

# one seed per row, searched (tests/test_peak_rows_cpu.py: test_ladder_sees_the_order_of_the_sum says what a seed has to give)
LADDER_SEEDS = {
    (2, "float32"): 1, (3, "float32"): 356, (7, "float32"): 31, (8, "float32"): 135, (9, "float32"): 1551, (15, "float32"): 333,
    (16, "float32"): 21, (17, "float32"): 229, (23, "float32"): 131, (24, "float32"): 106, (25, "float32"): 167, (63, "float32"): 6,
    (64, "float32"): 12, (65, "float32"): 25, (127, "float32"): 10, (128, "float32"): 44,
    (2, "float64"): 1, (3, "float64"): 9521, (7, "float64"): 141, (8, "float64"): 455, (9, "float64"): 363, (15, "float64"): 3184,
    (16, "float64"): 15, (17, "float64"): 175, (23, "float64"): 599, (24, "float64"): 2, (25, "float64"): 29, (63, "float64"): 28,
    (64, "float64"): 75, (65, "float64"): 124, (127, "float64"): 9, (128, "float64"): 55,
}


def ladder_length(radius):
    return (2 * radius + 1) * LADDER_K + 1


def ladder_positions(radius):
    return radius + (2 * radius + 1) * np.arange(LADDER_K)


def ladder_row(radius, dtype, seed):
    """A background of 2 + 2 U[0, 1) with one minimum of 1 + 0.5 U[0, 1) in every window: the candidates are the planted minima."""
    rng = np.random.default_rng(seed)
    row = 2.0 + 2.0 * rng.random(ladder_length(radius))
    row[ladder_positions(radius)] = 1.0 + 0.5 * rng.random(LADDER_K)
    return frozen(row.astype(dtype))


def mean_left_to_right(top):
    T = top.dtype.type
    res = T(0)
    for v in top:
        res = T(res + v)
    return T(res / T(len(top)))


def mean_descending(top):
    return mean_left_to_right(top[::-1])


def mean_widened(top):
    """The sum in a wider accumulator, rounded once: float64 for float32 terms, exact for float64 terms."""
    T = top.dtype.type
    if T is np.float32:
        res = np.float64(0)
        for v in top:
            res = res + np.float64(v)
        return T(T(res) / T(len(top)))
    return T(T(math.fsum(float(v) for v in top)) / T(len(top)))


WRONG_MEANS = (("left to right", mean_left_to_right), ("descending", mean_descending), ("widened", mean_widened))


def num2_values(row, radius, positions, mean=PR.tail_mean):
    """``num2`` of the search at ``positions`` under ``mean``, every operation in the row's type."""
    T = row.dtype.type
    out = []
    for i in positions:
        top = np.sort(row[i - radius:i + radius + 1], kind="stable")[-radius:]
        m = mean(top)
        out.append(np.abs(T(T(row[i] - m) / m)))
    return np.asarray(out, row.dtype)


@functools.lru_cache(maxsize=None)
def ladder_thresholds(radius, dtype):
    """(row, its num2 values, the thresholds of LADDER_RANKS)."""
    row = ladder_row(radius, dtype, LADDER_SEEDS[radius, dtype])
    num2 = num2_values(row, radius, ladder_positions(radius))
    ranked = np.sort(num2)
    return row, num2, tuple(ranked[k - 1] for k in LADDER_RANKS)


@functools.lru_cache(maxsize=None)
def ladder_rows(dtype):
    """Every threshold as a Python float (compared in the row's type) and, for float32 rows, as a NumPy float64 scalar as well
    (the comparison is promoted).  A planted minimum is a point iff its num2 is strictly greater."""
    out = []
    for radius in LADDER_RADII:
        row, _, thresholds = ladder_thresholds(radius, dtype)
        for t in thresholds:
            out.append((row, radius, float(t)))
            if dtype == "float32":
                out.append((row, radius, np.float64(t)))
    return out


# --------------------------------------------------------------------------- special values

@functools.lru_cache(maxsize=None)
def special_rows(dtype):
    T = np.dtype(dtype).type
    rng = np.random.default_rng(2753)
    out = []

    def add(row, radius, sensitive):
        out.append((frozen(np.array(row, dtype)), radius, sensitive))

    base = np.full(24, 5.0)
    base[[6, 14]] = 1.0
    row = base.copy()
    row[7] = np.inf                                   # in the tail of the minimum at 6: its mean is inf, num2 is NaN
    add(row, 2, 0.1)
    row = base.copy()
    row[6] = -np.inf                                  # the minimum itself: inf - inf is NaN, not 0
    add(row, 2, 0.1)
    row[15] = np.inf
    add(row, 3, -1.0)
    row = np.full(24, -9.0)
    row[8:13] = [-1.0, -2.0, -5.0, -3.0, 1.0]         # the tail of the minimum at 10 is {-1, +1}: a mean of exactly 0
    add(row, 2, 0.0)
    add(row, 2, -1.0)
    x = np.arange(300)
    negative = -(1.5 + np.cos(x * 2 * np.pi / 37.3) + 0.02 * rng.standard_normal(300))
    add(negative, 5, 0.05)                            # every mean is negative: the absolute value
    add(negative, 11, 0.1)
    zeros = np.zeros(64)
    zeros[rng.choice(64, 20, replace=False)] = -0.0
    add(zeros, 2, 0.0)
    add(zeros, 2, -1.0)
    zeros[[9, 10, 30, 47, 48, 49]] = 1.0              # tails with a mean above 0 around minima of either zero
    add(zeros, 2, 0.1)
    add(zeros, 3, -1.0)
    if dtype == "float32":
        tiny = float(np.finfo(np.float32).smallest_subnormal)
        sub = (3000.0 + 2000.0 * rng.random(96)) * tiny
        sub[[7, 30, 31, 60, 88]] = np.array([1000.0, 1.0, 1.0, 0.0, 500.0]) * tiny
        assert T(sub.max()) < np.finfo(np.float32).tiny
        add(sub, 3, 0.1)
        add(sub, 11, 0.1)
    for radius in (3, 11):
        length = 12 * radius + 4
        row = np.full(length, 5.0) + rng.random(length)
        m = [3 * radius, 5 * radius + 2, 7 * radius + 4, 9 * radius + 6]
        row[m] = 1.0
        row[m[0] - radius] = np.nan                   # in the window's first sample: no point
        row[m[1] - radius - 1] = np.nan               # one before it: a point
        row[m[2] + radius] = np.nan                   # in the window's last sample: no point
        row[m[3] + radius + 1] = np.nan               # one behind it: a point
        assert m[3] + radius + 1 < length and m[3] < search_range(length, radius)[1]
        add(row, radius, 0.1)
    return out


def all_rows(dtype):
    return step_rows(dtype) + crowded_rows(dtype) + ladder_rows(dtype) + special_rows(dtype)


@functools.lru_cache(maxsize=None)
def expected_positions(kind, dtype, index):
    """``PR.local_minima`` of row ``index`` of builder ``kind``, computed once."""
    row, radius, sensitive = BUILDERS[kind](dtype)[index]
    got = PR.local_minima(row, radius, sensitive)
    got.setflags(write=False)
    return got


BUILDERS = {"step": step_rows, "crowded": crowded_rows, "ladder": ladder_rows, "special": special_rows}
