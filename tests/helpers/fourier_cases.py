"""Geometry, integer tap tables and exact references for the tests of the Fourier Gaussian filter (dcp_fourier_gauss_2d,
discorpy_amd/csrc/fourier_kernels.hip, api_fourier.cpp).  NumPy only.

Why integer tables: with the Gaussian tables of prep._fourier_taps the taps at |d| = R are, by construction of the support bound, below
2^-56 of the table, so a window one or three indices too short, a leftover loop that stops one step early or a tap index taken as
a(k - j) changes the result by less than any tolerance can see.  The C ABI takes any table, and api_fourier.cpp derives the support from
it: taps with |d| <= R or |d| >= N - R, R the smallest radius at which the taps left out sum to at most 2^-56 of the table.  A table whose
kept taps are small nonzero integers and whose other taps are exact zeros has exactly the radius it was built with, and with integer
images every product and every partial sum of the two passes is an integer below 2^53: the float64 multiply-add chain is exact in any
order, and the result equals an integer Toeplitz product BIT FOR BIT (dense_exact, which asserts the 2^53 condition).

ROWS, STEPS and BLOCK are kFourierRows (dcp_internal.h), kFourierSteps and kFourierBlock (fourier_kernels.hip) as the case tables below
assume them; tests/test_fourier_gauss_cpu.py pins them to the sources and asserts, for every case, the conditions that make it the case
its name claims.
"""
import functools

import numpy as np

ROWS, STEPS, BLOCK = 8, 8, 256


# --------------------------------------------------------------------------- the kernels' run logic restated

def runs(o0, R, N):
    """fourier_runs of fourier_kernels.hip: (branch, [(a0, b0), (a1, b1)]) for the outputs o0 .. o0 + ROWS - 1 (padded coordinates)
    at radius R on an axis of N indices.  The second run is (0, -1), empty, where the window is one run."""
    lo, hi = o0 - R, o0 + ROWS - 1 + R
    if hi - lo + 1 >= N:
        return "all", [(0, N - 1), (0, -1)]
    if lo < 0:
        return "below", [(0, hi), (lo + N, N - 1)]
    if hi > N - 1:
        return "above", [(0, hi - N), (lo, N - 1)]
    return "one", [(lo, hi), (0, -1)]


def branches(side, pad, R):
    """runs() of every block of ROWS outputs of a cropped axis of `side` elements padded by `pad`."""
    return [runs(pad + b, R, side + 2 * pad) for b in range(0, side, ROWS)]


def geometry(side, pad, R):
    """What an axis does at radius R: the set of branches its blocks take, the lengths modulo STEPS of its `one` runs and of all its
    runs, the gaps between the two runs of its wrapped blocks, and whether a block's last outputs read the zeros behind the table."""
    N = side + 2 * pad
    out = dict(N=N, branches=set(), one_left=set(), left=set(), gaps=set(), tail=False)
    for b, (name, rr) in zip(range(0, side, ROWS), branches(side, pad, R)):
        out["branches"].add(name)
        for a, e in rr:
            if a <= e:
                out["left"].add((e - a + 1) % STEPS)
                if name == "one":
                    out["one_left"].add((e - a + 1) % STEPS)
        if name in ("below", "above"):
            out["gaps"].add(rr[1][0] - rr[0][1] - 1)
        # entry (o0 + ROWS - 1) - k + N - 1 of a table of 2 N - 1 is read at the smallest k of the block's runs
        first = min(a for a, e in rr if a <= e)
        out["tail"] = out["tail"] or (pad + b + ROWS - 1) - first + N - 1 > 2 * N - 2
    return out


def support_radius(re, im, n):
    """support_radius of api_fourier.cpp: the smallest r such that the taps with r < |d| < n - r sum to at most 2^-56 of the table."""
    mid, r, dropped = n - 1, n // 2, 0.0
    allowed = np.ldexp(float((np.abs(re) + np.abs(im)).sum()), -56)

    def mag(k):
        return abs(re[mid + k]) + abs(im[mid + k]) + abs(re[mid - k]) + abs(im[mid - k])
    while r > 0:
        more = mag(r) + (mag(n - r) if n - r != r else 0.0)
        if not dropped + more <= allowed:
            break
        dropped += more
        r -= 1
    return r


def taps_kept(n, r):
    """The count the launcher reports in dcp_debug_last_kernel: 4 r + 1, or the whole table once 2 r + 1 >= n."""
    return 2 * n - 1 if 2 * r + 1 >= n else 4 * r + 1


# --------------------------------------------------------------------------- tables

WHERE = ("both", "near", "wrapped", "negative", "positive")


def integer_table(n, r, rng, where="both"):
    """(re, im), 2 n - 1 float64 each, index d + n - 1 holding a(d): nonzero integers in [-8, 8] on the part of the support
    {|d| <= r or |d| >= n - r} that `where` selects, exact zeros elsewhere.  The selected taps include |d| = r or |d| = n - r, and every
    selected tap is nonzero, so that support_radius gives back exactly r (r <= n // 2)."""
    assert where in WHERE and 0 <= r <= n // 2
    d = np.arange(-(n - 1), n)
    near, wrapped = np.abs(d) <= r, np.abs(d) >= n - r
    keep = {"both": near | wrapped, "near": near, "wrapped": wrapped, "negative": (near | wrapped) & (d < 0),
            "positive": (near | wrapped) & (d > 0)}[where]
    out = []
    for _ in range(2):
        v = rng.integers(1, 8, size=d.size, endpoint=True) * rng.choice([-1, 1], size=d.size)
        out.append(np.where(keep, v, 0).astype(np.float64))
    return out[0], out[1]


def delta_table(n, d, imaginary=False):
    """a(d) = 1 (or i) and nothing else."""
    re, im = np.zeros(2 * n - 1), np.zeros(2 * n - 1)
    (im if imaginary else re)[d + n - 1] = 1.0
    return re, im


def toeplitz(table, n):
    """A[j, k] = a(j - k) from a table of 2 n - 1 entries."""
    j = np.arange(n)
    return table[j[:, None] - j[None, :] + n - 1]


# --------------------------------------------------------------------------- references

def dense_exact(mat, pad, mode, ty, tx):
    """real(A_y m A_x^T) cropped, with integer tables ty = (re, im) and tx = (re, im) and an integer or bool image, in exact integer
    arithmetic (int64; Python integers for uint64, which int64 does not hold), as float64.  m is np.pad of `mat` in mat's own dtype.
    Asserts what makes the kernels' float64 sums exact in any order: the sum of the magnitudes of all products of an output, through
    both passes, is below 2^53."""
    mat = np.asarray(mat)
    assert mat.dtype.kind in "iub", mat.dtype
    m = np.pad(mat, ((pad, pad), (pad, pad)), mode=mode)
    exact = object if mat.dtype == np.uint64 else np.int64
    m = m.astype(exact)
    ny, nx = m.shape
    mats = []
    for table, n in ((ty[0], ny), (ty[1], ny), (tx[0], nx), (tx[1], nx)):
        assert np.array_equal(table, np.rint(table)) and table.shape == (2 * n - 1,)
        mats.append(toeplitz(table.astype(np.int64), n).astype(exact))
    yr, yi, xr, xi = mats
    largest = int(np.abs(m).max()) if m.size else 0
    by = int((np.abs(ty[0]) + np.abs(ty[1])).sum())          # no row of |A_y,re| + |A_y,im| sums to more than its whole table
    bx = int((np.abs(tx[0]) + np.abs(tx[1])).sum())
    assert by * bx * largest < 2 ** 53, "not exact in float64: %d * %d * %d" % (by, bx, largest)
    out = (yr @ m) @ xr.T - (yi @ m) @ xi.T
    return out[pad:ny - pad, pad:nx - pad].astype(np.float64)


def dense_float(mat, pad, mode, ty, tx):
    """The same product in float64 matrices (for Gaussian tables): what the kernels compute, in NumPy's order."""
    m = np.pad(np.asarray(mat), ((pad, pad), (pad, pad)), mode=mode).astype(np.float64)
    ny, nx = m.shape
    out = (toeplitz(ty[0], ny) @ m) @ toeplitz(tx[0], nx).T - (toeplitz(ty[1], ny) @ m) @ toeplitz(tx[1], nx).T
    return out[pad:ny - pad, pad:nx - pad]


def truth(mat, sigma, pad, mode):
    """The reference's formula through dense long-double DFT matrices (g26_truth of tools/gen_golden.py restated): the yardstick of
    e_ref = max|reference - truth| / max|truth|, the reference's own rounding error, for a shape the fixture does not hold."""
    ld = np.longdouble
    m = np.pad(mat, ((pad, pad), (pad, pad)), mode=mode).astype(ld)
    pi = 4 * np.arctan(ld(1))

    def operator_of(n):                                                   # S conj(F) / n diag(w) F S as real and imaginary parts
        k = np.arange(n)
        ph = (np.outer(k, k) % n).astype(ld) * 2 * pi / n
        fr, fi = np.cos(ph), -np.sin(ph)
        w = np.exp(-((k.astype(ld) - (n - 1) / ld(2)) ** 2) / (2 * ld(sigma) * ld(sigma)))
        sg = np.where(k % 2 == 0, ld(1), ld(-1))
        br, bi = (fr * w) @ fr + (fi * w) @ fi, (fr * w) @ fi - (fi * w) @ fr
        return sg[:, None] * br * sg[None, :] / n, sg[:, None] * bi * sg[None, :] / n
    (yr, yi), (xr, xi) = operator_of(m.shape[0]), operator_of(m.shape[1])
    out = (yr @ m) @ xr.T - (yi @ m) @ xi.T
    return out[pad:m.shape[0] - pad, pad:m.shape[1] - pad]


def e_ref_of(ref, mat, sigma, pad, mode):
    t = truth(mat, sigma, pad, mode)
    return float(np.abs(ref - t).max() / np.abs(t).max())


# --------------------------------------------------------------------------- the cases of tests/test_fourier_taps_gpu.py

def integer_image(shape, dtype, seed):
    """Integers over the whole range of uint8 / uint16 (65535 included)."""
    info = np.iinfo(dtype)
    im = np.random.default_rng(seed).integers(0, info.max, size=shape, endpoint=True).astype(dtype)
    im.reshape(-1)[::17] = info.max
    return im


class Case:
    """A random-integer-table case: a (height, width) source of `dtype`, its pad and np.pad mode, the radius and the `where` of each
    axis' table, and what the case claims about each axis (checked on the CPU): `branches` the exact set of branches its blocks take,
    `one_left` the length modulo STEPS of its one-run windows, `turn` = 2 R + ROWS - N where the case is about the turn to the whole
    axis, `tail` whether a block reads the zeros behind the table."""

    def __init__(self, name, shape, pad, mode, dtype, ry, rx, where="both", branches=None, one_left=None, turn=None, tail=None,
                 wide=False):
        self.name, self.shape, self.pad, self.mode, self.dtype = name, shape, pad, mode, dtype
        self.r, self.where = (ry, rx), where
        self.branches, self.one_left, self.turn, self.tail, self.wide = branches, one_left, turn, tail, wide

    @property
    def n(self):
        return self.shape[0] + 2 * self.pad, self.shape[1] + 2 * self.pad

    def __repr__(self):
        return self.name


B3, B2 = ({"below", "one", "above"},) * 2, ({"one", "above"},) * 2
_MODES = ("reflect", "symmetric", "edge", "wrap")

# 41 x 45, pad 2 (N = 45 and 49, six blocks per axis, the last one ragged): a window of 8 + 2 R indices
RADII = [Case("r%d_%d" % (ry, rx), (41, 45), 2, _MODES[i % 4], ("uint8", "uint16")[i % 2], ry, rx,
              branches=tuple({"one", "above"} if r < 3 else {"below", "one", "above"} for r in (ry, rx)),
              one_left=((ROWS + 2 * ry) % STEPS, (ROWS + 2 * rx) % STEPS))
         for i, (ry, rx) in enumerate([(0, 0), (1, 1), (7, 7), (8, 8), (9, 9), (7, 9), (9, 1), (0, 8)])]
# the turn to the whole axis, N = 45 (odd) and 46 (even) on either axis: 2 R + 8 - N = -1 (the two runs leave one index out), 0 and
# +1 (the first windows that are the whole axis), and -2 / +2 next to them for the even side
TURN = [Case("turn_%dx%d_r%d_%d" % (h, w, ry, rx), (h, w), 2, _MODES[i % 4], ("uint16", "uint8")[i % 2], ry, rx,
             turn=(2 * ry + ROWS - h - 4, 2 * rx + ROWS - w - 4))
        for i, (h, w, ry, rx) in enumerate([(41, 42, 18, 19), (41, 42, 19, 18), (41, 42, 19, 20), (42, 41, 19, 18), (42, 41, 18, 19),
                                            (42, 41, 20, 19)])]
WHERES = [Case("where_" + w, (41, 45), 2, _MODES[i % 4], ("uint16", "uint8")[i % 2], 5, 5, where=w, branches=B3, one_left=(2, 2))
          for i, w in enumerate(WHERE[1:])]
# pad 0, and a pad below ROWS - 1 with sides that are no multiple of ROWS: the last block's outputs reach past N - 1
SMALL_PAD = [Case("pad0", (41, 45), 0, "reflect", "uint16", 6, 6, branches=B3, tail=(True, True)),
             Case("pad3", (43, 36), 3, "symmetric", "uint8", 4, 5, branches=B3, tail=(True, True)),
             Case("pad0_wrap", (41, 45), 0, "wrap", "uint8", 3, 11, branches=B3, tail=(True, True))]
# a second workgroup column in pass 1 (263 padded columns) and in pass 2 (261 rows)
WIDE = Case("wide", (261, 259), 2, "reflect", "uint16", 6, 6, branches=B3, one_left=(4, 4), wide=True)
# zeros that enter through the fold, not through the table
CONSTANT = Case("constant", (41, 45), 2, "constant", "uint16", 7, 9, branches=B3, one_left=(6, 2))
CASES = RADII + TURN + WHERES + SMALL_PAD + [WIDE, CONSTANT]
BOUNDS_CASES = RADII + TURN[:3] + [WHERES[1], WIDE]


@functools.lru_cache(maxsize=None)
def case_data(name):
    """(source, (ty_re, ty_im), (tx_re, tx_im), expected float64 plane) of a case, computed once and read-only."""
    c = next(c for c in CASES if c.name == name)
    seed = sum(ord(ch) * (k + 1) for k, ch in enumerate(name))
    rng = np.random.default_rng(seed)
    src = integer_image(c.shape, c.dtype, seed + 1)
    ty, tx = integer_table(c.n[0], c.r[0], rng, c.where), integer_table(c.n[1], c.r[1], rng, c.where)
    want = dense_exact(src, c.pad, c.mode, ty, tx)
    for a in (src, want) + ty + tx:
        a.setflags(write=False)
    return src, ty, tx, want


# --------------------------------------------------------------------------- Gaussian tables at the workload's geometry

# (shape, pad, sigma, mode): the default call on 2000 x 2000 (N = 2200, pad 100, sigma 10: R = 305 > pad) scaled down to sides <= 264,
# the N the suite's factor 8 was derived for.  On both axes R > pad, the blocks take all of below / one / above, and fewer than two
# thirds of the taps are kept.
GAUSS = [((203, 187), 10, 10, "reflect"), ((131, 150), 5, 6, "symmetric"), ((140, 131), 8, 8, "constant"), ((190, 203), 0, 10, "edge")]


@functools.lru_cache(maxsize=None)
def gauss_image(k):
    shape = GAUSS[k][0]
    im = np.random.default_rng(4000 + k).uniform(50.0, 250.0, shape).astype(np.float32)
    im.setflags(write=False)
    return im
