"""CPU suite for the Fourier Gaussian filter (discorpy_amd.prep.preprocessing.normalization_fft / _apply_fft_filter; dcp_fourier_gauss_2d):
the symbol is exported, declared and bound; every argument it refuses is refused with its code and a message of its own before any
device work (the buffers are host memory, dst stays untouched); the wrappers raise for what they do not take before they ask for a
device; _make_window is the reference's formula; the tap tables of _fourier_taps have the symmetry the derivation gives them and
transform back into the window's factor; and the mathematics holds without a GPU: dense NumPy Toeplitz matrices built from the tables,
applied to np.pad of every input of golden G26 (tools/gen_golden.py: the reference's own outputs), reproduce the reference's
background plane within 8 e_ref, e_ref the reference's own distance from a long-double evaluation (recorded per case in the fixture).

The second half pins the cases of tests/test_fourier_taps_gpu.py (tests/helpers/fourier_cases.py) to the kernels' constants: which
branches of fourier_runs each axis takes, the window against N at the turn to the whole axis, the steps its runs leave over, the
workgroup columns, the zeros read behind the table -- each with a shape that does not meet the condition --, that the integer tables
have the radius they were built with, that the exact reference returns the source under identity tables, that the restated truth
gives the fixture's e_ref back, and that the fixture and the tile cases never wrap a truncated window (why those cases exist)."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT, golden

from discorpy_amd import _ffi as F

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import fourier_cases as FC  # noqa: E402

SYMBOL = "dcp_fourier_gauss_2d"
INV, UNS = F.ERR_INVALID_ARG, F.ERR_UNSUPPORTED
H, W, PAD = 8, 10, 3
SRC = np.zeros(H * (W + 4) * 8, np.uint8)
SENTINEL = 0xA5
DST = np.full(H * W * 8, SENTINEL, np.uint8)
_dp = F.C.POINTER(F.C.c_double)
MODE_NP_REFLECT = 5         # DCP_MODE_MIRROR: np.pad's "reflect"


def tables():
    from discorpy_amd.prep import preprocessing as prep
    yr, yi = prep._fourier_taps(H + 2 * PAD, 2.0)
    xr, xi = prep._fourier_taps(W + 2 * PAD, 2.0)
    return dict(yr=yr.copy(), yi=yi.copy(), xr=xr.copy(), xi=xi.copy())


def poisoned(key, index, value):
    t = tables()[key]
    t[index] = value
    return t


VALID = dict(src=SRC.ctypes.data, dst=DST.ctypes.data, height=H, width=W, stride=W, dtype=F.DTYPE_BY_NAME["uint16"], pad=PAD, pad_mode=MODE_NP_REFLECT,
             yr="table", yi="table", xr="table", xi="table", mem_kind=F.MEM_HOST, device=-1, stream=None)
ORDER = "src dst height width stride dtype pad pad_mode yr yi xr xi mem_kind device stream".split()


def call(**override):
    args = dict(VALID, **override)
    keep = tables()
    for k in ("yr", "yi", "xr", "xi"):
        if isinstance(args[k], str):
            args[k] = keep[k]
        args[k] = None if args[k] is None else args[k].ctypes.data_as(_dp)
    return F.lib().dcp_fourier_gauss_2d(*[args[k] for k in ORDER])


def test_symbol_is_exported_declared_and_bound():
    assert hasattr(F.lib(), SYMBOL)
    header = open(os.path.join(ROOT, "include", "discorpy_hip.h")).read()
    assert re.search(r"^int %s\(const void\* src, void\* dst, int height, int width, long src_row_stride, int dtype,$" % SYMBOL, header, re.M)
    for word in ("DCP_MODE_MIRROR = \"reflect\"", "DCP_MODE_REFLECT = \"symmetric\"", "DCP_MODE_NEAREST = \"edge\"", "DCP_MODE_WRAP = \"wrap\"",
                 "DCP_MODE_CONSTANT = \"constant\"", "cannot be captured"):
        assert word in header, word
    exports = open(os.path.join(ROOT, "discorpy_amd", "csrc", "exports.map")).read()
    assert re.search(r"^\s*%s;" % SYMBOL, exports, re.M), "not named in csrc/exports.map"
    restype, argtypes = F.SIGNATURES[SYMBOL]
    assert restype is F.C.c_int and len(argtypes) == 15 and argtypes[4] is F.C.c_long and argtypes[8:12] == [_dp] * 4


CASES = [
    (dict(yr=None), INV, "null tap table"),
    (dict(yi=None), INV, "null tap table"),
    (dict(xr=None), INV, "null tap table"),
    (dict(xi=None), INV, "null tap table"),
    (dict(pad=-1), INV, "pad must be at least 0"),
    (dict(pad_mode=1), INV, "unknown pad mode 1"),               # the codes np.pad has no mode for
    (dict(pad_mode=3), INV, "unknown pad mode 3"),
    (dict(pad_mode=6), INV, "unknown pad mode 6"),
    (dict(pad_mode=8), INV, "unknown pad mode 8"),
    (dict(pad_mode=-1), INV, "unknown pad mode -1"),
    (dict(yr=poisoned("yr", 0, np.nan)), INV, "taps_y hold a value that is not finite"),
    (dict(yi=poisoned("yi", 13, np.inf)), INV, "taps_y hold a value that is not finite"),
    (dict(xr=poisoned("xr", 30, -np.inf)), INV, "taps_x hold a value that is not finite"),
    (dict(xi=poisoned("xi", 15, np.nan)), INV, "taps_x hold a value that is not finite"),
    (dict(pad=8189), UNS, "padded side above 16384"),             # 8 + 2 * 8189 = 16386; refused before a table is read
    (dict(height=1, width=1, pad=8192), UNS, "padded side above 16384"),
    (dict(dst=SRC.ctypes.data), INV, "overlap"),
    (dict(dst=SRC.ctypes.data + 2 * (H * W - 1)), INV, "overlap"),
    (dict(height=0), INV, "height"),
    (dict(width=-1), INV, "width"),
    (dict(stride=W - 1), INV, "src_row_stride"),
    (dict(dtype=99), INV, "dtype"),
    (dict(mem_kind=7), INV, "mem_kind"),
    (dict(mem_kind=F.MEM_DEVICE_UNORDERED), INV, "mem_kind"),
    (dict(src=None), INV, "src"),
    (dict(dst=None), INV, "dst"),
]


@pytest.mark.parametrize("override,rc,fragment", CASES, ids=["%02d-%s" % (i, "-".join(sorted(c[0]))) for i, c in enumerate(CASES)])
def test_refused_argument(override, rc, fragment):
    got = call(**override)
    assert (got, fragment in F.last_error()) == (rc, True), (got, F.last_error())
    assert (DST == SENTINEL).all(), "a refused call wrote to dst"


def test_arguments_at_the_limits_pass_the_checks():
    """pad = 0, every mode np.pad has, dst right behind the source and a padded side of exactly 16384 are legal: the call gets past
    the argument checks (and, with no device here, fails in the device layer -- or succeeds where a GPU is visible)."""
    from discorpy_amd.prep import preprocessing as prep
    ok = (F.OK, F.ERR_HIP, F.ERR_NO_DEVICE)
    dst = np.zeros(H * W * 8, np.uint8)
    for mode in (0, 2, 4, 5, 7):
        assert call(pad_mode=mode, dst=dst.ctypes.data) in ok, F.last_error()
    yr, yi = prep._fourier_taps(H, 2.0)
    xr, xi = prep._fourier_taps(W, 2.0)
    assert call(pad=0, yr=yr, yi=yi, xr=xr, xi=xi, dst=dst.ctypes.data) in ok, F.last_error()
    assert call(stride=W + 4, dst=SRC.ctypes.data + 2 * ((H - 1) * (W + 4) + W)) in ok, F.last_error()


def test_module_offers_the_reference_signatures():
    from discorpy_amd.prep import preprocessing as prep
    P = inspect.Parameter

    def sig(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    assert sig(prep.normalization_fft) == [("mat", P.empty), ("sigma", 10), ("pad", 100), ("mode", "reflect")]
    assert sig(prep._apply_fft_filter) == [("mat", P.empty), ("sigma", P.empty), ("pad", P.empty), ("mode", "reflect")]
    assert sig(prep._make_window) == [("height", P.empty), ("width", P.empty), ("sigma", 10)]
    assert prep.FOURIER[0] == "normalization_fft" and all(callable(getattr(prep, name)) for name in prep.FOURIER)
    from discorpy_amd.prep import linepattern as lp
    out = lp.__doc__.split("Out of scope")[1].split("\n\n")[0]
    assert "normalization_fft" not in out and "peak search" in out and "Radon" in out
    assert "normalization_fft" in prep.__doc__ and "Fourier Gaussian filter" in open(os.path.join(ROOT, "DESIGN.md")).read()


def test_refused_inputs_of_the_wrappers_need_no_device(monkeypatch):
    from discorpy_amd.prep import preprocessing as prep

    def no_device():
        raise AssertionError("require_device was reached")
    monkeypatch.setattr(F, "require_device", no_device)
    a = np.full((6, 7), 100.0, np.float32)
    for fn in (lambda m, **kw: prep.normalization_fft(m, **kw), lambda m, sigma=10, pad=100, mode="reflect": prep._apply_fft_filter(m, sigma, pad, mode)):
        for sigma in (0, -1.0, np.nan, np.inf, "wide", None):
            with pytest.raises(ValueError, match="sigma must be a positive finite number"):
                fn(a, sigma=sigma)
        for pad in (-1, 2.5, "3", None):
            with pytest.raises(ValueError, match="pad must be a non-negative integer"):
                fn(a, pad=pad)
        for mode in ("linear_ramp", "maximum", "mean", "median", "minimum", "empty", "mirror", "nearest"):
            with pytest.raises(NotImplementedError, match="reflect, symmetric, edge, wrap, constant"):
                fn(a, mode=mode)
        for dt in (np.complex64, np.complex128):
            with pytest.raises(TypeError, match="Complex type not supported"):
                fn(a.astype(dt))
        with pytest.raises(RuntimeError, match="data type not supported"):
            fn(a.astype(np.float16))
        with pytest.raises(ValueError, match="2-D"):
            fn(np.zeros((2, 3, 4), np.float32))
        with pytest.raises(NotImplementedError, match="padded side above 16384"):
            fn(a, pad=8190)
    # an empty plane needs no device either
    for shape in ((0, 5), (4, 0)):
        out = prep._apply_fft_filter(np.zeros(shape, np.uint16), 3, 2)
        assert out.shape == shape and out.dtype == np.float64


def test_other_device_arrays_are_pointed_to_the_filter():
    from discorpy_amd.prep import preprocessing as prep

    class Cai:
        __cuda_array_interface__ = {"shape": (4, 4), "typestr": "<f4", "data": (4096, False), "version": 3, "strides": None}
    with pytest.raises(TypeError, match="_apply_fft_filter"):
        prep.normalization_fft(Cai())


def test_make_window_is_the_references_formula():
    """exp(-(x * x / num + y * y / num)), num = 2.0 * sigma * sigma, x and y counted from the centre ((n - 1) / 2): float64 whatever
    the arguments are, for an odd and an even side (the parameters of two cases of G26: 237 x 252 at sigma 5, 240 x 251 at sigma 10)."""
    from discorpy_amd.prep import preprocessing as prep
    g = golden("g26_fourier_gauss")
    names = list(g["names"])
    for name in ("s37x52_p100_s5", "s40x51_p100_s10"):
        k = names.index(name)
        h, w = (int(v) + 2 * int(g["pad"][k]) for v in g[name + "_in"].shape)
        sigma = int(g["sigma"][k])
        for s in (sigma, float(sigma), np.float32(sigma)):
            win = prep._make_window(h, w, s)
            y = (np.arange(h) - (h - 1.0) / 2.0)[:, None]
            x = (np.arange(w) - (w - 1.0) / 2.0)[None, :]
            num = 2.0 * float(sigma) * float(sigma)
            assert win.dtype == np.float64 and win.shape == (h, w)
            assert np.array_equal(win, np.exp(-(x * x / num + y * y / num)))
    assert (h, w) == (240, 251) and prep._make_window(3, 4).shape == (3, 4)


@pytest.mark.parametrize("n", [237, 251, 1, 2])
@pytest.mark.parametrize("sigma", [0.5, 5, 10])
def test_tap_tables(n, sigma):
    from discorpy_amd.prep import preprocessing as prep
    re_, im_ = prep._fourier_taps(n, sigma)
    assert re_.dtype == im_.dtype == np.float64 and re_.shape == im_.shape == (2 * n - 1,)
    assert not re_.flags.writeable and prep._fourier_taps(n, float(sigma))[0] is re_, "cached per (n, sigma)"
    a = re_ + 1j * im_
    d = np.arange(1, n)
    # the wrapped half: a(d - n) = (-1)^n a(d)
    assert np.array_equal(a[d - n + n - 1], (-1.0) ** n * a[d + n - 1])
    # c[d] = (-1)^d a(d), d = 0 .. n - 1, is the inverse DFT of the window's factor: its DFT gives the factor back
    d = np.arange(n)
    c = np.where(d % 2 == 0, 1.0, -1.0) * a[d + n - 1]
    x = d - (n - 1.0) / 2.0
    w = np.exp(-(x * x / (2.0 * sigma * sigma)))
    err = np.abs(np.fft.fft(c) - w).max() / w.max()
    print("n = %d, sigma = %g: |fft(c) - w| / max w = %.3g" % (n, sigma, err))
    assert err <= 1e-15


@pytest.mark.parametrize("n,sigma,some", [(237, 10, True), (237, 5, True), (251, 10, True), (251, 5, True), (237, 0.5, False), (264, 40, False),
                                          (90, 1, False), (1, 5, False), (2, 0.5, False)])
def test_taps_set_to_zero_are_below_the_bound(n, sigma, some):
    """_taps_below_the_bound marks an entry of ifft(w) only where its TRUE magnitude (a dense long-double DFT here) is below
    2^-58 sum|c| / n, and the table holds exact zeros there; a window too narrow to decay (sigma 0.5, 1) or cut off at the ends of the
    axis (sigma 40 on 264) loses nothing.  The radius api_fourier.cpp's support_radius derives from the table (restated) is then about
    0.15 n (10 / sigma) where the decay is real, and n / 2 (everything) where it is not."""
    from discorpy_amd.prep import preprocessing as prep
    ld = np.longdouble
    d = np.arange(n)
    x = d - (n - 1.0) / 2.0
    c = np.fft.ifft(np.exp(-(x * x / (2.0 * sigma * sigma))))
    total = np.abs(c).sum()
    mask = prep._taps_below_the_bound(n, float(sigma), total)
    assert mask.shape == (n,) and bool(mask.any()) == some
    re_, im_ = prep._fourier_taps(n, sigma)
    zero = (re_[d + n - 1] == 0.0) & (im_[d + n - 1] == 0.0)
    assert np.array_equal(zero, mask) or not some
    if some:
        ph = (np.outer(d, d) % n).astype(ld) * (8 * np.arctan(ld(1))) / n
        wl = np.exp(-((d.astype(ld) - (n - 1) / ld(2)) ** 2) / (2 * ld(sigma) * ld(sigma)))
        true = np.hypot((np.cos(ph) * wl).sum(1), (np.sin(ph) * wl).sum(1)) / n
        print("n = %d, sigma = %g: %d entries zeroed, largest true magnitude among them %.3g, bound %.3g" % (
            n, sigma, mask.sum(), float(true[mask].max()), total * 2.0 ** -58 / n))
        assert float(true[mask].max()) <= total * 2.0 ** -58 / n
        assert not mask[0] and np.array_equal(mask[1:], mask[1:][::-1]), "symmetric in the cyclic distance"
    r = FC.support_radius(re_, im_, n)          # csrc/api_fourier.cpp's loop restated (tests/helpers/fourier_cases.py)
    if some:
        assert 0.12 * n * 10 / sigma < r < 0.17 * n * 10 / sigma, r
    else:
        assert r >= n // 2 - 1, r              # (an even side's middle tap cancels exactly and may go)


def dense_toeplitz(n, sigma):
    from discorpy_amd.prep import preprocessing as prep
    re_, im_ = prep._fourier_taps(n, sigma)
    j = np.arange(n)
    idx = j[:, None] - j[None, :] + n - 1
    return re_[idx], im_[idx]


def test_dense_toeplitz_matrices_reproduce_the_reference():
    """real(A_y m A_x^T) with dense matrices from _fourier_taps against the reference's planes of G26: within 8 e_ref on every case."""
    g = golden("g26_fourier_gauss")
    worst = 0.0
    for k, name in enumerate(g["names"]):
        mat = g[name + "_in"]
        if name.startswith("view_"):
            mat = mat[:, 3:-7]
        sigma, pad, mode = float(g["sigma"][k]), int(g["pad"][k]), str(g["mode"][k])
        m = np.pad(mat, pad, mode=mode).astype(np.float64)
        (yr, yi), (xr, xi) = dense_toeplitz(m.shape[0], sigma), dense_toeplitz(m.shape[1], sigma)
        got = ((yr @ m) @ xr.T - (yi @ m) @ xi.T)[pad:m.shape[0] - pad, pad:m.shape[1] - pad]
        ref = g[name + "_bck"]
        ratio = np.abs(got - ref).max() / np.abs(ref).max() / g["e_ref"][k]
        print("%-22s e_ref %.3g  |dense - ref| / max|ref| = %.2f e_ref" % (name, g["e_ref"][k], ratio))
        assert got.shape == ref.shape and ratio <= 8.0, (name, ratio)
        worst = max(worst, ratio)
    assert len(g["names"]) == 31 and worst > 0.0


# --------------------------------------------------------------------------- the cases of tests/test_fourier_taps_gpu.py, pinned

def fourier_constants():
    """kFourierRows of dcp_internal.h, kFourierSteps and kFourierBlock of fourier_kernels.hip."""
    csrc = os.path.join(ROOT, "discorpy_amd", "csrc")
    out = {}
    for name, source in (("kFourierRows", "dcp_internal.h"), ("kFourierSteps", "fourier_kernels.hip"), ("kFourierBlock", "fourier_kernels.hip")):
        m = re.search(r"^constexpr int %s = (\d+);" % name, open(os.path.join(csrc, source)).read(), re.M)
        assert m, "%s is not a named constant of %s" % (name, source)
        out[name] = int(m.group(1))
    return out


def test_case_tables_of_the_gpu_tests_are_the_kernels():
    """The helpers' ROWS / STEPS / BLOCK are the kernels' constants, runs() is fourier_runs (a window of 2 R + ROWS indices walked as
    at most two runs covers exactly the cyclic indices within R of a block's outputs), and every case of tests/test_fourier_taps_gpu.py
    is what its table says: the branches of each axis, the window against N at the turn, the leftover of its runs, a second workgroup
    column in both passes, the zeros behind the table read.  Each condition has a shape next to it that does not meet it."""
    const = fourier_constants()
    assert const == {"kFourierRows": 8, "kFourierSteps": 8, "kFourierBlock": 256}, "a constant moved: derive the cases again"
    assert (FC.ROWS, FC.STEPS, FC.BLOCK) == (const["kFourierRows"], const["kFourierSteps"], const["kFourierBlock"])
    # runs() against the definition, on every block of a few hundred (side, pad, R)
    for side, pad, R in [(s, p, r) for s in (1, 7, 8, 9, 41, 42) for p in (0, 2, 7, 23) for r in range(0, (s + 2 * p) // 2 + 1)]:
        N = side + 2 * pad
        for b, (name, rr) in zip(range(0, side, FC.ROWS), FC.branches(side, pad, R)):
            walked = [k for a, e in rr for k in range(a, e + 1)]
            window = {k % N for k in range(pad + b - R, pad + b + FC.ROWS + R)}
            assert len(walked) == len(set(walked)) and set(walked) == window, (side, pad, R, b, name)
            assert (name == "all") == (2 * R + FC.ROWS >= N) and all(0 <= a and e <= N - 1 for a, e in rr)
    left = set()
    for c in FC.CASES:
        src, ty, tx, want = FC.case_data(c.name)
        assert src.shape == c.shape and want.shape == c.shape and want.dtype == np.float64
        for ax, (re_, im_) in enumerate((ty, tx)):
            n, r = c.n[ax], c.r[ax]
            assert FC.support_radius(re_, im_, n) == r, "the library would not derive the radius the table was built with"
            d = np.abs(np.arange(-(n - 1), n))
            assert not ((re_ != 0) | (im_ != 0))[(d > r) & (d < n - r)].any() and np.abs(re_).max() <= 8 and np.abs(im_).max() <= 8
            g = FC.geometry(c.shape[ax], c.pad, r)
            if c.branches is not None:
                assert g["branches"] == c.branches[ax], (c, ax, g)
            if c.one_left is not None:
                assert g["one_left"] == {c.one_left[ax]}, (c, ax, g)
            if c.turn is not None:
                assert 2 * r + FC.ROWS - n == c.turn[ax] and abs(c.turn[ax]) <= 2
                assert g["branches"] == ({"all"} if c.turn[ax] >= 0 else {"below", "one", "above"}), (c, ax, g)
                assert g["gaps"] == ({-c.turn[ax]} if c.turn[ax] < 0 else set()), "the two runs leave out N - (2 R + ROWS) indices"
                assert FC.taps_kept(n, r) == 4 * r + 1 < 2 * n - 1, "the support is still truncated where the window is the whole axis"
            if c.tail is not None:
                assert g["tail"] == c.tail[ax], (c, ax, g)
            if c in FC.RADII:
                left |= g["left"]
        if c.wide:
            assert c.n[1] > FC.BLOCK and c.shape[0] > FC.BLOCK and c.n[1] <= 2 * FC.BLOCK, "a second workgroup column in pass 1 and in pass 2"
    assert left == set(range(FC.STEPS)), "the runs of the radius cases leave every count of steps over"
    assert {c.turn[ax] for c in FC.TURN for ax in (0, 1)} == {-2, -1, 0, 1, 2}
    assert {(c.n[ax] % 2, c.turn[ax]) for c in FC.TURN for ax in (0, 1)} >= {(1, -1), (1, 1), (0, 0)}, "both parities of N"
    assert sum(c.r[0] != c.r[1] for c in FC.RADII) >= 2 and {r for c in FC.RADII for r in c.r} == {0, 1, 7, 8, 9}
    assert {c.where for c in FC.WHERES} == {"near", "wrapped", "negative", "positive"} and {c.dtype for c in FC.CASES} == {"uint8", "uint16"}
    assert all(FC.case_data(c.name)[0].max() == np.iinfo(c.dtype).max for c in FC.CASES)
    assert any(c.pad == 0 for c in FC.SMALL_PAD) and any(0 < c.pad < FC.ROWS - 1 and c.shape[0] % FC.ROWS and c.shape[1] % FC.ROWS for c in FC.SMALL_PAD)
    assert set(FC.BOUNDS_CASES) <= set(FC.CASES) and len({c.name for c in FC.CASES}) == len(FC.CASES)
    # counter-examples: a shape that does not meet each condition
    assert FC.geometry(41, 2, 2)["branches"] == {"one", "above"}, "R <= pad: no window wraps below 0"
    assert FC.geometry(40, 8, 7)["branches"] == {"one"}, "R < pad and a side of whole blocks: no window wraps at all"
    assert FC.geometry(41, 2, 17)["gaps"] == {3} and FC.geometry(41, 2, 17)["branches"] == {"below", "one", "above"}, "2 R + 8 = N - 3: not at the turn"
    assert FC.geometry(41, 2, 8)["one_left"] == {0} != {(FC.ROWS + 2 * 7) % FC.STEPS}
    assert not FC.geometry(40, 0, 6)["tail"] and not FC.geometry(41, 7, 6)["tail"], "a side of whole blocks, or pad >= ROWS - 1: the table's end is never passed"
    assert 259 + 2 * 2 > FC.BLOCK >= 251 + 2 * 2 and 261 > FC.BLOCK >= 256, "255 padded columns or 256 rows are one workgroup column"


@pytest.mark.parametrize("where", FC.WHERE)
def test_integer_tables_have_the_radius_they_are_built_with(where):
    rng = np.random.default_rng(11)
    for n, r in ((45, 5), (46, 5), (45, 22), (46, 23), (9, 1), (45, 0), (2, 1), (1, 0)):
        if where in ("wrapped", "negative", "positive") and r == 0:
            continue                                   # (nothing is selected: the table would be empty)
        re_, im_ = FC.integer_table(n, r, rng, where)
        d = np.arange(-(n - 1), n)
        near, wrapped = np.abs(d) <= r, np.abs(d) >= n - r
        keep = {"both": near | wrapped, "near": near, "wrapped": wrapped, "negative": (near | wrapped) & (d < 0), "positive": (near | wrapped) & (d > 0)}[where]
        assert re_.dtype == im_.dtype == np.float64 and re_.shape == im_.shape == (2 * n - 1,)
        assert np.array_equal(re_ != 0, keep) and np.array_equal(im_ != 0, keep)
        assert np.array_equal(re_, np.rint(re_)) and np.abs(re_).max() <= 8 and np.abs(im_).max() <= 8
        assert FC.support_radius(re_, im_, n) == r, (n, r, where)
    if where == "wrapped":                              # a radius that ignored the wrapped half would find nothing here
        re_, im_ = FC.integer_table(45, 5, rng, where)
        assert not re_[45 - 1 - 5:45 - 1 + 6].any() and not im_[45 - 1 - 5:45 - 1 + 6].any()


@pytest.mark.parametrize("dtype", ["uint8", "int8", "uint16", "int16", "uint32", "int32", "int64", "uint64", "bool"])
def test_dense_exact_with_identity_tables_returns_the_source(dtype):
    """a(0) = 1 on both axes: the padded plane, cropped, is the source, whatever the pad and its mode; and the 2^53 condition is
    refused where it does not hold."""
    rng = np.random.default_rng(3)
    if dtype == "bool":
        src = rng.random((9, 13)) < 0.5
    else:
        info = np.iinfo(dtype)
        src = rng.integers(max(info.min, -2**52), min(info.max, 2**52), size=(9, 13), endpoint=True).astype(dtype)
    for pad, mode in ((0, "reflect"), (3, "symmetric"), (11, "wrap"), (4, "constant"), (2, "edge")):
        ty, tx = FC.delta_table(9 + 2 * pad, 0), FC.delta_table(13 + 2 * pad, 0)
        got = FC.dense_exact(src, pad, mode, ty, tx)
        assert got.dtype == np.float64 and np.array_equal(got, src.astype(np.float64))
    if dtype in ("int64", "uint64"):
        big = np.full((2, 2), 2**53 + 1, dtype)
        with pytest.raises(AssertionError, match="not exact in float64"):
            FC.dense_exact(big, 0, "reflect", FC.delta_table(2, 0), FC.delta_table(2, 0))
    # a shifted tap per axis moves the padded plane: dst[j, i] = m[j + pad - dy, i + pad - dx]
    m = np.pad(src, 3, mode="reflect").astype(np.float64)
    got = FC.dense_exact(src, 3, "reflect", FC.delta_table(15, 2), FC.delta_table(19, -3))
    assert np.array_equal(got, m[1:10, 6:19])


def test_restated_truth_reproduces_the_fixtures_e_ref():
    """helpers.truth is g26_truth of tools/gen_golden.py: from the fixture's own planes it gives the recorded e_ref back, equal to the
    last bit (the same long-double operations in the same order)."""
    g = golden("g26_fourier_gauss")
    names = list(g["names"])
    for name in ("s37x52_p100_s10", "full_30x45", "type_uint16"):
        k = names.index(name)
        e = FC.e_ref_of(g[name + "_bck"], g[name + "_in"], float(g["sigma"][k]), int(g["pad"][k]), str(g["mode"][k]))
        print("%-18s e_ref recorded %.17g restated %.17g" % (name, g["e_ref"][k], e))
        assert e == float(g["e_ref"][k]), (name, e, float(g["e_ref"][k]))


@pytest.mark.parametrize("k", range(len(FC.GAUSS)), ids=["%dx%d_p%d_s%d_%s" % (c[0] + c[1:]) for c in FC.GAUSS])
def test_gaussian_cases_at_the_workloads_geometry(k):
    """The Gaussian cases of tests/test_fourier_taps_gpu.py: on both axes R > pad, the blocks take below, one and above, fewer than
    two thirds of the taps are kept and the sides stay within 264; the dense float64 Toeplitz product stays within 8 e_ref of the
    reference restated on scipy.fftpack, e_ref measured for the case itself (1.4 - 1.6 here)."""
    from discorpy_amd.prep import preprocessing as prep
    from test_fourier_gauss_gpu import reference_filter, BCK_FACTOR
    shape, pad, sigma, mode = FC.GAUSS[k]
    mat = FC.gauss_image(k)
    taps = []
    for ax in (0, 1):
        n = shape[ax] + 2 * pad
        re_, im_ = prep._fourier_taps(n, sigma)
        r = FC.support_radius(re_, im_, n)
        g = FC.geometry(shape[ax], pad, r)
        assert r > pad and g["branches"] == {"below", "one", "above"} and 3 * FC.taps_kept(n, r) < 2 * (2 * n - 1) and n <= 264, (shape, ax, n, r, g)
        taps.append((re_, im_))
    ref = reference_filter(mat, sigma, pad, mode)
    e_ref = FC.e_ref_of(ref, mat, sigma, pad, mode)
    ratio = np.abs(FC.dense_float(mat, pad, mode, *taps) - ref).max() / np.abs(ref).max() / e_ref
    print("%s pad %d sigma %g %-9s e_ref %.3g  |dense - ref| / max|ref| = %.2f e_ref" % (shape, pad, sigma, mode, e_ref, ratio))
    assert 1e-17 < e_ref < 1e-14 and ratio <= BCK_FACTOR == 8.0, (shape, ratio)
    # the counter-example: the fixture's default-like case has R < pad and takes `one` only
    re_, im_ = prep._fourier_taps(237, 10)
    r = FC.support_radius(re_, im_, 237)
    assert r < 100 and FC.geometry(37, 100, r)["branches"] == {"one"}


def test_fixture_and_tile_cases_never_wrap_a_truncated_window():
    """Why the cases above exist: over golden G26 and TILE_CASES of tests/test_fourier_gauss_gpu.py an axis takes `below` or `above`
    only where at least 90 % of its taps are kept (the tile cases at sigma 3, R = 119 - 124 of N = 255 - 267), and the fixture's
    truncated cases (pad 100 > R) take `one` only."""
    from discorpy_amd.prep import preprocessing as prep
    import test_fourier_gauss_gpu as T

    def axis(side, pad, sigma):
        n = side + 2 * pad
        r = FC.support_radius(*prep._fourier_taps(n, sigma), n)
        return FC.geometry(side, pad, r)["branches"], FC.taps_kept(n, r) / (2.0 * n - 1.0)
    seen = []
    for name in T.NAMES:
        mat, sigma, pad = T.case(name)[:3]
        seen += [(name,) + axis(mat.shape[ax], pad, sigma) for ax in (0, 1)]
    for ax_, side, pad in T.TILE_CASES:
        shape = (side, 17) if ax_ == 0 else (17, side)
        seen += [("tile %s pad %d" % (shape, pad),) + axis(shape[ax], pad, 3) for ax in (0, 1)]
    wrapped = [s for s in seen if s[1] & {"below", "above"}]
    print("%d axes, %d of them wrap, smallest share of taps kept among those %.3f" % (len(seen), len(wrapped), min(s[2] for s in wrapped)))
    assert wrapped and all(s[2] >= 0.9 for s in wrapped), [s for s in wrapped if s[2] < 0.9]
    assert all(s[1] == {"one"} and s[2] < 2.0 / 3.0 for s in seen if s[0].startswith(("s37x52_", "s40x51_")))
