"""CPU suite for the peak search with select_peaks=True (prep.linecomplete; dcp_extrema_select_rows): the module carries the reference's
ten names and the reference's signatures on the five that take the flag; the entry point is exported, declared and bound and refuses
what it does not take before any device work, leaving its outputs untouched; the wrappers raise the reference's TypeError for a keyword
select_good_peaks does not take, and answer a clipped radius of 0 or 1 with empty results, before they ask for a device (this machine has
none: reaching the device would raise something else); prep.linepattern's five functions still refuse the flag; golden G33
(tools/gen_golden.py) keeps what its generator promised."""
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT, golden

from discorpy_amd import _ffi as F

INV, UNS = F.ERR_INVALID_ARG, F.ERR_UNSUPPORTED
P = inspect.Parameter
K, KW = P.POSITIONAL_OR_KEYWORD, P.VAR_KEYWORD
E = P.empty

# the reference's signatures (discorpy 1.7 prep/linepattern.py:195, 302, 378, 604, 684), parameter by parameter
SIGNATURES = {
    "get_local_extrema_points": [("list_data", E, K), ("option", "min", K), ("radius", 7, K), ("sensitive", 0.1, K), ("denoise", True, K),
                                 ("norm", True, K), ("subpixel", True, K), ("select_peaks", False, K), ("kwargs", E, KW)],
    "calc_slope_distance_hor_lines": [("mat", E, K), ("ratio", 0.3, K), ("search_range", 30.0, K), ("radius", 9, K), ("sensitive", 0.1, K),
                                      ("bgr", "bright", K), ("denoise", True, K), ("norm", True, K), ("subpixel", True, K), ("chessboard", False, K),
                                      ("select_peaks", False, K), ("kwargs", E, KW)],
    "get_cross_points_hor_lines": [("mat", E, K), ("slope_ver", E, K), ("dist_ver", E, K), ("ratio", 0.3, K), ("norm", True, K), ("offset", 0, K),
                                   ("bgr", "bright", K), ("radius", 11, K), ("sensitive", 0.1, K), ("denoise", True, K), ("subpixel", True, K),
                                   ("chessboard", False, K), ("select_peaks", False, K), ("kwargs", E, KW)],
}
SIGNATURES["calc_slope_distance_ver_lines"] = SIGNATURES["calc_slope_distance_hor_lines"]
SIGNATURES["get_cross_points_ver_lines"] = [("mat", E, K), ("slope_hor", E, K), ("dist_hor", E, K)] + SIGNATURES["get_cross_points_hor_lines"][3:]
TEN = ["locate_subpixel_point", "select_good_peaks", "sliding_window_slope", "get_local_extrema_points", "calc_slope_distance_hor_lines",
       "calc_slope_distance_ver_lines", "get_tilted_profile", "convert_chessboard_to_linepattern", "get_cross_points_hor_lines",
       "get_cross_points_ver_lines"]


@pytest.fixture(scope="module")
def lc():
    from discorpy_amd.prep import linecomplete
    return linecomplete


@pytest.fixture(scope="module")
def lp():
    from discorpy_amd.prep import linepattern
    return linepattern


def test_names_and_signatures_are_the_references(lc, lp):
    assert sorted(lc.__all__) == sorted(TEN) and len(set(lc.__all__)) == 10
    for name in lc.__all__:
        assert callable(getattr(lc, name)), name
    for name, want in SIGNATURES.items():
        got = [(p.name, p.default, p.kind) for p in inspect.signature(getattr(lc, name)).parameters.values()]
        assert got == want, name
        assert getattr(lc, name) is not getattr(lp, name)
    # what is re-exported is prep.linepattern's own object
    for name in ("locate_subpixel_point", "select_good_peaks", "sliding_window_slope", "get_tilted_profile", "convert_chessboard_to_linepattern",
                 "get_tilted_profiles", "gaussian_filter", "radon"):
        assert getattr(lc, name) is getattr(lp, name), name
    assert "import discorpy_amd.prep.linecomplete as lprep" in lc.__doc__ and "linecomplete" in lp.__doc__
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "discorpy_amd.prep.linecomplete" in integration


def test_symbol_is_exported_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "discorpy_hip.h")).read()
    exports = open(os.path.join(ROOT, "discorpy_amd", "csrc", "exports.map")).read()
    assert hasattr(F.lib(), "dcp_extrema_select_rows")
    assert re.search(r"^\s*dcp_extrema_select_rows;", exports, re.M)
    declared = re.search(r"^int dcp_extrema_select_rows\(([^;]*)\);", header, re.M)
    assert declared
    params = [" ".join(p.split()) for p in declared.group(1).split(",")]
    restype, argtypes = F.SIGNATURES["dcp_extrema_select_rows"]
    assert restype is F.C.c_int and len(argtypes) == len(params) == 18
    ctype_of = {"const void*": F.C.c_void_p, "void*": F.C.c_void_p, "unsigned char*": F.C.c_void_p, "double*": F.C.c_void_p, "int": F.C.c_int,
                "long": F.C.c_long, "double": F.C.c_double}
    for param, bound in zip(params, argtypes):
        assert ctype_of[param.rsplit(" ", 1)[0]] is bound, (param, bound)
    assert [p.rsplit(" ", 1)[1] for p in params] == ["src", "dst", "nrows", "length", "src_row_stride", "dtype", "radius", "sensitive", "subpixel", "sel",
                                                     "sel_row_stride", "tol", "use_offset", "cand", "keep", "mem_kind", "device", "stream"]


N, L = 4, 40
ROWS = np.zeros((N, L), np.float32)
SEL = np.ones((N, L + 2), np.float32)
SENTINEL = 0xA5
DST = np.full(N * L * 8, SENTINEL, np.uint8)
CAND = np.full(N * L * 8, SENTINEL, np.uint8)
KEEP = np.full(N * L, SENTINEL, np.uint8)
F32, F64, U16 = (F.DTYPE_BY_NAME[n] for n in ("float32", "float64", "uint16"))


def call(**o):
    a = dict(src=ROWS.ctypes.data, dst=DST.ctypes.data, nrows=N, length=L, stride=L, dtype=F32, radius=5, sensitive=0.1, subpixel=1,
             sel=SEL.ctypes.data, sel_stride=L + 2, tol=0.2, use_offset=1, cand=CAND.ctypes.data, keep=KEEP.ctypes.data, mem_kind=F.MEM_HOST, device=-1,
             stream=None)
    a.update(o)
    return F.lib().dcp_extrema_select_rows(*a.values())


REFUSALS = [
    (dict(src=None), INV, "null src / dst"),
    (dict(dst=None), INV, "null src / dst"),
    (dict(nrows=0), INV, "height and width must be at least 1"),
    (dict(length=0), INV, "height and width must be at least 1"),
    (dict(length=-4), INV, "height and width must be at least 1"),
    (dict(stride=L - 1), INV, "src_row_stride 39 is below the width 40"),
    (dict(sel_stride=L - 1), INV, "sel_row_stride 39 is below the width 40"),
    (dict(dtype=99), INV, "unknown dtype 99"),
    (dict(dtype=U16), UNS, "profiles are float32 or float64"),
    (dict(mem_kind=7), INV, "mem_kind"),
    (dict(radius=0), INV, "radius must be at least 1"),
    (dict(radius=-3), INV, "radius must be at least 1"),
    (dict(radius=129), UNS, "radius above 128"),
    (dict(sensitive=float("nan")), INV, "sensitive is NaN"),
    (dict(tol=float("nan")), INV, "tol is NaN"),
    (dict(subpixel=2), INV, "subpixel must be 0 or 1"),
    (dict(subpixel=-1), INV, "subpixel must be 0 or 1"),
    (dict(use_offset=2), INV, "use_offset must be 0 or 1"),
    (dict(use_offset=-1), INV, "use_offset must be 0 or 1"),
    (dict(dst=ROWS.ctypes.data + 8), INV, "src and dst overlap"),
    (dict(cand=ROWS.ctypes.data + ROWS.nbytes - 8), INV, "src and cand overlap"),
    (dict(keep=ROWS.ctypes.data + 16), INV, "src and keep overlap"),
    (dict(dst=SEL.ctypes.data), INV, "sel and dst overlap"),
    (dict(cand=SEL.ctypes.data + 64), INV, "sel and cand overlap"),
    (dict(keep=SEL.ctypes.data + SEL.nbytes - 12), INV, "sel and keep overlap"),
    (dict(cand=DST.ctypes.data + 8), INV, "dst and cand overlap"),
    (dict(keep=DST.ctypes.data + DST.nbytes - 1), INV, "dst and keep overlap"),
    (dict(keep=CAND.ctypes.data), INV, "cand and keep overlap"),
]


@pytest.mark.parametrize("override,code,fragment", REFUSALS, ids=["-".join(c[0]) + "-%d" % k for k, c in enumerate(REFUSALS)])
def test_entry_point_refuses_before_any_device_work(override, code, fragment):
    for out in (DST, CAND, KEEP):
        out[:] = SENTINEL
    rows, sel = ROWS.copy(), SEL.copy()
    assert call(**override) == code
    assert fragment in F.last_error(), F.last_error()
    assert all((out == SENTINEL).all() for out in (DST, CAND, KEEP)) and np.array_equal(ROWS, rows) and np.array_equal(SEL, sel)


def test_a_stride_of_sel_counts_only_where_sel_is_given():
    """(a later refusal shows that the stride was passed over)"""
    assert call(sel=None, sel_stride=0, radius=0) == INV and "radius must be at least 1" in F.last_error()
    assert call(sel_stride=0, radius=0) == INV and "sel_row_stride 0 is below the width 40" in F.last_error()


def test_wrappers_answer_before_any_device_work(lc):
    row = np.sin(np.arange(600.0) / 7.0)
    img = np.zeros((40, 60), np.float32)
    # a keyword select_good_peaks does not take: the reference's TypeError, from all five
    for name, args in (("get_local_extrema_points", (row,)), ("get_cross_points_hor_lines", (img, 0.01, 10.0)), ("get_cross_points_ver_lines", (img, 0.01, 10.0)),
                       ("calc_slope_distance_hor_lines", (img,)), ("calc_slope_distance_ver_lines", (img,))):
        with pytest.raises(TypeError, match=r"select_good_peaks\(\) got an unexpected keyword argument 'width'"):
            getattr(lc, name)(*args, select_peaks=True, tol=0.3, width=4)
    with pytest.raises(ValueError, match="tol is NaN"):
        lc.get_local_extrema_points(row, select_peaks=True, tol=float("nan"))
    with pytest.raises(ValueError, match="sigma is NaN"):
        lc.get_local_extrema_points(row, select_peaks=True, sigma=float("nan"))
    with pytest.raises(ValueError, match="could not convert"):
        lc.get_cross_points_hor_lines(img, 0.01, 10.0, select_peaks=True, sigma="wide")
    with pytest.raises(NotImplementedError, match="radius above 128"):
        lc.get_local_extrema_points(row, radius=129, select_peaks=True)
    with pytest.raises(TypeError, match="Complex type not supported"):
        lc.get_local_extrema_points(row.astype(np.complex64), select_peaks=True)
    # a clipped radius of 0 or 1: windows of at most 3 samples, which the reference does not fit -- nothing survives
    for data, radius in ((row, 1), (row, 0), (row[:7], 7), (row[:4], 3), (row[:3], 3), (row.astype(np.float32), 1), (np.arange(7), 5)):
        for subpixel in (True, False):
            got = lc.get_local_extrema_points(data, radius=radius, subpixel=subpixel, select_peaks=True, sigma=2)
            assert isinstance(got, np.ndarray) and got.shape == (0,) and got.dtype == np.asarray([]).dtype
    got = lc.get_local_extrema_points(row.reshape(3, 200), radius=1, select_peaks=True)
    assert isinstance(got, list) and len(got) == 3 and all(g.shape == (0,) and g.dtype == np.float64 for g in got)
    assert lc.get_local_extrema_points(np.zeros((0, 20)), select_peaks=True) == []


def test_linepattern_still_refuses_the_flag(lp):
    img = np.zeros((40, 60), np.float32)
    with pytest.raises(NotImplementedError, match="select_peaks"):
        lp.get_local_extrema_points(np.arange(600.0), select_peaks=True)
    for fn, args in ((lp.get_cross_points_hor_lines, (img, 0.01, 10.0)), (lp.get_cross_points_ver_lines, (img, 0.01, 10.0)),
                     (lp.calc_slope_distance_hor_lines, (img,)), (lp.calc_slope_distance_ver_lines, (img,))):
        with pytest.raises(NotImplementedError, match="select_peaks"):
            fn(*args, select_peaks=True, tol=0.3)


CLASSES = ("kept", "shift", "percentile", "offset", "raised")


def test_golden_keeps_what_its_generator_promised():
    g = golden("g33_select_wired")
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g33_select_wired.npz")) <= 1 << 20
    assert float(g["delta"]) == float(golden("g32_select_peaks")["delta"])
    case, cand, keep, clear, ref, tight = (g["tb_" + k] for k in ("case", "cand", "keep", "clear", "ref", "tight"))
    assert g["tb_rows"].shape == (27, 160) and np.array_equal(g["tb_rows"], np.concatenate([golden("g32_select_peaks")[k] for k in ("r7_rows", "h7_rows")]))
    assert case.shape[1] == 11 and len(cand) == len(keep) == len(clear) == len(ref) == len(tight) == case[:, 7].sum()
    assert len(g["tb_int"]) == len(g["tb_sub"]) == case[:, 9].sum() == keep.sum()
    # every combination the tables stand for: 27 rows x 3 radii x 3 sets of kwargs x 2 element types, and the subset through denoise / norm
    plain = case[(case[:, 4] == 0) & (case[:, 5] == 0)]
    assert len(plain) == 27 * 3 * 3 * 2 and set(plain[:, 1]) == {3, 7, 11} and set(plain[:, 2]) == {0, 1, 2} and set(plain[:, 3]) == {0, 1}
    assert {(int(d), int(n)) for d, n in case[:, 4:6]} == {(0, 0), (1, 0), (0, 1), (1, 1)}
    assert np.array_equal(g["kw_tol"], [0.2, 0.3, 0.2]) and np.array_equal(g["kw_sigma"], [0.0, 0.0, 1.5]) and g["kw_use_offset"].tolist() == [True, False, True]
    counts = dict.fromkeys(CLASSES, 0)
    for row, radius, k, dt, dn, nm, first, n, rfirst, rn, all_clear in case:
        tol, uo = float(g["kw_tol"][k]), bool(g["kw_use_offset"][k])
        sl = slice(first, first + n)
        v = ref[sl]
        # the decision follows from the four values as the reference's lines say; the returned positions are the kept candidates
        ok = (v[:, 0] == 1) & (np.abs(v[:, 1]) < radius // 2) & (v[:, 3] < tol) & ((np.abs(v[:, 2]) < tol) | (not uo))
        assert np.array_equal(ok, keep[sl]) and np.array_equal(g["tb_int"][rfirst:rfirst + rn], cand[sl][keep[sl]])
        assert bool(all_clear) == bool(clear[sl].all())
        assert ((cand[sl] >= radius) & (cand[sl] < 160 - radius - 1)).all() and (np.diff(cand[sl]) > 0).all()
        sub = g["tb_sub"][rfirst:rfirst + rn]
        assert (np.abs(sub - g["tb_int"][rfirst:rfirst + rn]) <= 1.0).all()
        for i in np.flatnonzero(clear[sl]):
            if keep[sl][i]:
                counts["kept"] += 1
            elif v[i, 0] == 0 and np.isfinite(v[i, 3]):
                counts["raised"] += 1
            elif v[i, 0] == 1 and abs(v[i, 1]) >= radius // 2:
                counts["shift"] += 1
            elif v[i, 0] == 1 and v[i, 3] >= tol:
                counts["percentile"] += 1
            elif v[i, 0] == 1 and uo:
                counts["offset"] += 1
    assert min(counts.values()) >= 20, counts
    assert case[:, 10].sum() >= 200                                   # rows whose candidates are all clear: what the GPU suite compares exactly
    # images: the points of every call, the candidates judged, the unclear ones
    im = g["im_case"]
    assert im.shape == (len(g["im_names"]), 6) and im[:, 2].sum() == len(g["im_pts"]) and g["im_pts"].shape[1] == 2
    assert (im[:, 2] <= im[:, 3]).all() and (im[:, 3] == im[:, 5]).all() and (im[:, 4] <= im[:, 3]).all()
    removed = im[:, 5] - im[:, 2]
    assert ((removed >= 10) & (im[:, 4] < removed / 2.0)).any()
    assert {n.rsplit("_", 2)[0] for n in g["im_names"]} == {"line", "tall", "big", "wide"} and g["img_wide"].shape == (240, 260)
    # slope and distance: G28's cases, at least two of them all clear with a distance to compare
    sd = g["sd_vals"]
    assert list(g["sd_names"]) == list(golden("g28_slope_distance")["case_names"]) and sd.shape == (len(g["sd_names"]), 5)
    assert ((sd[:, 2] == 1) & np.isfinite(sd[:, 1])).sum() >= 2
    # the share of unclear candidates, over everything the recorder saw
    total = case[:, 7].sum() + im[:, 3].sum() + sd[:, 3].sum()
    unclear = (~clear).sum() + im[:, 4].sum()
    assert unclear / total <= float(g["unclear_share"]) <= 0.15
