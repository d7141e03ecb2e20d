"""CPU suite for the selection of good peaks of discorpy_amd.prep.linepattern (select_good_peaks; dcp_select_peaks_rows): the name,
signature and defaults are the reference's; the entry point is exported, declared and bound and refuses what it does not take before
any device work, leaving its outputs untouched; the wrapper raises for what it does not take, and answers empty input, before it asks
for a device (this machine has none: reaching the device would raise something else); golden G32 (tools/gen_golden.py) keeps what its
generator promised."""
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT, golden

from discorpy_amd import _ffi as F

INV, UNS = F.ERR_INVALID_ARG, F.ERR_UNSUPPORTED
P = inspect.Parameter


@pytest.fixture(scope="module")
def lp():
    from discorpy_amd.prep import linepattern
    return linepattern


def test_name_signature_and_lists(lp):
    assert lp.PEAK_SELECTION == ["select_good_peaks"] and callable(lp.select_good_peaks)
    K = P.POSITIONAL_OR_KEYWORD
    assert [(p.name, p.default, p.kind) for p in inspect.signature(lp.select_good_peaks).parameters.values()] == [
        ("list_data", P.empty, K), ("peaks", P.empty, K), ("tol", 0.2, K), ("radius", 11, K), ("sigma", 0, K), ("use_offset", True, K)]
    # the other lists keep their contents
    assert set(lp.__all__) == {"gaussian_filter", "convert_chessboard_to_linepattern", "get_tilted_profile"}
    assert lp.CROSS_POINTS == ["get_tilted_profiles", "sliding_window_slope", "locate_subpixel_point", "get_local_extrema_points",
                               "get_cross_points_hor_lines", "get_cross_points_ver_lines"]
    assert lp.RADON == ["radon", "calc_slope_distance_hor_lines", "calc_slope_distance_ver_lines"]
    for word in ("select_good_peaks", "PEAK_SELECTION", "not wired"):
        assert word in lp.__doc__, word
    doc = lp.select_good_peaks.__doc__
    for word in ("get_local_extrema_points", "locate_subpixel_point", "np.max(d) - d", "denoise=False, norm=False", "max == min", "its own type"):
        assert word in doc, word


def test_symbol_is_exported_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "discorpy_hip.h")).read()
    exports = open(os.path.join(ROOT, "discorpy_amd", "csrc", "exports.map")).read()
    assert hasattr(F.lib(), "dcp_select_peaks_rows")
    assert re.search(r"^\s*dcp_select_peaks_rows;", exports, re.M)
    declared = re.search(r"^int dcp_select_peaks_rows\(([^;]*)\);", header, re.M)
    assert declared
    params = [" ".join(p.split()) for p in declared.group(1).split(",")]
    restype, argtypes = F.SIGNATURES["dcp_select_peaks_rows"]
    assert restype is F.C.c_int and len(argtypes) == len(params) == 16
    # the binding, argument by argument, against the header's types
    ctype_of = {"const void*": F.C.c_void_p, "void*": F.C.c_void_p, "unsigned char*": F.C.c_void_p, "double*": F.C.c_void_p, "int": F.C.c_int,
                "long": F.C.c_long, "double": F.C.c_double, "const int32_t*": F.C.POINTER(F.C.c_int32)}
    for param, bound in zip(params, argtypes):
        assert ctype_of[param.rsplit(" ", 1)[0]] is bound, (param, bound)


ROWS = np.zeros((4, 40), np.float32)
SENTINEL = 0xA5
KEEP = np.full(16, SENTINEL, np.uint8)
FIT = np.full(16 * 6 * 8, SENTINEL, np.uint8)
PEAK_ROW, PEAK_IDX = np.array([0, 1, 3], np.int32), np.array([5, 20, 39], np.int32)
F32, F64, U16 = (F.DTYPE_BY_NAME[n] for n in ("float32", "float64", "uint16"))
_i32 = F.C.POINTER(F.C.c_int32)


def select(**o):
    a = dict(src=ROWS.ctypes.data, nrows=4, length=40, stride=40, dtype=F32, peak_row=PEAK_ROW, peak_idx=PEAK_IDX, npeaks=3, radius=5, tol=0.2,
             use_offset=1, keep=KEEP.ctypes.data, fit=FIT.ctypes.data, mem_kind=F.MEM_HOST, device=-1, stream=None)
    a.update(o)
    for k in ("peak_row", "peak_idx"):
        a[k] = None if a[k] is None else a[k].ctypes.data_as(_i32)
    return F.lib().dcp_select_peaks_rows(*a.values())


REFUSALS = [
    (dict(src=None), INV, "null src"),
    (dict(peak_row=None), INV, "null peak_row / peak_index / keep"),
    (dict(peak_idx=None), INV, "null peak_row / peak_index / keep"),
    (dict(keep=None), INV, "null peak_row / peak_index / keep"),
    (dict(nrows=0), INV, "height and width must be at least 1"),
    (dict(length=0), INV, "height and width must be at least 1"),
    (dict(stride=39), INV, "src_row_stride 39 is below the width 40"),
    (dict(npeaks=0), INV, "npeaks must be at least 1"),
    (dict(npeaks=-3), INV, "npeaks must be at least 1"),
    (dict(peak_row=np.array([0, 4, 3], np.int32)), INV, "peak 1: row 4, index 20 lies outside the 4 x 40 plane"),
    (dict(peak_row=np.array([-1, 1, 3], np.int32)), INV, "peak 0: row -1"),
    (dict(peak_idx=np.array([5, 20, 40], np.int32)), INV, "peak 2: row 3, index 40 lies outside"),
    (dict(peak_idx=np.array([5, -1, 39], np.int32)), INV, "peak 1: row 1, index -1"),
    (dict(radius=0), INV, "radius must be at least 1"),
    (dict(radius=-2), INV, "radius must be at least 1"),
    (dict(radius=129), UNS, "radius above 128"),
    (dict(tol=float("nan")), INV, "tol is NaN"),
    (dict(use_offset=2), INV, "use_offset must be 0 or 1"),
    (dict(use_offset=-1), INV, "use_offset must be 0 or 1"),
    (dict(dtype=U16), UNS, "profiles are float32 or float64"),
    (dict(dtype=99), INV, "unknown dtype 99"),
    (dict(mem_kind=7), INV, "mem_kind"),
    (dict(keep=ROWS.ctypes.data + 8), INV, "src and keep / fit overlap"),
    (dict(fit=ROWS.ctypes.data + ROWS.nbytes - 8), INV, "src and keep / fit overlap"),
    (dict(fit=KEEP.ctypes.data), INV, "keep and fit overlap"),
]


@pytest.mark.parametrize("override,code,fragment", REFUSALS, ids=["-".join(c[0]) + "-%d" % k for k, c in enumerate(REFUSALS)])
def test_entry_point_refuses_before_any_device_work(override, code, fragment):
    KEEP[:] = SENTINEL
    FIT[:] = SENTINEL
    before = ROWS.copy()
    assert select(**override) == code
    assert fragment in F.last_error(), F.last_error()
    assert (KEEP == SENTINEL).all() and (FIT == SENTINEL).all() and np.array_equal(ROWS, before)


def test_wrapper_refuses_and_answers_empty_input_before_any_device_work(lp):
    row = np.arange(60.0)
    with pytest.raises(TypeError, match="Complex type not supported"):
        lp.select_good_peaks(row.astype(np.complex128), [5])
    with pytest.raises(NotImplementedError, match="radius above 128"):
        lp.select_good_peaks(row, [5], radius=129)
    with pytest.raises(ValueError, match="radius must be at least 1"):
        lp.select_good_peaks(row, [5], radius=0)
    for bad in ([60], [5, -1], np.array([3, 600])):
        with pytest.raises(ValueError, match=r"peak outside \[0, 60\)"):
            lp.select_good_peaks(row, bad)
    with pytest.raises(ValueError, match=r"row 1 has a peak outside \[0, 30\)"):
        lp.select_good_peaks(row.reshape(2, 30), [[5], [30]])
    with pytest.raises(ValueError, match="2 rows but 3 lists"):
        lp.select_good_peaks(row.reshape(2, 30), [[5], [6], [7]])
    with pytest.raises(ValueError, match="integers"):
        lp.select_good_peaks(row, [5.5])
    with pytest.raises(ValueError, match="tol is NaN"):
        lp.select_good_peaks(row, [5], tol=float("nan"))
    with pytest.raises(ValueError, match="1D array or an"):
        lp.select_good_peaks(np.zeros((2, 3, 4)), [5])
    # no candidates: the reference's empty array, for every element type and with a smoothing that would need the device
    for data in (row, row.astype(np.float32), row.astype(np.uint16)):
        for peaks in ([], np.asarray([]), np.zeros(0, np.int64)):
            got = lp.select_good_peaks(data, peaks, sigma=2)
            assert isinstance(got, np.ndarray) and got.shape == (0,) and got.dtype == np.asarray([]).dtype
    got = lp.select_good_peaks(row.reshape(3, 20), [[], [], []], sigma=1)
    assert isinstance(got, list) and len(got) == 3 and all(g.shape == (0,) for g in got)
    assert lp.select_good_peaks(np.zeros((0, 20)), []) == []


def test_restated_solver_decides_clear_candidates_as_the_reference_does():
    """tests/helpers/select_peaks_reference.py, the kernel's steps in NumPy, on a sample of golden G32: three line rows at radius 3 (the
    hardest windows: 7 samples, 4 parameters), two at radius 11, the noise row, the ramp and the square wave.  With the exact
    Jacobian in place of forward differences one clear candidate of the sample goes the other way ("Peak selection")."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
    import select_peaks_reference as SR
    g = golden("g32_select_peaks")
    compared = 0
    for name, rows_used in (("r3", (2, 14, 15)), ("r11", (1, 10)), ("h7", (0, 1, 2))):
        radius = int(g["radius"][list(g["case_names"]).index(name)])
        rows, row_of, idx = g[name + "_rows"], g[name + "_row_of"], g[name + "_idx"]
        keep, clear = g[name + "_f64_keep"], g[name + "_f64_clear"]
        for i in np.flatnonzero(np.isin(row_of, rows_used)):
            w = rows[row_of[i], max(0, idx[i] - radius):idx[i] + radius + 1]
            without, fit, nfev = SR.fit_window(w, radius, 0.2, False)
            assert 0 <= nfev <= SR.MAX_EVALS + 4 and (fit[5] == SR.CONSTANT) == (np.ptp(w) == 0)
            for col, got in enumerate((without and abs(fit[3]) < 0.2, without)):          # (with use_offset, without)
                if clear[i, col]:
                    assert got == keep[i, col], (name, i, col, fit, g[name + "_f64_ref"][i])
                    compared += 1
    assert compared >= 250
    i = int(np.flatnonzero((g["r3_row_of"] == 2) & (g["r3_idx"] == 14))[0])
    w = g["r3_rows"][2, 11:18]
    assert g["r3_f64_clear"][i].all() and not g["r3_f64_keep"][i].any()
    assert SR.fit_window(w, 3, 0.2, True, jacobian="analytic")[0] and not SR.fit_window(w, 3, 0.2, True)[0]
    assert SR.fit_window(np.zeros(3), 3, 0.2, True)[1][5] == SR.SHORT and SR.fit_window([1.0, np.inf, 0, 0, 2], 3, 0.2, True)[1][5] == SR.NOT_FINITE


def test_golden_keeps_what_its_generator_promised():
    g = golden("g32_select_peaks")
    delta, p99 = float(g["delta"]), float(g["p99"])
    assert delta == 4.0 * p99 and 0.0 < delta < 0.05
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "%.4g" % delta in design and "Peak selection" in design
    names = list(g["case_names"])
    assert {"r3", "r7", "r11", "h3", "h7", "big", "vec1", "vec2", "smooth"} == set(names)
    assert g["big_rows"].shape == (1, 600) and int(g["radius"][names.index("big")]) == 128 and g["r7_rows"].shape == (24, 160)
    total = unclear = 0
    kept = rejected = 0
    for name in names:
        radius, tol = int(g["radius"][names.index(name)]), float(g["tol"][names.index(name)])
        for key in ("f64", "f32"):
            ref, keep, clear = (g["%s_%s_%s" % (name, key, s)] for s in ("ref", "keep", "clear"))
            assert len(ref) == len(g[name + "_idx"]) == len(g[name + "_row_of"]) and keep.shape == clear.shape == (len(ref), 2)
            # the decision follows from the four values as the reference's lines say
            ok = (ref[:, 0] == 1) & (np.abs(ref[:, 1]) < radius // 2) & (ref[:, 3] < tol)
            assert np.array_equal(keep[:, 1], ok) and np.array_equal(keep[:, 0], ok & (np.abs(ref[:, 2]) < tol))
            total += clear.size
            unclear += int((~clear).sum())
            kept += int((keep & clear).sum())
            rejected += int((~keep & clear).sum())
    assert unclear <= 0.15 * total and abs(unclear / total - float(g["unclear_share"])) < 1e-12
    assert kept >= 100 and rejected >= 100
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g32_select_peaks.npz")) <= 1 << 20
