#!/usr/bin/env python
"""Generate tests/golden/*.npz by RUNNING THE REFERENCE (discorpy 1.7.0 at /root/reference).

Runs only in the build container (the reference never travels to the GPU box).  Each fixture
holds the inputs (or the seed that regenerates them) and the reference's outputs; nothing of the
reference's source is stored.  SURVEY.md section 8(c) lists the cases G1..G9; the later sets are described where they are made.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden.py
"""
import sys as _sys
if {"-h", "--help"} & set(_sys.argv[1:]):          # every tool answers --help without touching the GPU
    print(__doc__)
    raise SystemExit(0)
import os
import sys

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import scipy.ndimage as ndi  # noqa: E402
from scipy.ndimage import map_coordinates  # noqa: E402
import discorpy.post.postprocessing as post  # noqa: E402
import discorpy.proc.processing as proc  # noqa: E402
from discorpy_amd import configs  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
os.makedirs(OUT, exist_ok=True)


def save(name, **arrays):
    path = os.path.join(OUT, name + ".npz")
    if os.path.exists(path):
        old = np.load(path)
        if sorted(old.files) == sorted(arrays) and all(
                np.asarray(arrays[k]).dtype == old[k].dtype and np.array_equal(old[k], arrays[k], equal_nan=old[k].dtype.kind in "fc")
                for k in arrays):
            print("%-28s unchanged" % (name + ".npz"))
            return
    np.savez_compressed(path, **arrays)
    print("%-28s %7.1f KB" % (name + ".npz", os.path.getsize(path) / 1024.0))


def f64(v):
    return np.asarray(v, dtype=np.float64)


# ---- plane_refusals.json: what every refused argument of the plane entry points (dcp_*_2d of api_median / api_gauss / api_label /
# api_binarize.cpp) is answered with TODAY: the return code and the whole of dcp_last_error(), for every case of the tables of
# tests/test_{median,gaussian,label,binarize}_cpu.py (those match a fragment of the message only).  Run it with the library the
# recording is to pin, before a change to the argument checks -- not after, to make a failing replay pass:
#     python tools/gen_golden.py --plane-refusals
# Pointers are recorded by name ("null", "src", "dst", "src+166": bytes into the source buffer, the caller's outputs under their key);
# tests/test_plane_refusals_cpu.py builds buffers of the same sizes and replays the calls.
def plane_refusals():
    import json
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_binarize_cpu as tb
    import test_gaussian_cpu as tg
    import test_label_cpu as tl
    import test_median_cpu as tm
    from discorpy_amd import _ffi as F

    def encode(mod, key, v):
        if v is None:
            return "null"
        if isinstance(v, np.ndarray):          # weights of the Gaussian
            return {"repeat": float(v[0]), "n": len(v)} if len(v) > 8 and (v == v[0]).all() else [float(x) for x in v]
        if key in ("src", "dst", "weights", "labels"):
            for name, buf in (("src", mod.SRC), ("dst", mod.DST)):
                off = v - buf.ctypes.data
                if 0 <= off < buf.nbytes:
                    return name if off == 0 else "%s+%d" % (name, off)
            raise ValueError((key, v))
        if key in ("num", "sums", "boxes", "minmax", "bad", "counts", "count", "edges"):
            return key                          # the caller's outputs and the edges: the buffer of that name
        assert isinstance(v, (int, float)), (key, v)
        return v

    entries, cases = {}, []

    def record(mod, symbol, valid, order, table, call):
        entries[symbol] = {"order": order, "valid": {k: encode(mod, k, valid[k]) for k in order}}
        for override, rc, fragment in table:
            got = call(override)
            msg = F.last_error()
            assert got == rc and fragment in msg, (symbol, override, got, msg)
            cases.append({"entry": symbol, "override": {k: encode(mod, k, v) for k, v in sorted(override.items())}, "code": got, "message": msg})

    record(tm, "dcp_median_filter_2d", tm.VALID, tm.ORDER, tm.CASES, lambda o: tm.call(**o))
    record(tg, "dcp_correlate_sym_2d", tg.VALID, tg.ORDER, tg.CASES, lambda o: tg.call(**o))
    record(tl, "dcp_label_2d", tl.LABEL, tl.LABEL_ORDER, tl.LABEL_CASES, lambda o: tl.call("dcp_label_2d", tl.LABEL, tl.LABEL_ORDER, o))
    last = tl.SRC.ctypes.data + 2 * ((tl.H - 1) * (tl.W + 4) + tl.W)          # dst is bytes there: its first one on the source's last
    fill = [(dict(o, dst=last - 1) if o.get("dst") == last - 2 else o, rc, frag) for o, rc, frag in tl.SHARED]
    record(tl, "dcp_fill_holes_2d", tl.FILL, tl.FILL_ORDER, fill, lambda o: tl.call("dcp_fill_holes_2d", tl.FILL, tl.FILL_ORDER, o))
    record(tl, "dcp_label_measures_2d", tl.MEAS, tl.MEAS_ORDER, tl.MEAS_CASES, lambda o: tl.call("dcp_label_measures_2d", tl.MEAS, tl.MEAS_ORDER, o))
    for symbol, (valid, order) in tb.CALLS.items():
        record(tb, symbol, valid, order, [c[1:] for c in tb.REFUSALS if c[0] == symbol], lambda o, symbol=symbol: tb.call(symbol, o))
    assert not any("0x" in c["message"] for c in cases), "a message carries an address: mask it"
    path = os.path.join(OUT, "plane_refusals.json")
    with open(path, "w") as f:
        json.dump({"entries": entries, "cases": cases}, f, indent=1)
        f.write("\n")
    print("plane_refusals.json  %d cases of %d entry points" % (len(cases), len(entries)))


if "--plane-refusals" in sys.argv[1:]:
    plane_refusals()
    raise SystemExit(0)


# ---- G30: discorpy.proc.processing (what discorpy_amd/proc/processing.py restates): what every public function of the reference's
# module returns on three sets of grouped lines, the float32 tables under them, and the metric matrices of find_cod_fine.
#   A  the reference's own unit-test grid (tests/test_processing.py): 31 x 31 points at pitch 2, moved along their rays from
#      (33, 35) by 1 - 2e-3 r; point_dist 2;
#   B  the lines the reference grouped from G29's image a at roi 0.9 (hor2 / ver2: after the residual filter), point_dist its dist;
#   C  a 13 x 18 grid at pitch 32 in a 480 x 640 frame, centre (300, 250), factor 1 - 8e-5 r, Gaussian noise of 0.3 px (seed in the
#      file); P is the same points pushed through a mild homography (G30_HOMOGRAPHY).
# find_cod_fine depends on where BFGS stops (the metric minimises per line and candidate), so a case is recorded only where the
# reference's own choice is stable: on both passes, the gap between the smallest and the second-smallest entry of its metric matrix is
# at least 10 times the largest difference between that matrix and the same matrix with the exact minimiser (the real roots of the
# cubic derivative).  C's seed is the first from G30_FIRST_SEED on that passes; B is left out of that one function if it does not.
# Runs alone as   python tools/gen_golden.py --g30   (it needs g29_dot_grid.npz, which a full run writes before it).
G30_HOMOGRAPHY = [1.0, 0.012, 2.0, -0.009, 1.0, 3.0, 2.0e-5, -3.0e-5]
G30_FIRST_SEED = 3000
G30_RATIO = 10.0


def g30():
    import inspect
    import time
    import types
    import warnings

    def split(pts, lens):
        return np.split(f64(pts), np.cumsum(lens)[:-1])

    def radial_grid(ys, xs, xc, yc, k):
        y, x = np.meshgrid(f64(ys), f64(xs), indexing="ij")
        r = np.sqrt((x - xc) ** 2 + (y - yc) ** 2)
        fact = 1.0 - k * r
        return np.stack([yc + (y - yc) * fact, xc + (x - xc) * fact], axis=-1)          # (rows, columns, 2) of (y, x)

    def lines_of(grid):
        return [np.array(row) for row in grid], [np.array(col) for col in grid.transpose(1, 0, 2)]

    def homography(grid, c):
        y, x = grid[..., 0], grid[..., 1]
        den = c[6] * x + c[7] * y + 1.0
        return np.stack([(c[3] * x + c[4] * y + c[5]) / den, (c[0] * x + c[1] * y + c[2]) / den], axis=-1)

    class ExactMinimiser:
        """Stands in for scipy.optimize inside the reference's _calc_error: the global minimum of t**2 + (a t**2 + b t + c)**2."""
        @staticmethod
        def minimize(fun, x0, args=()):
            a, b, c = (np.float64(v) for v in args)
            roots = np.roots([2 * a * a, 3 * a * b, b * b + 2 * a * c + 1.0, b * c])
            real = roots[np.abs(roots.imag) < 1e-9 * (1.0 + np.abs(roots.real))].real
            return types.SimpleNamespace(x=np.array([real[np.argmin(fun(real, a, b, c))]]))

    def metric_matrix(hor, ver, xc, yc, shifts, exact):
        """The matrix inside the reference's _calc_metric: its own code runs, _calc_error's return values are collected."""
        values, inner, solver = [], proc._calc_error, proc.optimize

        def recorder(ch, cv):
            values.append(inner(ch, cv))
            return values[-1]
        proc._calc_error = recorder
        if exact:
            proc.optimize = ExactMinimiser
        try:
            chosen = proc._calc_metric(hor, ver, xc, yc, shifts, shifts)
        finally:
            proc._calc_error, proc.optimize = inner, solver
        mat = np.asarray(values, dtype=np.float32).reshape(len(shifts), len(shifts)).T          # filled [i, j] with j outermost
        row, col = np.unravel_index(mat.argmin(), mat.shape)
        assert (shifts[col], shifts[row]) == chosen
        return mat, (int(row), int(col))

    def fine_search(hor, ver, xc, yc, point_dist):
        """(recorded arrays, the two ratios) of find_cod_fine from (xc, yc)."""
        rec, ratios = {}, []
        cx, cy = xc, yc
        for name, shifts in (("pass1", np.arange(-point_dist, point_dist + 2.0, 2.0)), ("pass2", np.arange(-2.0, 2.5, 0.5))):
            mat, (row, col) = metric_matrix(hor, ver, cx, cy, shifts, False)
            exact, _ = metric_matrix(hor, ver, cx, cy, shifts, True)
            two = np.sort(mat.astype(np.float64).ravel())[:2]
            gap, moved = two[1] - two[0], np.abs(mat.astype(np.float64) - exact.astype(np.float64)).max()
            ratios.append(gap / moved)
            rec["metric_" + name], rec["index_" + name], rec["gap_" + name] = mat, np.array([row, col], np.int64), np.float64(gap)
            cx, cy = cx + shifts[col], cy + shifts[row]
        t0 = time.perf_counter()
        got = proc.find_cod_fine(hor, ver, xc, yc, point_dist)
        rec["seconds"] = np.float64(time.perf_counter() - t0)
        assert got == (cx, cy)
        rec["center"], rec["ratios"], rec["start"], rec["point_dist"] = f64(got), f64(ratios), f64([xc, yc]), np.float64(point_dist)
        return rec, ratios

    def groups_present(hor, ver, xc, yc):
        ch, cv = proc._para_fit_hor(hor, xc, yc)[0], proc._para_fit_ver(ver, xc, yc)[0]
        return all(n > 0 for n in ((ch[:, 0] > 0).sum(), (ch[:, 0] < 0).sum(), (cv[:, 0] > 0).sum(), (cv[:, 0] < 0).sum()))

    out = {}

    def lines_out(key, lines):
        out[key + "_pts"] = f64(np.concatenate(lines))
        out[key + "_len"] = np.array([len(line) for line in lines], np.int64)

    def tag(v):
        return v if isinstance(v, str) else "f%g" % v

    # ---- the line sets
    ticks = np.arange(1, 63, 2.0)
    hor_a, ver_a = lines_of(radial_grid(ticks, ticks, 33.0, 35.0, 2e-3))
    g29 = np.load(os.path.join(OUT, "g29_dot_grid.npz"))
    hor_b, ver_b = split(g29["hor2_a_90_pts"], g29["hor2_a_90_len"]), split(g29["ver2_a_90_pts"], g29["ver2_a_90_len"])
    clean_c = radial_grid(np.arange(40, 480 - 40 + 1, 32), np.arange(40, 640 - 40 + 1, 32), 300.0, 250.0, 8e-5)
    assert clean_c.shape == (13, 18, 2)
    point_dist_c = 6.0
    for seed in range(G30_FIRST_SEED, G30_FIRST_SEED + 40):
        noisy = clean_c + np.random.default_rng(seed).normal(0.0, 0.3, clean_c.shape)
        hor_c, ver_c = lines_of(noisy)
        xc, yc = (float(v) for v in proc.find_cod_coarse(hor_c, ver_c))
        fine_c, ratios = fine_search(hor_c, ver_c, xc, yc, point_dist_c)
        print("g30 C seed %d: ratios %.3g %.3g, %.2f s" % (seed, ratios[0], ratios[1], fine_c["seconds"]))
        if min(ratios) >= G30_RATIO:
            break
    else:
        raise AssertionError("no seed passes the condition")
    out["c_seed"], out["homography"] = np.int64(seed), f64(G30_HOMOGRAPHY)
    hor_p, ver_p = lines_of(homography(noisy, G30_HOMOGRAPHY))
    sets = {"a": (hor_a, ver_a, 2.0), "b": (hor_b, ver_b, float(g29["dist_a_90"])), "c": (hor_c, ver_c, point_dist_c),
            "p": (hor_p, ver_p, point_dist_c)}
    centers = {}
    for key, (hor, ver, dist) in sets.items():
        lines_out(key + "_hor", hor)
        lines_out(key + "_ver", ver)
        out[key + "_point_dist"] = np.float64(dist)
        # ---- centres; every later call takes the coarse centre as Python floats
        coarse = proc.find_cod_coarse(hor, ver)
        out[key + "_coarse"] = f64(coarse)
        xc, yc = centers[key] = (float(coarse[0]), float(coarse[1]))
        for it in (1, 2):
            out["%s_bailey_it%d" % (key, it)] = f64(proc.find_cod_bailey(hor, ver, iteration=it))
        # ---- float32 tables
        out[key + "_para_hor"], shifted = proc._para_fit_hor(hor, xc, yc)
        out[key + "_para_ver"] = proc._para_fit_ver(ver, xc, yc)[0]
        assert out[key + "_para_hor"].dtype == np.float32 and shifted[0].dtype == np.float64
        out[key + "_linear_hor"], out[key + "_linear_ver"] = proc._generate_linear_coef(hor, ver)
        out[key + "_linear_hor_center"], out[key + "_linear_ver_center"] = proc._generate_linear_coef(hor, ver, xc, yc)
        # ---- undistorted intercepts and the three radial fits
        for opt in (False, True):
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                out["%s_uc_hor_opt%d" % (key, opt)], out["%s_uc_ver_opt%d" % (key, opt)] = proc._calc_undistor_intercept(
                    hor, ver, xc, yc, optimizing=opt)
                for nf in (3, 5):
                    name = "%s_nf%d_opt%d" % (key, nf, opt)
                    out["backward_" + name] = proc.calc_coef_backward(hor, ver, xc, yc, nf, optimizing=opt)
                    out["forward_" + name] = proc.calc_coef_forward(hor, ver, xc, yc, nf, optimizing=opt)
                    out["bff_f_" + name], out["bff_b_" + name] = proc.calc_coef_backward_from_forward(hor, ver, xc, yc, nf, optimizing=opt)
            out["%s_warned_opt%d" % (key, opt)] = np.bool_(any(issubclass(w.category, UserWarning) for w in caught))
        # ---- the reversed model of the backward fit, on the default grid and on the case's own points
        own = np.concatenate(shifted + proc._para_fit_ver(ver, xc, yc)[1])
        for nf in (3, 5):
            back = out["backward_%s_nf%d_opt0" % (key, nf)]
            out["transform_%s_nf%d_default_backward" % (key, nf)] = proc.transform_coef_backward_and_forward(back)
            out["transform_%s_nf%d_default_forward" % (key, nf)] = proc.transform_coef_backward_and_forward(back, mapping="forward")
            out["transform_%s_nf%d_points_backward" % (key, nf)] = proc.transform_coef_backward_and_forward(back, ref_points=own)
            out["transform_%s_nf%d_points_forward" % (key, nf)] = proc.transform_coef_backward_and_forward(back, mapping="forward", ref_points=own)
        # ---- what post makes of the calibration (the reference's own functions), for the image-to-calibration test
        back3 = out["backward_%s_nf3_opt0" % key]
        out[key + "_check_hor"] = np.bool_(post.check_distortion(post.calc_residual_hor(post.unwarp_line_backward(hor, xc, yc, back3), xc, yc)))
        out[key + "_check_ver"] = np.bool_(post.check_distortion(post.calc_residual_ver(post.unwarp_line_backward(ver, xc, yc, back3), xc, yc)))
        # ---- regenerated grids
        out[key + "_grid_linear_hor"], out[key + "_grid_linear_ver"] = proc.regenerate_grid_points_linear(hor, ver)
        gh, gv = proc.regenerate_grid_points_linear(out[key + "_linear_hor"], out[key + "_linear_ver"], is_coef=True)
        assert np.array_equal(gh, out[key + "_grid_linear_hor"]) and np.array_equal(gv, out[key + "_grid_linear_ver"])
        for pers, find in ((False, False), (False, True), (True, False)):
            name = "%s_grid_parabola_p%d_c%d" % (key, pers, find)
            out[name + "_hor"], out[name + "_ver"] = proc.regenerate_grid_points_parabola(hor, ver, perspective=pers, find_center=find)
            assert out[name + "_hor"].dtype == np.float32 and out[name + "_hor"].shape == (len(hor), len(ver), 2)
        moved = proc.update_center(shifted, xc, yc)
        out[key + "_update_center"] = f64(np.concatenate(moved))
    # ---- a deleted middle line: the warning about missing lines
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        xc, yc = centers["c"]
        proc.calc_coef_backward(hor_c[:6] + hor_c[7:], ver_c, xc, yc, 3)
    out["c_warned_line6_deleted"] = np.bool_(any(issubclass(w.category, UserWarning) for w in caught))
    assert out["c_warned_line6_deleted"] and not out["c_warned_opt0"] and not out["a_warned_opt0"]
    # ---- find_cod_fine: A, C (its seed was chosen above), B where the condition holds
    fine_a, ratios_a = fine_search(hor_a, ver_a, *centers["a"], 2.0)
    assert min(ratios_a) >= G30_RATIO, ratios_a
    fine_b, ratios_b = fine_search(hor_b, ver_b, *centers["b"], sets["b"][2])
    print("g30 fine: A ratios %.3g %.3g (%.2f s); B ratios %.3g %.3g (%.2f s)"
          % (ratios_a[0], ratios_a[1], fine_a["seconds"], ratios_b[0], ratios_b[1], fine_b["seconds"]))
    fine_cases = [("a", fine_a), ("c", fine_c)] + ([("b", fine_b)] if min(ratios_b) >= G30_RATIO and fine_b["seconds"] < 5.0 else [])
    out["fine_cases"] = np.array([k for k, _ in fine_cases])
    out["fine_b_ratios"], out["fine_b_seconds"] = fine_b["ratios"], fine_b["seconds"]          # recorded whether or not B is a case
    for key, rec in fine_cases:
        for name, value in rec.items():
            out["fine_%s_%s" % (key, name)] = value
    # ---- vanishing points (barrel distortion: A, C and P), and the iteration with the perspective effect taken out
    for key in ("a", "c", "p"):
        hor, ver, _ = sets[key]
        out[key + "_vanishing"] = f64(proc.find_center_based_vanishing_points(hor, ver))
        assert groups_present(hor, ver, *centers[key])
    for key in ("c", "p"):
        hor, ver, _ = sets[key]
        for it in (1, 2):
            for method in ("mean", "median", "min", "max"):
                out["%s_vanishing_it%d_%s" % (key, it, method)] = f64(proc.find_center_based_vanishing_points_iteration(hor, ver, it, method))
    # the vanishing-point functions took their own way, not Bailey's
    saved = proc.find_cod_bailey

    def no_bailey(*args, **kwargs):
        raise AssertionError("fell back to find_cod_bailey")
    proc.find_cod_bailey = no_bailey
    try:
        for key in ("a", "c", "p"):
            proc.find_center_based_vanishing_points(sets[key][0], sets[key][1])
        proc.find_center_based_vanishing_points_iteration(hor_p, ver_p, 2, "mean")
    finally:
        proc.find_cod_bailey = saved
    # ---- the perspective route on P: undistorted lines, point pairs, four points, coefficients, corrected lines
    scales = ("mean", "median", "min", "max", 0.9)
    for scale in scales:
        for opt in (False, True):
            name = "p_undistorted_%s_opt%d" % (tag(scale), opt)
            out[name + "_hor"], out[name + "_ver"] = proc.generate_undistorted_perspective_lines(hor_p, ver_p, True, scale, opt)
            out["p_uintercept_%s_opt%d_hor" % (tag(scale), opt)], out["p_uintercept_%s_opt%d_ver" % (tag(scale), opt)] = \
                proc._calc_undistor_intercept_perspective(hor_p, ver_p, True, scale, opt)
        name = "p_undistorted_%s_unequal" % tag(scale)
        out[name + "_hor"], out[name + "_ver"] = proc.generate_undistorted_perspective_lines(hor_p, ver_p, False, scale, True)
        src, tgt = proc.generate_source_target_perspective_points(hor_p, ver_p, True, scale, True)
        out["p_source_%s" % tag(scale)], out["p_target_%s" % tag(scale)] = src, tgt
        for mapping in ("backward", "forward"):
            out["p_perspective_coef_%s_%s" % (tag(scale), mapping)] = proc.calc_perspective_coefficients(src, tgt, mapping)
    grid = out["p_grid_linear_hor"]
    four = np.array([grid[2, 14], grid[10, 3], grid[2, 3], grid[10, 14]])                  # (y, x), in no particular order
    out["four_points"] = four
    for order in ("yx", "xy"):
        given = four if order == "yx" else np.fliplr(four)
        for equal in (False, True):
            for scale in ("mean", "min", "max", 0.9):
                name = "four_%s_eq%d_%s" % (order, equal, tag(scale))
                out[name + "_source"], out[name + "_target"] = proc.generate_4_source_target_perspective_points(given, order, equal, scale)
                if order == "yx":
                    for mapping in ("backward", "forward"):
                        out[name + "_coef_" + mapping] = proc.calc_perspective_coefficients(out[name + "_source"], out[name + "_target"], mapping)
    xc, yc = centers["p"]
    for method in ("mean", "median", "min", "max"):
        for scale in ("mean", "max", 0.9):
            got_hor, got_ver = proc.correct_perspective_effect(hor_p, ver_p, xc, yc, method, scale)
            assert [len(line) for line in got_hor] == [len(line) for line in hor_p]
            out["p_effect_%s_%s_hor" % (method, tag(scale))] = f64(np.concatenate(got_hor))
            out["p_effect_%s_%s_ver" % (method, tag(scale))] = f64(np.concatenate(got_ver))
    # ---- refusals: the exception and its message
    refused = []
    for name, call in (("four_three_points", lambda: proc.generate_4_source_target_perspective_points(four[:3])),
                       ("four_five_points", lambda: proc.generate_4_source_target_perspective_points(np.concatenate([four, four[:1]]))),
                       ("four_flat_xy", lambda: proc.generate_4_source_target_perspective_points(four.ravel(), "xy")),
                       ("coef_flat_points", lambda: proc.calc_perspective_coefficients(four.ravel(), four.ravel())),
                       ("coef_no_points", lambda: proc.calc_perspective_coefficients(np.zeros((0, 2)), np.zeros((0, 2)))),
                       ("coef_unequal_counts", lambda: proc.calc_perspective_coefficients(four, four[:3]))):
        try:
            call()
        except Exception as err:
            refused.append((name, type(err).__name__, str(err)))
        else:
            raise AssertionError(name + ": the reference accepts it")
    out["refusal_names"], out["refusal_types"], out["refusal_messages"] = (np.array(col) for col in zip(*refused))
    # ---- names and signatures
    names = sorted(n for n, f in inspect.getmembers(proc, inspect.isfunction) if f.__module__ == proc.__name__ and not n.startswith("_"))
    out["public_names"] = np.array(names)
    out["signatures"] = np.array([str(inspect.signature(getattr(proc, n))) for n in names])
    assert "find_cod_fine" in names and "update_center" in names
    save("g30_proc", **out)
    size = os.path.getsize(os.path.join(OUT, "g30_proc.npz"))
    assert size <= 400 << 10, size


if "--g30" in sys.argv[1:]:
    g30()
    raise SystemExit(0)


# ---- G31: the rest of discorpy.prep.preprocessing (what discorpy_amd/prep/threshold.py, pointgrid.py and complete.py restate), skimage
# stubbed as for G26-G30: calculate_threshold on small images of five element types, parabola masks (np.packbits), the point-list
# functions on recorded points, both polyfit groupings on a barrel-distorted grid, and the module's public names with their signatures.
# The grid: 15 x 17 points at pitch 40 about (400, 450), pulled towards the centre by 1 / (1 + G31_BARREL r^2) and turned by the slope
# 0.02 -- strong enough that group_dots_hor_lines / group_dots_ver_lines alone lose outer points (asserted here), weak enough that the
# polyfit groupings with G31_GROUP return every row and column.  Runs alone as   python tools/gen_golden.py --g31
G31_BARREL = 3.5e-6
G31_SLOPE = 0.02
G31_PITCH = 40.0
G31_GROUP = dict(ratio=0.15, num_dot_miss=2)
G31_THRESHOLDS = [("float32", (48, 64), "bright", 2.0), ("float32", (40, 30), "dark", 1.5), ("float64", (40, 56), "bright", 3.0),
                  ("float64", (33, 47), "dark", 2.0), ("uint8", (96, 128), "bright", 2.0), ("uint8", (50, 70), "dark", 3.0),
                  ("uint16", (64, 48), "bright", 1.5), ("uint16", (31, 77), "dark", 2.0), ("int16", (48, 64), "bright", 2.0),
                  ("int16", (45, 45), "dark", 1.5), ("float32", (32, 64), "bright", 2.0)]          # (the last one: a constant middle half)
G31_MASKS = [dict(height=60, width=80, hor_curviness=0.3, ver_curviness=0.2, hor_margin=(10, 14), ver_margin=(6, 9), rotate=0.0),
             dict(height=64, width=64, hor_curviness=0.4, ver_curviness=0.4, hor_margin=8, ver_margin=8, rotate=7.5),
             dict(height=50, width=70, hor_curviness=0.1, ver_curviness=0.1, hor_margin=35, ver_margin=(20, 30), rotate=0.0)]


def g31_grid():
    rows, cols = 15, 17
    yy, xx = np.meshgrid((np.arange(rows) - rows // 2) * G31_PITCH, (np.arange(cols) - cols // 2) * G31_PITCH, indexing="ij")
    pull = 1.0 / (1.0 + G31_BARREL * (yy ** 2 + xx ** 2))
    y, x = yy * pull, xx * pull
    a = np.arctan(G31_SLOPE)
    pts = np.column_stack(((y * np.cos(a) + x * np.sin(a) + 400.0).ravel(), (-y * np.sin(a) + x * np.cos(a) + 450.0).ravel()))
    return pts[np.random.default_rng(7).permutation(len(pts))]


def g31():
    import inspect
    import types
    for name in ("skimage", "skimage.filters", "skimage.segmentation", "skimage.morphology", "skimage.measure", "skimage.transform"):
        sys.modules.setdefault(name, types.ModuleType(name))
    for mod, attr in (("skimage.filters", "threshold_otsu"), ("skimage.segmentation", "clear_border"), ("skimage.transform", "radon")):
        if not hasattr(sys.modules[mod], attr):
            setattr(sys.modules[mod], attr, None)
    import discorpy.prep.preprocessing as ref
    out = {}
    # ---- thresholds: a bright (dark) background with a gradient and noise, darker (brighter) dots on it
    rng = np.random.default_rng(3100)
    out["thres_dtype"] = np.array([c[0] for c in G31_THRESHOLDS])
    out["thres_bgr"] = np.array([c[2] for c in G31_THRESHOLDS])
    out["thres_snr"] = f64([c[3] for c in G31_THRESHOLDS])
    values = []
    for i, (dt, shape, bgr, snr) in enumerate(G31_THRESHOLDS):
        yy, xx = np.mgrid[:shape[0], :shape[1]]
        base = 0.7 + 0.1 * xx / shape[1] + 0.02 * np.round(rng.standard_normal(shape), 2)
        dots = ((yy % 12 - 6) ** 2 + (xx % 12 - 6) ** 2) < 9
        img = np.where(dots, 0.2 + 0.02 * np.round(rng.standard_normal(shape), 2), base)
        if bgr == "dark":
            img = 1.0 - img
        if i == len(G31_THRESHOLDS) - 1:
            flat = np.sort(img.ravel())
            flat[len(flat) // 4 - 8:3 * len(flat) // 4 + 8] = flat[len(flat) // 4 - 8]          # the middle half of the sorted values is one number
            img = flat[rng.permutation(len(flat))].reshape(shape)
        scale = {"float32": 1.0, "float64": 1.0, "uint8": 255.0, "uint16": 60000.0, "int16": 30000.0}[dt]
        img = (img * scale - (15000.0 if dt == "int16" else 0.0))
        img = np.round(img).astype(dt) if np.dtype(dt).kind in "iu" else img.astype(dt)
        out["thres_img%d" % i] = img
        values.append(ref.calculate_threshold(img, bgr=bgr, snr=snr))
    out["thres_value"] = f64(values)
    assert abs(np.polyfit(np.arange(8.0), np.full(8, 0.5), 1)[0]) < 1e-15
    # ---- parabola masks and the points they keep
    pts_rng = np.random.default_rng(3101)
    for i, kw in enumerate(G31_MASKS):
        mask = ref.make_parabola_mask(**kw)
        assert mask.dtype == np.float32 and set(np.unique(mask)) <= {0.0, 1.0}
        out["mask%d_bits" % i] = np.packbits(mask.astype(bool))
        # (also above and left of the frame: the truncation of -0.5 is 0, inside; further out the frame test discards the point)
        pts = np.column_stack((pts_rng.uniform(-5.0, kw["height"] - 0.01, 300), pts_rng.uniform(-5.0, kw["width"] - 0.01, 300)))
        out["mask%d_points" % i] = pts
        out["mask%d_kept" % i] = ref.remove_points_using_parabola_mask(pts, **kw)
    out["mask_args"] = np.array([repr(kw) for kw in G31_MASKS])
    # ---- rotate_points, remove_subset_points
    pts = pts_rng.uniform(0.0, 500.0, (40, 2))
    out["rot_points"] = pts
    out["rot_deg"] = ref.rotate_points(pts, 12.5)
    out["rot_rad"] = ref.rotate_points(pts, -0.3, degree_unit=False)
    out["subset_selected"] = pts[[3, 7, 7, 20]]
    out["subset_left"] = ref.remove_subset_points(pts[[3, 7, 7, 20]], pts)
    # ---- the polyfit groupings: the whole grid, two points removed, one outlier added
    grid = g31_grid()
    plain_h = sum(len(line) for line in ref.group_dots_hor_lines(grid, G31_SLOPE, G31_PITCH))
    plain_v = sum(len(line) for line in ref.group_dots_ver_lines(grid, G31_SLOPE, G31_PITCH))
    assert plain_h < len(grid) and plain_v < len(grid), (plain_h, plain_v)
    out["grid_plain_counts"] = np.array([plain_h, plain_v], np.int64)
    holes = np.delete(grid, [10, 100], axis=0)
    outlier = np.vstack([grid, [[409.0, 463.0]]])
    for name, pts in (("full", grid), ("holes", holes), ("outlier", outlier)):
        hor = ref.group_dots_hor_lines_based_polyfit(pts, G31_SLOPE, G31_PITCH, **G31_GROUP)
        ver = ref.group_dots_ver_lines_based_polyfit(pts, G31_SLOPE, G31_PITCH, **G31_GROUP)
        print("g31 grid %-8s rows %s columns %s" % (name, [len(line) for line in hor], [len(line) for line in ver]))
        out["grid_%s_points" % name] = pts
        for tag, lines in (("hor", hor), ("ver", ver)):
            out["grid_%s_%s_len" % (name, tag)] = np.array([len(line) for line in lines], np.int64)
            out["grid_%s_%s" % (name, tag)] = np.vstack(lines)
    assert list(out["grid_full_hor_len"]) == [17] * 15 and list(out["grid_full_ver_len"]) == [15] * 17
    # ---- names and signatures
    names = sorted(n for n, f in inspect.getmembers(ref, inspect.isfunction) if f.__module__ == ref.__name__ and not n.startswith("_"))
    out["public_names"] = np.array(names)
    out["signatures"] = np.array([str(inspect.signature(getattr(ref, n))) for n in names])
    private = ["_get_nearby_hor_points", "_get_nearby_hor_points_iter", "_get_nearby_ver_points", "_get_nearby_ver_points_iter"]
    out["private_names"] = np.array(private)
    out["private_signatures"] = np.array([str(inspect.signature(getattr(ref, n))) for n in private])
    save("g31_prep_rest", **out)
    size = os.path.getsize(os.path.join(OUT, "g31_prep_rest.npz"))
    assert size <= 400 << 10, size


if "--g31" in sys.argv[1:]:
    g31()
    raise SystemExit(0)


# ---- G32: select_good_peaks of discorpy.prep.linepattern (skimage stubbed as for G26-G31).  Cases of small profiles with candidate peaks
# and the arguments; per peak, for the float64 rows and for the same rows as float32: the reference's decision with and without
# use_offset (select_good_peaks on that one peak), the reference's four values (check, c, d, num) read through _get_gauss_peak_fit and the
# lines of select_good_peaks, and the same four from a refit with curve_fit's tolerances at 1e-14 and maxfev 20000.  delta = 4 x the 99th
# percentile, over the peaks where both fits succeed and differ by less than 0.05 in each quantity, of the largest difference among
# (c, d, num) between the two fits: the reference's own sensitivity to where its iteration stops.  A peak is CLEAR when the two fits give
# the same decision and, wherever a fit succeeded, | |c| - radius // 2 |, |num - tol| and (use_offset) | |d| - tol | are at least delta.
# Runs alone as   python tools/gen_golden.py --g32
G32_RADII = (3, 7, 11)
G32_HOPELESS_RADII = (3, 7)      # the noise row, the ramp and the square wave
G32_TOL = 0.2
G32_MAX_UNCLEAR = 0.15
G32_MIN_PER_CLASS = 20
G32_CLASSES = ("kept", "shift", "percentile", "offset", "raised")


def g32_rows():
    """(rows (27, 160), candidates per row): 6 kinds of line rows x 4 noise strengths, then a noise row, a ramp and a square wave."""
    rng = np.random.default_rng(32)
    x = np.arange(160.0)
    centres = np.arange(14.0, 150.0, 21.0) + np.array([0.0, 0.3, -0.4, 0.2, 0.45, -0.25, 0.1])

    def bumps(width, heights, base):
        return base + sum(h * np.exp(-0.5 * ((x - c) / width) ** 2) for c, h in zip(centres, heights))
    h_even = np.array([1.0, 0.8, 1.2, 0.6, 1.0, 0.9, 1.1])
    kinds = [bumps(1.0, h_even, 0.1), bumps(1.6, h_even[::-1], 0.3), bumps(2.4, h_even, 0.0), bumps(3.4, 0.7 * h_even, 0.5),
             # one shoulder on every line: a second, lower line 4 samples to the right
             bumps(1.5, h_even, 0.2) + sum(0.45 * h * np.exp(-0.5 * ((x - c - 4.0) / 1.5) ** 2) for c, h in zip(centres, h_even)),
             # flat-topped bumps: a line clipped at 55 % of its height
             np.minimum(bumps(2.5, np.ones(7), 0.0), 0.55) + 0.1]
    rows, cands = [], []
    for kind in kinds:
        for noise in (0.0, 0.01, 0.03, 0.08):
            rows.append(kind + noise * rng.standard_normal(160))
            on = np.round(centres).astype(np.int64)
            cands.append(np.concatenate((on, on - 1, on[::2] + 2, on[1::2] - 4, on[1::2] + 1)))
    every9 = np.arange(0, 160, 9)
    rows += [0.5 + 0.2 * rng.standard_normal(160), 0.01 * x + 0.25, ((x // 20) % 2).astype(np.float64)]
    cands += [every9, every9, every9]
    return np.asarray(rows), cands


def g32():
    import functools
    import types
    import warnings
    from scipy.optimize import curve_fit
    for name in ("skimage", "skimage.filters", "skimage.segmentation", "skimage.morphology", "skimage.measure", "skimage.transform"):
        sys.modules.setdefault(name, types.ModuleType(name))
    for mod, attr in (("skimage.filters", "threshold_otsu"), ("skimage.segmentation", "clear_border"), ("skimage.transform", "radon")):
        if not hasattr(sys.modules[mod], attr):
            setattr(sys.modules[mod], attr, None)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        import discorpy.prep.linepattern as rlp
    tight_fit = functools.partial(curve_fit, ftol=1e-14, xtol=1e-14, gtol=1e-14, maxfev=20000)

    def four(list_data, p, radius):
        """(check, c, d, num) of one peak: the lines of the reference's select_good_peaks around its own _get_gauss_peak_fit."""
        start, stop = max(0, p - radius), min(len(list_data), p + radius + 1)
        if stop - start <= 3:
            return [0.0, np.nan, np.nan, np.nan]
        list_sub = list_data[start:stop]
        std = np.std(list_sub)
        if std == 0.0:
            return [0.0, np.nan, np.nan, np.nan]
        list_norm = (list_sub - np.min(list_sub)) / std
        fit_data, del_x, offset, check = rlp._get_gauss_peak_fit(list_norm)
        return [float(check), float(del_x), float(offset), float(np.percentile(np.abs(fit_data - list_norm), 80))]

    def decide(v, radius, tol, use_offset):
        return bool(v[0]) and abs(v[1]) < radius // 2 and v[3] < tol and (not use_offset or abs(v[2]) < tol)

    rows, cands = g32_rows()
    # one row of 600 samples for radius 128: three wide lines, a little noise
    xb = np.arange(600.0)
    big = 0.2 + sum(h * np.exp(-0.5 * ((xb - c) / w) ** 2) for c, h, w in ((130.3, 1.0, 18.0), (300.0, 0.8, 26.0), (470.6, 1.2, 12.0)))
    big = big + 0.01 * np.random.default_rng(33).standard_normal(600)
    vec1 = np.array([0, 1.5, 5, 1.5, 0, 0, 3, 10, 3, 0])                       # the reference's two test vectors (test_linepattern.py:53-67)
    vec2 = np.array([0, 1, 2, 9, 2, 1, 0, 0, 3, 10, 3, 0, 0], np.float64)      # (an integer array there: scipy smooths it in its own type)
    # (name, rows, candidates per row, radius, tol, sigma)
    cases = [("r%d" % r, rows[:24], cands[:24], r, G32_TOL, 0.0) for r in G32_RADII]
    cases += [("h%d" % r, rows[24:], cands[24:], r, G32_TOL, 0.0) for r in G32_HOPELESS_RADII]
    cases.append(("big", big[None, :], [np.array([130, 300, 471, 120, 310, 480, 70, 215, 385, 560, 128, 129, 299, 301, 470, 472])], 128, G32_TOL, 0.0))
    cases.append(("vec1", vec1[None, :], [np.array([2, 7])], 3, 0.1, 0.0))
    cases.append(("vec2", vec2[None, :], [np.array([3, 9])], 3, 0.3, 1.0))
    cases.append(("smooth", rows[[3, 7, 11, 19, 22]], [cands[k] for k in (3, 7, 11, 19, 22)], 7, G32_TOL, 1.5))
    out = dict(case_names=np.array([c[0] for c in cases]), radius=np.array([c[3] for c in cases], np.int64), tol=f64([c[4] for c in cases]),
               sigma=f64([c[5] for c in cases]))
    measured = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for name, crow, ccand, radius, tol, sigma in cases:
            out[name + "_rows"] = f64(crow)
            out[name + "_row_of"] = np.concatenate([np.full(len(c), k, np.int32) for k, c in enumerate(ccand)])
            out[name + "_idx"] = np.concatenate(ccand).astype(np.int32)
            for dt in ("float64", "float32"):
                ref, tight, keep = [], [], []
                for k, peaks in enumerate(ccand):
                    data = crow[k].astype(dt)
                    smooth = ndi.gaussian_filter1d(data, sigma) if sigma > 0 else data
                    for p in peaks:
                        p = int(p)
                        ref.append(four(smooth, p, radius))
                        rlp.curve_fit = tight_fit
                        try:
                            tight.append(four(smooth, p, radius))
                        finally:
                            rlp.curve_fit = curve_fit
                        keep.append([len(rlp.select_good_peaks(data, [p], tol=tol, radius=radius, sigma=sigma, use_offset=uo)) == 1 for uo in (True, False)])
                        assert keep[-1] == [decide(ref[-1], radius, tol, uo) for uo in (True, False)]
                measured[name, dt] = (f64(ref), f64(tight), np.array(keep))
    # delta: over every case and both element types
    diffs = []
    for ref, tight, _ in measured.values():
        both = (ref[:, 0] == 1) & (tight[:, 0] == 1)
        d = np.abs(ref[both, 1:] - tight[both, 1:])
        diffs.append(d[(d < 0.05).all(axis=1)].max(axis=1))
    p99 = float(np.percentile(np.concatenate(diffs), 99))
    delta = 4.0 * p99
    out["p99"], out["delta"] = np.float64(p99), np.float64(delta)
    total, unclear = 0, 0
    counts = dict.fromkeys(G32_CLASSES, 0)
    for (name, dt), (ref, tight, keep) in measured.items():
        radius, tol = int(out["radius"][list(out["case_names"]).index(name)]), float(out["tol"][list(out["case_names"]).index(name)])
        clear = np.empty((len(ref), 2), bool)
        for i in range(len(ref)):
            for j, uo in enumerate((True, False)):
                ok = decide(ref[i], radius, tol, uo) == decide(tight[i], radius, tol, uo)
                for v in (ref[i], tight[i]):
                    if v[0] == 1:
                        margins = [abs(abs(v[1]) - radius // 2), abs(v[3] - tol)] + ([abs(abs(v[2]) - tol)] if uo else [])
                        ok = ok and min(margins) >= delta
                clear[i, j] = ok
            if clear[i, 0]:
                v, t = ref[i], tight[i]
                if keep[i, 0]:
                    counts["kept"] += 1
                elif v[0] == 0 and np.isfinite(v[3]):                     # (the fit raised -- not a window rejected before any fit)
                    counts["raised"] += 1
                elif v[0] == 1 and abs(v[1]) >= radius // 2:
                    counts["shift"] += 1
                elif v[0] == 1 and v[3] >= tol:
                    counts["percentile"] += 1
                elif v[0] == 1:
                    counts["offset"] += 1
        key = "%s_%s_" % (name, "f64" if dt == "float64" else "f32")
        out[key + "ref"], out[key + "tight"], out[key + "keep"], out[key + "clear"] = ref, tight, keep, clear
        total += clear.size
        unclear += int((~clear).sum())
        print("g32 %-7s %-7s peaks %4d kept %4d / %4d clear %4d / %4d" % (name, dt, len(ref), keep[:, 0].sum(), keep[:, 1].sum(), clear[:, 0].sum(),
                                                                       clear[:, 1].sum()))
    out["unclear_share"] = np.float64(unclear / total)
    print("g32 p99 %.4g delta %.4g unclear %.2f %% classes %s" % (p99, delta, 100.0 * unclear / total, counts))
    assert unclear <= G32_MAX_UNCLEAR * total, (unclear, total)
    assert min(counts.values()) >= G32_MIN_PER_CLASS, counts
    save("g32_select_peaks", **out)
    assert os.path.getsize(os.path.join(OUT, "g32_select_peaks.npz")) <= 400 << 10


if "--g32" in sys.argv[1:]:
    g32()
    raise SystemExit(0)


# ---- G33: select_peaks=True of discorpy.prep.linepattern as its callers reach it (get_local_extrema_points, the two cross-point functions,
# the two slope-and-distance functions; skimage stubbed as for G32, radon <- the NumPy restatement as for G28).  The reference's module-level
# select_good_peaks is wrapped by a recorder, so every candidate the reference judged is seen: per candidate its decision, the four
# values (check, c, d, num) of G32 from the reference's fit and from the tight refit, and `clear` by G32's rule with G32's recorded delta.
#   tables   the 27 rows of g32_rows() with option="max", float64 and the same rows as float32, radii 3, 7, 11, three sets of kwargs,
#            subpixel both ways (the selection is the same; both returns are stored), denoise / norm each both ways on a subset
#   images   G27's line and tall images, G28's big one and a 240 x 260 image of lines of sigma 2.5 at pitch 30 (where the selection removes
#            points), through both cross-point functions with the flag, with default kwargs and with {tol: 0.3, use_offset: False}
#   slopes   G28's cases with the flag
# Everything is stored flat: one row of `tb_case` / `im_case` per call, the candidates of all calls end to end.
# Runs alone as   python tools/gen_golden.py --g33
G33_KWARGS = ({}, dict(tol=0.3, use_offset=False), dict(sigma=1.5))
G33_SUBSET = (0, 5, 10, 15, 20, 24)          # rows that also go through denoise / norm


def g33_wide_image():
    rng = np.random.default_rng(3333)
    h, w, dist, sigma = 240, 260, 30.0, 2.5
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    t = np.deg2rad(1.5)
    u, v = x * np.cos(t) + y * np.sin(t) + 7.3, -x * np.sin(t) + y * np.cos(t) + 11.9
    du, dv = (u + dist / 2) % dist - dist / 2, (v + dist / 2) % dist - dist / 2
    img = 1.0 - 0.8 * np.maximum(np.exp(-du * du / (2 * sigma ** 2)), np.exp(-dv * dv / (2 * sigma ** 2)))
    return (img * (0.75 + 0.2 * x / w + 0.1 * y / h) * (1.0 + 0.01 * rng.standard_normal((h, w)))).astype(np.float32)


def g33():
    import functools
    import json
    import types
    import warnings
    from scipy.optimize import curve_fit
    for name in ("skimage", "skimage.filters", "skimage.segmentation", "skimage.morphology", "skimage.measure", "skimage.transform"):
        sys.modules.setdefault(name, types.ModuleType(name))
    for mod, attr in (("skimage.filters", "threshold_otsu"), ("skimage.segmentation", "clear_border"), ("skimage.transform", "radon")):
        if not hasattr(sys.modules[mod], attr):
            setattr(sys.modules[mod], attr, None)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        import discorpy.prep.linepattern as rlp
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from helpers import radon_reference as rr
    tight_fit = functools.partial(curve_fit, ftol=1e-14, xtol=1e-14, gtol=1e-14, maxfev=20000)
    g32_file = np.load(os.path.join(OUT, "g32_select_peaks.npz"))
    delta = float(g32_file["delta"])
    g27_file, g28_file = np.load(os.path.join(OUT, "g27_cross_points.npz")), np.load(os.path.join(OUT, "g28_slope_distance.npz"))

    def four(list_data, p, radius):
        start, stop = max(0, p - radius), min(len(list_data), p + radius + 1)
        if stop - start <= 3:
            return [0.0, np.nan, np.nan, np.nan]
        list_sub = list_data[start:stop]
        std = np.std(list_sub)
        if std == 0.0:
            return [0.0, np.nan, np.nan, np.nan]
        list_norm = (list_sub - np.min(list_sub)) / std
        fit_data, del_x, offset, check = rlp._get_gauss_peak_fit(list_norm)
        return [float(check), float(del_x), float(offset), float(np.percentile(np.abs(fit_data - list_norm), 80))]

    def decide(v, radius, tol, use_offset):
        return bool(v[0]) and abs(v[1]) < radius // 2 and v[3] < tol and (not use_offset or abs(v[2]) < tol)

    def is_clear(ref, tight, radius, tol, use_offset):
        ok = decide(ref, radius, tol, use_offset) == decide(tight, radius, tol, use_offset)
        for v in (ref, tight):
            if v[0] == 1:
                margins = [abs(abs(v[1]) - radius // 2), abs(v[3] - tol)] + ([abs(abs(v[2]) - tol)] if use_offset else [])
                ok = ok and min(margins) >= delta
        return ok

    calls = []           # one entry per call of select_good_peaks: (candidates, kept, ref, tight, clear)
    original = rlp.select_good_peaks

    def recorder(list_data, peaks, tol=0.2, radius=11, sigma=0, use_offset=True):
        got = original(list_data, peaks, tol=tol, radius=radius, sigma=sigma, use_offset=use_offset)
        smooth = ndi.gaussian_filter1d(list_data, sigma) if sigma > 0 else list_data
        cand, kept, ref, tight, clear = [], [], [], [], []
        for p in peaks:
            p = int(p)
            ref.append(four(smooth, p, radius))
            rlp.curve_fit = tight_fit
            try:
                tight.append(four(smooth, p, radius))
            finally:
                rlp.curve_fit = curve_fit
            cand.append(p)
            kept.append(p in got)
            assert kept[-1] == decide(ref[-1], radius, tol, use_offset)
            clear.append(is_clear(ref[-1], tight[-1], radius, tol, use_offset))
        calls.append((np.array(cand, np.int32), np.array(kept, bool), f64(ref).reshape(-1, 4), f64(tight).reshape(-1, 4), np.array(clear, bool)))
        return got

    def flagged(fn, *args, **kw):
        """fn(*args, select_peaks=True, **kw) under the recorder: (what it returns, the calls it made)."""
        del calls[:]
        rlp.select_good_peaks = recorder
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                got = fn(*args, select_peaks=True, **kw)
        finally:
            rlp.select_good_peaks = original
        return got, list(calls)

    out = {}
    classes = dict.fromkeys(G32_CLASSES, 0)
    total = unclear = 0
    # ---- tables
    rows, _ = g32_rows()
    out["tb_rows"] = f64(rows)
    out["kw_tol"] = f64([kw.get("tol", 0.2) for kw in G33_KWARGS])
    out["kw_sigma"] = f64([kw.get("sigma", 0) for kw in G33_KWARGS])
    out["kw_use_offset"] = np.array([kw.get("use_offset", True) for kw in G33_KWARGS])
    plans = [(r, radius, k, dt, False, False) for dt in (0, 1) for radius in G32_RADII for k in range(len(G33_KWARGS)) for r in range(len(rows))]
    plans += [(r, 7, 0, dt, dn, nm) for dt in (0, 1) for dn, nm in ((True, False), (False, True), (True, True)) for r in G33_SUBSET]
    case, cand, kept, ref, tight, clear, ints, subs = [], [], [], [], [], [], [], []
    ncand = nret = 0
    for r, radius, k, dt, dn, nm in plans:
        row = rows[r].astype(np.float32 if dt else np.float64)
        kw = G33_KWARGS[k]
        got_int, made = flagged(rlp.get_local_extrema_points, row, option="max", radius=radius, denoise=dn, norm=nm, subpixel=False, **kw)
        got_sub, again = flagged(rlp.get_local_extrema_points, row, option="max", radius=radius, denoise=dn, norm=nm, subpixel=True, **kw)
        assert len(made) == len(again) == 1 and np.array_equal(made[0][0], again[0][0]) and np.array_equal(made[0][1], again[0][1])
        c, kp, rf, tg, cl = made[0]
        got_int, got_sub = np.asarray(got_int), f64(got_sub)
        assert len(got_int) == len(got_sub) == kp.sum() and np.array_equal(got_int, c[kp])
        assert got_int.dtype == (np.int64 if len(got_int) else np.float64)
        case.append([r, radius, k, dt, int(dn), int(nm), ncand, len(c), nret, len(got_int), int(cl.all())])
        ncand += len(c)
        nret += len(got_int)
        cand.append(c), kept.append(kp), ref.append(rf), tight.append(tg), clear.append(cl), ints.append(got_int.astype(np.int64)), subs.append(got_sub)
        uo, tol = kw.get("use_offset", True), kw.get("tol", 0.2)
        for i in np.flatnonzero(cl):
            v = rf[i]
            if kp[i]:
                classes["kept"] += 1
            elif v[0] == 0 and np.isfinite(v[3]):
                classes["raised"] += 1
            elif v[0] == 1 and abs(v[1]) >= radius // 2:
                classes["shift"] += 1
            elif v[0] == 1 and v[3] >= tol:
                classes["percentile"] += 1
            elif v[0] == 1 and uo:
                classes["offset"] += 1
        total += len(c)
        unclear += int((~cl).sum())
    out["tb_case"] = np.array(case, np.int64)            # row, radius, kwargs set, float32?, denoise, norm, first candidate, candidates, first returned, returned, all clear
    out["tb_cand"], out["tb_keep"], out["tb_clear"] = np.concatenate(cand), np.concatenate(kept), np.concatenate(clear)
    out["tb_ref"], out["tb_tight"] = np.concatenate(ref), np.concatenate(tight)
    out["tb_int"], out["tb_sub"] = np.concatenate(ints), np.concatenate(subs)
    print("g33 tables: %d calls, %d candidates, %d unclear, %d rows all clear, classes %s" % (len(case), total, unclear,
                                                                                            int(out["tb_case"][:, 10].sum()), classes))
    table_total, table_unclear = total, unclear
    # ---- images
    wide = g33_wide_image()
    out["img_wide"] = wide
    images = dict(line=(g27_file["img_line"], 1.5, 20.0), tall=(g27_file["img_tall"], 1.5, 20.0), big=(g28_file["img_big"], 3.2, 30.0),
                  wide=(wide, 1.5, 30.0))
    im_names, im_case, im_pts = [], [], []
    npts = 0
    best_removed = None
    for key, (img, deg, dist) in images.items():
        slope = float(np.tan(np.deg2rad(deg)))
        for fn_name in ("hor", "ver"):
            fn = rlp.get_cross_points_hor_lines if fn_name == "hor" else rlp.get_cross_points_ver_lines
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                plain = fn(img, slope, dist)
            for k in (0, 1):
                pts, made = flagged(fn, img, slope, dist, **G33_KWARGS[k])
                pts = f64(pts).reshape(-1, 2)
                judged = int(sum(len(m[0]) for m in made))
                n_unclear = int(sum((~m[4]).sum() for m in made))
                assert judged == len(plain) and len(pts) == int(sum(m[1].sum() for m in made))
                im_names.append("%s_%s_%d" % (key, fn_name, k))
                im_case.append([k, npts, len(pts), judged, n_unclear, len(plain)])
                im_pts.append(pts)
                npts += len(pts)
                total += judged
                unclear += n_unclear
                removed = len(plain) - len(pts)
                if removed >= 10 and n_unclear < removed / 2.0 and (best_removed is None or removed > best_removed[1]):
                    best_removed = (im_names[-1], removed, n_unclear)
                print("g33 image %-12s points %4d of %4d, unclear %3d" % (im_names[-1], len(pts), len(plain), n_unclear))
    out["im_names"], out["im_case"], out["im_pts"] = np.array(im_names), np.array(im_case, np.int64), np.concatenate(im_pts)
    out["im_slope_deg"] = f64([images[n.split("_")[0]][1] for n in im_names])
    out["im_dist"] = f64([images[n.split("_")[0]][2] for n in im_names])
    # ---- slope and distance: G28's cases with the flag
    def radon(image, theta=None, circle=True):
        return rr.radon(image, theta=theta, circle=circle)
    sd_names, sd_vals = [], []
    for full in g28_file["case_names"]:
        full = str(full)
        mat = g28_file["img_" + str(g28_file["image_" + full])]
        prepare, kw = str(g28_file["prepare_" + full]), json.loads(str(g28_file["args_" + full]))
        if prepare == "invert":
            mat = mat.max() - mat
        if prepare == "float64":
            mat = mat.astype(np.float64)
        fn = rlp.calc_slope_distance_hor_lines if full.endswith("_hor") else rlp.calc_slope_distance_ver_lines
        rlp.radon = radon
        try:
            (slope, dist), made = flagged(fn, mat, **kw)
        finally:
            rlp.radon = None
        assert len(made) == 1 and slope == float(g28_file["slope_" + full])
        all_clear = bool(made[0][4].all())
        total += len(made[0][0])
        unclear += int((~made[0][4]).sum())
        sd_names.append(full)
        sd_vals.append([slope, dist, float(all_clear), float(len(made[0][0])), float(made[0][1].sum())])
        print("g33 slope %-12s slope %+.7f distance %.4f (without the flag %.4f), candidates %d kept %d, all clear %s" % (
            full, slope, dist, float(g28_file["dist_" + full]), len(made[0][0]), made[0][1].sum(), all_clear))
    out["sd_names"], out["sd_vals"] = np.array(sd_names), f64(sd_vals)
    out["delta"], out["unclear_share"] = np.float64(delta), np.float64(unclear / total)
    out["table_unclear_share"] = np.float64(table_unclear / table_total)
    print("g33: %d candidates, unclear %.2f %%, classes %s, best image %s" % (total, 100.0 * unclear / total, classes, best_removed))
    # what the tests rely on
    assert unclear <= G32_MAX_UNCLEAR * total, (unclear, total)
    assert min(classes.values()) >= G32_MIN_PER_CLASS, classes
    assert best_removed is not None
    assert sum(1 for v in sd_vals if v[2] == 1.0 and np.isfinite(v[1])) >= 2
    save("g33_select_wired", **out)
    assert os.path.getsize(os.path.join(OUT, "g33_select_wired.npz")) <= 1 << 20


if "--g33" in sys.argv[1:]:
    g33()
    raise SystemExit(0)


# ---- G1: the reference's own unwarp_image_backward test input (tests/test_postprocessing.py:77-85)
hei = wid = 64
mat = np.zeros((hei, wid), dtype=np.float32)
mat[4:-3, 4:-3] = 1.0
fact = [1.0, 3.0 * 10 ** (-3)]
save("g1_box64", mat=mat, xcenter=f64(wid // 2), ycenter=f64(hei // 2), list_fact=f64(fact),
     out_order1=post.unwarp_image_backward(mat, wid // 2, hei // 2, fact),
     out_order0=post.unwarp_image_backward(mat, wid // 2, hei // 2, fact, order=0))

# ---- G2: the reference's slice / chunk test volume (tests/test_postprocessing.py:98-123)
mat = np.zeros((hei, wid), dtype=np.float32)
mat[:, 6:-8:8] = 1.0
mat = np.float32(ndi.binary_dilation(np.int16(mat), iterations=1))
mat3d = np.zeros((10, hei, wid), dtype=np.float32)
mat3d[:] = mat
x0, y0 = wid // 2, hei // 2
save("g2_stripes10x64x64", mat=mat, depth=np.int64(10), xcenter=f64(x0), ycenter=f64(y0), list_fact=f64(fact),
     index=np.int64(y0), slice_out=post.unwarp_slice_backward(mat3d, x0, y0, fact, y0),
     start=np.int64(y0 - 5), stop=np.int64(y0 + 5),
     chunk_out=post.unwarp_chunk_slices_backward(mat3d, x0, y0, fact, y0 - 5, y0 + 5))

# ---- G3: the reference's perspective test (tests/test_postprocessing.py:205-238)
hor_line1 = np.asarray([[10.0 + 2 * i / 32, i] for i in range(64)])
hor_line2 = np.asarray([[60.0 - 5 * i / 32, i] for i in range(64)])
ver_line1 = np.asarray([[i, 5.0 + 3 * i / 32] for i in range(64)])
ver_line2 = np.asarray([[i, 60.0 - 3 * i / 32] for i in range(64)])
src_pts, tgt_pts = proc.generate_source_target_perspective_points(
    [hor_line1, hor_line2], [ver_line1, ver_line2], equal_dist=False, scale="mean", optimizing=False)
pers_f = proc.calc_perspective_coefficients(src_pts, tgt_pts, mapping="forward")
pers_b = proc.calc_perspective_coefficients(src_pts, tgt_pts, mapping="backward")
mat = np.zeros((64, 64), dtype=np.float32)
mat[10:11] = np.float32(1.0)
mat[45:46] = np.float32(0.5)
cor1 = post.correct_perspective_image(mat, pers_b)
cor2 = post.correct_perspective_image(cor1, pers_f)
save("g3_perspective64", mat=mat, coef_backward=f64(pers_b), coef_forward=f64(pers_f), cor_backward=cor1,
     cor_forward_of_backward=cor2, cor_backward_order0=post.correct_perspective_image(mat, pers_b, order=0))

# ---- G4: config 1 -- data/dot_pattern_05.jpg + data/coef_dot_05.txt.  The decoded JPEG is a data
# file of the reference; a 160x192 crop around the centre of distortion and eight full output rows
# are kept (JPEG decoding is library dependent: never decode on the GPU box).
from PIL import Image  # noqa: E402
img = np.array(Image.open("/root/reference/data/dot_pattern_05.jpg"), dtype=np.float32)
assert img.shape == configs.DOT_05_SHAPE
with open("/root/reference/data/coef_dot_05.txt") as fh:
    vals = [float(line.split()[-1]) for line in fh if line.strip()]
xc, yc, coef = vals[0], vals[1], vals[2:]
assert abs(xc - configs.XCENTER_DOT_05) < 1e-9 and len(coef) == 5
full = post.unwarp_image_backward(img, xc, yc, coef)
rows = np.array([0, 10, 137, 400, 462, 463, 700, 799])
crop = (slice(384, 544), slice(492, 684))      # 160 x 192 window holding the centre (462, 588)
crop_in = np.ascontiguousarray(img[crop])
# the same call on the crop alone (centre shifted): a self-contained input/output pair
crop_out = post.unwarp_image_backward(crop_in, xc - 492, yc - 384, coef)
save("g4_dot_pattern_05", crop_in=crop_in, crop_xcenter=f64(xc - 492), crop_ycenter=f64(yc - 384),
     list_fact=f64(coef), crop_out=crop_out, full_rows=rows, full_out_rows=full[rows],
     full_stats=f64([img.min(), img.max(), img.mean(), full.mean(), full[400, 640], full[10, 10], full[799, 1279]]),
     full_in_rows_band=img[395:406])

# ---- G4b: config 1 at full size -- the decoded 800 x 1280 frame as uint8 (mode L: the decode IS integers, so this
# is the float32 image the reference loads, losslessly), the SHA-256 of the reference's full float32 output and a
# 25 x 40 lattice of its pixels.  (The 4 MB output itself is not stored.)
import hashlib  # noqa: E402
assert np.array_equal(img, img.astype(np.uint8).astype(np.float32))
lat = (slice(0, 800, 32), slice(0, 1280, 32))
save("g4b_dot_pattern_05_full", frame_u8=img.astype(np.uint8), xcenter=f64(xc), ycenter=f64(yc), list_fact=f64(coef),
     out_sha256=np.frombuffer(hashlib.sha256(np.ascontiguousarray(full).tobytes()).digest(), dtype=np.uint8),
     out_lattice=np.ascontiguousarray(full[lat]), out_order0_sha256=np.frombuffer(hashlib.sha256(
         np.ascontiguousarray(post.unwarp_image_backward(img, xc, yc, coef, order=0)).tobytes()).digest(), dtype=np.uint8))

# ---- G5: configs 2 / 5 at reduced size, seeded noise; float32 coordinate planes kept
def coords_ref(h, w, xc, yc, fact):
    xu = np.arange(w) - xc
    yu = np.arange(h) - yc
    xm, ym = np.meshgrid(xu, yu)
    ru = np.sqrt(xm ** 2 + ym ** 2)
    fm = np.sum(np.asarray([f * ru ** i for i, f in enumerate(fact)]), axis=0)
    return (np.float32(np.clip(yc + fm * ym, 0, h - 1)), np.float32(np.clip(xc + fm * xm, 0, w - 1)))


for name, (h, w), seed, (xc5, yc5, fact5) in [
        ("g5_cfg2_160", (160, 160), 11, configs.rescale_model(160)),
        ("g5_offcentre_150x200", (150, 200), 12, (configs.rescale_model(200)[0] + 60.25,
                                                  configs.rescale_model(200)[1] - 37.5,
                                                  configs.rescale_model(200)[2])),
        ("g5_cfg5_9term_144", (144, 144), 13, (72.3, 77.7,
                                               [a * (8192 / 144) ** i for i, a in enumerate(configs.CFG5_FACT)]))]:
    im = np.random.default_rng(seed).random((h, w), dtype=np.float32)
    yd, xd = coords_ref(h, w, xc5, yc5, fact5)
    save(name, seed=np.int64(seed), shape=np.array([h, w]), xcenter=f64(xc5), ycenter=f64(yc5), list_fact=f64(fact5),
         yd=yd, xd=xd, out_order1=post.unwarp_image_backward(im, xc5, yc5, fact5),
         out_order0=post.unwarp_image_backward(im, xc5, yc5, fact5, order=0))

# ---- G6: slice / chunk on a (6, 800, 1280)-shaped problem, coef_dot_05, rows 0, 14, 400, 799
vol = np.random.default_rng(21).random((3, 800, 1280), dtype=np.float32)
c = configs
g6 = dict(seed=np.int64(21), shape=np.array(vol.shape), xcenter=f64(c.XCENTER_DOT_05), ycenter=f64(c.YCENTER_DOT_05),
          list_fact=f64(c.COEF_DOT_05), rows=np.array([0, 14, 400, 799]))
for r in (0, 14, 400, 799):
    g6["slice_%d" % r] = post.unwarp_slice_backward(vol, c.XCENTER_DOT_05, c.YCENTER_DOT_05, c.COEF_DOT_05, r)
g6["slice_frac_400p5"] = post.unwarp_slice_backward(vol, c.XCENTER_DOT_05, c.YCENTER_DOT_05, c.COEF_DOT_05, 400.5)
g6["chunk_395_402"] = post.unwarp_chunk_slices_backward(vol, c.XCENTER_DOT_05, c.YCENTER_DOT_05, c.COEF_DOT_05, 395, 402)
g6["chunk_0_2"] = post.unwarp_chunk_slices_backward(vol, c.XCENTER_DOT_05, c.YCENTER_DOT_05, c.COEF_DOT_05, 0, 2)
g6["chunk_797_799"] = post.unwarp_chunk_slices_backward(vol, c.XCENTER_DOT_05, c.YCENTER_DOT_05, c.COEF_DOT_05, 797, 799)
save("g6_stack3x800x1280", **g6)

# ---- G7: fused perspective -> radial, one map_coordinates call at the composed coordinates
h = w = 144
im = np.random.default_rng(31).random((h, w), dtype=np.float32)
s = 4096 / w
coef7 = list(configs.CFG3_COEF)
# rescale the 4096^2 homography to a 256^2 frame: x' = x/s  =>  c3,c6 / s ; c7,c8 * s
coef7 = [coef7[0], coef7[1], coef7[2] / s, coef7[3], coef7[4], coef7[5] / s, coef7[6] * s, coef7[7] * s]
xc7, yc7, fact7 = configs.rescale_model(w)
yp, xp = post._generate_perspective_map(im, coef7)
xp = np.float64(xp.reshape(h, w))
yp = np.float64(yp.reshape(h, w))
xu = xp - xc7
yu = yp - yc7
ru = np.sqrt(xu ** 2 + yu ** 2)
fm = np.sum(np.asarray([f * ru ** i for i, f in enumerate(fact7)]), axis=0)
xd = np.float32(np.clip(xc7 + fm * xu, 0, w - 1))
yd = np.float32(np.clip(yc7 + fm * yu, 0, h - 1))
fused = map_coordinates(im, (yd.reshape(-1, 1), xd.reshape(-1, 1)), order=1, mode="reflect").reshape(h, w)
twopass = post.correct_perspective_image(post.unwarp_image_backward(im, xc7, yc7, fact7), coef7)
save("g7_fused144", seed=np.int64(31), shape=np.array([h, w]), xcenter=f64(xc7), ycenter=f64(yc7), list_fact=f64(fact7),
     list_coef=f64(coef7), fused_out=fused, twopass_out=twopass, yd=yd, xd=xd,
     persp_out=post.correct_perspective_image(im, coef7))

# ---- G8: clipping stress -- 55 % of the coordinates clipped; all eight modes must agree
h, w = 120, 180
im = np.random.default_rng(41).random((h, w), dtype=np.float32)
fact8 = [1.3, 2e-3]
outs = {}
for order in (0, 1):
    base = post.unwarp_image_backward(im, 90.0, 60.0, fact8, order=order, mode="reflect")
    for mode in ("grid-mirror", "constant", "grid-constant", "nearest", "mirror", "grid-wrap", "wrap"):
        assert np.array_equal(base, post.unwarp_image_backward(im, 90.0, 60.0, fact8, order=order, mode=mode)), mode
    outs["out_order%d" % order] = base
yd, xd = coords_ref(h, w, 90.0, 60.0, fact8)
save("g8_clip120x180", seed=np.int64(41), shape=np.array([h, w]), xcenter=f64(90.0), ycenter=f64(60.0),
     list_fact=f64(fact8), clipped_fraction=f64(np.mean((xd == 0) | (xd == w - 1) | (yd == 0) | (yd == h - 1))), **outs)

# ---- G9: explicit coordinates incl. half-integers (order 0 rounds half up), edges, tiny fractions
im = np.random.default_rng(51).random((33, 47), dtype=np.float32)
ys = np.array([0.0, 0.5, 1.5, 2.5, 31.5, 32.0, 15.25, 7.999999, 1e-30, 31.999998, 0.49999997, 12.5, 20.0, 3.5],
              dtype=np.float32)
xs = np.array([0.0, 0.5, 2.5, 45.5, 46.0, 46.0, 22.75, 1e-20, 0.49999997, 45.999996, 10.5, 0.0, 46.0, 44.5],
              dtype=np.float32)
rng = np.random.default_rng(52)
ys = np.concatenate([ys, (rng.random(500) * 32).astype(np.float32)])
xs = np.concatenate([xs, (rng.random(500) * 46).astype(np.float32)])
yd64 = rng.random(300) * 32
xd64 = rng.random(300) * 46
save("g9_points33x47", seed=np.int64(51), shape=np.array([33, 47]), ys=ys, xs=xs,
     out_order0=map_coordinates(im, (ys, xs), order=0, mode="reflect"),
     out_order1=map_coordinates(im, (ys, xs), order=1, mode="reflect"),
     ys64=yd64, xs64=xd64, out64_order1=map_coordinates(im, (yd64, xd64), order=1, mode="reflect"),
     out64_order0=map_coordinates(im, (yd64, xd64), order=0, mode="reflect"))
# ---- G10: util.unwarp_color_image_backward (utility.py:278-342): channels, explicit pads, pad modes
import discorpy.util.utility as util  # noqa: E402
rgb = np.random.default_rng(61).random((40, 56, 3), dtype=np.float32)
fact10 = [1.0, 4e-3, 2e-5]
g10 = dict(seed=np.int64(61), shape=np.array(rgb.shape), xcenter=f64(27.4), ycenter=f64(19.1), list_fact=f64(fact10))
g10["nopad"] = util.unwarp_color_image_backward(rgb, 27.4, 19.1, fact10)
g10["pad_3_5_2_7_edge"] = util.unwarp_color_image_backward(rgb, 27.4, 19.1, fact10, pad=(3, 5, 2, 7), pad_mode="edge")
g10["pad_4_constant"] = util.unwarp_color_image_backward(rgb, 27.4, 19.1, fact10, pad=4)
g10["pad_4_reflect_order0"] = util.unwarp_color_image_backward(rgb, 27.4, 19.1, fact10, order=0, pad=4, pad_mode="reflect")
g10["gray_pad_6_mean"] = util.unwarp_color_image_backward(rgb[:, :, 1], 27.4, 19.1, fact10, pad=6, pad_mode="mean")
save("g10_color40x56x3", **g10)
# ---- G11: spline orders 2..5 (map_coordinates with prefilter), every boundary mode
im = np.random.default_rng(71).random((45, 60), dtype=np.float32)
fact11 = [1.0, 3e-3, 2e-5]
coef11 = [0.97, -0.02, 2.0, 0.015, 0.95, 1.5, -2e-4, 3e-4]
g11 = dict(seed=np.int64(71), shape=np.array(im.shape), xcenter=f64(31.3), ycenter=f64(21.8), list_fact=f64(fact11),
           list_coef=f64(coef11))
MODES = ("reflect", "grid-mirror", "constant", "grid-constant", "nearest", "mirror", "grid-wrap", "wrap")
for order in (2, 3, 4, 5):
    for mode in MODES:
        g11["radial_o%d_%s" % (order, mode)] = post.unwarp_image_backward(im, 31.3, 21.8, fact11, order=order, mode=mode)
for mode in MODES:
    g11["persp_o3_%s" % mode] = post.correct_perspective_image(im, coef11, order=3, mode=mode)   # demo_07.py:60 uses order=3
pts_y = (np.random.default_rng(72).random(500) * 44).astype(np.float32)
pts_x = (np.random.default_rng(73).random(500) * 59).astype(np.float32)
g11["pts_y"], g11["pts_x"] = pts_y, pts_x
for order in (2, 3, 4, 5):
    g11["points_o%d_reflect" % order] = map_coordinates(im, (pts_y, pts_x), order=order, mode="reflect")
save("g11_spline45x60", **g11)
# ---- G12: element types other than float32 (output dtype = input dtype; unwarp_slice_backward -> float32)
def typed_image(dt, shape, seed):
    rng = np.random.default_rng(seed)
    dt = np.dtype(dt)
    if dt.kind == "f":
        return (rng.random(shape) * 2000.0 - 700.0).astype(dt)
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max, size=shape, endpoint=True, dtype=np.int64).astype(dt)


g12 = dict(shape=np.array([40, 52]), xcenter=f64(24.6), ycenter=f64(20.3), list_fact=f64([1.0, 5e-3, 3e-5]),
           list_coef=f64([0.96, -0.03, 1.5, 0.02, 0.97, 1.0, -3e-4, 2e-4]), vol_shape=np.array([5, 40, 52]),
           index=np.int64(17), start=np.int64(8), stop=np.int64(21))
pts_y = (np.random.default_rng(82).random(400) * 39).astype(np.float32)
pts_x = (np.random.default_rng(83).random(400) * 51).astype(np.float32)
# exact halves between neighbouring integers: the integer stores round half away from zero
pts_y[:40] = np.repeat(np.arange(8, dtype=np.float32), 5)
pts_x[:40] = np.tile(np.array([0.5, 1.5, 2.5, 3.5, 4.0], dtype=np.float32), 8)
g12["pts_y"], g12["pts_x"] = pts_y, pts_x
for k, dt in enumerate(("uint8", "int8", "uint16", "int16", "uint32", "int32", "float64")):
    im = typed_image(dt, (40, 52), 800 + k)
    im[:8, :5] = np.arange(40).reshape(8, 5).astype(im.dtype) - (20 if np.dtype(dt).kind != "u" else 0)
    g12["seed_" + dt] = np.int64(800 + k)
    for order in (0, 1, 3):
        g12["radial_o%d_%s" % (order, dt)] = post.unwarp_image_backward(im, 24.6, 20.3, g12["list_fact"], order=order)
        g12["points_o%d_%s" % (order, dt)] = map_coordinates(im, (pts_y, pts_x), order=order, mode="reflect")
    g12["radial_o2_nearest_" + dt] = post.unwarp_image_backward(im, 24.6, 20.3, g12["list_fact"], order=2, mode="nearest")
    g12["persp_o1_" + dt] = post.correct_perspective_image(im, g12["list_coef"])
    g12["persp_o5_wrap_" + dt] = post.correct_perspective_image(im, g12["list_coef"], order=5, mode="grid-wrap")
    vol = typed_image(dt, (5, 40, 52), 900 + k)
    g12["slice_" + dt] = post.unwarp_slice_backward(vol, 24.6, 20.3, g12["list_fact"], 17)
    g12["chunk_" + dt] = post.unwarp_chunk_slices_backward(vol, 24.6, 20.3, g12["list_fact"], 8, 21)
    assert g12["radial_o1_" + dt].dtype == np.dtype(dt) and g12["chunk_" + dt].dtype == np.dtype(dt)
    assert g12["slice_" + dt].dtype == np.float32
save("g12_dtypes40x52", **g12)
# ---- G12b: the element types scipy reads as doubles with loss or stores through an undefined cast: int64, uint64 (taps above
# 2^53 round on the way in; a result of 2^63 / 2^64 -- any blend of taps at the type's maximum -- is stored as the x86-64
# cvttsd2si sequence stores it: INT64_MIN / 0) and bool (stored by truncating the double).  Inputs: conftest.wide_image.
def wide_image(dt, shape, seed):
    rng = np.random.default_rng(seed)
    if np.dtype(dt) == np.bool_:
        return rng.random(shape) < 0.5
    info = np.iinfo(dt)
    im = rng.integers(info.min, info.max, size=shape, endpoint=True, dtype=dt)
    flat = im.reshape(-1)
    flat[::7] = rng.integers(0, 1 << 20, size=flat[::7].shape).astype(dt)           # small values between the huge ones
    flat[3::11] = info.max
    flat[5::13] = info.min
    return im


g12b = dict(shape=np.array([40, 52]), xcenter=f64(24.6), ycenter=f64(20.3), list_fact=f64([1.0, 5e-3, 3e-5]),
            list_coef=g12["list_coef"], vol_shape=np.array([5, 40, 52]), index=np.int64(17), start=np.int64(8), stop=np.int64(21),
            pts_y=pts_y, pts_x=pts_x)
for k, dt in enumerate(("int64", "uint64", "bool")):
    im = wide_image(dt, (40, 52), 850 + k)
    g12b["seed_" + dt] = np.int64(850 + k)
    for order in (0, 1, 3):
        g12b["radial_o%d_%s" % (order, dt)] = post.unwarp_image_backward(im, 24.6, 20.3, g12b["list_fact"], order=order)
        g12b["points_o%d_%s" % (order, dt)] = map_coordinates(im, (pts_y, pts_x), order=order, mode="reflect")
    g12b["persp_o1_" + dt] = post.correct_perspective_image(im, g12b["list_coef"])
    vol = wide_image(dt, (5, 40, 52), 950 + k)
    g12b["slice_" + dt] = post.unwarp_slice_backward(vol, 24.6, 20.3, g12b["list_fact"], 17)
    g12b["chunk_" + dt] = post.unwarp_chunk_slices_backward(vol, 24.6, 20.3, g12b["list_fact"], 8, 21)
    assert g12b["radial_o1_" + dt].dtype == np.dtype(dt) and g12b["chunk_" + dt].dtype == np.dtype(dt) and g12b["slice_" + dt].dtype == np.float32
# complex data: scipy interpolates the real and the imaginary part separately
cim = (np.random.default_rng(861).random((40, 52)) + 1j * np.random.default_rng(862).random((40, 52))).astype(np.complex64)
g12b["radial_o1_complex64"] = post.unwarp_image_backward(cim, 24.6, 20.3, g12b["list_fact"])
g12b["persp_o1_complex64"] = post.correct_perspective_image(cim, g12b["list_coef"])
save("g12b_wide_types40x52", **g12b)
# ---- G13: unwarp_line_forward (postprocessing.py:36-64) on eight jittered dot lines of the 800 x 1280 pattern
rng13 = np.random.default_rng(5)
lines13 = [np.column_stack([np.full(12, 40.0 * k) + rng13.uniform(-2, 2, 12), np.linspace(5, 1270, 12) + rng13.uniform(-1, 1, 12)])
           for k in range(1, 9)]
fact13 = np.asarray([1.0, -2.9e-5, 8.9e-8, -1.5e-10, 8.0e-14])
save("g13_lines_forward", lines=np.asarray(lines13), xcenter=f64(588.69), ycenter=f64(462.09), list_fact=fact13,
     out=np.asarray(post.unwarp_line_forward(lines13, 588.69, 462.09, fact13)))
# ---- G19: correct_perspective_line (postprocessing.py:414-441) on the reference's own test lines (tests/test_postprocessing.py:
# 159-176): forward coefficients applied to the lines, backward coefficients applied to the result
hor19 = [np.asarray([[10.0 + 2 * i / 32, i] for i in range(32)]), np.asarray([[26.0 - 5 * i / 32, i] for i in range(32)])]
ver19 = [np.asarray([[i, 0.0 + 3 * i / 32] for i in range(32)]), np.asarray([[i, 20.0 - 3 * i / 32] for i in range(32)])]
src19, tgt19 = proc.generate_source_target_perspective_points(hor19, ver19, equal_dist=False, scale="mean", optimizing=False)
fcoef19 = proc.calc_perspective_coefficients(src19, tgt19, mapping="forward")
bcoef19 = proc.calc_perspective_coefficients(src19, tgt19, mapping="backward")
fwd19 = post.correct_perspective_line(hor19 + ver19, fcoef19)
save("g19_perspective_lines", lines=np.asarray(hor19 + ver19), fcoef=f64(fcoef19), bcoef=f64(bcoef19), forward=np.asarray(fwd19),
     back=np.asarray(post.correct_perspective_line(fwd19, bcoef19)))
# ---- G14: pad=True of util.unwarp_color_image_backward (utility.py:238-263): automatic pad widths from the forward
# model fitted by proc.transform_coef_backward_and_forward (processing.py:615-674), then the padded unwarp; plus the
# reference's own pad=True case (tests/test_utility.py:92-101) and the fitted coefficients themselves
rgb14 = np.random.default_rng(141).random((40, 56, 3), dtype=np.float32)
fact14 = [1.0, -6e-3, -2e-5]
g14 = dict(seed=np.int64(141), shape=np.array(rgb14.shape), xcenter=f64(27.4), ycenter=f64(19.1), list_fact=f64(fact14))
g14["pads"] = np.asarray(util._calc_pad(True, 40, 56, 27.4, 19.1, fact14), dtype=np.int64)
g14["pad_true_constant"] = util.unwarp_color_image_backward(rgb14, 27.4, 19.1, fact14, pad=True)
g14["pad_true_edge_order0"] = util.unwarp_color_image_backward(rgb14, 27.4, 19.1, fact14, order=0, pad=True, pad_mode="edge")
g14["gray_pad_true_reflect"] = util.unwarp_color_image_backward(rgb14[:, :, 2], 27.4, 19.1, fact14, pad=True, pad_mode="reflect")
grid14 = [[gy - 19.1, gx - 27.4] for gy in np.linspace(0, 40, 40) for gx in np.linspace(0, 56, 40)]
g14["forward_fact"] = f64(proc.transform_coef_backward_and_forward(fact14, ref_points=grid14))
g14["default_grid_backward"] = f64(proc.transform_coef_backward_and_forward([1.0, -3e-5, 9e-8]))
g14["default_grid_forward"] = f64(proc.transform_coef_backward_and_forward([1.0, -3e-5, 9e-8], mapping="forward"))
box = np.ones((40, 60), dtype=np.float32)      # tests/test_utility.py:75-101
box[:5] = 0
box[-5:] = 0
box[:, :5] = 0
box[:, -5:] = 0
ref14 = [[i - 20.0, j - 30.0] for i in range(0, 40, 10) for j in range(0, 60, 10)]
tfact14 = proc.transform_coef_backward_and_forward([1.0, 0.1, 0.01], ref_points=ref14)
g14["reftest_tfact"] = f64(tfact14)
g14["reftest_pads"] = np.asarray(util._calc_pad(True, 40, 60, 30.0, 20.0, tfact14), dtype=np.int64)
g14["reftest_pad_true"] = util.unwarp_color_image_backward(box, 30.0, 20.0, tfact14, 1, "constant", True, "constant")
save("g14_autopad40x56x3", **g14)

# G15: a FOLDING radial model on a chunk of rows -- the one documented deviation of the stack path that the reference's
# own tests never reach.  The reference crops the band [yd_min, yd_max) from the first row's minimum and the last row's
# maximum (postprocessing.py:289-301) and lets map_coordinates reflect inside that band; rows whose coordinates leave
# the band (possible only for a non-monotone map) therefore read reflected samples.  discorpy_amd samples the
# projection at the absolute coordinate.  The fixture pins both: the reference's output, the mask of pixels whose row
# coordinate leaves the band, and the absolute-coordinate result (scipy on the whole projection, same float32 coordinates).
def g15():
    d, h, w = 4, 64, 96
    xc, yc, fact = 48.3, 30.2, [1.0, 0.0, -4.0e-4]
    start, stop = 2, 20
    vol = np.random.default_rng(1515).random((d, h, w), dtype=np.float32)
    ref = post.unwarp_chunk_slices_backward(vol, xc, yc, fact, start, stop)
    xu = np.arange(0, w) - xc
    yu = np.arange(start, stop + 1) - yc
    xu_mat, yu_mat = np.meshgrid(xu, yu)
    ru = np.sqrt(xu_mat ** 2 + yu_mat ** 2)
    fm = np.sum(np.asarray([f * ru ** i for i, f in enumerate(fact)]), axis=0)
    xd = np.float32(np.clip(xc + fm * xu_mat, 0, w - 1))
    yd = np.float32(np.clip(yc + fm * yu_mat, 0, h - 1))
    yd_min = int(np.floor(np.amin(yd[0].astype(np.float64))))        # as the reference: first row's minimum,
    yd_max = int(np.ceil(np.amax(yd[-1].astype(np.float64)))) + 1    # last row's maximum (float64 there; same integers here)
    outside = (yd < yd_min) | (yd > yd_max - 1)
    absolute = np.asarray([map_coordinates(vol[i], (yd, xd), order=1, mode="reflect") for i in range(d)])
    assert outside.any() and not outside.all()
    assert np.array_equal(ref[:, ~outside], absolute[:, ~outside])
    assert not np.array_equal(ref[:, outside], absolute[:, outside])
    # the same chunk of a float64 and a uint16 stack (output dtype = input dtype): rows BELOW the band get a band-relative
    # coordinate larger in magnitude than the absolute one, where the reference's float32 subtraction yd_mat - yd_min rounds
    ref_f64 = post.unwarp_chunk_slices_backward(vol.astype(np.float64), xc, yc, fact, start, stop)
    ref_u16 = post.unwarp_chunk_slices_backward((vol * 60000).astype(np.uint16), xc, yc, fact, start, stop)
    # a second geometry whose rows leave the band on the low side by more than the coordinate itself
    vol2 = np.random.default_rng(1516).random((2, 55, 58), dtype=np.float32)
    case2 = (29.3, 8.4, [0.9105341112829652, -0.011490848185174918, -0.0006863296016646205], 46, 52)
    ref2 = post.unwarp_chunk_slices_backward(vol2, *case2)
    ref2_f64 = post.unwarp_chunk_slices_backward(vol2.astype(np.float64), *case2)
    save("g15_folding_chunk", seed=np.int64(1515), shape=np.array([d, h, w]), xcenter=f64(xc), ycenter=f64(yc),
         list_fact=f64(fact), start=np.int64(start), stop=np.int64(stop), ref_out=ref, outside_band=outside,
         absolute_out=absolute.astype(np.float32), band=np.array([yd_min, yd_max]), ref_out_f64=ref_f64, ref_out_u16=ref_u16,
         case2_seed=np.int64(1516), case2_shape=np.array([2, 55, 58]), case2_xcenter=f64(case2[0]), case2_ycenter=f64(case2[1]),
         case2_list_fact=f64(case2[2]), case2_rows=np.array(case2[3:]), case2_ref_out=ref2, case2_ref_out_f64=ref2_f64)


g15()


# G16: correct_perspective_image with a caller's map_index whose coordinates leave the image, under every boundary mode,
# orders 0 and 1 -- the reference passes map_index and mode straight to scipy (postprocessing.py:489-491), so this pins
# the out-of-image handling (scipy's coordinate mapping, tap folding, cval = 0) to the reference's own call.
def g16():
    h, w = 23, 31
    rng = np.random.default_rng(1616)
    mat = rng.random((h, w), dtype=np.float32)
    n = h * w                      # (the reference reshapes the result to the image's shape, :492)
    ys = (rng.random(n) * h * 7 - h * 3).astype(np.float32)
    xs = (rng.random(n) * w * 7 - w * 3).astype(np.float32)
    ys[:50] = np.linspace(-2.0, h + 1.0, 50)
    xs[:50] = 11.25
    out = {}
    coef = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]      # unused once map_index is given
    for mode in ("reflect", "grid-mirror", "constant", "grid-constant", "nearest", "mirror", "grid-wrap", "wrap"):
        for order in (0, 1):
            out["%s_o%d" % (mode.replace("-", "_"), order)] = post.correct_perspective_image(mat, coef, order=order, mode=mode,
                                                                                             map_index=(ys, xs))
    save("g16_map_index_outside", seed=np.int64(1616), shape=np.array([h, w]), ys=ys, xs=xs, **out)


g16()


# G17: small random frames (2..69 pixels a side) through unwarp_image_backward and correct_perspective_image at a random
# order 0..5 and boundary mode -- the regime where the spline prefilter's boundary handling (and scipy's quirks in it) is
# visible in every pixel.  60 cases; inputs regenerate from the seed.
def g17_case(rng):
    h, w = int(rng.integers(2, 70)), int(rng.integers(2, 70))
    img = rng.random((h, w), dtype=np.float32)
    xc, yc = float(rng.uniform(0, w)), float(rng.uniform(0, h))
    fact = [1.0, float(rng.uniform(-2e-3, 2e-3)), float(rng.uniform(-3e-5, 3e-5))]
    order = int(rng.integers(0, 6))
    mode = MODES_ALL[int(rng.integers(0, 8))]
    coef = [1 + rng.uniform(-.05, .05), rng.uniform(-.05, .05), rng.uniform(-3, 3), rng.uniform(-.05, .05),
            1 + rng.uniform(-.05, .05), rng.uniform(-3, 3), rng.uniform(-1e-4, 1e-4), rng.uniform(-1e-4, 1e-4)]
    return img, xc, yc, fact, order, mode, [float(c) for c in coef]


MODES_ALL = ("reflect", "grid-mirror", "constant", "grid-constant", "nearest", "mirror", "grid-wrap", "wrap")


def g17():
    rng = np.random.default_rng(1717)
    out = {}
    for k in range(60):
        img, xc, yc, fact, order, mode, coef = g17_case(rng)
        out["radial_%02d" % k] = post.unwarp_image_backward(img, xc, yc, fact, order=order, mode=mode)
        out["persp_%02d" % k] = post.correct_perspective_image(img, coef, order=order, mode=mode)
    save("g17_small_frames_orders_modes", seed=np.int64(1717), ncases=np.int64(60), **out)


g17()


# G18: unwarp_slice_backward with an `index` the reference does not validate (:215) -- fractional, negative, past the last row --
# on float32, uint16 and float64 stacks.  40 cases; inputs regenerate from the seed.
def g18_case(rng, t):
    d, h, w = int(rng.integers(1, 3)), int(rng.integers(3, 70)), int(rng.integers(3, 70))
    dt = [np.float32, np.uint16, np.float64][t % 3]
    vol = rng.random((d, h, w))
    vol = (vol * 60000).astype(dt) if dt == np.uint16 else vol.astype(dt)
    xc, yc = float(rng.uniform(-0.2 * w, 1.2 * w)), float(rng.uniform(-0.2 * h, 1.2 * h))
    fact = [1.0 + float(rng.uniform(-.1, .1)), float(rng.uniform(-3e-3, 3e-3)), float(rng.uniform(-1e-4, 1e-4))]
    idx = [float(rng.uniform(-5, h + 5)), int(rng.integers(-3, h + 3)), float(rng.integers(0, h)) + 0.5][(t // 3) % 3]
    return vol, xc, yc, fact, idx


def g18():
    rng = np.random.default_rng(1818)
    out = {}
    for t in range(40):
        vol, xc, yc, fact, idx = g18_case(rng, t)
        out["slice_%02d" % t] = post.unwarp_slice_backward(vol, xc, yc, fact, idx)
    save("g18_slice_any_index", seed=np.int64(1818), ncases=np.int64(40), **out)


g18()


# G20: the reference's losa/loadersaver on the files of tests/test_losa_hdf.py (h5py through tests/helpers/fake_h5py.py, images
# through PIL): what it reads from a seeded stack file, the errors it raises, the file it writes (index + datasets), the stream it
# opens, and the image files it writes (their bytes, PIL's decoding of them, and what its own load_image returns).
def g20():
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
    import fake_h5py
    sys.modules["h5py"] = fake_h5py
    from PIL import Image
    import discorpy.losa.loadersaver as ref
    out = {}
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "scan.nxs")
        vol = (np.random.default_rng(5).random((9, 14, 11)) * 60000).astype(">u2")          # test_losa_hdf._stack_file
        with fake_h5py.File(path, "w") as f:
            f.create_dataset("entry/data/data", data=vol)
            f.create_dataset("entry/angles", data=np.linspace(0.0, 180.0, 9))
        calls = [dict(key_path="entry/data/data"), dict(), dict(key_path="entry/data/data", index=3),
                 dict(key_path="entry/data/data", index=3, axis=1), dict(key_path="entry/data/data", index=3, axis=2),
                 dict(key_path="entry/data/data", index=(2, 7), axis=1), dict(key_path="entry/data/data", index=(1, 8, 3), axis=2),
                 dict(key_path="entry/data/data", index=[0, 2, 5, 6]), dict(key_path="entry/data/data", index=(4, 5), axis=1),
                 dict(key_path="entry/data/data", index=2, axis=7)]
        for k, kw in enumerate(calls):
            out["load_%d" % k] = ref.load_hdf_file(path, **kw)
        for k, (kw, fn) in enumerate(((dict(key_path="nope"), "load_hdf_file"), (dict(key_path="entry/data/data", index=(3, 3)), "load_hdf_file"),
                                      (dict(key_path="entry/none"), "load_hdf_object"))):
            try:
                getattr(ref, fn)(path, **kw)
            except ValueError as e:
                out["err_%d" % k] = np.array(str(e))
        v2 = np.arange(2 * 3 * 4, dtype=np.float32).reshape(2, 3, 4)
        a = str(ref.save_hdf_file(os.path.join(td, "ref_out.h5"), v2, key_path="entry/x"))
        out["saved_index"] = np.array(open(a).read())
        for fname in sorted(os.listdir(a + ".d")):
            out["saved_" + fname[:-4]] = np.load(os.path.join(a + ".d", fname))
        out["saved_read_back"] = ref.load_hdf_file(a)
        da = ref.open_hdf_stream(os.path.join(td, "ref_stream"), (2, 3, 4), key_path="entry/data", data_type="int16",
                                 options={"entry/energy": 53})
        out["stream_shape"], out["stream_dtype"], out["stream_name"] = np.array(da.shape), np.array(str(da.dtype)), np.array(da.name)
        out["stream_files"] = np.array(sorted(f for f in os.listdir(td) if f.startswith("ref_stream")))
        try:
            ref.open_hdf_stream(os.path.join(td, "r2.hdf"), (2, 2, 2), key_path="entry/data", options={"entry/data/angles": [1, 2]})
        except ValueError as e:
            out["err_stream"] = np.array(str(e))
        img = (np.random.default_rng(3).random((40, 52), dtype=np.float32) * 1000.0).astype(np.float32)      # conftest.noise(3, ...)
        for ext in ("tif", "png", "jpg"):
            p = str(ref.save_image(os.path.join(td, "ref_i." + ext), img))
            out["img_%s_file" % ext] = np.fromfile(p, dtype=np.uint8)
            with Image.open(p) as im:
                out["img_%s_mode" % ext], out["img_%s_pil" % ext] = np.array(im.mode), np.array(im)
            out["img_%s_load" % ext] = ref.load_image(p)
    save("g20_losa_reference", **out)


g20()


# G21: unwarp_image_forward (postprocessing.py:151-185), the scatter mat_unw[yu_mat, xu_mat] = mat.  Inputs come from
# tests/helpers/forward_emulation.py (g21_input: seeded frames, full-range element types, floats with NaN payloads and -0.0); the
# fixture keeps the parameters and the reference's outputs.  Every case that is not a tie case must keep all its unrounded coordinates
# at least 1e-9 px from a half-integer -- the kernels evaluate the polynomial in another order than NumPy (~4e-16 relative, < 1e-11 px
# on these frames), and only with that margin is bit equality with the reference a fair demand.  The margins are stored.
def g21():
    sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
    import forward_emulation as fe
    out = {}
    for name in fe.g21_names():
        mat, xc, yc, fact = fe.g21_input(name)
        res = post.unwarp_image_forward(mat, xc, yc, fact)
        assert res.dtype == mat.dtype and res.shape == mat.shape
        margin = fe.half_integer_margin(mat.shape[0], mat.shape[1], xc, yc, fact)
        if name.startswith("tie_"):
            assert margin == 0.0, (name, margin)
        else:
            assert margin >= 1e-9, "G21 case %s: a coordinate lies %.3g px from a half-integer; choose another model" % (name, margin)
        out["out_" + name], out["margin_" + name] = res, f64(margin)
        out["shape_" + name], out["xcenter_" + name], out["ycenter_" + name], out["list_fact_" + name] = (
            np.array(mat.shape), f64(xc), f64(yc), f64(fact))
    _, _, yf, xf = fe.forward_destinations(41, 57, 0.0, 0.0, [0.5])
    out["ties_tie_half"] = np.int64(np.count_nonzero((np.abs(yf - np.floor(yf) - 0.5) == 0) | (np.abs(xf - np.floor(xf) - 0.5) == 0)))
    assert out["ties_tie_half"] > 1000
    save("g21_forward_images", **out)


g21()


# G22: unwarp_line_backward (postprocessing.py:72-108; scipy.optimize.minimize per point) under two monotone models: the lines of the
# reference's own unit test (tests/test_postprocessing.py:36-59, 69-75) and a 15 x 20 grid over a 900 x 1200 frame plus the centre
# itself.  `*_dlines` = the grid under the model in NumPy (the reference test's construction), `*_ref` = the reference's answer,
# `*_min_dg` = the minimum of g'(ru) = sum (i + 1) a_i ru^i over [0, 1.01 max radius]: by the mean value theorem two radii whose
# equation residuals are e1 and e2 lie within (|e1| + |e2|) / min g' of each other.
def g22():
    def warp(lines, xc, yc, fact):
        res = []
        for line in lines:
            xu, yu = line[:, 1] - xc, line[:, 0] - yc
            ru = np.sqrt(xu ** 2 + yu ** 2)
            fl = np.sum(np.asarray([a * ru ** i for i, a in enumerate(fact)]), axis=0)
            res.append(np.asarray(list(zip(yc + yu * fl, xc + xu * fl))))
        return res

    out = {}
    unit = [np.asarray([[64 - y, x] for x in np.arange(1, 64, 2.0)]) for y in np.arange(1, 64, 2.0)]
    grid = [np.asarray([[y, x] for x in np.linspace(3.0, 1195.0, 20)]) for y in np.linspace(2.0, 897.0, 15)]
    grid.append(np.asarray([[450.7, 600.2]]))                                     # the centre itself
    for name, lines, xc, yc, fact in (("unit", unit, 33.5, 35.5, [1.0, -2.0e-3]), ("grid", grid, 600.2, 450.7, [1.0, 2.0e-4, 3.0e-7])):
        dlines = warp(lines, xc, yc, fact)
        ref = post.unwarp_line_backward(dlines, xc, yc, fact)
        rmax = max(np.sqrt((ln[:, 1] - xc) ** 2 + (ln[:, 0] - yc) ** 2).max() for ln in list(ref) + list(lines))
        r = np.linspace(0.0, 1.01 * rmax, 20001)
        dg = np.sum(np.asarray([(i + 1) * a * r ** i for i, a in enumerate(fact)]), axis=0)
        assert dg.min() > 0.1, (name, dg.min())                                   # monotone, with room
        out[name + "_xcenter"], out[name + "_ycenter"], out[name + "_list_fact"] = f64(xc), f64(yc), f64(fact)
        out[name + "_ulines"] = np.concatenate(lines)
        out[name + "_dlines"] = np.concatenate(dlines)
        out[name + "_ref"] = np.concatenate(ref)
        out[name + "_sizes"] = np.array([len(ln) for ln in lines])
        out[name + "_min_dg"] = f64(dg.min())
    save("g22_lines_backward", **out)


g22()


# G23: calc_residual_hor / calc_residual_ver / check_distortion (postprocessing.py:316-411) on warped and on corrected lines of the
# reference's unit test (tests/test_postprocessing.py:36-59, 125-157), both outcomes of the check present; and the names of the
# public functions of the reference's post module.
def g23():
    import inspect
    xc, yc = 33.5, 35.5
    hor = [np.asarray([[64 - y, x] for x in np.arange(1, 64, 2.0)]) for y in np.arange(1, 64, 2.0)]
    ver = [np.asarray([[64 - y, x] for y in np.arange(1, 64, 2.0)]) for x in np.arange(1, 64, 2.0)]

    def warp(lines, fact):
        res = []
        for line in lines:
            xu, yu = line[:, 1] - xc, line[:, 0] - yc
            ru = np.sqrt(xu ** 2 + yu ** 2)
            fl = np.sum(np.asarray([a * ru ** i for i, a in enumerate(fact)]), axis=0)
            res.append(np.asarray(list(zip(yc + yu * fl, xc + xu * fl))))
        return res

    out = dict(xcenter=f64(xc), ycenter=f64(yc))
    sets = {"hor_warped": (warp(hor, [1.0, -2.0e-2]), post.calc_residual_hor),
            "hor_corrected": (post.unwarp_line_forward(warp(hor, [1.0, -2.0e-3]), xc, yc, [1.0, 2.0e-3]), post.calc_residual_hor),
            "ver_warped": (warp(ver, [1.0, -2.0e-2]), post.calc_residual_ver),
            "ver_corrected": (post.unwarp_line_forward(warp(ver, [1.0, -2.0e-3]), xc, yc, [1.0, 2.0e-3]), post.calc_residual_ver)}
    checks = []
    for name, (lines, fn) in sets.items():
        res = fn(lines, xc, yc)
        out[name + "_lines"], out[name + "_residuals"] = np.asarray(lines), res
        out[name + "_check"] = np.bool_(post.check_distortion(res))
        checks.append(bool(out[name + "_check"]))
    assert True in checks and False in checks
    out["public_names"] = np.array(sorted(n for n, f in inspect.getmembers(post, inspect.isfunction)
                                          if f.__module__ == post.__name__ and not n.startswith("_")))
    save("g23_residuals", **out)


g23()


# G24: a colour photograph under a homography, as the reference's demos do it: examples/readthedocs_demo/demo_07.py:25,60 loops
# post.correct_perspective_image(mat[:, :, i], list_coef) over the channels (orders 1 and 3 there; order 0 added); and the one-pass
# perspective -> radial map per channel, formed exactly as G7 forms fused_out (one map_coordinates at the composed float32 planes).
# G10's frame (40 x 56 x 3), float32 and uint8 pixels, configs.CFG3_COEF rescaled as G7 rescales it.  Arrays only.
def g24():
    h, w, nc = 40, 56, 3
    seed = 2424
    rng = np.random.default_rng(seed)
    images = {"f32": rng.random((h, w, nc), dtype=np.float32) * np.float32(255.0),
              "u8": rng.integers(0, 256, (h, w, nc), dtype=np.uint8)}
    s = 4096 / w
    c = list(configs.CFG3_COEF)
    coef = [c[0], c[1], c[2] / s, c[3], c[4], c[5] / s, c[6] * s, c[7] * s]
    xc, yc, fact = configs.rescale_model(w)
    yp, xp = post._generate_perspective_map(images["f32"][:, :, 0], coef)
    xu = np.float64(xp.reshape(h, w)) - xc
    yu = np.float64(yp.reshape(h, w)) - yc
    ru = np.sqrt(xu ** 2 + yu ** 2)
    fm = np.sum(np.asarray([f * ru ** i for i, f in enumerate(fact)]), axis=0)
    xd = np.float32(np.clip(xc + fm * xu, 0, w - 1))
    yd = np.float32(np.clip(yc + fm * yu, 0, h - 1))
    out = dict(seed=np.int64(seed), shape=np.array([h, w, nc]), xcenter=f64(xc), ycenter=f64(yc), list_fact=f64(fact), list_coef=f64(coef),
               yd=yd, xd=xd)
    for tag, rgb in images.items():
        out["rgb_" + tag] = rgb
        for order in (1, 0, 3):
            planes = []
            for i in range(nc):                      # demo_07.py:25,60
                planes.append(post.correct_perspective_image(rgb[:, :, i], coef, order=order))
            out["persp_%s_o%d" % (tag, order)] = np.stack(planes, axis=2)
            out["fused_%s_o%d" % (tag, order)] = np.stack(
                [map_coordinates(rgb[:, :, i], (yd.reshape(-1, 1), xd.reshape(-1, 1)), order=order, mode="reflect").reshape(h, w)
                 for i in range(nc)], axis=2)
            assert out["persp_%s_o%d" % (tag, order)].dtype == rgb.dtype and out["fused_%s_o%d" % (tag, order)].dtype == rgb.dtype
    save("g24_colour_homography40x56x3", **out)


g24()


# G25: a colour image at spline orders 2..5 through util.unwarp_color_image_backward (utility.py:278-342 loops map_coordinates over
# mat_pad[:, :, i] with the caller's order and mode; examples/readthedocs_demo/demo_07.py:60 corrects a photograph with order=3).
# G10's frame and calibration, float32 and uint8 pixels: float32 at orders 2..5 under reflect / nearest / grid-wrap, uint8 at order 3
# under all eight modes, float32 at order 3 behind pad=4, pad_mode="edge".  Arrays only.
def g25():
    seed = 2510
    rng = np.random.default_rng(seed)
    rgb_f32 = rng.random((40, 56, 3), dtype=np.float32)
    rgb_u8 = rng.integers(0, 255, (40, 56, 3), endpoint=True).astype(np.uint8)
    xc, yc, fact = 27.4, 19.1, [1.0, 4e-3, 2e-5]
    modes = ["reflect", "grid-mirror", "constant", "grid-constant", "nearest", "mirror", "grid-wrap", "wrap"]
    out = dict(seed=np.int64(seed), shape=np.array(rgb_f32.shape), xcenter=f64(xc), ycenter=f64(yc), list_fact=f64(fact),
               rgb_f32=rgb_f32, rgb_u8=rgb_u8)
    for order in (2, 3, 4, 5):
        for mode in ("reflect", "nearest", "grid-wrap"):
            out["f32_o%d_%s" % (order, mode.replace("-", "_"))] = util.unwarp_color_image_backward(rgb_f32, xc, yc, fact, order=order, mode=mode)
    for mode in modes:
        out["u8_o3_%s" % mode.replace("-", "_")] = util.unwarp_color_image_backward(rgb_u8, xc, yc, fact, order=3, mode=mode)
    out["f32_o3_reflect_pad_4_edge"] = util.unwarp_color_image_backward(rgb_f32, xc, yc, fact, order=3, mode="reflect", pad=4, pad_mode="edge")
    for k, v in out.items():
        if k.startswith("f32_"):
            assert v.dtype == np.float32, k
        if k.startswith("u8_"):
            assert v.dtype == np.uint8 and v.shape == (40, 56, 3), k
    save("g25_colour_spline40x56x3", **out)


g25()


# G26: the Fourier Gaussian filter, discorpy.prep.preprocessing._apply_fft_filter and normalization_fft (preprocessing.py:76-158), on the
# cases of tests/test_fourier_gauss_gpu.py.  The module imports scikit-image at its top and never calls it in these two functions:
# empty stand-in modules carry the names, as fake_h5py stands in for h5py in G20.  Per case: the input, sigma / pad / mode, the
# reference's background plane and normalized result, and e_ref = max|reference - truth| / max|truth| with `truth` the same formula
# evaluated through dense long-double DFT matrices (the reference's own rounding error: the tolerance of the tests is a multiple of it).
# Images are uniform(50, 250) so that the background stays far from 0; integer types draw integers of that range (int8: up to 127),
# bool draws coin flips.  Arrays only.
def g26_cases():
    rng = np.random.default_rng(2626)

    def image(shape, dtype="float32"):
        dt = np.dtype(dtype)
        if dt == np.bool_:
            return rng.random(shape) < 0.5
        if dt.kind in "iu":
            return rng.integers(50, min(250, np.iinfo(dt).max), shape, endpoint=True).astype(dt)
        return rng.uniform(50.0, 250.0, shape).astype(dt)
    cases = []
    for shape in ((37, 52), (40, 51)):                                   # odd and even padded sides, the defaults and the cross-point sigma
        for sigma in (10, 5):
            cases.append(("s%dx%d_p100_s%d" % (shape + (sigma,)), image(shape), sigma, 100, "reflect"))
    cases.append(("full_50x61", image((50, 61)), 1, 20, "symmetric"))     # every tap kept
    cases.append(("full_30x45", image((30, 45)), 0.5, 10, "wrap"))
    cases.append(("narrow_64x48", image((64, 48)), 40, 100, "reflect"))   # support far narrower than the side
    cases.append(("pad0_33x47", image((33, 47)), 10, 0, "reflect"))
    for mode in ("reflect", "symmetric", "edge", "wrap", "constant"):     # the pad beyond the side: several folds
        cases.append(("folds_8x5_" + mode, image((8, 5)), 2, 23, mode))
    for shape in ((1, 9), (9, 1), (2, 2)):
        for mode in ("reflect", "symmetric"):
            cases.append(("tiny_%dx%d_%s" % (shape + (mode,)), image(shape), 2, 4, mode))
    for dt in ("float32", "float64", "int8", "uint8", "int16", "uint16", "int32", "uint32", "int64", "uint64", "bool"):
        cases.append(("type_" + dt, image((40, 51), dt), 3, 9, "reflect"))
    cases.append(("view_40x58", image((40, 58)), 3, 9, "reflect"))       # filtered as the view a[:, 3:-7]
    return cases


def g26_truth(mat, sigma, pad, mode):
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


def g26():
    import types
    import warnings
    for name in ("skimage", "skimage.filters", "skimage.segmentation", "skimage.morphology", "skimage.measure", "skimage.transform"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["skimage.filters"].threshold_otsu = None
    sys.modules["skimage.segmentation"].clear_border = None
    sys.modules["skimage.transform"].radon = None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        import discorpy.prep.preprocessing as rprep
    out = dict(names=[], sigma=[], pad=[], mode=[], e_ref=[])
    for name, mat, sigma, pad, mode in g26_cases():
        arg = mat[:, 3:-7] if name.startswith("view_") else mat
        bck = rprep._apply_fft_filter(arg, sigma, pad, mode)
        norm = rprep.normalization_fft(arg, sigma, pad, mode)
        truth = g26_truth(arg, sigma, pad, mode)
        assert bck.dtype == np.float64 and norm.dtype == np.float64 and bck.shape == arg.shape == norm.shape, name
        e_ref = float(np.abs(bck - truth).max() / np.abs(truth).max())
        assert 1e-17 < e_ref < 1e-14 and bck.min() > 0.05, (name, e_ref, bck.min())
        out["names"].append(name)
        out["sigma"].append(float(sigma))
        out["pad"].append(pad)
        out["mode"].append(mode)
        out["e_ref"].append(e_ref)
        out[name + "_in"], out[name + "_bck"], out[name + "_norm"] = mat, bck, norm
    for k in ("names", "mode"):
        out[k] = np.array(out[k])
    out["sigma"], out["pad"], out["e_ref"] = f64(out["sigma"]), np.array(out["pad"], np.int64), f64(out["e_ref"])
    save("g26_fourier_gauss", **out)


g26()


# ---- g27: the cross-point route of prep.linepattern (get_local_extrema_points, sliding_window_slope, get_cross_points_hor_lines /
# get_cross_points_ver_lines): what the reference's own functions return (skimage stubbed as for g26), for the peak tables, the slope rows
# and the image cases of tests/test_cross_points_{cpu,gpu}.py.  Images are stored as float32; a float64 case is their cast.
def g27_tables():
    rng = np.random.default_rng(2727)
    tables = []          # (row, radius, sensitive)

    def add(row, radii, sensitive=0.1):
        for r in radii:
            tables.append((row, r, sensitive))
    for dt in (np.float32, np.float64):
        for n in (1, 2, 3, 4, 5, 8):
            add(rng.integers(0, 6, n).astype(dt), (1, 5))
        for n in (255, 256, 257, 513):
            radii = (1, 5, 11, 63, 128)
            add(rng.integers(1, 10, n).astype(dt), radii)                                     # small integers: ties, every sum exact
            x = np.arange(n)
            add((2.0 + np.cos(x * 2 * np.pi / 37.3) + 0.05 * rng.standard_normal(n)).astype(dt), radii)
            add((2.0 + np.cos(x * 2 * np.pi / 37.3) + 0.05 * rng.standard_normal(n)).astype(dt), (5, 11), np.float64(0.3))   # promotes
        plateau = np.full(257, 4.0)
        plateau[20:27] = 1.0                                                                  # a flat minimum: every sample of it is a point
        plateau[100:102] = 2.0
        plateau[180] = 3.0
        plateau[181] = 3.0
        add(plateau.astype(dt), (1, 5, 11))
        withnan = (3.0 + np.sin(np.arange(256) / 5.0)).astype(dt)
        withnan[77] = np.nan
        add(withnan, (1, 5, 11, 63))
        zeros = np.zeros(255)
        zeros[40::30] = -1.0                                                                  # the largest elements are all 0: m == 0
        add(zeros.astype(dt), (1, 5, 11))
        exact = np.full(256, 2.0)
        exact[30::40] = 1.0                                                                   # |(1 - 2) / 2| = 0.5 exactly
        add(exact.astype(dt), (1, 5, 11), 0.5)
        add(exact.astype(dt), (5,), 0.25)
    return tables


def g27_images(with_g28=False):
    rng = np.random.default_rng(2728)

    def grid(shape, dist, deg, chess):
        h, w = shape
        y, x = np.mgrid[0:h, 0:w].astype(np.float64)
        t = np.deg2rad(deg)
        u, v = x * np.cos(t) + y * np.sin(t) + 7.3, -x * np.sin(t) + y * np.cos(t) + 11.9
        ramp = 0.75 + 0.2 * x / w + 0.1 * y / h
        if chess:
            img = ((np.floor(u / dist) + np.floor(v / dist)) % 2) * 0.8 + 0.1
            img = ndi.gaussian_filter(img, 1.0)
        else:
            du, dv = (u + dist / 2) % dist - dist / 2, (v + dist / 2) % dist - dist / 2
            img = 1.0 - 0.8 * np.maximum(np.exp(-du * du / (2 * 1.6 ** 2)), np.exp(-dv * dv / (2 * 1.6 ** 2)))
        return (img * ramp * (1.0 + 0.01 * rng.standard_normal(shape))).astype(np.float32)
    images = dict(line=grid((160, 200), 20, 1.5, False), chess=grid((160, 200), 24, 1.5, True), tall=grid((300, 96), 20, 1.5, False))
    if with_g28:             # (drawn after g27's three, which stay what they were)
        images["big"] = grid((400, 420), 30, 3.2, False)
    return images


def g27():
    import types
    import warnings
    for name in ("skimage", "skimage.filters", "skimage.segmentation", "skimage.morphology", "skimage.measure", "skimage.transform"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["skimage.filters"].threshold_otsu = None
    sys.modules["skimage.segmentation"].clear_border = None
    sys.modules["skimage.transform"].radon = None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        import discorpy.prep.linepattern as rlp
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from helpers import peaks_reference as pr
    out = {}
    e_sub, e_slope = 0.0, 0.0
    # -- peak tables
    tables = g27_tables()
    out["pk_radius"] = np.array([t[1] for t in tables], np.int64)
    out["pk_sensitive"] = f64([t[2] for t in tables])
    out["pk_promotes"] = np.array([isinstance(t[2], np.float64) for t in tables])
    for k, (row, radius, sensitive) in enumerate(tables):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ints = rlp.get_local_extrema_points(row, option="min", radius=radius, sensitive=sensitive, denoise=False, norm=False, subpixel=False)
            subs = rlp.get_local_extrema_points(row, option="min", radius=radius, sensitive=sensitive, denoise=False, norm=False, subpixel=True)
        ints = np.asarray(ints, np.int64)
        subs = f64(subs)
        assert len(ints) == len(subs)
        # a flat triple has no parabola: the polyfit's rounding noise decides there, the closed form says argmin (not compared)
        curved = np.array([not (row[i - 1] == row[i] == row[i + 1]) for i in ints], bool)
        if curved.any():
            e_sub = max(e_sub, float(np.abs(pr.refine(row, ints)[curved] - subs[curved]).max()))
        out["pk%d_row" % k], out["pk%d_int" % k], out["pk%d_sub" % k], out["pk%d_curved" % k] = row, ints, subs, curved
    out["pk_count"] = np.int64(len(tables))
    assert sum(len(out["pk%d_int" % k]) for k in range(len(tables))) > 300
    # -- rows through denoise and norm
    rng = np.random.default_rng(2729)
    dn = []
    for dt in (np.float32, np.float64):
        for n in (257, 513):
            x = np.arange(n)
            dn.append(((3.0 + 0.004 * x - 2.5 * np.exp(-(((x + 20) % 41.7) - 20) ** 2 / 18.0) + 0.05 * rng.standard_normal(n)).astype(dt), 11))   # narrow dips
    for k, (row, radius) in enumerate(dn):
        ints = np.asarray(rlp.get_local_extrema_points(row, radius=radius, subpixel=False), np.int64)
        subs = f64(rlp.get_local_extrema_points(row, radius=radius, subpixel=True))
        assert len(ints) > 4 and len(ints) == len(subs)
        out["dn%d_row" % k], out["dn%d_int" % k], out["dn%d_sub" % k] = row, ints, subs
    out["dn_count"], out["dn_radius"] = np.int64(len(dn)), np.int64(11)
    # -- slope rows
    sl = [(2.0 + np.cos(np.arange(257) / 6.0) + 0.05 * rng.standard_normal(257)), rng.integers(0, 9, 8).astype(np.float64)]
    for k, row in enumerate(sl):
        out["sl%d_row" % k] = row
        for size in (3, 5):
            raw = rlp.sliding_window_slope(row, size=size, norm=False)
            out["sl%d_s%d" % (k, size)] = raw
            out["sl%d_s%d_norm" % (k, size)] = rlp.sliding_window_slope(row, size=size, norm=True)
            e_slope = max(e_slope, float(np.abs(pr.window_slope(row, size) - raw).max() / np.abs(raw).max()))
    out["sl_count"] = np.int64(len(sl))
    # -- images
    images = g27_images()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        images["chess"] = rlp.convert_chessboard_to_linepattern(images["chess"].astype(np.float64)).astype(np.float32)
    for name, img in images.items():
        out["img_" + name] = img
    slope = float(np.tan(np.deg2rad(1.5)))
    flags = [("default", "line", {}), ("nonorm", "line", dict(norm=False)), ("nodenoise", "line", dict(denoise=False)),
             ("dark", "line", dict(bgr="dark")), ("offset", "line", dict(offset=9)), ("chess", "chess", dict(chessboard=True))]
    names, noise_rng = [], np.random.default_rng(2730)

    def profiles_of(mat, hor, kw):                                  # the reference's body up to the profiles, for the margin check
        bgr, norm, denoise, offset = kw.get("bgr", "bright"), kw.get("norm", True), kw.get("denoise", True), kw.get("offset", 0)
        (height, width) = mat.shape
        if bgr == "bright":
            mat = np.max(mat) - mat
        if norm is True:
            mat = rlp.prep.normalization_fft(mat, 5)
        if denoise is True:
            mat = ndi.gaussian_filter(mat, 3)
        angle = np.arctan(slope)
        if hor:
            lo, hi = rlp._calc_index_range(height, width, np.rad2deg(angle), direction="vertical")
            offset = int(np.clip(offset, 0, min(height, width) // 3))
            return [rlp.get_tilted_profile(mat, i, np.rad2deg(angle), direction="vertical")[2] for i in np.arange(lo + offset, hi - offset, 0.3 * dist)]
        lo, hi = rlp._calc_index_range(height, width, -np.rad2deg(angle), direction="horizontal")
        offset = int(np.clip(offset, 0, min(height, width) // 8))
        return [rlp.get_tilted_profile(mat, i, -np.rad2deg(angle), direction="horizontal")[2] for i in np.arange(lo + offset, hi - offset, 0.3 * dist)]
    for dt in ("float32", "float64"):
        for flag, key, kw in flags:
            dist = 24.0 if key == "chess" else 20.0
            mat = images[key].astype(dt)
            if flag == "dark":
                mat = mat.max() - mat
            for fn in ("hor", "ver"):
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    ref_fn = rlp.get_cross_points_hor_lines if fn == "hor" else rlp.get_cross_points_ver_lines
                    pts = ref_fn(mat, slope, dist, **kw)
                    name = "%s_%s_%s" % (flag, dt, fn)
                    assert pts.ndim == 2 and len(pts) >= 50, (name, pts.shape)
                    for prof in profiles_of(mat, fn == "hor", kw):
                        if kw.get("chessboard"):
                            prof = rlp.sliding_window_slope(prof, size=3)
                        args = dict(option="max", radius=11, sensitive=0.1, denoise=not kw.get("denoise", True), norm=not kw.get("norm", True),
                                    subpixel=False)
                        a = rlp.get_local_extrema_points(prof, **args)
                        b = rlp.get_local_extrema_points(prof * (1 + 1e-9 * noise_rng.standard_normal(len(prof))), **args)
                        assert np.array_equal(a, b), (name, a, b)
                        if len(a):                     # the sub-pixel closed form against the polyfit on the profile the reference searched
                            d = np.copy(prof)
                            if args["denoise"]:
                                d = ndi.gaussian_filter(d, 3)
                            d = np.max(d) - d
                            if not args["norm"]:
                                sub = rlp.get_local_extrema_points(prof, **dict(args, subpixel=True))
                                e_sub = max(e_sub, float(np.abs(pr.refine(d, np.asarray(a, np.int64)) - sub).max()))
                names.append(name)
                out["pts_" + name] = pts
    out["case_names"] = np.array(names)
    out["slope"], out["e_sub"], out["e_slope"] = np.float64(slope), np.float64(e_sub), np.float64(e_slope)
    assert e_sub < 1e-9 and e_slope < 1e-12, (e_sub, e_slope)
    print("g27: %d tables, %d image cases, e_sub %.3g, e_slope %.3g" % (len(tables), len(names), e_sub, e_slope))
    save("g27_cross_points", **out)
    assert os.path.getsize(os.path.join(OUT, "g27_cross_points.npz")) <= os.path.getsize(os.path.join(OUT, "g26_fourier_gauss.npz"))


# ---- g28: the slope and distance search of prep.linepattern (calc_slope_distance_hor_lines / calc_slope_distance_ver_lines): what the
# reference's own functions return with skimage stubbed as for g27 and skimage.transform.radon set to the NumPy restatement of its
# documented definition (tests/helpers/radon_reference.py) -- scikit-image itself is not installed, so that link is UNVERIFIED.  Per case:
# slope, distance, the relative gap between the two largest column maxima of the coarse and of the fine sinogram (no fixture may sit on a
# tie), and e_dist: how far the reference's distance lies from the same computation with the closed-form sub-pixel parabola.
def g28():
    import json
    import warnings
    import discorpy.prep.linepattern as rlp                         # (imported, with its stubs, by g27)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from helpers import peaks_reference as pr
    from helpers import radon_reference as rr
    sinograms = []

    def radon(image, theta=None, circle=True):
        sinograms.append(rr.radon(image, theta=theta, circle=circle))
        return sinograms[-1]
    images = g27_images(with_g28=True)
    line, big, chess = images["line"], images["big"], images["chess"]
    out = dict(img_line=line, img_big=big, img_chess=chess)
    small = dict(ratio=0.9, search_range=5, radius=5)
    # (name, image, what is done to it, directions, arguments)
    cases = [("line", "line", "", ("hor", "ver"), small),
             ("big", "big", "", ("ver",), dict(ratio=0.5, search_range=10, radius=5)),
             ("chess", "chess", "", ("hor", "ver"), dict(small, chessboard=True)),
             ("dark", "line", "invert", ("hor", "ver"), dict(small, bgr="dark")),
             ("float64", "line", "float64", ("hor", "ver"), small),
             ("plain", "line", "", ("hor", "ver"), dict(small, denoise=False, norm=False, subpixel=False))]
    names = []
    polyfit = rlp.locate_subpixel_point

    def closed_form(list_point, option="min"):
        return pr.subpixel_offset(*list_point)
    for name, key, prepare, directions, kw in cases:
        mat = out["img_" + key]
        if prepare == "invert":
            mat = mat.max() - mat
        if prepare == "float64":
            mat = mat.astype(np.float64)
        for direction in directions:
            fn = rlp.calc_slope_distance_hor_lines if direction == "hor" else rlp.calc_slope_distance_ver_lines
            del sinograms[:]
            rlp.radon = radon
            try:
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    slope, dist = fn(mat, **kw)
                    rlp.locate_subpixel_point = closed_form
                    slope_closed, dist_closed = fn(mat, **kw)
            finally:
                rlp.radon, rlp.locate_subpixel_point = None, polyfit
            assert slope_closed == slope and len(sinograms) == 4
            gaps = []
            for sino in sinograms[:2]:
                top = np.sort(np.amax(sino, axis=0))
                gaps.append((top[-1] - top[-2]) / top[-1])
            assert min(gaps) > 1e-9, (name, direction, gaps)
            e_dist = abs(dist - dist_closed)
            assert np.isfinite(dist) and e_dist < 1e-9 and (kw.get("subpixel", True) or e_dist == 0), (name, direction, dist, e_dist)
            full = "%s_%s" % (name, direction)
            names.append(full)
            out["image_" + full], out["prepare_" + full], out["args_" + full] = np.array(key), np.array(prepare), np.array(json.dumps(kw, sort_keys=True))
            out["slope_" + full], out["dist_" + full] = np.float64(slope), np.float64(dist)
            out["gap1_" + full], out["gap2_" + full], out["e_dist_" + full] = np.float64(gaps[0]), np.float64(gaps[1]), np.float64(e_dist)
            print("g28 %-12s slope %+.7f distance %.4f gaps %.3g %.3g e_dist %.3g" % (full, slope, dist, gaps[0], gaps[1], e_dist))
    out["case_names"] = np.array(names)
    # the generator's own lines: 1.5 degree (line, chess) and 3.2 degree (big), recovered to the 0.05 degree grid of the fine search
    assert abs(out["slope_line_hor"] - np.tan(np.deg2rad(1.5))) < 1e-3 and abs(out["slope_big_ver"] + np.tan(np.deg2rad(3.2))) < 1e-3
    save("g28_slope_distance", **out)
    assert os.path.getsize(os.path.join(OUT, "g28_slope_distance.npz")) <= 1 << 20


# ---- g29: the dot-grid route of prep.dotpattern (calc_size_distance, select_dots_based_ratio / _distance, calc_hor_slope / calc_ver_slope,
# the grouping and the residual filter): what the reference's own functions return with skimage stubbed as for g28 -- radon <- the padded
# restatement (tests/helpers/radon_padded_reference.py), clear_border <- binarize_reference.clear_border, regionprops <- the moments
# helper (tests/helpers/regionprops_reference.py); scikit-image itself is not installed, so those links are UNVERIFIED.  Per case: the
# relative gap between the two largest column maxima of each sinogram and the least |val - ratio| / ratio over the dots (no fixture may
# sit on a tie or on the threshold).
def g29_images():
    def grid(shape, pitch, radius, deg, k):
        h, w = shape
        img = np.zeros(shape, np.uint8)
        y, x = np.mgrid[0:h, 0:w].astype(np.float64)
        t = np.deg2rad(deg)
        n = max(h, w) // pitch + 2
        for i in range(-n, n + 1):
            for j in range(-n, n + 1):
                u, v = j * pitch * np.cos(t) - i * pitch * np.sin(t), j * pitch * np.sin(t) + i * pitch * np.cos(t)
                s = 1.0 + k * (u * u + v * v)                  # a mild radial term
                cy, cx = h / 2 + 0.3 + s * v, w / 2 - 0.4 + s * u
                if radius + 3 <= cy < h - radius - 3 and radius + 3 <= cx < w - radius - 3:
                    img[(y - cy) ** 2 + (x - cx) ** 2 <= radius * radius] = 1
        return img

    def spoil(img, pitch, radius, dropped):
        h, w = img.shape
        labels, num = ndi.label(img)
        cents = np.asarray(ndi.center_of_mass(img, labels, np.arange(1, num + 1)))
        boxes = ndi.find_objects(labels)
        mid = np.array([h / 2, w / 2])
        order = np.argsort(((cents - mid) ** 2).sum(1))
        y, x = np.mgrid[0:h, 0:w].astype(np.float64)

        def ellipse(cy, cx, a, b):
            return ((y - cy) / b) ** 2 + ((x - cx) / a) ** 2 <= 1.0
        marks = {}                                              # a pixel of each spoiled item
        # two merged dots: a dot and its neighbour to the right (away from the middle: the slope search starts at the dot nearest the mean)
        c0 = cents[order[24]]
        right = min((i for i in range(num) if cents[i][1] > c0[1] + pitch / 2), key=lambda i: ((cents[i] - c0) ** 2).sum())
        yy = int(round((c0[0] + cents[right][0]) / 2))
        img[yy - 1:yy + 2, int(c0[1]):int(cents[right][1]) + 1] = 1
        marks["merged"] = (yy, int(c0[1]))
        # an ellipse at axis ratio 1.25 (kept) and one at `dropped` (1.4; 1.6 at radius 4, where the pixels of 1.25 and 1.4 are the same)
        for pos, axis_ratio, mark in ((order[5], 1.25, "ellipse_kept"), (order[6], dropped, "ellipse_dropped")):
            img[boxes[pos]] = 0
            img[ellipse(cents[pos][0], cents[pos][1], radius * np.sqrt(axis_ratio), radius / np.sqrt(axis_ratio))] = 1
            marks[mark] = (int(round(cents[pos][0])), int(round(cents[pos][1])))
        # a dot whose box contains part of a neighbour: a 2 x 2 block with one pixel in the corner of the box
        pos = order[9]
        by, bx = boxes[pos][0].start, boxes[pos][1].start
        assert img[by, bx] == 0 and img[by + 1, bx] == 0 and img[by, bx + 1] == 0 and not img[by - 2:by + 1, bx - 2:bx + 1].any()
        img[by - 1:by + 1, bx - 1:bx + 1] = 1
        marks["neighbour"], marks["crowded_dot"] = (by, bx), (int(round(cents[pos][0])), int(round(cents[pos][1])))
        # between four dots: a 1-pixel-high bar, a 2 x 2 block, a diagonal pixel pair
        for pos, kind in ((order[30], "bar"), (order[40], "block"), (order[50], "pair")):
            gy, gx = int(cents[pos][0] + pitch / 2), int(cents[pos][1] + pitch / 2)
            assert not img[gy - 2:gy + 4, gx - 4:gx + 5].any(), kind
            marks[kind] = (gy, gx)
            if kind == "bar":
                img[gy, gx - 2:gx + 3] = 1
            elif kind == "block":
                img[gy:gy + 2, gx:gx + 2] = 1
            else:
                img[gy, gx] = img[gy + 1, gx + 1] = 1
        # a dot touching the border
        gx = int(cents[order[0]][1] + pitch / 2)
        img[ellipse(2.0, gx, radius, radius)] = 1
        marks["border"] = (0, gx)
        assert all(img[m] == 1 for m in marks.values())
        assert ndi.label(img)[1] == num - 1 + 1 + 1 + 1 + 2 + 1       # merged, neighbour, bar, block, pair (two labels), border dot
        return img, marks
    return dict(a=spoil(grid((200, 260), 20, 4, 2.0, 2e-7), 20, 4, 1.6), b=spoil(grid((360, 300), 24, 5, -1.5, 1e-7), 24, 5, 1.4))


def g29():
    import types
    import warnings
    for name in ("skimage", "skimage.filters", "skimage.segmentation", "skimage.morphology", "skimage.measure", "skimage.transform"):
        sys.modules.setdefault(name, types.ModuleType(name))
    for mod, attr in (("skimage.filters", "threshold_otsu"), ("skimage.segmentation", "clear_border"), ("skimage.transform", "radon")):
        if not hasattr(sys.modules[mod], attr):
            setattr(sys.modules[mod], attr, None)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        import discorpy.prep.preprocessing as rprep
    sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
    import binarize_reference as br
    import radon_padded_reference as rpr
    import regionprops_reference as rgp
    sinograms = []

    def radon(image, theta=None, circle=True):
        assert circle is False
        sinograms.append(rpr.radon(image, theta=theta))
        return sinograms[-1]
    saved = rprep.radon, rprep.clear_border, getattr(rprep.meas, "regionprops", None)
    rprep.radon, rprep.clear_border, rprep.meas.regionprops = radon, br.clear_border, rgp.regionprops
    select_ratio = 0.3
    out, names = {}, []

    def lines_out(key, lines):
        out[key + "_pts"] = f64(np.concatenate(lines))
        out[key + "_len"] = np.array([len(line) for line in lines], np.int64)
    try:
        for key, (img, marks) in g29_images().items():
            out["img_" + key] = img
            out["mark_names_" + key], out["marks_" + key] = np.array(sorted(marks)), np.array([marks[m] for m in sorted(marks)], np.int64)
            mat = np.int16(img)
            # the least |val - ratio| / ratio over the dots the reference measures (boxes of at least 2 x 2)
            labels, num = ndi.label(mat)
            margins, vals = [], []
            for box in ndi.find_objects(labels):
                sub = mat[box]
                if min(sub.shape) >= 2:
                    major, minor = rgp.axis_lengths(sub)
                    assert minor > 0
                    vals.append(abs(major / minor - 1.0))
                    margins.append(abs(vals[-1] - select_ratio) / select_ratio)
            assert min(margins) > 1e-6, (key, min(margins))
            kept_ratio = rprep.select_dots_based_ratio(mat, select_ratio)
            want = dict(merged=0, ellipse_kept=1, ellipse_dropped=0, neighbour=1, crowded_dot=1, bar=0, block=1, pair=0)
            assert all(kept_ratio[marks[m]] == v for m, v in want.items()), {m: int(kept_ratio[marks[m]]) for m in want}
            for roi in (0.9, 0.6):
                name = "%s_%d" % (key, round(roi * 100))
                del sinograms[:]
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    size, dist = rprep.calc_size_distance(mat, roi)
                    slope_hor = rprep.calc_hor_slope(mat, roi)
                    slope_ver = rprep.calc_ver_slope(mat, roi)
                assert len(sinograms) == 2
                gaps = []
                for sino in sinograms:
                    top = np.sort(np.amax(sino, axis=0))
                    gaps.append((top[-1] - top[-2]) / top[-1])
                assert min(gaps) > 1e-9, (name, gaps)
                kept_size = rprep.select_dots_based_size(mat, size)
                kept_dist = rprep.select_dots_based_distance(mat, dist)
                # the flow of the reference's example_01: size, ratio, then the lines
                mat1 = rprep.select_dots_based_ratio(kept_size, select_ratio)
                hor = rprep.group_dots_hor_lines(mat1, slope_hor, dist)
                ver = rprep.group_dots_ver_lines(mat1, slope_ver, dist)
                hor2 = rprep.remove_residual_dots_hor(hor, slope_hor)
                ver2 = rprep.remove_residual_dots_ver(ver, slope_ver)
                lab1, num1 = ndi.label(mat1)
                points = f64(ndi.center_of_mass(mat1, lab1, np.arange(1, num1 + 1)))
                for a, b in zip(hor + ver, rprep.group_dots_hor_lines(points, slope_hor, dist) + rprep.group_dots_ver_lines(points, slope_ver, dist)):
                    assert np.array_equal(a, b)          # (the point-list path: the same lines)
                names.append(name)
                out["roi_" + name], out["size_" + name], out["dist_" + name] = np.float64(roi), np.float64(size), np.float64(dist)
                out["slope_hor_" + name], out["slope_ver_" + name] = np.float64(slope_hor), np.float64(slope_ver)
                out["gap_hor_" + name], out["gap_ver_" + name] = np.float64(gaps[0]), np.float64(gaps[1])
                out["kept_size_" + name], out["kept_dist_" + name] = kept_size.astype(np.uint8), kept_dist.astype(np.uint8)
                out["flow_" + name], out["points_" + name] = mat1.astype(np.uint8), points
                lines_out("hor_" + name, hor)
                lines_out("ver_" + name, ver)
                lines_out("hor2_" + name, hor2)
                lines_out("ver2_" + name, ver2)
                print("g29 %-5s size %.1f dist %.4f slopes %+.6f %+.6f gaps %.3g %.3g lines %d / %d margin %.3g"
                      % (name, size, dist, slope_hor, slope_ver, gaps[0], gaps[1], len(hor), len(ver), min(margins)))
            out["kept_ratio_" + key] = kept_ratio.astype(np.uint8)
            out["margin_" + key], out["vals_" + key] = np.float64(min(margins)), f64(vals)
    finally:
        rprep.radon, rprep.clear_border, rprep.meas.regionprops = saved
    out["case_names"], out["select_ratio"] = np.array(names), np.float64(select_ratio)
    # the generator's own grids: 2.0 and -1.5 degree
    assert abs(out["slope_hor_a_90"] - np.tan(np.deg2rad(2.0))) < 2e-3 and abs(out["slope_ver_a_90"] + np.tan(np.deg2rad(2.0))) < 2e-3
    assert abs(out["slope_hor_b_90"] + np.tan(np.deg2rad(1.5))) < 2e-3
    save("g29_dot_grid", **out)
    assert os.path.getsize(os.path.join(OUT, "g29_dot_grid.npz")) <= 1 << 20


g27()
g28()
g29()
g30()
g31()
g32()
g33()
print("done")
