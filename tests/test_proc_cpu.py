"""CPU suite for discorpy_amd.proc.processing (host code: NumPy and SciPy, no device) against golden G30 (tools/gen_golden.py g30():
what the reference's own functions returned on three sets of grouped lines -- A its unit-test grid, B the lines grouped from G29's
image, C a noisy 13 x 18 grid, P the same grid under a mild homography).

Bounds, and where they come from:

* centres, grids, points, intercepts: 1e-3 px.  A fit computed on another CPU may round a float32 coefficient one ulp the other way:
  3e-5 px on an intercept of 500, less through the slopes; ``fsolve`` stops at 1.5e-8 relative, below a float32 ulp.  The float32
  tables are held to the same 1e-3 px, each coefficient weighted by the power of the largest abscissa it multiplies;
* radial coefficients: the model, not the coefficients -- ``F(r) = sum c_i r**i`` on 256 radii over [0, r_max] within 1e-9, the bound
  the change was specified with: rebuilding the design matrix with running products in place of ``np.power`` (an equally valid order)
  moved F by at most 1.2e-11 at ``num_fact`` 5 on the grids it was derived on (condition numbers up to 1.6e13), by nothing at 3.  On
  the golden's own cases the same rebuild moves F by up to 1.9e-10 at ``num_fact`` 5 ("Calibration (proc)", case
  by case): 1e-9 leaves a factor of five there, not a hundred;
* perspective coefficients: by effect -- the points they are applied to, mapped with both sets: 100 times what writing the rows of the
  design matrix in another order moves them (measured on the golden's cases, figures at the two constants below), at least 1e-9 px;
* find_cod_fine: only the cases whose choice is stable in the reference itself (the recorded gap between the best and the second-best
  candidate is at least 10 times what the exact minimiser moves the metric, both passes): the chosen index pairs equal the golden's,
  the metric matrices within a tenth of the recorded gap."""
import inspect
import warnings

import numpy as np
import pytest

from conftest import golden

RADIAL_BOUND = 1e-9
PIXEL_BOUND = 1e-3
# Writing the rows of the design matrix in another order (all x-equations, then all y-equations: the same least-squares problem) moved
# the mapped points of the golden's own cases by at most 1.15e-9 px (the 234 point pairs of the grid, every scale, both mappings) and
# 1.82e-9 px (four points, every option, both mappings).  The bounds are 100 times those, above the floor of 1e-9 px.
GRID_PAIRS_BOUND = 1.15e-7
FOUR_POINTS_BOUND = 1.82e-7

CASES = ["a", "b", "c", "p"]
SCALES = ["mean", "median", "min", "max", 0.9]
METHODS = ["mean", "median", "min", "max"]


@pytest.fixture(scope="module")
def g30():
    g = golden("g30_proc")
    for v in g.values():
        v.setflags(write=False)
    return g


@pytest.fixture(scope="module")
def proc():
    from discorpy_amd.proc import processing
    return processing


def tag(v):
    return v if isinstance(v, str) else "f%g" % v


def lines(g, key):
    return (np.split(g[key + "_hor_pts"], np.cumsum(g[key + "_hor_len"])[:-1]),
            np.split(g[key + "_ver_pts"], np.cumsum(g[key + "_ver_len"])[:-1]))


def center(g, key):
    return float(g[key + "_coarse"][0]), float(g[key + "_coarse"][1])


def close(got, want, bound=PIXEL_BOUND, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    worst = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max()) if got.size else 0.0
    print("%s: max |difference| %.3g (bound %.3g)" % (what, worst, bound))
    assert worst <= bound, (what, worst)


def same_kind(got, want, what=""):
    assert isinstance(got, np.ndarray) and got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape)


def model_close(g, key, got, want, what):
    """F(r) of two coefficient sets on 256 radii over [0, the largest radius of an input point]."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and got.dtype == np.float64
    xc, yc = center(g, key)
    pts = np.concatenate([g[key + "_hor_pts"], g[key + "_ver_pts"]])
    radii = np.linspace(0.0, np.sqrt((pts[:, 1] - xc) ** 2 + (pts[:, 0] - yc) ** 2).max(), 256)
    powers = radii[:, None] ** np.arange(len(want))[None, :]
    worst = float(np.abs(powers @ got - powers @ want).max())
    print("%s: max |F - F_golden| %.3g" % (what, worst))
    assert worst <= RADIAL_BOUND, (what, worst)


def map_points(points_yx, c):
    """The eight-coefficient homography on (y, x) points, in (x, y) convention as post.correct_perspective_line reads it."""
    y, x = points_yx[:, 0].astype(np.float64), points_yx[:, 1].astype(np.float64)
    den = c[6] * x + c[7] * y + 1.0
    return np.stack([(c[3] * x + c[4] * y + c[5]) / den, (c[0] * x + c[1] * y + c[2]) / den], axis=1)


# --------------------------------------------------------------------------- names and refusals

def test_every_public_name_with_the_references_signature(g30, proc):
    assert len(g30["public_names"]) == 17 and sorted(proc.__all__) == sorted(g30["public_names"])
    for name, want in zip(g30["public_names"], g30["signatures"]):
        assert str(inspect.signature(getattr(proc, str(name)))) == str(want), name
    from discorpy_amd.util import utility
    assert proc.transform_coef_backward_and_forward is utility.transform_coef_backward_and_forward          # not a second copy
    for helper in ("_para_fit_hor", "_para_fit_ver", "_calc_error", "_calc_metric", "_check_missing_lines", "_calc_undistor_intercept",
                   "_generate_linear_coef", "_generate_non_perspective_parabola_coef", "_find_cross_point_between_lines",
                   "_find_cross_point_between_parabolas", "_find_cross_point_between_parabolas_same_direction",
                   "_calc_undistor_intercept_perspective"):
        assert callable(getattr(proc, helper)), helper
    import discorpy_amd.proc
    assert discorpy_amd.proc.processing is proc


def test_refusals_are_the_references(g30, proc):
    four = g30["four_points"]
    calls = {"four_three_points": lambda: proc.generate_4_source_target_perspective_points(four[:3]),
             "four_five_points": lambda: proc.generate_4_source_target_perspective_points(np.concatenate([four, four[:1]])),
             "four_flat_xy": lambda: proc.generate_4_source_target_perspective_points(four.ravel(), "xy"),
             "coef_flat_points": lambda: proc.calc_perspective_coefficients(four.ravel(), four.ravel()),
             "coef_no_points": lambda: proc.calc_perspective_coefficients(np.zeros((0, 2)), np.zeros((0, 2))),
             "coef_unequal_counts": lambda: proc.calc_perspective_coefficients(four, four[:3])}
    assert sorted(calls) == sorted(str(n) for n in g30["refusal_names"])
    for name, kind, message in zip(g30["refusal_names"], g30["refusal_types"], g30["refusal_messages"]):
        with pytest.raises(Exception) as caught:
            calls[str(name)]()
        assert type(caught.value).__name__ == str(kind) and str(caught.value) == str(message), name
    assert "Input must be a list of 4 points!!!" in [str(m) for m in g30["refusal_messages"]]


def test_perspective_effect_names_the_missing_group(g30, proc):
    """Lines that all curve one way: the reference's messages (which the reference itself never reaches: module docstring)."""
    t = np.linspace(-100.0, 100.0, 9)
    up = [np.stack([c + 1e-3 * t * t, t], axis=1) for c in (-50.0, 0.0, 50.0)]
    right = [np.stack([t, c + 1e-3 * t * t], axis=1) for c in (-50.0, 0.0, 50.0)]
    down = [np.stack([c - 1e-3 * t * t, t], axis=1) for c in (-50.0, 0.0, 50.0)]
    for hor, ver, word in ((up, right, "downwards"), (down, right, "upwards"), (up[:1] + down[:1], right, "leftwards")):
        with pytest.raises(ValueError, match="Input error!!! No curved line open %s !!!" % word):
            proc._perspective_effect_model(hor, ver, 0.0, 0.0, "mean", "mean")
    with pytest.raises(ValueError, match="Need at least 2 horizontal lines!!!"):
        proc._perspective_effect_model(up[:1], right, 0.0, 0.0, "mean", "mean")
    with pytest.raises(ValueError, match="Need at least 2 vertical lines!!!"):
        proc._perspective_effect_model(up, right[:1], 0.0, 0.0, "mean", "mean")


# --------------------------------------------------------------------------- centres

@pytest.mark.parametrize("key", CASES)
def test_coarse_and_bailey_centres(g30, proc, key):
    hor, ver = lines(g30, key)
    close(proc.find_cod_coarse(hor, ver), g30[key + "_coarse"], what=key + " coarse")
    for it in (1, 2):
        close(proc.find_cod_bailey(hor, ver, iteration=it), g30["%s_bailey_it%d" % (key, it)], what="%s bailey %d" % (key, it))
    close(proc.find_cod_bailey(hor, ver), g30[key + "_bailey_it2"], what=key + " bailey default")


def test_case_a_centres_within_the_references_unit_test_bounds(g30, proc):
    hor, ver = lines(g30, "a")
    xcenter, ycenter = proc.find_cod_coarse(hor, ver)
    assert abs(xcenter - 33.0) < float(g30["a_point_dist"]) and abs(ycenter - 35.0) < float(g30["a_point_dist"])
    xcenter, ycenter = proc.find_cod_bailey(hor, ver)
    assert abs(xcenter - 33.0) < 1.0 and abs(ycenter - 35.0) < 1.0


@pytest.mark.parametrize("key", ["a", "c", "p"])
def test_vanishing_point_centre(g30, proc, key):
    hor, ver = lines(g30, key)
    close(proc.find_center_based_vanishing_points(hor, ver), g30[key + "_vanishing"], what=key + " vanishing points")


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("key", ["c", "p"])
def test_vanishing_point_iteration_centre(g30, proc, key, method):
    hor, ver = lines(g30, key)
    for it in (1, 2):
        want = g30["%s_vanishing_it%d_%s" % (key, it, method)]
        close(proc.find_center_based_vanishing_points_iteration(hor, ver, it, method), want, what="%s iteration %d %s" % (key, it, method))
    if method == "mean":
        close(proc.find_center_based_vanishing_points_iteration(hor, ver), g30[key + "_vanishing_it2_mean"], what=key + " defaults")


@pytest.mark.parametrize("key", ["a", "c"])
def test_find_cod_fine_on_the_stable_cases(g30, proc, key, monkeypatch):
    assert key in [str(k) for k in g30["fine_cases"]]
    # each matrix costs thousands of BFGS runs: computed once per pass, and handed again to _calc_metric and find_cod_fine when they ask
    # for the same lines, centre and candidates
    compute, known = proc._metric_matrix, {}

    def remembered(hor, ver, xcenter, ycenter, list_xshift, list_yshift):
        ident = (id(hor), id(ver), float(xcenter), float(ycenter), list_xshift.tobytes(), list_yshift.tobytes())
        if ident not in known:
            known[ident] = compute(hor, ver, xcenter, ycenter, list_xshift, list_yshift)
        return known[ident]
    monkeypatch.setattr(proc, "_metric_matrix", remembered)
    ratios = g30["fine_%s_ratios" % key]
    assert ratios.min() >= 10.0                                  # the condition that makes the comparison meaningful
    hor, ver = lines(g30, key)
    xc, yc = (float(v) for v in g30["fine_%s_start" % key])
    point_dist = float(g30["fine_%s_point_dist" % key])
    cx, cy = xc, yc
    for name, shifts in (("pass1", np.arange(-point_dist, point_dist + 2.0, 2.0)), ("pass2", np.arange(-2.0, 2.5, 0.5))):
        want = g30["fine_%s_metric_%s" % (key, name)]
        got = proc._metric_matrix(hor, ver, cx, cy, shifts, shifts)
        same_kind(got, want, name)
        close(got, want, bound=0.1 * float(g30["fine_%s_gap_%s" % (key, name)]), what="%s metric %s" % (key, name))
        row, col = np.unravel_index(got.argmin(), got.shape)
        assert (row, col) == tuple(g30["fine_%s_index_%s" % (key, name)]), name
        assert proc._calc_metric(hor, ver, cx, cy, shifts, shifts) == (shifts[col], shifts[row])
        cx, cy = cx + shifts[col], cy + shifts[row]
    xcenter, ycenter = proc.find_cod_fine(hor, ver, xc, yc, point_dist)
    assert isinstance(xcenter, float) and isinstance(ycenter, float)
    close([xcenter, ycenter], g30["fine_%s_center" % key], what=key + " fine centre")
    close([xcenter, ycenter], [cx, cy], bound=0.0, what=key + " the two passes")
    assert len(known) == 2                                       # find_cod_fine asked for the same two sets of candidates


def test_fine_search_takes_the_numpy_float32_centre_of_the_coarse_search(g30, proc):
    hor, ver = lines(g30, "a")
    xc, yc = proc.find_cod_coarse(hor, ver)
    xcenter, ycenter = proc.find_cod_fine(hor, ver, xc, yc, 2.0)
    assert isinstance(xcenter, float) and isinstance(ycenter, float)
    close([xcenter, ycenter], g30["fine_a_center"], what="fine centre from the coarse one")


# --------------------------------------------------------------------------- tables and intercepts

@pytest.mark.parametrize("key", CASES)
def test_float32_tables(g30, proc, key):
    hor, ver = lines(g30, key)
    xc, yc = center(g30, key)
    reach = max(np.abs(g30[key + "_hor_pts"]).max(), np.abs(g30[key + "_ver_pts"]).max())
    for name, fit, arg in (("para_hor", proc._para_fit_hor, hor), ("para_ver", proc._para_fit_ver, ver)):
        table, shifted = fit(arg, xc, yc)
        want = g30["%s_%s" % (key, name)]
        same_kind(table, want, name)
        close(table * reach ** np.array([2, 1, 0]), want * reach ** np.array([2, 1, 0]), what="%s %s" % (key, name))
        assert all(s.dtype == np.float64 and s.shape == a.shape for s, a in zip(shifted, arg))
        assert all(np.array_equal(s, np.stack([a[:, 0] - yc, a[:, 1] - xc], axis=1)) for s, a in zip(shifted, arg))
    for suffix, args in (("", ()), ("_center", (xc, yc))):
        got = proc._generate_linear_coef(hor, ver, *args)
        for table, name in zip(got, ("linear_hor", "linear_ver")):
            want = g30["%s_%s%s" % (key, name, suffix)]
            same_kind(table, want, name)
            close(table * reach ** np.array([1, 0]), want * reach ** np.array([1, 0]), what="%s %s%s" % (key, name, suffix))


@pytest.mark.parametrize("optimizing", [False, True])
@pytest.mark.parametrize("key", CASES)
def test_undistorted_intercepts(g30, proc, key, optimizing):
    hor, ver = lines(g30, key)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        got = proc._calc_undistor_intercept(hor, ver, *center(g30, key), optimizing=optimizing)
    for uc, name in zip(got, ("hor", "ver")):
        want = g30["%s_uc_%s_opt%d" % (key, name, optimizing)]
        same_kind(uc, want, name)
        close(uc, want, what="%s intercepts %s" % (key, name))


# --------------------------------------------------------------------------- radial coefficients

@pytest.mark.parametrize("optimizing", [False, True])
@pytest.mark.parametrize("num_fact", [3, 5])
@pytest.mark.parametrize("key", CASES)
def test_radial_models(g30, proc, key, num_fact, optimizing):
    hor, ver = lines(g30, key)
    xc, yc = center(g30, key)
    name = "%s_nf%d_opt%d" % (key, num_fact, optimizing)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        back = proc.calc_coef_backward(hor, ver, xc, yc, num_fact, optimizing=optimizing)
        warned = any(issubclass(w.category, UserWarning) for w in caught)
        fwd = proc.calc_coef_forward(hor, ver, xc, yc, num_fact, optimizing=optimizing)
        bff = proc.calc_coef_backward_from_forward(hor, ver, xc, yc, num_fact, optimizing=optimizing)
    assert warned == bool(g30["%s_warned_opt%d" % (key, optimizing)])
    model_close(g30, key, back, g30["backward_" + name], "backward " + name)
    model_close(g30, key, fwd, g30["forward_" + name], "forward " + name)
    model_close(g30, key, bff[0], g30["bff_f_" + name], "forward of backward-from-forward " + name)
    model_close(g30, key, bff[1], g30["bff_b_" + name], "backward-from-forward " + name)


@pytest.mark.parametrize("num_fact", [3, 5])
@pytest.mark.parametrize("key", CASES)
def test_reversed_models(g30, proc, key, num_fact):
    back = g30["backward_%s_nf%d_opt0" % (key, num_fact)]
    hor, ver = lines(g30, key)
    xc, yc = center(g30, key)
    own = np.concatenate(proc._para_fit_hor(hor, xc, yc)[1] + proc._para_fit_ver(ver, xc, yc)[1])
    for mapping in ("backward", "forward"):
        model_close(g30, key, proc.transform_coef_backward_and_forward(back, mapping=mapping),
                    g30["transform_%s_nf%d_default_%s" % (key, num_fact, mapping)], "%s reversed, default grid, %s" % (key, mapping))
        model_close(g30, key, proc.transform_coef_backward_and_forward(back, mapping, own),
                    g30["transform_%s_nf%d_points_%s" % (key, num_fact, mapping)], "%s reversed, own points, %s" % (key, mapping))


def test_case_a_coefficients_within_the_references_unit_test_bounds(g30, proc):
    hor, ver = lines(g30, "a")
    xc, yc = proc.find_cod_coarse(hor, ver)
    truth = [1.0, -2.0e-3]

    def errors(fact, sign=1.0):
        return abs((fact[0] - truth[0]) / truth[0]), abs((fact[1] - sign * truth[1]) / truth[1])
    e1, e2 = errors(proc.calc_coef_backward(hor, ver, xc, yc, 2))
    assert e1 < 0.1 and e2 < 0.1
    e1, e2 = errors(proc.calc_coef_backward(hor, ver, xc, yc, 2, optimizing=True))
    assert e1 < 0.1 and e2 < 0.15
    e1, e2 = errors(proc.calc_coef_forward(hor, ver, xc, yc, 2), -1.0)
    assert e1 < 0.1 and e2 < 0.2
    ffact, bfact = proc.calc_coef_backward_from_forward(hor, ver, xc, yc, 2)
    assert max(errors(ffact, -1.0)[0], errors(bfact)[0]) < 0.1 and max(errors(ffact, -1.0)[1], errors(bfact)[1]) < 0.2


def test_num_fact_is_clamped_to_one(g30, proc):
    hor, ver = lines(g30, "a")
    xc, yc = center(g30, "a")
    for num_fact in (0, -3):
        got = proc.calc_coef_backward(hor, ver, xc, yc, num_fact)
        assert got.shape == (1,) and np.array_equal(got, proc.calc_coef_backward(hor, ver, xc, yc, 1))
        assert proc.calc_coef_forward(hor, ver, xc, yc, num_fact).shape == (1,)
        assert [len(f) for f in proc.calc_coef_backward_from_forward(hor, ver, xc, yc, num_fact)] == [1, 1]


def test_missing_line_warning_fires_only_when_a_line_is_missing(g30, proc):
    hor, ver = lines(g30, "c")
    xc, yc = center(g30, "c")
    assert bool(g30["c_warned_line6_deleted"]) and not bool(g30["c_warned_opt0"])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        proc.calc_coef_backward(hor, ver, xc, yc, 3)
        proc.calc_coef_forward(hor, ver, xc, yc, 3)
    message = "\n!!! Check if there is any missing grouped line !!!\nParameters of the methods of grouping points may need to be adjusted!"
    for call in (proc.calc_coef_backward, proc.calc_coef_forward, proc.calc_coef_backward_from_forward):
        with pytest.warns(UserWarning) as caught:
            call(hor[:6] + hor[7:], ver, xc, yc, 3)
        assert str(caught[0].message) == message
    with pytest.warns(UserWarning):
        proc.calc_coef_backward(hor, ver[:9] + ver[10:], xc, yc, 3)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        proc.calc_coef_backward(hor[:6] + hor[7:], ver, xc, yc, 3, threshold=5.0)


# --------------------------------------------------------------------------- grids and points

@pytest.mark.parametrize("key", CASES)
def test_regenerated_grids(g30, proc, key):
    hor, ver = lines(g30, key)
    got = proc.regenerate_grid_points_linear(hor, ver)
    from_tables = proc.regenerate_grid_points_linear(g30[key + "_linear_hor"], g30[key + "_linear_ver"], is_coef=True)
    for a, b, name in zip(got, from_tables, ("hor", "ver")):
        want = g30["%s_grid_linear_%s" % (key, name)]
        same_kind(a, want, name)
        close(a, want, what="%s linear grid %s" % (key, name))
        assert np.array_equal(b, want)                         # from the golden's own tables: the same float32 arithmetic
    assert got[0].shape == (len(hor), len(ver), 2) and np.array_equal(got[1], got[0].transpose(1, 0, 2))
    for pers, find in ((False, False), (False, True), (True, False)):
        name = "%s_grid_parabola_p%d_c%d" % (key, pers, find)
        got = proc.regenerate_grid_points_parabola(hor, ver, perspective=pers, find_center=find)
        for a, side in zip(got, ("hor", "ver")):
            same_kind(a, g30["%s_%s" % (name, side)], name)
            close(a, g30["%s_%s" % (name, side)], what="%s %s" % (name, side))
    defaults = proc.regenerate_grid_points_parabola(hor, ver)
    close(defaults[0], g30[key + "_grid_parabola_p0_c0_hor"], what=key + " parabola grid, defaults")


def test_list_coefficients_go_through_python_arithmetic(proc):
    hor, ver = [[0.01, 5.0], [-0.02, 40.0]], [[0.03, 7.0], [0.0, 30.0], [-0.01, 60.0]]
    got_hor, got_ver = proc.regenerate_grid_points_linear(hor, ver, is_coef=True)
    assert got_hor.shape == (2, 3, 2) and got_ver.shape == (3, 2, 2) and got_hor.dtype == np.float32
    for i, (a1, b1) in enumerate(hor):
        for j, (a2, b2) in enumerate(ver):
            y = (a1 * b2 + b1) / (1.0 - a1 * a2)
            assert np.array_equal(got_hor[i, j], np.float32([y, a2 * y + b2])) and np.array_equal(got_ver[j, i], got_hor[i, j])
            x, y2 = proc._find_cross_point_between_lines(hor[i], ver[j])
            assert (x, y2) == (a2 * y + b2, y)


@pytest.mark.parametrize("scale", SCALES, ids=tag)
def test_undistorted_perspective_lines_and_point_pairs(g30, proc, scale):
    hor, ver = lines(g30, "p")
    for opt in (False, True):
        got = proc.generate_undistorted_perspective_lines(hor, ver, True, scale, opt)
        inter = proc._calc_undistor_intercept_perspective(hor, ver, True, scale, opt)
        for a, u, side in zip(got, inter, ("hor", "ver")):
            want = g30["p_undistorted_%s_opt%d_%s" % (tag(scale), opt, side)]
            same_kind(a, want, side)
            close(a, want, what="undistorted %s opt %d %s" % (tag(scale), opt, side))
            same_kind(u, g30["p_uintercept_%s_opt%d_%s" % (tag(scale), opt, side)], side)
            close(u, g30["p_uintercept_%s_opt%d_%s" % (tag(scale), opt, side)], what="intercepts %s opt %d %s" % (tag(scale), opt, side))
    got = proc.generate_undistorted_perspective_lines(hor, ver, False, scale, True)
    for a, side in zip(got, ("hor", "ver")):
        close(a, g30["p_undistorted_%s_unequal_%s" % (tag(scale), side)], what="undistorted %s unequal %s" % (tag(scale), side))
    src, tgt = proc.generate_source_target_perspective_points(hor, ver, True, scale, True)
    same_kind(src, g30["p_source_" + tag(scale)], "source")
    same_kind(tgt, g30["p_target_" + tag(scale)], "target")
    close(src, g30["p_source_" + tag(scale)], what="source points " + tag(scale))
    close(tgt, g30["p_target_" + tag(scale)], what="target points " + tag(scale))
    if scale == "mean":
        defaults = proc.generate_source_target_perspective_points(hor, ver)
        assert np.array_equal(defaults[0], src) and np.array_equal(defaults[1], tgt)
        assert np.array_equal(proc.generate_undistorted_perspective_lines(hor, ver)[0], g30["p_undistorted_mean_opt1_hor"])


@pytest.mark.parametrize("scale", ["mean", "min", "max", 0.9], ids=tag)
@pytest.mark.parametrize("equal_dist", [False, True])
@pytest.mark.parametrize("order", ["yx", "xy"])
def test_four_source_target_points(g30, proc, order, equal_dist, scale):
    four = g30["four_points"]
    given = four if order == "yx" else np.fliplr(four)
    name = "four_%s_eq%d_%s" % (order, equal_dist, tag(scale))
    src, tgt = proc.generate_4_source_target_perspective_points(given, order, equal_dist, scale)
    same_kind(src, g30[name + "_source"], "source")
    same_kind(tgt, g30[name + "_target"], "target")
    close(src, g30[name + "_source"], what=name + " source")
    close(tgt, g30[name + "_target"], what=name + " target")
    assert np.array_equal(src, np.float32(four)[[2, 0, 1, 3]])          # top-left, top-right, bottom-left, bottom-right
    if order == "yx" and not equal_dist and scale == "mean":
        defaults = proc.generate_4_source_target_perspective_points(given.tolist())
        assert np.array_equal(defaults[0], src) and np.array_equal(defaults[1], tgt)


def perspective_close(got, want, points, bound, what):
    assert got.shape == (8,) and got.dtype == np.float64
    worst = float(np.sqrt(((map_points(points, got) - map_points(points, want)) ** 2).sum(axis=1)).max())
    print("%s: mapped points move by at most %.3g px (bound %.3g)" % (what, worst, bound))
    assert worst <= bound, (what, worst)


@pytest.mark.parametrize("mapping", ["backward", "forward"])
def test_perspective_coefficients_by_their_effect(g30, proc, mapping):
    for scale in SCALES:
        src, tgt = g30["p_source_" + tag(scale)], g30["p_target_" + tag(scale)]
        got = proc.calc_perspective_coefficients(src, tgt, mapping)
        points = src if mapping == "forward" else tgt              # the points the coefficients are applied to
        perspective_close(got, g30["p_perspective_coef_%s_%s" % (tag(scale), mapping)], points, GRID_PAIRS_BOUND,
                          "grid %s %s" % (tag(scale), mapping))
    for equal in (False, True):
        for scale in ("mean", "min", "max", 0.9):
            name = "four_yx_eq%d_%s" % (equal, tag(scale))
            src, tgt = g30[name + "_source"], g30[name + "_target"]
            got = proc.calc_perspective_coefficients(src, tgt, mapping)
            points = src if mapping == "forward" else tgt
            perspective_close(got, g30["%s_coef_%s" % (name, mapping)], points, FOUR_POINTS_BOUND, "%s %s" % (name, mapping))
            # four pairs determine the eight coefficients: they take each point to its partner
            assert np.abs(map_points(points, got) - (tgt if mapping == "forward" else src)).max() < 1e-6
    src, tgt = g30["p_source_mean"], g30["p_target_mean"]
    assert np.array_equal(proc.calc_perspective_coefficients(src, tgt), proc.calc_perspective_coefficients(src, tgt, "backward"))
    assert np.array_equal(proc.calc_perspective_coefficients(src.tolist(), tgt.tolist(), "forward"),
                          proc.calc_perspective_coefficients(src.astype(np.float64), tgt.astype(np.float64), "forward"))


@pytest.mark.parametrize("key", CASES)
def test_update_center(g30, proc, key):
    hor, ver = lines(g30, key)
    xc, yc = center(g30, key)
    shifted = proc._para_fit_hor(hor, xc, yc)[1]
    moved = proc.update_center(shifted, xc, yc)
    assert isinstance(moved, list) and [m.shape for m in moved] == [h.shape for h in hor] and all(m.dtype == np.float64 for m in moved)
    close(np.concatenate(moved), g30[key + "_update_center"], what=key + " update_center")
    assert all(np.array_equal(m, np.stack([s[:, 0] + yc, s[:, 1] + xc], axis=1)) for m, s in zip(moved, shifted))
    assert proc.update_center([[[1, 2], [3, 4]]], 0.5, 0.25)[0].tolist() == [[1.25, 2.5], [3.25, 4.5]]


@pytest.mark.parametrize("method", METHODS)
def test_perspective_effect_on_the_host_route_of_the_iteration(g30, proc, method):
    """The model of correct_perspective_effect with the homography applied in NumPy (what the vanishing-point iteration does, without a
    device): the lines the reference returned.  tests/test_proc_gpu.py holds the public function, through the device, to the same."""
    hor, ver = lines(g30, "p")
    xc, yc = center(g30, "p")
    for scale in ("mean", "max", 0.9):
        shifted_hor, shifted_ver, coef = proc._perspective_effect_model(hor, ver, xc, yc, method, scale)
        got_hor = proc.update_center(proc._perspective_lines_host(shifted_hor, coef), xc, yc)
        got_ver = proc.update_center(proc._perspective_lines_host(shifted_ver, coef), xc, yc)
        assert [len(line) for line in got_hor] == [len(line) for line in hor] and [len(line) for line in got_ver] == [len(line) for line in ver]
        close(np.concatenate(got_hor), g30["p_effect_%s_%s_hor" % (method, tag(scale))], what="effect %s %s hor" % (method, tag(scale)))
        close(np.concatenate(got_ver), g30["p_effect_%s_%s_ver" % (method, tag(scale))], what="effect %s %s ver" % (method, tag(scale)))


def test_cross_points_of_parabolas(proc):
    x, y = proc._find_cross_point_between_parabolas(np.float32([1e-4, 0.02, 30.0]), np.float32([-2e-4, 0.01, 50.0]))
    assert abs(1e-4 * x * x + 0.02 * x + 30.0 - y) < 1e-4 and abs(-2e-4 * y * y + 0.01 * y + 50.0 - x) < 1e-4
    roots = proc._find_cross_point_between_parabolas_same_direction([1e-3, 0.0, -10.0], [-1e-3, 0.0, 10.0])
    assert sorted(np.round(roots, 9)) == [-100.0, 100.0]
    assert proc._find_cross_point_between_parabolas_same_direction([1e-3, 0.0, 10.0], [-1e-3, 0.0, -10.0]) is None
