"""GPU suite for discorpy_amd.proc.processing: the one function of the module that needs a device (correct_perspective_effect, which ends
in post.correct_perspective_line: dcp_map_points_perspective_f64), the route from a calibration image to a calibration with every
stage from this package, and the smoke step.  Golden G30 (tools/gen_golden.py g30()) holds what the reference returned.

Bounds as in tests/test_proc_cpu.py: 1e-3 px on centres and points (a float32 coefficient may round one ulp the other way on another
CPU: 3e-5 px on an intercept of 500), 1e-9 on the radial model F(r) over 256 radii up to the largest radius of an input point."""
import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu

METHODS = ["mean", "median", "min", "max"]
SCALES = ["mean", "max", 0.9]


@pytest.fixture(scope="module")
def g30():
    return golden("g30_proc")


@pytest.fixture(scope="module")
def proc(hip):
    from discorpy_amd.proc import processing
    return processing


@pytest.fixture(scope="module")
def post(hip):
    from discorpy_amd.post import postprocessing
    return postprocessing


def tag(v):
    return v if isinstance(v, str) else "f%g" % v


def lines(g, key):
    return (np.split(g[key + "_hor_pts"], np.cumsum(g[key + "_hor_len"])[:-1]),
            np.split(g[key + "_ver_pts"], np.cumsum(g[key + "_ver_len"])[:-1]))


@pytest.mark.parametrize("scale", SCALES, ids=tag)
@pytest.mark.parametrize("method", METHODS)
def test_correct_perspective_effect_is_the_references(g30, proc, method, scale):
    hor, ver = lines(g30, "p")
    xc, yc = float(g30["p_coarse"][0]), float(g30["p_coarse"][1])
    got_hor, got_ver = proc.correct_perspective_effect(hor, ver, xc, yc, method, scale)
    for got, given, side in ((got_hor, hor, "hor"), (got_ver, ver, "ver")):
        want = g30["p_effect_%s_%s_%s" % (method, tag(scale), side)]
        assert isinstance(got, list) and [len(line) for line in got] == [len(line) for line in given]
        assert all(line.dtype == np.float64 and line.shape == (len(line), 2) for line in got)
        worst = np.abs(np.concatenate(got) - want).max()
        print("%s %s %s: max |difference| %.3g px" % (method, tag(scale), side, worst))
        assert worst <= 1e-3
    # the host route the vanishing-point iteration takes: the same bits as the device's
    shifted_hor, shifted_ver, coef = proc._perspective_effect_model(hor, ver, xc, yc, method, scale)
    for got, shifted in ((got_hor, shifted_hor), (got_ver, shifted_ver)):
        host = proc.update_center(proc._perspective_lines_host(shifted, coef), xc, yc)
        assert all(np.array_equal(a.view(np.uint64), b.view(np.uint64)) for a, b in zip(got, host))
    if method == "mean" and scale == "mean":
        defaults = proc.correct_perspective_effect(hor, ver, xc, yc)
        assert all(np.array_equal(a, b) for a, b in zip(defaults[0] + defaults[1], got_hor + got_ver))


def test_from_the_image_to_the_calibration(g30, proc, post, hip):
    """G29's image a through this package's GPU route as tests/test_dot_grid_gpu.py runs it, then proc, then post."""
    from discorpy_amd.prep import preprocessing as prep
    g29 = golden("g29_dot_grid")
    mat = np.int16(g29["img_a"])
    assert mat.shape == (200, 260)
    roi = float(g29["roi_a_90"])
    size, dist = prep.calc_size_distance(mat, roi)
    slope_hor, slope_ver = prep.calc_hor_slope(mat, roi), prep.calc_ver_slope(mat, roi)
    mat1 = prep.select_dots_based_ratio(prep.select_dots_based_size(mat, size), float(g29["select_ratio"]))
    hor = prep.remove_residual_dots_hor(prep.group_dots_hor_lines(mat1, slope_hor, dist), slope_hor)
    ver = prep.remove_residual_dots_ver(prep.group_dots_ver_lines(mat1, slope_ver, dist), slope_ver)
    assert [len(line) for line in hor] == g30["b_hor_len"].tolist() and [len(line) for line in ver] == g30["b_ver_len"].tolist()
    assert dist == float(g30["b_point_dist"])
    xcenter, ycenter = proc.find_cod_coarse(hor, ver)
    print("centre %r %r (golden %r)" % (xcenter, ycenter, g30["b_coarse"]))
    assert abs(xcenter - g30["b_coarse"][0]) <= 1e-3 and abs(ycenter - g30["b_coarse"][1]) <= 1e-3
    xcenter, ycenter = float(xcenter), float(ycenter)
    list_fact = proc.calc_coef_backward(hor, ver, xcenter, ycenter, 3)
    want = g30["backward_b_nf3_opt0"]
    pts = np.concatenate(hor + ver)
    radii = np.linspace(0.0, np.sqrt((pts[:, 1] - xcenter) ** 2 + (pts[:, 0] - ycenter) ** 2).max(), 256)
    powers = radii[:, None] ** np.arange(3)[None, :]
    worst = np.abs(powers @ list_fact - powers @ want).max()
    print("max |F - F_golden| %.3g" % worst)
    assert list_fact.shape == (3,) and worst <= 1e-9
    res_hor = post.calc_residual_hor(post.unwarp_line_backward(hor, xcenter, ycenter, list_fact), xcenter, ycenter)
    res_ver = post.calc_residual_ver(post.unwarp_line_backward(ver, xcenter, ycenter, list_fact), xcenter, ycenter)
    print("residuals: hor max %.3g, ver max %.3g px" % (res_hor[:, 1].max(), res_ver[:, 1].max()))
    # corrected lines are straight here exactly when they were straight for the reference
    assert post.check_distortion(res_hor) == bool(g30["b_check_hor"]) and post.check_distortion(res_ver) == bool(g30["b_check_ver"])
    assert not bool(g30["b_check_hor"]) and not bool(g30["b_check_ver"])


def test_smoke_step_of_the_calibration(hip):
    """The step smoke() gained, alone (the whole of smoke() takes ten seconds and runs with every check of a change anyway)."""
    import inspect
    import __graft_entry__
    assert "smoke_calibration()" in inspect.getsource(__graft_entry__.smoke)
    assert __graft_entry__.smoke_calibration() is None
