"""GPU suite for the slope and distance search of discorpy_amd.prep.linepattern (calc_slope_distance_hor_lines /
calc_slope_distance_ver_lines on top of radon, gaussian_filter and get_local_extrema_points) against the reference's own results, golden
G28 (tools/gen_golden.py: the reference's functions with skimage.transform.radon set to tests/helpers/radon_reference.py).

For every case of the fixture, NumPy and tensor input: the slope equals the reference's (the same arithmetic, the same angle grid, the
same argmax; the fixture asserts that no case sits on a tie); the distance equals it with ``subpixel=False`` and lies within 4 e_dist of
it otherwise (e_dist: the fixture's own distance between the reference's polyfit and the closed-form parabola, per case), and in any
case within 1e-6 pixel.  Every case prints its figures before it asserts."""
import functools
import json

import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu

CAP = 1e-6                   # pixel: a condition, the one tests/test_cross_points_gpu.py uses
CASES = [str(n) for n in golden("g28_slope_distance")["case_names"]]


@functools.lru_cache(maxsize=None)
def G():
    g = golden("g28_slope_distance")
    for v in g.values():
        v.setflags(write=False)
    return g


@pytest.fixture(scope="module")
def lp(hip):
    from discorpy_amd.prep import linepattern
    return linepattern


def case(name):
    g = G()
    mat = g["img_" + str(g["image_" + name])]
    prepare = str(g["prepare_" + name])
    if prepare == "invert":
        mat = mat.max() - mat
    if prepare == "float64":
        mat = mat.astype(np.float64)
    return mat, json.loads(str(g["args_" + name]))


@pytest.mark.parametrize("kind", ["numpy", "torch"])
@pytest.mark.parametrize("name", CASES)
def test_slope_and_distance_are_the_references(lp, name, kind):
    g = G()
    mat, kw = case(name)
    fn = lp.calc_slope_distance_hor_lines if name.endswith("_hor") else lp.calc_slope_distance_ver_lines
    if kind == "torch":
        import torch
        mat = torch.from_numpy(np.array(mat)).to("cuda:0")
    slope, dist = fn(mat, **kw)
    want_slope, want_dist, e_dist = float(g["slope_" + name]), float(g["dist_" + name]), float(g["e_dist_" + name])
    print("%-12s %-5s slope %+.9f (reference %+.9f)  distance %.12f (reference %.12f): off by %.3g, e_dist %.3g" % (
        name, kind, slope, want_slope, dist, want_dist, abs(dist - want_dist), e_dist))
    assert slope == want_slope
    if kw.get("subpixel", True) is False:
        assert dist == want_dist
    else:
        assert abs(dist - want_dist) <= 4 * e_dist
    assert abs(dist - want_dist) <= CAP


def test_select_peaks_raises(lp):
    mat, kw = case("line_hor")
    for fn in (lp.calc_slope_distance_hor_lines, lp.calc_slope_distance_ver_lines):
        with pytest.raises(NotImplementedError, match="select_peaks"):
            fn(mat, select_peaks=True, **kw)


def test_result_feeds_the_cross_points(lp):
    mat, kw = case("line_hor")
    slope_hor, dist_hor = lp.calc_slope_distance_hor_lines(mat, **kw)
    slope_ver, dist_ver = lp.calc_slope_distance_ver_lines(mat, **kw)
    hor = lp.get_cross_points_hor_lines(mat, slope_ver, dist_ver)
    ver = lp.get_cross_points_ver_lines(mat, slope_hor, dist_hor)
    print("cross points from the searched slopes and distances: %d on horizontal lines, %d on vertical lines" % (len(hor), len(ver)))
    assert hor.ndim == 2 and hor.shape[1] == 2 and len(hor) >= 50 and ver.ndim == 2 and len(ver) >= 50
