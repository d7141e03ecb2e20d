"""CPU suite for the completed post module: the NumPy emulation of the forward scatter against the reference's outputs (golden G21),
the three NumPy assessment helpers against the reference's (golden G23), and the module's public surface against the reference's
list of public names.  No GPU: the emulation helper stands in for an oracle the forward scatter does not have."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, golden

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import forward_emulation as fe  # noqa: E402


@pytest.fixture(scope="module")
def g21():
    return golden("g21_forward_images")


@pytest.fixture(scope="module")
def g23():
    return golden("g23_residuals")


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", fe.g21_names())
def test_emulation_equals_the_reference_bit_for_bit(g21, name):
    mat, xc, yc, fact = fe.g21_input(name)
    assert tuple(g21["shape_" + name]) == mat.shape and float(g21["xcenter_" + name]) == xc and list(g21["list_fact_" + name]) == fact
    assert same_bytes(fe.unwarp_image_forward(mat, xc, yc, fact), g21["out_" + name])


def test_golden_margins_make_bit_equality_a_fair_demand(g21):
    """Every case that is not a tie case keeps its coordinates >= 1e-9 px from a half-integer (the generator refuses less); the tie
    cases sit exactly on them, more than a thousand times."""
    for name in fe.g21_names():
        margin = float(g21["margin_" + name])
        assert margin == fe.half_integer_margin(*fe.g21_input(name)[0].shape, *fe.g21_input(name)[1:])
        assert (margin == 0.0) if name.startswith("tie_") else (margin >= 1e-9), (name, margin)
    assert int(g21["ties_tie_half"]) > 1000


def test_one_pixel_case_keeps_the_last_source_pixel(g21):
    mat, xc, yc, fact = fe.g21_input("one_pixel")
    out = g21["out_one_pixel"]
    assert np.count_nonzero(out) == 1 and out[int(np.rint(yc)), int(np.rint(xc))] == mat[-1, -1]


@pytest.mark.parametrize("name", ["hor_warped", "hor_corrected", "ver_warped", "ver_corrected"])
def test_residuals_and_check_agree_with_the_reference(g23, name):
    import discorpy_amd.post.postprocessing as post
    fn = post.calc_residual_hor if name.startswith("hor") else post.calc_residual_ver
    res = fn(list(g23[name + "_lines"]), float(g23["xcenter"]), float(g23["ycenter"]))
    want = g23[name + "_residuals"]
    assert res.shape == want.shape and res.dtype == want.dtype
    np.testing.assert_allclose(res, want, rtol=1e-9, atol=0)
    check = post.check_distortion(res)
    assert isinstance(check, bool) and check == bool(g23[name + "_check"])
    assert post.check_distortion(want) == bool(g23[name + "_check"])


def test_both_outcomes_of_the_check_are_present(g23):
    assert {bool(g23[k]) for k in g23 if k.endswith("_check")} == {True, False}


def test_residuals_of_lists_and_mixed_line_lengths():
    import discorpy_amd.post.postprocessing as post
    lines = [[[10.0, 1.0], [10.5, 5.0], [10.2, 9.0]], np.array([[20.0, 0.0], [20.0, 4.0], [20.0, 8.0], [20.0, 12.0]])]
    res = post.calc_residual_hor(lines, 6.0, 15.0)
    assert res.shape == (7, 2) and np.all(np.diff(res[:, 0]) >= 0)
    straight = res[np.isin(res[:, 0], np.hypot(np.array([0.0, 4.0, 8.0, 12.0]) - 6.0, 5.0))]
    assert np.all(straight[:, 1] < 1e-12)
    assert post.check_distortion(np.array([[0.0, 2.0]] * 16 + [[0.0, 0.5]] * 84)) is True       # 16 % above one pixel
    assert post.check_distortion(np.array([[0.0, 2.0]] * 15 + [[0.0, 0.5]] * 85)) is False      # 15 % is not "more than"


def test_every_public_name_of_the_reference_is_offered(g23):
    import discorpy_amd.post.postprocessing as post
    names = [str(n) for n in g23["public_names"]]
    assert len(names) == 11 and "unwarp_image_forward" in names and "check_distortion" in names
    for n in names:
        assert callable(getattr(post, n)), n
        assert n in post.__all__, n


def test_new_symbols_are_declared_and_bound():
    from discorpy_amd import _ffi as F
    header = open(os.path.join(ROOT, "include", "discorpy_hip.h")).read()
    for sym in ("dcp_unwarp_image_forward", "dcp_map_points_inverse_f64"):
        assert sym in F.SIGNATURES and ("int " + sym + "(") in header
