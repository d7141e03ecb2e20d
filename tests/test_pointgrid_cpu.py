"""CPU suite for discorpy_amd.prep.pointgrid against golden G31 (what the reference's functions returned): the parabola masks and the
points they keep by ==, rotate_points and remove_subset_points by ==, both polyfit groupings on a barrel-distorted grid line for line
(the same number of lines and of points per line, coordinates within 1e-9 px: a fit rounded differently on another CPU may move a
rotated coordinate by an ulp, as tests/test_proc_cpu.py argues for its fits), and the reference's ValueErrors."""
import ast
import os

import numpy as np
import pytest

from conftest import ROOT

from discorpy_amd.prep import dotpattern, pointgrid

G31 = np.load(os.path.join(ROOT, "tests", "golden", "g31_prep_rest.npz"))
MASKS = [ast.literal_eval(str(s)) for s in G31["mask_args"]]
SLOPE, PITCH, GROUP = 0.02, 40.0, dict(ratio=0.15, num_dot_miss=2)


def test_the_recorded_masks_cover_the_three_shapes():
    assert len(MASKS) == 3
    assert isinstance(MASKS[0]["hor_margin"], tuple) and isinstance(MASKS[0]["ver_margin"], tuple)
    assert MASKS[1]["rotate"] == 7.5
    assert 2 * MASKS[2]["hor_margin"] == MASKS[2]["width"] and sum(MASKS[2]["ver_margin"]) == MASKS[2]["height"]


@pytest.mark.parametrize("i", range(3))
def test_parabola_mask_equals_the_references(i):
    kw = MASKS[i]
    mask = pointgrid.make_parabola_mask(**kw)
    assert mask.dtype == np.float32 and mask.shape == (kw["height"], kw["width"])
    want = np.unpackbits(G31["mask%d_bits" % i])[:mask.size].reshape(mask.shape)
    assert np.array_equal(mask, want.astype(np.float32))
    if i == 2:
        assert not mask.any()          # margins that meet leave nothing
    else:
        assert 0 < mask.sum() < mask.size


@pytest.mark.parametrize("i", range(3))
def test_points_kept_equal_the_references_and_the_full_mask_lookup(i):
    kw = MASKS[i]
    pts = G31["mask%d_points" % i]
    kept = pointgrid.remove_points_using_parabola_mask(pts, **kw)
    assert np.array_equal(kept, G31["mask%d_kept" % i])
    # the lookup the reference performs, point by point, truncation and frame test included
    mask = pointgrid.make_parabola_mask(**kw)
    y, x = np.int32(pts[:, 0]), np.int32(pts[:, 1])
    lookup = (y >= 0) & (y < kw["height"]) & (x >= 0) & (x < kw["width"]) & (mask[y, x] == 1.0)
    assert np.array_equal(kept, pts[lookup])
    assert (pts < 0).any() and (np.int32(pts[(pts < 0).any(axis=1)]) == 0).any()          # points that only the truncation brings inside


def test_points_at_every_pixel_equal_the_mask():
    """Without rotation the inequalities are evaluated at the points: every pixel centre and corner of a frame agrees with the mask."""
    kw = dict(height=37, width=53, hor_curviness=0.5, ver_curviness=0.25, hor_margin=(4, 9), ver_margin=3)
    mask = pointgrid.make_parabola_mask(**kw)
    yy, xx = np.mgrid[:37, :53]
    for shift in (0.0, 0.5, 0.999):
        pts = np.column_stack((yy.ravel() + shift, xx.ravel() + shift))
        kept = pointgrid.remove_points_using_parabola_mask(pts, **kw)
        assert np.array_equal(kept, pts[mask.ravel() == 1.0])
    with pytest.raises(IndexError):
        pointgrid.remove_points_using_parabola_mask(np.array([[37.0, 3.0]]), **kw)          # as the reference's lookup raises


def test_rotate_points_and_remove_subset_points_equal_the_references():
    pts = G31["rot_points"]
    assert np.array_equal(pointgrid.rotate_points(pts, 12.5), G31["rot_deg"])
    assert np.array_equal(pointgrid.rotate_points(pts, -0.3, degree_unit=False), G31["rot_rad"])
    assert np.array_equal(pointgrid.rotate_points(pts.tolist(), 12.5), G31["rot_deg"])
    left = pointgrid.remove_subset_points(G31["subset_selected"], pts)
    assert np.array_equal(left, G31["subset_left"]) and len(left) == len(pts) - 3


def split(flat, lengths):
    return np.split(flat, np.cumsum(lengths)[:-1])


@pytest.mark.parametrize("name", ["full", "holes", "outlier"])
@pytest.mark.parametrize("tag", ["hor", "ver"])
def test_polyfit_grouping_equals_the_references(name, tag):
    pts = G31["grid_%s_points" % name]
    group = pointgrid.group_dots_hor_lines_based_polyfit if tag == "hor" else pointgrid.group_dots_ver_lines_based_polyfit
    lines = group(pts, SLOPE, PITCH, **GROUP)
    want_len = G31["grid_%s_%s_len" % (name, tag)]
    assert [len(line) for line in lines] == list(want_len)
    for line, want in zip(lines, split(G31["grid_%s_%s" % (name, tag)], want_len)):
        assert np.abs(line - want).max() <= 1e-9
    if name == "full":
        assert list(want_len) == ([17] * 15 if tag == "hor" else [15] * 17)
    if name == "outlier":          # the point between the lines joins none
        assert sum(want_len) == len(pts) - 1


def test_the_grid_is_too_curved_for_the_plain_grouping():
    pts = G31["grid_full_points"]
    plain_h = sum(len(line) for line in dotpattern.group_dots_hor_lines(pts, SLOPE, PITCH))
    plain_v = sum(len(line) for line in dotpattern.group_dots_ver_lines(pts, SLOPE, PITCH))
    assert [plain_h, plain_v] == list(G31["grid_plain_counts"])
    assert plain_h < len(pts) and plain_v < len(pts)


def test_the_references_value_errors():
    with pytest.raises(ValueError, match="Input is empty!!!"):
        pointgrid.group_dots_hor_lines_based_polyfit(np.zeros((0, 2)), SLOPE, PITCH)
    with pytest.raises(ValueError, match="Input is empty!!!"):
        pointgrid.group_dots_ver_lines_based_polyfit([], SLOPE, PITCH)
    with pytest.raises(ValueError, match="Invalid horizontal margin!!!"):
        pointgrid.make_parabola_mask(50, 70, hor_margin=(35, 36))
    with pytest.raises(ValueError, match="Invalid vertical margin!!!"):
        pointgrid.make_parabola_mask(50, 70, hor_margin=10, ver_margin=26)
    with pytest.raises(ValueError, match="Invalid vertical margin!!!"):
        pointgrid.remove_points_using_parabola_mask(np.zeros((3, 2)), 50, 70, hor_margin=10, ver_margin=[30, 21])
