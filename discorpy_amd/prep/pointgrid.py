"""The point-list steps of ``discorpy.prep.preprocessing`` that strongly curved (fisheye) grids need between the points and ``proc``:
the parabola mask, rotation and removal of points, and the grouping of dots into lines that follows each line with a polynomial fit.

* :func:`make_parabola_mask`, :func:`remove_points_using_parabola_mask`   reference ``preprocessing.py:856-963``
* :func:`rotate_points`, :func:`remove_subset_points`   reference ``preprocessing.py:1000-1047``
* :func:`group_dots_hor_lines_based_polyfit`, :func:`group_dots_ver_lines_based_polyfit`   reference ``preprocessing.py:1144-1404``

Same names, arguments, defaults, messages and return types.  All of it is host NumPy / SciPy: a grid has a few thousand points and
these steps run once per lens (``DESIGN.md`` section 4 draws the line between image-sized work, which runs on the GPU, and this).  The
groupings start from this package's :func:`~discorpy_amd.prep.dotpattern.group_dots_hor_lines` /
:func:`~discorpy_amd.prep.dotpattern.group_dots_ver_lines` on the strip around the middle of the grid, where the lines are straight,
and grow each line outwards: a parabola is fitted to the points collected so far and the points of the next strip that lie within
``ratio * line_dist`` of it join the line.

:func:`remove_points_using_parabola_mask` without rotation evaluates the mask's four inequalities at the truncated coordinates of the
points instead of building the mask: the same comparisons on the same numbers, so the same points as the full-mask lookup.
"""
import numpy as np
import scipy.ndimage as ndi

from .dotpattern import group_dots_hor_lines, group_dots_ver_lines

__all__ = ["make_parabola_mask", "remove_points_using_parabola_mask", "rotate_points", "remove_subset_points",
           "group_dots_hor_lines_based_polyfit", "group_dots_ver_lines_based_polyfit"]


def _margins(hor_margin, ver_margin, height, width):
    """(top, bottom, left, right) of an int or a (first, last) pair per axis, with the reference's checks."""
    top, bot = (ver_margin[0], ver_margin[-1]) if isinstance(ver_margin, (tuple, list)) else (ver_margin, ver_margin)
    left, right = (hor_margin[0], hor_margin[-1]) if isinstance(hor_margin, (tuple, list)) else (hor_margin, hor_margin)
    if (left + right) > width:
        raise ValueError("Invalid horizontal margin!!!")
    if (top + bot) > height:
        raise ValueError("Invalid vertical margin!!!")
    return top, bot, left, right


def _inside_parabolas(y, x, height, width, hor_curviness, ver_curviness, margins):
    """The four inequalities of the mask at integer coordinates ``y``, ``x`` (arrays that broadcast): below the top parabola, above the
    bottom one, right of the left one, left of the right one."""
    top, bot, left, right = margins
    sag_y = (ver_curviness / width) * (x - width / 2) ** 2
    sag_x = (hor_curviness / height) * (y - height / 2) ** 2
    return (y > sag_y + top) & (y < -sag_y + height - bot) & (x > sag_x + left) & (x < -sag_x + width - right)


def make_parabola_mask(height, width, hor_curviness=0.3, ver_curviness=0.3, hor_margin=100, ver_margin=100, rotate=0.0):
    """
    Create a 2D mask with parabolic boundary: parabolic curves on the four sides of a 2D array, optionally rotated.

    Parameters
    ----------
    height : int
        Height of the mask.
    width : int
        Width of the mask.
    hor_curviness : float, optional
        Horizontal curvature factor of the left and right boundaries. Larger is stronger.
    ver_curviness : float, optional
        Vertical curvature factor of the top and bottom boundaries. Larger is stronger.
    hor_margin : int or tuple of int, optional
        Horizontal margins (left and right of an image).
    ver_margin : int or tuple of int, optional
        Vertical margins (top and bottom of an image).
    rotate : float, optional
        Angle (degrees) to rotate the mask.

    Returns
    -------
    mask : array_like
        2D float32 array which values are 1.0 inside the mask and 0.0 outside.
    """
    margins = _margins(hor_margin, ver_margin, height, width)
    y, x = np.ogrid[:height, :width]
    mask = np.float32(_inside_parabolas(y, x, height, width, hor_curviness, ver_curviness, margins))
    if rotate != 0.0:
        mask = np.round(ndi.rotate(mask, rotate, reshape=False))
    return np.float32(mask)


def remove_points_using_parabola_mask(points, height, width, hor_curviness=0.3, ver_curviness=0.3, hor_margin=100, ver_margin=100,
                                      rotate=0.0):
    """
    Remove points outside a parabolic mask (:func:`make_parabola_mask` with the same arguments).

    Parameters
    ----------
    points : array_like
        Array of shape (N, 2) of (y, x)-coordinates of points.
    height, width, hor_curviness, ver_curviness, hor_margin, ver_margin, rotate
        As for :func:`make_parabola_mask`.

    Returns
    -------
    array_like
        Filtered points. Array of shape (M, 2) of (y, x)-coordinates of points: those whose coordinates, truncated to ``np.int32``,
        lie inside the frame and on a pixel of the mask that is 1.
    """
    y_cors, x_cors = np.int32(points[:, 0]), np.int32(points[:, 1])
    in_frame = (y_cors >= 0) & (y_cors < height) & (x_cors >= 0) & (x_cors < width)
    if rotate != 0.0:
        mask = make_parabola_mask(height, width, hor_curviness=hor_curviness, ver_curviness=ver_curviness, hor_margin=hor_margin,
                                  ver_margin=ver_margin, rotate=rotate)
        # (as in the reference, an index outside the frame wraps or raises inside the lookup before the frame test discards it)
        return points[in_frame & (mask[y_cors, x_cors] == 1.0)]
    margins = _margins(hor_margin, ver_margin, height, width)
    if np.any(y_cors >= height) or np.any(y_cors < -height) or np.any(x_cors >= width) or np.any(x_cors < -width):
        np.empty((height, width), np.bool_)[y_cors, x_cors]          # the reference's lookup raises NumPy's IndexError here
    # the mask's own index arrays are int64 (np.ogrid): the same comparisons on the same numbers
    inside = _inside_parabolas(y_cors.astype(np.int64), x_cors.astype(np.int64), height, width, hor_curviness, ver_curviness, margins)
    return points[in_frame & inside]


def rotate_points(points, angle, degree_unit=True):
    """
    Rotate a set of 2D points by a specified angle.

    Parameters
    ----------
    points : array_like
        Array of shape (N, 2) of (y, x)-coordinates of points.
    angle : float
        Rotation angle in degree or radian. Positive values rotate counterclockwise.
    degree_unit : bool, optional
        To select the unit of the input angle.

    Returns
    -------
    array_like
        Array of shape (N, 2) of rotated (y, x)-coordinates of the points.
    """
    points = np.asarray(points)
    if degree_unit:
        angle = np.deg2rad(angle)
    y, x = points[:, 0], points[:, 1]
    cos_a, sin_a = np.cos(angle), np.sin(angle)
    return np.column_stack((x * sin_a + y * cos_a, x * cos_a - y * sin_a))


def remove_subset_points(selected_points, points):
    """
    Remove a subset points from a set of points.

    Parameters
    ----------
    selected_points : array_like
        Array of shape (N, 2) of (y, x)-coordinates of points to exclude.
    points : array_like
        Array of shape (M, 2) of (y, x)-coordinates of points.

    Returns
    -------
    array_like
        Array of shape (K, 2) of points after the removal (compared coordinate for coordinate, exactly).
    """
    excluded = {tuple(pair) for pair in selected_points}
    return np.asarray([pair for pair in points if tuple(pair) not in excluded])


# --------------------------------------------------------------------------- grouping that follows a polynomial fit
# `along` is the column of the coordinate that runs along a line (1: x for horizontal lines, 0: y for vertical ones), 1 - along the
# column of the coordinate the fit predicts.

def _nearby_points(current_points, points, residual, order, along):
    fit = np.poly1d(np.polyfit(current_points[:, along], current_points[:, 1 - along], int(order)))
    distances = np.abs(points[:, 1 - along] - fit(points[:, along]))
    return points[distances <= residual]


def _get_nearby_hor_points(current_points, points, residual, order=2):
    """The ``points`` (an (M, 2) array of (y, x)) within ``residual`` in y of the polynomial y(x) of degree ``order`` fitted to
    ``current_points``."""
    return _nearby_points(current_points, points, residual, order, 1)


def _get_nearby_ver_points(current_points, points, residual, order=2):
    """The ``points`` within ``residual`` in x of the polynomial x(y) of degree ``order`` fitted to ``current_points``."""
    return _nearby_points(current_points, points, residual, order, 0)


def _nearby_points_iter(initial_points, points, low, high, search_dist, residual, overlap_ratio, order, along):
    """Grow ``initial_points`` strip by strip: the strips ``(high, high + search_dist]`` and ``[low - search_dist, low)`` of the coordinate
    along the line, each widened by ``overlap_ratio * search_dist`` on both sides, move outwards one ``search_dist`` per step; the points
    of both strips near the fit through everything selected so far are added (duplicates merged, rows sorted: ``np.unique``).  Stops
    at the first step whose strips are empty or add nothing."""
    overlap = search_dist * np.clip(overlap_ratio, 0.0, 1.0)
    coord = points[:, along]
    selected = initial_points
    while True:
        in_strips = (((high + search_dist + overlap >= coord) & (coord > high - overlap))
                     | ((low - search_dist - overlap <= coord) & (coord < low + overlap)))
        indices = np.where(in_strips)[0]
        if len(indices) == 0:
            break
        nearby = _nearby_points(selected, points[indices], residual, order, along)
        if len(nearby) == 0:
            break
        selected = np.unique(np.vstack([selected, nearby]), axis=0)
        high = high + search_dist
        low = low - search_dist
    return selected


def _get_nearby_hor_points_iter(initial_points, points, x_left, x_right, search_dist, residual, overlap_ratio=0.5, order=2):
    """Iteratively collect the points of a horizontal line outwards from ``x_left`` / ``x_right`` (see :func:`_nearby_points_iter`)."""
    return _nearby_points_iter(initial_points, points, x_left, x_right, search_dist, residual, overlap_ratio, order, 1)


def _get_nearby_ver_points_iter(initial_points, points, y_left, y_right, search_dist, residual, overlap_ratio=0.5, order=2):
    """Iteratively collect the points of a vertical line outwards from ``y_left`` / ``y_right`` (see :func:`_nearby_points_iter`)."""
    return _nearby_points_iter(initial_points, points, y_left, y_right, search_dist, residual, overlap_ratio, order, 0)


def _group_based_polyfit(points, slope, line_dist, ratio, num_dot_miss, accepted_ratio, overlap_ratio, order, along):
    angle = -np.arctan(slope) if along == 1 else np.arctan(slope)
    num_points = len(points)
    if num_points == 0:
        raise ValueError("Input is empty!!!")
    points = rotate_points(points, angle, degree_unit=False)
    points = points[points[:, along].argsort()]
    coord = points[:, along]
    c_min, c_max = coord[0], coord[-1]
    c_mid = (c_min + c_max) * 0.5
    num_dot_miss = np.clip(num_dot_miss, 1, num_points)
    search_dist = num_dot_miss * line_dist + 0.5 * line_dist
    c_start = np.clip(c_mid - search_dist, c_min, c_max)
    c_stop = np.clip(c_mid + search_dist, c_min, c_max)
    strip = np.where((coord >= c_start) & (coord <= c_stop))[0]
    group_strip = group_dots_hor_lines if along == 1 else group_dots_ver_lines
    list_lines = []
    if len(strip) > 0:
        selected = points[strip]
        seeds = group_strip(selected, 0.0, line_dist, ratio=ratio, num_dot_miss=num_dot_miss, accepted_ratio=accepted_ratio)
        residual = ratio * line_dist
        for seed in seeds:
            # (a seed of one or two points is not grown: the line found before it stands in for it, as in the reference)
            if len(seed) > 2:
                selected = _nearby_points_iter(seed, points, seed[0, along], seed[-1, along], search_dist, residual, overlap_ratio,
                                               order, along)
            if len(selected) > 2:
                selected = rotate_points(selected, -angle, degree_unit=False)
                selected = selected[selected[:, along].argsort()]
                list_lines.append(selected)
    len_accepted = np.int16(accepted_ratio * np.max([len(line) for line in list_lines]))
    lines = [line for line in list_lines if len(line) > len_accepted]
    # of neighbouring lines at the same place across the grid (less than a tenth of the line distance apart) only the first stays
    across = [np.median(line[:, 1 - along]) for line in lines]
    distinct = np.where(np.abs(np.diff(across)) > 0.1 * line_dist)[0]
    if len(distinct) > 0:
        distinct = np.insert(distinct + 1, 0, 0)
        lines = [line for idx, line in enumerate(lines) if idx in distinct]
    return sorted(lines, key=lambda line: np.mean(line[:, 1 - along]))


def group_dots_hor_lines_based_polyfit(points, slope, line_dist, ratio=0.1, num_dot_miss=3, accepted_ratio=0.65, overlap_ratio=0.5,
                                       order=2):
    """
    Group dots into horizontal lines by following each line with a polynomial fit.

    Parameters
    ----------
    points : array_like
        Array of shape (N, 2) of (y, x)-coordinates of points.
    slope : float
        Horizontal slope of the grid.
    line_dist : float
        Nominal distance between two lines.
    ratio : float
        Acceptable variation.
    num_dot_miss : int
        Acceptable missing dots between dot1 and dot2.
    accepted_ratio : float
        Use to select lines having the number of dots equal to or larger than the multiplication of the `accepted_ratio` and the
        maximum number of dots per line.
    overlap_ratio : float, optional
        To specify the overlap of the searching range between searching steps.
    order : int, optional
        Polynomial order.

    Returns
    -------
    list of array_like
        List of 2D arrays. Each array is (y, x)-coordinates of points belong to the same group. Length of each list may be different.
    """
    return _group_based_polyfit(points, slope, line_dist, ratio, num_dot_miss, accepted_ratio, overlap_ratio, order, 1)


def group_dots_ver_lines_based_polyfit(points, slope, line_dist, ratio=0.1, num_dot_miss=3, accepted_ratio=0.65, overlap_ratio=0.5,
                                       order=2):
    """
    Group dots into vertical lines by following each line with a polynomial fit.

    Parameters
    ----------
    points : array_like
        Array of shape (N, 2) of (y, x)-coordinates of points.
    slope : float
        Vertical slope of the grid.
    line_dist : float
        Nominal distance between two lines.
    ratio, num_dot_miss, accepted_ratio, overlap_ratio, order
        As for :func:`group_dots_hor_lines_based_polyfit`.

    Returns
    -------
    list of array_like
        List of 2D arrays. Each array is (y, x)-coordinates of points belong to the same group. Length of each list may be different.
    """
    return _group_based_polyfit(points, slope, line_dist, ratio, num_dot_miss, accepted_ratio, overlap_ratio, order, 0)
