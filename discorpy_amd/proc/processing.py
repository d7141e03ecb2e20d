"""Drop-in for ``discorpy.proc.processing``: from grouped lines of points to a calibration.

The step between ``prep`` (an image becomes lines of points) and ``post`` (a calibration is applied): the centre of distortion
(:func:`find_cod_coarse`, :func:`find_cod_fine`, :func:`find_cod_bailey`, the two vanishing-point searches), the polynomial of the
radial model (:func:`calc_coef_backward`, :func:`calc_coef_forward`, :func:`calc_coef_backward_from_forward`,
:func:`transform_coef_backward_and_forward`), regenerated grids, and the eight coefficients of a homography
(:func:`calc_perspective_coefficients` and what feeds it).  Same names, parameters, defaults, return types and messages as the
reference's module (``discorpy/proc/processing.py``).

All of it is NumPy and SciPy on the host (a few thousand numbers, once per lens); there is no kernel under this
module.  The one function that needs a device is :func:`correct_perspective_effect`, whose last step is
``post.correct_perspective_line`` (``dcp_map_points_perspective_f64``).

What the results depend on, kept as the reference has it:

* the tables of parabola and line coefficients, the undistorted intercepts and the regenerated ``(H, V, 2)`` grids are float32; the
  lines that come back shifted to the centre are float64 for float64 input;
* whatever the reference computes from a float32 table in float32 (the coarse centre, Bailey's update, the vanishing points) is
  computed in float32 here: the expressions carry NumPy scalars of the table's type, as the reference's do;
* the optimiser calls (``scipy.optimize.minimize`` with BFGS from the reference's start value, ``scipy.optimize.fsolve`` from
  ``(0, 0)``) get the same problem: same callable arithmetic, same argument types, default tolerances.  :func:`find_cod_fine` depends
  on where BFGS stops, not on the true minimum ("Calibration (proc)"), so it is host code on purpose;
* least squares is ``np.linalg.lstsq(..., rcond=1e-64)`` on design matrices built with ``np.power(value, np.arange(num_fact,
  dtype=np.int16))``.

The reference's loops over the points of a line are array expressions here with the same arithmetic per element; loops over lines and
the optimiser calls stay loops.

One deliberate difference: :func:`correct_perspective_effect` raises the reference's "No curved line open ..." messages when a group
of lines is empty.  The reference tests the length of ``np.where``'s tuple, which is never zero, and goes on to a NaN (``"mean"``,
``"median"``) or an ``IndexError`` (``"min"``, ``"max"``).
"""
import warnings

import numpy as np
from scipy import optimize

from ..post import postprocessing as post
from ..util.utility import transform_coef_backward_and_forward

__all__ = ["find_cod_coarse", "find_cod_fine", "find_cod_bailey", "calc_coef_backward", "calc_coef_forward",
           "calc_coef_backward_from_forward", "transform_coef_backward_and_forward", "regenerate_grid_points_parabola",
           "regenerate_grid_points_linear", "generate_undistorted_perspective_lines", "generate_source_target_perspective_points",
           "generate_4_source_target_perspective_points", "calc_perspective_coefficients", "update_center",
           "correct_perspective_effect", "find_center_based_vanishing_points", "find_center_based_vanishing_points_iteration"]


# --------------------------------------------------------------------------- parabola tables

def _para_fit(list_lines, xcenter, ycenter, horizontal):
    table = np.zeros((len(list_lines), 3), dtype=np.float32)
    shifted = []
    for i, item in enumerate(list_lines):
        line = np.asarray(item)
        dy, dx = line[:, 0] - ycenter, line[:, 1] - xcenter
        table[i] = np.polyfit(dx, dy, 2) if horizontal else np.polyfit(dy, dx, 2)
        shifted.append(np.stack((dy, dx), axis=1))
    return table, shifted


def _para_fit_hor(list_lines, xcenter, ycenter):
    """
    Fit a parabola ``y = a x**2 + b x + c`` to every horizontal line, in coordinates relative to the centre.

    Parameters
    ----------
    list_lines : list of 2D arrays
        (y, x) coordinates of the points of each line.
    xcenter, ycenter : float
        The centre the coordinates are shifted to.

    Returns
    -------
    list_coef : array_like
        float32 table ``(number of lines, 3)`` of ``(a, b, c)``.
    list_slines : list of 2D arrays
        The lines as ``(y - ycenter, x - xcenter)``.
    """
    return _para_fit(list_lines, xcenter, ycenter, True)


def _para_fit_ver(list_lines, xcenter, ycenter):
    """
    Fit a parabola ``x = a y**2 + b y + c`` to every vertical line, in coordinates relative to the centre.

    Parameters and returns as :func:`_para_fit_hor`.
    """
    return _para_fit(list_lines, xcenter, ycenter, False)


def _turning_pair(table, column):
    """Mean of `column` over the two neighbouring lines between which the curvature changes sign."""
    pos = np.argmax(np.abs(np.diff(np.sign(table[:, 0])))) + 1
    return (table[pos - 1, column] + table[pos, column]) * 0.5


def find_cod_coarse(list_hor_lines, list_ver_lines):
    """
    Coarse estimate of the centre of distortion: where the horizontal and the vertical line of zero curvature cross, each taken
    as the mean of the two neighbouring lines whose curvatures have opposite signs.

    Parameters
    ----------
    list_hor_lines : list of 2D arrays
        List of (y,x)-coordinates of points on each horizontal line.
    list_ver_lines : list of 2D arrays
        List of (y,x)-coordinates of points on each vertical line.

    Returns
    -------
    xcenter : float
        Center of distortion in the x-direction.
    ycenter : float
        Center of distortion in the y-direction.
    """
    coef_hor = _para_fit_hor(list_hor_lines, 0.0, 0.0)[0]
    coef_ver = _para_fit_ver(list_ver_lines, 0.0, 0.0)[0]
    ycenter0, slope_hor = _turning_pair(coef_hor, 2), _turning_pair(coef_hor, 1)
    xcenter0, slope_ver = _turning_pair(coef_ver, 2), _turning_pair(coef_ver, 1)
    ycenter = (ycenter0 + xcenter0 * slope_hor) / (1.0 - slope_hor * slope_ver)
    xcenter = (xcenter0 + ycenter0 * slope_ver) / (1.0 - slope_hor * slope_ver)
    return xcenter, ycenter


# --------------------------------------------------------------------------- the fine search

def _sq_dist_to_origin(t, a, b, c):
    """Squared distance from the origin to the point of the parabola ``a t**2 + b t + c`` at ``t``."""
    return t ** 2 + (a * t ** 2 + b * t + c) ** 2


def _nearest_points(table):
    """Per parabola of the table: where BFGS, started at 0, stops on its way to the point nearest to the origin -- (argument, value),
    written into float32."""
    points = np.zeros((len(table), 2), dtype=np.float32)
    for i, coefs in enumerate(table):
        t = optimize.minimize(_sq_dist_to_origin, 0.0, args=tuple(coefs)).x[0]
        points[i, 0] = t
        points[i, 1] = coefs[0] * t ** 2 + coefs[1] * t + coefs[2]
    return points


def _calc_error(list_coef_hor, list_coef_ver):
    """
    How far the fitted parabolas are from passing through the origin: the point of each parabola nearest to the origin is located,
    a straight line is fitted through those points per direction, and the magnitudes of the two intercepts are added.

    Parameters
    ----------
    list_coef_hor, list_coef_ver : array_like
        Tables of parabola coefficients of the horizontal and the vertical lines.

    Returns
    -------
    float
    """
    hpoints = _nearest_points(list_coef_hor)
    vpoints = _nearest_points(list_coef_ver)
    error_h = np.polyfit(hpoints[:, 0], hpoints[:, 1], 1)[-1]
    error_v = np.polyfit(vpoints[:, 0], vpoints[:, 1], 1)[-1]
    return np.abs(error_h) + np.abs(error_v)


def _middle_lines(position, num_use, num_line):
    return max(0, position - num_use), min(num_line, position + num_use + 1)


def _metric_matrix(list_hor_lines, list_ver_lines, xcenter, ycenter, list_xshift, list_yshift):
    """The float32 matrix :func:`_calc_metric` takes its minimum of: ``[i, j]`` is :func:`_calc_error` of the middle lines -- already
    shifted by the centre -- fitted again about ``(list_xshift[j], list_yshift[i])``."""
    coef_hor, hor_lines = _para_fit_hor(list_hor_lines, xcenter, ycenter)
    coef_ver, ver_lines = _para_fit_ver(list_ver_lines, xcenter, ycenter)
    num_hline, num_vline = len(hor_lines), len(ver_lines)
    num_use = min(5, num_hline // 2 - 1, num_vline // 2 - 1)
    h1, h2 = _middle_lines(np.argmin(np.abs(coef_hor[:, 2])), num_use, num_hline)
    v1, v2 = _middle_lines(np.argmin(np.abs(coef_ver[:, 2])), num_use, num_vline)
    metric = np.zeros((len(list_xshift), len(list_yshift)), dtype=np.float32)
    for j, xshift in enumerate(list_xshift):
        for i, yshift in enumerate(list_yshift):
            metric[i, j] = _calc_error(_para_fit_hor(hor_lines[h1:h2], xshift, yshift)[0],
                                       _para_fit_ver(ver_lines[v1:v2], xshift, yshift)[0])
    return metric


def _calc_metric(list_hor_lines, list_ver_lines, xcenter, ycenter, list_xshift, list_yshift):
    """
    The shift of the centre, among the candidates, at which the middle lines pass closest to it.

    Parameters
    ----------
    list_hor_lines, list_ver_lines : list of 2D arrays
        (y, x) coordinates of the points of each line.
    xcenter, ycenter : float
        Centre the candidates are offsets from.
    list_xshift, list_yshift : list of float
        Candidate offsets in x and in y.

    Returns
    -------
    xshift, yshift : float
        The chosen offsets.
    """
    metric = _metric_matrix(list_hor_lines, list_ver_lines, xcenter, ycenter, list_xshift, list_yshift)
    row, col = np.unravel_index(metric.argmin(), metric.shape)
    return list_xshift[col], list_yshift[row]


def find_cod_fine(list_hor_lines, list_ver_lines, xcenter, ycenter, point_dist):
    """
    Search around a coarse centre of distortion: first offsets of up to ``point_dist`` in steps of 2, then offsets of up to 2 in
    steps of 0.5 around the first pass's choice.

    Parameters
    ----------
    list_hor_lines : list of 2D arrays
        List of the (y,x)-coordinates of points on each horizontal line.
    list_ver_lines : list of 2D arrays
        List of the (y,x)-coordinates of points on each vertical line.
    xcenter : float
        Coarse estimation of the CoD in x-direction.
    ycenter : float
        Coarse estimation of the CoD in y-direction.
    point_dist : float
        Median distance of two nearest points.

    Returns
    -------
    xcenter : float
        Center of distortion in x-direction.
    ycenter : float
        Center of distortion in y-direction.
    """
    coarse_step, fine_step = 2.0, 0.5
    shifts = np.arange(-point_dist, point_dist + coarse_step, coarse_step)
    xshift, yshift = _calc_metric(list_hor_lines, list_ver_lines, xcenter, ycenter, shifts, shifts)
    xcenter, ycenter = xcenter + xshift, ycenter + yshift
    shifts = np.arange(-coarse_step, coarse_step + fine_step, fine_step)
    xshift, yshift = _calc_metric(list_hor_lines, list_ver_lines, xcenter, ycenter, shifts, shifts)
    return xcenter + xshift, ycenter + yshift


# --------------------------------------------------------------------------- undistorted intercepts, radial coefficients

def _check_missing_lines(list_coef_hor, list_coef_ver, threshold=0.3):
    """
    Is a line missing from the grid?  The gaps between neighbouring intercepts are fitted with a parabola over the line index; a gap
    further than ``threshold`` (relative) from the fit says yes.

    Parameters
    ----------
    list_coef_hor, list_coef_ver : array_like
        Tables of parabola coefficients of the horizontal and the vertical lines.
    threshold : float
        Larger is less sensitive.

    Returns
    -------
    bool
    """
    worst = []
    for table in (list_coef_hor, list_coef_ver):
        gaps = np.abs(np.diff(table[:, 2]))
        index = np.arange(len(gaps))
        fact = np.polyfit(index, gaps, 2)
        fitted = fact[0] * index ** 2 + fact[1] * index + fact[2]
        worst.append(np.max(np.abs((gaps - fitted) / fitted)))
    return bool(worst[0] > threshold or worst[1] > threshold)


def _radial_spacing_cost(spacing, anchor, anchor_index, *intercepts):
    """Squared misfit of intercepts laid out at multiples of `spacing` on both sides of the anchor line."""
    return np.sum(np.asarray([(np.sign(c) * np.abs(i - anchor_index) * spacing + anchor - c) ** 2 for i, c in enumerate(intercepts)]))


def _perspective_spacing_cost(spacing, anchor, anchor_index, *intercepts):
    """Squared misfit of intercepts laid out at signed multiples of `spacing` from the anchor line."""
    return np.sum(np.asarray([((i - anchor_index) * spacing + anchor - c) ** 2 for i, c in enumerate(intercepts)]))


def _fit_spacing(cost, start, anchor_index, intercepts):
    """BFGS from `start` on one of the two costs above; the intercepts go in one by one, as scalars of their table's type."""
    return optimize.minimize(cost, start, args=(intercepts[anchor_index], anchor_index) + tuple(intercepts)).x[0]


def _calc_undistor_intercept(list_hor_lines, list_ver_lines, xcenter, ycenter, optimizing=False, threshold=0.3):
    """
    Intercepts of the undistorted lines: equally spaced on both sides of the line nearest to the centre, at the mean gap of the
    middle lines (refined by a one-parameter fit when ``optimizing``).

    Parameters
    ----------
    list_hor_lines, list_ver_lines : list of 2D arrays
        (y, x) coordinates of the points of each line.
    xcenter, ycenter : float
        Centre of distortion.
    optimizing : bool, optional
        Apply optimization if True.
    threshold : float
        To determine if there are missing lines. Larger is less sensitive.

    Returns
    -------
    list_hor_uc, list_ver_uc : array_like
        float32 intercepts of the undistorted horizontal and vertical lines.
    """
    coef_hor = _para_fit_hor(list_hor_lines, xcenter, ycenter)[0]
    coef_ver = _para_fit_ver(list_ver_lines, xcenter, ycenter)[0]
    if _check_missing_lines(coef_hor, coef_ver, threshold=threshold):
        warnings.warn("\n!!! Check if there is any missing grouped line !!!\n"
                      "Parameters of the methods of grouping points may need to be "
                      "adjusted!", UserWarning)
    num_hline, num_vline = len(coef_hor), len(coef_ver)
    num_use = min(3, num_hline // 2 - 1, num_vline // 2 - 1)
    result = []
    for table, num_line in ((coef_hor, num_hline), (coef_ver, num_vline)):
        inter = table[:, 2]
        pos = np.argmin(np.abs(inter))
        first, last = _middle_lines(pos, num_use, num_line)
        spacing = np.mean(np.abs(np.diff(inter[first:last])))
        if optimizing is True:
            spacing = _fit_spacing(_radial_spacing_cost, spacing, pos, inter)
        undistorted = np.zeros(num_line, dtype=np.float32)
        for i in range(num_line):
            undistorted[i] = np.sign(inter[i]) * (np.abs(i - pos) * spacing) + inter[pos]
        result.append(undistorted)
    return result[0], result[1]


def _clamp_num_fact(num_fact):
    return np.int16(np.clip(num_fact, 1, None))


def _solve(rows, values):
    """Least squares of the stacked blocks; without a single row it is NumPy's refusal of an empty matrix, as in the reference."""
    design = np.concatenate(rows) if rows else np.zeros((0, 0))
    if design.shape[0] == 0:
        design = np.asarray([], dtype=np.float64)
    target = np.concatenate(values) if values else np.asarray([], dtype=np.float64)
    return np.linalg.lstsq(design, target, rcond=1e-64)[0]


def _line_terms(line, coefs, horizontal):
    """Of every point of a shifted line: its radius, and the parabola without its linear term at the point's abscissa."""
    line = np.asarray(line, dtype=np.float64)
    yd, xd = line[:, 0], line[:, 1]
    a_coef, _, c_coef = np.float64(coefs)
    radius = np.sqrt(xd * xd + yd * yd)
    along = xd if horizontal else yd
    return radius, a_coef * along * along + c_coef


def _factor_rows(list_hor_lines, list_ver_lines, xcenter, ycenter, optimizing, threshold):
    """Per line: (radius of each point, parabola term of each point, undistorted intercept)."""
    hor_uc, ver_uc = _calc_undistor_intercept(list_hor_lines, list_ver_lines, xcenter, ycenter, optimizing=optimizing,
                                              threshold=threshold)
    coef_hor, hor_lines = _para_fit_hor(list_hor_lines, xcenter, ycenter)
    coef_ver, ver_lines = _para_fit_ver(list_ver_lines, xcenter, ycenter)
    for lines, table, uc, horizontal in ((hor_lines, coef_hor, hor_uc, True), (ver_lines, coef_ver, ver_uc, False)):
        for i, line in enumerate(lines):
            yield _line_terms(line, table[i], horizontal) + (np.float64(uc[i]),)


def calc_coef_backward(list_hor_lines, list_ver_lines, xcenter, ycenter, num_fact, optimizing=False, threshold=0.3):
    """
    Coefficients of the backward model: the polynomial ``B`` with ``rd / ru = B(ru)``, fitted over every point of every line.

    Parameters
    ----------
    list_hor_lines : list of 2D arrays
        List of the (y,x)-coordinates of points on each horizontal line.
    list_ver_lines : list of 2D arrays
        List of the (y,x)-coordinates of points on each vertical line.
    xcenter : float
        Center of distortion in x-direction.
    ycenter : float
        Center of distortion in y-direction.
    num_fact : int
        Number of the factors of polynomial.
    optimizing : bool, optional
        Apply optimization if True.
    threshold : float
        To determine if there are missing lines. Larger is less sensitive.

    Returns
    -------
    list_fact : list of float
        Coefficients of the polynomial.
    """
    expo = np.arange(_clamp_num_fact(num_fact), dtype=np.int16)
    rows, values = [], []
    for radius, term, uc in _factor_rows(list_hor_lines, list_ver_lines, xcenter, ycenter, optimizing, threshold):
        factor = term / uc
        rows.append(np.power((radius / factor)[:, None], expo[None, :]))
        values.append(factor)
    return _solve(rows, values)


def calc_coef_forward(list_hor_lines, list_ver_lines, xcenter, ycenter, num_fact, optimizing=False, threshold=0.3):
    """
    Coefficients of the forward model: the polynomial ``F`` with ``ru / rd = F(rd)``.  Lines whose undistorted intercept is zero
    and points whose factor is zero are left out.

    Parameters
    ----------
    list_hor_lines : list of 2D arrays
        List of the (y,x)-coordinates of points on each horizontal line.
    list_ver_lines : list of 2D arrays
        List of the (y,x)-coordinates of points on each vertical line.
    xcenter : float
        Center of distortion in x-direction.
    ycenter : float
        Center of distortion in y-direction.
    num_fact : int
        Number of the factors of polynomial.
    optimizing : bool, optional
        Apply optimization if True.
    threshold : float
        To determine if there are missing lines. Larger is less sensitive.

    Returns
    -------
    list_fact : list of float
        Coefficients of the polynomial.
    """
    expo = np.arange(_clamp_num_fact(num_fact), dtype=np.int16)
    rows, values = [], []
    for radius, term, uc in _factor_rows(list_hor_lines, list_ver_lines, xcenter, ycenter, optimizing, threshold):
        if uc != 0.0:
            factor = uc / term
            keep = factor != 0.0
            rows.append(np.power(radius[keep][:, None], expo[None, :]))
            values.append(factor[keep])
    return _solve(rows, values)


def calc_coef_backward_from_forward(list_hor_lines, list_ver_lines, xcenter, ycenter, num_fact, optimizing=False, threshold=0.3):
    """
    The forward model first, then the backward model as its reversal over the same points: ``B(F(rd) rd) = 1 / F(rd)``.

    Parameters
    ----------
    list_hor_lines : list of 2D arrays
        List of the (y,x)-coordinates of points on each horizontal line.
    list_ver_lines : list of 2D arrays
        List of the (y,x)-coordinates of points on each vertical line.
    xcenter : float
        Center of distortion in x-direction.
    ycenter : float
        Center of distortion in y-direction.
    num_fact : int
        Number of the factors of polynomial.
    optimizing : bool, optional
        Apply optimization if True.
    threshold : float
        To determine if there are missing lines. Larger is less sensitive.

    Returns
    -------
    list_ffact : list of floats
        Polynomial coefficients of the forward model.
    list_bfact : list of floats
        Polynomial coefficients of the backward model.
    """
    num_fact = _clamp_num_fact(num_fact)
    list_ffact = np.asarray(calc_coef_forward(list_hor_lines, list_ver_lines, xcenter, ycenter, num_fact, optimizing=optimizing,
                                              threshold=threshold), dtype=np.float64)
    expo = np.arange(num_fact, dtype=np.int16)
    rows, values = [], []
    for line in _para_fit_hor(list_hor_lines, xcenter, ycenter)[1] + _para_fit_ver(list_ver_lines, xcenter, ycenter)[1]:
        line = np.asarray(line, dtype=np.float64)
        yd, xd = line[:, 0], line[:, 1]
        radius = np.sqrt(xd * xd + yd * yd)
        forward = np.sum(list_ffact[None, :] * np.power(radius[:, None], expo[None, :]), axis=1)
        keep = forward != 0.0
        rows.append(np.power((forward[keep] * radius[keep])[:, None], expo[None, :]))
        values.append(1 / forward[keep])
    return list_ffact, _solve(rows, values)


def find_cod_bailey(list_hor_lines, list_ver_lines, iteration=2):
    """
    Centre of distortion by Bailey's approach (https://www-ist.massey.ac.nz/dbailey/sprg/pdfs/2002_IVCNZ_59.pdf): the curvature of
    the lines is linear in their intercept and vanishes at the centre.  Starts from :func:`find_cod_coarse`.

    Parameters
    ----------
    list_hor_lines : list of 2D-arrays
        List of the (y,x)-coordinates of points on each horizontal line.
    list_ver_lines : list of 2D-arrays
        List of the (y,x)-coordinates of points on each vertical line.
    iteration : int
        Number of further updates after the first.

    Returns
    -------
    xcenter : float
        Center of distortion in x-direction.
    ycenter : float
        Center of distortion in y-direction.
    """
    xcenter, ycenter = find_cod_coarse(list_hor_lines, list_ver_lines)
    for _ in range(iteration + 1):
        coef_hor = _para_fit_hor(list_hor_lines, xcenter, ycenter)[0]
        coef_ver = _para_fit_ver(list_ver_lines, xcenter, ycenter)[0]
        a1, b1 = np.polyfit(coef_hor[:, 2], coef_hor[:, 0], 1)[0:2]
        a2, b2 = np.polyfit(coef_ver[:, 2], coef_ver[:, 0], 1)[0:2]
        xcenter = xcenter - b2 / a2
        ycenter = ycenter - b1 / a1
    return xcenter, ycenter


# --------------------------------------------------------------------------- regenerated grids

def _common_slope(inter_hor, slope_hor, inter_ver, slope_ver, limit):
    """The slope both directions share at a zero intercept: each direction's slopes are fitted linearly against its intercepts
    (the vertical ones negated), and the two fits are solved for their common value; their mean where they are parallel."""
    ah, bh = np.polyfit(inter_hor, slope_hor, 1)[0:2]
    av, bv = np.polyfit(inter_ver, -slope_ver, 1)[0:2]
    if np.abs(ah - av) >= limit:
        return (ah * bv - av * bh) / (ah - av)
    return (bh + bv) * 0.5


def _generate_non_perspective_parabola_coef(list_hor_lines, list_ver_lines):
    """
    Parabola tables with the effect of perspective taken out: one common linear term, and the direction with the smaller line
    distance rescaled to the other's.  The tables refer to the centre that is returned with them, not to (0, 0).

    Parameters
    ----------
    list_hor_lines, list_ver_lines : list of 2D-arrays
        (y, x) coordinates of the points of each line.

    Returns
    -------
    list_coef_hor, list_coef_ver : array_like
        The corrected float32 tables.
    xcenter, ycenter : float
        Centre of distortion (:func:`find_cod_bailey`).
    """
    num_hline, num_vline = len(list_hor_lines), len(list_ver_lines)
    xcenter, ycenter = find_cod_bailey(list_hor_lines, list_ver_lines)
    coef_hor = _para_fit_hor(list_hor_lines, xcenter, ycenter)[0]
    coef_ver = _para_fit_ver(list_ver_lines, xcenter, ycenter)[0]
    b0 = _common_slope(coef_hor[:, 2], coef_hor[:, 1], coef_ver[:, 2], coef_ver[:, 1], 0.001)
    coef_hor[:, 1] = b0
    coef_ver[:, 1] = -b0
    num_use = min(3, num_hline // 2 - 1, num_vline // 2 - 1)
    dist = []
    for table, num_line in ((coef_hor, num_hline), (coef_ver, num_vline)):
        pos = np.argmax(np.abs(np.diff(np.sign(table[:, 0])))) + 1
        first, last = _middle_lines(pos, num_use, num_line)
        dist.append(np.mean(np.abs(np.diff(table[first:last, 2]))))
    dist_hor, dist_ver = dist
    if dist_hor > dist_ver:
        coef_ver[:, 2] = coef_ver[:, 2] * dist_hor / dist_ver
        coef_ver[:, 0] = coef_ver[:, 0] * dist_hor / dist_ver
    else:
        coef_hor[:, 2] = coef_hor[:, 2] * dist_ver / dist_hor
        coef_hor[:, 0] = coef_hor[:, 0] * dist_ver / dist_hor
    return coef_hor, coef_ver, xcenter, ycenter


def _find_cross_point_between_parabolas(para_coef_hor, para_coef_ver):
    """
    Where a horizontal parabola (``y = a x**2 + b x + c``) and a vertical one (``x = a y**2 + b y + c``) cross: ``fsolve`` from (0, 0).

    Returns
    -------
    x, y : floats
    """
    a1, b1, c1 = para_coef_hor[0:3]
    a2, b2, c2 = para_coef_ver[0:3]

    def residual(point):
        x, y = point
        return a1 * x ** 2 + b1 * x + c1 - y, a2 * y ** 2 + b2 * y + c2 - x

    x, y = optimize.fsolve(residual, (0, 0))
    return x, y


def regenerate_grid_points_parabola(list_hor_lines, list_ver_lines, perspective=False, find_center=False):
    """
    Regenerate the grid points as the cross points of the parabolas fitted to the horizontal and to the vertical lines.

    Parameters
    ----------
    list_hor_lines : list of 2D-arrays
        List of the (y,x)-coordinates of points on each horizontal line.
    list_ver_lines : list of 2D-arrays
        List of the (y,x)-coordinates of points on each vertical line.
    perspective : bool, optional
        If True, apply perspective correction and set "find_center" to True.
    find_center : bool, optional
        If True, the parabolas are fitted about the centre of distortion (:func:`find_cod_bailey`) and the points moved back.

    Returns
    -------
    new_hor_lines : array_like
        float32 ``(H, V, 2)``: the (y,x)-coordinates of the points of each horizontal line.
    new_ver_lines : array_like
        float32 ``(V, H, 2)``: the same points, line by vertical line.
    """
    if perspective is True:
        coef_hor, coef_ver, xcenter, ycenter = _generate_non_perspective_parabola_coef(list_hor_lines, list_ver_lines)
    else:
        if find_center is True:
            xcenter, ycenter = find_cod_bailey(list_hor_lines, list_ver_lines)
        else:
            xcenter, ycenter = 0.0, 0.0
        coef_hor = _para_fit_hor(list_hor_lines, xcenter, ycenter)[0]
        coef_ver = _para_fit_ver(list_ver_lines, xcenter, ycenter)[0]
    new_hor_lines = np.zeros((len(coef_hor), len(coef_ver), 2), dtype=np.float32)
    for i, para_hor in enumerate(coef_hor):
        for j, para_ver in enumerate(coef_ver):
            x, y = _find_cross_point_between_parabolas(para_hor, para_ver)
            new_hor_lines[i, j] = (y + ycenter, x + xcenter)
    return new_hor_lines, np.ascontiguousarray(new_hor_lines.transpose(1, 0, 2))


def _generate_linear_coef(list_hor_lines, list_ver_lines, xcenter=0.0, ycenter=0.0):
    """
    Straight-line fits: ``y = a x + b`` of the horizontal lines and ``x = a y + b`` of the vertical ones, about ``(xcenter, ycenter)``.

    Returns
    -------
    list_coef_hor, list_coef_ver : array_like
        float32 tables ``(number of lines, 2)`` of ``(a, b)``.
    """
    coef_hor = np.zeros((len(list_hor_lines), 2), dtype=np.float32)
    coef_ver = np.zeros((len(list_ver_lines), 2), dtype=np.float32)
    for i, item in enumerate(list_hor_lines):
        line = np.asarray(item)
        coef_hor[i] = np.polyfit(line[:, 1] - xcenter, line[:, 0] - ycenter, 1)
    for i, item in enumerate(list_ver_lines):
        line = np.asarray(item)
        coef_ver[i] = np.polyfit(line[:, 0] - ycenter, line[:, 1] - xcenter, 1)
    return coef_hor, coef_ver


def _find_cross_point_between_lines(line_coef_hor, line_coef_ver):
    """
    Where a horizontal line (``y = a x + b``) and a vertical one (``x = a y + b``) cross.

    Returns
    -------
    x, y : floats
    """
    a1, b1 = line_coef_hor
    a2, b2 = line_coef_ver
    y = (a1 * b2 + b1) / (1.0 - a1 * a2)
    x = a2 * y + b2
    return x, y


def _cross_grid(coef_hor, coef_ver):
    """Every horizontal line crossed with every vertical one (the expression above on broadcast columns): float32 (H, V, 2) of
    (y, x), and the same points as (V, H, 2)."""
    coef_hor, coef_ver = np.asarray(coef_hor), np.asarray(coef_ver)
    grid = np.zeros((len(coef_hor), len(coef_ver), 2), dtype=np.float32)
    if grid.size:
        x, y = _find_cross_point_between_lines((coef_hor[:, 0][:, None], coef_hor[:, 1][:, None]),
                                               (coef_ver[:, 0][None, :], coef_ver[:, 1][None, :]))
        grid[:, :, 0], grid[:, :, 1] = y, x
    return grid, np.ascontiguousarray(grid.transpose(1, 0, 2))


def _calc_undistor_intercept_perspective(list_hor_lines, list_ver_lines, equal_dist=True, scale="mean", optimizing=True):
    """
    Intercepts of the lines with the perspective taken out: equally spaced from the middle line.

    Parameters
    ----------
    list_hor_lines, list_ver_lines : list of 2D-arrays
        (y, x) coordinates of the points of each line.
    equal_dist : bool
        Use the condition that lines are equidistant if True.
    scale : {'mean', 'median', 'min', 'max', float}
        Scale option for the undistorted grid.
    optimizing : bool
        Apply optimization for finding line-distance if True.

    Returns
    -------
    u_intercept_hor, u_intercept_ver : array_like
        float32 intercepts of the horizontal and the vertical lines.
    """
    coef_hor, coef_ver = _generate_linear_coef(list_hor_lines, list_ver_lines)
    num_hline, num_vline = len(list_hor_lines), len(list_ver_lines)
    pos_hor, pos_ver = num_hline // 2, num_vline // 2
    num_use = min(np.clip(num_hline // 2 - 1, 1, None), np.clip(num_vline // 2 - 1, 1, None))
    reduce = {"max": np.max, "min": np.min, "median": np.median}.get(scale if isinstance(scale, str) else None, np.mean)
    dist = []
    for table, pos, num_line in ((coef_hor, pos_hor, num_hline), (coef_ver, pos_ver, num_vline)):
        first, last = _middle_lines(pos, num_use, num_line)
        spacing = reduce(np.abs(np.diff(table[first:last, 1])))
        if reduce is np.mean and isinstance(scale, float):
            spacing = scale * spacing
        if optimizing is True:
            spacing = _fit_spacing(_perspective_spacing_cost, spacing, pos, table[:, 1])
        dist.append(spacing)
    dist_hor, dist_ver = dist
    if equal_dist is True:
        if isinstance(scale, str) and scale == "max":
            dist_hor = dist_ver = max(dist_hor, dist_ver)
        elif isinstance(scale, str) and scale == "min":
            dist_hor = dist_ver = min(dist_hor, dist_ver)
        else:
            dist_hor = dist_ver = (dist_hor + dist_ver) * 0.5
    u_intercept_hor = np.zeros(num_hline, dtype=np.float32)
    u_intercept_ver = np.zeros(num_vline, dtype=np.float32)
    for i in range(num_hline):
        u_intercept_hor[i] = (i - pos_hor) * dist_hor + coef_hor[pos_hor, 1]
    for i in range(num_vline):
        u_intercept_ver[i] = (i - pos_ver) * dist_ver + coef_ver[pos_ver, 1]
    return u_intercept_hor, u_intercept_ver


def regenerate_grid_points_linear(list_hor_lines, list_ver_lines, is_coef=False):
    """
    Regenerate the grid points as the cross points of the straight lines fitted to the horizontal and to the vertical lines.

    Parameters
    ----------
    list_hor_lines : list of 2D-arrays
        List of the (y, x)-coordinates of points on each horizontal line,
        or list of linear fitted coefficients of lines (if is_coef=True).
    list_ver_lines : list of 2D-arrays
        List of the (y, x)-coordinates of points on each vertical line,
        or list of linear fitted coefficients of lines (if is_coef=True).
    is_coef : bool, optional
        Whether the input is linear fitted coefficients of lines.
        If False, linear fitting will be applied to the input lines.

    Returns
    -------
    new_hor_lines : array_like
        float32 ``(H, V, 2)``: the (y,x)-coordinates of the points of each horizontal line.
    new_ver_lines : array_like
        float32 ``(V, H, 2)``: the same points, line by vertical line.
    """
    if is_coef is not True:
        coef_hor, coef_ver = _generate_linear_coef(list_hor_lines, list_ver_lines)
    else:
        coef_hor, coef_ver = list_hor_lines, list_ver_lines
    return _cross_grid(coef_hor, coef_ver)


def generate_undistorted_perspective_lines(list_hor_lines, list_ver_lines, equal_dist=True, scale="mean", optimizing=True):
    """
    The grid the perspective lines come from: parallel, equally spaced lines with the slope both directions share.

    Parameters
    ----------
    list_hor_lines : list of 2D-arrays
        List of the (y,x)-coordinates of points on each horizontal line.
    list_ver_lines : list of 2D-arrays
        List of the (y,x)-coordinates of points on each vertical line.
    equal_dist : bool
        Use the condition that lines are equidistant if True.
    scale : {'mean', 'median', 'min', 'max', float}
        Scale option for the undistorted grid.
    optimizing : bool
        Apply optimization for finding line-distance if True.

    Returns
    -------
    list_uhor_lines : array_like
        float32 ``(H, V, 2)``: (y,x)-coordinates of the points on the undistorted horizontal lines.
    list_uver_lines : array_like
        float32 ``(V, H, 2)``: the same points on the undistorted vertical lines.
    """
    coef_hor, coef_ver = _generate_linear_coef(list_hor_lines, list_ver_lines)
    a0 = _common_slope(coef_hor[:, 1], coef_hor[:, 0], coef_ver[:, 1], coef_ver[:, 0], 0.0001)
    coef_uhor, coef_uver = np.copy(coef_hor), np.copy(coef_ver)
    coef_uhor[:, 0] = a0
    coef_uver[:, 0] = -a0
    coef_uhor[:, 1], coef_uver[:, 1] = _calc_undistor_intercept_perspective(list_hor_lines, list_ver_lines, equal_dist, scale,
                                                                            optimizing)
    return _cross_grid(coef_uhor, coef_uver)


def generate_source_target_perspective_points(list_hor_lines, list_ver_lines, equal_dist=True, scale="mean", optimizing=True):
    """
    Pairs of points for :func:`calc_perspective_coefficients`: the cross points of the fitted straight lines (source, distorted) and
    the corresponding points of the undistorted grid (target).

    Parameters
    ----------
    list_hor_lines : list of 2D-arrays
        List of the (y,x)-coordinates of points on each horizontal line.
    list_ver_lines : list of 2D-arrays
        List of the (y,x)-coordinates of points on each vertical line.
    equal_dist : bool
        Use the condition that lines are equidistant if True.
    scale : {'mean', 'median', 'min', 'max', float}
        Scale option for the undistorted grid.
    optimizing : bool
        Apply optimization for finding line-distance if True.

    Returns
    -------
    source_points : array_like
        ``(H * V, 2)`` (y,x)-coordinates of distorted points.
    target_points : array_like
        ``(H * V, 2)`` (y,x)-coordinates of undistorted points.
    """
    hor_slines, ver_slines = regenerate_grid_points_linear(list_hor_lines, list_ver_lines)
    hor_tlines, _ = generate_undistorted_perspective_lines(hor_slines, ver_slines, equal_dist, scale, optimizing)
    return hor_slines.reshape(-1, 2).copy(), hor_tlines.reshape(-1, 2).copy()


def generate_4_source_target_perspective_points(points, input_order="yx", equal_dist=False, scale="mean"):
    """
    The rectangle four perspective-distorted points come from.  The points are sorted into top-left, top-right, bottom-left and
    bottom-right; the rectangle has the mean slope and the mean (or smallest, largest, scaled) side lengths of the quadrilateral.

    Parameters
    ----------
    points : list of 1D-arrays
        List of the coordinates of 4 perspective-distorted points.
    input_order : {'yx', 'xy'}
        Order of the coordinates of input-points.
    equal_dist : bool
        Use the condition that the rectangular making of 4-points is square if
        True.
    scale : {'mean', 'min', 'max', float}
        Scale option for the undistorted points.

    Returns
    -------
    source_points : list of 1D-arrays
        List of the (y,x)-coordinates of distorted points.
    target_points : list of 1D-arrays
        List of the (y,x)-coordinates of undistorted points.
    """
    points = np.asarray(points, dtype=np.float32)
    if input_order == "xy":
        points = np.fliplr(points)
    if len(points) != 4:
        raise ValueError("Input must be a list of 4 points!!!")
    by_row = points[points[:, 0].argsort()]
    top, bottom = by_row[0:2], by_row[-2:]
    (y1, x1), (y2, x2) = top[top[:, 1].argsort()]
    (y3, x3), (y4, x4) = bottom[bottom[:, 1].argsort()]
    source_points = np.asarray([[y1, x1], [y2, x2], [y3, x3], [y4, x4]])
    # the two horizontal sides as y = a x + b, the two vertical ones as x = a y + b; their means
    a12 = (y1 - y2) / (x1 - x2)
    b12 = y1 - a12 * x1
    a34 = (y3 - y4) / (x3 - x4)
    b34 = y3 - a34 * x3
    ah, bh = (a12 + a34) * 0.5, (b12 + b34) * 0.5
    a13 = (x1 - x3) / (y1 - y3)
    b13 = x1 - a13 * y1
    a24 = (x2 - x4) / (y2 - y4)
    b24 = x2 - a24 * y2
    av, bv = (a13 + a24) * 0.5, (b13 + b24) * 0.5
    a0 = np.sign(ah) * (np.abs(ah) + np.abs(av)) * 0.5
    dist12 = np.sqrt((x1 - x2) ** 2 + (y1 - y2) ** 2)
    dist13 = np.sqrt((x1 - x3) ** 2 + (y1 - y3) ** 2)
    dist24 = np.sqrt((x2 - x4) ** 2 + (y2 - y4) ** 2)
    dist34 = np.sqrt((x3 - x4) ** 2 + (y3 - y4) ** 2)
    if isinstance(scale, str) and scale in ("max", "min"):
        pick = max if scale == "max" else min
        dist_h, dist_v = pick(dist12, dist34), pick(dist13, dist24)
        if equal_dist is True:
            dist_h = dist_v = pick(dist_v, dist_h)
    else:
        dist_h = (dist12 + dist34) * 0.5
        dist_v = (dist13 + dist24) * 0.5
        if isinstance(scale, float):
            dist_h = dist_h * scale
            dist_v = dist_v * scale
        if equal_dist is True:
            dist_h = dist_v = (dist_v + dist_h) * 0.5
    dist_h, dist_v = dist_h * 0.5, dist_v * 0.5
    # the rectangle's sides: y = a0 x + b1, b2 and x = -a0 y + b3, b4, half a side either way of the mean lines
    b1 = bh - np.abs(dist_v / np.cos(np.arctan(a0)))
    b2 = bh + np.abs(dist_v / np.cos(np.arctan(a0)))
    b3 = bv - np.abs(dist_h / np.cos(np.arctan(a0)))
    b4 = bv + np.abs(dist_h / np.cos(np.arctan(a0)))
    corners = []
    for b_hor, b_ver in ((b1, b3), (b1, b4), (b2, b3), (b2, b4)):
        y = (a0 * b_ver + b_hor) / (1.0 + a0 ** 2)
        corners.append([y, -a0 * y + b_ver])
    return source_points, np.asarray(corners)


def calc_perspective_coefficients(source_points, target_points, mapping="backward"):
    """
    The eight coefficients of the homography that maps source points to target points (https://doi.org/10.1016/S0262-8856(98)00183-8),
    by least squares over all pairs.  Points are in (y,x)-order, as everywhere in the module; the coefficients are in the
    (x, y) convention ``post.correct_perspective_image`` / ``_line`` read.

    Parameters
    ----------
    source_points : array_like
        List of the (y,x)-coordinates of distorted points.
    target_points : array_like
        List of the (y,x)-coordinates of undistorted points.
    mapping : {'backward', 'forward'}
        To select mapping direction.

    Returns
    -------
    array_like
        1D array of 8 coefficients.
    """
    if mapping == "forward":
        s_points = np.fliplr(np.asarray(source_points))
        t_points = np.fliplr(np.asarray(target_points))
    else:
        s_points = np.fliplr(np.asarray(target_points))
        t_points = np.fliplr(np.asarray(source_points))
    num = min(len(s_points), len(t_points))
    design = np.zeros((2 * num, 8), dtype=np.float64) if num else np.asarray([], dtype=np.float64)
    if num:
        sx, sy, tx, ty = s_points[:num, 0], s_points[:num, 1], t_points[:num, 0], t_points[:num, 1]
        design[0::2, 0], design[0::2, 1], design[0::2, 2] = sx, sy, 1
        design[0::2, 6], design[0::2, 7] = -tx * sx, -tx * sy
        design[1::2, 3], design[1::2, 4], design[1::2, 5] = sx, sy, 1
        design[1::2, 6], design[1::2, 7] = -ty * sx, -ty * sy
    target = np.asarray(t_points, dtype=np.float64).flatten()
    return np.linalg.lstsq(design, target, rcond=1e-64)[0]


def update_center(list_lines, xcenter, ycenter):
    """
    Move the points of lines to another origin: ``(y + ycenter, x + xcenter)``.

    Parameters
    ----------
    list_lines : list of 2D-arrays
        List of the (y,x)-coordinates of points on lines.
    xcenter : float
        X-origin of the coordinate system.
    ycenter : float
        Y-origin of the coordinate system.

    Returns
    -------
        list of 2D-arrays.
    """
    updated_lines = []
    for item in list_lines:
        line = np.asarray(item)
        if len(line) == 0:
            updated_lines.append(np.asarray([]))
            continue
        updated_lines.append(np.stack((line[:, 0] + ycenter, line[:, 1] + xcenter), axis=1))
    return updated_lines


# --------------------------------------------------------------------------- perspective effect on curved lines

def _representative_line(table, chosen, method):
    """(b, c) of the straight line that stands for the chosen parabolas: their mean or median, or the line of the parabola with the
    weakest ("min") or strongest ("max") curvature."""
    a_val, b_val, c_val = table[chosen, 0], table[chosen, 1], table[chosen, 2]
    if method == "median":
        return np.median(b_val), np.median(c_val)
    if method in ("max", "min"):
        order = a_val.argsort()
        opens_positive = a_val[order][0] > 0
        pos = order[-1] if opens_positive == (method == "max") else order[0]
        return b_val[pos], c_val[pos]
    return np.mean(b_val), np.mean(c_val)


def _perspective_effect_model(list_hor_lines, list_ver_lines, xcenter, ycenter, method, scale):
    """The lines shifted to the centre and the eight forward coefficients that take the perspective effect out of them."""
    coef_hor, hor_lines = _para_fit_hor(list_hor_lines, xcenter, ycenter)
    coef_ver, ver_lines = _para_fit_ver(list_ver_lines, xcenter, ycenter)
    if len(coef_hor) < 2:
        raise ValueError("Need at least 2 horizontal lines!!!")
    if len(coef_ver) < 2:
        raise ValueError("Need at least 2 vertical lines!!!")
    found = []
    for table, positive, direction in ((coef_hor, True, "upwards"), (coef_hor, False, "downwards"),
                                       (coef_ver, True, "rightwards"), (coef_ver, False, "leftwards")):
        chosen = np.where(table[:, 0] > 0 if positive else table[:, 0] < 0)[0]
        if len(chosen) == 0:
            raise ValueError("Input error!!! No curved line open %s !!!" % direction)
        found.append(list(_representative_line(table, chosen, method)))
    hor1, hor2, ver1, ver2 = found
    corners = []
    for hor, ver in ((hor1, ver1), (hor1, ver2), (hor2, ver1), (hor2, ver2)):
        x, y = _find_cross_point_between_lines(hor, ver)
        corners.append([y, x])
    source_points, target_points = generate_4_source_target_perspective_points(np.asarray(corners), input_order="yx",
                                                                               equal_dist=False, scale=scale)
    return hor_lines, ver_lines, calc_perspective_coefficients(source_points, target_points, mapping="forward")


def correct_perspective_effect(list_hor_lines, list_ver_lines, xcenter, ycenter, method="mean", scale="mean"):
    """
    Correct perspective effect of radial-distorted grid lines.  Four straight lines stand for the parabolas that open up, down,
    right and left; their four cross points and the rectangle those come from give a homography, which is applied to every point
    (on the GPU: ``post.correct_perspective_line``).

    Parameters
    ----------
    list_hor_lines : list of 2D-arrays
        List of the (y,x)-coordinates of points on each horizontal line.
    list_ver_lines : list of 2D-arrays
        List of the (y,x)-coordinates of points on each vertical line.
    xcenter : float
        Center of radial distortion in x-direction.
    ycenter : float
        Center of radial distortion in y-direction.
    method : {'mean', 'median', 'min', 'max'}
        Method to find 4 representative straight lines of parabolas with
        opposite curves in each direction. 4 intersection points of these lines
        are used to calculate perspective coefficients.
    scale : {'mean', 'median', 'min', 'max', float}
        Scale option for perspective-corrected grid.

    Returns
    -------
    corr_hor_lines : list of 2D-arrays
        List of the corrected (y,x)-coordinates of points on each horizontal
        line.
    corr_ver_lines : list of 2D-arrays
        List of the corrected (y,x)-coordinates of points on each vertical line.
    """
    hor_lines, ver_lines, pers_coef = _perspective_effect_model(list_hor_lines, list_ver_lines, xcenter, ycenter, method, scale)
    corr_hor_lines = post.correct_perspective_line(hor_lines, pers_coef)
    corr_ver_lines = post.correct_perspective_line(ver_lines, pers_coef)
    return update_center(corr_hor_lines, xcenter, ycenter), update_center(corr_ver_lines, xcenter, ycenter)


# --------------------------------------------------------------------------- vanishing points

def _find_cross_point_between_parabolas_same_direction(para_coef1, para_coef2):
    """
    Where two parabolas of the same orientation cross: the roots of ``(a1 - a2) t**2 + (b1 - b2) t + (c1 - c2)``.

    Parameters
    ----------
    para_coef1, para_coef2 : tuple
        Coefficients (a, b, c), highest order first.

    Returns
    -------
    tuple of floats, or None
        The abscissas of the cross points (x for horizontal parabolas, y for vertical ones); None where the roots are complex.
    """
    roots = np.roots([para_coef1[0] - para_coef2[0], para_coef1[1] - para_coef2[1], para_coef1[2] - para_coef2[2]])
    if np.iscomplexobj(roots):
        return None
    return roots


def _cross_points_of_pairs(pairs):
    """[abscissa, ordinate] of the cross points of each pair of parabolas: the first root on the first parabola, the second on the
    second."""
    found = []
    for first, second in pairs:
        roots = _find_cross_point_between_parabolas_same_direction(first, second)
        if roots is not None:
            t1, t2 = roots
            found.append([t1, first[0] * t1 ** 2 + first[1] * t1 + first[2]])
            found.append([t2, second[0] * t2 ** 2 + second[1] * t2 + second[2]])
    return found


def _opposite_pairs(table):
    """Parabolas opening one way paired with those opening the other way, each side from the weakest curvature up."""
    positive, negative = table[table[:, 0] > 0], table[table[:, 0] < 0]
    positive = positive[np.argsort(np.abs(positive[:, 0]))]
    negative = negative[np.argsort(np.abs(negative[:, 0]))]
    return list(zip(positive, negative))


def _straightest_pairs(table):
    """Every parabola paired with the one of least curvature."""
    pos_min = np.argmin(np.abs(table[:, 0]))
    return [(table[i], table[pos_min]) for i in np.delete(np.arange(len(table)), pos_min)]


def _center_from_vanishing_points(list_hor_lines, list_ver_lines, pairing):
    """The cross points of the paired horizontal parabolas lie on one line, those of the vertical ones on another; the centre is
    where the two lines cross.  Bailey's centre where a direction yields no more than two points."""
    coef_hor, hor_lines = _para_fit_hor(list_hor_lines, 0, 0)
    coef_ver, ver_lines = _para_fit_ver(list_ver_lines, 0, 0)
    xy_hlist = _cross_points_of_pairs(pairing(coef_hor))
    if len(xy_hlist) > 2:
        yx_vlist = _cross_points_of_pairs(pairing(coef_ver))
        if len(yx_vlist) > 2:
            xy_hlist, yx_vlist = np.asarray(xy_hlist), np.asarray(yx_vlist)
            a1, b1 = np.polyfit(xy_hlist[:, 0], xy_hlist[:, 1], 1)[:2]
            a2, b2 = np.polyfit(yx_vlist[:, 0], yx_vlist[:, 1], 1)[:2]
            ycenter = (a1 * b2 + b1) / (1.0 - a1 * a2)
            xcenter = a2 * ycenter + b2
            return xcenter, ycenter
    return find_cod_bailey(hor_lines, ver_lines)


def find_center_based_vanishing_points(list_hor_lines, list_ver_lines):
    """
    Find the center of distortion (COD) using vanishing points formed by the intersections of parabolas with opposite curves in
    the horizontal and vertical directions.  Valid only for barrel distortion.

    Parameters
    ----------
    list_hor_lines : list of 2D-arrays
        List of (y,x)-coordinates of points on each horizontal line.
    list_ver_lines : list of 2D-arrays
        List of (y,x)-coordinates of points on each vertical line.

    Returns
    -------
    xcenter : float
        Center of distortion in the x-direction.
    ycenter : float
        Center of distortion in the y-direction.
    """
    return _center_from_vanishing_points(list_hor_lines, list_ver_lines, _opposite_pairs)


def _find_center_based_vanishing_points_2nd_way(list_hor_lines, list_ver_lines):
    """The same with every parabola crossed with the line of minimum curvature of its direction."""
    return _center_from_vanishing_points(list_hor_lines, list_ver_lines, _straightest_pairs)


def _perspective_lines_host(list_lines, list_coef):
    """The homography on the points of lines in NumPy, in the operation order of the reference's ``correct_perspective_line`` -- for
    lines that stay inside this module (``post.correct_perspective_line`` gives the same bits through the device)."""
    c1, c2, c3, c4, c5, c6, c7, c8 = list_coef
    mapped = []
    for item in list_lines:
        line = np.asarray(item)
        x, y = line[:, 1], line[:, 0]
        xn = (c1 * x + c2 * y + c3) / (c7 * x + c8 * y + 1.0)
        yn = (c4 * x + c5 * y + c6) / (c7 * x + c8 * y + 1.0)
        mapped.append(np.stack((yn, xn), axis=1))
    return mapped


def find_center_based_vanishing_points_iteration(list_hor_lines, list_ver_lines, iteration=2, method="mean"):
    """
    Find the center of distortion (COD) using vanishing points formed by the intersections of parabolas with lines of minimum
    curvature in the horizontal and vertical directions, the perspective effect taken out of the lines before each further round.
    More robust than the others when there's significant perspective distortion.

    The corrected lines of each round never leave the function, so they are mapped on the host and no device is needed; the
    arithmetic is that of :func:`correct_perspective_effect`.

    Parameters
    ----------
    list_hor_lines : list of 2D-arrays
        List of (y,x)-coordinates of points on each horizontal line.
    list_ver_lines : list of 2D-arrays
        List of (y,x)-coordinates of points on each vertical line.
    iteration : int, optional
        Iteration number
    method : {'mean', 'median', 'min', 'max'}
        Method to find 4 representative straight lines of parabolas with
        opposite curves in each direction. 4 intersection points of these lines
        are used to correct perspective distortion.

    Returns
    -------
    xcenter : float
        Center of distortion in the x-direction.
    ycenter : float
        Center of distortion in the y-direction.
    """
    xcenter, ycenter = _find_center_based_vanishing_points_2nd_way(list_hor_lines, list_ver_lines)
    for _ in range(iteration):
        hor_lines, ver_lines, pers_coef = _perspective_effect_model(list_hor_lines, list_ver_lines, xcenter, ycenter, method, "mean")
        # (moving the corrected lines back to the image's origin and shifting them to the centre again, as the reference does: the
        # two roundings are part of the result)
        hor_lines = _para_fit_hor(update_center(_perspective_lines_host(hor_lines, pers_coef), xcenter, ycenter), xcenter, ycenter)[1]
        ver_lines = _para_fit_ver(update_center(_perspective_lines_host(ver_lines, pers_coef), xcenter, ycenter), xcenter, ycenter)[1]
        xshift, yshift = _find_center_based_vanishing_points_2nd_way(hor_lines, ver_lines)
        xcenter += xshift
        ycenter += yshift
    return xcenter, ycenter
