"""The rest of the dot-pattern route of ``discorpy.prep.preprocessing`` (reference ``preprocessing.py:274-813``): from a binary dot image to
the grouped lines of dot centroids.  Every name is imported into :mod:`discorpy_amd.prep.preprocessing` (its ``DOT_GRID``), so the
reference's scripts run on ``import discorpy_amd.prep.preprocessing as prep`` from ``binarization`` to ``remove_residual_dots_ver``.

* :func:`radon_padded`   ``skimage.transform.radon(image, theta, circle=False)`` restated from its documentation (``dcp_radon_padded_2d``)
* :func:`calc_size_distance`, :func:`select_dots_based_ratio`, :func:`calc_hor_slope`, :func:`calc_ver_slope`   the reference's
  functions: same names, arguments and defaults
* :func:`group_dots_hor_lines`, :func:`group_dots_ver_lines`, :func:`remove_residual_dots_hor`, :func:`remove_residual_dots_ver`
  host NumPy with the reference's signatures, messages and return shapes; only an image argument touches the GPU

Three pieces of work are HIP kernels (``csrc/dotgrid_kernels.hip``; ``DESIGN.md``, "Dot grid"); there is no CPU path for them:

``dcp_radon_padded_2d``   The H x W image sits in a square of zeros of side ``S = int(ceil(sqrt(2) * max(H, W)))`` with its first element
at ``(S // 2 - H // 2, S // 2 - W // 2)``; that square is transformed as :func:`discorpy_amd.prep.linepattern.radon` transforms its plane
(same angle table, made for side ``S``; bilinear interpolation between ``floor`` and ``ceil``; 0.0 outside; float64; rows added in
ascending order) but without the circle.  No padded plane is made: a tap outside the image's rectangle is 0.0, one inside is the element
(a NaN included), read through the row stride.  The result equals the NumPy restatement ``tests/helpers/radon_padded_reference.py`` bit
for bit.  Agreement with scikit-image itself is UNVERIFIED: it is not installed where this was written.

``dcp_nearest_sq_dists``   The four smallest SQUARED distances ``(y_i - y_j) * (y_i - y_j) + (x_i - x_j) * (x_i - x_j)`` from every
centroid to all centroids (itself included), the operations NumPy performs for the reference's expression; the root is taken in NumPy.
The distances behind ``calc_size_distance`` and ``select_dots_based_distance`` therefore equal the reference's bit for bit.

``dcp_box_moments_2d``   Count and first and second coordinate sums of every nonzero pixel inside a dot's bounding box -- per box, not per
label: the reference measures ``mat[box]``, so a neighbour's pixels that reach into the box count -- as int64.  The axis lengths
of :func:`select_dots_based_ratio` come from these exact integers (:func:`_axis_lengths`): the eigenvalues of the inertia tensor
``mu / mu00`` that the documentation of ``skimage.measure.regionprops`` defines ``major_axis_length`` and ``minor_axis_length`` by.  That
link is by construction and UNVERIFIED; the independent check is ``tests/helpers/regionprops_reference.py`` (float64 central moments,
``np.linalg.eigvalsh``).  Stated difference: a dot whose minor axis is 0 has ``val = inf`` and is dropped without a warning; what
scikit-image does there is unverified.

Out of scope: ``calculate_threshold``, the parabola masks (``make_parabola_mask``, ``remove_points_using_parabola_mask``),
``rotate_points``, ``remove_subset_points``, the polyfit-based grouping (``group_dots_hor_lines_based_polyfit`` /
``group_dots_ver_lines_based_polyfit``), ``get_points_dot_pattern(binarize=True)`` (it keeps raising) and everything of ``proc``.
"""
import math

import numpy as np

from .. import _ffi as F
from . import preprocessing as _p

__all__ = ["radon_padded", "calc_size_distance", "select_dots_based_ratio", "calc_hor_slope", "calc_ver_slope", "group_dots_hor_lines",
           "group_dots_ver_lines", "remove_residual_dots_hor", "remove_residual_dots_ver"]

NEAREST_MAX_POINTS = 1 << 20          # dcp_nearest_sq_dists


def _padded_side(height, width):
    """Side of the square of zeros an H x W image is embedded in: ``ceil(sqrt(2) * max(H, W))`` in float64."""
    return int(np.ceil(np.sqrt(2) * max(height, width)))


def radon_padded(image, theta=None):
    """
    Radon transform of a 2D image without the circle: ``skimage.transform.radon(image, theta, circle=False)`` restated from its
    documentation, all angles in one launch of the GPU (``dcp_radon_padded_2d``).  Agreement with scikit-image itself is UNVERIFIED; the
    oracle is the NumPy restatement ``tests/helpers/radon_padded_reference.py``, which the result equals bit for bit.

    Parameters
    ----------
    image : array_like
        2D array of float32 / float64, any shape: a NumPy array, a ROCm torch tensor or a ``__cuda_array_interface__`` device array.  A
        strided view (a region of interest) is read in place.  The other types raise as in :func:`discorpy_amd.prep.linepattern.radon`.
    theta : array_like, optional
        Projection angles in degree; ``np.arange(180)`` if None.

    Returns
    -------
    array_like
        (S, len(theta)) float64 sinogram of the input's kind, ``S = int(ceil(sqrt(2) * max(image.shape)))``: the transform of the image
        embedded in an S x S square of zeros with its first element at ``(S // 2 - H // 2, S // 2 - W // 2)``, rotated about
        ``(S // 2, S // 2)``.  Everything inside the image counts, a NaN included.  Everything is float64, also for float32 input.
    """
    from . import linepattern as lp
    if _p._is_complex(image):
        raise TypeError("Complex type not supported")
    shape = tuple(image.shape) if hasattr(image, "shape") else np.shape(image)
    if len(shape) != 2:
        raise ValueError("The input image must be 2-D")                      # scikit-image's words
    img = _p._Image(image, 2)
    if img.code not in (F.DTYPE_BY_NAME["float32"], F.DTYPE_BY_NAME["float64"]):
        raise NotImplementedError("radon: element type %s is not implemented on the GPU path (float32 and float64 only; integers are "
                                  "not rescaled as scikit-image rescales them)" % (img.dtype,))
    theta = np.arange(180) if theta is None else np.atleast_1d(np.asarray(theta, dtype=np.float64))
    if theta.ndim != 1:
        raise ValueError("theta must be a 1D sequence of angles")
    img = _p._rows_image(img)
    height, width = img.shape
    nangles = len(theta)
    if min(height, width) < 1:
        raise ValueError("The input image must not be empty")
    side = _padded_side(height, width)
    if side > lp.RADON_MAX_SIDE or nangles > lp.RADON_MAX_ANGLES:
        raise NotImplementedError("radon: a side above %d or more than %d angles is not implemented on the GPU path (got %d, %d)"
                                  % (lp.RADON_MAX_SIDE, lp.RADON_MAX_ANGLES, side, nangles))
    table = lp._radon_table(theta, side)
    if not np.isfinite(table).all():
        raise ValueError("theta must be finite")
    res, optr = _p._new_like(img, (side, nangles), np.float64)
    if nangles == 0:
        return res
    F.require_device()
    F.check(F.lib().dcp_radon_padded_2d(img.ptr, optr, height, width, _p._row_stride(img), img.code, nangles,
                                        table.ctypes.data_as(F.C.POINTER(F.C.c_double)), img.mem, img.device, img.stream))
    return res


def _nearest_sq(points):
    """(N, 4) float64: per point of ``points`` (an (N, 2) host array of finite (y, x)) the four smallest squared distances to all points,
    itself included, ascending; ``+inf`` where N < 4 (``dcp_nearest_sq_dists``).  No point: an empty table, no device work."""
    points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 2)
    num = len(points)
    if not np.isfinite(points).all():
        raise ValueError("the coordinates of the points must be finite")
    if num > NEAREST_MAX_POINTS:
        raise NotImplementedError("more than %d points (got %d)" % (NEAREST_MAX_POINTS, num))
    out = np.empty((num, 4), np.float64)
    if num == 0:
        return out
    F.require_device()
    F.check(F.lib().dcp_nearest_sq_dists(points.ctypes.data, out.ctypes.data, num, F.MEM_HOST, -1, None))
    return out


def _box_moments(mask, boxes):
    """(n, 6) int64 NumPy array: count, sum y, sum x, sum y y, sum x y, sum x x of the nonzero elements of ``mask`` (a 2D bool or 8- /
    16-bit integer array or tensor) inside each of the ``boxes`` ((n, 4) int32: min y, max y, min x, max x, inclusive), coordinates
    relative to the box's corner (``dcp_box_moments_2d``)."""
    img = _p._rows_image(mask)
    if img.code not in [F.DTYPE_BY_NAME[name] for name in _p._MEASURED]:
        raise NotImplementedError("box moments take bool and 8- / 16-bit integer images; got %s" % (img.dtype,))
    boxes = np.ascontiguousarray(boxes, dtype=np.int32).reshape(-1, 4)
    num = len(boxes)
    height, width = img.shape
    if num == 0 or height == 0 or width == 0:
        return np.zeros((num, 6), np.int64)
    F.require_device()
    sums, sptr = _p._new_like(img, (num, 6), np.int64)
    F.check(F.lib().dcp_box_moments_2d(img.ptr, height, width, _p._row_stride(img), img.code, boxes.ctypes.data, num, sptr, img.mem,
                                       img.device, img.stream))
    return _p._to_host(img, sums)


def _dots(mat):
    """(centroids as an (N, 2) float64 NumPy array in label order, boxes (N, 4), sums (N, 4)) of a bool or 8- / 16-bit integer dot image,
    labelled (4-neighbours) and measured on the GPU with the image's own values as weights."""
    labels, num = _p.label(mat)
    sums, boxes = _p._measures(mat, labels, num, top=num)
    cents = np.asarray(_p._centroids(sums, np.arange(1, num + 1)), dtype=np.float64).reshape(-1, 2)
    return cents, boxes, sums


def _cleared_roi(mat, ratio):
    """(int16 plane of ``clear_border(_select_roi(mat, ratio))``, of the kind of ``mat``; that kind)."""
    if _p._is_complex(mat):
        raise TypeError("Complex type not supported")
    mat, kind = _p._as_kind(mat)
    if len(mat.shape) != 2:
        raise ValueError("expected a 2-D array")
    cleared = _p.clear_border(_p._select_roi(mat, ratio))
    if kind == "torch":
        import torch
        return cleared.to(torch.int16), kind
    return np.int16(cleared), kind


def calc_size_distance(mat, ratio=0.3):
    """
    Find the median size of dots and the median distance between two nearest dots (reference ``preprocessing.py:274-305``).

    Parameters
    ----------
    mat : array_like
        2D binary array (NumPy array or ROCm torch tensor).
    ratio : float
        Used to select the ROI around the middle of an image.

    Returns
    -------
    dot_size : float
        Median size of the dots.
    dot_dist : float
        Median distance between two nearest dots.

    The ROI (a view), ``clear_border``, the labels and the per-label sums run on the GPU; the centroids are scipy's quotients bit for
    bit; the nearest distances are the second smallest of each row of ``dcp_nearest_sq_dists`` under ``np.sqrt``.  Both values equal the
    reference's exactly.
    """
    mat, _ = _cleared_roi(mat, ratio)
    cents, _, sums = _dots(mat)
    dot_size = np.median(sums[:, 1].astype(np.float64))
    dot_dist = np.median(np.sqrt(_nearest_sq(cents))[:, 1])
    return dot_size, dot_dist


def _axis_lengths(moments):
    """
    ``(major, minor)`` axis lengths of the ellipse with the second central moments of a set of pixels, from the exact integer sums
    ``(n, sum y, sum x, sum y y, sum x y, sum x x)`` of one row of :func:`_box_moments`: with ``A = n sum x x - (sum x)^2``,
    ``C = n sum y y - (sum y)^2``, ``B = n sum x y - sum x sum y`` and ``D = 4 B^2 + (A - C)^2`` as Python integers, the eigenvalues of
    the inertia tensor ``mu / mu00`` are ``l = (float(A + C) +/- sqrt(float(D))) / (2 n^2)`` (the smaller clipped at 0), and the lengths
    are ``4 sqrt(l)``.
    """
    n, sy, sx, syy, sxy, sxx = (int(v) for v in moments)
    a = n * sxx - sx * sx
    c = n * syy - sy * sy
    b = n * sxy - sx * sy
    d = 4 * b * b + (a - c) * (a - c)
    root = math.sqrt(float(d))
    norm = float(2 * n * n)
    l1 = (float(a + c) + root) / norm
    l2 = max((float(a + c) - root) / norm, 0.0)
    return 4.0 * math.sqrt(l1), 4.0 * math.sqrt(l2)


def _axes_ratio_value(moments):
    """``|major / minor - 1|`` of :func:`_axis_lengths`; ``inf`` where the minor axis is 0 (no warning)."""
    major, minor = _axis_lengths(moments)
    if minor == 0.0:
        return float("inf")
    return abs(major / minor - 1.0)


def select_dots_based_ratio(mat, ratio=0.3):
    """
    Select dots having the ratio between the axes length of the fitted ellipse smaller than a threshold (reference
    ``preprocessing.py:363-419``).

    Parameters
    ----------
    mat : array_like
        2D binary array (NumPy array or ROCm torch tensor) that holds only 0 and 1; anything else raises the reference's "not a binary
        image" ``ValueError``.
    ratio : float
        Threshold value.

    Returns
    -------
    array_like
        2D int16 NumPy array (also for a tensor). Selected dots.

    Labels, boxes and the per-box moments come from the GPU.  A box under 2 pixels high or wide is dropped; otherwise the dot is kept iff
    ``|major / minor - 1| < ratio`` with the lengths of :func:`_axis_lengths`, measured over every set pixel inside the box as the
    reference measures ``mat[box]``; a kept dot is copied box and all.  A minor axis of 0 drops the dot without a warning (a stated
    difference).  The link to scikit-image's ``regionprops`` is by construction and UNVERIFIED.
    """
    mask = _p._binary_mask(mat)
    host = np.int16(_p._host_array(mat))
    labels, num_dots = _p.label(mask)
    _, boxes = _p._measures(None, labels, num_dots, top=num_dots)
    moments = _box_moments(mask, boxes)
    kept = np.zeros_like(host)
    for box, box_slice, row in zip(boxes, _p._slices(boxes, num_dots), moments):
        if box[1] - box[0] + 1 < 2 or box[3] - box[2] + 1 < 2:
            continue
        if _axes_ratio_value(row) < ratio:
            kept[box_slice] = host[box_slice]
    return kept


def _grid_slope(mat, ratio, hor):
    """The body :func:`calc_hor_slope` and :func:`calc_ver_slope` share: the reference's steps in its order, the sinogram and the
    centroids from the GPU, the rest NumPy as the reference writes it (its float32 ``ones`` against float64 scalars included)."""
    coarse_range = 30.0  # Degree
    radi = np.pi / 180.0
    mat, kind = _cleared_roi(mat, ratio)
    (height, width) = mat.shape
    list_angle = (90.0 if hor else 0.0) + np.arange(-coarse_range, coarse_range + 1.0)
    if kind == "torch":
        import torch
        list_max = radon_padded(mat.to(torch.float32), theta=list_angle).amax(dim=0).cpu().numpy()
    else:
        list_max = np.amax(radon_padded(np.float32(mat), theta=list_angle), axis=0)
    cents, _, _ = _dots(mat)
    num_dots = len(cents)
    if hor:
        best_angle = -(list_angle[np.argmax(list_max)] - 90.0)             # (the first of equal maxima, as the reference takes it)
        dist_error = 0.5 * width * (np.tan(radi) / np.cos(best_angle * radi))
        list_cent = - cents  # For coordinate consistency
    else:
        best_angle = (list_angle[np.argmax(list_max)])
        dist_error = 0.5 * width * np.tan(radi) / np.cos(best_angle * radi)
        list_cent = np.fliplr(cents)
    mean_x = np.mean(list_cent[:, 1])
    mean_y = np.mean(list_cent[:, 0])
    index_mid_dot = np.argsort(np.sqrt((mean_x - list_cent[:, 1]) ** 2 + (mean_y - list_cent[:, 0]) ** 2))[0]
    used_dot = list_cent[index_mid_dot]
    line_slope = np.tan(best_angle * radi)
    list_tmp = np.sqrt(np.ones(num_dots, dtype=np.float32) * line_slope ** 2 + 1.0)
    list_tmp2 = used_dot[0] * np.ones(num_dots, dtype=np.float32) - line_slope * used_dot[1]
    list_dist = np.abs(line_slope * list_cent[:, 1] - list_cent[:, 0] + list_tmp2) / list_tmp
    dots_selected = list_cent[list_dist < dist_error]
    if len(dots_selected) > 1:
        slope = np.polyfit(dots_selected[:, 1], dots_selected[:, 0], 1)[0]
    else:
        slope = line_slope
    return slope


def calc_hor_slope(mat, ratio=0.3):
    """
    Calculate the slope of horizontal lines against the horizontal axis (reference ``preprocessing.py:460-508``).

    Parameters
    ----------
    mat : array_like
        2D binary array (NumPy array or ROCm torch tensor).
    ratio : float
        Used to select the ROI around the middle of an image.

    Returns
    -------
    float
        Horizontal slope of the grid.

    ROI, ``clear_border``, the conversion to float32, :func:`radon_padded` at the 61 angles around 90 degree, the labels and the
    centroids run on the GPU; the column maxima (the first of equal maxima wins) and the reference's remaining arithmetic are NumPy,
    step for step.  The slope equals the reference's exactly, the reference run on the restated transform.
    """
    return _grid_slope(mat, ratio, True)


def calc_ver_slope(mat, ratio=0.3):
    """
    Calculate the slope of vertical lines against the vertical axis (reference ``preprocessing.py:511-558``).

    Parameters
    ----------
    mat : array_like
        2D binary array (NumPy array or ROCm torch tensor).
    ratio : float
        Used to select the ROI around the middle of a image.

    Returns
    -------
    float
        Vertical slope of the grid.

    As :func:`calc_hor_slope`, with the 61 angles around 0 degree.
    """
    return _grid_slope(mat, ratio, False)


def _dot_list(mat):
    """(the (N, 2) table of (y, x) dots of the argument of a grouping function, N): a point list as it is (never on the GPU), an image
    (``shape[-1] > 2``; NumPy array or tensor) labelled and measured on the GPU as int16."""
    if not (_p._is_torch(mat) and mat.is_cuda):
        mat = np.asarray(mat.detach().cpu().numpy() if _p._is_torch(mat) else mat)
    if mat.shape[-1] > 2:
        if _p._is_torch(mat):
            import torch
            mat = mat.to(torch.int16)
        else:
            mat = np.int16(mat)
        list_dots, _, _ = _dots(mat)
        return list_dots, len(list_dots)
    if _p._is_torch(mat):
        mat = mat.cpu().numpy()
    num_dots = len(mat)
    if num_dots == 0:
        raise ValueError("Input is empty!!!")
    return mat, num_dots


def _group_lines(mat, slope, dot_dist, ratio, num_dot_miss, accepted_ratio, ver):
    """The greedy chain of the two grouping functions, in the reference's order: the dots sorted by the coordinate along the line; from
    the first dot left, every later dot that lies within ``num_dot_miss * dot_dist`` along the line and within ``ratio * dot_dist``
    of the line of slope ``slope`` through the chain's last dot joins the chain and becomes its last dot; chains of more than one dot are
    lines.  What is left is kept as a list of positions, so that a pass costs its own length."""
    list_dots, num_dots = _dot_list(mat)
    if ver:
        list_dots = np.fliplr(list_dots)  # Swap the coordinates
    list_dots = np.copy(list_dots)
    list_dots = list_dots[list_dots[:, 1].argsort()]
    if num_dots > 1 and list_dots.shape[1] != 2:
        raise ValueError("Invalid input!!!")
    dist_error = ratio * dot_dist
    search_dist = num_dot_miss * dot_dist
    ntemp1 = np.sqrt(slope * slope + 1.0)
    left = list(range(len(list_dots)))
    list_lines = []
    while len(left) > 1:
        dot1 = list_dots[left[0]]
        chain, rest = [left[0]], []
        for pos in left[1:]:
            dot2 = list_dots[pos]
            check = False
            if dot1[1] - search_dist < dot2[1] < dot1[1] + search_dist:
                ntemp2 = dot1[0] - slope * dot1[1]
                check = np.abs(slope * dot2[1] - dot2[0] + ntemp2) / ntemp1 < dist_error
            if check:
                dot1 = dot2
                chain.append(pos)
            else:
                rest.append(pos)
        left = rest
        if len(chain) > 1:
            dots_selected = list_dots[chain]
            list_lines.append(np.fliplr(dots_selected) if ver else dots_selected)
    list_len = [len(i) for i in list_lines]
    len_accepted = int(accepted_ratio * np.max(list_len))
    lines_selected = [line for line in list_lines if len(line) > len_accepted]
    return sorted(lines_selected, key=lambda list_: np.mean(list_[:, 1 if ver else 0]))


def group_dots_hor_lines(mat, slope, dot_dist, ratio=0.3, num_dot_miss=6, accepted_ratio=0.65):
    """
    Group dots into horizontal lines (reference ``preprocessing.py:561-668``).

    Parameters
    ----------
    mat : array_like
        A binary image or a list of (y,x)-coordinates of points.  An image (``shape[-1] > 2``) is labelled and measured on the GPU; a
        point list never touches it.
    slope : float
        Horizontal slope of the grid.
    dot_dist : float
        Median distance of two nearest dots.
    ratio : float
        Acceptable variation.
    num_dot_miss : int
        Acceptable missing dots between dot1 and dot2.
    accepted_ratio : float
        Use to select lines having the number of dots equal to or larger than the multiplication of the `accepted_ratio` and the
        maximum number of dots per line.

    Returns
    -------
    list of array_like
        List of 2D arrays. Each array is (y, x)-coordinates of points belong to the same group. Length of each list may be different.
    """
    return _group_lines(mat, slope, dot_dist, ratio, num_dot_miss, accepted_ratio, False)


def group_dots_ver_lines(mat, slope, dot_dist, ratio=0.3, num_dot_miss=6, accepted_ratio=0.75):
    """
    Group dots into vertical lines (reference ``preprocessing.py:671-740``).

    Parameters
    ----------
    mat : array_like
        A binary image or a list of (y,x)-coordinates of points, as for :func:`group_dots_hor_lines`.
    slope : float
        Vertical slope of the grid.
    dot_dist : float
        Median distance of two nearest dots.
    ratio : float
        Acceptable variation.
    num_dot_miss : int
        Acceptable missing dots between dot1 and dot2.
    accepted_ratio : float
        Use to select lines having the number of dots equal to or larger than the multiplication of the `accepted_ratio` and the
        maximum number of dots per line.

    Returns
    -------
    list of array_like
        List of 2D arrays. Each array is (y,x)-coordinates of points belong to the same group. Length of each list may be different.
    """
    return _group_lines(mat, slope, dot_dist, ratio, num_dot_miss, accepted_ratio, True)


def _remove_residual(list_lines, slope, residual, ver):
    list_lines2 = []
    for list_ in list_lines:
        if ver:
            list_ = np.fliplr(list_)  # Swap the coordinates
        (a2, a1, a0) = np.polyfit(list_[:, 1], list_[:, 0], 2)
        error = np.abs(((a2 * list_[:, 1] ** 2 + a1 * list_[:, 1] + a0) - list_[:, 0]) * np.cos(np.arctan(slope)))
        dots_left = list_[error < residual]
        if len(dots_left) > 0:
            list_lines2.append(np.fliplr(dots_left) if ver else dots_left)
    if len(list_lines2) == 0:
        raise ValueError("No dots left. Check the input or residual !!!")
    return list_lines2


def remove_residual_dots_hor(list_lines, slope, residual=2.5):
    """
    Remove dots having distances larger than a certain value from fitted horizontal parabolas (reference ``preprocessing.py:743-775``).
    Host NumPy.

    Parameters
    ----------
    list_lines : list of array_like
        List of the coordinates of dot-centroids on horizontal lines.
    slope : float
        Horizontal slope of the grid.
    residual : float
        Acceptable distance in pixel unit between a dot and a fitted parabola.

    Returns
    -------
    list of array_like
        List of 2D arrays. Each list is the coordinates (y, x) of dot-centroids belong to the same group. Length of each list may be
        different.
    """
    return _remove_residual(list_lines, slope, residual, False)


def remove_residual_dots_ver(list_lines, slope, residual=2.5):
    """
    Remove dots having distances larger than a certain value from fitted vertical parabolas (reference ``preprocessing.py:778-813``).
    Host NumPy.

    Parameters
    ----------
    list_lines : list of array_like
        List of the coordinates of the dot-centroids on the vertical lines.
    slope : float
        Slope of the vertical line.
    residual : float
        Acceptable distance in pixel unit between the dot and the fitted parabola.

    Returns
    -------
    list of array_like
        List of 2D array. Each list is the coordinates (y, x) of dot-centroids belong to the same group. Length of each list may be
        different.
    """
    return _remove_residual(list_lines, slope, residual, True)
