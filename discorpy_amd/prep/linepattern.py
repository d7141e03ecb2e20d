"""MI355X counterpart of the image-sized work of ``discorpy.prep.linepattern`` (line and chessboard patterns).

* :func:`gaussian_filter`   ``scipy.ndimage.gaussian_filter`` for 2-D input: the ``denoise`` step of the reference's
  ``get_cross_points_hor_lines`` / ``get_cross_points_ver_lines`` (``linepattern.py:659,739``) and the smoothing of
  :func:`convert_chessboard_to_linepattern`
* :func:`convert_chessboard_to_linepattern`   reference ``linepattern.py:570-601``: same name, arguments and defaults
* :func:`get_tilted_profile`, :func:`_calc_index_range`   reference ``linepattern.py:452-567``: same names, arguments, checks and
  error texts; the cubic-spline sampling runs through :func:`discorpy_amd.post.postprocessing.remap_coordinates`

The ``norm=True`` step of ``get_cross_points_hor_lines`` / ``get_cross_points_ver_lines`` (``linepattern.py:657,737``),
``normalization_fft``, is :func:`discorpy_amd.prep.preprocessing.normalization_fft`: with it every image-sized step of those two
functions runs on the GPU.

* :func:`get_cross_points_hor_lines`, :func:`get_cross_points_ver_lines`   reference ``linepattern.py:604-761``: same names, arguments
  and defaults; every step but the final scale and rotation of the positions runs on the GPU
* :func:`get_tilted_profiles`   N calls of :func:`get_tilted_profile` on one image in one (``dcp_tilted_profiles_2d``)
* :func:`sliding_window_slope`, :func:`get_local_extrema_points`, :func:`locate_subpixel_point`   reference ``linepattern.py:46-72,
  155-274``: same names, arguments and defaults, on one profile or on an (N, L) batch of profiles (``dcp_window_slope_rows``,
  ``dcp_local_extrema_rows``; the kernels are in ``csrc/profile_kernels.hip``)

These names are listed in :data:`CROSS_POINTS`; ``__all__`` keeps the three names it had.

Where the peak search differs from the reference: the sub-pixel position of a point is the closed form of the parabola through
``d[i-1], d[i], d[i+1]`` (``a = (d0 - 2 d1 + d2) / 2``, ``b = (-3 d0 + 4 d1 - d2) / 2``, vertex ``-b / (2 a)``) instead of
``np.polyfit``'s least-squares solve: the two agree to ~1e-13 pixel, except that on exactly collinear triples the polyfit's rounding
noise can leave ``a`` nonzero where the closed form gives ``a == 0`` and falls back to the argmin; ``select_peaks=True`` (a
``scipy.optimize.curve_fit`` per peak on the host) raises ``NotImplementedError``; a search radius above 128 raises
``NotImplementedError``; element types other than float32 are searched as float64.  The integer positions are the reference's exactly:
the minimum test, the mean of the ``radius`` largest window elements (NumPy's pairwise sum, restated bit for bit) and the sensitivity
quotient are evaluated in the profile's own type as NumPy 2 evaluates them.

* :func:`radon`   ``skimage.transform.radon(image, theta, circle=True)`` restated from its documentation (``dcp_radon_2d``; the kernel is
  in ``csrc/radon_kernels.hip``): all angles in one launch, float64, equal bit for bit to the NumPy restatement of its definition
  (``DESIGN.md``, "Radon transform"; ``tests/helpers/radon_reference.py``).  scikit-image is not installed where this was written, so
  agreement with scikit-image itself is UNVERIFIED
* :func:`calc_slope_distance_hor_lines`, :func:`calc_slope_distance_ver_lines`, :func:`_make_circle_mask`   reference
  ``linepattern.py:277-449``: same names, arguments and defaults, step for step; the Gaussian, the two sinograms, their maxima and the
  peak search run on the GPU.  They give the ``slope_*`` and ``dist_*`` the cross-point functions take

These names are listed in :data:`RADON`.

* :func:`select_good_peaks`   reference ``linepattern.py:75-152``: same name, arguments and defaults, on one profile or on an (N, L)
  batch of profiles with their candidate peaks: one Gaussian fit per candidate, one wave of the GPU per fit (``dcp_select_peaks_rows``;
  the kernel is in ``csrc/select_peaks_kernels.hip``; ``DESIGN.md``, "Peak selection")

This name is listed in :data:`PEAK_SELECTION`.

Out of scope: the ``select_peaks`` flag, which is not wired to :func:`select_good_peaks` yet, so ``select_peaks=True`` still raises
``NotImplementedError`` in the peak search, in the cross-point functions and in the Radon slope functions alike (the docstring of
:func:`select_good_peaks` shows the composition that works today), and ``circle=False`` of the Radon transform, which raises too.
:mod:`discorpy_amd.prep.linecomplete` carries the five functions with the flag working: the search, the fits and the sub-pixel step in
one call of the GPU (``dcp_extrema_select_rows``), through the private bodies of this module.

The Gaussian runs as hand-written HIP kernels through ``dcp_correlate_sym_2d`` (``include/discorpy_hip.h``; the kernels are in
``csrc/gauss_kernels.hip``) with scipy's arithmetic restated operation by operation (``DESIGN.md``), so the result equals scipy's bit
for bit wherever the float64 result lies within the element type's range.  The weights are computed here, in NumPy, exactly as scipy's
``_gaussian_kernel1d`` computes them.  There is no CPU path: a missing library or GPU raises.  Inputs are NumPy arrays (staged through
the GPU), ROCm torch tensors (zero-copy, on torch's current stream) or ``__cuda_array_interface__`` device arrays, as in
:mod:`discorpy_amd.prep.preprocessing`.

Where :func:`gaussian_filter` differs from scipy: only 2-D input and ``order=0`` are taken (a derivative order raises
``NotImplementedError``); bool and float16 raise ``RuntimeError("data type not supported")`` (scipy takes both); a radius above 192
(sigma 48 at ``truncate=4``) raises ``NotImplementedError``; one ``mode`` serves both axes.
"""
import numbers

import numpy as np

from .. import _ffi as F
from ..post.postprocessing import _Image, _MODES, remap_coordinates
from .preprocessing import _as_kind, _is_complex, _new_like, _row_stride, _rows_image, _select_roi, _thres_double, normalization_fft

__all__ = ["gaussian_filter", "convert_chessboard_to_linepattern", "get_tilted_profile"]
# the slope and distance search in front of the cross-point route, and the Radon transform it rests on
RADON = ["radon", "calc_slope_distance_hor_lines", "calc_slope_distance_ver_lines"]
RADON_MAX_SIDE, RADON_MAX_ANGLES = 32768, 65535       # dcp_radon_2d: every index of the kernel fits 32 bits
# the cross-point route (batched profiles, the peak search and the reference's two functions on top of them)
CROSS_POINTS = ["get_tilted_profiles", "sliding_window_slope", "locate_subpixel_point", "get_local_extrema_points",
                "get_cross_points_hor_lines", "get_cross_points_ver_lines"]
PEAK_MAX_RADIUS = 128          # dcp_local_extrema_rows: the sorted tail stays inside one block of NumPy's pairwise sum
# the selection of good peaks behind the peak search
PEAK_SELECTION = ["select_good_peaks"]
SELECT_MAX_RADIUS = 128        # dcp_select_peaks_rows: the window of one wave, 257 doubles of LDS


def _gaussian_weights(sigma, truncate=4.0, radius=None):
    """The ``2 * radius + 1`` float64 weights of scipy's ``gaussian_filter1d(order=0)``: symmetric to the bit, summing to 1."""
    if radius is None:
        radius = int(truncate * float(sigma) + 0.5)
    if not isinstance(radius, numbers.Integral) or radius < 0:
        raise ValueError("Radius must be a nonnegative integer.")           # scipy's words
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return phi / phi.sum()


def _per_axis(value, what):
    """(axis 0, axis 1) of a scalar or a pair."""
    if value is None or np.ndim(value) == 0:
        return value, value
    values = tuple(value)
    if len(values) != 2:
        raise RuntimeError("sequence argument must have length equal to input rank")     # scipy's words
    return values


def gaussian_filter(mat, sigma, *, order=0, mode="reflect", cval=0.0, truncate=4.0, radius=None, out=None):
    """
    2-D Gaussian filter: ``scipy.ndimage.gaussian_filter(mat, sigma, mode=mode, cval=cval, truncate=truncate, radius=radius)`` on
    the GPU, bit for bit.

    Parameters
    ----------
    mat : array_like
        2D array (NumPy array, ROCm torch tensor or ``__cuda_array_interface__`` device array) of float32 / float64 or an 8- to
        64-bit integer type.  A view whose rows are strided (``a[:, 3:-7]``) is read in place.
    sigma : float or (float, float)
        Standard deviation, or ``(sigma_y, sigma_x)``.  An axis whose sigma is at most 1e-15 is not filtered.
    order : int
        Only 0 (no derivative) is implemented.
    mode : {"reflect", "constant", "nearest", "mirror", "wrap", "grid-mirror", "grid-constant", "grid-wrap"}
        How a line is extended beyond its ends; the ``grid-`` names are scipy's aliases.
    cval : float
        Value beyond the ends under ``"constant"``; it enters the sums as a double, not cast to the element type.
    truncate : float
        The radius of an axis is ``int(truncate * sigma + 0.5)``.
    radius : None, int or (int, int)
        Radius of the window, overriding ``truncate``.
    out : array_like, optional
        Destination of the same kind, shape and dtype; must not overlap ``mat``.

    Returns
    -------
    array_like
        2D array of the input's kind and dtype.  Axis 0 is filtered first; its result is rounded to the element type before
        axis 1 is filtered, as scipy stores it between the passes.  Integer types truncate toward zero.
    """
    if _is_complex(mat):
        raise TypeError("Complex type not supported")
    if any(o != 0 for o in _per_axis(order, "order")):
        raise NotImplementedError("gaussian_filter: derivative orders are not implemented on the GPU path (order=0 only)")
    if mode not in _MODES:
        raise RuntimeError("boundary mode not supported")                   # scipy's words
    sigmas, radii = _per_axis(sigma, "sigma"), _per_axis(radius, "radius")
    img = _Image(mat, 2)
    if img.code == F.DTYPE_BY_NAME["bool"]:
        raise RuntimeError("data type not supported")
    weights = [_gaussian_weights(s, truncate, r) if s > 1e-15 else None for s, r in zip(sigmas, radii)]
    img = _rows_image(img)
    height, width = img.shape
    res, optr = img.empty((height, width), out=out)
    if height == 0 or width == 0:
        return res
    F.require_device()
    wargs = []
    for w in weights:
        wargs += [None, -1] if w is None else [w.ctypes.data_as(F.C.POINTER(F.C.c_double)), len(w) // 2]
    F.check(F.lib().dcp_correlate_sym_2d(img.ptr, optr, height, width, _row_stride(img), img.code, *wargs, _MODES.index(mode), float(cval),
                                         img.mem, img.device, img.stream))
    return res


def convert_chessboard_to_linepattern(mat, smooth=True, bgr="bright", sigma=3):
    """
    Convert a chessboard image to a line-pattern image (reference ``linepattern.py:570-601``).

    Parameters
    ----------
    mat : array_like
        2D array.  A NumPy array (or anything ``numpy.asarray`` takes), or a torch tensor on a ROCm device.
    smooth : bool, optional
        Apply a gaussian smoothing filter if True.
    bgr : {'bright', 'dark'}
        Select the background of the output image.
    sigma : int
        Sigma of the Gaussian window, if smooth is True.

    Returns
    -------
    array_like
        Line-pattern image.  NumPy input: the Gaussian (``mode="nearest"``) comes from the GPU, the gradient, the crop and edge
        pad, the inversion and the division by the mean are NumPy's, as the reference writes them -- the reference's result bit for
        bit.  A device tensor: the same steps with torch on the device (integer input as float64, as ``numpy.gradient`` reads
        it); the mean is then a reduction in another order, so the result agrees to rounding; a tensor is returned.
    """
    crop = 4 if smooth is True else 2
    mat, kind = _as_kind(mat, "convert_chessboard_to_linepattern takes NumPy arrays and torch tensors; use gaussian_filter for other device arrays")
    if smooth is True:
        mat = gaussian_filter(mat, sigma, mode="nearest")
    if kind == "torch":
        import torch
        if not mat.is_floating_point():
            mat = mat.to(torch.float64)
        grad_y, grad_x = torch.gradient(mat)
        mat_line = (grad_y.abs() + grad_x.abs()) / 2
        inner = mat_line[crop:-crop, crop:-crop]
        mat_line = torch.nn.functional.pad(inner[None, None], (crop, crop, crop, crop), mode="replicate")[0, 0]
        if bgr == "bright":
            mat_line = mat_line.max() - mat_line
        return mat_line / mat_line.abs().mean()
    mat_line = np.mean(np.abs(np.gradient(mat)), axis=0)
    mat_line = np.pad(mat_line[crop:-crop, crop:-crop], crop, mode="edge")
    if bgr == "bright":
        mat_line = np.max(mat_line) - mat_line
    return mat_line / np.mean(np.abs(mat_line))


def _calc_index_range(height, width, angle_deg, direction):
    """
    Extractable range of a tilted line-profile (reference ``linepattern.py:452-509``).  Positive angle is counterclockwise.

    Parameters
    ----------
    height : int
        Height of the image.
    width : int
        Width of the image.
    angle_deg : float
        Tilted angle in Degree.
    direction : {"horizontal", "vertical"}
        Direction of line-profile.

    Returns
    -------
    min_idx : int
        Minimum index of lines.
    max_idx : int
        Maximum index of lines.
    """
    horizontal = direction == "horizontal"
    if np.abs(angle_deg) == 90.0:
        raise ValueError("If the input angle is around 90-degree, use the '%s' option and update the angle to around 0-degree "
                         "instead!!!" % ("vertical" if horizontal else "horizontal"))
    # the line crosses `along` pixels and drifts by along * tan(angle) across the `across` indices it may start from
    along, across = (width, height) if horizontal else (height, width)
    drift = along * np.tan(np.abs(angle_deg * np.pi / 180.0))
    min_idx, max_idx = 0, across - 1
    if horizontal:
        if angle_deg > 0:
            min_idx = int(np.ceil(along * np.tan(angle_deg * np.pi / 180.0)))
        else:
            max_idx = across - 1 - int(np.floor(drift))
    else:
        if angle_deg > 0:
            max_idx = across - 1 - int(np.ceil(along * np.tan(angle_deg * np.pi / 180.0)))
        else:
            min_idx = int(np.floor(drift))
    if not (0 <= min_idx < across and 0 <= max_idx < across):
        raise ValueError("%s index is out of range, please select the direction correctly !!!" % ("Row" if horizontal else "Column"))
    return min_idx, max_idx


def get_tilted_profile(mat, index, angle_deg, direction):
    """
    Get the intensity-profile along a tilted line across an image (reference ``linepattern.py:512-567``).  Positive angle is
    counterclockwise.

    Parameters
    ----------
    mat : array_like
        2D array: a NumPy array or a ROCm torch tensor (anything with ``shape`` and 2-D slicing that ``remap_coordinates`` takes).
    index : int
        Index of the line.
    angle_deg : float
        Tilted angle in Degree.
    direction : {"horizontal", "vertical"}
        Direction of line-profile.

    Returns
    -------
    xlist : array_like
        1D array. x-positions of points on the line.
    ylist : array_like
        1D array. y-positions of points on the line.
    profile : array_like
        1D array. Intensities of points on the line: ``remap_coordinates(band, ..., order=3, mode="nearest")`` on the band of rows
        (columns) the line crosses, sliced as the reference slices it -- the spline prefilter sees the band's edges, not the
        image's.  Of the input's kind.
    """
    shape = tuple(mat.shape)
    if len(shape) != 2:
        raise ValueError("Input must be a 2D array !!!")
    (height, width) = shape
    (min_idx, max_idx) = _calc_index_range(height, width, angle_deg, direction)
    angle = angle_deg * np.pi / 180.0
    if (index < min_idx) or (index > max_idx):
        raise ValueError("Input index is out of possible range: [{0}, {1}]".format(min_idx, max_idx))
    if direction == "horizontal":
        rlist = np.linspace(0, np.floor(width / np.cos(angle)), width)
        xlist = np.clip(rlist * np.cos(angle), 0, width - 1)
        ylist = np.clip(index + rlist * np.sin(-angle), 0, height - 1)
        ymin = int(np.floor(np.amin(ylist)))
        ymax = int(np.ceil(np.amax(ylist))) + 1
        profile = remap_coordinates(mat[ymin:ymax, :], ylist - ymin, xlist, order=3, mode="nearest")
    else:
        rlist = np.linspace(0, np.floor(height / np.cos(angle)), height)
        ylist = np.clip(rlist * np.cos(angle), 0, height - 1)
        xlist = np.clip(index + rlist * np.sin(angle), 0, width - 1)
        xmin = int(np.floor(np.amin(xlist)))
        xmax = int(np.ceil(np.amax(xlist))) + 1
        profile = remap_coordinates(mat[:, xmin:xmax], ylist, xlist - xmin, order=3, mode="nearest")
    return xlist, ylist, profile


# --------------------------------------------------------------------------- the cross-point route

def _line_coordinates(height, width, index, angle, direction):
    """(xlist, ylist, first row / column of the band, its count): the expressions of the reference's ``get_tilted_profile``."""
    if direction == "horizontal":
        rlist = np.linspace(0, np.floor(width / np.cos(angle)), width)
        xlist = np.clip(rlist * np.cos(angle), 0, width - 1)
        ylist = np.clip(index + rlist * np.sin(-angle), 0, height - 1)
        across = ylist
    else:
        rlist = np.linspace(0, np.floor(height / np.cos(angle)), height)
        ylist = np.clip(rlist * np.cos(angle), 0, height - 1)
        xlist = np.clip(index + rlist * np.sin(angle), 0, width - 1)
        across = xlist
    lo = int(np.floor(np.amin(across)))
    return xlist, ylist, lo, int(np.ceil(np.amax(across))) + 1 - lo


def get_tilted_profiles(mat, indices, angle_deg, direction):
    """
    Get the intensity-profiles along N parallel tilted lines across an image: what N calls of :func:`get_tilted_profile` return,
    from one call of the GPU.  Positive angle is counterclockwise.

    Parameters
    ----------
    mat : array_like
        2D array: a NumPy array or a ROCm torch tensor.  float32 / float64 take the batched kernels (``dcp_tilted_profiles_2d``: the
        cubic prefilter of every line's own band, then the samples); other element types go line by line through
        :func:`get_tilted_profile`.
    indices : sequence of float
        Index of every line.
    angle_deg : float
        Tilted angle in Degree.
    direction : {"horizontal", "vertical"}
        Direction of the line-profiles.

    Returns
    -------
    xlists : ndarray
        (N, L) float64. x-positions of the points on every line, the reference's bit for bit.
    ylists : ndarray
        (N, L) float64. y-positions of the points on every line.
    profiles : array_like
        (N, L) of the input's kind and dtype. Intensities of the points on every line.
    """
    if direction not in ("horizontal", "vertical"):
        raise ValueError("direction must be 'horizontal' or 'vertical'")
    if _is_complex(mat):
        raise TypeError("Complex type not supported")
    shape = tuple(mat.shape) if hasattr(mat, "shape") else np.shape(mat)
    if len(shape) != 2:
        raise ValueError("Input must be a 2D array !!!")
    (height, width) = shape
    (min_idx, max_idx) = _calc_index_range(height, width, angle_deg, direction)
    angle = angle_deg * np.pi / 180.0
    indices = np.atleast_1d(np.asarray(indices))
    if indices.ndim != 1:
        raise ValueError("indices must be a 1D sequence")
    for index in indices:
        if (index < min_idx) or (index > max_idx):
            raise ValueError("Input index is out of possible range: [{0}, {1}]".format(min_idx, max_idx))
    nprof, length = len(indices), width if direction == "horizontal" else height
    xlists, ylists = np.empty((nprof, length)), np.empty((nprof, length))
    band_lo, band_n = np.empty(nprof, np.int32), np.empty(nprof, np.int32)
    for p, index in enumerate(indices):
        xlists[p], ylists[p], band_lo[p], band_n[p] = _line_coordinates(height, width, index, angle, direction)
    mat, kind = _as_kind(mat, "get_tilted_profiles takes NumPy arrays and torch tensors")
    img = _Image(mat, 2)
    if img.code not in (F.DTYPE_BY_NAME["float32"], F.DTYPE_BY_NAME["float64"]) or nprof == 0:
        rows = [get_tilted_profile(mat, index, angle_deg, direction)[2] for index in indices]
        if kind == "torch":
            import torch
            return xlists, ylists, torch.stack(rows) if rows else mat.new_empty((0, length))
        return xlists, ylists, np.asarray(rows, dtype=img.dtype).reshape(nprof, length)
    img = _rows_image(img)
    res, optr = img.empty((nprof, length))
    F.require_device()
    if kind == "torch":
        import torch
        ydev, xdev = torch.from_numpy(ylists).to(mat.device), torch.from_numpy(xlists).to(mat.device)
        yptr, xptr = ydev.data_ptr(), xdev.data_ptr()
    else:
        yptr, xptr = ylists.ctypes.data, xlists.ctypes.data
    i32p = F.C.POINTER(F.C.c_int32)
    F.check(F.lib().dcp_tilted_profiles_2d(img.ptr, optr, height, width, _row_stride(img), img.code, 0 if direction == "horizontal" else 1, nprof,
                                           length, yptr, xptr, band_lo.ctypes.data_as(i32p), band_n.ctypes.data_as(i32p), img.mem, img.device,
                                           img.stream))
    return xlists, ylists, res


def _profile_rows(list_data, what):
    """(``list_data`` as a fresh (N, L) float32 / float64 NumPy array, whether it was one 1-D profile)."""
    if _is_complex(list_data):
        raise TypeError("Complex type not supported")
    rows, _ = _as_kind(list_data, "%s takes NumPy arrays and torch tensors" % what)
    if hasattr(rows, "detach"):
        rows = rows.detach().cpu().numpy()
    rows = np.array(rows, dtype=None if rows.dtype in (np.float32, np.float64) else np.float64)
    if rows.ndim not in (1, 2):
        raise ValueError("%s takes a 1D array or an (N, L) batch of them" % what)
    return np.atleast_2d(rows), rows.ndim == 1


def sliding_window_slope(list_data, size=3, norm=True):
    """
    Compute the absolute slopes of a linear fit within a sliding window across the input data, normalized by the mean slope if norm
    is True (reference ``linepattern.py:155-192``).

    Parameters
    ----------
    list_data : array-like
        1d-array, or an (N, L) batch of them.  float32 / float64; other types are read as float64.
    size : int, optional
        Size of the sliding window for the linear fit.
    norm : bool, optional
        Normalize the result by the mean slope if True.

    Returns
    -------
    array_like
        Normalized absolute slopes for each data point, of the input's shape.  The slope of the window's least-squares line is the
        closed form ``sum_k (k - r) p[i + k] / sum_k (k - r)^2`` of the reference's ``np.polyfit`` (``dcp_window_slope_rows``; float64
        sums, agreeing with the polyfit to ~1e-14 of the largest slope); the division by the mean is NumPy's, row by row.
    """
    rows, single = _profile_rows(list_data, "sliding_window_slope")
    npoint = rows.shape[1]
    if npoint < 3:
        raise ValueError("Data size must be larger than 2")
    size = int(np.clip(size, 3, npoint))
    if size % 2 == 0:
        size += 1
    slopes = np.empty_like(rows)
    if rows.shape[0] > 0:
        F.require_device()
        img = _rows_image(rows)
        F.check(F.lib().dcp_window_slope_rows(img.ptr, slopes.ctypes.data, rows.shape[0], npoint, _row_stride(img), img.code, size, img.mem, img.device,
                                              img.stream))
    if norm is True:
        for p in range(rows.shape[0]):
            nmean = np.mean(slopes[p])
            if nmean != 0.0:
                slopes[p] = slopes[p] / nmean
    return slopes[0] if single else slopes


def locate_subpixel_point(list_point, option="min"):
    """
    Locate the extremum point of a 1D array with subpixel accuracy (reference ``linepattern.py:46-72``).

    Parameters
    ----------
    list_point : array_like
        1D array.
    option : {"min", "max"}
        To locate the minimum point or the maximum point.

    Returns
    -------
    float
        Subpixel position of the extremum point.  Three points: the vertex of the parabola through them in closed form (what the
        reference's ``np.polyfit`` solves by least squares; module docstring); any other number of points: ``np.polyfit``.
    """
    num_point = len(list_point)
    if num_point == 3:
        d0, d1, d2 = (np.float64(v) for v in list_point)
        a = (d0 - 2.0 * d1 + d2) / 2.0
        b = (-3.0 * d0 + 4.0 * d1 - d2) / 2.0
    else:
        a, b, _ = np.polyfit(np.arange(num_point), list_point, 2)
    if option == "min":
        pos = np.argmin(list_point)
    else:
        pos = np.argmax(list_point)
    if a != 0.0:
        with np.errstate(all="ignore"):
            num = - b / (2 * a)
        if (num >= 0) and (num < num_point):
            pos = num
    return pos


def _normalize_background(list_data):
    """The ``norm`` step of the reference's ``get_local_extrema_points`` (``linepattern.py:236-253``) on one row, call for call."""
    num_point = len(list_data)
    xlist = np.arange(num_point)
    mat_comb = np.asarray(np.vstack((xlist, list_data)))
    mat_sort = mat_comb[:, mat_comb[1, :].argsort()]
    list_sort = mat_sort[1]
    ndrop = int(0.25 * num_point)
    (a1, a0) = np.polyfit(xlist[ndrop:-ndrop - 1], list_sort[ndrop:-ndrop - 1], 1)[:2]
    list_fit = a1 * xlist + a0
    l_thres, u_thres = a0, a1 * xlist[-1] + a0
    list_sort[(list_fit >= l_thres) & (list_fit <= u_thres)] = list_fit[(list_fit >= l_thres) & (list_fit <= u_thres)]
    mat_sort[1] = list_sort
    nmean = np.mean(np.abs(list_fit))
    backgr = mat_sort[:, mat_sort[0, :].argsort()][1]
    return np.divide(list_data, backgr, out=nmean * np.ones_like(list_data), where=backgr != 0)


def get_local_extrema_points(list_data, option="min", radius=7, sensitive=0.1, denoise=True, norm=True, subpixel=True, select_peaks=False,
                             **kwargs):
    """
    Get a list of local extremum points from a 1D array (reference ``linepattern.py:195-274``), or from every row of a batch.

    Parameters
    ----------
    list_data : array_like
        1D array, or an (N, L) batch of them.  float32 / float64; other types are read as float64.
    option : {"min", "max"}
        To get minimum points or maximum points
    radius : int
        Search radius. Used to locate extremum points.  Clipped to ``[1, L // 4]`` as in the reference; at most 128.
    sensitive : float
        To detect extremum points against random noise. Smaller is more sensitive.  A Python float is rounded to the profile's type,
        a NumPy float64 scalar promotes the comparison, as NumPy 2 compares them.
    denoise : bool, optional
        Applying a smoothing filter if True: this module's :func:`gaussian_filter` along the rows, sigma 3.
    norm : bool, optional
        Apply background normalization to the array: the reference's sorted-background line fit, row by row in NumPy.
    subpixel : bool, optional
        Locate points with subpixel accuracy (the closed form of :func:`locate_subpixel_point`, in the kernel).
    select_peaks : bool, optional
        Not implemented (a ``curve_fit`` per peak on the host): True raises ``NotImplementedError``.

    Returns
    -------
    array_like
        1D array. Positions of local extremum points.  For a batch: a list of N such arrays.
    """
    if select_peaks is True:
        raise NotImplementedError("get_local_extrema_points: select_peaks=True (a scipy curve_fit per peak) is not implemented on the GPU path")
    return _extrema_points(list_data, option, radius, sensitive, denoise, norm, subpixel, None)


def _selection(select_peaks, kwargs, what="select_good_peaks"):
    """What ``select_peaks=True, **kwargs`` asks of the reference's ``select_good_peaks``: None without the flag (the reference then
    ignores ``kwargs``), else ``dict(tol, sigma, use_offset)``; a name the reference's function does not take raises its ``TypeError``."""
    if select_peaks is not True:
        return None
    select = dict(tol=0.2, sigma=0, use_offset=True)
    for name in kwargs:
        if name not in select:
            raise TypeError("%s() got an unexpected keyword argument '%s'" % (what, name))
    select.update(kwargs)
    select["tol"], select["sigma"], select["use_offset"] = float(select["tol"]), float(select["sigma"]), bool(select["use_offset"])
    if select["tol"] != select["tol"] or select["sigma"] != select["sigma"]:
        raise ValueError("select_good_peaks: %s is NaN" % ("tol" if select["tol"] != select["tol"] else "sigma"))
    return select


def _extrema_points(list_data, option, radius, sensitive, denoise, norm, subpixel, select):
    """The body of :func:`get_local_extrema_points`; select: None, or the selection of :func:`_selection`, which the search, the fits
    and the sub-pixel step then go through in one call (``dcp_extrema_select_rows``)."""
    rows, single = _profile_rows(list_data, "get_local_extrema_points")
    nrows, num_point = rows.shape
    radius = int(np.clip(radius, 1, num_point // 4))
    if radius > PEAK_MAX_RADIUS:
        raise NotImplementedError("get_local_extrema_points: a search radius above %d is not implemented on the GPU path (got %d)"
                                  % (PEAK_MAX_RADIUS, radius))
    # (with the selection a window of radius 0 or 1 has at most 3 samples: the reference fits none of them and keeps nothing)
    if nrows == 0 or num_point == 0 or (select is not None and radius < 2):
        return np.asarray([]) if single else [np.asarray([]) for _ in range(nrows)]
    if denoise is True:
        rows = gaussian_filter(rows, (0, 3))
    if option == "max":
        rows = np.max(rows, axis=1, keepdims=True) - rows
    if norm is True:
        rows = np.asarray([_normalize_background(row) for row in rows])
    in_kernel = subpixel is True and radius >= 1
    found = np.empty((nrows, num_point))
    F.require_device()
    img = _rows_image(rows)
    if select is None:
        F.check(F.lib().dcp_local_extrema_rows(img.ptr, found.ctypes.data, nrows, num_point, _row_stride(img), img.code, radius,
                                               _thres_double(sensitive, rows.dtype.name), 1 if in_kernel else 0, img.mem, img.device, img.stream))
    else:
        # the fits read np.max(list_data) - list_data: formed by the kernel itself, or here where it is to be smoothed first
        sel_ptr, sel_stride = None, num_point
        if select["sigma"] > 0:
            sel = _rows_image(gaussian_filter(np.max(rows, axis=1, keepdims=True) - rows, (0, select["sigma"])))
            sel_ptr, sel_stride = sel.ptr, _row_stride(sel)
        F.check(F.lib().dcp_extrema_select_rows(img.ptr, found.ctypes.data, nrows, num_point, _row_stride(img), img.code, radius,
                                                _thres_double(sensitive, rows.dtype.name), 1 if in_kernel else 0, sel_ptr, sel_stride,
                                                select["tol"], 1 if select["use_offset"] else 0, None, None, img.mem, img.device, img.stream))
    results = []
    for p in range(nrows):
        count = int(found[p, -1])
        if count == 0:
            results.append(np.asarray([]))
        elif subpixel is True:
            if in_kernel:
                results.append(found[p, :count].copy())
            else:       # (rows of fewer than 4 samples, where the radius clips to 0: the reference's loop, on the host)
                results.append(np.asarray([i - 1 + locate_subpixel_point(rows[p, i - 1:i + 2], option="min") for i in found[p, :count].astype(np.int64)]))
        else:
            results.append(found[p, :count].astype(np.int64))
    return results[0] if single else results


def select_good_peaks(list_data, peaks, tol=0.2, radius=11, sigma=0, use_offset=True):
    """
    Select good peaks from the input data based on Gaussian fitting and tolerance criteria (reference ``linepattern.py:105-152``),
    on one profile or on every row of a batch: one wave of the GPU per candidate (``dcp_select_peaks_rows``).

    Parameters
    ----------
    list_data : array_like
        1d-array, or an (N, L) batch of them.  float32 / float64; other types are read as float64 before everything (scipy would
        smooth an integer profile in its own type).
    peaks : list of int
        Indices of candidate peaks in the data.  For a batch: a list of N such lists, one per row.
    tol : float, optional
        Tolerance for peak fitting accuracy.
    radius : int, optional
        Radius around each peak to consider for fitting.  At most 128.
    sigma : float, optional
        Standard deviation for Gaussian smoothing: this module's :func:`gaussian_filter` along the rows.
    use_offset : bool, optional
        Use fitted offset value for judging if True.

    Returns
    -------
    list of int
        Indices of the selected good peaks, as an array in the order given (``np.asarray([])`` where none is selected, as in the
        reference).  For a batch: a list of N such arrays.

    Notes
    -----
    The fit restates the Levenberg-Marquardt iteration scipy's ``curve_fit`` runs for the reference (``DESIGN.md``, "Peak
    selection"); the decisions are the reference's wherever its own fit does not hang on where the iteration stops.  A constant
    window is rejected by ``max == min``, where the reference tests ``np.std(...) != 0.0``.

    ``select_peaks=True`` of the peak search is not wired to this function yet in this module; :mod:`discorpy_amd.prep.linecomplete`
    takes the flag and runs the search, these fits and the sub-pixel step in one call.  The composition that works today, on data the
    caller has prepared (``denoise=False, norm=False``)::

        points = get_local_extrema_points(d, option="min", radius=r, denoise=False, norm=False, subpixel=False)
        points = select_good_peaks(np.max(d) - d, points, radius=r)
        points = [p - 1 + locate_subpixel_point(d[p - 1:p + 2], option="min") for p in points]
    """
    rows, single = _profile_rows(list_data, "select_good_peaks")
    nrows, num_point = rows.shape
    radius = int(radius)
    if radius < 1:
        raise ValueError("select_good_peaks: radius must be at least 1 (got %d)" % radius)
    if radius > SELECT_MAX_RADIUS:
        raise NotImplementedError("select_good_peaks: a radius above %d is not implemented on the GPU path (got %d)" % (SELECT_MAX_RADIUS, radius))
    tol = float(tol)
    if tol != tol:
        raise ValueError("select_good_peaks: tol is NaN")
    per_row = [peaks] if single else list(peaks)
    if len(per_row) != nrows:
        raise ValueError("select_good_peaks: %d rows but %d lists of peaks" % (nrows, len(per_row)))
    per_row = [np.asarray(p) for p in per_row]
    for k, p in enumerate(per_row):
        if p.ndim != 1 or (p.size and p.dtype.kind not in "iu"):
            raise ValueError("select_good_peaks: the peaks of a row are a 1D sequence of integers")
        if p.size and (p.min() < 0 or p.max() >= num_point):
            raise ValueError("select_good_peaks: row %d has a peak outside [0, %d)" % (k, num_point))
    counts = [p.size for p in per_row]
    npeaks = int(sum(counts))
    if npeaks == 0:
        return np.asarray([]) if single else [np.asarray([]) for _ in range(nrows)]
    if sigma > 0:
        rows = gaussian_filter(rows, (0, sigma))
    peak_row = np.repeat(np.arange(nrows, dtype=np.int32), counts)
    peak_idx = np.concatenate(per_row).astype(np.int32)
    keep = np.zeros(npeaks, np.uint8)
    F.require_device()
    img = _rows_image(rows)
    i32p = F.C.POINTER(F.C.c_int32)
    F.check(F.lib().dcp_select_peaks_rows(img.ptr, nrows, num_point, _row_stride(img), img.code, peak_row.ctypes.data_as(i32p),
                                          peak_idx.ctypes.data_as(i32p), npeaks, radius, tol, 1 if use_offset else 0, keep.ctypes.data, None,
                                          img.mem, img.device, img.stream))
    results, first = [], 0
    for p, count in zip(per_row, counts):
        good = p[keep[first:first + count] != 0]
        results.append(good if good.size else np.asarray([]))
        first += count
    return results[0] if single else results


def _cross_points(mat, slope, dist, ratio, norm, offset, bgr, radius, sensitive, denoise, subpixel, chessboard, select, across_hor):
    """The body the two cross-point functions share; across_hor: the generated lines run horizontally (``get_cross_points_ver_lines``);
    select: None, or the selection of :func:`_selection` for the peak search of all profiles."""
    if _is_complex(mat):
        raise TypeError("Complex type not supported")
    mat, kind = _as_kind(mat, "the cross-point functions take NumPy arrays and torch tensors")
    if len(mat.shape) != 2:
        raise ValueError("Input must be a 2D array !!!")
    (height, width) = mat.shape
    if bgr == "bright":
        mat = (mat.max() - mat) if kind == "torch" else (np.max(mat) - mat)
    if norm is True:
        mat = normalization_fft(mat, 5)
    if denoise is True:
        mat = gaussian_filter(mat, 3)
    angle = np.arctan(slope)
    if across_hor:
        angle_deg, direction = -np.rad2deg(angle), "horizontal"
        first, last = _calc_index_range(height, width, angle_deg, direction=direction)
        offset = int(np.clip(offset, 0, min(height, width) // 8))
    else:
        angle_deg, direction = np.rad2deg(angle), "vertical"
        first, last = _calc_index_range(height, width, angle_deg, direction=direction)
        offset = int(np.clip(offset, 0, min(height, width) // 3))
    indices = np.arange(first + offset, last - offset, ratio * dist)
    xlists, ylists, profiles = get_tilted_profiles(mat, indices, angle_deg, direction)
    if kind == "torch":
        profiles = profiles.cpu().numpy()
    if len(indices) == 0:
        return np.asarray([])
    if chessboard is True:
        profiles = sliding_window_slope(profiles, size=3)
    rlists = _extrema_points(profiles, "max", radius, sensitive, not denoise, not norm, subpixel, select)
    list_points = []
    for xlist, ylist, rlist in zip(xlists, ylists, rlists):
        scale = np.sqrt((xlist[-1] - xlist[0]) ** 2 + (ylist[-1] - ylist[0]) ** 2) / ((width if across_hor else height) - 1)
        rlist = rlist * scale
        if across_hor:
            xlist1 = rlist * np.cos(angle) + xlist[0]
            ylist1 = rlist * np.sin(angle) + ylist[0]
        else:
            xlist1 = rlist * np.sin(angle) + xlist[0]
            ylist1 = rlist * np.cos(angle) + ylist[0]
        list_points.extend(np.asarray(list(zip(ylist1, xlist1))))
    return np.asarray(list_points)


def get_cross_points_hor_lines(mat, slope_ver, dist_ver, ratio=0.3, norm=True, offset=0, bgr="bright", radius=11, sensitive=0.1,
                               denoise=True, subpixel=True, chessboard=False, select_peaks=False, **kwargs):
    """
    Get points on horizontal lines of a line-pattern image, or a chessboard image, by intersecting with a list of generated
    vertical-lines (reference ``linepattern.py:604-681``).

    Parameters
    ----------
    mat : array_like
        2D array.  A NumPy array, or a torch tensor on a ROCm device (it stays there up to the profiles).
    slope_ver : float
        Representative slope of vertical lines.
    dist_ver : float
        Representative distance between vertical lines.
    ratio : float
        To adjust the distance (=ratio * dist_ver) between generated lines to create more or fewer lines.
    norm : bool, optional
        Apply background normalization to the array.
    offset : int
        Starting index of generated lines.
    bgr : {"bright", "dark"}
        Specify the brightness of the background relative to the lines.
    radius : int
        Search radius. Used to locate extremum points.
    sensitive : float
        To detect extremum points against random noise. Smaller is more sensitive.
    denoise : bool, optional
        Applying a smoothing filter if True.
    subpixel : bool, optional
        Locate points with subpixel accuracy.
    chessboard : bool, optional
        If True, cross points are located by finding local maxima of slopes of local linear fits of the generated lines.
    select_peaks : bool, optional
        Not implemented: True raises ``NotImplementedError``.

    Returns
    -------
    array_like
        List of (y,x)-coordinates of points: an (N, 2) NumPy array in the reference's order.  ``max - mat``,
        :func:`~discorpy_amd.prep.preprocessing.normalization_fft`, :func:`gaussian_filter`, all profiles
        (:func:`get_tilted_profiles`), the slopes and the peak search run on the GPU; the scale and rotation of the positions are NumPy's.
    """
    if select_peaks is True:
        raise NotImplementedError("select_peaks=True (a scipy curve_fit per peak) is not implemented on the GPU path")
    return _cross_points(mat, slope_ver, dist_ver, ratio, norm, offset, bgr, radius, sensitive, denoise, subpixel, chessboard, None, False)


def get_cross_points_ver_lines(mat, slope_hor, dist_hor, ratio=0.3, norm=True, offset=0, bgr="bright", radius=11, sensitive=0.1,
                               denoise=True, subpixel=True, chessboard=False, select_peaks=False, **kwargs):
    """
    Get points on vertical lines of a line-pattern image, or a chessboard image, by intersecting with a list of generated
    horizontal-lines (reference ``linepattern.py:684-761``).

    Parameters
    ----------
    mat : array_like
        2D array.  A NumPy array, or a torch tensor on a ROCm device (it stays there up to the profiles).
    slope_hor : float
        Representative slope of horizontal lines.
    dist_hor : float
        Representative distance between horizontal lines.
    ratio : float
        To adjust the distance (=ratio * dist_hor) between generated lines to create more or fewer lines.
    norm : bool, optional
        Apply background normalization to the array.
    offset : int
        Starting index of generated lines.
    bgr : {"bright", "dark"}
        Specify the brightness of the background against the lines.
    radius : int
        Search radius. Used to locate extremum points.
    sensitive : float
        To detect extremum points against random noise. Smaller is more sensitive.
    denoise : bool, optional
        Applying a smoothing filter if True.
    subpixel : bool, optional
        Locate points with subpixel accuracy.
    chessboard : bool, optional
        If True, cross points are located by finding local maxima of slopes of local linear fits of the generated lines.
    select_peaks : bool, optional
        Not implemented: True raises ``NotImplementedError``.

    Returns
    -------
    array_like
        List of (y,x)-coordinates of points: an (N, 2) NumPy array in the reference's order; see :func:`get_cross_points_hor_lines`.
    """
    if select_peaks is True:
        raise NotImplementedError("select_peaks=True (a scipy curve_fit per peak) is not implemented on the GPU path")
    return _cross_points(mat, slope_hor, dist_hor, ratio, norm, offset, bgr, radius, sensitive, denoise, subpixel, chessboard, None, True)


# --------------------------------------------------------------------------- the Radon transform and the slope and distance search

def _radon_table(theta, side):
    """(A, 4) float64, C-contiguous: ``cos a, sin a, tx, ty`` of every angle of ``theta`` (degrees) -- the rotation about
    ``(side // 2, side // 2)`` that ``dcp_radon_2d`` applies, in NumPy float64."""
    center = side // 2
    angle = np.deg2rad(np.asarray(theta, dtype=np.float64))
    cos_a, sin_a = np.cos(angle), np.sin(angle)
    shift_x = -center * (cos_a + sin_a - 1)
    shift_y = -center * (cos_a - sin_a - 1)
    return np.ascontiguousarray(np.stack([cos_a, sin_a, shift_x, shift_y], axis=1))


def radon(image, theta=None, circle=True):
    """
    Radon transform of a 2D image: ``skimage.transform.radon(image, theta, circle=True)`` restated from its documentation, all angles
    in one launch of the GPU (``dcp_radon_2d``).  Agreement with scikit-image itself is UNVERIFIED: it is not installed where this was
    written; the oracle is the NumPy restatement of the definition below (``tests/helpers/radon_reference.py``), which the result
    equals bit for bit.

    Parameters
    ----------
    image : array_like
        2D array of float32 / float64: a NumPy array, a ROCm torch tensor (zero-copy, on torch's current stream) or a
        ``__cuda_array_interface__`` device array.  A strided view (a region of interest) is read in place.  A non-square image is
        cropped to its centred square, each axis starting at ``ceil(excess / 2)``, as a view.  Integer and bool input raise
        ``NotImplementedError`` (scikit-image would rescale them; that is not imitated), float16 raises ``RuntimeError``, complex
        input ``TypeError``.
    theta : array_like, optional
        Projection angles in degree; ``np.arange(180)`` if None.
    circle : bool
        Only True is implemented: the image is zero outside its inscribed circle.  What lies there is replaced by 0.0, not
        multiplied by it, so a NaN outside the circle does not reach the result.  The warning scikit-image gives for nonzero
        elements outside the circle is not reproduced.

    Returns
    -------
    array_like
        (N, len(theta)) float64 sinogram of the input's kind, column ``i`` the projection at ``theta[i]``.  With ``c0 = N // 2`` and
        ``a`` the angle in radian, sample ``(r, c)`` reads the image at ``x = cos(a) c + sin(a) r - c0 (cos(a) + sin(a) - 1)``,
        ``y = -sin(a) c + cos(a) r - c0 (cos(a) - sin(a) - 1)`` by bilinear interpolation between ``floor`` and ``ceil`` with zeros
        outside the image, and ``sinogram[c, i]`` is the sum over ``r`` in ascending order.  Everything is float64, also for float32
        input, where scikit-image would stay in float32: a stated difference.
    """
    if _is_complex(image):
        raise TypeError("Complex type not supported")
    if circle is not True:
        raise NotImplementedError("radon: circle=False is not implemented on the GPU path")
    shape = tuple(image.shape) if hasattr(image, "shape") else np.shape(image)
    if len(shape) != 2:
        raise ValueError("The input image must be 2-D")                      # scikit-image's words
    img = _Image(image, 2)
    if img.code not in (F.DTYPE_BY_NAME["float32"], F.DTYPE_BY_NAME["float64"]):
        raise NotImplementedError("radon: element type %s is not implemented on the GPU path (float32 and float64 only; integers are "
                                  "not rescaled as scikit-image rescales them)" % (img.dtype,))
    theta = np.arange(180) if theta is None else np.atleast_1d(np.asarray(theta, dtype=np.float64))
    if theta.ndim != 1:
        raise ValueError("theta must be a 1D sequence of angles")
    img = _rows_image(img)
    side, nangles = min(img.shape), len(theta)
    if side < 1:
        raise ValueError("The input image must not be empty")
    if side > RADON_MAX_SIDE or nangles > RADON_MAX_ANGLES:
        raise NotImplementedError("radon: a side above %d or more than %d angles is not implemented on the GPU path (got %d, %d)"
                                  % (RADON_MAX_SIDE, RADON_MAX_ANGLES, side, nangles))
    table = _radon_table(theta, side)
    if not np.isfinite(table).all():
        raise ValueError("theta must be finite")
    res, optr = _new_like(img, (side, nangles), np.float64)
    if nangles == 0:
        return res
    # the centred square, as a view: a shifted pointer, the same row stride
    first = [int(np.ceil((n - side) / 2)) for n in img.shape]
    ptr = img.ptr + (first[0] * img.strides[0] + first[1] * img.strides[1]) * (4 if img.f32 else 8)
    F.require_device()
    F.check(F.lib().dcp_radon_2d(ptr, optr, side, img.strides[0] if img.shape[0] > 1 else side, img.code, nangles,
                                 table.ctypes.data_as(F.C.POINTER(F.C.c_double)), img.mem, img.device, img.stream))
    return res


def _make_circle_mask(width, ratio):
    """
    Create a circle mask (reference ``linepattern.py:277-299``).

    Parameters
    -----------
    width : int
        Width of a square array.
    ratio : float
        Ratio between the diameter of the mask and the width of the array.

    Returns
    ------
    array_like
         Square array: float32, 1.0 inside the circle, 0.0 outside.
    """
    mask = np.zeros((width, width), dtype=np.float32)
    center = width // 2
    radius = ratio * center
    y, x = np.ogrid[-center:width - center, -center:width - center]
    mask[x * x + y * y <= radius * radius] = 1.0
    return mask


def _slope_distance(mat, ratio, search_range, radius, sensitive, bgr, denoise, norm, subpixel, chessboard, select, hor):
    """The body the two slope functions share; hor: the lines run horizontally (the search is centred on 90 degree); select: None, or
    the selection of :func:`_selection` for the peak search of the best projection."""
    if _is_complex(mat):
        raise TypeError("Complex type not supported")
    mat, kind = _as_kind(mat, "the slope functions take NumPy arrays and torch tensors")
    if len(mat.shape) != 2:
        raise ValueError("Input must be a 2D array !!!")
    if chessboard is True:
        if kind == "torch":
            # (on a host copy: torch sums the conversion's mean in another order, which moved a distance by 1e-7 pixel; the copy
            # keeps a tensor's result equal to an array's)
            import torch
            mat = torch.from_numpy(convert_chessboard_to_linepattern(mat.cpu().numpy())).to(mat.device)
        else:
            mat = convert_chessboard_to_linepattern(mat)
    if denoise is True:
        mat = gaussian_filter(mat, 3)
    mat_roi = _select_roi(mat, ratio, square=True)
    mask = _make_circle_mask(mat_roi.shape[0], 0.92)
    if kind == "torch":
        import torch
        if bgr == "bright":
            mat_roi = mat_roi.max() - mat_roi
        masked = mat_roi * torch.from_numpy(mask).to(mat_roi.device)

        def column_maxima(sinogram):
            return sinogram.amax(dim=0).cpu().numpy()
    else:
        if bgr == "bright":
            mat_roi = np.max(mat_roi) - mat_roi
        masked = mat_roi * mask

        def column_maxima(sinogram):
            return np.amax(sinogram, axis=0)
    angle_coarse = (90.0 if hor else 0.0) + np.arange(-search_range, search_range + 1.0)
    best_angle1 = angle_coarse[np.argmax(column_maxima(radon(masked, theta=angle_coarse, circle=True)))]
    angle_fine = np.arange(best_angle1 - 1.0, best_angle1 + 1.05, 0.05)
    sinogram2 = radon(masked, theta=angle_fine, circle=True)
    pos_max2 = np.argmax(column_maxima(sinogram2))       # (A numbers: the first of equal maxima, as the reference takes it)
    best_angle2 = -(angle_fine[pos_max2] - 90) if hor else angle_fine[pos_max2]
    slope = np.tan(best_angle2 * np.pi / 180.0)
    profile = sinogram2[:, pos_max2]
    list_ext_point = _extrema_points(profile.cpu().numpy() if kind == "torch" else profile, "max", radius, sensitive, denoise, norm, subpixel,
                                     select)
    if len(list_ext_point) > 3:
        distance = np.median(np.abs(np.diff(list_ext_point)))
    else:
        distance = np.mean(np.abs(np.diff(list_ext_point)))
    return slope, distance


def calc_slope_distance_hor_lines(mat, ratio=0.3, search_range=30.0, radius=9, sensitive=0.1, bgr="bright", denoise=True, norm=True,
                                  subpixel=True, chessboard=False, select_peaks=False, **kwargs):
    """
    Calculate the representative distance between horizontal lines and the representative slope of these lines using the ROI around
    the middle of a line-pattern image or a chessboard image (reference ``linepattern.py:302-375``).

    Parameters
    ----------
    mat : array_like
        2D array.  A NumPy array, or a torch tensor on a ROCm device (it stays there up to the best projection).
    ratio : float
        Used to select the ROI around the middle of an image.
    search_range : float
        Search range in Degree to determine the slope of lines.
    radius : int
        Search radius. Used to locate lines.
    sensitive : float
        To detect lines against random noise. Smaller is more sensitive.
    bgr : {"bright", "dark"}
        Specify the brightness of the background against the lines.
    denoise : bool, optional
        Apply a smoothing filter if True.
    norm : bool, optional
        Apply background normalization to the array.
    subpixel : bool, optional
        Locate points with subpixel accuracy.
    chessboard : bool, optional
        If True, converts the input chessboard image to a line-pattern image.  For a tensor the conversion
        (:func:`convert_chessboard_to_linepattern`) runs on a host copy and goes back to the device: torch sums the conversion's mean
        in another order than NumPy, and a tensor must give the array's slope and distance.
    select_peaks : bool, optional
        Not implemented: True raises ``NotImplementedError``.

    Returns
    -------
    slope : float
        Slope of horizontal lines in Radian.
    distance : float
        Distance between horizontal lines.  The reference's steps one for one: :func:`gaussian_filter`, the square ROI, ``max - roi``,
        the circle mask, a coarse sinogram (:func:`radon`) over ``90 + arange(-search_range, search_range + 1)`` degree, a fine one in
        steps of 0.05 degree around its best angle, and :func:`get_local_extrema_points` on the best projection.  The elementwise
        steps are NumPy's or torch's by the input's kind; the maxima over a projection are taken where the sinogram lives.  The
        sinograms are float64 also for float32 images (:func:`radon`).
    """
    if select_peaks is True:
        raise NotImplementedError("select_peaks=True (a scipy curve_fit per peak) is not implemented on the GPU path")
    return _slope_distance(mat, ratio, search_range, radius, sensitive, bgr, denoise, norm, subpixel, chessboard, None, True)


def calc_slope_distance_ver_lines(mat, ratio=0.3, search_range=30.0, radius=9, sensitive=0.1, bgr="bright", denoise=True, norm=True,
                                  subpixel=True, chessboard=False, select_peaks=False, **kwargs):
    """
    Calculate the representative distance between vertical lines and the representative slope of these lines using the ROI around
    the middle of a line-pattern image or a chessboard image (reference ``linepattern.py:378-449``).

    Parameters
    ----------
    mat : array_like
        2D array.  A NumPy array, or a torch tensor on a ROCm device (it stays there up to the best projection).
    ratio : float
        Used to select the ROI around the middle of an image.
    search_range : float
        Search range in Degree to determine the slope of lines.
    radius : int
        Search radius. Used to locate lines.
    sensitive : float
        To detect lines against random noise. Smaller is more sensitive.
    bgr : {"bright", "dark"}
        Specify the brightness of the background against the lines.
    denoise : bool, optional
        Applying a smoothing filter if True.
    norm : bool, optional
        Apply background normalization to the array.
    subpixel : bool, optional
        Locate points with subpixel accuracy.
    chessboard : bool, optional
        If True, converts the input chessboard image to a line-pattern image.
    select_peaks : bool, optional
        Not implemented: True raises ``NotImplementedError``.

    Returns
    -------
    slope : float
        Slope of vertical lines in Radian.
    distance : float
        Distance between vertical lines; see :func:`calc_slope_distance_hor_lines` (the search is centred on 0 degree).
    """
    if select_peaks is True:
        raise NotImplementedError("select_peaks=True (a scipy curve_fit per peak) is not implemented on the GPU path")
    return _slope_distance(mat, ratio, search_range, radius, sensitive, bgr, denoise, norm, subpixel, chessboard, None, False)
