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

Out of scope: the 1-D peak search (``get_local_extrema_points``, ``select_good_peaks``: host-side scipy fitting on one profile at a
time), the Radon functions (scikit-image) and therefore ``get_cross_points_hor_lines`` / ``get_cross_points_ver_lines`` as whole
functions: what remains host-side of them is the slope search where no angle is given and, per profile, the peak search and its
fits; a caller runs the image-sized steps here and those per-profile steps with the reference.

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
from .preprocessing import _as_kind, _is_complex, _row_stride, _rows_image

__all__ = ["gaussian_filter", "convert_chessboard_to_linepattern", "get_tilted_profile"]


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
