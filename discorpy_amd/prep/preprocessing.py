"""MI355X counterpart of the ``scipy.ndimage`` part of ``discorpy.prep.preprocessing``: the median filter and the dot-pattern route.

* :func:`normalization`   reference ``discorpy/prep/preprocessing.py:50-73``: same name, arguments and default
* :func:`median_filter`   the ``scipy.ndimage.median_filter(mat, size, mode="reflect")`` both :func:`normalization` (size 51) and the
  denoise step of the reference's ``binarization`` (size 2) rest on
* :func:`normalization_fft`, :func:`_apply_fft_filter`, :func:`_make_window`   reference ``preprocessing.py:76-158``: same names, arguments
  and defaults; the Fourier Gaussian filter runs on the GPU without an FFT (below)
* :func:`label`, :func:`sum_labels`, :func:`center_of_mass`, :func:`find_objects`, :func:`binary_fill_holes`   the ``scipy.ndimage``
  functions of those names the reference calls on binary dot images (``preprocessing.py:247-445``, ``:966-997``), equal to scipy's
  results element for element
* :func:`check_num_dots`, :func:`get_points_dot_pattern` (``binarize=False``), :func:`select_dots_based_size`,
  :func:`select_dots_based_distance`   the reference's functions on top of them: same names, arguments, messages and prints

* :func:`threshold_otsu`, :func:`clear_border`, :func:`opening`, :func:`binarization`   the reference's ``binarization``
  (``preprocessing.py:216-248``) and the three scikit-image functions it calls, each restated through what NumPy and scipy define:
  ``np.histogram`` / ``np.bincount`` and the published Otsu formula, ``scipy.ndimage.label`` with the full 3 x 3 structure,
  ``scipy.ndimage.grey_opening`` with the 3 x 3 cross.  Results equal those composites element for element; scikit-image itself is
  not installed where this was written, so the link to it is by construction and UNVERIFIED ("Binarization")

The rest of the reference's module that rests on scikit-image (``regionprops`` behind ``select_dots_based_ratio``, the
Radon-based angle search of ``calc_hor_slope`` / ``calc_ver_slope``) is restated from the documentation in :mod:`discorpy_amd.prep.dotpattern`, with
``calc_size_distance`` and the grouping of the dots into lines, and imported here (``DOT_GRID``, at the bottom); scikit-image itself stays
out of scope: it is not installed where this was written, so those links are by construction and UNVERIFIED.  Not here:
``calculate_threshold``, the parabola masks, ``rotate_points``, ``remove_subset_points`` and the polyfit-based grouping.

The median runs as a hand-written HIP kernel through ``dcp_median_filter_2d`` (``include/discorpy_hip.h``; the kernels are in
``csrc/median_kernels.hip``): it SELECTS the element of rank ``(size_y * size_x) // 2`` of every window by a binary search on
order-preserving integer keys, so the result is one of the input's elements, bit for bit -- what scipy returns.  There is no CPU
path: a missing library or GPU raises.  Inputs are NumPy arrays (staged through the GPU), ROCm torch tensors (zero-copy, on torch's
current stream) or ``__cuda_array_interface__`` device arrays, as in :mod:`discorpy_amd.post.postprocessing`.

Labelling (``dcp_label_2d``, ``csrc/label_kernels.hip``) is a union-find whose roots are the components' smallest linear indices: a
tile per workgroup in LDS, the tile seams by atomic min on a parent plane, then a prefix sum over the root flags, which numbers the
components in the raster order of their first pixels -- scipy's numbering, without a sort or a host pass.  The measurements
(``dcp_label_measures_2d``) are int64 sums and 32-bit boxes accumulated with integer atomics, exact in any order; the quotients are
formed in NumPy float64 as scipy forms them, so for bool and 8- / 16-bit integer images (every partial sum an integer below 2**53)
they equal scipy's bit for bit.  Float and wider integer weights raise ``NotImplementedError``: the reference only ever measures
binary images.  :func:`binary_fill_holes` is the same labelling run on the complement (4-neighbour structure) plus a border flag.

Binarization (``csrc/binarize_kernels.hip``; ``dcp_clear_border_2d`` beside the labelling it reuses): the GPU delivers exact integers --
minimum and maximum, int64 bin counts, the number of set pixels, 0 / 1 planes -- and the few quotients of the Otsu formula are formed
in NumPy float64 on at most 65536 numbers, the division of labour of the centroids.  :func:`binarization` uploads a NumPy image once,
runs every step on device planes and downloads the int16 result once; a tensor stays on torch's current stream.  Departures from the
reference: the contrast is inverted iff ``2 * count > height * width`` on the exact count of set pixels (the reference's float32
``np.sum`` is exact below 2**24 set pixels and may round above); a given ``thres`` reaches the kernel as one double (NumPy 2's
promotion: a Python float against a float32 image is rounded to float32, a NumPy float64 scalar promotes the comparison to float64), so
64-bit integer images beyond 2**53 are compared after rounding to double, as NumPy compares them with a float threshold.

The Fourier Gaussian filter (``dcp_fourier_gauss_2d``, ``csrc/fourier_kernels.hip``): the reference pads the image, multiplies by the sign
plane ``(-1)^(x + y)``, transforms, multiplies by a centred Gaussian window, transforms back, multiplies by the sign plane again, takes
the real part and crops.  Sign and window are products of a factor per axis, so the whole operator is ``real(A_y m A_x^T)`` with one
complex Toeplitz matrix per axis (:func:`_fourier_taps`; ``DESIGN.md``, "Fourier Gaussian filter"): two float64 passes that read the
source through the pad's index fold and compute the cropped rows and columns only -- no padded plane, no complex plane of the padded
size.  The tables are made here in NumPy (one 1-D inverse FFT of the window's factor per axis, cached) and the kernels sum the taps
that matter: what is left out is bounded by 2**-56 of the table's absolute sum.  The result agrees with the reference's to rounding
(both lie about 1e-15 of ``max|result|`` from a long-double evaluation), not bit for bit.  Departures, all raised before any device
work: a ``sigma`` that is not a positive finite number and a ``pad`` that is not a non-negative integer raise ``ValueError`` (the
reference silently produces NaNs for ``sigma = 0``); ``np.pad`` modes other than "reflect", "symmetric", "edge", "wrap" and "constant"
(zeros) raise ``NotImplementedError``; complex and float16 input raise as for the median; a padded side above 16384 raises
``NotImplementedError``.  The result is float64 for every input type, as the reference's is.

Where the median differs from scipy:

* floats are selected in IEEE 754 total order, so the result is defined bit for bit: ``-0.0`` sorts below ``+0.0`` (scipy treats them
  as equal and either may come out of it), negative NaNs sort below ``-inf`` and positive NaNs above ``+inf``, each by payload (in
  scipy the outcome depends on where the NaNs sit in the window).  A NaN counts as one element of the windows that hold it and
  touches no other pixel;
* 64-bit integers are selected exactly; scipy passes them through a double, so values beyond 2**53 may differ from it;
* the window is reflected with period ``2 n`` for any number of folds, so an image may be much smaller than the window.  scipy
  1.15.3 does not reflect correctly once half the window reaches ``4 * side`` on a side longer than 1 (e.g. a 3 x 40 image at size
  31); there the two differ, and this one follows the rule above;
* complex input raises scipy's ``TypeError("Complex type not supported")``; float16 raises ``RuntimeError("data type not
  supported")`` as everywhere in this package (scipy's median filter itself accepts float16);
* only 2-D input is taken.
"""
import ctypes
import functools
import operator

import numpy as np

from .. import _ffi as F
from ..post.postprocessing import _Image, _is_cai, _is_torch

__all__ = ["normalization", "median_filter"]
# the Fourier route to the same end (the names the reference's linepattern module calls, and the table behind them)
FOURIER = ["normalization_fft", "_apply_fft_filter", "_make_window", "_fourier_taps"]
# the dot-pattern route (labelling, measurements, hole filling and the reference's functions on top of them)
# the binarization of a dot image in front of that route
BINARIZATION = ["threshold_otsu", "clear_border", "opening", "binarization"]
DOT_PATTERN = ["label", "sum_labels", "center_of_mass", "find_objects", "binary_fill_holes", "check_num_dots", "get_points_dot_pattern",
               "select_dots_based_size", "select_dots_based_distance"]
# the rest of that route, from prep.dotpattern (imported at the bottom of this module)
DOT_GRID = ["radon_padded", "calc_size_distance", "select_dots_based_ratio", "calc_hor_slope", "calc_ver_slope", "group_dots_hor_lines",
            "group_dots_ver_lines", "remove_residual_dots_hor", "remove_residual_dots_ver"]


def _window(size):
    """(size_y, size_x) of an int or a pair."""
    try:
        sy = sx = operator.index(size)
    except TypeError:
        sizes = tuple(size)
        if len(sizes) != 2:
            raise RuntimeError("sequence argument must have length equal to input rank")     # scipy's words
        sy, sx = operator.index(sizes[0]), operator.index(sizes[1])
    return sy, sx


def _is_complex(mat):
    if _is_torch(mat):
        return mat.is_complex()
    if _is_cai(mat):
        return np.dtype(mat.__cuda_array_interface__["typestr"]).kind == "c"
    return np.asarray(mat).dtype.kind == "c"


def _as_kind(mat, refusal="takes NumPy arrays and torch tensors"):
    """(``mat`` as the array the steps work on, "torch" / "numpy"): a ROCm tensor stays, a CPU tensor or an array-like becomes a NumPy
    array, any other device array is a ``TypeError`` of the text ``refusal``."""
    if _is_torch(mat) and mat.is_cuda:
        return mat, "torch"
    if _is_cai(mat):
        raise TypeError(refusal)
    return np.asarray(mat.detach().cpu().numpy() if _is_torch(mat) else mat), "numpy"


def _rows_image(mat):
    """``mat`` (or the :class:`_Image` of it) as a 2-D :class:`_Image` with unit column stride and non-overlapping rows (a copy where it
    is not)."""
    img = mat if isinstance(mat, _Image) else _Image(mat, 2)
    if img.strides[1] != 1 and img.shape[1] > 1 or img.strides[0] < img.shape[1] and img.shape[0] > 1:
        if img.cai:
            raise ValueError("device arrays must have unit column stride and non-overlapping rows")
        img = _Image(img.keep.contiguous() if img.torch else np.ascontiguousarray(img.keep), 2)
    return img


def _row_stride(img):
    return img.strides[0] if img.shape[0] > 1 else img.shape[1]          # (a single row's stride is arbitrary)


def _real_plane(mat):
    """``mat`` as a 2-D :class:`_Image` of a real element type (the module's ``TypeError`` for complex input)."""
    if _is_complex(mat):
        raise TypeError("Complex type not supported")
    return _rows_image(mat)


def median_filter(mat, size, *, out=None):
    """
    2-D median filter with scipy's ``mode="reflect"``: ``scipy.ndimage.median_filter(mat, size, mode="reflect")`` on the GPU.

    Parameters
    ----------
    mat : array_like
        2D array (NumPy array, ROCm torch tensor or ``__cuda_array_interface__`` device array) of float32 / float64, an 8- to
        64-bit integer type or bool.  A view whose rows are strided (``a[:, 3:-7]``) is read in place.
    size : int or (int, int)
        Size of the window, or ``(size_y, size_x)``.  An even size leans towards the lower indices and yields the upper median,
        as scipy's does.
    out : array_like, optional
        Destination of the same kind, shape and dtype; must not overlap ``mat``.

    Returns
    -------
    array_like
        2D array of the input's kind and dtype: at every pixel the element of rank ``(size_y * size_x) // 2`` of its window.
    """
    if _is_complex(mat):
        raise TypeError("Complex type not supported")
    sy, sx = _window(size)
    img = _rows_image(mat)
    height, width = img.shape
    res, optr = img.empty((height, width), out=out)
    if height == 0 or width == 0:
        return res
    F.require_device()
    F.check(F.lib().dcp_median_filter_2d(img.ptr, optr, height, width, _row_stride(img), img.code, sy, sx, img.mem, img.device, img.stream))
    return res


def normalization(mat, size=51):
    """
    Correct a non-uniform background of an image using the median filter (reference ``preprocessing.py:50-73``).

    Parameters
    ----------
    mat : array_like
        2D array.  A NumPy array (or anything ``numpy.asarray`` takes), or a torch tensor on a ROCm device.
    size : int
        Size of the median filter.

    Returns
    -------
    array_like
        2D array. Corrected background.  NumPy input: the median plane comes from the GPU and the mean and the quotient are
        computed in NumPy as the reference writes them -- the reference's result bit for bit, for every dtype.  A device tensor:
        the median plane is computed on torch's current stream, its mean is taken in float64 and rounded to the result type
        (the input's for floats, float64 otherwise) and the quotient is computed with torch; a tensor is returned.
    """
    mat, kind = _as_kind(mat, "normalization takes NumPy arrays and torch tensors; use median_filter for other device arrays")
    mat_bck = median_filter(mat, size)
    if kind == "torch":
        import torch
        rtype = mat.dtype if mat.is_floating_point() else torch.float64
        mean_val = mat_bck.to(torch.float64).mean().to(rtype)
        return mean_val * mat.to(rtype) / mat_bck.to(rtype)
    mean_val = np.mean(mat_bck)
    try:
        mat_cor = mean_val * mat / mat_bck
    except ZeroDivisionError:
        mat_bck[mat_bck == 0.0] = mean_val
        mat_cor = mean_val * mat / mat_bck
    return mat_cor


# --------------------------------------------------------------------------- the Fourier Gaussian background filter

# np.pad's modes that fold an index (or pad with zeros), and the DCP_MODE_* each one is under dcp_fourier_gauss_2d
_PAD_MODES = {"reflect": 5, "symmetric": 0, "edge": 4, "wrap": 7, "constant": 2}
_FOURIER_MAX_SIDE = 16384       # kFourierMaxSide of csrc/dcp_internal.h: refused here before a table of that length is made


def _make_window(height, width, sigma=10):
    """
    Create a 2D Gaussian window (reference ``preprocessing.py:76-99``): ``exp(-(x * x / num + y * y / num))`` with ``num = 2.0 * sigma *
    sigma``, ``x = -(width - 1) / 2 ... (width - 1) / 2`` along the columns and ``y`` likewise along the rows.

    Parameters
    ----------
    height : int
        Height of the window.
    width : int
        Width of the window.
    sigma : int
        Sigma of the Gaussian window.

    Returns
    -------
    array_like
        2D float64 array.
    """
    xcenter = (width - 1.0) / 2.0
    ycenter = (height - 1.0) / 2.0
    y, x = np.ogrid[-ycenter:height - ycenter, -xcenter:width - xcenter]
    num = 2.0 * sigma * sigma
    window = np.exp(-(x * x / num + y * y / num))
    return window


def _taps_below_the_bound(n, sigma, total):
    """
    Mask of the ``d`` in ``0 .. n - 1`` at which ``c = ifft(w)`` is PROVABLY below ``2**-58 * total / n`` in magnitude (``total`` the sum
    of ``|c|``), so that all of them together weigh less than ``2**-58`` of the table.  A float64 FFT leaves rounding noise of about
    ``1e-17 max|c|`` in every entry, also where the true value is ``1e-40``; hundreds of such entries add up to more than the kernels'
    truncation bound (``2**-56`` of the table) allows to drop, and the sums would run over the whole axis for nothing.  The bound:
    ``w`` is the Gaussian ``g(x) = exp(-x^2 / (2 sigma^2))`` sampled at ``x = u - (n - 1) / 2``, ``u = 0 .. n - 1``.  Summed over ALL
    integers ``u`` the transform is, by Poisson's formula, ``sigma sqrt(2 pi) / n`` times a sum over the integers ``m`` of
    ``exp(-2 pi^2 sigma^2 (m - d / n)^2)`` up to phases; the samples outside ``0 .. n - 1`` add at most
    ``(2 / n) g(a) (1 + sigma^2 / a)``, ``a = (n + 1) / 2`` (the first one left out plus the integral of the tail).  A window that is
    cut off visibly at the ends of the axis (``sigma`` above about ``n / 18``) keeps every tap: its transform has an algebraic tail.
    """
    frac = np.arange(n, dtype=np.float64) / n
    q = 2.0 * np.pi * np.pi * sigma * sigma
    edge = (n + 1.0) / 2.0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        aliases = np.exp(-q * frac * frac) + np.exp(-q * (1.0 - frac) * (1.0 - frac)) + 2.0 * np.exp(-q) / (1.0 - np.exp(-q))
        bound = sigma * np.sqrt(2.0 * np.pi) / n * aliases + 2.0 / n * np.exp(-edge * edge / (2.0 * sigma * sigma)) * (1.0 + sigma * sigma / edge)
        return bound <= np.ldexp(total, -58) / n


@functools.lru_cache(maxsize=8)
def _fourier_taps_of(n, sigma):
    x = np.arange(n, dtype=np.float64) - (n - 1.0) / 2.0
    num = 2.0 * sigma * sigma
    c = np.fft.ifft(np.exp(-(x * x / num)))
    c[_taps_below_the_bound(n, sigma, np.abs(c).sum())] = 0.0
    delta = np.arange(-(n - 1), n)
    a = np.where(delta % 2 == 0, 1.0, -1.0) * c[delta % n]
    re, im = np.ascontiguousarray(a.real), np.ascontiguousarray(a.imag)
    re.setflags(write=False)
    im.setflags(write=False)
    return re, im


def _fourier_taps(n, sigma):
    """
    The taps of the Fourier Gaussian filter along an axis of padded length ``n``: the operator ``S F^-1 diag(w) F S`` (``S`` the sign
    ``(-1)^k``, ``F`` the DFT, ``w[k] = exp(-(k - (n - 1) / 2)^2 / (2 sigma^2))``) is the Toeplitz matrix ``A[j, k] = a(j - k)`` with
    ``a(d) = (-1)^d c[d mod n]``, ``c = ifft(w)``; for odd ``n`` the wrapped half enters with the opposite sign,
    ``a(d - n) = -a(d)``, which is why the table runs over the signed difference.

    Returns
    -------
    (re, im) : two read-only float64 arrays of length ``2 n - 1``; index ``d + n - 1`` holds ``a(d)``.  Cached per ``(n, sigma)``.
    ``c`` comes from a float64 inverse FFT; its entries that are provably negligible (:func:`_taps_below_the_bound`) are exact zeros
    instead of the FFT's rounding noise, so that the kernels' support bound can see where the taps end.
    """
    return _fourier_taps_of(int(n), float(sigma))


def _check_fft_arguments(mat, sigma, pad, mode):
    """(sigma as a float, pad as an int, the DCP_MODE_* of ``mode``), or the documented exception; no device work."""
    try:
        sigma_f = float(sigma)
    except (TypeError, ValueError):
        sigma_f = float("nan")
    if not (np.isfinite(sigma_f) and sigma_f > 0.0):
        raise ValueError("sigma must be a positive finite number (got %r)" % (sigma,))
    try:
        pad_i = operator.index(pad)
    except TypeError:
        pad_i = -1
    if pad_i < 0:
        raise ValueError("pad must be a non-negative integer (got %r)" % (pad,))
    if mode not in _PAD_MODES:
        raise NotImplementedError("pad mode %r is not implemented on the GPU path (supported: %s)" % (mode, ", ".join(_PAD_MODES)))
    if _is_complex(mat):
        raise TypeError("Complex type not supported")
    return sigma_f, pad_i, _PAD_MODES[mode]


def _apply_fft_filter(mat, sigma, pad, mode='reflect'):
    """
    Apply a Fourier Gaussian filter (reference ``preprocessing.py:102-128``) on the GPU, without an FFT: the reference's
    ``real(ifft2(fft2(mat * sign) * window) * sign)`` on the padded image is ``real(A_y mat A_x^T)`` with the Toeplitz matrices of
    :func:`_fourier_taps`, evaluated in float64 by ``dcp_fourier_gauss_2d`` for the cropped rows and columns only.

    Parameters
    ----------
    mat : array_like
        2D array (NumPy array, ROCm torch tensor or ``__cuda_array_interface__`` device array) of float32 / float64, an 8- to
        64-bit integer type or bool.  A view whose rows are strided (``a[:, 3:-7]``) is read in place.
    sigma : float
        Sigma of the Gaussian filter.
    pad : int
        Pad width; it may exceed the image's sides.
    mode : {"reflect", "symmetric", "edge", "wrap", "constant"}
        ``np.pad``'s mode (``"constant"`` pads with zeros).

    Returns
    -------
    array_like
        2D float64 array of the input's kind and shape. Filtered image.
    """
    sigma, pad, code = _check_fft_arguments(mat, sigma, pad, mode)
    img = _rows_image(mat)
    height, width = img.shape
    res, rptr = _new_like(img, (height, width), np.float64)
    if height == 0 or width == 0:
        return res
    if max(height, width) + 2 * pad > _FOURIER_MAX_SIDE:
        raise NotImplementedError("padded side above %d (got %d x %d)" % (_FOURIER_MAX_SIDE, height + 2 * pad, width + 2 * pad))
    F.require_device()
    taps = _fourier_taps(height + 2 * pad, sigma) + _fourier_taps(width + 2 * pad, sigma)
    F.check(F.lib().dcp_fourier_gauss_2d(img.ptr, rptr, height, width, _row_stride(img), img.code, pad, code,
                                         *[t.ctypes.data_as(F.C.POINTER(F.C.c_double)) for t in taps], img.mem, img.device, img.stream))
    return res


def normalization_fft(mat, sigma=10, pad=100, mode='reflect'):
    """
    Correct a non-uniform background image using a Fourier Gaussian filter (reference ``preprocessing.py:131-158``).

    Parameters
    ----------
    mat : array_like
        2D array.  A NumPy array (or anything ``numpy.asarray`` takes), or a torch tensor on a ROCm device.
    sigma : int
        Sigma of the Gaussian.
    pad : int
        Pad width.
    mode : str
        Padding mode: "reflect", "symmetric", "edge", "wrap" or "constant".

    Returns
    -------
    array_like
        2D float64 array. Corrected background image.  NumPy input: the background plane comes from the GPU (:func:`_apply_fft_filter`)
        and the mean and the quotient are computed in NumPy as the reference writes them.  A device tensor: the plane is computed on
        torch's current stream, its mean is taken in float64 and the quotient is formed with torch; a float64 tensor is returned.
    """
    _check_fft_arguments(mat, sigma, pad, mode)
    mat, kind = _as_kind(mat, "normalization_fft takes NumPy arrays and torch tensors; use _apply_fft_filter for other device arrays")
    mat_bck = _apply_fft_filter(mat, sigma, pad, mode=mode)
    if kind == "torch":
        import torch
        mean_val = mat_bck.mean()
        return mean_val * mat.to(torch.float64) / mat_bck
    mean_val = np.mean(mat_bck)
    try:
        mat_cor = mean_val * mat / mat_bck
    except ZeroDivisionError:
        mat_bck[mat_bck == 0.0] = mean_val
        mat_cor = mean_val * mat / mat_bck
    return mat_cor


# --------------------------------------------------------------------------- the dot-pattern route

_CROSS = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], bool)
_MEASURED = ("bool", "uint8", "int8", "uint16", "int16")


def _new_like(img, shape, dtype):
    """(array, pointer): a fresh C-contiguous array of NumPy dtype ``dtype`` and of the kind of ``img``."""
    if img.torch:
        import torch
        out = torch.empty(shape, dtype=getattr(torch, np.dtype(dtype).name), device=img.keep.device)
        return out, out.data_ptr()
    if img.cai:
        out = F.DeviceArray(shape, dtype, img.device)
        return out, out.ptr
    out = np.empty(shape, dtype)
    return out, out.ctypes.data


def _to_host(img, arr):
    """NumPy copy of ``arr``, an array :func:`_new_like` made for ``img`` (after the work enqueued on the image's stream)."""
    if img.torch:
        return arr.cpu().numpy()
    if img.cai:
        F.check(F.lib().dcp_stream_synchronize(img.device, img.stream))
        return arr.copy_to_host()
    return arr


def _connectivity(structure):
    """4 or 8 for ``structure`` = None, the 3 x 3 cross or the 3 x 3 block (compared by value)."""
    if structure is None:
        return 4
    st = np.asarray(structure, dtype=bool)
    if st.ndim != 2:
        raise RuntimeError("structure and input must have equal rank")          # scipy's words
    if st.shape != (3, 3):
        raise ValueError("structure dimensions must be equal to 3")             # scipy's words
    if np.array_equal(st, _CROSS):
        return 4
    if st.all():
        return 8
    raise NotImplementedError("structure must be None, the 3 x 3 cross or the full 3 x 3 block")


def label(mat, structure=None):
    """
    Label the connected components of the nonzero pixels: ``scipy.ndimage.label(mat, structure)`` on the GPU.

    Parameters
    ----------
    mat : array_like
        2D array (NumPy array, ROCm torch tensor or ``__cuda_array_interface__`` device array) of any real element type.  A pixel
        is set where it is nonzero (NaN is, ``-0.0`` is not).  A view whose rows are strided is read in place.
    structure : array_like, optional
        None or the 3 x 3 cross (4-connectivity), or the full 3 x 3 block (8-connectivity).

    Returns
    -------
    labels : array_like
        2D int32 array of the input's kind: 0 for background, 1..num numbered as scipy numbers them.
    num : int
        Number of components.
    """
    if _is_complex(mat):
        raise TypeError("Complex type not supported")
    conn = _connectivity(structure)
    img = _rows_image(mat)
    height, width = img.shape
    labels, lptr = _new_like(img, (height, width), np.int32)
    if height == 0 or width == 0:
        return labels, 0
    F.require_device()
    num = ctypes.c_int(0)
    F.check(F.lib().dcp_label_2d(img.ptr, lptr, height, width, _row_stride(img), img.code, conn, ctypes.byref(num), img.mem, img.device,
                                 img.stream))
    return labels, int(num.value)


def binary_fill_holes(mat):
    """
    Fill the holes of the nonzero pixels: ``scipy.ndimage.binary_fill_holes(mat)`` (default structure) on the GPU.

    Parameters
    ----------
    mat : array_like
        2D array of any real element type, as for :func:`label`.

    Returns
    -------
    array_like
        2D bool array of the input's kind: the nonzero pixels and every region of zeros that reaches no border through its
        4-neighbours.
    """
    img = _real_plane(mat)
    height, width = img.shape
    res, rptr = _new_like(img, (height, width), np.bool_)
    if height == 0 or width == 0:
        return res
    F.require_device()
    F.check(F.lib().dcp_fill_holes_2d(img.ptr, rptr, height, width, _row_stride(img), img.code, img.mem, img.device, img.stream))
    return res


def _is_device(a):
    return (_is_torch(a) and a.is_cuda) or _is_cai(a)


_WIDE_LABELS = "labels outside the int32 range are not implemented: the kernels' labels are int32 (scipy's own label type)"


def _int32_labels(labels):
    """``labels`` as int32, read in place where it is; a wider plane is converted after a check that no value would wrap."""
    lo, hi = np.iinfo(np.int32).min, np.iinfo(np.int32).max
    if _is_torch(labels):
        import torch
        if labels.dtype == torch.int32:
            return labels
        if labels.is_floating_point() or labels.is_complex():
            raise TypeError("labels must be integers")
        if labels.element_size() >= 4 and labels.numel() and (int(labels.min()) < lo or int(labels.max()) > hi):
            raise NotImplementedError(_WIDE_LABELS)
        return labels.to(torch.int32)
    if _is_cai(labels):
        if np.dtype(labels.__cuda_array_interface__["typestr"]) != np.dtype(np.int32):
            raise TypeError("a device array of labels must be int32")
        return labels
    labels = np.asarray(labels)
    if labels.dtype.kind not in "iub":
        raise TypeError("labels must be integers")
    if labels.dtype == np.dtype(np.int32):
        return labels
    if labels.dtype.itemsize >= 4 and labels.size and (int(labels.min()) < lo or int(labels.max()) > hi):
        raise NotImplementedError(_WIDE_LABELS)
    return labels.astype(np.int32)


def _max_label(limg):
    if limg.torch:
        return int(limg.keep.max().item()) if limg.keep.numel() else 0
    if limg.cai:
        return None
    return int(limg.keep.max()) if limg.keep.size else 0


def _measures(mat, labels, num=None, top=None):
    """One call of ``dcp_label_measures_2d``: ``(sums, boxes)`` as NumPy arrays of shape (num, 4) for the labels 1..num -- int64 pixel
    count, sum v, sum y v, sum x v and int32 min y, max y, min x, max x.  ``mat`` None: every pixel weighs 1.  ``num`` None: the greatest
    label; a greater ``num`` is cut down to it (the labels above are absent).  ``top``: the greatest label where the caller knows it
    (the count :func:`label` returned) -- the plane is then not searched for it."""
    if labels is None:
        raise NotImplementedError("labels=None is not implemented: pass the label plane")
    if mat is not None:
        if _is_complex(mat):
            raise TypeError("Complex type not supported")
        if _is_device(mat) != _is_device(labels):
            raise ValueError("the image and its labels must both be host arrays or both be device arrays")
        wimg = _rows_image(mat)
        if wimg.code not in [F.DTYPE_BY_NAME[name] for name in _MEASURED]:
            raise NotImplementedError("measurements take bool and 8- / 16-bit integer images (their sums are exact); got %s" % (wimg.dtype,))
    limg = _rows_image(_int32_labels(labels))
    if mat is not None and wimg.shape != limg.shape:
        raise ValueError("input and labels must have the same shape")
    if top is None:
        top = _max_label(limg)
    if num is None:
        if top is None:
            raise NotImplementedError("give the labels to measure: the greatest label of a plain device array is not read back")
        num = top
    elif top is not None:
        num = min(int(num), top)
    num = max(int(num), 0)
    height, width = limg.shape
    if num == 0 or height == 0 or width == 0:
        boxes = np.empty((num, 4), np.int32)
        boxes[:] = (height, -1, width, -1)
        return np.zeros((num, 4), np.int64), boxes
    F.require_device()
    sums, sptr = _new_like(limg, (num, 4), np.int64)
    boxes, bptr = _new_like(limg, (num, 4), np.int32)
    F.check(F.lib().dcp_label_measures_2d(wimg.ptr if mat is not None else None, limg.ptr, height, width,
                                          _row_stride(wimg) if mat is not None else width, _row_stride(limg),
                                          wimg.code if mat is not None else F.DTYPE_BY_NAME["uint8"], num, sptr, bptr, limg.mem, limg.device,
                                          limg.stream))
    return _to_host(limg, sums), _to_host(limg, boxes)


def _index_array(index):
    """(int64 array of the labels asked for, None for "all labels > 0")."""
    if index is None:
        return None
    idx = np.asarray(index)
    if idx.dtype.kind not in "iub" and idx.size:
        raise TypeError("index must be an integer or a sequence of integers")
    idx = idx.astype(np.int64)
    if idx.size and idx.min() < 1:
        raise NotImplementedError("index values below 1 (the background) are not measured")
    return idx


def _gather(sums, idx):
    """Rows of ``sums`` for the labels ``idx`` (zeros for a label beyond the table: it has no pixels)."""
    out = np.zeros(idx.shape + (4,), np.int64)
    have = idx <= sums.shape[0]
    out[have] = sums[idx[have] - 1]
    return out


def sum_labels(mat, labels=None, index=None):
    """
    Sum of the values of ``mat`` over the pixels of each label: ``scipy.ndimage.sum_labels`` (``ndi.sum``) on the GPU.

    ``mat`` is a 2D bool or 8- / 16-bit integer image, ``labels`` the label plane (any integers; int32 is read in place), ``index`` a
    label, a sequence of labels (each >= 1) or None for all pixels with a label above 0.  Returns float64 as scipy does: a scalar for
    a scalar index, else an array of the index's shape.  The sums are accumulated in int64 on the GPU, so they are exact.
    """
    idx = _index_array(index)
    sums, _ = _measures(mat, labels, None if idx is None else (int(idx.max()) if idx.size else 0))
    if idx is None:
        return np.float64(sums[:, 1].sum())
    res = _gather(sums, idx)[..., 1].astype(np.float64)
    return res[()] if res.ndim == 0 else res


def _centroids(sums, idx):
    """scipy's return value of center_of_mass for the labels ``idx`` (an int64 array) from the table of :func:`_measures`."""
    rows = _gather(sums, idx).astype(np.float64)
    norm = rows[..., 1]
    results = [rows[..., 2] / norm, rows[..., 3] / norm]
    if idx.ndim == 0:
        return tuple(r[()] for r in results)
    return [tuple(v) for v in np.array(results).T]


def _slices(boxes, length):
    """scipy's return value of find_objects, ``length`` entries, from the boxes of :func:`_measures`."""
    found = [None if b[1] < 0 else (slice(int(b[0]), int(b[1]) + 1, None), slice(int(b[2]), int(b[3]) + 1, None)) for b in boxes]
    return found + [None] * (length - len(found))


def center_of_mass(mat, labels=None, index=None):
    """
    Centre of mass of the values of ``mat`` over each label: ``scipy.ndimage.center_of_mass`` on the GPU.

    Arguments as for :func:`sum_labels`.  Returns a tuple ``(y, x)`` for a scalar index (or None), else a list of such tuples, as scipy
    does; each coordinate is ``float64(sum y v) / float64(sum v)`` of exact integer sums -- scipy's own quotient bit for bit.  A label
    without pixels (or of weight 0) divides 0 by 0: NaN and NumPy's warning, as in scipy.
    """
    idx = _index_array(index)
    sums, _ = _measures(mat, labels, None if idx is None else (int(idx.max()) if idx.size else 0))
    if idx is None:
        tot = sums.sum(axis=0)
        norm = np.float64(tot[1])
        return (np.float64(tot[2]) / norm, np.float64(tot[3]) / norm)
    return _centroids(sums, idx)


def find_objects(labels, max_label=0):
    """
    Bounding boxes of the labels: ``scipy.ndimage.find_objects`` on the GPU.

    Returns a list of length ``max_label`` (the greatest label if below 1): entry ``j - 1`` is ``(slice(y0, y1), slice(x0, x1))`` of
    label ``j``, or None where no pixel carries it.
    """
    max_label = operator.index(max_label)
    _, boxes = _measures(None, labels, None if max_label < 1 else max_label)
    return _slices(boxes, max(max_label, len(boxes)))


def check_num_dots(mat):
    """
    True when ``mat`` (2D binary array) holds fewer than 5 x 5 dots, too few for the parabolic fits; prints the reference's warning
    then (reference ``preprocessing.py:251-271``).  The dots are counted by :func:`label`.
    """
    _, num_dots = label(mat)
    if num_dots >= 5 * 5:
        return False
    print("WARNING!!! Number of detected dots: {}".format(num_dots))
    print("is not enough for the algorithm to work!")
    return True


def _binary_mask(mat):
    """uint8 mask of a 0 / 1 image of any dtype and kind; the reference's check (``preprocessing.py:991-993``) and its message, applied
    to every value."""
    msg = "Input not a binary image, e.i. maximum_value=1 and minimum value=0!!!"
    mat, kind = _as_kind(mat, "takes NumPy arrays and torch tensors; label other device arrays with label()")
    if kind == "torch":
        import torch
        if mat.numel() == 0 or mat.max() != 1.0 or mat.min() != 0.0 or not bool(((mat == 0) | (mat == 1)).all()):
            raise ValueError(msg)
        return (mat != 0).to(torch.uint8)
    if np.max(mat) != 1.0 or np.min(mat) != 0.0:
        raise ValueError(msg)
    if not np.all((mat == 0) | (mat == 1)):
        raise ValueError(msg)
    return (mat != 0).astype(np.uint8)


def get_points_dot_pattern(mat, binarize=True, ratio=0.3, thres=None):
    """
    The (y, x) centroids of the dots of a binary image, an (N, 2) array in label order (reference ``preprocessing.py:966-997``).

    ``mat`` is a 2D image of any dtype that holds only 0 and 1 (NumPy array or torch tensor); anything else raises the reference's
    ``ValueError``.  It is labelled and measured on the GPU as a uint8 mask, which for the values 0 and 1 is the reference's
    arithmetic.  ``binarize`` must be False: the reference's default (with ``ratio`` and ``thres``) raises ``NotImplementedError``
    here.  Binarize first -- ``get_points_dot_pattern(binarization(mat, ratio, thres), binarize=False)`` -- with :func:`binarization`.
    """
    if binarize:
        raise NotImplementedError("binarize=True rests on scikit-image's Otsu threshold (threshold_otsu), clear_border and opening, "
                                  "which are not implemented here: binarize the image first and pass binarize=False")
    mask = _binary_mask(mat)
    mat_label, num_dots = label(mask)
    sums, _ = _measures(mask, mat_label, num_dots, top=num_dots)          # (label() has just counted them: no search for the greatest)
    return np.asarray(_centroids(sums, np.arange(1, num_dots + 1)))


def _host_array(mat):
    mat, kind = _as_kind(mat)
    return mat.detach().cpu().numpy() if kind == "torch" else mat


def select_dots_based_size(mat, dot_size, ratio=0.3):
    """
    Keep the dots of a 2D binary image whose size lies within ``dot_size * (1 -/+ ratio)`` (reference ``preprocessing.py:332-360``).

    Returns an int16 NumPy array (also for a tensor).  The labels and their boxes come from the GPU; as in the reference, a dot's size
    is the sum over every pixel inside its box and a kept dot is copied box and all.
    """
    mat = _host_array(mat)
    lowest = np.clip(dot_size - ratio * dot_size, 0, None)
    highest = dot_size + ratio * dot_size
    labels, num_dots = label(np.int16(mat))
    _, boxes = _measures(None, labels, num_dots, top=num_dots)
    kept = np.zeros_like(mat, dtype=np.int16)
    for box in _slices(boxes, num_dots):
        size = mat[box].sum()
        if (size >= lowest) and (size <= highest):
            kept[box] = mat[box]
    return kept


def select_dots_based_distance(mat, dot_dist, ratio=0.3):
    """
    Keep the dots one of whose three nearest neighbours lies within ``ratio`` (as a fraction of ``dot_dist``) above a whole multiple
    of ``dot_dist`` (reference ``preprocessing.py:422-457``).

    Returns an int16 NumPy array (also for a tensor).  Labels, boxes and centroids come from the GPU, and so do the squared distances
    from every centroid to its nearest ones (``dcp_nearest_sq_dists``: the operations NumPy performs for the reference's expression,
    so the same bits); their root, the test and the per-box copy are NumPy.  A centroid that is not finite raises ``ValueError``.
    """
    from .dotpattern import _nearest_sq
    mat = np.int16(_host_array(mat))
    labels, num_dots = label(mat)
    sums, boxes = _measures(mat, labels, num_dots, top=num_dots)          # boxes and centroids from one launch
    boxes = _slices(boxes, num_dots)
    cents = np.asarray(_centroids(sums, np.arange(1, num_dots + 1)))
    kept = np.zeros_like(mat)
    nearest = np.sqrt(_nearest_sq(cents))[:, 1:min(4, num_dots)]          # (the sorted row's [1:4]; fewer dots, fewer entries)
    for i, box in enumerate(boxes):
        dist = nearest[i]
        dist_error = (dist - (dist // dot_dist) * dot_dist) / dot_dist
        if any(dist_error < ratio):
            kept[box] = mat[box]
    return kept


# --------------------------------------------------------------------------- binarization

_HISTOGRAMMED = ("float32", "float64", "uint8", "int8", "uint16", "int16")


class _PlaneView:
    """A 2-D window of a device array (anything with ``__cuda_array_interface__``): ``view[y0:y1, x0:x1]`` is another window of the
    same allocation, read in place through its row stride."""

    def __init__(self, base):
        cai = base.__cuda_array_interface__
        self.base = getattr(base, "base", base)          # keeps the allocation alive
        self.dtype = np.dtype(cai["typestr"])
        self.shape = tuple(int(v) for v in cai["shape"])
        if len(self.shape) != 2:
            raise ValueError("expected a 2-D array")
        st = cai.get("strides")
        self.strides = tuple(int(v) for v in st) if st is not None else (self.shape[1] * self.dtype.itemsize, self.dtype.itemsize)
        self.ptr = int(cai["data"][0])
        self.stream = cai.get("stream")

    @property
    def __cuda_array_interface__(self):
        cai = {"shape": self.shape, "typestr": self.dtype.str, "data": (self.ptr, False), "version": 3, "strides": self.strides}
        if self.stream is not None:
            cai["stream"] = self.stream
        return cai

    def __getitem__(self, key):
        if not (isinstance(key, tuple) and len(key) == 2 and all(isinstance(k, slice) for k in key)):
            raise IndexError("a device plane takes two slices")
        view = _PlaneView(self)
        for axis, k in enumerate(key):
            start, stop, step = k.indices(self.shape[axis])
            if step != 1:
                raise IndexError("a device plane takes slices of step 1")
            view.ptr += start * self.strides[axis]
            view.shape = view.shape[:axis] + (max(stop - start, 0),) + view.shape[axis + 1:]
        return view


def _abs_plane(img):
    """``np.abs`` of the plane of ``img`` (an :class:`_Image`) as a fresh array of its kind; unsigned and bool planes come back as they are."""
    if np.dtype(_np_name(img)).kind in "ub":
        return img.keep
    height, width = img.shape
    res, rptr = _new_like(img, (height, width), _np_name(img))
    F.check(F.lib().dcp_abs_2d(img.ptr, rptr, height, width, _row_stride(img), img.code, img.mem, img.device, img.stream))
    return res


def _np_name(img):
    """NumPy name of the element type of an :class:`_Image`."""
    return str(img.dtype).replace("torch.", "") if img.torch else np.dtype(img.dtype).name


def _minmax(img):
    """(minimum, maximum, number of non-finite elements) of the plane of ``img``; the first two as Python floats holding the element
    exactly (NaN where any element is NaN, as ``a.min()`` gives it).  Waits for the image's stream."""
    out = (ctypes.c_double * 2)()
    bad = ctypes.c_int64(0)
    height, width = img.shape
    F.check(F.lib().dcp_minmax_2d(img.ptr, height, width, _row_stride(img), img.code, out, ctypes.byref(bad), img.mem, img.device, img.stream))
    return out[0], out[1], int(bad.value)


def _histogram(img, nbins, edges=None, first=0):
    """int64 counts of the plane of ``img``: between the ``nbins + 1`` ``edges`` (a NumPy array of the plane's float type; the last bin
    closed) or, for 8- / 16-bit integers, per value from ``first``.  Waits for the image's stream."""
    counts = np.empty(nbins, np.int64)
    height, width = img.shape
    if edges is not None:
        edges = np.ascontiguousarray(edges, dtype=_np_name(img))
        assert edges.shape == (nbins + 1,)
    F.check(F.lib().dcp_histogram_2d(img.ptr, height, width, _row_stride(img), img.code, None if edges is None else edges.ctypes.data, nbins,
                                     int(first), counts.ctypes.data, img.mem, img.device, img.stream))
    return counts


def _threshold_plane(img, thres):
    """(uint8 plane of ``(double)a > thres`` of the kind of ``img``, the exact number of set pixels).  Waits for the image's stream."""
    height, width = img.shape
    mask, mptr = _new_like(img, (height, width), np.uint8)
    if img.mem == F.MEM_HOST:          # the count is a word of the memory the plane is in
        count = np.zeros(1, np.int64)
        cptr = count.ctypes.data
    elif img.torch:
        import torch
        count = torch.zeros(1, dtype=torch.int64, device=img.keep.device)
        cptr = count.data_ptr()
    else:
        count = F.DeviceArray((1,), np.int64, img.device).copy_from_host(np.zeros(1, np.int64))
        cptr = count.ptr
    F.check(F.lib().dcp_threshold_2d(img.ptr, mptr, height, width, _row_stride(img), img.code, float(thres), cptr, img.mem, img.device, img.stream))
    return mask, int(_to_host(img, count)[0])


def _clear_border_plane(img, invert=False, conn=8):
    """uint8 plane of the kind of ``img``: its nonzero (``invert``: zero) pixels whose component (``conn`` 4 or 8) touches no border."""
    height, width = img.shape
    res, rptr = _new_like(img, (height, width), np.uint8)
    F.check(F.lib().dcp_clear_border_2d(img.ptr, rptr, height, width, _row_stride(img), img.code, conn, 1 if invert else 0, img.mem, img.device,
                                        img.stream))
    return res


def _morph_plane(img, op):
    """Erosion (0), dilation (1) or opening (2) by the 3 x 3 cross of the uint8 / bool plane of ``img``, as a uint8 plane of its kind."""
    height, width = img.shape
    res, rptr = _new_like(img, (height, width), np.uint8)
    F.check(F.lib().dcp_morph_cross_2d(img.ptr, rptr, height, width, _row_stride(img), op, img.mem, img.device, img.stream))
    return res


def _select_roi(mat, ratio, square=False):
    """
    The region of interest around the middle of an image (reference ``preprocessing.py:161-191``): a view, never a copy.

    ``mat`` is a 2D array, tensor or device plane, ``ratio`` the ROI's size over the image's (clipped to [0.05, 1]); ``square``
    selects a square of that ratio of the shorter side.
    """
    (height, width) = mat.shape
    ratio = np.clip(ratio, 0.05, 1.0)
    if square is True:
        c_hei = height // 2
        c_wid = width // 2
        radi = int(ratio * min(height, width)) // 2
        return mat[c_hei - radi:c_hei + radi, c_wid - radi:c_wid + radi]
    depad_hei = int((height - ratio * height) / 2)
    depad_wid = int((width - ratio * width) / 2)
    return mat[depad_hei:height - depad_hei, depad_wid:width - depad_wid]


def _invert_dots_contrast(mat):
    """
    Invert a 2D binary array (NumPy array or torch tensor) where more than half of it is set, so that dots are white (reference
    ``preprocessing.py:194-213``).  The set pixels are counted on the GPU and the test is ``2 * count > height * width`` in integers;
    the reference's float32 ``np.sum`` is exact below 2**24 set pixels and may round above.
    """
    mat, _ = _as_kind(mat)
    (height, width) = mat.shape
    if height == 0 or width == 0:
        return mat
    F.require_device()
    _, count = _threshold_plane(_real_plane(mat), 0.0)
    if 2 * count > height * width:
        mat = mat.max() - mat
    return mat


def threshold_otsu(image, nbins=256):
    """
    Otsu's threshold of a 2D image: scikit-image's ``threshold_otsu(image, nbins)`` restated through NumPy.

    Parameters
    ----------
    image : array_like
        2D array (NumPy array, ROCm torch tensor or device array) of float32 / float64 or an 8- / 16-bit integer type; a strided
        view (a region of interest) is read in place.
    nbins : int
        Number of bins of a float image's histogram (integer images are counted per value).

    Returns
    -------
    NumPy scalar
        The centre of the bin that maximises the between-class variance: for floats a centre of ``np.histogram(image, nbins)``, of
        the image's type; for integers a value of ``arange(min, max + 1)``.  A constant image returns its value.  Minimum, maximum
        and the int64 counts come from the GPU; the formula runs in NumPy float64 on the counts.  A NaN or an infinity raises
        NumPy's ``ValueError("autodetected range of [..] is not finite")``, a range too narrow for ``nbins`` bins its ``ValueError("Too
        many bins for data range...")``.
    """
    img = _real_plane(image)
    nbins = operator.index(nbins)
    if nbins < 1:
        raise ValueError("`bins` must be positive, when an integer")          # NumPy's words
    name = _np_name(img)
    if name not in _HISTOGRAMMED:
        raise NotImplementedError("threshold_otsu takes float32 / float64 and 8- / 16-bit integer images; got %s" % name)
    dt = np.dtype(name)
    height, width = img.shape
    if height == 0 or width == 0:
        raise ValueError("threshold_otsu of an empty image")
    F.require_device()
    lo, hi, bad = _minmax(img)
    first, last = dt.type(lo), dt.type(hi)
    if bad:
        raise ValueError("autodetected range of [{}, {}] is not finite".format(first, last))
    if first == last:
        return first
    if dt.kind == "f":
        if nbins > 65536:
            raise NotImplementedError("at most 65536 bins")
        edges = np.linspace(first, last, nbins + 1, endpoint=True, dtype=dt)
        if np.any(edges[:-1] >= edges[1:]):
            raise ValueError(f'Too many bins for data range. Cannot create {nbins} finite-sized bins.')
        counts = _histogram(img, nbins, edges=edges)
        centres = (edges[:-1] + edges[1:]) / 2
    else:
        counts = _histogram(img, int(last) - int(first) + 1, first=int(first))
        centres = np.arange(int(first), int(last) + 1)
    return _otsu_of_counts(counts, centres)


def _otsu_of_counts(counts, centres):
    """The published Otsu formula on a histogram, in float64: the centre that maximises the between-class variance."""
    c = counts.astype(np.float64)
    w1 = np.cumsum(c)
    w2 = np.cumsum(c[::-1])[::-1]
    m1 = np.cumsum(c * centres) / w1
    m2 = (np.cumsum((c * centres)[::-1]) / w2[::-1])[::-1]
    v = w1[:-1] * w2[1:] * (m1[:-1] - m2[1:]) ** 2
    return centres[np.argmax(v)]


def clear_border(mat):
    """
    Set every 8-connected component of the nonzero pixels that touches the image border to 0: scikit-image's
    ``clear_border(mat)`` for a binary image, restated as ``scipy.ndimage.label`` with the full 3 x 3 structure.

    ``mat`` is a 2D NumPy array or torch tensor of any real element type; the result has its kind and dtype.  Only binary use is
    promised; ``buffer_size``, ``bgval`` and ``mask`` are not taken.
    """
    if _is_complex(mat):
        raise TypeError("Complex type not supported")
    mat, kind = _as_kind(mat)
    img = _rows_image(mat)
    if img.shape[0] == 0 or img.shape[1] == 0:
        return mat.clone() if kind == "torch" else mat.copy()
    F.require_device()
    keep = _clear_border_plane(img)
    if kind == "torch":
        import torch
        return torch.where(keep != 0, mat, torch.zeros_like(mat))
    return np.where(keep != 0, mat, mat.dtype.type(0))


def _cross_footprint(footprint):
    if footprint is None:
        return
    fp = np.asarray(footprint)
    if fp.shape != (3, 3) or not np.array_equal(fp != 0, _CROSS):
        raise NotImplementedError("footprint must be None or the 3 x 3 cross (skimage.morphology.disk(1))")


def opening(mat, footprint=None):
    """
    Morphological opening by the 3 x 3 cross: scikit-image's ``opening(mat, disk(1))``, restated as
    ``scipy.ndimage.grey_opening(mat, footprint=cross, mode="reflect")`` (what lies outside the image is ignored).

    ``mat`` is a 2D NumPy array or torch tensor: uint8 / bool of any values, or a 0 / 1 plane of any other real type (anything else
    raises ``ValueError``).  ``footprint`` is None or the cross; another one raises ``NotImplementedError``.  The result has the
    input's kind and dtype.
    """
    _cross_footprint(footprint)
    if _is_complex(mat):
        raise TypeError("Complex type not supported")
    mat, kind = _as_kind(mat)
    img = _rows_image(mat)
    if img.shape[0] == 0 or img.shape[1] == 0:
        return mat.clone() if kind == "torch" else mat.copy()
    F.require_device()
    if _np_name(img) in ("uint8", "bool"):
        res = _morph_plane(img, 2)
        if _np_name(img) == "bool":
            res = res != 0
        return res
    if not bool(((mat == 0) | (mat == 1)).all()):
        raise ValueError("opening takes uint8 / bool images or 0 / 1 planes of another type")
    if kind == "torch":
        import torch
        return _morph_plane(_rows_image((mat != 0).to(torch.uint8)), 2).to(mat.dtype)
    return _morph_plane(_rows_image((mat != 0).astype(np.uint8)), 2).astype(mat.dtype)


def _thres_double(thres, name):
    """The double the threshold kernel compares with, for a threshold given against an image of NumPy type ``name`` as NumPy 2 compares
    it: a Python number is weak (rounded to a float image's own type), a NumPy scalar promotes the comparison and is exact in it."""
    if isinstance(thres, (bool, int, float)) and not isinstance(thres, np.generic) and np.dtype(name).kind == "f":
        return float(np.dtype(name).type(thres))
    return float(thres)


def binarization(mat, ratio=0.3, thres=None, denoise=True):
    """
    Apply a list of operations: binarizing an 2D array; inverting the contrast of dots if needs to; removing border components;
    cleaning salty noise; and filling holes (reference ``preprocessing.py:216-248``), every step on the GPU.

    Parameters
    ----------
    mat : array_like
        2D array.  A NumPy array (uploaded once; the result is downloaded once) or a ROCm torch tensor (every step on torch's
        current stream).  float32 / float64 or an 8- / 16-bit integer type where ``thres`` is None.
    ratio : float
        Used to select the ROI around the middle of the image for calculating threshold.
    thres : float, optional
        Threshold for binarizing. Automatically calculated if None (:func:`threshold_otsu` of the ROI, 512 bins).
    denoise : bool, optional
        Apply denoising to the image if True (the 2 x 2 median of the absolute values).

    Returns
    -------
    array_like
        2D binary int16 array of the input's kind.  Feed it to ``get_points_dot_pattern(..., binarize=False)``.
    """
    if _is_complex(mat):
        raise TypeError("Complex type not supported")
    mat, kind = _as_kind(mat)
    if len(mat.shape) != 2:
        raise ValueError("expected a 2-D array")
    height, width = mat.shape
    if height == 0 or width == 0:
        if kind == "torch":
            import torch
            return torch.zeros((height, width), dtype=torch.int16, device=mat.device)
        return np.zeros((height, width), np.int16)
    if kind == "numpy":
        host = _Image(mat, 2)          # (its checks, its byte order)
        if thres is None and _np_name(host) not in _HISTOGRAMMED:
            raise NotImplementedError("threshold_otsu takes float32 / float64 and 8- / 16-bit integer images; got %s" % _np_name(host))
        F.require_device()
        plane = _PlaneView(F.DeviceArray((height, width), host.dtype, host.device).copy_from_host(host.keep))
    else:
        if thres is None and str(mat.dtype).replace("torch.", "") not in _HISTOGRAMMED:
            raise NotImplementedError("threshold_otsu takes float32 / float64 and 8- / 16-bit integer images; got %s" % mat.dtype)
        F.require_device()
        plane = mat

    def view(a):
        return a if kind == "torch" else _PlaneView(a)

    if denoise:
        plane = view(median_filter(view(_abs_plane(_rows_image(plane))), (2, 2)))
    img = _rows_image(plane)
    if thres is None:
        thres = threshold_otsu(_select_roi(plane, ratio), nbins=512)
    mask, count = _threshold_plane(img, _thres_double(thres, _np_name(img)))
    mask = _clear_border_plane(_rows_image(mask), invert=2 * count > height * width)
    mask = _morph_plane(_rows_image(mask), 2)
    filled = binary_fill_holes(mask)
    if kind == "torch":
        import torch
        return filled.to(torch.int16)
    F.check(F.lib().dcp_stream_synchronize(img.device, img.stream))
    return np.int16(filled.copy_to_host())


# --------------------------------------------------------------------------- the rest of the dot-pattern route (prep.dotpattern)

from .dotpattern import (radon_padded, calc_size_distance, select_dots_based_ratio, calc_hor_slope, calc_ver_slope,  # noqa: E402,F401
                         group_dots_hor_lines, group_dots_ver_lines, remove_residual_dots_hor, remove_residual_dots_ver)
