"""``calculate_threshold`` of ``discorpy.prep.preprocessing`` (reference ``preprocessing.py:816-853``) on the GPU.

The reference sorts every pixel of the image (``np.sort`` of the flattened array), shrinks the sorted list to ``max(mat.shape)`` points
with a cubic-spline ``scipy.ndimage.zoom(..., mode="nearest")``, fits a line through the middle half and reads the threshold off the
line's ends.  The first two steps are image-sized and run here as hand-written HIP kernels (``csrc/sort_kernels.hip``):

* :func:`sort_values`   ``np.sort(mat, axis=None)`` through ``dcp_sort_plane_2d``: a least-significant-digit radix sort on 8-bit digits
  of order-preserving integer keys.  Floats order as NumPy orders them, NaNs of either sign last.  Where NumPy leaves the order open it
  is fixed: ``-0.0`` before ``+0.0``, NaNs by payload, and a negative NaN comes out as the positive NaN of the same payload.
* :func:`zoom_sorted`   ``scipy.ndimage.zoom(values, out_len / len(values), order=3, mode="nearest")`` of a 1-D array through
  ``dcp_zoom_cubic_nearest_1d``: scipy 1.15's arithmetic restated, each output point filtering a window of 64 samples on either side of
  its four taps instead of the whole line (the start-up error is below 2**-121 of the window's magnitude).  float32 and integer results
  equal scipy's; float64 results lie within a few ulps of it (``tests/test_threshold_cpu.py`` has the figure).
* :func:`calculate_threshold`   the reference's function: a NumPy image is uploaded once, sort and zoom run on device buffers, only the
  ``max(mat.shape)`` zoomed values come back, and the trim, ``np.polyfit`` and the two closing formulas are the reference's NumPy.

Inputs are NumPy arrays, ROCm torch tensors (on torch's current stream) or ``__cuda_array_interface__`` device arrays; a view whose rows
are strided is read in place.  float32 / float64 and the 8- to 64-bit integers; bool raises ``NotImplementedError``, complex
``TypeError`` and float16 ``RuntimeError`` as elsewhere in the package.  There is no CPU path.
"""
import operator

import numpy as np

from .. import _ffi as F
from ..post.postprocessing import _Image
from .preprocessing import _PlaneView, _is_complex, _new_like, _np_name, _row_stride, _rows_image, _to_host

__all__ = ["sort_values", "zoom_sorted", "calculate_threshold"]


def _plane(mat):
    if _is_complex(mat):
        raise TypeError("Complex type not supported")
    img = _rows_image(mat)
    if _np_name(img) == "bool":
        raise NotImplementedError("bool images are not sorted: float32, float64 and the 8- to 64-bit integers only")
    return img


def _sort_plane(img):
    """The sorted elements of the plane of ``img`` as a fresh 1-D array of its kind (enqueued on the image's stream)."""
    height, width = img.shape
    res, rptr = _new_like(img, (height * width,), _np_name(img))
    F.check(F.lib().dcp_sort_plane_2d(img.ptr, rptr, height, width, _row_stride(img), img.code, img.mem, img.device, img.stream))
    return res


def _zoom_line(img, line, n, out_len):
    """``out_len`` zoomed values of the 1-D array ``line`` (``n`` elements at pointer ``line``), a fresh array of the kind of ``img``."""
    res, rptr = _new_like(img, (out_len,), _np_name(img))
    F.check(F.lib().dcp_zoom_cubic_nearest_1d(line, n, rptr, out_len, img.code, img.mem, img.device, img.stream))
    return res


def _pointer(img, arr):
    """Device or host pointer of an array :func:`_new_like` made for ``img``."""
    if img.torch:
        return arr.data_ptr()
    if img.cai:
        return arr.ptr
    return arr.ctypes.data


def sort_values(mat):
    """
    The elements of a 2D array in ascending order: ``np.sort(mat, axis=None)`` on the GPU.

    Parameters
    ----------
    mat : array_like
        2D array (NumPy array, ROCm torch tensor or ``__cuda_array_interface__`` device array) of float32 / float64 or an 8- to
        64-bit integer type.  A view whose rows are strided (``a[:, 3:-7]``) is read in place.

    Returns
    -------
    array_like
        1D array of the input's kind and dtype with ``mat.size`` elements.  NaNs of either sign come last (a negative NaN comes out
        positive), ``-0.0`` before ``+0.0``.
    """
    img = _plane(mat)
    height, width = img.shape
    if height == 0 or width == 0:
        return _new_like(img, (0,), _np_name(img))[0]
    F.require_device()
    return _sort_plane(img)


def zoom_sorted(values, out_len):
    """
    ``scipy.ndimage.zoom(values, out_len / len(values), order=3, mode="nearest")`` of a 1D array on the GPU.

    Parameters
    ----------
    values : array_like
        1D array (NumPy array, ROCm torch tensor or device array) of float32 / float64 or an 8- to 64-bit integer type, contiguous
        (a strided NumPy array or tensor is copied).  It need not be sorted.
    out_len : int
        Number of output points: what scipy computes as ``round(len(values) * zoom)``.

    Returns
    -------
    array_like
        1D array of ``out_len`` elements of the input's kind and dtype.
    """
    if _is_complex(values):
        raise TypeError("Complex type not supported")
    out_len = operator.index(out_len)
    line = _Image(values, 1)
    if _np_name(line) == "bool":
        raise NotImplementedError("bool arrays are not zoomed: float32, float64 and the 8- to 64-bit integers only")
    n = line.shape[0]
    if n < 1 or out_len < 1:
        raise ValueError("zoom_sorted needs at least one input and one output point")
    if line.strides[0] != 1 and n > 1:
        if line.cai:
            raise ValueError("device arrays must be contiguous")
        line = _Image(line.keep.contiguous() if line.torch else np.ascontiguousarray(line.keep), 1)
    F.require_device()
    return _zoom_line(line, line.ptr, n, out_len)


def calculate_threshold(mat, bgr="bright", snr=2.0):
    """
    Calculate a threshold value based on Algorithm 4 in Ref. [1] (reference ``preprocessing.py:816-853``).

    Parameters
    ----------
    mat : array_like
        2D array: NumPy array (uploaded once), ROCm torch tensor or device array.
    bgr : {"bright", "dark"}
        To indicate the brightness of the background against image features.
    snr : float
        Ratio (>1.0) used to separate image features against noise. Greater is less sensitive.

    Returns
    -------
    float
        Threshold value.

    References
    ----------
    [1] https://doi.org/10.1364/OE.26.028396
    """
    if _is_complex(mat):
        raise TypeError("Complex type not supported")
    if len(mat.shape) != 2:
        raise ValueError("expected a 2-D array")
    height, width = (int(v) for v in mat.shape)
    if height == 0 or width == 0:
        raise ValueError("calculate_threshold of an empty image")
    img = _plane(mat)
    F.require_device()
    if img.mem == F.MEM_HOST:          # one upload; sort and zoom then run on device buffers
        plane = _PlaneView(F.DeviceArray((height, width), np.dtype(img.dtype), img.device).copy_from_host(img.keep))
        img = _rows_image(plane)
    size = max(height, width)
    total = height * width
    npoint = int(round(total * (1.0 * size / total)))          # scipy's output length for the reference's zoom factor
    list_sort = _sort_plane(img)
    list_dsp = np.asarray(_to_host(img, _zoom_line(img, _pointer(img, list_sort), total, npoint)))
    return _threshold_of_profile(list_dsp, bgr, snr)


def _threshold_of_profile(profile, bgr, snr):
    """The host half of the reference's formula: a line through the middle half of the zoomed profile (a quarter dropped at the low end,
    a quarter and one point at the high end), its value at the first and last point, and half their distance times ``snr`` below the
    first (bright background) or above the last."""
    position = np.arange(0, len(profile), 1.0)
    quarter = int(0.25 * len(profile))
    middle = slice(quarter, -quarter - 1)
    slope, intercept = np.polyfit(position[middle], profile[middle], 1)[:2]
    y_end = intercept + slope * position[-1]
    noise_level = np.abs(y_end - intercept)
    if bgr == "bright":
        return intercept - noise_level * snr * 0.5
    return y_end + noise_level * snr * 0.5
