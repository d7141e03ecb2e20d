"""MI355X counterpart of the median-filter part of ``discorpy.prep.preprocessing``.

* :func:`normalization`   reference ``discorpy/prep/preprocessing.py:50-73``: same name, arguments and default
* :func:`median_filter`   the ``scipy.ndimage.median_filter(mat, size, mode="reflect")`` both :func:`normalization` (size 51) and the
  denoise step of the reference's ``binarization`` (size 2) rest on -- the one expensive image operation of that module

The rest of the reference's module (Otsu threshold, ``clear_border``, morphology, labelling, the Radon-based angle search) rests on
scikit-image and is out of scope here: there is nothing to compare an implementation against.

The median runs as a hand-written HIP kernel through ``dcp_median_filter_2d`` (``include/discorpy_hip.h``; the kernels are in
``csrc/median_kernels.hip``): it SELECTS the element of rank ``(size_y * size_x) // 2`` of every window by a binary search on
order-preserving integer keys, so the result is one of the input's elements, bit for bit -- what scipy returns.  There is no CPU
path: a missing library or GPU raises.  Inputs are NumPy arrays (staged through the GPU), ROCm torch tensors (zero-copy, on torch's
current stream) or ``__cuda_array_interface__`` device arrays, as in :mod:`discorpy_amd.post.postprocessing`.

Where this differs from scipy:

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
import operator

import numpy as np

from .. import _ffi as F
from ..post.postprocessing import _Image, _is_cai, _is_torch

__all__ = ["normalization", "median_filter"]


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
    img = _Image(mat, 2)
    if img.strides[1] != 1 and img.shape[1] > 1 or img.strides[0] < img.shape[1] and img.shape[0] > 1:
        if img.cai:
            raise ValueError("device arrays must have unit column stride and non-overlapping rows")
        img = _Image(img.keep.contiguous() if img.torch else np.ascontiguousarray(img.keep), 2)
    height, width = img.shape
    res, optr = img.empty((height, width), out=out)
    if height == 0 or width == 0:
        return res
    F.require_device()
    row_stride = img.strides[0] if height > 1 else width          # (a single row's stride is arbitrary)
    F.check(F.lib().dcp_median_filter_2d(img.ptr, optr, height, width, row_stride, img.code, sy, sx, img.mem, img.device, img.stream))
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
    if _is_torch(mat) and mat.is_cuda:
        import torch
        mat_bck = median_filter(mat, size)
        rtype = mat.dtype if mat.is_floating_point() else torch.float64
        mean_val = mat_bck.to(torch.float64).mean().to(rtype)
        return mean_val * mat.to(rtype) / mat_bck.to(rtype)
    if _is_cai(mat):
        raise TypeError("normalization takes NumPy arrays and torch tensors; use median_filter for other device arrays")
    mat = np.asarray(mat.detach().cpu().numpy() if _is_torch(mat) else mat)
    mat_bck = median_filter(mat, size)
    mean_val = np.mean(mat_bck)
    try:
        mat_cor = mean_val * mat / mat_bck
    except ZeroDivisionError:
        mat_bck[mat_bck == 0.0] = mean_val
        mat_cor = mean_val * mat / mat_bck
    return mat_cor
