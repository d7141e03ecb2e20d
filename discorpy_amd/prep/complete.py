"""Every public function of ``discorpy.prep.preprocessing`` under its name: the module a user swaps in.

    import discorpy_amd.prep.complete as prep          # was: import discorpy.prep.preprocessing as prep

The functions of :mod:`discorpy_amd.prep.preprocessing` re-exported as they are, :func:`calculate_threshold` of
:mod:`discorpy_amd.prep.threshold`, the point-list functions of :mod:`discorpy_amd.prep.pointgrid`, and one function of its own:
:func:`get_points_dot_pattern` with the reference's default ``binarize=True``, which :mod:`discorpy_amd.prep.preprocessing` refuses.
"""
import numpy as _np

from . import preprocessing as _pre
from .preprocessing import (normalization, normalization_fft, binarization, check_num_dots, calc_size_distance,  # noqa: F401
                            select_dots_based_size, select_dots_based_ratio, select_dots_based_distance, calc_hor_slope, calc_ver_slope,
                            group_dots_hor_lines, group_dots_ver_lines, remove_residual_dots_hor, remove_residual_dots_ver)
from .threshold import calculate_threshold  # noqa: F401
from .pointgrid import (make_parabola_mask, remove_points_using_parabola_mask, rotate_points, remove_subset_points,  # noqa: F401
                        group_dots_hor_lines_based_polyfit, group_dots_ver_lines_based_polyfit)

__all__ = ["normalization", "normalization_fft", "binarization", "check_num_dots", "calc_size_distance", "select_dots_based_size",
           "select_dots_based_ratio", "select_dots_based_distance", "calc_hor_slope", "calc_ver_slope", "group_dots_hor_lines",
           "group_dots_ver_lines", "remove_residual_dots_hor", "remove_residual_dots_ver", "calculate_threshold", "make_parabola_mask",
           "remove_points_using_parabola_mask", "get_points_dot_pattern", "rotate_points", "remove_subset_points",
           "group_dots_hor_lines_based_polyfit", "group_dots_ver_lines_based_polyfit"]


def get_points_dot_pattern(mat, binarize=True, ratio=0.3, thres=None):
    """
    Extract dot-centroids of a dot-pattern from a binary or grayscale image (reference ``preprocessing.py:966-997``).

    Parameters
    ----------
    mat : array_like
        2D array: a NumPy array or a ROCm torch tensor.
    binarize : bool, optional
        Binarize the image first (:func:`binarization` with ``ratio`` and ``thres``); the binary plane then stays on the GPU through
        labelling and measuring, and only the centroids come back.  False: ``mat`` must hold only 0 and 1.
    ratio : float
        Used to select the ROI around the middle of the image for calculating threshold.
    thres : float, optional
        Threshold for binarizing. Automatically calculated if None.

    Returns
    -------
    array_like
        (y, x)-coordinates of the dot centroids, an (N, 2) NumPy array in label order.
    """
    if not binarize:
        return _pre.get_points_dot_pattern(mat, binarize=False)
    mat, kind = _pre._as_kind(mat)
    # (element types torch has no full support for -- the wider unsigned integers -- take binarization's NumPy route: one download
    # of the int16 plane and one upload of the mask more, the same result)
    if kind == "numpy" and mat.ndim == 2 and mat.size and mat.dtype.name in ("float32", "float64", "uint8", "int8", "int16"):
        import torch
        _pre.F.require_device()
        host = _pre._Image(mat, 2).keep          # (its checks, its byte order)
        mat = torch.from_numpy(_np.ascontiguousarray(host)).to("cuda")          # one upload: every later step reads device planes
    return _pre.get_points_dot_pattern(binarization(mat, ratio=ratio, thres=thres), binarize=False)
