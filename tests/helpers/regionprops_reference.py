"""The two axis lengths of ``skimage.measure.regionprops`` as its documentation defines them (no GPU, no scikit-image needed): the
independent check of ``discorpy_amd.prep.dotpattern._axis_lengths``, and the stand-in for ``regionprops`` when tools/gen_golden.py runs
the reference's ``select_dots_based_ratio``.  "The length of the major (minor) axis of the ellipse that has the same normalized second
central moments as the region": with the float64 central moments ``mu`` of the region's pixels about their float centroid, the inertia
tensor is ``[[mu02, -mu11], [-mu11, mu20]] / mu00`` and the lengths are ``4 sqrt(l)`` of its eigenvalues.  Nothing here comes from
scikit-image's source; agreement with a real scikit-image is UNVERIFIED.

The route differs from the code under test on purpose: float central moments and ``np.linalg.eigvalsh`` here, exact integer raw sums
and the closed form of a 2 x 2 eigenproblem there.
"""
import numpy as np


def axis_lengths(mat):
    """``(major_axis_length, minor_axis_length)`` of the nonzero pixels of the 2-D array ``mat``, all taken as one region."""
    ys, xs = np.nonzero(np.asarray(mat))
    ys, xs = ys.astype(np.float64), xs.astype(np.float64)
    m00 = float(len(ys))
    cy, cx = ys.sum() / m00, xs.sum() / m00
    dy, dx = ys - cy, xs - cx
    mu20, mu02, mu11 = (dy * dy).sum(), (dx * dx).sum(), (dy * dx).sum()
    tensor = np.array([[mu02, -mu11], [-mu11, mu20]], np.float64) / m00
    low, high = np.clip(np.linalg.eigvalsh(tensor), 0.0, None)
    return 4.0 * np.sqrt(high), 4.0 * np.sqrt(low)


class _Region:
    def __init__(self, mat):
        self.major_axis_length, self.minor_axis_length = axis_lengths(mat)


def regionprops(mat):
    """What the reference reads of ``skimage.measure.regionprops(mat)``: a list whose first entry has the two lengths (every nonzero
    pixel of ``mat`` as one region -- the reference passes the 0 / 1 plane of one box, whose only label is 1)."""
    return [_Region(mat)]
