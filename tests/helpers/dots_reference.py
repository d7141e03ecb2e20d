"""The dot-pattern functions of ``discorpy.prep.preprocessing`` restated on scipy alone (the reference module cannot be imported without
scikit-image): what ``discorpy_amd.prep.preprocessing`` must return, computed on the CPU.  Line numbers are the reference's.

Also the synthetic target of the tests: a grid of discs with two of them merged and one speck.
"""
import numpy as np
from scipy import ndimage as ndi

BINARY_ERROR = "Input not a binary image, e.i. maximum_value=1 and minimum value=0!!!"


def dot_grid(rows=7, cols=9, pitch=14, radius=4, dtype=np.float32):
    """rows x cols discs of `radius` on a `pitch`; the discs (2, 3) and (2, 4) are joined by a bar, a single pixel sits between two rows."""
    h, w = rows * pitch + 5, cols * pitch + 3
    y, x = np.mgrid[0:h, 0:w]
    m = np.zeros((h, w), bool)
    for r in range(rows):
        for c in range(cols):
            cy, cx = pitch // 2 + 2 + r * pitch, pitch // 2 + 1 + c * pitch
            m |= (y - cy) ** 2 + (x - cx) ** 2 <= radius * radius
    cy = pitch // 2 + 2 + 2 * pitch
    m[cy - 1:cy + 2, pitch // 2 + 1 + 3 * pitch:pitch // 2 + 1 + 4 * pitch] = True
    m[pitch + 2, 5 * pitch + 1] = True
    return m.astype(dtype)


def check_num_dots(mat):                                           # :251-271
    return ndi.label(mat)[1] < 5 * 5


def get_points_dot_pattern(mat):                                   # :990-997 with binarize=False
    if np.max(mat) != 1.0 or np.min(mat) != 0.0:
        raise ValueError(BINARY_ERROR)
    labels, num = ndi.label(np.int16(mat))
    return np.asarray(ndi.center_of_mass(mat, labels=labels, index=np.arange(1, num + 1)))


def select_dots_based_size(mat, dot_size, ratio=0.3):              # :351-360
    lo, hi = np.clip(dot_size - ratio * dot_size, 0, None), dot_size + ratio * dot_size
    labels, _ = ndi.label(np.int16(mat))
    out = np.zeros_like(mat, dtype=np.int16)
    for box in ndi.find_objects(labels):
        if lo <= mat[box].sum() <= hi:
            out[box] = mat[box]
    return out


def select_dots_based_distance(mat, dot_dist, ratio=0.3):          # :440-457
    mat = np.int16(mat)
    labels, num = ndi.label(mat)
    boxes = ndi.find_objects(labels)
    cent = np.asarray(ndi.center_of_mass(mat, labels=labels, index=np.arange(1, num + 1)))
    out = np.zeros_like(mat)
    for i, box in enumerate(boxes):
        dist = np.sort(np.sqrt((cent[i][0] - cent[:, 0]) ** 2 + (cent[i][1] - cent[:, 1]) ** 2))[1:4]
        num_steps = dist // dot_dist
        if any((dist - num_steps * dot_dist) / dot_dist < ratio):
            out[box] = mat[box]
    return out
