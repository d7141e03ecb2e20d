"""NumPy restatement of the Radon transform WITHOUT the circle (no GPU, no scikit-image needed): the oracle of
``discorpy_amd.prep.dotpattern.radon_padded`` / ``dcp_radon_padded_2d``.  Written from the definition in DESIGN.md ("Dot grid"), which
restates the documentation of ``skimage.transform.radon(image, theta, circle=False)``; nothing here comes from scikit-image's source, and
agreement with a real scikit-image is UNVERIFIED.

* :func:`padded_side`   ``S = int(ceil(sqrt(2) * max(H, W)))`` in float64
* :func:`pad_square`    the image in an S x S square of zeros, its first element at ``(S // 2 - H // 2, S // 2 - W // 2)``
* :func:`angle_table`   ``{cos a, sin a, tx, ty}`` per angle for the rotation about ``(S // 2, S // 2)``
* :func:`radon`         the sinogram of that square: bilinear interpolation between floor and ceil with 0.0 outside the square, the rows
  added in ascending order, all float64.  This one materialises the square; the kernel does not.
"""
import numpy as np


def padded_side(height, width):
    return int(np.ceil(np.sqrt(2) * max(height, width)))


def pad_square(image):
    """The (S, S) float64 square of zeros that holds ``image`` (2-D), and the image's corner in it."""
    image = np.asarray(image)
    height, width = image.shape
    side = padded_side(height, width)
    py, px = side // 2 - height // 2, side // 2 - width // 2
    square = np.zeros((side, side), np.float64)
    square[py:py + height, px:px + width] = image
    return square, (py, px)


def angle_table(theta, side):
    """(A, 4) float64: ``ca, sa, tx, ty`` of every angle of ``theta`` (degrees) for a square of ``side``."""
    c0 = side // 2
    a = np.deg2rad(np.asarray(theta, dtype=np.float64))
    ca, sa = np.cos(a), np.sin(a)
    tx = -c0 * (ca + sa - 1)
    ty = -c0 * (ca - sa - 1)
    return np.stack([ca, sa, tx, ty], axis=1)


def _tap(g, yf, xf):
    """``g[yf, xf]`` (float coordinates holding integers), 0.0 where an index lies outside the square."""
    side = g.shape[0]
    ok = (yf >= 0.0) & (yf < side) & (xf >= 0.0) & (xf < side)
    yi = np.where(ok, yf, 0.0).astype(np.int64)
    xi = np.where(ok, xf, 0.0).astype(np.int64)
    return np.where(ok, g[yi, xi], 0.0)


def radon(image, theta=None):
    """The (S, len(theta)) float64 sinogram of a 2-D float image of any shape, ``theta`` in degrees."""
    if theta is None:
        theta = np.arange(180)
    g, _ = pad_square(image)
    side = g.shape[0]
    rows = np.arange(side)
    r = rows.astype(np.float64)[:, None]
    c = rows.astype(np.float64)[None, :]
    table = angle_table(np.atleast_1d(theta), side)
    sinogram = np.empty((side, len(table)), np.float64)
    with np.errstate(all="ignore"):
        for i, (ca, sa, tx, ty) in enumerate(table):
            x = ca * c + sa * r + tx
            y = -sa * c + ca * r + ty
            x0, x1, y0, y1 = np.floor(x), np.ceil(x), np.floor(y), np.ceil(y)
            dx, dy = x - x0, y - y0
            top = (1 - dx) * _tap(g, y0, x0) + dx * _tap(g, y0, x1)
            bot = (1 - dx) * _tap(g, y1, x0) + dx * _tap(g, y1, x1)
            v = (1 - dy) * top + dy * bot
            acc = v[0].copy()
            for k in range(1, side):                                # r = 0, 1, ..., S - 1: one rounded addition at a time
                acc = acc + v[k]
            sinogram[:, i] = acc
    return sinogram
