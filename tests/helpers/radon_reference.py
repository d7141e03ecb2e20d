"""NumPy restatement of what csrc/radon_kernels.hip computes, operation by operation (no GPU, no scikit-image needed): the oracle of
the Radon transform.  Written from the definition in DESIGN.md ("Radon transform"), which restates the documentation of
``skimage.transform.radon(image, theta, circle=True)``; nothing here comes from scikit-image's source, and agreement with a real
scikit-image is UNVERIFIED.

* :func:`crop_square`   the centred square of a non-square image: each axis starts at ``ceil(excess / 2)``
* :func:`angle_table`   ``{cos a, sin a, tx, ty}`` per angle, NumPy float64
* :func:`radon`         the sinogram: circle, rotation by bilinear interpolation with zeros outside, row sums in ascending order
"""
import numpy as np


def crop_square(image):
    """The centred ``min(shape)`` square of a 2-D array, as a view."""
    image = np.asarray(image)
    side = min(image.shape)
    starts = [int(np.ceil((n - side) / 2)) for n in image.shape]
    return image[starts[0]:starts[0] + side, starts[1]:starts[1] + side]


def angle_table(theta, side):
    """(A, 4) float64: ``ca, sa, tx, ty`` of every angle of ``theta`` (degrees) for a plane of ``side``."""
    c0 = side // 2
    a = np.deg2rad(np.asarray(theta, dtype=np.float64))
    ca, sa = np.cos(a), np.sin(a)
    tx = -c0 * (ca + sa - 1)
    ty = -c0 * (ca - sa - 1)
    return np.stack([ca, sa, tx, ty], axis=1)


def _tap(g, yf, xf):
    """``g[yf, xf]`` (float coordinates holding integers), 0.0 where an index lies outside the plane."""
    side = g.shape[0]
    ok = (yf >= 0.0) & (yf < side) & (xf >= 0.0) & (xf < side)
    yi = np.where(ok, yf, 0.0).astype(np.int64)
    xi = np.where(ok, xf, 0.0).astype(np.int64)
    return np.where(ok, g[yi, xi], 0.0)


def radon(image, theta=None, circle=True):
    """The (N, len(theta)) float64 sinogram of a 2-D float image (cropped to its centred square), ``theta`` in degrees."""
    if circle is not True:
        raise NotImplementedError("circle=False")
    image = crop_square(image)
    if theta is None:
        theta = np.arange(180)
    side = image.shape[0]
    c0 = side // 2
    rows = np.arange(side)
    inside = (rows[:, None] - c0) ** 2 + (rows[None, :] - c0) ** 2 <= c0 ** 2
    g = np.where(inside, image.astype(np.float64), 0.0)          # an assignment: what lies outside the circle is never read
    r = rows.astype(np.float64)[:, None]
    c = rows.astype(np.float64)[None, :]
    table = angle_table(theta, side)
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
            for k in range(1, side):                                # r = 0, 1, ..., N - 1: one rounded addition at a time
                acc = acc + v[k]
            sinogram[:, i] = acc
    return sinogram
