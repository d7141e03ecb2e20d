"""The contract of ``unwarp_image_forward`` in plain NumPy, written from the contract and not from any implementation: every source
pixel s = y * W + x goes to the rounded (half to even), clipped position the forward model gives it, a destination keeps the
GREATEST s that reaches it, destinations nobody reaches are zero, and pixels are moved, never computed with.  The coordinates are
evaluated in the reference's operation order (powers, products, one sum over the terms), so on frames where no coordinate lies
within rounding of a half-integer this IS the reference's result -- golden G21 pins that, tie cases included.

Also the inputs of golden G21 (``g21_input``): tools/gen_golden.py and the tests build them with this one function, the fixture
stores only the parameters and the reference's outputs."""
import numpy as np

G21_DTYPES = ("float32", "float64", "uint8", "int8", "uint16", "int16", "uint32", "int32", "int64", "uint64", "bool")
# name -> (shape, xcenter, ycenter, list_fact, seed); the two *tie* cases land on exact half-integers whatever the operation order
G21_CASES = {
    "expand": ((120, 180), 88.3, 61.7, [1.0, 1.0e-3, 2.0e-6], 2101),
    "compress": ((123, 177), 91.6, 58.2, [1.0, -1.5e-3, -2.0e-6], 2102),
    "offcentre_border": ((90, 140), 131.4, 12.6, [1.15, 4.0e-3], 2103),
    "one_pixel": ((30, 40), 17.3, 11.8, [0.0], 2104),
    "tie_half": ((41, 57), 0.0, 0.0, [0.5], 2105),
    "tie_quarter": ((37, 50), 4.0, 2.0, [0.25], 2106),
}
G21_TYPED = ((40, 52), 24.6, 20.3, [1.0, 5.0e-3, 3.0e-5], 2150)


def forward_destinations(height, width, xcenter, ycenter, list_fact):
    """(yu, xu, unrounded y, unrounded x): destination indices of every source pixel and the clipped coordinates they round."""
    xd, yd = np.meshgrid(np.arange(width) - xcenter, np.arange(height) - ycenter)
    rd = np.sqrt(xd ** 2 + yd ** 2)
    fact = np.zeros_like(rd)
    if len(list_fact):
        fact = np.sum(np.asarray([a * rd ** i for i, a in enumerate(list_fact)]), axis=0)
    xf = np.clip(xcenter + fact * xd, 0, width - 1)
    yf = np.clip(ycenter + fact * yd, 0, height - 1)
    return np.rint(yf).astype(np.int64), np.rint(xf).astype(np.int64), yf, xf


def unwarp_image_forward(mat, xcenter, ycenter, list_fact):
    mat = np.asarray(mat)
    height, width = mat.shape
    yu, xu, _, _ = forward_destinations(height, width, xcenter, ycenter, list_fact)
    winner = np.zeros(height * width, dtype=np.int64)                      # 0 = vacant, else source index + 1
    np.maximum.at(winner, (yu * width + xu).ravel(), np.arange(1, height * width + 1))
    out = np.zeros(height * width, dtype=mat.dtype)
    taken = winner > 0
    out[taken] = mat.reshape(-1)[winner[taken] - 1]
    return out.reshape(height, width)


def half_integer_margin(height, width, xcenter, ycenter, list_fact):
    """Smallest distance of any clipped, unrounded coordinate to a half-integer (0 on an exact tie)."""
    _, _, yf, xf = forward_destinations(height, width, xcenter, ycenter, list_fact)
    return float(min(np.abs(v - np.floor(v) - 0.5).min() for v in (yf, xf)))


def typed_frame(dtype, shape, seed):
    """A full-range frame of `dtype`; floats carry NaNs with payloads, infinities and -0.0 (the scatter must move them untouched)."""
    rng = np.random.default_rng(int(seed))
    dt = np.dtype(dtype)
    if dt == np.bool_:
        return rng.random(shape) < 0.5
    if dt.kind == "f":
        im = (rng.random(shape) * 2000.0 - 700.0).astype(dt)
        bits = im.view(np.uint32 if dt.itemsize == 4 else np.uint64).reshape(-1)
        quiet = 0x7FC00000 if dt.itemsize == 4 else 0x7FF8000000000000
        bits[5::37] = quiet | 0x1234                                        # quiet NaNs with a payload
        bits[7::41] = (quiet | 0x0BAD) | (1 << (8 * dt.itemsize - 1))       # ... and a sign
        bits[11::43] = 1 << (8 * dt.itemsize - 1)                           # -0.0
        im.reshape(-1)[13::47] = np.inf
        return im
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max, size=shape, endpoint=True, dtype=dt)


def g21_input(name):
    """(mat, xcenter, ycenter, list_fact) of case `name` of golden G21: a key of G21_CASES, "typed_<dtype>" or "complex64"."""
    if name in G21_CASES:
        shape, xc, yc, fact, seed = G21_CASES[name]
        return np.random.default_rng(seed).random(shape, dtype=np.float32) + np.float32(0.5), xc, yc, fact
    shape, xc, yc, fact, seed = G21_TYPED
    if name == "complex64":
        re, im = typed_frame("float32", shape, seed + 50), typed_frame("float32", shape, seed + 51)
        mat = np.empty(shape, np.complex64)
        mat.real, mat.imag = re, im
        return mat, xc, yc, fact
    dt = name[len("typed_"):]
    return typed_frame(dt, shape, seed + G21_DTYPES.index(dt)), xc, yc, fact


def g21_names():
    return list(G21_CASES) + ["typed_" + dt for dt in G21_DTYPES] + ["complex64"]
