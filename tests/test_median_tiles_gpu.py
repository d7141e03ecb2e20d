"""GPU suite for what tests/test_median_gpu.py cannot reach with scipy as its reference: every launch configuration of the median
filter (csrc/median_kernels.hip: tiles of 64 x 16 / 8 / 4 under the 64 KiB and the 160 KiB cap, the global kernel) on both sides of
every boundary of the chooser, windows that fold many times over a small image, floats at their edges (infinities, subnormals, zeros of
both signs, NaNs), degenerate windows, the global kernel for every element type, the memory around a device destination, and small
calls after a call that raised a kernel's dynamic-LDS limit.

Every comparison is byte equality with tests/helpers/median_reference.py, a NumPy restatement of the specification that selects floats
in IEEE total order (tests/test_median_reference_cpu.py checks it against scipy and against a literal loop, and ties the chooser's
tables used below to the constants in the source).  (21, 70) is the smallest frame with a partial tile in both axes for every tile
height: 21 is no multiple of 16, 8 or 4, and 70 columns are one full and one partial tile."""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import median_reference as mr  # noqa: E402

pytestmark = pytest.mark.gpu

ALL_DTYPES = ("float32", "float64", "uint8", "int8", "uint16", "int16", "uint32", "int32", "int64", "uint64", "bool")
FRAME = (21, 70)
FOLDS = [((3, 40), 31), ((5, 7), 51), ((2, 3), 51), ((1, 5), (1, 51)), ((4, 1), (9, 1)), ((2, 2), 171), ((3, 3), (2, 2))]
BY_KEY = {4: ("float32", "uint8"), 8: ("float64", "int64")}
SEEN = set()           # every kernel name a call of this file reported


def _seed(*key):
    """The same seed in every process (hash() of a string is not)."""
    return sum(ord(c) * (i + 1) for i, c in enumerate(repr(key))) % (1 << 31)


def _id(v):
    return "x".join(str(s) for s in v) if isinstance(v, tuple) else str(v)


@functools.lru_cache(maxsize=None)
def image(shape, dtype, kind):
    """kind "ties": integers 0..8 (heavy ties); "normal": standard_normal (negative values) with a block of zeros, scaled into the
    range of an integer type; "wide": draws over the whole range of an integer type, the 64-bit ones included (8-bit types: a noisy ramp over
    their whole range), plain standard_normal for floats -- no block of equal values, so the median depends on the position however often the window covers the image
    ("ties" gives 4 and "normal" 0 at every pixel once it covers it more than once).  Read-only: shared between tests."""
    rng = np.random.default_rng(_seed(shape, dtype, kind))
    dt = np.dtype(dtype)
    h, w = shape
    if kind == "ties":
        a = rng.integers(0, 9, size=shape).astype(dt)
    elif kind == "wide" and dt.kind == "f":
        a = rng.standard_normal(shape).astype(dt)
    elif kind == "normal":
        a = rng.standard_normal(shape)
        if dt.kind in "iu":
            info = np.iinfo(dt)
            a = np.clip(a * 40.0 + (128.0 if dt.kind == "u" else 0.0), info.min, info.max)
        a = a.astype(dt)
        a[h // 4:h // 4 + max(h // 2, 1), w // 4:w // 4 + max(w // 2, 1)] = 0
    elif dt.kind == "b":
        a = rng.random(shape) < 0.5
    elif dt.itemsize == 1:
        # (the median of thousands of uniform draws from 256 values is 127 or 128 everywhere: a ramp over the frame under the noise)
        y, x = np.mgrid[0:h, 0:w]
        a = 255.0 * (0.7 * x / max(w - 1, 1) + 0.3 * y / max(h - 1, 1)) + 12.0 * rng.standard_normal(shape)
        a = (np.clip(np.rint(a), 0, 255) + np.iinfo(dt).min).astype(dt)
    else:
        info = np.iinfo(dt)
        a = rng.integers(info.min, info.max, size=shape, endpoint=True, dtype=dt)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def want(shape, dtype, kind, size):
    out = mr.median_reference(image(shape, dtype, kind), size)
    out.setflags(write=False)
    return out


def varied(shape, dtype, size):
    """The expectation of the "wide" image, after checking that it can tell pixels apart: at least 8 distinct medians (a constant
    expectation would accept a kernel that reads a shifted window, a wrong box height or a wrong row pitch)."""
    ref = want(shape, dtype, "wide", size)
    assert len(np.unique(ref.view("u%d" % ref.itemsize))) >= 8, "the expected image of %s %s at %s is all but constant" % (shape, dtype, size)
    return ref


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def bits_of(dtype):
    return np.dtype(dtype).itemsize * 8


def key_bytes_of(dtype):
    return 8 if np.dtype(dtype).itemsize == 8 else 4


class DeviceView:
    """A strided view of a device allocation through ``__cuda_array_interface__`` (strides in bytes)."""

    def __init__(self, base, shape, strides, offset=0):
        self.base, self.shape, self.dtype = base, tuple(shape), base.dtype
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": base.dtype.str, "data": (base.ptr + offset, False),
                                         "version": 3, "strides": None if strides is None else tuple(strides)}


@pytest.fixture(scope="module")
def prep(hip):
    from discorpy_amd.prep import preprocessing
    return preprocessing


@pytest.fixture
def global_kernel(hip):
    """x_median_lds = 0 for the test, restored afterwards."""
    old = hip.get_option("x_median_lds")
    hip.set_option("x_median_lds", 0)
    try:
        yield hip
    finally:
        hip.set_option("x_median_lds", old)


@pytest.fixture(params=["default", "global"])
def routing(request, hip):
    """The default choice of a kernel, and again with x_median_lds = 0 (restored afterwards)."""
    old = hip.get_option("x_median_lds")
    hip.set_option("x_median_lds", 1 if request.param == "default" else 0)
    try:
        yield request.param
    finally:
        hip.set_option("x_median_lds", old)


def run(prep, hip, a, size, name=None, **kw):
    """One call; its kernel name is recorded and, where given, checked."""
    got = prep.median_filter(a, size, **kw)
    SEEN.add(hip.last_kernel())
    if name is not None:
        assert hip.last_kernel() == name, (hip.last_kernel(), name)
    return got


def expected_name(dtype, size, routing="default"):
    sy, sx = mr.window_sizes(size)
    th = mr.tile_rows(sy, sx, key_bytes_of(dtype))[0] if routing == "default" else 0
    return mr.kernel_name(bits_of(dtype), th)


# ------------------------------------------------------------------------------------ a. every launch configuration, every boundary

SQUARES = [(kb, s, th, dt) for kb in (4, 8) for s, th in mr.BOUNDARY_SIZES[kb] for dt in BY_KEY[kb]]


@pytest.mark.parametrize("key_bytes,size,th,dtype", SQUARES, ids=["%s-%d-%s" % (dt, s, "64x%d" % th if th else "global")
                                                                   for kb, s, th, dt in SQUARES])
def test_both_sides_of_every_boundary_of_the_chooser(prep, hip, key_bytes, size, th, dtype):
    """The table of tests/helpers/median_reference.py: the expected tile height is a literal there, not the chooser's answer."""
    name = mr.kernel_name(bits_of(dtype), th)
    for shape in [FRAME] + ([(16, 64)] if th in (8, 4) else []):           # (16, 64): exactly a whole number of tiles
        for kind in ("ties", "normal"):
            got = run(prep, hip, image(shape, dtype, kind), size, name)
            assert same_bytes(got, want(shape, dtype, kind, size)), (shape, kind)
        assert same_bytes(run(prep, hip, image(shape, dtype, "wide"), size, name), varied(shape, dtype, size)), shape


NONSQUARE = [(size, th, dt) for kb, size, th, cap in mr.NONSQUARE for dt in BY_KEY[kb]]


@pytest.mark.parametrize("size,th,dtype", NONSQUARE, ids=["%s-%s-64x%d" % (dt, _id(s), th) for s, th, dt in NONSQUARE])
def test_non_square_windows_under_either_cap(prep, hip, size, th, dtype):
    """A window per cap whose 16-row box misses the cap, and the wide and the tall line, (1, 301) and (301, 1): several folds of a
    21 x 70 frame, and at 8-byte keys a box of 161 792 bytes."""
    name = mr.kernel_name(bits_of(dtype), th)
    for kind in ("ties", "normal"):
        got = run(prep, hip, image(FRAME, dtype, kind), size, name)
        assert same_bytes(got, want(FRAME, dtype, kind, size)), kind
    assert same_bytes(run(prep, hip, image(FRAME, dtype, "wide"), size, name), varied(FRAME, dtype, size))


# ------------------------------------------------------------------------------------ b. many folds, both kernels

@pytest.mark.parametrize("dtype", ["float32", "uint16", "float64"])
@pytest.mark.parametrize("shape,size", FOLDS, ids=["%s-%s" % (_id(s), _id(k)) for s, k in FOLDS])
def test_windows_that_fold_many_times(prep, hip, routing, shape, size, dtype):
    """The index crosses several periods of 2 n: median_reflect's modulo in the LDS kernel, the walked index in the global one."""
    for kind in ("wide", "ties"):
        got = run(prep, hip, image(shape, dtype, kind), size, expected_name(dtype, size, routing))
        assert same_bytes(got, want(shape, dtype, kind, size)), kind


# ------------------------------------------------------------------------------------ c. float edges

@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_infinities_subnormals_and_zeros_of_both_signs(prep, hip, routing, dtype):
    a = mr.edge_image(dtype, FRAME, _seed("edge", dtype))
    for size in ((9, 5), 3, (2, 2)):
        ref = mr.median_reference(a, size)
        zeros = np.signbit(ref[ref == 0])
        assert zeros.sum() >= 50 and (~zeros).sum() >= 50, "the image no longer puts zeros of both signs at the median rank"
        got = run(prep, hip, a, size, expected_name(dtype, size, routing))
        assert same_bytes(got, ref), size                                  # bytes: -0.0 below +0.0


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_nans_stay_in_their_own_windows(prep, hip, routing, dtype):
    """Pixels whose window holds no NaN are untouched by the NaNs elsewhere; every other pixel returns one of its own window's
    elements.  Beyond that, the kernel's keys order NaNs as IEEE total order does (negative ones below -inf, positive ones above
    +inf, by payload), so those pixels are fully defined too: the last assertion pins that order, which the module's docstring
    states, where scipy leaves the outcome to the position of the NaNs."""
    a, mask = mr.nan_image(dtype, FRAME, _seed("nan", dtype))
    cells = a.view("u%d" % a.itemsize)
    for size in ((9, 5), 3, (2, 2)):
        ref = mr.median_reference(a, size)
        got = run(prep, hip, a, size, expected_name(dtype, size, routing))
        touched = np.zeros(FRAME, bool)
        for y in range(FRAME[0]):
            for x in range(FRAME[1]):
                touched[y, x] = mr.window_of(mask, y, x, size).any()
        assert 0 < touched.sum() < touched.size // 2                       # most windows hold none
        assert got[~touched].tobytes() == ref[~touched].tobytes(), size
        out = got.view(cells.dtype)
        for y, x in zip(*np.nonzero(touched)):
            assert out[y, x] in mr.window_of(cells, y, x, size), (size, y, x)
        assert same_bytes(got, ref), size
    assert np.isnan(mr.median_reference(a, 3)).sum() >= 2                  # the blocks' centres: a NaN of either sign is selected


# ------------------------------------------------------------------------------------ d. identity and degenerate windows

@pytest.mark.parametrize("dtype", ALL_DTYPES)
@pytest.mark.parametrize("shape", [(17, 65), (1, 1)], ids=_id)
def test_windows_of_one_and_two_elements(prep, hip, shape, dtype):
    a = image(shape, dtype, "wide")
    name = mr.kernel_name(bits_of(dtype), 16)
    assert same_bytes(run(prep, hip, a, 1, name), a)                        # rank 0 of one element: the input's bytes
    for size in ((1, 2), (2, 1)):
        assert same_bytes(run(prep, hip, a, size, name), want(shape, dtype, "wide", size)), size
    if shape != (1, 1):
        base = image((shape[0], shape[1] + 10), dtype, "wide")
        view = base[:, 3:-7]
        assert not view.flags.c_contiguous
        assert same_bytes(run(prep, hip, view, 1, name), view)


# ------------------------------------------------------------------------------------ e. the global kernel, every element type

@pytest.mark.parametrize("dtype", ALL_DTYPES)
@pytest.mark.parametrize("shape", [(5, 65), (4, 64)], ids=_id)
def test_global_kernel_every_element_type_and_its_own_tile_edges(prep, global_kernel, shape, dtype):
    """(5, 65) ends one row and one column inside the kernel's 64 x 4 tile, (4, 64) is exactly one."""
    for size in ((9, 5), (2, 2)):
        got = run(prep, global_kernel, image(shape, dtype, "wide"), size, mr.kernel_name(bits_of(dtype), 0))
        assert same_bytes(got, want(shape, dtype, "wide", size)), size


def test_global_kernel_selects_sixty_four_bit_integers_exactly(prep, global_kernel):
    rng = np.random.default_rng(5)
    for dt in (np.int64, np.uint64):
        info = np.iinfo(dt)
        a = rng.integers(info.min, info.max, size=(9, 11), endpoint=True, dtype=dt)
        a[2, 3:6] = info.max - np.arange(3).astype(dt)            # neighbours that one double cannot tell apart
        a[5, 1:4] = info.min + np.arange(3).astype(dt)
        got = run(prep, global_kernel, a, 3, "median_global_kernel<bits=64>")
        assert same_bytes(got, mr.median_reference(a, 3))


# ------------------------------------------------------------------------------------ f. nothing is written around the destination

def extremes(dtype):
    dt = np.dtype(dtype)
    info = np.finfo(dt) if dt.kind == "f" else np.iinfo(dt)
    return dt.type(info.min), dt.type(info.max)


@pytest.mark.parametrize("dtype,size,th", [("float32", 9, 16), ("float32", 92, 8), ("float32", 97, 4), ("float32", 172, 0),
                                           ("float64", 111, 4), ("uint8", (9, 5), 16)],
                         ids=lambda v: _id(v))
def test_nothing_is_written_around_a_device_destination(prep, hip, dtype, size, th):
    """The destination sits 37 elements into a room of sentinels; the source is a row-strided view whose skipped columns hold the
    type's extremes.  The frame's medians depend on the position (varied() checks that), so a source read at a wrong pitch or from
    a wrong first column, or a result stored at a wrong place, changes the frame."""
    dt = np.dtype(dtype)
    h, w = FRAME
    lead, pitch, left = 37, w + 10, 3
    a = image(FRAME, dtype, "wide")
    lo, hi = extremes(dtype)
    wide = np.empty((h, pitch), dt)
    wide[:, :left], wide[:, left + w:] = hi, lo
    wide[:, left:left + w] = a
    src = hip.DeviceArray(wide.shape, dt).copy_from_host(wide)
    sentinel = np.frombuffer(bytes([0xA5]) * ((h * w + 2 * lead) * dt.itemsize), dt)
    room = hip.DeviceArray(sentinel.shape, dt).copy_from_host(sentinel)
    before = room.copy_to_host().tobytes()
    assert before == sentinel.tobytes()
    out = DeviceView(room, FRAME, None, lead * dt.itemsize)
    view = DeviceView(src, FRAME, (pitch * dt.itemsize, dt.itemsize), left * dt.itemsize)
    assert run(prep, hip, view, size, mr.kernel_name(bits_of(dtype), th), out=out) is out
    got = room.copy_to_host()
    n = dt.itemsize
    assert got[:lead].tobytes() == before[:lead * n] and got[lead + h * w:].tobytes() == before[(lead + h * w) * n:]
    assert same_bytes(got[lead:lead + h * w].reshape(FRAME), varied(FRAME, dtype, size))
    assert same_bytes(src.copy_to_host(), wide)                            # and the source is as it was


# ------------------------------------------------------------------------------------ g. the raised limit is sticky and harmless

def test_small_calls_after_the_limit_of_their_kernel_was_raised(prep, hip):
    """One instantiation, float32 on the 64 x 16 tile: 9 (6 912 bytes), 101 (76 096: raises the limit), 9, 164 (162 532: raises it
    further), 9 -- and a call at a raised size on a stream that is not the default one."""
    name = "median_lds_kernel<bits=32, tile=64x16>"
    for size in (9, 101, 9, 164, 9):
        for kind in ("normal", "ties"):
            assert same_bytes(run(prep, hip, image(FRAME, "float32", kind), size, name), want(FRAME, "float32", kind, size)), size
        assert same_bytes(run(prep, hip, image(FRAME, "float32", "wide"), size, name), varied(FRAME, "float32", size)), size
    torch = pytest.importorskip("torch")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        t = torch.from_numpy(image(FRAME, "float32", "wide").copy()).to("cuda:0")
        big = run(prep, hip, t, 164, name)
        small = run(prep, hip, t, 9, name)
    stream.synchronize()
    assert same_bytes(big.cpu().numpy(), varied(FRAME, "float32", 164))
    assert same_bytes(small.cpu().numpy(), varied(FRAME, "float32", 9))


# ------------------------------------------------------------------------------------ the configurations this file reaches

def test_every_launch_configuration_is_reached(prep, hip):
    """One call per configuration, so that a change of the chooser cannot silently stop this file from covering one: the names are
    literals.  Prints every name the file's calls reported (the tests above included, where they ran in this process)."""
    required = {"median_lds_kernel<bits=32, tile=64x16>", "median_lds_kernel<bits=32, tile=64x8>", "median_lds_kernel<bits=32, tile=64x4>",
                "median_lds_kernel<bits=64, tile=64x16>", "median_lds_kernel<bits=64, tile=64x8>", "median_lds_kernel<bits=64, tile=64x4>",
                "median_global_kernel<bits=32>", "median_global_kernel<bits=64>",
                "median_lds_kernel<bits=8, tile=64x16>", "median_lds_kernel<bits=8, tile=64x8>", "median_lds_kernel<bits=8, tile=64x4>",
                "median_global_kernel<bits=8>", "median_lds_kernel<bits=16, tile=64x16>", "median_lds_kernel<bits=16, tile=64x4>",
                "median_global_kernel<bits=16>"}
    here = set()
    for dtype, sizes in (("float32", (91, 92, 97, 99, 165, 170, 172)), ("float64", (54, 55, 60, 63, 107, 111, 114)),
                         ("uint8", (91, 92, 97, 172)), ("uint16", (9, 171))):
        for size in sizes:
            got = run(prep, hip, image((16, 64), dtype, "wide"), size)
            here.add(hip.last_kernel())
            assert same_bytes(got, want((16, 64), dtype, "wide", size)), (dtype, size)
    old = hip.get_option("x_median_lds")
    hip.set_option("x_median_lds", 0)
    try:
        got = run(prep, hip, image((16, 64), "uint16", "wide"), 9)
        here.add(hip.last_kernel())
    finally:
        hip.set_option("x_median_lds", old)
    assert same_bytes(got, want((16, 64), "uint16", "wide", 9))
    print("kernel names observed by test_median_tiles_gpu.py:")
    for name in sorted(SEEN):
        print("   ", name)
    assert here == required, sorted(here ^ required)
