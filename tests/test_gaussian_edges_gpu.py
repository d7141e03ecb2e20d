"""GPU suite for what the data of tests/test_gaussian_gpu.py cannot see of the Gaussian filter (csrc/gauss_kernels.hip): the order
of the additions, the pairing of the taps and the absence of fused multiply-adds in every element type (plateau images: an integer
result truncates a float64 sum that lies within a few ulp of the plateau's level, so a one-ulp change shows as L against L - 1;
tests/test_gaussian_reference_cpu.py holds on the CPU that each of those changes is visible on exactly these images), the three
element types that test never launches, tiles clear of every edge, radius 0, 1 and 192, both sides of the LDS cap, tall and thin
images, special floats, the memory around a device destination and small calls after a raised dynamic-LDS limit.

Every comparison is equality with scipy.ndimage.gaussian_filter; floats are compared on their bytes, so -0.0 is not +0.0.  Where an
input holds NaN or infinities, equality is NaN at the same positions and equal bytes everywhere else: sign and payload of a NaN
are not compared, because x86 and the GPU generate different default NaNs.  Every case runs under x_gauss_lds = 1, 2 and 0 and names
the kernels it expects."""
import functools

import numpy as np
import pytest
from scipy import ndimage as ndi

from helpers import gaussian_reference as G
from test_gaussian_gpu import CVAL, FUSED_MAX_LDS, FUSED_MAX_RADIUS, MODES, SUBSET_SHAPES, SUBSET_SIGMAS, image, lds_bytes, route  # noqa: F401
from test_median_tiles_gpu import DeviceView, extremes

pytestmark = pytest.mark.gpu

ALL_DTYPES = ["float32", "float64", "uint8", "int8", "uint16", "int16", "uint32", "int32", "int64", "uint64"]
PLATEAU_SHAPE, PLATEAU_BLOCK = (100, 300), (44, 50)
PLATEAU_SIGMAS = [3, (1, 5.3)]
LDS_CAP = 160 << 10                                     # kGaussLdsMax of csrc/gauss_kernels.hip
SEEN = set()                                            # every kernel name a call of this file reported


def _id(v):
    return "x".join(str(s) for s in v) if isinstance(v, tuple) else str(v)


@pytest.fixture(scope="module")
def lp(hip):
    from discorpy_amd.prep import linepattern
    return linepattern


def fused(dtype):
    return "gauss_lds_kernel<%s, tile=128x32>" % np.dtype(dtype).name


def both(dtype):
    return "gauss_axis_kernel<%s, axis=0> + gauss_axis_kernel<%s, axis=1>" % (np.dtype(dtype).name, np.dtype(dtype).name)


def one(dtype, axis):
    return "gauss_axis_kernel<%s, axis=%d>" % (np.dtype(dtype).name, axis)


def radii_of(sigma=None, radius=None):
    """(ry, rx) of a call; -1: the axis is skipped."""
    sig = (sigma, sigma) if np.ndim(sigma) == 0 else tuple(sigma)
    rad = (radius, radius) if radius is None or np.ndim(radius) == 0 else tuple(radius)
    return tuple(-1 if s <= 1e-15 else (int(4.0 * float(s) + 0.5) if r is None else r) for s, r in zip(sig, rad))


def names_for(dtype, ry, rx):
    """What x_gauss_lds = 1 (the default), 2 and 0 run at these radii: gauss_takes_lds of csrc/gauss_kernels.hip restated."""
    if ry < 0 and rx < 0:
        return {1: "gauss_copy", 2: "gauss_copy", 0: "gauss_copy"}
    if ry < 0 or rx < 0:
        name = one(dtype, 0 if ry >= 0 else 1)
        return {1: name, 2: name, 0: name}
    lds = lds_bytes(ry, rx, np.dtype(dtype).itemsize)
    default = max(ry, rx) <= FUSED_MAX_RADIUS and lds <= FUSED_MAX_LDS
    return {1: fused(dtype) if default else both(dtype), 2: fused(dtype) if lds <= LDS_CAP else both(dtype), 0: both(dtype)}


def same(got, ref):
    """Equal dtype, shape and bytes; where the expectation holds NaNs, NaN at the same positions and equal bytes elsewhere."""
    return G.same_but_for_nan_bits(got, ref)


def check(lp, hip, route, a, names=None, ref=None, what=(), values=(1, 2, 0), **kw):
    """One call per route of lp.gaussian_filter(a, **kw): the kernel's name against `names` (worked out from the radii where not
    given), the result against scipy's."""
    if names is None:
        names = names_for(a.dtype, *radii_of(kw.get("sigma"), kw.get("radius")))
    if ref is None:
        with np.errstate(all="ignore"):
            ref = ndi.gaussian_filter(np.asarray(a), **kw)
    for value in values:
        got = route(value, lambda: lp.gaussian_filter(a, **kw))
        SEEN.add(hip.last_kernel())
        assert hip.last_kernel() == names[value], (what, kw, value, hip.last_kernel(), names[value])
        assert same(got, ref), (what, kw, "x_gauss_lds = %d" % value, int((np.asarray(got) != ref).sum()))
    return ref


@functools.lru_cache(maxsize=None)
def plateau(shape, dtype):
    return G.plateau_image(shape, dtype, PLATEAU_BLOCK)


def wide_uint64(shape):
    """The normal data of tests/test_gaussian_gpu.py moved above 2^63 as int64 is moved to 2^40 there, with low bits set so that the
    read through a double rounds; every float64 result stays below 2^64."""
    a = image(shape, "uint16").astype(np.uint64)
    assert a.max() < 480
    out = (np.uint64(1) << np.uint64(63)) + (a << np.uint64(54)) + a * np.uint64(977) + np.uint64(1)
    assert out.min() > 2 ** 63 and float(out.max()) < 2.0 ** 64 - 2.0 ** 16 and (out.astype(np.float64).astype(np.uint64) != out).any()
    out.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------ B.1 plateaus: the order of operations, per type

def test_the_plateau_shape_has_a_tile_clear_of_every_edge_and_tiles_on_each():
    """gauss_lds_kernel's tile is 128 x 32: tile row 1 (rows 32..63) and tile column 1 (columns 128..255) of 100 x 300 stay at least
    32 pixels clear of every edge (radii up to 32 take the unchecked tap loop there under constant), and the first and last tile of
    either axis reach over one."""
    h, w = PLATEAU_SHAPE
    assert 32 - 32 >= 0 and 64 + 32 <= h and 128 - 32 >= 0 and 256 + 32 <= w
    assert (h + 31) // 32 == 4 and (w + 127) // 128 == 3
    assert PLATEAU_BLOCK[0] > 2 * 12 + 1 and PLATEAU_BLOCK[1] > 2 * 21 + 1          # wider than the windows of sigma 3 and (1, 5.3)


@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_plateaus_every_element_type_every_mode(lp, hip, route, dtype):
    """(100, 300) in blocks of 44 x 50 (G.plateau_image: the type's extremes among the levels; int64 within +-2^62, uint64 up to
    2^64 - 2^16 with levels that round when read through a double).  A reordered, re-paired or fused tap loop changes at least 32
    pixels of every integer case here but fused at sigma (1, 5.3) in the 8-bit types
    (tests/test_gaussian_reference_cpu.py::test_plateaus_see_every_wrong_arithmetic), and the float64 case sees any change of the sum."""
    a = plateau(PLATEAU_SHAPE, dtype)
    assert hip.get_option("x_gauss_lds") == 1
    for sigma in PLATEAU_SIGMAS:
        for mode in MODES:
            check(lp, hip, route, a, sigma=sigma, mode=mode, cval=CVAL)
    name = np.dtype(dtype).name
    wide = np.dtype(dtype).itemsize == 8                  # sigma 3: 107 008 bytes of LDS, above the default route's 80 KiB
    assert names_for(dtype, 12, 12) == {1: both(dtype) if wide else "gauss_lds_kernel<%s, tile=128x32>" % name,
                                        2: "gauss_lds_kernel<%s, tile=128x32>" % name,
                                        0: "gauss_axis_kernel<%s, axis=0> + gauss_axis_kernel<%s, axis=1>" % (name, name)}
    assert names_for(dtype, 4, 21)[1] == (both(dtype) if wide else fused(dtype)) and names_for(dtype, 4, 21)[2] == fused(dtype)


# ------------------------------------------------------------------------------------ B.2 the three types that never ran

@pytest.mark.parametrize("dtype", ["int8", "uint32", "uint64"])
@pytest.mark.parametrize("shape", SUBSET_SHAPES, ids=_id)
def test_normal_data_in_the_types_that_never_ran(lp, hip, route, shape, dtype):
    a = wide_uint64(shape) if dtype == "uint64" else image(shape, dtype)
    for sigma in SUBSET_SIGMAS:
        for mode in MODES:
            check(lp, hip, route, a, sigma=sigma, mode=mode, cval=CVAL)
    assert names_for("uint64", 2, 2)[1] == fused("uint64") and names_for("uint64", 12, 12)[1] == both("uint64")


# ------------------------------------------------------------------------------------ B.3 special floats

@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_nan_infinities_negative_zero_subnormals_and_the_maximum(lp, hip, route, dtype):
    """G.special_image: one NaN, +inf and -inf 35 columns apart, a 28 x 28 block of -0.0, one of the smallest subnormals, a 2 x 2 block
    of the type's maximum, at sigma 3 under every mode (tests/test_gaussian_reference_cpu.py: scipy returns NaN, +inf, -inf,
    subnormals, -0.0 and normal values from it).  NaNs are compared by position only: x86 and the GPU generate different default NaNs
    (inf - inf is negative on the one and positive on the other), everything else by its bytes."""
    a = G.special_image(dtype)
    for mode in MODES:
        ref = check(lp, hip, route, a, sigma=3, mode=mode, cval=CVAL)
        kinds = (np.isnan(ref).any(), (ref == np.inf).any(), (ref == -np.inf).any(), ((ref == 0) & np.signbit(ref)).any())
        assert all(kinds), (mode, kinds)
    zeros = np.full((40, 70), -0.0, dtype)
    ref = check(lp, hip, route, zeros, sigma=3, mode="reflect")
    assert np.signbit(ref).all()
    tiny = G.tiny_image(dtype)
    for mode in ("reflect", "constant"):
        ref = check(lp, hip, route, tiny, sigma=3, mode=mode, cval=0.0)
        assert (ref != 0).all() and (np.abs(ref) < np.finfo(dtype).tiny).all()
    plain = image((40, 70), dtype)
    for cval in (np.inf, np.nan, -1e300, 1e40):
        check(lp, hip, route, plain, sigma=3, mode="constant", cval=cval)


# ------------------------------------------------------------------------------------ B.4 radii

@pytest.mark.parametrize("dtype", ["float32", "uint8", "int64"])
def test_radius_zero_is_an_empty_tap_loop(lp, hip, route, dtype):
    a = plateau((57, 153), dtype)
    n = np.dtype(dtype).name
    zero = {1: "gauss_lds_kernel<%s, tile=128x32>" % n, 2: "gauss_lds_kernel<%s, tile=128x32>" % n,
            0: "gauss_axis_kernel<%s, axis=0> + gauss_axis_kernel<%s, axis=1>" % (n, n)}
    for mode in ("reflect", "constant"):
        ref = check(lp, hip, route, a, names=zero, sigma=0.1, mode=mode, cval=CVAL)           # int(0.4 + 0.5) = 0
        assert ref.tobytes() == a.tobytes() or dtype == "int64"              # (int64 is read through a double: 2^62 - 513 is not one)
        ref = check(lp, hip, route, a, names=zero, sigma=3, radius=0, mode=mode, cval=CVAL)
        assert ref.tobytes() == a.tobytes() or dtype == "int64"
        check(lp, hip, route, a, names=zero, sigma=3, radius=(0, 5), mode=mode, cval=CVAL)
        check(lp, hip, route, a, names=zero, sigma=3, radius=(5, 0), mode=mode, cval=CVAL)
        check(lp, hip, route, image((57, 153), dtype), names=zero, sigma=3, radius=(0, 5), mode=mode, cval=CVAL)


@pytest.mark.parametrize("dtype", ["uint8", "int16"])
def test_radius_one_pads_the_second_plane_to_sixteen_bytes(lp, hip, route, dtype):
    """34 x 130 elements: 4420 bytes (uint8) and 8840 (int16), no multiples of 16, so the second plane starts 12 and 8 bytes further."""
    size = np.dtype(dtype).itemsize
    assert 34 * 130 * size == {1: 4420, 2: 8840}[size] and lds_bytes(1, 1, size) == {1: 4432 + 4160, 2: 8848 + 8320}[size]
    for a in (plateau((57, 153), dtype), image((57, 153), dtype), image((33, 129), dtype)):
        for mode in MODES:
            check(lp, hip, route, a, names={1: fused(dtype), 2: fused(dtype), 0: both(dtype)}, sigma=3, radius=1, mode=mode, cval=CVAL)


@pytest.mark.parametrize("radius", [(40, 2), (2, 40)], ids=_id)
def test_asymmetric_radii(lp, hip, route, radius):
    """Radius 40 is beyond the default route's 24; under x_gauss_lds = 2 the planes are 76 032 and 56 576 bytes."""
    assert lds_bytes(40, 2, 4) == 76032 and lds_bytes(2, 40, 4) == 56576
    names = {1: "gauss_axis_kernel<float32, axis=0> + gauss_axis_kernel<float32, axis=1>", 2: "gauss_lds_kernel<float32, tile=128x32>",
             0: "gauss_axis_kernel<float32, axis=0> + gauss_axis_kernel<float32, axis=1>"}
    for a in (image((57, 153), "float32"), plateau(PLATEAU_SHAPE, "float32")):
        for mode in MODES:
            check(lp, hip, route, a, names=names, sigma=(10, 0.6) if radius[0] == 40 else (0.6, 10), radius=radius, mode=mode, cval=CVAL)


@pytest.mark.parametrize("dtype", ["float32", "uint8"])
@pytest.mark.parametrize("shape", [(5, 400), (40, 70)], ids=_id)
def test_the_largest_radius(lp, hip, route, shape, dtype):
    """Radius 192 at sigma 48: the largest argument block (193 weights per axis), up to 77 folds of a line of 5; one launch per axis on
    every route (uint8: 416 x 512 bytes of LDS for the first plane alone)."""
    assert lds_bytes(192, 192, 1) > LDS_CAP
    a = image(shape, dtype)
    for mode in MODES:
        check(lp, hip, route, a, names={1: both(dtype), 2: both(dtype), 0: both(dtype)}, sigma=48, radius=192, mode=mode, cval=CVAL)
    check(lp, hip, route, plateau(shape, dtype), names={1: both(dtype), 2: both(dtype), 0: both(dtype)}, sigma=48, mode="reflect")   # int(192.5)


def test_radius_193_is_refused_before_any_launch(lp, hip):
    a = image((40, 70), "float32")
    lp.gaussian_filter(a, 0)
    assert hip.last_kernel() == "gauss_copy"
    for kw in (dict(radius=193), dict(radius=(2, 193)), dict(radius=(193, 2)), dict(truncate=4.02)):       # int(4.02 * 48 + 0.5) = 193
        with pytest.raises(NotImplementedError, match="above 192"):
            lp.gaussian_filter(a, 48, **kw)
        assert hip.last_kernel() == "gauss_copy"
    with pytest.raises(NotImplementedError, match="above 192"):
        lp.gaussian_filter(a, (0, 48), radius=(500, 193))                    # the skipped axis' radius is not looked at; the other is


CAP = [("float32", 54, 162368, 55, 165648), ("float64", 25, 162336, 26, 167040), ("uint8", 155, 163824, 156, 165440)]


@pytest.mark.parametrize("dtype,fits,fits_bytes,beyond,beyond_bytes", CAP, ids=[c[0] for c in CAP])
def test_both_sides_of_the_lds_cap(lp, hip, route, dtype, fits, fits_bytes, beyond, beyond_bytes):
    """x_gauss_lds = 2 takes the fused kernel up to 163 840 bytes of dynamic LDS: the last radius whose planes fit and the first whose
    planes do not (uint8 at radius 155: 163 824 bytes, 16 below the cap)."""
    size = np.dtype(dtype).itemsize
    assert lds_bytes(fits, fits, size) == fits_bytes <= 163840 < beyond_bytes == lds_bytes(beyond, beyond, size)
    n = np.dtype(dtype).name
    for a in (image((57, 153), dtype), plateau((57, 153), dtype)):
        for mode in ("reflect", "constant"):
            check(lp, hip, route, a, names={2: "gauss_lds_kernel<%s, tile=128x32>" % n}, values=(2,), sigma=fits / 4.0, radius=fits, mode=mode,
                  cval=CVAL)
            check(lp, hip, route, a, names={2: "gauss_axis_kernel<%s, axis=0> + gauss_axis_kernel<%s, axis=1>" % (n, n)}, values=(2,),
                  sigma=fits / 4.0, radius=beyond, mode=mode, cval=CVAL)
    check(lp, hip, route, image((57, 153), dtype), sigma=fits / 4.0, radius=fits, mode="reflect", values=(1, 0),
          names={1: both(dtype), 0: both(dtype)})


# ------------------------------------------------------------------------------------ B.5 shapes

SHAPES = [(300, 2), (129, 1), (1, 129), (4, 64), (5, 65), (33, 257)]


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_one_more_than_a_tile_and_narrower_than_the_radius(lp, hip, route, shape):
    """One more than a tile of either kernel on each axis (128 x 32 and 64 x 4), images narrower than every radius, tall and thin
    ones: float64 normal data (order-sensitive as it is) and uint16 plateaus."""
    for a in (image(shape, "float64"), plateau(shape, "uint16")):
        for sigma in PLATEAU_SIGMAS:
            for mode in MODES:
                check(lp, hip, route, a, sigma=sigma, mode=mode, cval=CVAL)
    assert names_for("float64", 12, 12)[1] == both("float64") and names_for("uint16", 4, 21)[1] == fused("uint16")


# ------------------------------------------------------------------------------------ B.6 nothing is written around the destination

@pytest.mark.parametrize("mode", ["wrap", "constant"])
@pytest.mark.parametrize("dtype", ["float32", "uint8", "float64"])
def test_nothing_is_written_around_a_device_destination(lp, hip, route, dtype, mode):
    """The destination sits 37 elements into a room of 0xA5 bytes; the source is a row-strided device view whose skipped columns hold
    the type's extremes, so a row read at a wrong pitch or a column folded into the wrong place changes the frame."""
    dt = np.dtype(dtype)
    h, w = 33, 129
    lead, pitch, left = 37, w + 10, 3
    lo, hi = extremes(dtype)
    wide = np.empty((h, pitch), dt)
    wide[:, :left], wide[:, left + w:] = hi, lo
    wide[:, left:left + w] = image((h, w), dtype)
    ref = ndi.gaussian_filter(wide[:, left:left + w], 3, mode=mode, cval=CVAL)
    src = hip.DeviceArray(wide.shape, dt).copy_from_host(wide)
    sentinel = np.frombuffer(bytes([0xA5]) * ((h * w + 2 * lead) * dt.itemsize), dt)
    names = names_for(dtype, 12, 12)
    assert names[2] == fused(dtype) and names[0] == both(dtype)
    for value in (1, 2, 0):
        room = hip.DeviceArray(sentinel.shape, dt).copy_from_host(sentinel)
        out = DeviceView(room, (h, w), None, lead * dt.itemsize)
        view = DeviceView(src, (h, w), (pitch * dt.itemsize, dt.itemsize), left * dt.itemsize)
        assert route(value, lambda: lp.gaussian_filter(view, 3, mode=mode, cval=CVAL, out=out)) is out
        SEEN.add(hip.last_kernel())
        assert hip.last_kernel() == names[value]
        got = room.copy_to_host()
        n = dt.itemsize
        before = sentinel.tobytes()
        assert got[:lead].tobytes() == before[:lead * n] and got[lead + h * w:].tobytes() == before[(lead + h * w) * n:], value
        assert same(got[lead:lead + h * w].reshape(h, w), ref), value
        assert src.copy_to_host().tobytes() == wide.tobytes()                # and the source is as it was


# ------------------------------------------------------------------------------------ B.7 the raised limit is sticky and harmless

def test_small_calls_after_the_limit_of_their_kernel_was_raised(lp, hip, route):
    """One instantiation, gauss_lds_kernel<float32>: radius 2 (35 904 bytes), 54 (162 368: raises the limit to the cap), 2, 32
    (98 304: a smaller raised size after a larger one), 2 -- and calls on a stream that is not the default one."""
    assert (lds_bytes(2, 2, 4), lds_bytes(54, 54, 4), lds_bytes(32, 32, 4)) == (35904, 162368, 98304)
    name = {2: "gauss_lds_kernel<float32, tile=128x32>"}
    a = image((57, 153), "float32")
    for radius in (2, 54, 2, 32, 2):
        for mode in ("reflect", "constant"):
            check(lp, hip, route, a, names=name, values=(2,), sigma=max(radius / 4.0, 1.0), radius=radius, mode=mode, cval=CVAL)
    torch = pytest.importorskip("torch")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        t = torch.from_numpy(a.copy()).to("cuda:0")
        big = route(2, lambda: lp.gaussian_filter(t, 13.5, radius=54, mode="mirror"))
        assert hip.last_kernel() == name[2]
        small = route(2, lambda: lp.gaussian_filter(t, 1, radius=2, mode="mirror"))
        assert hip.last_kernel() == name[2]
    stream.synchronize()
    assert same(big.cpu().numpy(), ndi.gaussian_filter(a, 13.5, radius=54, mode="mirror"))
    assert same(small.cpu().numpy(), ndi.gaussian_filter(a, 1, radius=2, mode="mirror"))


# ------------------------------------------------------------------------------------ B.8 the bounds-checking build

def test_bounds_checking_build_counts_no_tap_outside_its_plane_at_the_edges_of_the_chooser(hip):
    """The library built with -DDCP_DEBUG_BOUNDS, in a process of its own as in tests/test_gaussian_gpu.py: radius 0, radius 1 in uint8
    (a first plane that is no multiple of 16 bytes), the radii of the LDS cap in uint8 and float32, and 100 x 300 under constant, where
    one image has tiles on both instantiations of the tap loop."""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    lib = os.path.join(ROOT, "discorpy_amd", "lib", "libdiscorpy_hip_bounds.so")
    assert os.path.exists(lib), "build() makes the bounds-checking library; it is missing"
    code = """
import sys, numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
from scipy import ndimage as ndi
from helpers import gaussian_reference as G
from discorpy_amd import _ffi as F
from discorpy_amd.prep import linepattern as lp
F.require_device()
assert F.debug_bounds()[4] == 1
F.set_option("x_gauss_lds", 2)
rng = np.random.default_rng(3)
noise = lambda shape, dtype: (rng.standard_normal(shape) * 40.0 + 128.0).clip(0, 255).astype(dtype)
cases = [(noise((57, 153), "float32"), dict(sigma=0.1)), (noise((57, 153), "uint8"), dict(sigma=3, radius=(0, 5))),
         (noise((57, 153), "uint8"), dict(sigma=3, radius=1)), (noise((33, 129), "uint8"), dict(sigma=3, radius=1)),
         (noise((57, 153), "uint8"), dict(sigma=38.75, radius=155)), (noise((57, 153), "float32"), dict(sigma=13.5, radius=54)),
         (G.plateau_image((100, 300), "uint16", (44, 50)), dict(sigma=3)), (noise((100, 300), "float32"), dict(sigma=(1, 5.3))),
         (noise((100, 300), "float32"), dict(sigma=8))]
for a, kw in cases:
    for mode in ("constant", "reflect"):
        assert np.array_equal(lp.gaussian_filter(a, mode=mode, cval=1.5, **kw), ndi.gaussian_filter(a, mode=mode, cval=1.5, **kw)), (a.shape, kw, mode)
        assert F.last_kernel().startswith("gauss_lds_kernel"), F.last_kernel()
b = F.debug_bounds()
assert b[0] == 0 and b[4] == 1, b
print("bounds ok", b)
""" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT, env=dict(os.environ, DCP_LIB_PATH=lib))
    assert r.returncode == 0 and "bounds ok" in r.stdout, (r.stdout + r.stderr)[-3000:]


# ------------------------------------------------------------------------------------ B.9 the configurations this file reaches

def test_every_configuration_is_reached(lp, hip, route):
    """One call per configuration and element type, so that a change of the chooser cannot silently stop this file from covering
    one: the names are literals.  Prints every name the file's calls reported (the tests above included, where they ran in this
    process)."""
    types = ("float32", "float64", "uint8", "int8", "uint16", "int16", "uint32", "int32", "int64", "uint64")
    required = {"gauss_copy"}
    for t in types:
        required |= {"gauss_lds_kernel<%s, tile=128x32>" % t, "gauss_axis_kernel<%s, axis=0> + gauss_axis_kernel<%s, axis=1>" % (t, t),
                     "gauss_axis_kernel<%s, axis=0>" % t, "gauss_axis_kernel<%s, axis=1>" % t}
    assert len(required) == 41
    here = set()
    for t in types:
        a = plateau((33, 129), t)
        for value, sigma in ((2, 3), (0, 3), (1, (3, 0)), (1, (0, 3)), (1, 0)):
            got = route(value, lambda: lp.gaussian_filter(a, sigma, mode="mirror"))
            here.add(hip.last_kernel())
            assert same(got, ndi.gaussian_filter(a, sigma, mode="mirror")), (t, value, sigma)
    SEEN.update(here)
    print("kernel names observed by test_gaussian_edges_gpu.py:")
    for name in sorted(SEEN):
        print("   ", name)
    assert here == required, sorted(here ^ required)
