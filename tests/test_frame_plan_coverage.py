"""Frame plans (csrc/frame_plan.cpp, plan_table_kernel, remap_wg_kernel<.., PLAN>): what tests/test_frame_plan.py does not reach.

1. every one of the 40 planned instantiations (NF 1..10 x four samplers) runs, under a condition that a plan which certifies nothing
   cannot meet: the certificate is computed a second time in NumPy (tests/helpers/plan_emulation.py) and the device must certify at
   least half as many wave tiles;
2. the centres, calibrations, shapes and options where the plan's special cases live;
3. plans of row bands (y_origin / rows_out in the key) through the host paths;
4. the cache's rules that nothing else executes: the retirement cap, the ring of once-seen keys, host threads racing on one new
   calibration, stream capture (in a child process: tests/helpers/capture_frames.py).

Bar, everywhere: np.array_equal with the CPU oracle (POLY_KERNEL, matching blend) and with the same call under x_frame_plan = 0.
"""
import json
import math
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from conftest import ROOT, noise

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
from plan_emulation import emulated_certificate  # noqa: E402

from discorpy_amd import configs  # noqa: E402

gpu = pytest.mark.gpu

SAMPLERS = ["f64lerp", "scipy", "f32", "order0"]
KERNEL_SAMPLER = {"f64lerp": "f64lerp", "scipy": "scipy", "f32": "f32lerp", "order0": "nearest"}
H0, W0 = 1024, 1536
BASE = [1.0, -0.04, 0.03, -0.02, 0.012, -0.008, 0.005, -0.003, 0.002, -0.001]
FAMILY_CENTRES = [(W0 / 2 + 0.3, H0 / 2 - 0.4), (768.0, 512.0), (640.0, 480.0)]


def family(nf, shape=(H0, W0)):
    """fact[k] = BASE[k] / R**k, R = half the frame's diagonal: every term moves a corner pixel by BASE[k] of the radius."""
    R = math.hypot(*shape) / 2
    return [BASE[k] / R ** k for k in range(nf)]


def full_plan_tiles(shape):
    H, W = shape
    return 4 * ((W + 127) // 128) * ((H + 31) // 32)


def _want(orc, img, xc, yc, fact, sampler):
    if sampler == "order0":
        return orc.unwarp_image_backward(img, xc, yc, fact, order=0, poly=orc.POLY_KERNEL)
    blend = {"scipy": orc.BLEND_SCIPY, "f64lerp": orc.BLEND_F64LERP, "f32": orc.BLEND_F32LERP}[sampler]
    return orc.unwarp_image_backward(img, xc, yc, fact, poly=orc.POLY_KERNEL, blend=blend)


def _call(hip, src, dst, shape, xc, yc, fact, sampler, mem=None, stream=None):
    H, W = shape
    fa, nf = hip.fact_array(fact)
    order = 0 if sampler == "order0" else 1
    blend = hip.BLEND_F64LERP if sampler == "order0" else hip.BLEND_BY_NAME[sampler]
    hip.check(hip.lib().dcp_unwarp_image_f32(src.ptr, dst.ptr, H, W, W, 1, xc, yc, fa, nf, order, 1, blend,
                                             hip.MEM_DEVICE if mem is None else mem, -1, None if stream is None else stream.ptr))


@pytest.fixture
def plan_mode(hip):
    """Sets x_frame_plan for the test and starts it from an empty plan cache; restores the default afterwards."""
    old = hip.get_option("x_frame_plan")

    def set_mode(v):
        hip.set_option("x_frame_plan", v)
    hip.release_scratch()
    yield set_mode
    hip.set_option("x_frame_plan", old)
    hip.release_scratch()


@pytest.fixture
def option(hip):
    """set(key, value) for the test; every key touched gets its old value back."""
    old = {}

    def set_option(key, value):
        old.setdefault(key, hip.get_option(key))
        hip.set_option(key, value)
    yield set_option
    for k, v in old.items():
        hip.set_option(k, v)


def _planned_twice_then_unplanned(hip, plan_mode, img, xc, yc, fact, sampler, **kw):
    """Mode 2: one call that builds the plan (if the kernel that runs has plans) and one that finds it; then the same call under mode 0
    (the cache is left alone: plans stay, unused).  Returns ([planned, planned, unplanned], kernel, wave tiles, uncertified tiles)."""
    shape = img.shape
    src = hip.DeviceBuffer(img.nbytes).upload(img)
    dst = [hip.DeviceBuffer(img.nbytes).upload(np.full(shape, -1.0, np.float32)) for _ in range(3)]
    try:
        plan_mode(2)
        _call(hip, src, dst[0], shape, xc, yc, fact, sampler, **kw)
        _call(hip, src, dst[1], shape, xc, yc, fact, sampler, **kw)
        kernel = hip.last_kernel()
        if kw.get("stream") is not None:
            kw["stream"].synchronize()
        tiles, exact = hip.get_option("x_frame_plan_tiles"), hip.get_option("x_frame_plan_exact_tiles")
        plan_mode(0)
        _call(hip, src, dst[2], shape, xc, yc, fact, sampler, **kw)
        if kw.get("stream") is not None:
            kw["stream"].synchronize()
        return [d.download(shape, np.float32) for d in dst], kernel, tiles, exact
    finally:
        for b in [src] + dst:
            b.free()


def _assert_not_vacuous(shape, xc, yc, fact, tiles, exact):
    """The floor of section 1: the plan of a whole frame certifies at least half the wave tiles the NumPy emulation reproduces (the
    half: the device fuses its multiply-adds and refuses clipped, oversized and partial tiles)."""
    tiles_e, reproduced = emulated_certificate(shape, xc, yc, fact)
    assert tiles == tiles_e == full_plan_tiles(shape) and 0 <= exact <= tiles
    assert reproduced > 0 and 2 * (tiles - exact) >= reproduced, (tiles, exact, reproduced)
    return reproduced


def _assert_equal_all(got, want, what):
    for i, g in enumerate(got):
        assert np.array_equal(g, want), (what, i)
    assert np.array_equal(got[0], got[2]) and np.array_equal(got[1], got[2]), what


# ------------------------------------------------------------------ the emulation itself (no GPU)

def test_emulation_leaves_124_of_16384_wave_tiles_of_config_2():
    """The figure the device reports for config 2 at 4096 x 4096 (tests/test_frame_plan.py bounds it from above): the NumPy
    certificate, which shares no code with the device's, arrives at the same count."""
    c = configs.cfg2()
    tiles, reproduced = emulated_certificate(c["shape"], c["xcenter"], c["ycenter"], c["list_fact"])
    assert (tiles, tiles - reproduced) == (16384, 124)


def test_emulation_of_the_model_family():
    """A constant factor is reproduced everywhere; the longer models on 73 to 81 % of the 1 536 wave tiles."""
    assert emulated_certificate((H0, W0), *FAMILY_CENTRES[0], family(1)) == (1536, 1536)
    for nf in range(2, 11):
        for xc, yc in FAMILY_CENTRES:
            tiles, reproduced = emulated_certificate((H0, W0), xc, yc, family(nf))
            assert tiles == 1536 and 0.73 * tiles <= reproduced <= 0.81 * tiles, (nf, xc, yc, reproduced)


# ------------------------------------------------------------------ 1. all 40 instantiations

@gpu
@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("nf", range(1, 11))
def test_every_planned_instantiation_certifies_what_the_emulation_does(hip, orc, plan_mode, nf, sampler):
    """remap_wg_kernel<Radial, NF, sampler, float, PLAN> for every NF and sampler, at the three centres the host certifies for
    128 x 32 tiles.  The certificate is only sound if this instantiation evaluates radial_rows_interp as plan_table_kernel<NF> did: a
    difference shows as unequal pixels on some certified tile.  It is only exercised if tiles ARE certified: at least half of those
    the NumPy emulation reproduces (the half: the device fuses its multiply-adds and refuses clipped, oversized and partial tiles).

    Tried on a scratch build whose frame kernel alone has 1 / 749 for the cubic's 1 / 750: the 27 cases of NF >= 2 with an
    interpolating blend fail.  NF = 1 cannot (the differences of a constant factor are zero, whatever multiplies them), and an
    order-0 output moves only where a coordinate crosses a rounding boundary, which that change did not bring about in these frames:
    the order-0 instantiations are held by equality with the oracle alone."""
    fact = family(nf)
    img = noise(7000 + 16 * nf + SAMPLERS.index(sampler), (H0, W0))
    for xc, yc in FAMILY_CENTRES:
        assert hip.tile_certificate(H0, W0, xc, yc, fact) == 2
        reproduced = emulated_certificate((H0, W0), xc, yc, fact)[1]
        want = _want(orc, img, xc, yc, fact, sampler)
        got, kernel, tiles, exact = _planned_twice_then_unplanned(hip, plan_mode, img, xc, yc, fact, sampler)
        print("NF=%d %s centre (%.1f, %.1f): %s, wave tiles %d, emulation reproduces %d, device certifies %d"
              % (nf, sampler, xc, yc, kernel, tiles, reproduced, tiles - exact))
        assert kernel == "remap_wg_kernel<Radial,NF=%d,%s>" % (nf, KERNEL_SAMPLER[sampler])
        _assert_equal_all(got, want, (nf, sampler, xc, yc))
        _assert_not_vacuous((H0, W0), xc, yc, fact, tiles, exact)
        hip.release_scratch()


# ------------------------------------------------------------------ 2. centres, calibrations, shapes, options

GENTLE = [1.001, -5e-6, 4e-9, -1e-12]           # level 2 wherever the centre lies, inside the frame or on its corners

SPECIAL_CENTRES = {
    "integer_pixel_tile_corner_row0": (768.0, 512.0),
    "node_row5": (700.0, 517.0),
    "node_row10": (700.0, 522.0),
    "node_row15": (700.0, 527.0),
    "non_node_row": (700.0, 519.0),
    "half_pixel": (700.5, 519.5),
    "first_pixel": (0.0, 0.0),
    "first_pixel_minus_zero": (-0.0, -0.0),
    "last_pixel": (W0 - 1.0, H0 - 1.0),
}


@gpu
@pytest.mark.parametrize("sampler", ["f64lerp", "scipy"])
@pytest.mark.parametrize("centre", list(SPECIAL_CENTRES))
def test_centres_where_r2_vanishes_and_the_kink_tile_lives(hip, orc, plan_mode, centre, sampler):
    """The NF = 5 model of the family (at the frame's corners the host does not certify it: whatever kernel runs, the result is
    equal), and a gentle model that is certified for 128 x 32 tiles at every centre of the list, the corners included."""
    xc, yc = SPECIAL_CENTRES[centre]
    img = noise(7300 + len(centre), (H0, W0))
    for model, fact in (("family", family(5)), ("gentle", GENTLE)):
        got, kernel, tiles, exact = _planned_twice_then_unplanned(hip, plan_mode, img, xc, yc, fact, sampler)
        print("%s %s %s: %s, wave tiles %d, not certified %d" % (centre, model, sampler, kernel, tiles, exact))
        _assert_equal_all(got, _want(orc, img, xc, yc, fact, sampler), (centre, model, sampler))
        if model == "gentle":
            assert hip.tile_certificate(H0, W0, xc, yc, fact) == 2
            assert kernel == "remap_wg_kernel<Radial,NF=4,%s>" % KERNEL_SAMPLER[sampler]
        if kernel.startswith("remap_wg_kernel"):
            # (the tile that holds the centre, where ru has its kink, is never certified)
            _assert_not_vacuous((H0, W0), xc, yc, fact, tiles, exact)
            assert exact >= 1
        else:
            assert tiles == 0
        hip.release_scratch()


@gpu
@pytest.mark.parametrize("sampler", ["f64lerp", "scipy"])
def test_plus_and_minus_zero_are_two_calibrations_with_one_result(hip, orc, plan_mode, sampler):
    """The plan key compares bit patterns: (0.0, 0.0) and (-0.0, -0.0) never share a plan, and give the same frame."""
    fact = GENTLE
    shape = (H0, W0)
    assert hip.tile_certificate(H0, W0, 0.0, 0.0, fact) == 2 and hip.tile_certificate(H0, W0, -0.0, -0.0, fact) == 2
    img = noise(7400, shape)
    want = _want(orc, img, 0.0, 0.0, fact, sampler)
    assert np.array_equal(want, _want(orc, img, -0.0, -0.0, fact, sampler))
    src = hip.DeviceBuffer(img.nbytes).upload(img)
    dst = [hip.DeviceBuffer(img.nbytes) for _ in range(5)]
    plan_mode(1)                                                   # build on the second sighting of a key
    _call(hip, src, dst[0], shape, 0.0, 0.0, fact, sampler)
    assert hip.last_kernel() == "remap_wg_kernel<Radial,NF=4,%s>" % KERNEL_SAMPLER[sampler]
    assert hip.get_option("x_frame_plan_tiles") == 0
    _call(hip, src, dst[1], shape, -0.0, -0.0, fact, sampler)      # one key would make this the second sighting
    assert hip.get_option("x_frame_plan_tiles") == 0
    _call(hip, src, dst[2], shape, 0.0, 0.0, fact, sampler)
    assert hip.get_option("x_frame_plan_tiles") == full_plan_tiles(shape)
    _call(hip, src, dst[3], shape, -0.0, -0.0, fact, sampler)
    _call(hip, src, dst[4], shape, -0.0, -0.0, fact, sampler)
    got = [d.download(shape, np.float32) for d in dst]
    for b in [src] + dst:
        b.free()
    for i, g in enumerate(got):
        assert np.array_equal(g, want), i


CALIBRATIONS = {
    # (centre, coefficients, level of the host's certificate)
    "mirrored": ((760.3, 500.2), [-1.0, 1e-5], 2),
    "folding": ((760.3, 500.2), [1.0, -1e-3, 4e-7], 0),
}


@gpu
@pytest.mark.parametrize("sampler", ["f64lerp", "scipy"])
@pytest.mark.parametrize("name", list(CALIBRATIONS))
def test_mirrored_and_folding_calibrations(hip, orc, plan_mode, name, sampler):
    (xc, yc), fact, level = CALIBRATIONS[name]
    assert hip.tile_certificate(H0, W0, xc, yc, fact) == level
    img = noise(7500 + len(name), (H0, W0))
    got, kernel, tiles, exact = _planned_twice_then_unplanned(hip, plan_mode, img, xc, yc, fact, sampler)
    print("%s %s: %s, wave tiles %d, not certified %d" % (name, sampler, kernel, tiles, exact))
    _assert_equal_all(got, _want(orc, img, xc, yc, fact, sampler), (name, sampler))
    if level == 2:
        assert kernel == "remap_wg_kernel<Radial,NF=%d,%s>" % (len(fact), KERNEL_SAMPLER[sampler])
        assert tiles == full_plan_tiles((H0, W0))
    else:
        assert not kernel.startswith("remap_wg_kernel") and tiles == 0     # whatever ran has no plan


# (H, W): one pixel past, one short of and exactly one workgroup tile; the smallest frame; one tile row of many columns and the
# reverse; eight tile columns (XCD stripes kept) and nine (launch_wg falls back to the plain order)
SHAPES = [(33, 129), (31, 127), (32, 128), (2, 2), (17, 2000), (1000, 65), (96, 1024), (96, 1152)]


@gpu
@pytest.mark.parametrize("sampler", ["f64lerp", "scipy"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_partial_tiles_and_both_tile_orders(hip, orc, plan_mode, shape, sampler):
    """The model of configs.rescale_model(W) (on the small frames the host certifies it for 64 x 16 tiles at most: other kernels,
    equal results), and a gentle one that is certified for 128 x 32 tiles on every shape, so that the planned kernel meets the
    partial tiles."""
    H, W = shape
    img = noise(7600 + H, shape)
    for model, (xc, yc, fact) in (("rescaled", configs.rescale_model(W)), ("gentle", (W / 2 + 0.3, H / 2 - 0.4, [1.0, -1e-5]))):
        got, kernel, tiles, exact = _planned_twice_then_unplanned(hip, plan_mode, img, xc, yc, fact, sampler)
        print("%dx%d %s %s: %s, wave tiles %d, not certified %d" % (H, W, model, sampler, kernel, tiles, exact))
        _assert_equal_all(got, _want(orc, img, xc, yc, fact, sampler), (shape, model, sampler))
        assert 0 <= exact <= tiles
        if model == "gentle":
            assert hip.tile_certificate(H, W, xc, yc, fact) == 2
            assert kernel == "remap_wg_kernel<Radial,NF=2,%s>" % KERNEL_SAMPLER[sampler]
        assert tiles == (full_plan_tiles(shape) if kernel.startswith("remap_wg_kernel") else 0)
        hip.release_scratch()


@gpu
@pytest.mark.parametrize("sampler", ["f64lerp", "scipy"])
@pytest.mark.parametrize("built_under, read_under", [(2, 0), (0, 2)])
def test_a_plan_built_under_one_tile_order_serves_the_other(hip, orc, plan_mode, option, built_under, read_under, sampler):
    """The plan's table is in plain tile order whatever order the workgroups are dealt in (x_xcd_remap 0: row-major, 2: XCD stripes;
    1024 columns = 8 tile columns, where launch_wg keeps the stripes)."""
    shape = (H0, 1024)
    xc, yc, fact = 500.3, 520.6, family(5, shape)
    assert hip.tile_certificate(shape[0], shape[1], xc, yc, fact) == 2
    img = noise(7700 + built_under, shape)
    want = _want(orc, img, xc, yc, fact, sampler)
    src = hip.DeviceBuffer(img.nbytes).upload(img)
    dst = [hip.DeviceBuffer(img.nbytes) for _ in range(3)]
    plan_mode(2)
    option("x_xcd_remap", built_under)
    _call(hip, src, dst[0], shape, xc, yc, fact, sampler)
    assert hip.last_kernel().startswith("remap_wg_kernel")
    tiles, exact = hip.get_option("x_frame_plan_tiles"), hip.get_option("x_frame_plan_exact_tiles")
    _assert_not_vacuous(shape, xc, yc, fact, tiles, exact)
    option("x_xcd_remap", read_under)
    _call(hip, src, dst[1], shape, xc, yc, fact, sampler)
    plan_mode(0)
    _call(hip, src, dst[2], shape, xc, yc, fact, sampler)
    got = [d.download(shape, np.float32) for d in dst]
    for b in [src] + dst:
        b.free()
    _assert_equal_all(got, want, (built_under, read_under, sampler))


@gpu
@pytest.mark.parametrize("sampler", ["f64lerp", "scipy"])
@pytest.mark.parametrize("wg_per_cu", [1, 2, 3, 4, 5])
def test_planned_launch_with_capped_occupancy(hip, orc, plan_mode, option, wg_per_cu, sampler):
    """x_wg_per_cu pads the launch with unused dynamic LDS; at 1 and 2 the padding is beyond what a launch may ask for by default and
    the planned instantiation needs its own hipFuncSetAttribute."""
    xc, yc = FAMILY_CENTRES[0]
    fact = family(5)
    img = noise(7800 + wg_per_cu, (H0, W0))
    option("x_wg_per_cu", wg_per_cu)
    got, kernel, tiles, exact = _planned_twice_then_unplanned(hip, plan_mode, img, xc, yc, fact, sampler)
    assert kernel == "remap_wg_kernel<Radial,NF=5,%s>" % KERNEL_SAMPLER[sampler]
    _assert_not_vacuous((H0, W0), xc, yc, fact, tiles, exact)
    _assert_equal_all(got, _want(orc, img, xc, yc, fact, sampler), (wg_per_cu, sampler))


@gpu
@pytest.mark.parametrize("sampler", ["f64lerp", "scipy"])
def test_planned_launch_that_may_overlap_its_predecessor(hip, orc, plan_mode, sampler):
    """DCP_MEM_DEVICE_UNORDERED on one stream from the very first call: the launch that reads a plan still under construction keeps
    its barrier bit."""
    xc, yc = FAMILY_CENTRES[2]
    fact = family(7)
    img = noise(7900, (H0, W0))
    s = hip.Stream()
    got, kernel, tiles, exact = _planned_twice_then_unplanned(hip, plan_mode, img, xc, yc, fact, sampler, mem=hip.MEM_DEVICE_UNORDERED,
                                                              stream=s)
    assert kernel == "remap_wg_kernel<Radial,NF=7,%s>" % KERNEL_SAMPLER[sampler]
    _assert_not_vacuous((H0, W0), xc, yc, fact, tiles, exact)
    _assert_equal_all(got, _want(orc, img, xc, yc, fact, sampler), sampler)


# ------------------------------------------------------------------ 3. row-band plans through the host paths

HOST_SHAPE = (2200, 2100)                    # 18.5 MB: above the 16 MiB threshold of the direct and banded host paths
HOST_CENTRE = (1049.6, 1100.3)


def _host_frames(hip, orc, pp, img, fact, sampler, n, out=None):
    """n calls of pp.unwarp_image_backward with one calibration; every result against the oracle."""
    xc, yc = HOST_CENTRE
    want = _want(orc, img, xc, yc, fact, sampler)
    for i in range(n):
        if sampler == "order0":
            got = pp.unwarp_image_backward(img, xc, yc, fact, order=0, out=out)
        else:
            got = pp.unwarp_image_backward(img, xc, yc, fact, blend=sampler, out=out)
        assert np.array_equal(got, want), (sampler, i)
        del got
    return want


@gpu
@pytest.mark.parametrize("sampler", SAMPLERS)
def test_row_band_plans_of_the_host_paths(hip, orc, plan_mode, option, sampler):
    """A NumPy frame above 16 MiB whose destination is registered goes through the GPU in bands of rows (x host_direct = 2:
    run_host_direct, one launch_frame per band): y_origin and rows_out are part of the plan key and of what plan_table_kernel
    computes.  With host_direct = 0 an interpolating blend travels in bands of the stack kernel where the runtime overlaps the two
    directions of the link -- no plan, the count stays 0 -- and is staged whole otherwise, as order 0 always is: one whole-frame plan."""
    from discorpy_amd.post import postprocessing as pp
    H, W = HOST_SHAPE
    fact = family(5, HOST_SHAPE)
    assert hip.tile_certificate(H, W, HOST_CENTRE[0], HOST_CENTRE[1], fact) == 2
    img = noise(8000 + SAMPLERS.index(sampler), HOST_SHAPE)
    full = full_plan_tiles(HOST_SHAPE)
    wg = "remap_wg_kernel<Radial,NF=5,%s>" % KERNEL_SAMPLER[sampler]
    out = np.zeros(HOST_SHAPE, np.float32)
    L = hip.lib()
    hip.check(L.dcp_host_register(out.ctypes.data, out.nbytes, -1))
    try:
        plan_mode(2)
        option("host_direct", 2)
        want = _host_frames(hip, orc, pp, img, fact, sampler, 3, out=out)
        kernel, tiles = hip.last_kernel(), hip.get_option("x_frame_plan_tiles")
        print("%s host_direct=2: %s, wave tiles of the plan built last %d of %d" % (sampler, kernel, tiles, full))
        assert kernel == wg                        # a registered destination under host_direct = 2 is always written band by band
        assert 0 < tiles < full                    # the plan of a band
        # (run_host_direct cuts the frame into host_bands bands of equal height, a multiple of 64 rows: the plan built last is that of
        # the last band, and the floor of section 1 holds for it as for a whole frame)
        rows_per = -(-(-(-H // hip.get_option("host_bands"))) // 64) * 64
        y_last = (H - 1) // rows_per * rows_per
        tiles_e, reproduced = emulated_certificate((H - y_last, W), *HOST_CENTRE, fact, y_origin=y_last)
        certified = tiles - hip.get_option("x_frame_plan_exact_tiles")
        print("   last band: rows %d..%d, emulation reproduces %d, device certifies %d" % (y_last, H, reproduced, certified))
        assert tiles == tiles_e and reproduced > 0 and 2 * certified >= reproduced
        hip.release_scratch()

        option("host_direct", 0)
        _host_frames(hip, orc, pp, img, fact, sampler, 3)
        kernel, tiles = hip.last_kernel(), hip.get_option("x_frame_plan_tiles")
        print("%s host_direct=0: %s, wave tiles of the plan built last %d of %d" % (sampler, kernel, tiles, full))
        if kernel.startswith("remap_wg_kernel"):
            assert tiles == full                   # staged whole: one launch over the frame
        else:
            assert sampler != "order0" and tiles == 0      # bands of the stack kernel, which has no plan
        hip.release_scratch()

        plan_mode(0)
        for mode in (2, 0):
            option("host_direct", mode)
            got = pp.unwarp_image_backward(img, *HOST_CENTRE, fact, **({"order": 0} if sampler == "order0" else {"blend": sampler}),
                                           out=out if mode == 2 else None)
            assert np.array_equal(got, want), (sampler, mode)
            del got
        assert hip.get_option("x_frame_plan_tiles") == 0
    finally:
        hip.check(L.dcp_host_unregister(out.ctypes.data))


@gpu
@pytest.mark.parametrize("sampler", ["f64lerp", "order0"])
def test_more_row_bands_than_the_cache_holds_plans(hip, orc, plan_mode, option, sampler):
    """host_bands = 20 cuts the 2 200 rows into 18 bands of 128: one frame needs more plans than the 16 slots, so every frame after
    the first replaces plans that a launch may still be reading, and the fifth runs into the cap on replaced plans."""
    from discorpy_amd.post import postprocessing as pp
    H, W = HOST_SHAPE
    fact = family(5, HOST_SHAPE)
    img = noise(8100 + SAMPLERS.index(sampler), HOST_SHAPE)
    out = np.zeros(HOST_SHAPE, np.float32)
    L = hip.lib()
    hip.check(L.dcp_host_register(out.ctypes.data, out.nbytes, -1))
    try:
        plan_mode(2)
        option("host_direct", 2)
        option("host_bands", 20)
        _host_frames(hip, orc, pp, img, fact, sampler, 5, out=out)
        assert hip.last_kernel().startswith("remap_wg_kernel")
        tiles = hip.get_option("x_frame_plan_tiles")
        assert tiles in (4 * 17 * 4, 4 * 17 * 1)           # a band of 128 rows, or the last one of 24
        hip.release_scratch()
        _host_frames(hip, orc, pp, img, fact, sampler, 2, out=out)
    finally:
        hip.check(L.dcp_host_unregister(out.ctypes.data))


# ------------------------------------------------------------------ 4. cache rules

SMALL_A, SMALL_B = (512, 640), (480, 640)          # 4 * 5 * 16 = 320 and 4 * 5 * 15 = 300 wave tiles


@gpu
def test_no_plan_is_built_past_the_retirement_cap(hip, orc, plan_mode):
    """16 plans fill the slots, each of the next 64 replaces one, whose memory is kept (a launch or a captured graph may read it): at
    64 kept the cache builds nothing more until dcp_release_scratch."""
    xc0, yc, fact = configs.rescale_model(SMALL_A[1])
    assert hip.tile_certificate(*SMALL_A, xc0, yc, fact) == 2 and hip.tile_certificate(*SMALL_B, xc0, yc, fact) == 2
    img_a, img_b = noise(8200, SMALL_A), noise(8201, SMALL_B)
    src_a, src_b = hip.DeviceBuffer(img_a.nbytes).upload(img_a), hip.DeviceBuffer(img_b.nbytes).upload(img_b)
    dst = hip.DeviceBuffer(img_a.nbytes)
    plan_mode(2)
    try:
        for i in range(16 + 64):
            xc = xc0 + 0.25 * i
            _call(hip, src_a, dst, SMALL_A, xc, yc, fact, "f64lerp")
            assert np.array_equal(dst.download(SMALL_A, np.float32), _want(orc, img_a, xc, yc, fact, "f64lerp")), i
        assert hip.last_kernel().startswith("remap_wg_kernel")
        assert hip.get_option("x_frame_plan_tiles") == 320
        _call(hip, src_b, dst, SMALL_B, xc0, yc, fact, "f64lerp")
        assert hip.get_option("x_frame_plan_tiles") == 320           # nothing was built: still the last plan of the first shape
        want_b = _want(orc, img_b, xc0, yc, fact, "f64lerp")
        assert np.array_equal(dst.download(SMALL_B, np.float32), want_b)
        hip.release_scratch()
        for _ in range(2):
            _call(hip, src_b, dst, SMALL_B, xc0, yc, fact, "f64lerp")
            assert hip.get_option("x_frame_plan_tiles") == 300
            assert np.array_equal(dst.download(SMALL_B, np.float32), want_b)
    finally:
        for b in (src_a, src_b, dst):
            b.free()


@gpu
def test_the_ring_of_once_seen_keys_forgets_after_sixteen(hip, orc, plan_mode):
    """Default mode: a centre search (121 centres, each used once) builds nothing; a key whose first sighting lies 16 other keys back
    has been forgotten and is a first sighting again."""
    xc0, yc0, fact = configs.rescale_model(SMALL_A[1])
    img = noise(8300, SMALL_A)
    src = hip.DeviceBuffer(img.nbytes).upload(img)
    dst = hip.DeviceBuffer(img.nbytes)

    def frame(xc, yc):
        _call(hip, src, dst, SMALL_A, xc, yc, fact, "f64lerp")
        assert np.array_equal(dst.download(SMALL_A, np.float32), _want(orc, img, xc, yc, fact, "f64lerp")), (xc, yc)

    plan_mode(1)
    try:
        for j in range(11):
            for i in range(11):
                frame(xc0 + 0.5 * (i - 5), yc0 + 0.5 * (j - 5))
        assert hip.last_kernel().startswith("remap_wg_kernel")
        assert hip.get_option("x_frame_plan_tiles") == 0
        a = (xc0 + 0.125, yc0 + 0.125)
        frame(*a)
        for i in range(16):
            frame(xc0 + 7.0 + 0.5 * i, yc0)
        frame(*a)
        assert hip.get_option("x_frame_plan_tiles") == 0             # forgotten: a first sighting again
        frame(*a)
        assert hip.get_option("x_frame_plan_tiles") == 320
        frame(*a)
    finally:
        src.free()
        dst.free()


@gpu
@pytest.mark.parametrize("mode", [2, 1])
def test_host_threads_racing_on_one_new_calibration(hip, orc, plan_mode, mode):
    """Four host threads, a stream each, eight frames each, all of one calibration the library has not seen: one of them builds the
    plan, the others wait for it on the device."""
    nthreads, nframes = 4, 8
    shape = (H0, W0)
    xc, yc = FAMILY_CENTRES[0][0] + 0.0625 * mode, FAMILY_CENTRES[0][1]
    fact = family(6)
    frames = [noise(8400 + i, shape) for i in range(nframes)]
    want = [_want(orc, f, xc, yc, fact, "f64lerp") for f in frames]
    src = [hip.DeviceBuffer(f.nbytes).upload(f) for f in frames]
    dst = [[hip.DeviceBuffer(frames[0].nbytes).upload(np.full(shape, -1.0, np.float32)) for _ in range(nframes)] for _ in range(nthreads)]
    streams = [hip.Stream() for _ in range(nthreads)]
    errors = []
    start = threading.Barrier(nthreads)
    plan_mode(mode)

    def work(t):
        try:
            start.wait()
            for i in range(nframes):
                _call(hip, src[i], dst[t][i], shape, xc, yc, fact, "f64lerp", stream=streams[t])
            streams[t].synchronize()
        except Exception as e:      # noqa: BLE001 -- reported by the main thread
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(nthreads)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    try:
        assert not errors, errors
        assert hip.get_option("x_frame_plan_tiles") == full_plan_tiles(shape)
        for t in range(nthreads):
            for i in range(nframes):
                assert np.array_equal(dst[t][i].download(shape, np.float32), want[i]), (t, i)
    finally:
        for b in src + [d for row in dst for d in row]:
            b.free()


CAPTURE_SCENARIOS = ["empty_cache", "ready_plan_then_evicted", "plan_just_built"]


@gpu
@pytest.mark.parametrize("scenario", CAPTURE_SCENARIOS)
def test_frames_captured_into_a_graph(hip, orc, plan_mode, scenario):
    """tests/helpers/capture_frames.py, in a process of its own under a time limit: nothing is built, queried or waited for while the
    calling stream is being captured, and a replayed graph keeps reading valid plan memory after the plan was replaced."""
    helper = os.path.join(ROOT, "tests", "helpers", "capture_frames.py")
    r = subprocess.run([sys.executable, helper, scenario], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    text = r.stdout.decode("utf-8", "replace")
    print(text)
    assert r.returncode == 0, text
    report = json.loads([ln for ln in text.splitlines() if ln.startswith("{")][-1])
    assert report["scenario"] == scenario and report["ok"] is True, report
