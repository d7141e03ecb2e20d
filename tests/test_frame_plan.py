"""Frame plans of remap_wg_kernel (csrc/frame_plan.cpp): per calibration and frame shape, the hull of every 128 x 32 tile and one
certificate bit per 64 x 16 wave tile, built once on the device and kept for the frames that follow.  A certified wave tile takes
twelve of its sixteen coordinate rows from a cubic in the row index (radial_rows_interp); the certificate is the device's own
comparison of that evaluation with the exact one, so every output stays what it was.

Bar: np.array_equal with the CPU oracle (POLY_KERNEL, matching blend) and with the same call under x_frame_plan = 0 -- no tolerance.
"""
import numpy as np
import pytest

from conftest import noise

pytestmark = pytest.mark.gpu

from discorpy_amd import configs  # noqa: E402

SAMPLERS = ["f64lerp", "scipy", "f32", "order0"]


def _cases():
    c2, c5 = configs.cfg2(), configs.cfg5()
    x4, y4, f4 = configs.rescale_model(2560)
    xr, yr, fr = configs.rescale_model(1400)
    return {
        "cfg2_4096": ((4096, 4096), c2["xcenter"], c2["ycenter"], c2["list_fact"]),
        "cfg4_model_2560": ((2560, 2560), x4, y4, f4),
        # (nine coefficients, but the host certifies config 5 for 64 x 16 tiles only -- level 1: like the strong model below it runs on
        # remap_lds_kernel and exercises no plan; NF = 9 on a plan: tests/test_frame_plan_coverage.py)
        "cfg5_8192_nf9": ((8192, 8192), c5["xcenter"], c5["ycenter"], c5["list_fact"]),
        # (certified for 64 x 16 tiles only: runs on remap_lds_kernel, which has no plan -- the result must be equal all the same)
        "strong_1280x1000": ((1000, 1280), 500.3, 400.7, [1.0, -1e-4, 3e-7, -2e-10, 1e-13]),
        "ragged_1100x1400_centre_inside": ((1100, 1400), xr, yr, fr),
        "centre_outside_1024x1536": ((1024, 1536), -200.5, 1300.25, [1.001, -5e-6, 4e-9, -1e-12]),
    }


CASES = _cases()


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


@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("case", list(CASES))
def test_planned_frames_equal_the_oracle_and_the_unplanned_call(hip, orc, plan_mode, case, sampler):
    shape, xc, yc, fact = CASES[case]
    img = noise(4100 + len(case), shape)
    want = _want(orc, img, xc, yc, fact, sampler)
    src = hip.DeviceBuffer(img.nbytes).upload(img)
    dst = [hip.DeviceBuffer(img.nbytes) for _ in range(3)]
    plan_mode(2)
    _call(hip, src, dst[0], shape, xc, yc, fact, sampler)          # builds the plan and runs on it
    _call(hip, src, dst[1], shape, xc, yc, fact, sampler)          # finds it
    kernel = hip.last_kernel()
    tiles, exact = hip.get_option("x_frame_plan_tiles"), hip.get_option("x_frame_plan_exact_tiles")
    print("%s %s: %s, wave tiles %d, not certified %d" % (case, sampler, kernel, tiles, exact))
    plan_mode(0)
    _call(hip, src, dst[2], shape, xc, yc, fact, sampler)
    got = [d.download(shape, np.float32) for d in dst]
    for b in [src] + dst:
        b.free()
    assert np.array_equal(got[0], want)
    assert np.array_equal(got[1], want)
    assert np.array_equal(got[2], want)
    assert np.array_equal(got[0], got[2]) and np.array_equal(got[1], got[2])
    assert 0 <= exact <= tiles
    if kernel.startswith("remap_wg_kernel"):
        H, W = shape
        assert tiles == 4 * ((W + 127) // 128) * ((H + 31) // 32)


def test_cfg2_takes_the_fast_path_on_nearly_every_interior_tile(hip, plan_mode):
    """The condition that keeps a plan which certifies nothing from passing every equality test: at 4096 x 4096 under config 2, the
    wave tiles left on the exact evaluation number at most those of the 316 border workgroup tiles (1 264) plus 3 % of the other
    15 120."""
    c = configs.cfg2()
    shape = tuple(c["shape"])
    img = noise(c["seed"], shape)
    src = hip.DeviceBuffer(img.nbytes).upload(img)
    dst = hip.DeviceBuffer(img.nbytes)
    plan_mode(2)
    assert hip.get_option("x_frame_plan_tiles") == 0               # the cache starts empty
    _call(hip, src, dst, shape, c["xcenter"], c["ycenter"], c["list_fact"], "f64lerp")
    assert hip.last_kernel() == "remap_wg_kernel<Radial,NF=5,f64lerp>"
    tiles, exact = hip.get_option("x_frame_plan_tiles"), hip.get_option("x_frame_plan_exact_tiles")
    print("cfg2: wave tiles %d, not certified %d" % (tiles, exact))
    src.free()
    dst.free()
    assert tiles == 16384
    assert exact <= 1264 + 0.03 * 15120


def test_strong_model_reports_its_count(hip, orc, plan_mode):
    """The strong barrel model: only that the count is reported and the result equal.  (The host certifies this model for 64 x 16
    tiles only, so the frame runs on remap_lds_kernel, for which no plan exists: 0 of 0 is the count reported then.)"""
    shape, xc, yc, fact = CASES["strong_1280x1000"]
    img = noise(77, shape)
    src = hip.DeviceBuffer(img.nbytes).upload(img)
    dst = hip.DeviceBuffer(img.nbytes)
    plan_mode(2)
    _call(hip, src, dst, shape, xc, yc, fact, "f64lerp")
    _call(hip, src, dst, shape, xc, yc, fact, "f64lerp")
    tiles, exact = hip.get_option("x_frame_plan_tiles"), hip.get_option("x_frame_plan_exact_tiles")
    print("strong model: %s, wave tiles %d, not certified %d" % (hip.last_kernel(), tiles, exact))
    got = dst.download(shape, np.float32)
    src.free()
    dst.free()
    assert 0 <= exact <= tiles
    assert np.array_equal(got, _want(orc, img, xc, yc, fact, "f64lerp"))


def test_default_mode_builds_on_the_second_sighting_and_keeps_no_stale_plan(hip, orc, plan_mode):
    shape, xc, yc, fact = CASES["cfg4_model_2560"]
    xc = xc + 0.125                                               # a calibration no other test of the session has shown the library
    img = noise(91, shape)
    want = _want(orc, img, xc, yc, fact, "f64lerp")
    src = hip.DeviceBuffer(img.nbytes).upload(img)
    dst = [hip.DeviceBuffer(img.nbytes) for _ in range(4)]
    plan_mode(1)
    _call(hip, src, dst[0], shape, xc, yc, fact, "f64lerp")
    assert hip.get_option("x_frame_plan_tiles") == 0               # first sighting: remembered, nothing built
    _call(hip, src, dst[1], shape, xc, yc, fact, "f64lerp")
    assert hip.get_option("x_frame_plan_tiles") == 4 * 20 * 80     # second: built
    _call(hip, src, dst[2], shape, xc, yc, fact, "f64lerp")
    xc1 = float(np.nextafter(xc, np.inf))                          # one float64 ulp: another calibration
    _call(hip, src, dst[3], shape, xc1, yc, fact, "f64lerp")
    got = [d.download(shape, np.float32) for d in dst]
    for b in [src] + dst:
        b.free()
    for g in got[:3]:
        assert np.array_equal(g, want)
    assert np.array_equal(got[3], _want(orc, img, xc1, yc, fact, "f64lerp"))


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("unordered", [False, True])
def test_two_streams_from_the_first_call(hip, orc, plan_mode, mode, unordered):
    """Frames dealt alternately to two streams from the very first call: the stream that did not build the plan waits for it on the
    device, and a launch that may overlap its predecessor (DCP_MEM_DEVICE_UNORDERED) does not run ahead of the build."""
    c2 = configs.cfg2()
    H, W, n = 1536, 2048, 4
    xc, yc, fact = configs.rescale_model(W)
    xc += 0.25 * mode + (0.0625 if unordered else 0.0)
    frames = [noise(c2["seed"] + 50 + i, (H, W)) for i in range(n)]
    want = [_want(orc, f, xc, yc, fact, "f64lerp") for f in frames]
    src = [hip.DeviceBuffer(f.nbytes).upload(f) for f in frames]
    dst = [hip.DeviceBuffer(frames[0].nbytes) for _ in range(3 * n)]
    for d in dst:
        d.upload(np.zeros((H, W), np.float32))
    s = [hip.Stream(), hip.Stream()]
    plan_mode(mode)
    mem = hip.MEM_DEVICE_UNORDERED if unordered else hip.MEM_DEVICE
    for i in range(3 * n):
        _call(hip, src[i % n], dst[i], (H, W), xc, yc, fact, "f64lerp", mem=mem, stream=s[i & 1])
    s[0].synchronize()
    s[1].synchronize()
    assert hip.get_option("x_frame_plan_tiles") == 4 * 16 * 48
    got = [d.download((H, W), np.float32) for d in dst]
    for b in src + dst:
        b.free()
    for i in range(3 * n):
        assert np.array_equal(got[i], want[i % n]), i


def test_more_calibrations_than_the_cache_holds(hip, orc, plan_mode):
    """Twenty calibrations (the cache holds sixteen plans per device), cycled twice with a plan built at every first sight: every plan of
    the second cycle replaces one that a launch may still be reading."""
    H, W, ncal = 512, 640, 20
    xc0, yc, fact = configs.rescale_model(W)
    img = noise(5, (H, W))
    src = hip.DeviceBuffer(img.nbytes).upload(img)
    dst = [hip.DeviceBuffer(img.nbytes) for _ in range(2 * ncal)]
    plan_mode(2)
    for i in range(2 * ncal):
        _call(hip, src, dst[i], (H, W), xc0 + 0.5 * (i % ncal), yc, fact, "f64lerp")
    assert hip.get_option("x_frame_plan_tiles") == 4 * 5 * 16
    got = [d.download((H, W), np.float32) for d in dst]
    for b in [src] + dst:
        b.free()
    for i in range(ncal):
        want = _want(orc, img, xc0 + 0.5 * i, yc, fact, "f64lerp")
        assert np.array_equal(got[i], want), i
        assert np.array_equal(got[ncal + i], want), i
