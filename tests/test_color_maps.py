"""Interleaved colour images under the homography and under the one-pass perspective -> radial map
(util.correct_perspective_color_image, util.unwarp_perspective_fused_color_image): what the reference's demos write as a loop of
post.correct_perspective_image over mat[:, :, i] (examples/readthedocs_demo/demo_07.py:25,60; demo_05.py:127,147) in one launch of
remap_wg_color_kernel<Persp / Fused> or, where the call does not qualify, of typed_channels_kernel<Persp / Fused>.
Every comparison is bit for bit: against the single-plane functions on each channel under the same blend, against the oracle,
and against golden G24 (the reference's own outputs)."""
import ctypes as C

import numpy as np
import pytest

from conftest import HOST, golden, noise, oblend, typed_image

pytestmark = pytest.mark.gpu

MAP_PERSP, MAP_FUSED = 1, 2
CFG3 = (0.9450284704184375, -0.019662775048787898, 55.99511925916719, -0.01478311636447244,
        0.9403850653789713, 45.65706672670265, -8.075209829141167e-06, -1.0417072082535193e-05)
MILD = [0.98, -0.01, 3.0, 0.012, 0.97, 2.0, -1e-5, 2e-5]
STRONG = [0.9, 0.02, 4.0, -0.015, 1.1, -3.0, 6e-4, 4e-4]      # projective terms that cost a 700-pixel frame its level-2 certificate
FACT3 = [1.0, -2e-5, 3e-8]
FACT7 = [0.98, 1e-5, 1e-8, 1e-12, 1e-15, 1e-18, 1e-21]        # more than five terms: the NF = 10 instantiation


def cfg3_for(width):
    """configs.CFG3_COEF (a 4096-pixel frame) rescaled to `width` pixels as tools/gen_golden.py rescales it for G7 and G24."""
    s = 4096.0 / width
    return [CFG3[0], CFG3[1], CFG3[2] / s, CFG3[3], CFG3[4], CFG3[5] / s, CFG3[6] * s, CFG3[7] * s]


def pole_inside(width):
    """not tame: the denominator changes sign inside the frame (tests/test_gpu_parity.py, wild homographies)"""
    return [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, -1.0 / (width / 2 + 0.37), 0.0]


def case_coef(coef, width):
    return cfg3_for(width) if coef == "cfg3" else pole_inside(width) if coef == "pole" else coef


def certificate(hip, kind, h, w, radial, coef):
    ca, _ = hip.fact_array(coef)
    if kind == MAP_PERSP:
        return hip.lib().dcp_debug_tile_certificate(kind, h, w, 0.0, 0.0, None, 0, ca)
    fa, nf = hip.fact_array(radial[2])
    return hip.lib().dcp_debug_tile_certificate(kind, h, w, radial[0], radial[1], fa, nf, ca)


def staged_layout(img):
    """the layouts remap_wg_color_kernel takes: 3 / 4 dense channels of float32 / uint8 / uint16, rows a multiple of 4 bytes"""
    h, w, c = img.shape
    return c in (3, 4) and img.dtype in (np.float32, np.uint8, np.uint16) and (w * c * img.dtype.itemsize) % 4 == 0 and h >= 2 and w >= 2


def expect_kernel(hip, kind, img, radial, coef):
    level = certificate(hip, kind, img.shape[0], img.shape[1], radial, coef)
    staged = level >= 2 and staged_layout(img)
    name = hip.last_kernel()
    tag = "Persp" if kind == MAP_PERSP else "Fused"
    assert name.startswith(("remap_wg_color_kernel<%s," if staged else "typed_channels_kernel<%s>") % tag), (level, name)
    return staged


FLOAT_CASES = [
    ((40, 56, 3), MILD, (27.4, 19.1, [1.0, 3e-5, 3e-7])),                    # one partial tile
    ((40, 56, 3), "cfg3", (27.4, 19.1, [1.0, 3e-5, 3e-7])),                  # G24's homography: rescaled to 56 pixels it loses level 2
    ((17, 129, 3), MILD, (60.0, 8.0, FACT3)),                                # a one-pixel second tile column, a one-row second tile row
    ((517, 1031, 4), "cfg3", (500.0, 250.0, FACT3)),                         # ragged on both axes, four channels
    ((300, 700, 3), "cfg3", (350.0, 150.0, FACT7)),                          # seven radial terms
    ((300, 700, 3), "cfg3", (-50.0, 900.0, FACT7)),                          # ... centre far outside: the fused map loses its certificate
    ((300, 700, 3), STRONG, (350.0, 150.0, FACT3)),                          # no certificate at this width
    ((300, 700, 3), "pole", (350.0, 150.0, FACT3)),                          # not tame: IEEE division, one thread per pixel
]


@pytest.mark.parametrize("shape, coef, radial", FLOAT_CASES, ids=["%dx%dx%d-%s" % (c[0] + (c[1] if isinstance(c[1], str) else "coef%d" % i,))
                                                                  for i, c in enumerate(FLOAT_CASES)])
def test_float32_colour_equals_the_single_plane_calls_and_the_oracle(hip, orc, shape, coef, radial):
    from discorpy_amd.post import postprocessing as pp
    from discorpy_amd.util import utility as util
    coef = case_coef(coef, shape[1])
    rgb = noise(24, shape) * 255.0
    planes = [np.ascontiguousarray(rgb[:, :, c]) for c in range(shape[2])]
    for order, blend in ((1, None), (1, "scipy"), (0, None)):
        ob = oblend(orc, blend or HOST)
        got = util.correct_perspective_color_image(rgb, coef, order=order, blend=blend)
        expect_kernel(hip, MAP_PERSP, rgb, None, coef)
        assert got.dtype == np.float32 and got.shape == rgb.shape
        for c, plane in enumerate(planes):
            assert np.array_equal(got[:, :, c], pp.correct_perspective_image(plane, coef, order=order, blend=blend)), ("persp", order, blend, c)
            assert np.array_equal(got[:, :, c], orc.correct_perspective_image(plane, coef, order=order, blend=ob)), ("persp oracle", order, blend, c)
        got = util.unwarp_perspective_fused_color_image(rgb, *radial, coef, order=order, blend=blend)
        expect_kernel(hip, MAP_FUSED, rgb, radial, coef)
        assert got.dtype == np.float32 and got.shape == rgb.shape
        for c, plane in enumerate(planes):
            assert np.array_equal(got[:, :, c], pp.unwarp_perspective_fused(plane, *radial, coef, order=order, blend=blend)), ("fused", order, blend, c)
            assert np.array_equal(got[:, :, c], orc.unwarp_fused(plane, *radial, coef, order=order, poly=orc.POLY_KERNEL, blend=ob)), ("fused oracle", order, blend, c)


def test_the_float32_cases_reach_both_kernels_under_both_maps(hip):
    """Every float32 case above asserts that it ran the kernel its certificate selects (expect_kernel); here: under each map the
    certificates send at least one of those cases to the staged kernel and at least one to the fallback."""
    for kind in (MAP_PERSP, MAP_FUSED):
        counts = [0, 0]                    # [fallback, staged]
        for shape, coef, radial in FLOAT_CASES:
            counts[certificate(hip, kind, shape[0], shape[1], radial, case_coef(coef, shape[1])) >= 2] += 1
        assert counts[0] > 0 and counts[1] > 0, (kind, counts)


@pytest.mark.parametrize("dt, channels, width", [("uint8", 3, 1532), ("uint8", 4, 1001), ("uint16", 3, 1030), ("uint16", 4, 777)])
def test_integer_colour_blends_and_stores_as_scipy_does(hip, orc, dt, channels, width):
    from discorpy_amd.post import postprocessing as pp
    from discorpy_amd.util import utility as util
    rgb = typed_image(dt, (600, width, channels), 5)
    coef = cfg3_for(width)
    radial = (610.2, 333.3, [1.0, -3e-5, 4e-8])
    planes = [np.ascontiguousarray(rgb[:, :, c]) for c in range(channels)]
    yd, xd = orc.perspective_coords(600, width, coef)
    for order in (1, 0):
        got = util.correct_perspective_color_image(rgb, coef, order=order)
        assert expect_kernel(hip, MAP_PERSP, rgb, None, coef), hip.last_kernel()
        assert got.dtype == rgb.dtype and got.shape == rgb.shape
        for c, plane in enumerate(planes):
            assert np.array_equal(got[:, :, c], orc.map_coordinates(plane, yd, xd, order)), (dt, channels, order, c)
        got = util.unwarp_perspective_fused_color_image(rgb, *radial, coef, order=order)
        assert expect_kernel(hip, MAP_FUSED, rgb, radial, coef), hip.last_kernel()
        assert got.dtype == rgb.dtype and got.shape == rgb.shape
        for c, plane in enumerate(planes):
            assert np.array_equal(got[:, :, c], pp.unwarp_perspective_fused(plane, *radial, coef, order=order)), (dt, channels, order, c)


def test_what_the_staged_kernel_declines_gives_the_same_bits(hip):
    """uint8 x 3 of odd width (rows not dword-aligned), 2 / 5 channels, a pixel stride above the channel count and float64 pixels
    go to the one-thread-per-pixel kernel under a certified homography: every channel equals the single-plane call."""
    from discorpy_amd.post import postprocessing as pp
    from discorpy_amd.util import utility as util
    radial = (410.2, 233.3, [1.0, -3e-5, 4e-8])
    rgba = noise(8, (300, 640, 4))
    images = [typed_image("uint8", (300, 801, 3), 6), noise(7, (300, 640, 2)), noise(7, (300, 640, 5)), rgba[:, :, :3],
              typed_image("float64", (300, 640, 3), 9)]
    for img in images:
        h, w, nc = img.shape
        coef = cfg3_for(w)
        assert certificate(hip, MAP_PERSP, h, w, None, coef) >= 2 and certificate(hip, MAP_FUSED, h, w, radial, coef) >= 2
        for blend in ((None, "scipy") if img.dtype == np.float32 else (None,)):
            got = util.correct_perspective_color_image(img, coef, blend=blend)
            assert hip.last_kernel().startswith("typed_channels_kernel<Persp>"), hip.last_kernel()
            assert got.dtype == img.dtype and got.shape == img.shape
            for c in range(nc):
                assert np.array_equal(got[:, :, c], pp.correct_perspective_image(np.ascontiguousarray(img[:, :, c]), coef, blend=blend)), (img.dtype, nc, c)
            got = util.unwarp_perspective_fused_color_image(img, *radial, coef, blend=blend)
            assert hip.last_kernel().startswith("typed_channels_kernel<Fused>"), hip.last_kernel()
            for c in range(nc):
                assert np.array_equal(got[:, :, c], pp.unwarp_perspective_fused(np.ascontiguousarray(img[:, :, c]), *radial, coef, blend=blend)), (img.dtype, nc, c)


@pytest.mark.parametrize("tag", ["f32", "u8"])
def test_golden_g24_through_both_functions(hip, tag):
    """The reference's own outputs (tools/gen_golden.py runs demo_07's loop of post.correct_perspective_image, and G7's composed
    planes per channel) from host arrays, on whichever kernel the certificate selects; order 3 goes plane by plane."""
    from discorpy_amd.post import postprocessing as pp
    from discorpy_amd.util import utility as util
    g = golden("g24_colour_homography40x56x3")
    rgb = g["rgb_" + tag]
    coef = list(g["list_coef"])
    radial = (float(g["xcenter"]), float(g["ycenter"]), list(g["list_fact"]))
    for order in (1, 0, 3):
        got = util.correct_perspective_color_image(rgb, coef, order=order, blend="scipy")
        if order <= 1:
            expect_kernel(hip, MAP_PERSP, rgb, None, coef)
        assert got.dtype == rgb.dtype and np.array_equal(got, g["persp_%s_o%d" % (tag, order)]), ("persp", tag, order)
        fused = util.unwarp_perspective_fused_color_image(rgb, *radial, coef, order=order, blend="scipy")
        if order <= 1:
            expect_kernel(hip, MAP_FUSED, rgb, radial, coef)
        assert fused.dtype == rgb.dtype and np.array_equal(fused, g["fused_%s_o%d" % (tag, order)]), ("fused", tag, order)
        if order == 3:         # the plane-by-plane route: exactly the single-plane calls
            for c in range(3):
                assert np.array_equal(got[:, :, c], pp.correct_perspective_image(rgb[:, :, c], coef, order=3, blend="scipy"))
                assert np.array_equal(fused[:, :, c], pp.unwarp_perspective_fused(rgb[:, :, c], *radial, coef, order=3, blend="scipy"))
    # map_index= goes plane by plane too: the reference's composed float32 planes give the fused output
    via_map = util.correct_perspective_color_image(rgb, coef, map_index=(g["yd"].reshape(-1, 1), g["xd"].reshape(-1, 1)), blend="scipy")
    assert np.array_equal(via_map, g["fused_%s_o1" % tag])


def test_a_rocm_tensor_in_gives_a_rocm_tensor_out(hip):
    import torch
    from discorpy_amd.util import utility as util
    rgb = noise(31, (150, 260, 3))
    coef = cfg3_for(260)
    radial = (120.5, 80.25, FACT3)
    t = torch.from_numpy(rgb).cuda()
    for blend in ("scipy", "f64lerp"):
        dev = util.correct_perspective_color_image(t, coef, blend=blend)
        assert isinstance(dev, torch.Tensor) and dev.is_cuda and dev.dtype == torch.float32 and tuple(dev.shape) == rgb.shape
        torch.cuda.synchronize()
        assert np.array_equal(dev.cpu().numpy(), util.correct_perspective_color_image(rgb, coef, blend=blend)), blend
        dev = util.unwarp_perspective_fused_color_image(t, *radial, coef, blend=blend)
        assert isinstance(dev, torch.Tensor) and dev.is_cuda and tuple(dev.shape) == rgb.shape
        torch.cuda.synchronize()
        assert np.array_equal(dev.cpu().numpy(), util.unwarp_perspective_fused_color_image(rgb, *radial, coef, blend=blend)), blend
    u8 = typed_image("uint8", (150, 260, 4), 32)
    dev = util.correct_perspective_color_image(torch.from_numpy(u8).cuda(), coef, order=0)
    torch.cuda.synchronize()
    assert dev.dtype == torch.uint8 and np.array_equal(dev.cpu().numpy(), util.correct_perspective_color_image(u8, coef, order=0))


def test_a_host_array_past_the_staged_whole_path_equals_the_device_result(hip):
    """512 rows and 16 MiB are where host_path (api_image.cpp) stops staging a host frame whole: 512 x 2731 x 3 float32 is the
    smallest such image of three float32 channels (2730 pixels a row stay 4 096 bytes below)."""
    import torch
    from discorpy_amd.util import utility as util
    h, w, nc = 512, 2731, 3
    assert h * w * nc * 4 >= 16 * 1048576 > h * (w - 1) * nc * 4
    rgb = noise(33, (h, w, nc))
    coef = cfg3_for(w)
    radial = (1300.5, 250.25, [1.0, -3e-6, 1e-9])
    t = torch.from_numpy(rgb).cuda()
    dev = util.correct_perspective_color_image(t, coef, blend="scipy")
    torch.cuda.synchronize()
    assert np.array_equal(util.correct_perspective_color_image(rgb, coef, blend="scipy"), dev.cpu().numpy())
    dev = util.unwarp_perspective_fused_color_image(t, *radial, coef, blend="scipy")
    torch.cuda.synchronize()
    assert np.array_equal(util.unwarp_perspective_fused_color_image(rgb, *radial, coef, blend="scipy"), dev.cpu().numpy())


# ---- the error contract of the two entry points (as tests/test_abi_contract.py has it for dcp_unwarp_color_image)
_H, _W = 8, 10
_keep = []


def _buf(nbytes):
    a = np.zeros(int(nbytes), np.uint8)
    _keep.append(a)
    return a.ctypes.data


def _dbl(vals):
    a = np.array(vals, np.float64)
    _keep.append(a)
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _entries():
    from discorpy_amd import _ffi as F
    img = dict(src=_buf(_H * _W * 3 * 4), dst=_buf(_H * _W * 3 * 4), dtype=F.DTYPE_F32, height=_H, width=_W, channels=3, rs=3 * _W, cs=3)
    tail = dict(order=1, blend=F.BLEND_SCIPY, mem_kind=F.MEM_HOST, device=-1, stream=None)
    coef = _dbl([1.0, 0.0, 0.5, 0.0, 1.0, -0.5, 0.0, 0.0])
    return {"dcp_perspective_color_image": ("src dst dtype height width channels rs cs coef order blend mem_kind device stream",
                                            dict(img, coef=coef, **tail)),
            "dcp_unwarp_fused_color_image": ("src dst dtype height width channels rs cs xc yc fact nfact coef order blend mem_kind device stream",
                                             dict(img, xc=5.0, yc=4.0, fact=_dbl([1.0, -1e-4, 0.0]), nfact=3, coef=coef, **tail))}


@pytest.mark.parametrize("name", ["dcp_perspective_color_image", "dcp_unwarp_fused_color_image"])
@pytest.mark.parametrize("override, code, fragment", [
    ({"channels": 0}, "ERR_INVALID_ARG", "channels = 0 outside [1, 64]"),
    ({"order": 2}, "ERR_UNSUPPORTED", "the interleaved-channel kernels take orders 0 an"),
    ({"coef": None}, "ERR_INVALID_ARG", "null homography pointer"),
    ({"mem_kind": 0x101}, "ERR_INVALID_ARG", "unknown mem_kind 257"),
], ids=["channels=0", "order=2", "coef=None", "mem_kind=0x101"])
def test_invalid_argument_is_refused(hip, name, override, code, fragment):
    from discorpy_amd import _ffi as F
    names, base = _entries()[name]
    args = dict(base, **override)
    got = getattr(F.lib(), name)(*[args[k] for k in names.split()])
    assert (got, fragment in F.last_error()) == (getattr(F, code), True), (got, F.last_error())


@pytest.mark.parametrize("name", ["dcp_perspective_color_image", "dcp_unwarp_fused_color_image"])
def test_the_valid_call_of_the_contract_cases_succeeds(hip, name):
    from discorpy_amd import _ffi as F
    names, base = _entries()[name]
    F.check(getattr(F.lib(), name)(*[base[k] for k in names.split()]))
