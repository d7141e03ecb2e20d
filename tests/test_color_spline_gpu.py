"""Colour images at spline orders 2..5 in one call (util.unwarp_color_image_backward, util.correct_perspective_color_image,
util.unwarp_perspective_fused_color_image -> dcp_*_color_image_spline): a prefilter per channel, then ONE gather launch of
spline_wg_color_kernel (certified radial / perspective maps on frames of at least one 128 x 32 tile) or spline_remap_color_kernel.

The contract: every channel of the result is bit for bit what the single-plane function (post.unwarp_image_backward,
post.correct_perspective_image, post.unwarp_perspective_fused) returns for the strided view mat[:, :, c] with the same arguments --
under blend="scipy" and under the default factorised sum, from host and device arrays, on both gather kernels.  Beside it: the
reference's own outputs (goldens G25 and G24), the oracle, the workspace slots on two streams and the error contract of the ABI."""
import ctypes as C

import numpy as np
import pytest

from conftest import golden, noise, typed_image, ulp_diff

pytestmark = pytest.mark.gpu

MAP_RADIAL, MAP_PERSP, MAP_FUSED = 0, 1, 2
MODES8 = ("reflect", "grid-mirror", "constant", "grid-constant", "nearest", "mirror", "grid-wrap", "wrap")
MODES = ("reflect", "mirror", "nearest", "grid-constant", "grid-wrap", "constant")
DTYPES = ("float32", "uint8", "uint16", "int16", "float64")
CFG3 = (0.9450284704184375, -0.019662775048787898, 55.99511925916719, -0.01478311636447244,
        0.9403850653789713, 45.65706672670265, -8.075209829141167e-06, -1.0417072082535193e-05)
MILD = [0.98, -0.01, 3.0, 0.012, 0.97, 2.0, -1e-5, 2e-5]
STRONG = [0.9, 0.02, 4.0, -0.015, 1.1, -3.0, 6e-4, 4e-4]      # projective terms that cost a 700-pixel frame its level-2 certificate
FACT3 = [1.0, -2e-5, 3e-8]
FACT7 = [0.98, 1e-5, 1e-8, 1e-12, 1e-15, 1e-18, 1e-21]        # more than five terms: the NF = -1 instantiation of the staged kernel
TILE_W, TILE_H = 128, 32                                       # spline_wg_kernel's workgroup tile


def cfg3_for(width):
    """configs.CFG3_COEF (a 4096-pixel frame) rescaled to `width` pixels as tools/gen_golden.py rescales it for G7 and G24."""
    s = 4096.0 / width
    return [CFG3[0], CFG3[1], CFG3[2] / s, CFG3[3], CFG3[4], CFG3[5] / s, CFG3[6] * s, CFG3[7] * s]


def spline_close(got, ref):
    """tests/test_gpu_parity.py's criterion for frames whose lines are prefiltered in chunks"""
    d = ulp_diff(got, ref)
    return d.max() <= 1 and np.count_nonzero(d) <= max(2, got.size // 500)


def certificate(hip, kind, h, w, radial, coef):
    if kind == MAP_RADIAL:
        fa, nf = hip.fact_array(radial[2])
        return hip.lib().dcp_debug_tile_certificate(kind, h, w, radial[0], radial[1], fa, nf, None)
    ca, _ = hip.fact_array(coef)
    if kind == MAP_PERSP:
        return hip.lib().dcp_debug_tile_certificate(kind, h, w, 0.0, 0.0, None, 0, ca)
    fa, nf = hip.fact_array(radial[2])
    return hip.lib().dcp_debug_tile_certificate(kind, h, w, radial[0], radial[1], fa, nf, ca)


def expect_kernel(hip, kind, shape, radial, coef, order, wg_option=1):
    """The size rule and the certificate decide the gather kernel (launch_spline_color): the staged one under a level-2 certificate
    of a radial or perspective map on a frame of at least one tile.  Returns whether the staged kernel ran."""
    h, w, nc = shape
    staged = bool(kind != MAP_FUSED and certificate(hip, kind, h, w, radial, coef) >= 2 and h >= TILE_H and w >= TILE_W and wg_option)
    name = hip.last_kernel()
    tail = "+ %s<order=%d, channels=%d>" % ("spline_wg_color_kernel" if staged else "spline_remap_color_kernel", order, nc)
    assert name.endswith(tail) and name.startswith("spline_"), (name, tail)
    return staged


def calls(kind, radial, coef):
    """(colour function, single-plane function) of a map kind, as functions of (image, order=, mode=, blend=)"""
    from discorpy_amd.post import postprocessing as pp
    from discorpy_amd.util import utility as util
    if kind == MAP_RADIAL:
        return (lambda m, **kw: util.unwarp_color_image_backward(m, *radial, **kw), lambda m, **kw: pp.unwarp_image_backward(m, *radial, **kw))
    if kind == MAP_PERSP:
        return (lambda m, **kw: util.correct_perspective_color_image(m, coef, **kw), lambda m, **kw: pp.correct_perspective_image(m, coef, **kw))
    return (lambda m, **kw: util.unwarp_perspective_fused_color_image(m, *radial, coef, **kw),
            lambda m, **kw: pp.unwarp_perspective_fused(m, *radial, coef, **kw))


def image_of(dt, shape, seed):
    return noise(seed, shape) * np.float32(255.0) if dt == "float32" else typed_image(dt, shape, seed)


# shape, homography, radial model: the smallest frames at which each path can go wrong
CASES = [
    ((40, 56, 3), MILD, (27.4, 19.1, [1.0, 0.004, 2e-5])),          # under one tile: the global kernel
    ((33, 129, 2), MILD, (60.0, 8.0, FACT3)),                       # one full tile, a one-pixel tile column, a one-row tile row
    ((70, 300, 3), "cfg3", (150.3, 35.2, FACT3)),                   # ragged staged tiles
    ((517, 1031, 4), "cfg3", (500.0, 250.0, FACT3)),                # ragged staged tiles, four channels, lines prefiltered in chunks
    ((300, 700, 3), STRONG, (350.0, 150.0, FACT7)),                 # uncertified homography; seven radial terms (NF = -1)
    ((70, 300, 1), "cfg3", (150.3, 35.2, FACT3)),                   # one channel
]
CASE_IDS = ["%dx%dx%d" % c[0] for c in CASES]


def case_coef(coef, width):
    return cfg3_for(width) if isinstance(coef, str) else coef


def combos(case_index):
    """(kind, blend, order, mode, dtype) for all three maps x both blends x orders 2..5; boundary modes and element types cycle
    through them with different periods (6 and 5 against 24 combinations), shifted from case to case."""
    i = case_index
    for kind in (MAP_RADIAL, MAP_PERSP, MAP_FUSED):
        for blend in (None, "scipy"):
            for order in (2, 3, 4, 5):
                yield kind, blend, order, MODES[i % len(MODES)], DTYPES[i % len(DTYPES)]
                i += 1


def test_the_combinations_cover_every_mode_and_element_type_on_both_kernels_and_blends():
    for ci in range(len(CASES)):
        seen = list(combos(ci))
        assert len(seen) == 24 and {s[3] for s in seen} == set(MODES) and {s[4] for s in seen} == set(DTYPES)
        for blend in (None, "scipy"):
            assert {s[4] for s in seen if s[1] == blend} == set(DTYPES), (ci, blend)
    # every element type meets every order and both blends under the radial map (the staged kernel's) over the staged cases
    radial = {(s[4], s[2], s[1]) for ci in (1, 2, 3, 4, 5) for s in combos(ci) if s[0] == MAP_RADIAL}
    assert {r[0] for r in radial} == set(DTYPES) and {(r[1], r[2]) for r in radial} == {(o, b) for o in (2, 3, 4, 5) for b in (None, "scipy")}


@pytest.mark.parametrize("ci", range(len(CASES)), ids=CASE_IDS)
def test_every_channel_equals_the_single_plane_call(hip, ci):
    shape, coef, radial = CASES[ci]
    coef = case_coef(coef, shape[1])
    images = {dt: image_of(dt, shape, 40 + ci) for dt in DTYPES}
    kernels = set()
    for kind, blend, order, mode, dt in combos(ci):
        colour, plane = calls(kind, radial, coef)
        img = images[dt]
        got = colour(img, order=order, mode=mode, blend=blend)
        kernels.add((kind, expect_kernel(hip, kind, shape, radial, coef, order)))
        assert isinstance(got, np.ndarray) and got.dtype == img.dtype and got.shape == img.shape
        for c in range(shape[2]):
            want = plane(img[:, :, c], order=order, mode=mode, blend=blend)
            assert np.array_equal(got[:, :, c], want), (kind, blend, order, mode, dt, c, int(np.count_nonzero(got[:, :, c] != want)))
    # which kernels this case is there for
    if ci == 0:
        assert kernels == {(MAP_RADIAL, False), (MAP_PERSP, False), (MAP_FUSED, False)}
    elif ci == 4:
        assert kernels == {(MAP_RADIAL, True), (MAP_PERSP, False), (MAP_FUSED, False)}
    else:
        assert kernels == {(MAP_RADIAL, True), (MAP_PERSP, True), (MAP_FUSED, False)}


@pytest.mark.parametrize("layout", ["rgba[:, :, :3]", "padded rows", "both"])
def test_a_non_dense_image_is_read_in_place(hip, layout):
    """Three channels of a four-channel buffer, rows padded by a few elements: pixel stride 4, row stride above width x pixel stride."""
    h, w = 70, 300
    coef, radial = cfg3_for(w), (150.3, 35.2, FACT3)
    for dt, order, mode, blend in (("float32", 3, "reflect", None), ("uint8", 3, "nearest", "scipy"), ("uint16", 5, "mirror", None),
                                   ("float64", 2, "grid-wrap", None), ("int16", 4, "constant", "scipy")):
        buf = image_of(dt, (h, w + 5, 4), 77)
        img = {"rgba[:, :, :3]": buf[:, :w + 5, :3], "padded rows": buf[:, :w, :], "both": buf[:, :w, :3]}[layout]
        nc = img.shape[2]
        assert not img.flags.c_contiguous and img.strides[2] == img.itemsize and img.strides[1] == 4 * img.itemsize
        for kind in (MAP_RADIAL, MAP_PERSP, MAP_FUSED):
            colour, plane = calls(kind, radial, coef)
            got = colour(img, order=order, mode=mode, blend=blend)
            expect_kernel(hip, kind, img.shape, radial, coef, order)
            assert got.flags.c_contiguous and got.shape == img.shape and got.dtype == img.dtype
            for c in range(nc):
                assert np.array_equal(got[:, :, c], plane(img[:, :, c], order=order, mode=mode, blend=blend)), (layout, dt, kind, c)


@pytest.mark.parametrize("ci", [2, 3], ids=[CASE_IDS[2], CASE_IDS[3]])
def test_rocm_tensors_give_the_same_bits_as_host_arrays(hip, ci):
    import torch
    shape, coef, radial = CASES[ci]
    coef = case_coef(coef, shape[1])
    for dt, order, mode in (("float32", 3, "reflect"), ("uint8", 3, "nearest"), ("float64", 5, "mirror"), ("int16", 2, "grid-wrap"),
                            ("float32", 4, "grid-constant")):
        img = image_of(dt, shape, 50 + ci)
        dev = torch.from_numpy(img).cuda()
        for kind in (MAP_RADIAL, MAP_PERSP, MAP_FUSED):
            colour, plane = calls(kind, radial, coef)
            for blend in (None, "scipy"):
                got = colour(dev, order=order, mode=mode, blend=blend)
                assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == dev.dtype and tuple(got.shape) == shape
                expect_kernel(hip, kind, shape, radial, coef, order)
                torch.cuda.synchronize()
                assert np.array_equal(got.cpu().numpy(), colour(img, order=order, mode=mode, blend=blend)), (dt, order, kind, blend)
                for c in range(shape[2]):
                    assert torch.equal(got[:, :, c], plane(dev[:, :, c], order=order, mode=mode, blend=blend)), (dt, order, kind, blend, c)
        # a view of a wider device buffer, read in place
        rgba = torch.from_numpy(image_of(dt, (shape[0], shape[1], shape[2] + 1), 60)).cuda()
        view = rgba[:, :, :shape[2]]
        colour, plane = calls(MAP_RADIAL, radial, coef)
        got = colour(view, order=order, mode=mode)
        for c in range(shape[2]):
            assert torch.equal(got[:, :, c], plane(view[:, :, c], order=order, mode=mode)), (dt, c)


def test_a_staged_case_without_the_staged_kernel_gives_the_same_bits(hip):
    """x_spline_wg = 0 sends every frame to the global kernel; under blend="scipy" both kernels sum the taps in scipy's order with
    scipy's weights, so the bits are the same (the default blend's factorised sum is the staged kernel's alone: there the single-plane
    call, under the same option, is the reference)."""
    from discorpy_amd.post import postprocessing as pp
    from discorpy_amd.util import utility as util
    shape, coef, radial = CASES[2]
    coef = case_coef(coef, shape[1])
    img = image_of("float32", shape, 91)
    u16 = image_of("uint16", shape, 92)
    staged = {}
    for order in (3, 5):
        staged[order] = util.unwarp_color_image_backward(img, *radial, order=order, blend="scipy")
        assert expect_kernel(hip, MAP_RADIAL, shape, radial, coef, order)
        staged[order, "p"] = util.correct_perspective_color_image(u16, coef, order=order, mode="mirror", blend="scipy")
        assert expect_kernel(hip, MAP_PERSP, shape, radial, coef, order)
    hip.set_option("x_spline_wg", 0)
    try:
        for order in (3, 5):
            got = util.unwarp_color_image_backward(img, *radial, order=order, blend="scipy")
            assert not expect_kernel(hip, MAP_RADIAL, shape, radial, coef, order, wg_option=0)
            assert np.array_equal(got, staged[order]), order
            got = util.correct_perspective_color_image(u16, coef, order=order, mode="mirror", blend="scipy")
            assert not expect_kernel(hip, MAP_PERSP, shape, radial, coef, order, wg_option=0)
            assert np.array_equal(got, staged[order, "p"]), order
            got = util.unwarp_color_image_backward(img, *radial, order=order)
            for c in range(3):
                assert np.array_equal(got[:, :, c], pp.unwarp_image_backward(img[:, :, c], *radial, order=order)), (order, c)
    finally:
        hip.set_option("x_spline_wg", 1)


@pytest.mark.parametrize("source", ["numpy", "torch"])
def test_golden_g25_and_g24_order_3(hip, source):
    """The reference's own outputs, blend="scipy", from NumPy arrays and from ROCm tensors: bit-equal, through the new kernels."""
    from discorpy_amd.util import utility as util
    if source == "torch":
        import torch

    def put(a):
        return torch.from_numpy(a).cuda() if source == "torch" else a

    def get(a):
        return a.cpu().numpy() if source == "torch" else a

    def ran(order):
        name = hip.last_kernel()
        assert name.endswith("+ spline_remap_color_kernel<order=%d, channels=3>" % order), name      # (40 x 56: under one tile)

    g = golden("g25_colour_spline40x56x3")
    a = (float(g["xcenter"]), float(g["ycenter"]), list(g["list_fact"]))
    f32, u8 = put(g["rgb_f32"]), put(g["rgb_u8"])
    for order in (2, 3, 4, 5):
        for mode in ("reflect", "nearest", "grid-wrap"):
            got = get(util.unwarp_color_image_backward(f32, *a, order=order, mode=mode, blend="scipy"))
            ran(order)
            assert got.dtype == np.float32 and np.array_equal(got, g["f32_o%d_%s" % (order, mode.replace("-", "_"))]), (order, mode)
    for mode in MODES8:
        got = get(util.unwarp_color_image_backward(u8, *a, order=3, mode=mode, blend="scipy"))
        ran(3)
        assert got.dtype == np.uint8 and np.array_equal(got, g["u8_o3_%s" % mode.replace("-", "_")]), mode
    got = get(util.unwarp_color_image_backward(f32, *a, order=3, mode="reflect", pad=4, pad_mode="edge", blend="scipy"))
    ran(3)
    assert np.array_equal(got, g["f32_o3_reflect_pad_4_edge"])
    g = golden("g24_colour_homography40x56x3")
    coef = list(g["list_coef"])
    radial = (float(g["xcenter"]), float(g["ycenter"]), list(g["list_fact"]))
    for tag in ("f32", "u8"):
        rgb = put(g["rgb_" + tag])
        got = get(util.correct_perspective_color_image(rgb, coef, order=3, blend="scipy"))
        ran(3)
        assert got.dtype == g["rgb_" + tag].dtype and np.array_equal(got, g["persp_%s_o3" % tag]), tag
        got = get(util.unwarp_perspective_fused_color_image(rgb, *radial, coef, order=3, blend="scipy"))
        ran(3)
        assert got.dtype == g["rgb_" + tag].dtype and np.array_equal(got, g["fused_%s_o3" % tag]), tag


def test_the_oracle_bit_for_bit_under_one_tile(hip, orc):
    """(40, 56, 3): every line is prefiltered by one serial recursion, so GPU and oracle agree to the last bit."""
    from discorpy_amd.util import utility as util
    shape, coef, radial = CASES[0]
    yd, xd = orc.perspective_coords(shape[0], shape[1], coef)
    for dt in ("float32", "uint8", "uint16"):
        img = image_of(dt, shape, 70)
        planes = [np.ascontiguousarray(img[:, :, c]) for c in range(3)]
        for order in (2, 3, 4, 5):
            for mode in MODES:
                got = util.unwarp_color_image_backward(img, *radial, order=order, mode=mode, blend="scipy")
                for c in range(3):
                    assert np.array_equal(got[:, :, c], orc.unwarp_image_backward(planes[c], *radial, order=order, mode=mode, poly=orc.POLY_KERNEL)), (dt, order, mode, c)
                got = util.correct_perspective_color_image(img, coef, order=order, mode=mode, blend="scipy")
                for c in range(3):
                    assert np.array_equal(got[:, :, c], orc.map_coordinates(planes[c], yd, xd, order, mode)), (dt, order, mode, c)


def test_the_oracle_on_a_frame_prefiltered_in_chunks(hip, orc):
    """(517, 1031, 4): lines longer than 256 samples restart their recursions chunk by chunk, which rules out bit equality exactly as
    for single planes -- the criterion of tests/test_gpu_parity.py (at most one ulp on at most size // 500 elements, at most 8
    differing elements per plane), which the single-plane kernels hold on larger frames and per-plane bit equality carries over."""
    from discorpy_amd.util import utility as util
    shape, coef, radial = CASES[3]
    img = noise(81, shape)
    planes = [np.ascontiguousarray(img[:, :, c]) for c in range(4)]
    for order, mode in [(3, "reflect"), (5, "mirror"), (2, "grid-wrap"), (4, "nearest")]:
        for blend in (None, "scipy"):
            got = util.unwarp_color_image_backward(img, *radial, order=order, mode=mode, blend=blend)
            assert expect_kernel(hip, MAP_RADIAL, shape, radial, None, order)
            for c in range(4):
                want = orc.unwarp_image_backward(planes[c], *radial, order=order, mode=mode, poly=orc.POLY_KERNEL)
                differing = int(np.count_nonzero(got[:, :, c] != want))
                print("order %d %-9s blend %-5s plane %d: %d differing elements, at most %d ulp" % (order, mode, blend, c, differing,
                                                                                                  int(ulp_diff(got[:, :, c], want).max())))
                assert spline_close(got[:, :, c], want), (order, mode, blend, c)
                assert differing <= 8, (order, mode, blend, c)


def test_the_tallest_boxes_at_three_channels(hip):
    """The calibration and frame size of tests/test_gpu_parity.py::test_spline_gather_tiles_with_the_tallest_boxes -- boxes of the
    slab's full height, where the last LDS-DMA load of a fill must keep its trailing lanes masked for EVERY channel -- at three
    channels, orders 3 and 5, both blends, once each, against the single-plane calls."""
    import torch
    from discorpy_amd.post import postprocessing as pp
    from discorpy_amd.util import utility as util
    h, w = 1571, 1532
    img = (np.random.default_rng(5).random((h, w, 3)) * 400.0 - 100.0).astype(np.float32)
    xc, yc, fact = 499.99635858988756, 218.84785084205987, [1.0, 1.9458361635865997e-05, 6.617751424219899e-09, 8.312873297400471e-13]
    dev = torch.from_numpy(img).cuda()
    for order in (3, 5):
        for blend in (None, "scipy"):
            got = util.unwarp_color_image_backward(dev, xc, yc, fact, order=order, mode="reflect", blend=blend)
            assert hip.last_kernel().endswith("+ spline_wg_color_kernel<order=%d, channels=3>" % order), hip.last_kernel()
            for c in range(3):
                want = pp.unwarp_image_backward(dev[:, :, c], xc, yc, fact, order=order, mode="reflect", blend=blend)
                assert "spline_wg_kernel" in hip.last_kernel()
                assert torch.equal(got[:, :, c], want), (order, blend, c, int((got[:, :, c] != want).sum()))


def test_four_alternating_calls_on_two_streams(hip):
    """Device tensors, two streams, four colour calls handed over alternately: each stream keeps its workspace slot of
    (channels + 1) planes, and the results equal the serial ones."""
    import torch
    from discorpy_amd.util import utility as util
    shape, coef, radial = CASES[3]
    coef = case_coef(coef, shape[1])
    a = torch.from_numpy(noise(95, shape)).cuda()
    b = torch.from_numpy(noise(96, (300, 700, 3))).cuda()
    jobs = [lambda: util.unwarp_color_image_backward(a, *radial, order=3),
            lambda: util.correct_perspective_color_image(b, cfg3_for(700), order=5, mode="mirror"),
            lambda: util.unwarp_perspective_fused_color_image(a, *radial, coef, order=2, mode="nearest", blend="scipy"),
            lambda: util.unwarp_color_image_backward(b, 350.0, 150.0, FACT7, order=4, mode="grid-wrap")]
    serial = [job() for job in jobs]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for s in streams:
        s.wait_stream(torch.cuda.current_stream())
    results = []
    for rep in range(2):
        for k, job in enumerate(jobs):
            with torch.cuda.stream(streams[k % 2]):
                results.append((k, job()))
    torch.cuda.synchronize()
    assert len(results) == 8
    for k, got in results:
        assert torch.equal(got, serial[k]), k


# ---- the error contract of the three entry points: refused with the right code before any launch
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
    tail = dict(order=3, mode=0, mem_kind=F.MEM_HOST, device=-1, stream=None)
    coef = _dbl([1.0, 0.0, 0.5, 0.0, 1.0, -0.5, 0.0, 0.0])
    fact = _dbl([1.0, -1e-4, 0.0])
    return {"dcp_unwarp_color_image_spline": ("src dst dtype height width channels rs cs xc yc fact nfact order mode mem_kind device stream",
                                              dict(img, xc=5.0, yc=4.0, fact=fact, nfact=3, **tail), "fact"),
            "dcp_perspective_color_image_spline": ("src dst dtype height width channels rs cs coef order mode mem_kind device stream",
                                                   dict(img, coef=coef, **tail), "coef"),
            "dcp_unwarp_fused_color_image_spline": ("src dst dtype height width channels rs cs xc yc fact nfact coef order mode mem_kind device stream",
                                                    dict(img, xc=5.0, yc=4.0, fact=fact, nfact=3, coef=coef, **tail), "coef")}


NAMES = ["dcp_unwarp_color_image_spline", "dcp_perspective_color_image_spline", "dcp_unwarp_fused_color_image_spline"]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("override, code, fragment", [
    ({"order": 1}, "ERR_INVALID_ARG", "spline order 1 outside [2, 5]"),
    ({"order": 6}, "ERR_INVALID_ARG", "spline order 6 outside [2, 5]"),
    ({"channels": 0}, "ERR_INVALID_ARG", "channels = 0 outside [1, 4]"),
    ({"channels": 5, "cs": 5, "rs": 5 * _W}, "ERR_INVALID_ARG", "channels = 5 outside [1, 4]"),
    ({"cs": 2}, "ERR_INVALID_ARG", "pixel stride 2 smaller than 3 channels"),
    ({"rs": 3 * _W - 1}, "ERR_INVALID_ARG", "overlaps rows"),
    ({"mode": 8}, "ERR_INVALID_ARG", "unknown boundary mode 8"),
    ({"mode": 0x108}, "ERR_INVALID_ARG", "unknown boundary mode"),
    ({"mem_kind": 0x101}, "ERR_INVALID_ARG", "unknown mem_kind 257"),
    ({"null": True}, "ERR_INVALID_ARG", "null"),
    ({"dtype": 11}, "ERR_INVALID_ARG", "unknown element type 11"),
], ids=["order=1", "order=6", "channels=0", "channels=5", "pixel stride<channels", "rows overlap", "mode=8", "mode=8|SCIPY_SUM", "mem_kind=0x101",
        "null coefficients", "dtype=11"])
def test_invalid_argument_is_refused_without_a_launch(hip, name, override, code, fragment):
    from discorpy_amd import _ffi as F
    from discorpy_amd.post import postprocessing as pp
    names, base, coefficients = _entries()[name]
    pp.unwarp_image_backward(noise(1, (8, 10)), 5.0, 4.0, [1.0, 1e-3])          # names the last kernel: any later launch would rename it
    before = F.last_kernel()
    assert before and "spline" not in before
    args = dict(base, **({coefficients: None} if "null" in override else override))
    got = getattr(F.lib(), name)(*[args[k] for k in names.split()])
    assert (got, fragment in F.last_error()) == (getattr(F, code), True), (got, F.last_error())
    assert F.last_kernel() == before


@pytest.mark.parametrize("name", NAMES)
def test_the_valid_call_of_the_contract_cases_succeeds(hip, name):
    from discorpy_amd import _ffi as F
    names, base, _ = _entries()[name]
    for mode in (0, 7, 0x100, 0x104):
        F.check(getattr(F.lib(), name)(*[dict(base, mode=mode)[k] for k in names.split()]))
    assert F.last_kernel().endswith("+ spline_remap_color_kernel<order=3, channels=3>"), F.last_kernel()
