"""Frames of one calibration under the homography and under the one-pass perspective -> radial map in ONE launch of
stack_wg_kernel<Persp / Fused> (dcp_remap_frames_typed, post.correct_perspective_images, post.unwarp_perspective_fused_images), and
frame by frame where that kernel does not apply.  Every comparison is bit for bit: against the oracle and against the single-frame
function on each frame under the same blend."""
import ctypes as C

import numpy as np
import pytest

from conftest import noise, oblend, typed_image
from discorpy_amd import configs

pytestmark = pytest.mark.gpu

MAP_PERSP, MAP_FUSED = 1, 2
MILD = [0.98, -0.01, 3.0, 0.012, 0.97, 2.0, -1e-5, 2e-5]
STRONG = [0.9, 0.02, 4.0, -0.015, 1.1, -3.0, 6e-4, 4e-4]      # level 1 (perspective) / 0 (fused) at 480 x 420: frame by frame
FACT3 = [1.0, -2e-5, 3e-8]
FACT5 = [1.002, -3e-5, 9e-8, -1.5e-10, 8e-14]
FACT7 = [0.98, 1e-5, 1e-8, 1e-12, 1e-15, 1e-18, 1e-21]
N = 9                                                          # three depth chunks of four frames, the last one ragged
DTYPE = {"float32": 0, "float64": 1, "uint8": 2, "uint16": 4, "int32": 7}


def cfg3_for(width):
    """configs.CFG3_COEF (a 4096-pixel frame) rescaled to `width` pixels"""
    s = 4096.0 / width
    c = configs.CFG3_COEF
    return [c[0], c[1], c[2] / s, c[3], c[4], c[5] / s, c[6] * s, c[7] * s]


def pole_inside(width):
    """not tame: the denominator changes sign inside the frame"""
    return [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, -1.0 / (width / 2 + 0.37), 0.0]


def centre(h, w):
    return (w / 2 + 0.3, h / 2 - 0.2)


def certificate(hip, kind, h, w, radial, coef):
    ca, _ = hip.fact_array(coef)
    if kind == MAP_PERSP:
        return hip.lib().dcp_debug_tile_certificate(kind, h, w, 0.0, 0.0, None, 0, ca)
    fa, nf = hip.fact_array(radial[2])
    return hip.lib().dcp_debug_tile_certificate(kind, h, w, radial[0], radial[1], fa, nf, ca)


class forced:
    """x_stack_wg = 2 (stack_wg_kernel whenever the call is eligible, however small) inside the block, 1 after it"""

    def __init__(self, hip, value=2):
        self.hip, self.value = hip, value

    def __enter__(self):
        self.hip.set_option("x_stack_wg", self.value)

    def __exit__(self, *exc):
        self.hip.set_option("x_stack_wg", 1)


def frames_call(hip, frames, kind, radial, coef, order=1, blend="f64lerp", gap=4096):
    """dcp_remap_frames_typed on a device buffer that holds `frames` with `gap` elements between the end of one and the start of the next"""
    n, h, w = frames.shape
    pitch = h * w + gap
    host = np.zeros(n * pitch, frames.dtype)
    for i in range(n):
        host[i * pitch:i * pitch + h * w] = frames[i].ravel()
    src = hip.DeviceBuffer(host.nbytes).upload(host)
    dst = hip.DeviceBuffer(frames.nbytes)
    fa, nf = hip.fact_array(radial[2])
    ca, _ = hip.fact_array(coef)
    try:
        hip.check(hip.lib().dcp_remap_frames_typed(src.ptr, dst.ptr, DTYPE[frames.dtype.name], kind, n, h, w, pitch, w, radial[0], radial[1], fa, nf, ca,
                                                   order, hip.BLEND_BY_NAME[blend], hip.MEM_DEVICE, -1, None))
        return dst.download(frames.shape, frames.dtype)
    finally:
        src.free()
        dst.free()


@pytest.fixture(scope="module")
def stacks():
    """the float32 frames of tests 1, 2 and 4 (made once)"""
    return {shape: noise(71 + shape[1], (N,) + shape) for shape in ((481, 419), (480, 420))}


@pytest.mark.parametrize("shape", [(481, 419), (480, 420)], ids=["481x419", "480x420"])
@pytest.mark.parametrize("coef", ["mild", "cfg3"])
def test_float32_frames_in_one_launch_equal_the_oracle_and_the_single_calls(hip, orc, stacks, shape, coef):
    """Ragged tiles on both axes (481 x 419), 16 tile rows = the XCD tile-row order (480 x 420 gives 15 -> padded to 16), three depth
    chunks; through the C entry on a buffer with a gap between the frames, and through the Python functions on a tensor."""
    torch = pytest.importorskip("torch")
    from discorpy_amd.post import postprocessing as pp
    h, w = shape
    coef = MILD if coef == "mild" else cfg3_for(w)
    radial = centre(h, w) + (FACT5,)
    frames = stacks[shape]
    assert certificate(hip, MAP_PERSP, h, w, None, coef) >= 2 and certificate(hip, MAP_FUSED, h, w, radial, coef) >= 2
    t = torch.from_numpy(frames).cuda()
    with forced(hip):
        for blend in (None, "scipy", "f32"):
            name = {None: "f64lerp", "scipy": "scipy", "f32": "f32lerp"}[blend]
            ob = oblend(orc, blend or "f64lerp")
            got_c = frames_call(hip, frames, MAP_PERSP, (0.0, 0.0, []), coef, blend=blend or "f64lerp")
            assert hip.last_kernel().startswith("stack_wg_kernel<Persp,NF=0," + name), hip.last_kernel()
            got_p = pp.correct_perspective_images(t, coef, blend=blend)
            assert hip.last_kernel().startswith("stack_wg_kernel<Persp,NF=0," + name), hip.last_kernel()
            assert tuple(got_p.shape) == frames.shape and got_p.dtype == torch.float32
            got_p = got_p.cpu().numpy()
            for i in range(N):
                want = orc.correct_perspective_image(frames[i], coef, blend=ob)
                assert np.array_equal(got_c[i], want), ("persp, C entry", blend, i)
                assert np.array_equal(got_p[i], want), ("persp, Python", blend, i)
            got_c = frames_call(hip, frames, MAP_FUSED, radial, coef, blend=blend or "f64lerp")
            assert hip.last_kernel().startswith("stack_wg_kernel<Fused,NF=5," + name), hip.last_kernel()
            got_p = pp.unwarp_perspective_fused_images(t, *radial, coef, blend=blend)
            assert hip.last_kernel().startswith("stack_wg_kernel<Fused,NF=5," + name), hip.last_kernel()
            got_p = got_p.cpu().numpy()
            for i in range(N):
                want = orc.unwarp_fused(frames[i], *radial, coef, poly=orc.POLY_KERNEL, blend=ob)
                assert np.array_equal(got_c[i], want), ("fused, C entry", blend, i)
                assert np.array_equal(got_p[i], want), ("fused, Python", blend, i)
        # (outside the forced block the single calls below could not reach the stack kernel anyway: they hand over one frame)
    for blend in (None, "scipy", "f32"):
        got_p = pp.correct_perspective_images(t, coef, blend=blend)            # frame by frame now (a small launch): the same bits
        got_f = pp.unwarp_perspective_fused_images(t, *radial, coef, blend=blend)
        for i in (0, N - 1):
            assert np.array_equal(got_p[i].cpu().numpy(), pp.correct_perspective_image(t[i], coef, blend=blend).cpu().numpy()), (blend, i)
            assert np.array_equal(got_f[i].cpu().numpy(), pp.unwarp_perspective_fused(t[i], *radial, coef, blend=blend).cpu().numpy()), (blend, i)
    with forced(hip):
        for blend in (None, "scipy", "f32"):
            one = pp.correct_perspective_images(t, coef, blend=blend).cpu().numpy()
            assert hip.last_kernel().startswith("stack_wg_kernel<Persp,"), hip.last_kernel()
            two = pp.unwarp_perspective_fused_images(t, *radial, coef, blend=blend).cpu().numpy()
            assert hip.last_kernel().startswith("stack_wg_kernel<Fused,"), hip.last_kernel()
            for i in range(N):
                assert np.array_equal(one[i], pp.correct_perspective_image(t[i], coef, blend=blend).cpu().numpy()), (blend, i)
                assert np.array_equal(two[i], pp.unwarp_perspective_fused(t[i], *radial, coef, blend=blend).cpu().numpy()), (blend, i)


@pytest.mark.parametrize("shape", [(300, 420), (517, 1031)], ids=["300x420", "517x1031"])
def test_the_looped_polynomial_and_the_padded_one_under_both_centres(hip, orc, shape):
    """Seven radial terms loop over the coefficients in LDS (NF = -1), three are padded to the NF = 5 instantiation; a centre inside the
    frame and one far outside it.  The host's certificate (dcp_debug_tile_certificate, no device needed) holds level 2 for every
    combination at 300 x 420; at 517 x 1031 seven terms around the far centre lose it (level 0) under both homographies: that call
    must go frame by frame -- and give the oracle's bits all the same."""
    h, w = shape
    frames = noise(5, (N,) + shape)
    far = (-50.0, 900.0)
    with forced(hip):
        for coef in (MILD, cfg3_for(w)):
            for fact, nf in ((FACT7, "-1"), (FACT3, "5")):
                for xc, yc in (centre(h, w), far):
                    radial = (xc, yc, fact)
                    level = certificate(hip, MAP_FUSED, h, w, radial, coef)
                    assert level == (0 if (w == 1031 and fact is FACT7 and (xc, yc) == far) else 2), (coef, fact, xc, level)
                    got = frames_call(hip, frames, MAP_FUSED, radial, coef, blend="scipy")
                    if level >= 2:
                        assert hip.last_kernel().startswith("stack_wg_kernel<Fused,NF=%s,scipy" % nf), hip.last_kernel()
                    else:
                        assert not hip.last_kernel().startswith("stack_wg_kernel<"), hip.last_kernel()
                    for i in (0, 4, N - 1):
                        assert np.array_equal(got[i], orc.unwarp_fused(frames[i], *radial, coef, poly=orc.POLY_KERNEL, blend=orc.BLEND_SCIPY)), (fact, xc, i)


@pytest.mark.parametrize("dt, tag", [("uint16", "16-bit"), ("uint8", "8-bit")])
def test_uint16_and_uint8_frames_blend_and_store_as_scipy_does(hip, orc, dt, tag):
    from discorpy_amd.post import postprocessing as pp
    h, w = 480, 420
    frames = (noise(33, (N, h, w)) * 60000).astype(np.uint16) if dt == "uint16" else typed_image("uint8", (N, h, w), 34)
    dev = hip.DeviceArray(frames.shape, frames.dtype).copy_from_host(frames)
    radial = centre(h, w) + (FACT5,)
    results = []
    try:
        for exact in (1, 0):
            hip.set_option("x_int_exact", exact)
            with forced(hip):
                for coef in (MILD, cfg3_for(w)):
                    got = pp.correct_perspective_images(dev, coef)
                    assert hip.last_kernel() == "stack_wg_kernel<Persp,NF=0,scipy,%s>" % tag, hip.last_kernel()
                    assert isinstance(got, hip.DeviceArray) and got.shape == frames.shape and got.dtype == frames.dtype
                    got = got.copy_to_host()
                    results.append(got)
                    for i in range(N):
                        assert np.array_equal(got[i], orc.correct_perspective_image(frames[i], coef)), ("persp", exact, i)
                    got = frames_call(hip, frames, MAP_FUSED, radial, coef)
                    assert hip.last_kernel() == "stack_wg_kernel<Fused,NF=5,scipy,%s>" % tag, hip.last_kernel()
                    results.append(got)
            for k, coef in enumerate((MILD, cfg3_for(w))):
                for i in range(N):
                    assert np.array_equal(results[-3 + 2 * k][i], pp.unwarp_perspective_fused(frames[i], *radial, coef)), ("fused", exact, i)
    finally:
        hip.set_option("x_int_exact", 1)
    for a, b in zip(results[:4], results[4:]):
        assert np.array_equal(a, b)


def test_declined_calls_give_the_same_bits_and_say_so(hip, orc, stacks):
    torch = pytest.importorskip("torch")
    from discorpy_amd.post import postprocessing as pp
    h, w = 480, 420
    frames = stacks[(h, w)][:5]
    t = torch.from_numpy(frames).cuda()
    radial = centre(h, w) + (FACT3,)
    mild = MILD

    def declined():
        name = hip.last_kernel()
        assert not name.startswith(("stack_wg_kernel<Persp", "stack_wg_kernel<Fused")), name

    def same(got_p, got_f, mats, coef, **kw):
        for i in range(len(mats)):
            a, b = pp.correct_perspective_image(mats[i], coef, **kw), pp.unwarp_perspective_fused(mats[i], *radial, coef, **kw)
            for got, want in ((got_p[i], a), (got_f[i], b)):
                got = got.cpu().numpy() if hasattr(got, "cpu") else got
                want = want.cpu().numpy() if hasattr(want, "cpu") else want
                assert np.array_equal(got, want), (i, kw)

    def both(mats, coef, **kw):
        got_p = pp.correct_perspective_images(mats, coef, **kw)
        declined()
        got_f = pp.unwarp_perspective_fused_images(mats, *radial, coef, **kw)
        declined()
        same(got_p, got_f, mats, coef, **kw)
        return got_p, got_f

    assert certificate(hip, MAP_PERSP, h, w, None, STRONG) == 1 and certificate(hip, MAP_FUSED, h, w, radial, STRONG) == 0
    with forced(hip):
        both(t, STRONG)                                             # no level-2 certificate
        both(t, pole_inside(w))                                     # not tame
        both(t, mild, order=0)
        for dt in ("int32", "float64"):
            both(torch.from_numpy(typed_image(dt, (3, h, w), 8)).cuda(), mild)
        wide = torch.from_numpy(noise(9, (3, h, 2 * w))).cuda()
        both(wide[:, :, ::2], mild)                                 # column stride 2
        both(frames, mild)                                          # host memory (blend=None is scipy's there)
        got_p, got_f = both([t[i] for i in range(3)], mild)         # separate tensors
        assert isinstance(got_p, list) and isinstance(got_f, list) and len(got_p) == 3
        both(t[:2], mild, order=3)
        # the C entry itself on host memory and at order 0
        for kind, want in ((MAP_PERSP, pp.correct_perspective_image(frames[1], mild, blend="scipy")),
                           (MAP_FUSED, pp.unwarp_perspective_fused(frames[1], *radial, mild, blend="scipy"))):
            out = np.empty_like(frames)
            fa, nf = hip.fact_array(radial[2])
            ca, _ = hip.fact_array(mild)
            hip.check(hip.lib().dcp_remap_frames_typed(frames.ctypes.data, out.ctypes.data, 0, kind, len(frames), h, w, h * w, w, radial[0], radial[1],
                                                       fa, nf, ca, 1, hip.BLEND_SCIPY, hip.MEM_HOST, -1, None))
            declined()
            assert np.array_equal(out[1], want)
    both(t, mild)                                                   # x_stack_wg = 1: five small frames are too little work


def test_out_and_return_kinds(hip, orc):
    torch = pytest.importorskip("torch")
    from discorpy_amd.post import postprocessing as pp
    h, w = 300, 420
    frames = noise(12, (4, h, w))
    radial = centre(h, w) + (FACT3,)
    t = torch.from_numpy(frames).cuda()
    want_p = [orc.correct_perspective_image(f, MILD, blend=orc.BLEND_F64LERP) for f in frames]
    want_f = [orc.unwarp_fused(f, *radial, MILD, poly=orc.POLY_KERNEL, blend=orc.BLEND_F64LERP) for f in frames]
    with forced(hip):
        for fn, args, want in ((pp.correct_perspective_images, (MILD,), want_p), (pp.unwarp_perspective_fused_images, radial + (MILD,), want_f)):
            got = fn(t, *args)                                          # a tensor in, a tensor out
            assert torch.is_tensor(got) and got.is_cuda and tuple(got.shape) == frames.shape
            assert hip.last_kernel().startswith("stack_wg_kernel<"), hip.last_kernel()
            assert all(np.array_equal(got[i].cpu().numpy(), want[i]) for i in range(4))
            dev = hip.DeviceArray(frames.shape, np.float32).copy_from_host(frames)
            got = fn(dev, *args)                                        # a device array that is no tensor: ONE 3-D DeviceArray
            assert isinstance(got, hip.DeviceArray) and got.shape == frames.shape
            assert all(np.array_equal(got[i].copy_to_host(), want[i]) for i in range(4))
            got = fn([t[i] for i in range(4)], *args)                   # a sequence in, a list out
            assert isinstance(got, list) and len(got) == 4 and all(torch.is_tensor(g) for g in got)
            assert all(np.array_equal(got[i].cpu().numpy(), want[i]) for i in range(4))
            out = torch.full(frames.shape, -1.0, dtype=torch.float32, device="cuda")
            assert fn(t, *args, out=out) is out                         # out= filled and returned (one launch)
            assert hip.last_kernel().startswith("stack_wg_kernel<"), hip.last_kernel()
            assert all(np.array_equal(out[i].cpu().numpy(), want[i]) for i in range(4))
            outs = [torch.full((h, w), -1.0, dtype=torch.float32, device="cuda") for _ in range(4)]
            got = fn([t[i] for i in range(4)], *args, out=outs)         # a list of outputs: frame by frame, each filled
            assert all(g is o for g, o in zip(got, outs))
            assert all(np.array_equal(outs[i].cpu().numpy(), want[i]) for i in range(4))
            host_out = np.full(frames.shape, -1.0, np.float32)
            assert fn(frames, *args, blend="f64lerp", out=host_out) is host_out
            assert all(np.array_equal(host_out[i], want[i]) for i in range(4))
            with pytest.raises(ValueError):
                fn(t, *args, out=torch.empty((4, h, w + 1), dtype=torch.float32, device="cuda"))


def test_five_larger_frames_take_the_kernel_on_their_own(hip, orc):
    """2048 x 2304 under configs.cfg3 rescaled: 1152 tiles x 2 depth chunks -- the launcher takes the call at its default setting."""
    torch = pytest.importorskip("torch")
    from discorpy_amd.post import postprocessing as pp
    H, W, n = 2048, 2304, 5
    c2 = configs.cfg2()
    s = 4096.0 / W
    radial = (c2["xcenter"] / s, c2["ycenter"] / s, [v * s ** k for k, v in enumerate(c2["list_fact"])])
    coef = cfg3_for(W)
    frames = np.stack([noise(600 + i, (H, W)) for i in range(n)])
    t = torch.from_numpy(frames).cuda()
    assert hip.get_option("x_stack_wg") == 1
    got = pp.unwarp_perspective_fused_images(t, *radial, coef).cpu().numpy()
    assert hip.last_kernel().startswith("stack_wg_kernel<Fused,NF=5,f64lerp"), hip.last_kernel()
    for i in (0, 4):
        assert np.array_equal(got[i], orc.unwarp_fused(frames[i], *radial, coef, poly=orc.POLY_KERNEL, blend=orc.BLEND_F64LERP)), i
    got = pp.correct_perspective_images(t, coef).cpu().numpy()
    assert hip.last_kernel().startswith("stack_wg_kernel<Persp,NF=0,f64lerp"), hip.last_kernel()
    for i in (0, 4):
        assert np.array_equal(got[i], orc.correct_perspective_image(frames[i], coef, blend=orc.BLEND_F64LERP)), i
