#!/usr/bin/env python
"""A/B on one box: a device-resident 4096^2 interleaved colour image (util.unwarp_color_image_backward's kernel call) through
remap_wg_color_kernel, through the one-thread-per-pixel kernel (option wg_box=0), and as NC single-plane launches of
remap_wg_kernel on planar copies.  us per image, HIP events after 300 ms of the same launches; a ring of images larger than the
256 MB Infinity Cache.

--map perspective / fused: the interleaved image under the homography (dcp_perspective_color_image) or the one-pass perspective ->
radial map (dcp_unwarp_fused_color_image) against NC single-plane calls on planes that are already split and dense (the two
transposes a user of the single-plane functions also pays are not charged to them), the two ALTERNATING in one run: --rounds
rounds of --reps launches each, median and range per side, the core clock under the colour kernel.

--order N (2..5): the spline orders.  Side A is the one-call path of the three util functions (a prefilter per channel, one gather
launch: dcp_*_color_image_spline), side B the plane-by-plane route the same functions took before it -- the channels as dense planes
through post.unwarp_images_backward under the radial map, a loop of the single-plane function over mat[:, :, i] and a stack of the
planes under the other two.  The two alternate in one process, --rounds rounds (at least five) of --reps calls each, synchronised host
times per call; printed: the median and range of both sides, B's spread over its rounds, whether A is slower than B by more than
that spread, whether the two outputs are equal, and the core clock under side A.  Cases: a device-resident --size x --size x 3
float32 image under --map, and (--map radial) a host 3000 x 4000 x 3 uint8 NumPy image.

    python tools/time_color.py [--map radial|perspective|fused] [--size 4096] [--ring 6] [--reps 60] [--rounds 5] [--cases f32x3,f32x4,u8x3,u16x3]
    python tools/time_color.py --order 3 [--map radial|perspective|fused] [--size 4096] [--reps 5] [--rounds 5] [--no-host]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench  # noqa: E402
from discorpy_amd import _ffi as F  # noqa: E402
from discorpy_amd import configs  # noqa: E402


def ab_homography(a, L, dev):
    """--map perspective / fused: colour call against NC single-plane calls, alternating."""
    H = W = a.size
    s = a.size / 4096.0
    cfg = configs.cfg3()
    c = cfg["list_coef"]
    ca, _ = F.fact_array([c[0], c[1], c[2] * s, c[3], c[4], c[5] * s, c[6] / s, c[7] / s])     # (as tools/gen_golden.py rescales it)
    fa, nf = F.fact_array([v * s ** -i for i, v in enumerate(cfg["list_fact"])])
    xc, yc = cfg["xcenter"] * s, cfg["ycenter"] * s
    fused = a.map == "fused"
    dt = {"f32": ("float32", 0), "u8": ("uint8", 2), "u16": ("uint16", 4)}
    rng = np.random.default_rng(3)
    for case in a.cases.split(","):
        tname, nc = case.split("x")
        nc = int(nc)
        if tname not in dt or nc not in (3, 4):
            continue
        npdt, code = dt[tname]
        es = np.dtype(npdt).itemsize
        nbytes = H * W * nc * es
        ring = max(2, min(a.ring, int(3e9 // (4 * nbytes)) or 2))
        img = (rng.random((H, W, nc), dtype=np.float32) * (255 if tname != "f32" else 1)).astype(npdt)
        srcs = [F.DeviceBuffer(nbytes, dev).upload(img) for _ in range(ring)]
        dsts = [F.DeviceBuffer(nbytes, dev) for _ in range(ring)]
        planes = [F.DeviceBuffer(H * W * es, dev).upload(np.ascontiguousarray(img[:, :, k % nc])) for k in range(nc * ring)]
        outs = [F.DeviceBuffer(H * W * es, dev) for _ in range(nc * ring)]
        for name, order, blend in (("f64lerp", 1, F.BLEND_F64LERP), ("scipy", 1, F.BLEND_SCIPY), ("nearest", 0, F.BLEND_SCIPY)):
            if tname != "f32" and name == "f64lerp":
                continue

            def colour(i):
                sp, dp = srcs[i % ring].ptr, dsts[i % ring].ptr
                if fused:
                    F.check(L.dcp_unwarp_fused_color_image(sp, dp, code, H, W, nc, W * nc, nc, xc, yc, fa, nf, ca, order, blend, F.MEM_DEVICE, dev, None))
                else:
                    F.check(L.dcp_perspective_color_image(sp, dp, code, H, W, nc, W * nc, nc, ca, order, blend, F.MEM_DEVICE, dev, None))

            def planar(i):
                for k in range(nc):
                    j = (i % ring) * nc + k
                    sp, dp = planes[j].ptr, outs[j].ptr
                    if tname == "f32" and fused:
                        F.check(L.dcp_unwarp_fused_f32(sp, dp, H, W, W, 1, xc, yc, fa, nf, ca, order, blend, F.MEM_DEVICE, dev, None))
                    elif tname == "f32":
                        F.check(L.dcp_perspective_image_f32(sp, dp, H, W, W, 1, ca, order, blend, F.MEM_DEVICE, dev, None))
                    elif fused:
                        F.check(L.dcp_unwarp_fused_typed(sp, dp, code, H, W, W, 1, xc, yc, fa, nf, ca, order, 0, F.MEM_DEVICE, dev, None))
                    else:
                        F.check(L.dcp_perspective_image_typed(sp, dp, code, H, W, W, 1, ca, order, 0, F.MEM_DEVICE, dev, None))

            tc, tp = [], []
            for r in range(a.rounds):
                tc.append(bench.timed_launches(colour, a.reps, dev, settle_ms=300.0 if r == 0 else 60.0))
                kc = F.last_kernel()
                tp.append(bench.timed_launches(planar, a.reps, dev, settle_ms=60.0))
                kp = F.last_kernel()
            mc, mp = float(np.median(tc)), float(np.median(tp))
            print("%-11s %-6s %-8s colour %8.2f us [%.2f .. %.2f]  %.3f of 8 TB/s (%d B/px)  %s" % (
                a.map, case, name, mc, min(tc), max(tc), 2 * nbytes / (mc * 1e-6) / 8e12, 2 * nc * es, kc), flush=True)
            print("%-11s %-6s %-8s %d planes %7.2f us [%.2f .. %.2f]  colour / planes = %.3f  %s" % (
                a.map, case, name, nc, mp, min(tp), max(tp), mc / mp, kp), flush=True)
            if name != "nearest" and not a.no_generic:
                F.set_option("x_wg_box", 0)
                tg = bench.timed_launches(colour, max(4, a.reps // 4), dev, settle_ms=100.0)
                F.set_option("x_wg_box", 1)
                print("%-11s %-6s %-8s one thread per pixel: %.2f us" % (a.map, case, name, tg), flush=True)
            if name in ("f64lerp", "scipy") and (tname == "f32") == (name == "f64lerp"):
                clk = bench.clocks_under_load(lambda: colour(0), lambda: F.check(L.dcp_stream_synchronize(dev, None)))
                print("%-11s %-6s clock under the colour kernel: %s" % (a.map, case, clk), flush=True)
        for b in srcs + dsts + planes + outs:
            b.free()


def ab_spline(a):
    """--order 2..5: the one-call path (A) against the plane-by-plane route (B), alternating."""
    import time
    import torch
    from discorpy_amd.post import postprocessing as pp
    from discorpy_amd.util import utility as util
    order, rounds = a.order, max(5, a.rounds)

    def sync():
        torch.cuda.synchronize()

    def per_call(fn, reps):
        sync()
        t0 = time.perf_counter()
        for _ in range(reps):
            out = fn()
        sync()
        return (time.perf_counter() - t0) / reps * 1e3, out

    def alternate(tag, side_a, side_b, reps):
        per_call(side_a, 1)
        per_call(side_b, 1)                      # first use: workspace planes, output pool, clock ramp
        ta, tb = [], []
        for r in range(rounds):
            t, out_a = per_call(side_a, reps)
            ka = F.last_kernel()
            ta.append(t)
            t, out_b = per_call(side_b, reps)
            kb = F.last_kernel()
            tb.append(t)
        same = bool(torch.equal(out_a, out_b)) if torch.is_tensor(out_a) else bool(np.array_equal(out_a, np.asarray(out_b)))
        ma, mb, spread = float(np.median(ta)), float(np.median(tb)), max(tb) - min(tb)
        print("%s order %d  A one call      %9.3f ms [%.3f .. %.3f]  %s" % (tag, order, ma, min(ta), max(ta), ka), flush=True)
        print("%s order %d  B plane by plane %8.3f ms [%.3f .. %.3f]  spread %.3f ms  %s" % (tag, order, mb, min(tb), max(tb), spread, kb), flush=True)
        print("%s order %d  A / B = %.3f   A - B = %+.3f ms against B's spread of %.3f ms: %s   outputs equal: %s" % (
            tag, order, ma / mb, ma - mb, spread, "within the bar" if ma - mb <= spread else "MISSES the bar", same), flush=True)

    size = a.size
    s = size / 4096.0
    if a.map == "radial":
        cfg = configs.cfg2()
        xc, yc, fact = cfg["xcenter"] * s, cfg["ycenter"] * s, [c * s ** -i for i, c in enumerate(cfg["list_fact"])]
        coef = None
    else:
        cfg = configs.cfg3()
        c = cfg["list_coef"]
        coef = [c[0], c[1], c[2] * s, c[3], c[4], c[5] * s, c[6] / s, c[7] / s]
        xc, yc, fact = cfg["xcenter"] * s, cfg["ycenter"] * s, [v * s ** -i for i, v in enumerate(cfg["list_fact"])]
    rng = np.random.default_rng(3)
    dev_img = torch.from_numpy(rng.random((size, size, 3), dtype=np.float32)).cuda()
    for blend in (None, "scipy"):
        if a.map == "radial":
            def side_a():
                return util.unwarp_color_image_backward(dev_img, xc, yc, fact, order=order, blend=blend)

            def side_b():
                planes = dev_img.permute(2, 0, 1).contiguous()
                return pp.unwarp_images_backward(planes, xc, yc, fact, order=order, blend=blend).permute(1, 2, 0)
        elif a.map == "perspective":
            def side_a():
                return util.correct_perspective_color_image(dev_img, coef, order=order, blend=blend)

            def side_b():
                return torch.stack([pp.correct_perspective_image(dev_img[:, :, i], coef, order=order, blend=blend) for i in range(3)], dim=2)
        else:
            def side_a():
                return util.unwarp_perspective_fused_color_image(dev_img, xc, yc, fact, coef, order=order, blend=blend)

            def side_b():
                return torch.stack([pp.unwarp_perspective_fused(dev_img[:, :, i], xc, yc, fact, coef, order=order, blend=blend)
                                    for i in range(3)], dim=2)
        alternate("device %dx%dx3 f32 %-11s blend=%-5s" % (size, size, a.map, blend), side_a, side_b, a.reps)
    clk = bench.clocks_under_load(side_a, sync)
    print("clock under side A: %s" % (clk,), flush=True)
    del dev_img
    if a.map == "radial" and not a.no_host:
        h, w = 3000, 4000                       # the reference's GoPro photograph (examples/readthedocs_demo/demo_07.py)
        sh = w / 4096.0
        cfg = configs.cfg2()
        hxc, hyc, hfact = cfg["xcenter"] * sh, 0.5 * h, [c * sh ** -i for i, c in enumerate(cfg["list_fact"])]
        photo = rng.integers(0, 255, (h, w, 3), endpoint=True).astype(np.uint8)

        def host_a():
            return util.unwarp_color_image_backward(photo, hxc, hyc, hfact, order=order)

        def host_b():
            planes = np.ascontiguousarray(np.moveaxis(photo, 2, 0))
            return np.moveaxis(np.asarray(pp.unwarp_images_backward(planes, hxc, hyc, hfact, order=order)), 0, 2)
        alternate("host %dx%dx3 u8 radial" % (h, w), host_a, host_b, max(1, a.reps // 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--order", type=int, default=1, choices=(1, 2, 3, 4, 5),
                    help="2..5: the one-call spline path against the plane-by-plane route (see the module docstring)")
    ap.add_argument("--no-host", action="store_true", help="--order 2..5: skip the host 3000 x 4000 x 3 uint8 case")
    ap.add_argument("--map", choices=("radial", "perspective", "fused"), default="radial")
    ap.add_argument("--rounds", type=int, default=5, help="--map perspective / fused: alternations of the two sides")
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--ring", type=int, default=6)
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--cases", default="f32x3,f32x4,u8x3,u16x3,f64x1,i32x1")
    ap.add_argument("--no-generic", action="store_true")
    a = ap.parse_args()
    L = F.lib()
    F.require_device()
    dev = -1
    if a.order >= 2:
        return ab_spline(a)
    if a.map != "radial":
        return ab_homography(a, L, dev)
    cfg = configs.cfg2()
    s = a.size / 4096.0
    fact = [c * s ** -i for i, c in enumerate(cfg["list_fact"])]
    xc, yc = cfg["xcenter"] * s, cfg["ycenter"] * s
    fa, nf = F.fact_array(fact)
    H = W = a.size
    dt = {"f32": ("float32", 0), "u8": ("uint8", 2), "u16": ("uint16", 4), "f64": ("float64", 1), "i32": ("int32", 7)}
    rng = np.random.default_rng(3)
    for case in a.cases.split(","):
        tname, nc = case.split("x")
        nc = int(nc)
        npdt, code = dt[tname]
        es = np.dtype(npdt).itemsize
        nbytes = H * W * nc * es
        ring = max(2, min(a.ring, int(3e9 // (2 * nbytes)) or 2))
        img = (rng.random((H, W, nc), dtype=np.float32) * (255 if tname not in ("f32", "f64") else 1)).astype(npdt)
        srcs = [F.DeviceBuffer(nbytes, dev).upload(img) for _ in range(ring)]
        dsts = [F.DeviceBuffer(nbytes, dev) for _ in range(ring)]
        for name, order, blend in (("f64lerp", 1, F.BLEND_F64LERP), ("scipy", 1, F.BLEND_SCIPY), ("nearest", 0, F.BLEND_SCIPY)):
            if tname != "f32" and name == "f64lerp":
                continue

            if nc == 1:        # single planes go through the typed image entry point
                def run(i):
                    F.check(L.dcp_unwarp_image_typed(srcs[i % ring].ptr, dsts[i % ring].ptr, code, H, W, W, 1, xc, yc, fa, nf, order, 0, F.MEM_DEVICE, dev, None))
                t = bench.timed_launches(run, a.reps, dev, settle_ms=300.0)
                k = F.last_kernel()
                F.set_option("x_wg_box", 0)
                tg = bench.timed_launches(run, max(4, a.reps // 4), dev, settle_ms=100.0)
                F.set_option("x_wg_box", 1)
                print("%-6s %-8s %8.2f us  %.3f of 8 TB/s (%d B/px)  %s   | one thread per pixel: %.2f us" % (
                    case, name, t, 2 * nbytes / (t * 1e-6) / 8e12, 2 * es, k, tg), flush=True)
                continue

            def run(i):
                F.check(L.dcp_unwarp_color_image(srcs[i % ring].ptr, dsts[i % ring].ptr, code, H, W, nc, W * nc, nc, xc, yc, fa, nf, order, blend,
                                                 F.MEM_DEVICE, dev, None))
            t = bench.timed_launches(run, a.reps, dev, settle_ms=300.0)
            k = F.last_kernel()
            line = "%-6s %-8s %8.2f us  %.3f of 8 TB/s (%d B/px)  %s" % (case, name, t, 2 * nbytes / (t * 1e-6) / 8e12, 2 * nc * es, k)
            if not a.no_generic:
                F.set_option("x_wg_box", 0)
                tg = bench.timed_launches(run, max(4, a.reps // 4), dev, settle_ms=100.0)
                F.set_option("x_wg_box", 1)
                line += "   | one thread per pixel: %.2f us" % tg
            print(line, flush=True)
        if tname == "f32":
            # the same bytes as NC planar single-plane launches (what three K1 calls cost)
            planes = [F.DeviceBuffer(H * W * 4, dev).upload(np.ascontiguousarray(img[:, :, c % nc])) for c in range(nc * ring)]
            outs = [F.DeviceBuffer(H * W * 4, dev) for _ in range(nc * ring)]

            def k1(i):
                for c in range(nc):
                    j = (i % ring) * nc + c
                    F.check(L.dcp_unwarp_image_f32(planes[j].ptr, outs[j].ptr, H, W, W, 1, xc, yc, fa, nf, 1, 1, F.BLEND_F64LERP, F.MEM_DEVICE, dev, None))
            t = bench.timed_launches(k1, a.reps, dev, settle_ms=300.0)
            print("%-6s %d planar launches of %s: %.2f us" % (case, nc, F.last_kernel(), t), flush=True)
            for b in planes + outs:
                b.free()
        for b in srcs + dsts:
            b.free()


if __name__ == "__main__":
    main()
