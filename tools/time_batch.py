#!/usr/bin/env python
"""A/B on one box: BASELINE config 2 frames through (a) one dcp_unwarp_image_f32 launch per frame, (b) ONE dcp_unwarp_images_f32
call for the ring (remap_wg_batch_kernel, every frame its own calibration), (c) the stack entry point (same calibration), for
every sampler.  us per 4096^2 frame, HIP events on the launch stream after 300 ms of the same launches.

    python tools/time_batch.py [--batch 24] [--reps 40] [--option key=value ...]

--map perspective | fused: BASELINE config 3's homography (fused: with config 2's radial model) over a ring of --batch frames through
(a) one dcp_perspective_image_f32 / dcp_unwarp_fused_f32 call per frame, (b) ONE dcp_remap_frames_typed call for the ring
(stack_wg_kernel<Persp / Fused>), alternated --rounds times on one box: median and range of us per frame per side, the fraction of
8 B per pixel at 8 TB/s, the kernel names, whether (b) is faster by more than the spread of (a), and the clock under (b).

    python tools/time_batch.py --map fused [--batch 24] [--reps 10] [--rounds 5] [--samplers f64lerp,scipy,f32lerp]

--order 2..5 (with any --map): a stack of --batch device-resident frames of one calibration (config 2's radial model, config 3's
homography, or both) at a spline order through (a) the frame-by-frame route -- one single-frame spline call per frame, what
post.unwarp_images_backward / correct_perspective_images / unwarp_perspective_fused_images did before -- and (b) ONE
dcp_remap_frames_spline call, alternated --rounds times (at least five) in one process: us per frame (median and range) per side, the
route's round-to-round spread, whether the outputs of both sides are equal, the kernel names and the box clock under (b).  --groups
2,4,8,16 times (b) under each of these values of the lab option x_spline_frames as well (the choice of its default).

    python tools/time_batch.py --order 3 --map radial --batch 16 --reps 2 [--dtype float32|uint16] [--sum default|scipy] [--groups 2,4,8,16]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench  # noqa: E402
from discorpy_amd import _ffi as F  # noqa: E402
from discorpy_amd import configs  # noqa: E402


def frames_under_map(a, L, dev):
    """--map perspective | fused: one single-frame call per frame against one dcp_remap_frames_typed call for the ring"""
    cfg = configs.cfg3()
    H, W = cfg["shape"]
    n = a.batch
    fused = a.map == "fused"
    kind = F.MAP_FUSED if fused else F.MAP_PERSPECTIVE
    xc, yc = cfg["xcenter"], cfg["ycenter"]
    fa, nf = F.fact_array(cfg["list_fact"])
    ca, _ = F.fact_array(cfg["list_coef"])
    rng = np.random.default_rng(1)
    frame = H * W * 4
    src, dst = F.DeviceBuffer(n * frame, dev), F.DeviceBuffer(n * frame, dev)
    for i in range(n):
        img = rng.random((H, W), dtype=np.float32)
        F.check(L.dcp_memcpy(src.ptr + i * frame, img.ctypes.data, frame, F.COPY_H2D, dev, None))
    for name in a.samplers.split(","):
        if name == "nearest":
            continue                    # (order 0 has no one-launch kernel under these maps)
        blend = bench.BLEND_NAMES[name]

        def per_frame(i):
            sp, dp = src.ptr + (i % n) * frame, dst.ptr + (i % n) * frame
            if fused:
                F.check(L.dcp_unwarp_fused_f32(sp, dp, H, W, W, 1, xc, yc, fa, nf, ca, 1, blend, F.MEM_DEVICE, dev, None))
            else:
                F.check(L.dcp_perspective_image_f32(sp, dp, H, W, W, 1, ca, 1, blend, F.MEM_DEVICE, dev, None))

        def ring(_i):
            F.check(L.dcp_remap_frames_typed(src.ptr, dst.ptr, F.DTYPE_F32, kind, n, H, W, H * W, W, xc, yc, fa, nf, ca, 1, blend, F.MEM_DEVICE,
                                             dev, None))
        ta, tb = [], []
        for r in range(a.rounds):
            ta.append(bench.timed_launches(per_frame, a.reps * n, dev, settle_ms=300.0 if r == 0 else 60.0))
            ka = F.last_kernel()
            tb.append(bench.timed_launches(ring, a.reps, dev, settle_ms=60.0) / n)
            kb = F.last_kernel()
        ma, mb = float(np.median(ta)), float(np.median(tb))
        spread = max(ta) - min(ta)
        frac = lambda us: H * W * configs.BYTES_PER_PIXEL / (us * 1e-6) / (configs.HBM_PEAK_GBPS * 1e9)      # noqa: E731
        print("%-11s %-8s (a) per frame  %7.2f us [%.2f .. %.2f]  %.3f of 8 TB/s  %s" % (a.map, name, ma, min(ta), max(ta), frac(ma), ka), flush=True)
        print("%-11s %-8s (b) one call   %7.2f us [%.2f .. %.2f]  %.3f of 8 TB/s  %s" % (a.map, name, mb, min(tb), max(tb), frac(mb), kb), flush=True)
        print("%-11s %-8s (b) / (a) = %.3f; (a) - (b) = %.2f us per frame against a spread of (a) of %.2f us over %d rounds: %s" % (
            a.map, name, mb / ma, ma - mb, spread, a.rounds, "faster" if ma - mb > spread else "NOT faster by more than the spread"), flush=True)
        if name == "f64lerp":
            clk = bench.clocks_under_load(lambda: ring(0), lambda: F.check(L.dcp_stream_synchronize(dev, None)))
            print("%-11s clock under (b): %s" % (a.map, clk), flush=True)
    src.free()
    dst.free()


def frames_spline(a, L, dev):
    """--order 2..5: the frame-by-frame route of single-frame spline calls against one dcp_remap_frames_spline call for the stack"""
    radial = a.map == "radial"
    cfg = configs.cfg2() if radial else configs.cfg3()
    H, W = cfg["shape"]
    n, order = a.batch, a.order
    kind = {"radial": F.MAP_RADIAL, "perspective": F.MAP_PERSPECTIVE, "fused": F.MAP_FUSED}[a.map]
    xc, yc = cfg["xcenter"], cfg["ycenter"]
    fa, nf = F.fact_array(cfg["list_fact"])
    ca, _ = F.fact_array(cfg["list_coef"]) if not radial else (None, 0)
    dt = np.dtype(a.dtype)
    code = F.DTYPE_BY_NAME[dt.name]
    f32 = dt == np.float32
    mode = 0x100 if a.sum == "scipy" else 0                # "reflect", optionally DCP_SPLINE_SCIPY_SUM
    rng = np.random.default_rng(1)
    frame = H * W * dt.itemsize
    src, dst_a, dst_b = F.DeviceBuffer(n * frame, dev), F.DeviceBuffer(n * frame, dev), F.DeviceBuffer(n * frame, dev)
    for i in range(n):
        img = rng.random((H, W), dtype=np.float32) if f32 else rng.integers(0, 65535, (H, W), endpoint=True).astype(dt)
        F.check(L.dcp_memcpy(src.ptr + i * frame, img.ctypes.data, frame, F.COPY_H2D, dev, None))

    def per_frame(i):
        sp, dp = src.ptr + (i % n) * frame, dst_a.ptr + (i % n) * frame
        if radial:
            F.check(L.dcp_unwarp_image_spline_f32(sp, dp, H, W, W, 1, xc, yc, fa, nf, order, mode, F.MEM_DEVICE, dev, None) if f32 else
                    L.dcp_unwarp_image_typed(sp, dp, code, H, W, W, 1, xc, yc, fa, nf, order, mode, F.MEM_DEVICE, dev, None))
        elif kind == F.MAP_PERSPECTIVE:
            F.check(L.dcp_perspective_image_spline_f32(sp, dp, H, W, W, 1, ca, order, mode, F.MEM_DEVICE, dev, None) if f32 else
                    L.dcp_perspective_image_typed(sp, dp, code, H, W, W, 1, ca, order, mode, F.MEM_DEVICE, dev, None))
        else:
            F.check(L.dcp_unwarp_fused_spline_f32(sp, dp, H, W, W, 1, xc, yc, fa, nf, ca, order, mode, F.MEM_DEVICE, dev, None) if f32 else
                    L.dcp_unwarp_fused_typed(sp, dp, code, H, W, W, 1, xc, yc, fa, nf, ca, order, mode, F.MEM_DEVICE, dev, None))

    def one_call(_i):
        F.check(L.dcp_remap_frames_spline(src.ptr, dst_b.ptr, code, kind, n, H, W, H * W, W, xc, yc, fa, nf, ca, order, mode, F.MEM_DEVICE, dev,
                                          None))
    default = F.get_option("x_spline_frames")
    caps = [default] + [int(v) for v in a.groups.split(",") if v and int(v) != default]
    rounds = max(a.rounds, 5)
    ta, tb, kb = [], {c: [] for c in caps}, {}
    try:
        for r in range(rounds):
            ta.append(bench.timed_launches(per_frame, a.reps * n, dev, settle_ms=300.0 if r == 0 else 60.0))
            ka = F.last_kernel()
            for c in caps:
                F.set_option("x_spline_frames", c)
                tb[c].append(bench.timed_launches(one_call, a.reps, dev, settle_ms=60.0) / n)
                kb[c] = F.last_kernel()
        F.set_option("x_spline_frames", default)
        # the outputs of both sides, frame by frame
        for i in range(n):
            per_frame(i)
        one_call(0)
        F.check(L.dcp_stream_synchronize(dev, None))
        ha, hb = np.empty((H, W), dt), np.empty((H, W), dt)
        differing = 0
        for i in range(n):
            F.check(L.dcp_memcpy(ha.ctypes.data, dst_a.ptr + i * frame, frame, F.COPY_D2H, dev, None))
            F.check(L.dcp_memcpy(hb.ctypes.data, dst_b.ptr + i * frame, frame, F.COPY_D2H, dev, None))
            differing += int(np.count_nonzero(ha.view(np.uint8) != hb.view(np.uint8)))
        tag = "%-11s order %d %-7s %-7s" % (a.map, order, dt.name, a.sum)
        ma, spread = float(np.median(ta)), max(ta) - min(ta)
        print("%s (a) frame by frame       %8.2f us per frame [%.2f .. %.2f], spread %.2f us over %d rounds  %s" % (tag, ma, min(ta), max(ta), spread,
                                                                                                              rounds, ka), flush=True)
        for c in caps:
            mb = float(np.median(tb[c]))
            verdict = "within the bar" if mb - ma <= spread else "SLOWER than the route by more than its spread"
            print("%s (b) one call, groups of %2d%s %8.2f us per frame [%.2f .. %.2f]  (b) / (a) = %.3f: %s  %s" % (
                tag, c, " (default)" if c == default else "          ", mb, min(tb[c]), max(tb[c]), mb / ma, verdict, kb[c]), flush=True)
        print("%s outputs of (a) and (b): %s" % (tag, "equal" if differing == 0 else "%d bytes DIFFER" % differing), flush=True)
        clk = bench.clocks_under_load(lambda: one_call(0), lambda: F.check(L.dcp_stream_synchronize(dev, None)))
        print("%s clock under (b): %s" % (tag, clk), flush=True)
    finally:
        F.set_option("x_spline_frames", default)
        src.free()
        dst_a.free()
        dst_b.free()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--map", choices=("radial", "perspective", "fused"), default="radial")
    ap.add_argument("--batch", type=int, default=24)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5, help="--map perspective | fused: alternations of the two sides")
    ap.add_argument("--order", type=int, choices=(2, 3, 4, 5), default=None,
                    help="a spline order: the frame-by-frame route against one dcp_remap_frames_spline call (any --map)")
    ap.add_argument("--dtype", choices=("float32", "uint16"), default="float32", help="--order: element type of the frames")
    ap.add_argument("--sum", choices=("default", "scipy"), default="default", help="--order: the factorised tap sum or scipy's order")
    ap.add_argument("--groups", default="", help="--order: values of x_spline_frames to time (b) under, beside the default (e.g. 2,4,8,16)")
    ap.add_argument("--option", action="append", default=[])
    ap.add_argument("--samplers", default="f64lerp,scipy,f32lerp,nearest")
    a = ap.parse_args()
    L = F.lib()
    F.require_device()
    for kv in a.option:
        k, v = kv.split("=")
        F.set_option(k, int(v))
    dev = -1
    if a.order is not None:
        return frames_spline(a, L, dev)
    if a.map != "radial":
        return frames_under_map(a, L, dev)
    cfg = configs.cfg2()
    H, W = cfg["shape"]
    n = a.batch
    rng = np.random.default_rng(1)
    srcs = [F.DeviceBuffer(H * W * 4, dev).upload(rng.random((H, W), dtype=np.float32)) for _ in range(n)]
    dsts = [F.DeviceBuffer(H * W * 4, dev) for _ in range(n)]
    cals = bench.distinct_calibrations(cfg, n)
    nf = len(cfg["list_fact"])
    table = np.ascontiguousarray([c[2] for c in cals], dtype=np.float64)
    sp = (C.c_void_p * n)(*[b.ptr for b in srcs])
    dp = (C.c_void_p * n)(*[b.ptr for b in dsts])
    xa, ya = (C.c_double * n)(*[c[0] for c in cals]), (C.c_double * n)(*[c[1] for c in cals])
    tp = table.ctypes.data_as(C.POINTER(C.c_double))
    fa, _ = F.fact_array(cfg["list_fact"])
    for name in a.samplers.split(","):
        order = 0 if name == "nearest" else 1
        blend = F.BLEND_SCIPY if name == "nearest" else bench.BLEND_NAMES[name]

        def per_frame(i):
            F.check(L.dcp_unwarp_image_f32(srcs[i % n].ptr, dsts[i % n].ptr, H, W, W, 1, cfg["xcenter"], cfg["ycenter"], fa, nf, order, 1, blend,
                                           F.MEM_DEVICE, dev, None))

        def batch(_i):
            F.check(L.dcp_unwarp_images_f32(sp, dp, n, H, W, W, 1, xa, ya, tp, nf, order, 1, blend, F.MEM_DEVICE, dev, None))
        t1 = bench.timed_launches(per_frame, a.reps * n, dev, settle_ms=300.0)
        k1 = F.last_kernel()
        t2 = bench.timed_launches(batch, a.reps, dev, settle_ms=300.0) / n
        k2 = F.last_kernel()
        t1b = bench.timed_launches(per_frame, a.reps * n, dev, settle_ms=300.0)
        print("%-8s per-launch %.2f / %.2f us (%s)   batched %.2f us per frame (%s)" % (name, t1, t1b, k1, t2, k2), flush=True)


if __name__ == "__main__":
    main()
