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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--map", choices=("radial", "perspective", "fused"), default="radial")
    ap.add_argument("--batch", type=int, default=24)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5, help="--map perspective | fused: alternations of the two sides")
    ap.add_argument("--option", action="append", default=[])
    ap.add_argument("--samplers", default="f64lerp,scipy,f32lerp,nearest")
    a = ap.parse_args()
    L = F.lib()
    F.require_device()
    for kv in a.option:
        k, v = kv.split("=")
        F.set_option(k, int(v))
    dev = -1
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
