#!/usr/bin/env python
"""Time the Gaussian filter (prep.linepattern.gaussian_filter's call, dcp_correlate_sym_2d) on device-resident images: the fused kernel
(gauss_lds_kernel: both passes in one launch, the planes in LDS; x_gauss_lds = 2, wherever the planes fit) against the per-axis route
(one gauss_axis_kernel launch per axis, x_gauss_lds = 0), alternated in one process, and scipy.ndimage.gaussian_filter on the same box.  Images of 2048^2 and 4096^2, float32
and uint16, sigma 3 (the reference's denoise step and chessboard default) and sigma 10, mode "nearest".

Per case: warm-up calls of both routes, then `--rounds` (at least five) rounds; a round times `--reps` back-to-back calls of the
fused route between HIP events, then the same of the per-axis route.  Printed in ms per call: the median round of each route, the
per-axis route's round-to-round spread (max - min), the difference fused - per-axis and whether it is within that spread (the bar
for making the fused kernel the default, kGaussFusedMaxRadius and kGaussFusedMaxLds of csrc/dcp_internal.h: it is not slower than the
per-axis route by more than that route's own spread), whether the two outputs are equal, and the kernels that ran.  scipy is timed at the `--scipy-side` (2048) only, once per
case, and there the line also carries the ratio scipy / GPU and whether scipy's output equals the GPU's.  The last line is the core
clock and package power under the 4096^2 float32 sigma-3 call.

    python tools/time_gaussian.py [--sides 2048,4096] [--dtypes float32,uint16] [--sigmas 3,10] [--rounds 5] [--reps 10] [--no-scipy]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

MODE_NEAREST = 4        # DCP_MODE_NEAREST


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sides", default="2048,4096")
    ap.add_argument("--dtypes", default="float32,uint16")
    ap.add_argument("--sigmas", default="3,10")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scipy-side", type=int, default=2048, help="the side at which scipy is timed and compared (0 or --no-scipy: never)")
    ap.add_argument("--no-scipy", action="store_true")
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("--rounds must be at least 5")
    import bench
    from discorpy_amd import _ffi as F
    from discorpy_amd.prep.linepattern import _gaussian_weights
    L = F.lib()
    F.require_device()
    dev = -1
    rng = np.random.default_rng(7)
    dptr = F.C.POINTER(F.C.c_double)
    clock_call = None
    for side in [int(s) for s in a.sides.split(",")]:
        for name in a.dtypes.split(","):
            dt = np.dtype(name)
            code = F.DTYPE_BY_NAME[dt.name]
            # a line-pattern-like image: a smooth illumination gradient under noise
            img = ((rng.random((side, side), dtype=np.float32) + np.linspace(0.5, 1.5, side, dtype=np.float32)) * 100.0).astype(dt)
            src = F.DeviceBuffer(img.nbytes, dev).upload(img)
            dst = {1: F.DeviceBuffer(img.nbytes, dev), 0: F.DeviceBuffer(img.nbytes, dev)}
            for sigma in [float(s) for s in a.sigmas.split(",")]:
                w = _gaussian_weights(sigma)
                wp, r = w.ctypes.data_as(dptr), len(w) // 2

                def run(lds):
                    F.check(L.dcp_correlate_sym_2d(src.ptr, dst[lds].ptr, side, side, side, code, wp, r, wp, r, MODE_NEAREST, 0.0, F.MEM_DEVICE, dev, None))

                def timed(lds):
                    F.set_option("x_gauss_lds", 2 * lds)
                    e0, e1 = F.Event(dev), F.Event(dev)
                    e0.record()
                    for _r in range(a.reps):
                        run(lds)
                    e1.record()
                    e1.synchronize()
                    return e0.elapsed_ms(e1) / a.reps
                names = {}
                for lds in (1, 0):
                    F.set_option("x_gauss_lds", 2 * lds)
                    for _ in range(a.warmup):
                        run(lds)
                    names[lds] = F.last_kernel()
                F.check(L.dcp_stream_synchronize(dev, None))
                rounds = {1: [], 0: []}
                for _ in range(a.rounds):
                    for lds in (1, 0):
                        rounds[lds].append(timed(lds))
                F.set_option("x_gauss_lds", 1)
                fused, axis = float(np.median(rounds[1])), float(np.median(rounds[0]))
                spread = max(rounds[0]) - min(rounds[0])
                out1, out0 = dst[1].download(img.shape, dt), dst[0].download(img.shape, dt)
                line = ("%-8s %4d x %-4d sigma %-4g r %-3d fused %8.4f ms (rounds %.4f .. %.4f)  per-axis %8.4f ms (rounds %.4f .. %.4f, spread %.4f)"
                        "  fused - per-axis %+.4f ms: %s  routes equal: %s" % (
                            dt.name, side, side, sigma, r, fused, min(rounds[1]), max(rounds[1]), axis, min(rounds[0]), max(rounds[0]), spread,
                            fused - axis, "within the bar" if fused - axis <= spread else "MISSES the bar", np.array_equal(out1, out0)))
                if not a.no_scipy and side == a.scipy_side:
                    from scipy import ndimage as ndi
                    t0 = time.perf_counter()
                    ref = ndi.gaussian_filter(img, sigma, mode="nearest")
                    cpu_ms = (time.perf_counter() - t0) * 1e3
                    line += "  scipy %9.1f ms  ratio %8.1f  equal to scipy: %s" % (cpu_ms, cpu_ms / fused, np.array_equal(out1, ref))
                print(line + "  [%s | %s]" % (names[1], names[0]), flush=True)
                if side >= 4096 and dt == np.float32 and sigma == 3.0:
                    clock_call = (src, dst[1], side, code, w, r)
            if clock_call is None or clock_call[0] is not src:
                src.free()
            for lds in (1, 0):
                if clock_call is None or clock_call[1] is not dst[lds]:
                    dst[lds].free()
    if clock_call:
        src, out, side, code, w, r = clock_call
        wp = w.ctypes.data_as(dptr)
        clk = bench.clocks_under_load(lambda: F.check(L.dcp_correlate_sym_2d(src.ptr, out.ptr, side, side, side, code, wp, r, wp, r, MODE_NEAREST, 0.0,
                                                                             F.MEM_DEVICE, dev, None)),
                                      lambda: F.check(L.dcp_stream_synchronize(dev, None)))
        print("clock under the %d x %d float32 sigma-3 call: %s" % (side, side, clk), flush=True)


if __name__ == "__main__":
    main()
