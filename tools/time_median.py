#!/usr/bin/env python
"""Time the median filter (prep.median_filter's call, dcp_median_filter_2d) on a device-resident image against
scipy.ndimage.median_filter on the same box: images of 512^2 and 2048^2, windows of 51 (prep.normalization's default) and (2, 2)
(binarization's denoise step), float32, uint16 and uint8.

Per case: warm-up calls, then `--rounds` (at least five) rounds of `--reps` back-to-back calls between HIP events; the median round
and the spread of the rounds are printed in ms per call, with the kernel that ran.  scipy is timed at 512^2 only, once per case (a
2048^2 image at size 51 takes it minutes), and there the line also carries the ratio scipy / GPU and whether the two outputs are
equal.  The last line is the core clock and package power under the 2048^2 / 51 float32 call.

    python tools/time_median.py [--sides 512,2048] [--dtypes float32,uint16,uint8] [--rounds 5] [--reps 2] [--no-scipy]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

SIZES = ((51, 51), (2, 2))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sides", default="512,2048")
    ap.add_argument("--dtypes", default="float32,uint16,uint8")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scipy-side", type=int, default=512, help="the side at which scipy is timed and compared (0 or --no-scipy: never)")
    ap.add_argument("--no-scipy", action="store_true")
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("--rounds must be at least 5")
    import bench
    from discorpy_amd import _ffi as F
    L = F.lib()
    F.require_device()
    dev = -1
    rng = np.random.default_rng(7)
    clock_call = None
    for side in [int(s) for s in a.sides.split(",")]:
        for name in a.dtypes.split(","):
            dt = np.dtype(name)
            code = F.DTYPE_BY_NAME[dt.name]
            # a dot-pattern-like image: a smooth illumination gradient under noise
            img = ((rng.random((side, side), dtype=np.float32) + np.linspace(0.5, 1.5, side, dtype=np.float32)) * 100.0).astype(dt)
            src = F.DeviceBuffer(img.nbytes, dev).upload(img)
            dst = F.DeviceBuffer(img.nbytes, dev)
            for sy, sx in SIZES:
                def run(_i=0):
                    F.check(L.dcp_median_filter_2d(src.ptr, dst.ptr, side, side, side, code, sy, sx, F.MEM_DEVICE, dev, None))
                for _ in range(a.warmup):
                    run()
                F.check(L.dcp_stream_synchronize(dev, None))
                rounds = []
                for _ in range(a.rounds):
                    e0, e1 = F.Event(dev), F.Event(dev)
                    e0.record()
                    for _r in range(a.reps):
                        run()
                    e1.record()
                    e1.synchronize()
                    rounds.append(e0.elapsed_ms(e1) / a.reps)
                gpu_ms = float(np.median(rounds))
                line = "%-8s %4d x %-4d size (%d, %d)  GPU %9.3f ms per call (rounds %.3f .. %.3f)  %s" % (
                    dt.name, side, side, sy, sx, gpu_ms, min(rounds), max(rounds), F.last_kernel())
                if not a.no_scipy and side == a.scipy_side:
                    from scipy import ndimage as ndi
                    t0 = time.perf_counter()
                    ref = ndi.median_filter(img, (sy, sx), mode="reflect")
                    cpu_ms = (time.perf_counter() - t0) * 1e3
                    line += "  scipy %10.1f ms  ratio %8.1f  equal: %s" % (cpu_ms, cpu_ms / gpu_ms, np.array_equal(dst.download(img.shape, dt), ref))
                print(line, flush=True)
                if side >= 2048 and dt == np.float32 and sy == 51:
                    clock_call = (src, dst, side, code)
            if clock_call is None or clock_call[0] is not src:
                src.free()
                dst.free()
    if clock_call:
        src, dst, side, code = clock_call
        clk = bench.clocks_under_load(lambda: F.check(L.dcp_median_filter_2d(src.ptr, dst.ptr, side, side, side, code, 51, 51, F.MEM_DEVICE, dev, None)),
                                      lambda: F.check(L.dcp_stream_synchronize(dev, None)))
        print("clock under the %d x %d float32 size-51 call: %s" % (side, side, clk), flush=True)


if __name__ == "__main__":
    main()
