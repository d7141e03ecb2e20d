#!/usr/bin/env python
"""Time connected-component labelling (dcp_label_2d), labelling plus the dot measurements (dcp_label_measures_2d) and hole filling
(dcp_fill_holes_2d) on device-resident images: the default route (x_label_lds = 1: a 128 x 32 tile per workgroup labelled in LDS, then
the tile seams) against the global union over every pixel pair (x_label_lds = 0), alternated in one process, and scipy.ndimage on the
same box.  Images of 2048^2 and 4096^2: a grid of dots of radius 8 on a pitch of 40 in uint8 and float32, and one image of random noise
of density 0.55 in uint8 (large ragged components: the hard case for a union-find).

Per case: warm-up calls of both routes, then `--rounds` (at least five) rounds; a round times `--reps` back-to-back calls of the tiled
route with a host clock around calls that end in a stream synchronise (dcp_label_2d synchronises by itself), then the same of the global
route.  Printed in ms per call: the median round of each route, the global route's round-to-round spread (max - min), the difference
tiled - global and whether it is within that spread (the bar for keeping x_label_lds = 1 the default: it is not slower than the global
route by more than that route's own spread, on the dot grid and on the noise), whether the two outputs are equal, and the number of
labels.  scipy is timed at the `--scipy-side` (2048) only, once per case, and there the line also carries the ratio scipy / GPU and
whether scipy's output equals the GPU's.  The last line is the core clock and package power under the 4096^2 uint8 label call.

    python tools/time_label.py [--sides 2048,4096] [--dtypes uint8,float32] [--rounds 5] [--reps 3] [--no-scipy]

With `--dotgrid` it times the kernels that follow the labelling in the dot-pattern route instead (discorpy_amd.prep.dotpattern;
csrc/dotgrid_kernels.hip), in ms per call: warm-up calls, then `--rounds` rounds of back-to-back calls that end synchronised, the median
round and the rounds' minimum and maximum; where two routes are compared they alternate round by round in one process.

  * the nearest squared distances (dcp_nearest_sq_dists, host points in and out) against the NumPy loop it replaces -- per point
    ``np.sort(np.sqrt(...))[1:4]`` over all points -- at `--points` (400, 2 000 and 10 000), with whether the results are equal;
  * radon_padded against linepattern.radon on the same device-resident 600 x 600 float32 ROI x 61 angles: the padded one has sqrt(2)
    times the columns and sqrt(2) times the rows, so twice the samples; the ratio is printed;
  * whole calc_size_distance and calc_hor_slope on a `--grid-side` (2048) square dot grid (radius 8, pitch 40, rotated by 1.5 degree)
    from a tensor.

    python tools/time_label.py --dotgrid [--rounds 5] [--dotgrid-reps 10] [--points 400,2000,10000] [--grid-side 2048]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def dot_grid(side, radius=8, pitch=40):
    y, x = np.mgrid[0:side, 0:side]
    return ((y % pitch - pitch // 2) ** 2 + (x % pitch - pitch // 2) ** 2 <= radius * radius)


def rotated_dot_grid(side, radius=8, pitch=40, deg=1.5):
    y, x = np.mgrid[0:side, 0:side].astype(np.float64)
    t = np.deg2rad(deg)
    u, v = x * np.cos(t) + y * np.sin(t) + 7.3, -x * np.sin(t) + y * np.cos(t) + 11.9
    du, dv = (u + pitch / 2) % pitch - pitch / 2, (v + pitch / 2) % pitch - pitch / 2
    return (du * du + dv * dv <= radius * radius).astype(np.int16)


def nearest_numpy_loop(cents):
    return np.asarray([np.sort(np.sqrt((dot[0] - cents[:, 0]) ** 2 + (dot[1] - cents[:, 1]) ** 2))[1:4] for dot in cents])


def dotgrid(a):
    """The --dotgrid mode (module docstring)."""
    import torch
    from discorpy_amd import _ffi as F
    from discorpy_amd.prep import dotpattern as dp
    from discorpy_amd.prep import linepattern as lp
    F.require_device()

    def sync():
        torch.cuda.synchronize()

    def alternated(routes, reps):
        """{name: ms per call of every round} of the routes (name -> callable), alternated round by round."""
        got = {name: [] for name in routes}
        for fn in routes.values():
            for _ in range(a.warmup + 1):
                fn()
        sync()
        for _ in range(a.rounds):
            for name, fn in routes.items():
                t0 = time.perf_counter()
                for _r in range(reps):
                    fn()
                sync()
                got[name].append((time.perf_counter() - t0) * 1e3 / reps)
        return got

    def line(label, r):
        print("%-58s %10.4f ms  (rounds %.4f .. %.4f)" % (label, float(np.median(r)), min(r), max(r)), flush=True)
        return float(np.median(r))

    rng = np.random.default_rng(11)
    for n in [int(v) for v in a.points.split(",")]:
        side = int(np.ceil(np.sqrt(n)))
        cents = (np.stack(np.divmod(np.arange(n), side), axis=1) * 40.0 + rng.random((n, 2)) * 6.0).astype(np.float64)
        got = alternated({"gpu": lambda: np.sqrt(dp._nearest_sq(cents))[:, 1:4], "numpy": lambda: nearest_numpy_loop(cents)}, 1 if n > 2000 else 3)
        g = line("nearest distances, N = %d: dcp_nearest_sq_dists + sqrt" % n, got["gpu"])
        c = line("nearest distances, N = %d: the NumPy loop" % n, got["numpy"])
        print("    ratio %.1f, equal: %s" % (c / g, np.array_equal(np.sqrt(dp._nearest_sq(cents))[:, 1:4], nearest_numpy_loop(cents))), flush=True)
    roi = torch.from_numpy(rng.random((600, 600)).astype(np.float32)).to("cuda:0")
    theta = 90.0 + np.arange(-30.0, 31.0)
    got = alternated({"padded": lambda: dp.radon_padded(roi, theta), "circle": lambda: lp.radon(roi, theta)}, a.dotgrid_reps)
    p = line("radon_padded, 600 x 600 float32 x 61 angles (side %d)" % dp._padded_side(600, 600), got["padded"])
    c = line("radon (circle), the same ROI", got["circle"])
    print("    ratio padded / circle %.2f (twice the samples)" % (p / c), flush=True)
    grid = torch.from_numpy(rotated_dot_grid(a.grid_side)).to("cuda:0")
    got = alternated({"size": lambda: dp.calc_size_distance(grid), "slope": lambda: dp.calc_hor_slope(grid)}, max(a.dotgrid_reps // 2, 1))
    line("calc_size_distance, %d x %d int16 tensor" % (a.grid_side, a.grid_side), got["size"])
    line("calc_hor_slope, %d x %d int16 tensor" % (a.grid_side, a.grid_side), got["slope"])
    print("    size, distance %r; slope %r" % (dp.calc_size_distance(grid), dp.calc_hor_slope(grid)), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sides", default="2048,4096")
    ap.add_argument("--dtypes", default="uint8,float32")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--scipy-side", type=int, default=2048, help="the side at which scipy is timed and compared (0 or --no-scipy: never)")
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--dotgrid", action="store_true", help="time the dot-grid kernels instead (the last part of the description)")
    ap.add_argument("--dotgrid-reps", type=int, default=10)
    ap.add_argument("--points", default="400,2000,10000")
    ap.add_argument("--grid-side", type=int, default=2048)
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("--rounds must be at least 5")
    if a.dotgrid:
        return dotgrid(a)
    import bench
    from discorpy_amd import _ffi as F
    L = F.lib()
    F.require_device()
    dev = -1
    clock_call = None
    for side in [int(s) for s in a.sides.split(",")]:
        images = [("dots", np.dtype(name), dot_grid(side).astype(name)) for name in a.dtypes.split(",")]
        images.append(("noise", np.dtype(np.uint8), (np.random.default_rng(55).random((side, side)) < 0.55).astype(np.uint8)))
        for what, dt, img in images:
            code = F.DTYPE_BY_NAME[dt.name]
            src = F.DeviceBuffer(img.nbytes, dev).upload(img)
            lab = {v: F.DeviceBuffer(img.size * 4, dev) for v in (1, 0)}
            filled = {v: F.DeviceBuffer(img.size, dev) for v in (1, 0)}
            num = F.C.c_int(0)
            F.check(L.dcp_label_2d(src.ptr, lab[1].ptr, side, side, side, code, 4, F.C.byref(num), F.MEM_DEVICE, dev, None))
            count = max(num.value, 1)
            sums, boxes = F.DeviceBuffer(count * 32, dev), F.DeviceBuffer(count * 16, dev)

            def label(v):
                F.check(L.dcp_label_2d(src.ptr, lab[v].ptr, side, side, side, code, 4, F.C.byref(num), F.MEM_DEVICE, dev, None))

            def label_measure(v):
                label(v)
                F.check(L.dcp_label_measures_2d(src.ptr if dt.itemsize <= 2 else None, lab[v].ptr, side, side, side, side, code, num.value, sums.ptr,
                                                boxes.ptr, F.MEM_DEVICE, dev, None))
                F.check(L.dcp_stream_synchronize(dev, None))

            def fill(v):
                F.check(L.dcp_fill_holes_2d(src.ptr, filled[v].ptr, side, side, side, code, F.MEM_DEVICE, dev, None))
                F.check(L.dcp_stream_synchronize(dev, None))

            for op_name, op in (("label", label), ("label + measures", label_measure), ("fill_holes", fill)):
                def timed(v):
                    F.set_option("x_label_lds", v)
                    t0 = time.perf_counter()
                    for _r in range(a.reps):
                        op(v)
                    return (time.perf_counter() - t0) * 1e3 / a.reps
                for v in (1, 0):
                    F.set_option("x_label_lds", v)
                    for _ in range(a.warmup):
                        op(v)
                rounds = {1: [], 0: []}
                for _ in range(a.rounds):
                    for v in (1, 0):
                        rounds[v].append(timed(v))
                F.set_option("x_label_lds", 1)
                tiled, glob = float(np.median(rounds[1])), float(np.median(rounds[0]))
                spread = max(rounds[0]) - min(rounds[0])
                if op is fill:
                    out1, out0 = filled[1].download(img.shape, np.bool_), filled[0].download(img.shape, np.bool_)
                else:
                    out1, out0 = lab[1].download(img.shape, np.int32), lab[0].download(img.shape, np.int32)
                line = ("%-5s %-8s %4d x %-4d %-16s tiled %9.4f ms (rounds %.4f .. %.4f)  global %9.4f ms (rounds %.4f .. %.4f, spread %.4f)"
                        "  tiled - global %+.4f ms: %s  routes equal: %s  labels: %d" % (
                            what, dt.name, side, side, op_name, tiled, min(rounds[1]), max(rounds[1]), glob, min(rounds[0]), max(rounds[0]), spread,
                            tiled - glob, "within the bar" if tiled - glob <= spread else "MISSES the bar", np.array_equal(out1, out0), num.value))
                if not a.no_scipy and side == a.scipy_side:
                    from scipy import ndimage as ndi
                    t0 = time.perf_counter()
                    if op is fill:
                        ref = ndi.binary_fill_holes(img)
                    else:
                        ref, ref_num = ndi.label(img)
                        if op is label_measure:
                            idx = np.arange(1, ref_num + 1)
                            weights = img if dt.itemsize <= 2 else ref > 0
                            ndi.sum_labels(weights, ref, idx), ndi.center_of_mass(weights, ref, idx), ndi.find_objects(ref)
                    cpu_ms = (time.perf_counter() - t0) * 1e3
                    line += "  scipy %9.1f ms  ratio %8.1f  equal to scipy: %s" % (cpu_ms, cpu_ms / tiled, np.array_equal(out1, ref))
                print(line, flush=True)
            if side >= 4096 and what == "dots" and dt == np.uint8:
                clock_call = (src, lab[1], side, code)
            for buf in [sums, boxes, filled[1], filled[0], lab[0]] + ([] if clock_call and clock_call[0] is src else [src, lab[1]]):
                buf.free()
    if clock_call:
        src, out, side, code = clock_call
        num = F.C.c_int(0)
        clk = bench.clocks_under_load(lambda: F.check(L.dcp_label_2d(src.ptr, out.ptr, side, side, side, code, 4, F.C.byref(num), F.MEM_DEVICE, dev, None)),
                                      lambda: F.check(L.dcp_stream_synchronize(dev, None)))
        print("clock under the %d x %d uint8 label call: %s" % (side, side, clk), flush=True)


if __name__ == "__main__":
    main()
