#!/usr/bin/env python
"""Time the binarization of a dot image (discorpy_amd.prep.preprocessing.binarization and the entry points under it) on 2048^2 and
4096^2 float32 images: a grid of dots of radius 8 on a pitch of 40 over a gradient background with salt-and-pepper noise.

Per side, in ms per call (warm-up calls, then `--rounds` (at least five) rounds of `--reps` back-to-back calls with a host clock around
calls that end in a stream synchronise; the median round, and the rounds' minimum and maximum):

  * every step on the device-resident plane: abs, the 2 x 2 median, minimum / maximum, the 512-bin histogram of the ROI, the threshold,
    clear_border, the opening, hole filling;
  * the opening as one launch against two (lab option x_morph_fused 1 / 0) and the histogram counted in LDS against global atomics
    (x_hist_lds 1 / 0), alternated in one process, with the difference and the second route's spread;
  * the whole binarization for NumPy input (upload, every step, download) and for a torch tensor on the device;
  * at `--scipy-side` (2048) the scipy / NumPy composite of tests/helpers/binarize_reference.py on the host -- the only route before
    this one -- with the ratio and whether the outputs are equal.

The last line is the core clock and package power under the 4096^2 threshold call.

    python tools/time_binarize.py [--sides 2048,4096] [--rounds 5] [--reps 10] [--no-scipy]

`--threshold` times the other way to a threshold instead, calculate_threshold and the sort under it (its own --help:
`python tools/time_binarize.py --threshold --help`).
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))


def dot_image(side, radius=8, pitch=40, seed=5):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:side, 0:side]
    r2 = ((y + 7) % pitch - pitch // 2) ** 2 + ((x + 13) % pitch - pitch // 2) ** 2
    ring = ((y + 7) // pitch + (x + 13) // pitch) % 3 == 0
    dots = (r2 <= radius * radius) & ~(ring & (r2 <= 9))
    img = np.where(dots, 0.8, 0.15 + 0.04 * x / side + 0.02 * y / side)
    noise = rng.random((side, side))
    img = np.where(noise < 0.004, 1.0, np.where(noise > 0.996, 0.0, img)) + 0.01 * rng.standard_normal((side, side))
    return img.astype(np.float32)


# --------------------------------------------------------------------------- --threshold: calculate_threshold and its sort

THRESHOLD_DOC = """Time calculate_threshold (discorpy_amd.prep.threshold) and the sort under it on 2048^2 and 4096^2 planes of float32, float64, uint16
and uint8: a bright background with a gradient and noise, darker dots on a pitch of 40.

Two sides alternate round by round (`--rounds`, at least five; a round is `--reps` back-to-back calls that end synchronised, host clock
around them), in ms per call with the median round, the rounds' minimum and maximum and the spread:

  * calculate_threshold from a device tensor and from a NumPy array, against the same formula through np.sort / scipy.ndimage.zoom /
    np.polyfit on this machine's host (one call per round: it takes seconds), with whether the two thresholds are equal;
  * the sort alone (sort_values of the device tensor) against torch.sort of the same tensor flattened, with whether the outputs are equal
    and the difference of the medians beside torch.sort's own round-to-round spread.

The last line is the core clock and package power under the 4096^2 float32 sort.

    python tools/time_binarize.py --threshold [--sides 2048,4096] [--dtypes float32,float64,uint16,uint8] [--rounds 5] [--reps 5] [--no-host]
"""


def dot_plane(side, dtype, seed=5):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:side, 0:side]
    r2 = ((y + 7) % 40 - 20) ** 2 + ((x + 13) % 40 - 20) ** 2
    img = np.where(r2 <= 64, 0.2, 0.75 + 0.04 * x / side + 0.02 * y / side) + 0.01 * rng.standard_normal((side, side))
    scale = {"float32": 1.0, "float64": 1.0, "uint16": 60000.0, "uint8": 250.0}[dtype]
    img = np.clip(img, 0.0, 1.0) * scale
    return np.round(img).astype(dtype) if np.dtype(dtype).kind == "u" else img.astype(dtype)


def threshold_main():
    ap = argparse.ArgumentParser(description=THRESHOLD_DOC, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--threshold", action="store_true", help="this mode")
    ap.add_argument("--sides", default="2048,4096")
    ap.add_argument("--dtypes", default="float32,float64,uint16,uint8")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-host", action="store_true", help="leave out the np.sort / ndi.zoom / np.polyfit side")
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("--rounds must be at least 5")
    import scipy.ndimage as ndi
    import torch
    import bench
    from discorpy_amd import _ffi as F
    from discorpy_amd.prep import threshold as thr
    F.require_device()

    def sync():
        torch.cuda.synchronize()

    def timed(fn, reps):
        t0 = time.perf_counter()
        for _ in range(reps):
            out = fn()
        sync()
        return (time.perf_counter() - t0) * 1e3 / reps, out

    def alternate(sides):
        """{name: rounds} and {name: last result} of the callables of `sides` = [(name, fn, reps)], taking turns round by round."""
        got, last = {name: [] for name, _, _ in sides}, {}
        for name, fn, _ in sides:
            for _ in range(a.warmup):
                fn()
            sync()
        for _ in range(a.rounds):
            for name, fn, reps in sides:
                ms, last[name] = timed(fn, reps)
                got[name].append(ms)
        return got, last

    def line(label, r):
        print("  %-44s %10.4f ms  (rounds %.4f .. %.4f, spread %.4f)" % (label, float(np.median(r)), min(r), max(r), max(r) - min(r)), flush=True)
        return float(np.median(r))

    def host_formula(img):
        profile = ndi.zoom(np.sort(img, axis=None), 1.0 * max(img.shape) / img.size, mode="nearest")
        return thr._threshold_of_profile(profile, "bright", 2.0)

    clock_plane = None
    for side in [int(s) for s in a.sides.split(",")]:
        for dtype in a.dtypes.split(","):
            img = dot_plane(side, dtype)
            t = torch.from_numpy(img.view(np.int16) if dtype == "uint16" else img).to("cuda:0")          # (torch sorts int16: the same bits, another order)
            print("---- %d x %d %s" % (side, side, dtype), flush=True)
            if dtype == "uint16":
                dev = F.DeviceArray(img.shape, img.dtype).copy_from_host(img)          # a device array of the plane's own type
                sides = [("calculate_threshold, device array", lambda: thr.calculate_threshold(dev), a.reps)]
            else:
                sides = [("calculate_threshold, device tensor", lambda: thr.calculate_threshold(t), a.reps)]
            sides.append(("calculate_threshold, NumPy array", lambda: thr.calculate_threshold(img), a.reps))
            if not a.no_host:
                sides.append(("np.sort / ndi.zoom / np.polyfit on the host", lambda: host_formula(img), 1))
            got, last = alternate(sides)
            med = {name: line(name, r) for name, r in got.items()}
            values = list(last.values())
            print("  thresholds %s   equal: %s" % (" ".join("%.9g" % v for v in values), all(v == values[0] for v in values)), flush=True)
            if not a.no_host:
                host = med["np.sort / ndi.zoom / np.polyfit on the host"]
                print("  host / device: %.1f from the device, %.1f from NumPy" % (host / med[sides[0][0]], host / med[sides[1][0]]), flush=True)
            flat = t.reshape(-1)
            got, last = alternate([("sort_values (radix sort kernels)", lambda: thr.sort_values(t), a.reps),
                                   ("torch.sort of the same tensor", lambda: torch.sort(flat).values, a.reps)])
            ours, theirs = line("sort_values (radix sort kernels)", got["sort_values (radix sort kernels)"]), line("torch.sort of the same tensor", got["torch.sort of the same tensor"])
            spread = max(got["torch.sort of the same tensor"]) - min(got["torch.sort of the same tensor"])
            print("  sort_values - torch.sort: %+.4f ms (torch.sort's spread %.4f)   outputs equal: %s" % (
                ours - theirs, spread, bool(torch.equal(last["sort_values (radix sort kernels)"], last["torch.sort of the same tensor"]))), flush=True)
            if side >= 4096 and dtype == "float32":
                clock_plane = t
    if clock_plane is not None:
        print("clock under the 4096 x 4096 float32 sort: %s" % (bench.clocks_under_load(lambda: thr.sort_values(clock_plane), sync),), flush=True)


def main():
    if "--threshold" in sys.argv[1:]:
        return threshold_main()
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sides", default="2048,4096")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--scipy-side", type=int, default=2048, help="the side at which the scipy / NumPy composite is timed and compared (0 or --no-scipy: never)")
    ap.add_argument("--no-scipy", action="store_true")
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("--rounds must be at least 5")
    import bench
    import torch
    from discorpy_amd import _ffi as F
    from discorpy_amd.prep import preprocessing as prep
    F.require_device()

    def sync():
        torch.cuda.synchronize()

    def rounds_of(fn, setup=None):
        if setup:
            setup()
        for _ in range(a.warmup):
            fn()
        sync()
        out = []
        for _ in range(a.rounds):
            if setup:
                setup()
            t0 = time.perf_counter()
            for _r in range(a.reps):
                fn()
            sync()
            out.append((time.perf_counter() - t0) * 1e3 / a.reps)
        return out

    def report(label, r):
        print("%-46s %9.4f ms  (rounds %.4f .. %.4f)" % (label, float(np.median(r)), min(r), max(r)), flush=True)
        return float(np.median(r))

    def ab(label, key, fn):
        """fn under the lab option `key` = 1 and 0, alternated round by round."""
        got = {1: [], 0: []}
        for v in (1, 0):
            F.set_option(key, v)
            for _ in range(a.warmup):
                fn()
            sync()
        for _ in range(a.rounds):
            for v in (1, 0):
                F.set_option(key, v)
                t0 = time.perf_counter()
                for _r in range(a.reps):
                    fn()
                sync()
                got[v].append((time.perf_counter() - t0) * 1e3 / a.reps)
        F.set_option(key, 1)
        one, zero = float(np.median(got[1])), float(np.median(got[0]))
        spread = max(got[0]) - min(got[0])
        print("%-46s %s=1 %9.4f ms (rounds %.4f .. %.4f)   %s=0 %9.4f ms (rounds %.4f .. %.4f, spread %.4f)   1 - 0: %+.4f ms" % (
            label, key, one, min(got[1]), max(got[1]), key, zero, min(got[0]), max(got[0]), spread, one - zero), flush=True)

    clock_call = None
    for side in [int(s) for s in a.sides.split(",")]:
        img = dot_image(side)
        t = torch.from_numpy(img).to("cuda:0")
        print("---- %d x %d float32" % (side, side), flush=True)
        im = prep._rows_image(t)
        report("abs", rounds_of(lambda: prep._abs_plane(im)))
        absd = prep._abs_plane(im)
        report("median 2 x 2", rounds_of(lambda: prep.median_filter(absd, (2, 2))))
        den = prep.median_filter(absd, (2, 2))
        roi = prep._rows_image(prep._select_roi(den, 0.3))
        report("minimum / maximum of the ROI", rounds_of(lambda: prep._minmax(roi)))
        lo, hi, _ = prep._minmax(roi)
        edges = np.linspace(np.float32(lo), np.float32(hi), 513, dtype=np.float32)
        report("histogram of the ROI, 512 bins", rounds_of(lambda: prep._histogram(roi, 512, edges=edges)))
        whole = prep._rows_image(den)
        ab("histogram of the whole plane, 512 bins", "x_hist_lds", lambda: prep._histogram(whole, 512, edges=edges))
        report("threshold_otsu of the ROI", rounds_of(lambda: prep.threshold_otsu(prep._select_roi(den, 0.3), 512)))
        thres = prep.threshold_otsu(prep._select_roi(den, 0.3), 512)
        report("threshold + count", rounds_of(lambda: prep._threshold_plane(whole, float(thres))))
        mask, count = prep._threshold_plane(whole, float(thres))
        mi = prep._rows_image(mask)
        report("clear_border", rounds_of(lambda: prep._clear_border_plane(mi)))
        cleared = prep._rows_image(prep._clear_border_plane(mi))
        for op, name in ((0, "erosion"), (1, "dilation")):
            report(name, rounds_of(lambda op=op: prep._morph_plane(cleared, op)))
        ab("opening", "x_morph_fused", lambda: prep._morph_plane(cleared, 2))
        opened = prep._morph_plane(cleared, 2)
        report("binary_fill_holes", rounds_of(lambda: prep.binary_fill_holes(opened)))
        gpu_t = report("binarization, torch tensor on the device", rounds_of(lambda: prep.binarization(t)))
        gpu_n = report("binarization, NumPy in and out", rounds_of(lambda: prep.binarization(img)))
        got = prep.binarization(img)
        print("set pixels %d of %d, dots %d" % (int(got.sum()), got.size, prep.label(got)[1]), flush=True)
        if not a.no_scipy and side == a.scipy_side:
            import binarize_reference as bref
            t0 = time.perf_counter()
            want = bref.binarization_stages(img)["filled"]
            cpu_ms = (time.perf_counter() - t0) * 1e3
            print("%-46s %9.1f ms  ratio to NumPy in and out %.1f, to the tensor %.1f  equal: %s" % (
                "scipy / NumPy composite on the host", cpu_ms, cpu_ms / gpu_n, cpu_ms / gpu_t, np.array_equal(got, want)), flush=True)
        if side >= 4096:
            clock_call = (whole, float(thres))
    if clock_call:
        whole, thres = clock_call
        clk = bench.clocks_under_load(lambda: prep._threshold_plane(whole, thres), sync)
        print("clock under the 4096 x 4096 threshold call: %s" % (clk,), flush=True)


if __name__ == "__main__":
    main()
