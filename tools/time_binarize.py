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


def main():
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
