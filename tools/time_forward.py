#!/usr/bin/env python
"""Time the forward scatter (post.unwarp_image_forward's call, dcp_unwarp_image_forward) on a device-resident frame under the model of
configs.cfg2(): float32 and uint16, us per call from HIP events around back-to-back calls after a warm-up, and the bytes per pixel
that time stands for at the HBM peak, next to the design's 16-20 B per float32 pixel (4 B atomic, 4 B to clear the winner plane, 4 B
read of it, 4 B gathered, 4 B stored).  A ring of frames larger than the 256 MB Infinity Cache.

The two kernels of a call cannot be told apart by events around the call; their split comes from a kernel trace taken in a run of
its own:

    python tools/time_forward.py [--size 4096] [--ring 4] [--reps 40] [--dtypes float32,uint16]
    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python tools/time_forward.py --reps 10
    python tools/time_forward.py --split-from DIR        # no GPU: average ns of forward_winner_kernel / forward_fill_kernel / the clear
"""
import argparse
import csv
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def split_from(trace_dir):
    """Average duration of the winner pass, the fill pass and the plane clear in every *kernel_trace.csv under `trace_dir`."""
    groups = {"forward_winner_kernel": [], "forward_fill_kernel": [], "clear": []}
    for base, _, files in os.walk(trace_dir):
        for f in files:
            if not f.endswith("kernel_trace.csv"):
                continue
            with open(os.path.join(base, f), newline="") as fh:
                for row in csv.DictReader(fh):
                    name, dur = row["Kernel_Name"], int(row["End_Timestamp"]) - int(row["Start_Timestamp"])
                    key = next((k for k in ("forward_winner_kernel", "forward_fill_kernel") if k in name), None)
                    if key is None and ("fill" in name.lower() or "memset" in name.lower()):
                        key = "clear"
                    if key:
                        groups[key].append(dur)
    total = sum(np.mean(v) for v in groups.values() if v)
    for key, v in groups.items():
        if v:
            # the trace holds both element types: the median separates nothing, so the spread is printed too
            print("%-22s %6d launches  mean %8.1f us  min %8.1f  max %8.1f  (%4.1f %% of the three)" % (
                key, len(v), np.mean(v) / 1e3, np.min(v) / 1e3, np.max(v) / 1e3, 100.0 * np.mean(v) / total))
        else:
            print("%-22s none in the trace" % key)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--ring", type=int, default=4)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--dtypes", default="float32,uint16")
    ap.add_argument("--split-from", default=None, metavar="DIR")
    a = ap.parse_args()
    if a.split_from:
        return split_from(a.split_from)
    import bench
    from discorpy_amd import _ffi as F
    from discorpy_amd import configs
    L = F.lib()
    F.require_device()
    dev = -1
    cfg = configs.cfg2()
    s = a.size / 4096.0
    fact = [c * s ** -i for i, c in enumerate(cfg["list_fact"])]
    xc, yc = cfg["xcenter"] * s, cfg["ycenter"] * s
    fa, nf = F.fact_array(fact)
    H = W = a.size
    rng = np.random.default_rng(7)
    for name in a.dtypes.split(","):
        dt = np.dtype(name)
        code = F.DTYPE_BY_NAME[dt.name]
        img = (rng.random((H, W), dtype=np.float32) * 60000.0).astype(dt)
        srcs = [F.DeviceBuffer(img.nbytes, dev).upload(img) for _ in range(a.ring)]
        dsts = [F.DeviceBuffer(img.nbytes, dev) for _ in range(a.ring)]

        def run(i):
            F.check(L.dcp_unwarp_image_forward(srcs[i % a.ring].ptr, dsts[i % a.ring].ptr, code, H, W, W, 1, xc, yc, fa, nf, F.MEM_DEVICE, dev, None))
        t = bench.timed_launches(run, a.reps, dev, settle_ms=300.0)
        design = 12 + 2 * dt.itemsize                       # atomic + clear + plane read, element gathered + stored
        print("%-8s %d x %d  %8.2f us per call  = %5.1f B/px at 8 TB/s (design: %d B/px, %.1f us at 8 TB/s)  %s" % (
            dt.name, H, W, t, t * 1e-6 * 8e12 / (H * W), design, design * H * W / 8e12 * 1e6, F.last_kernel()), flush=True)
        for b in srcs + dsts:
            b.free()


if __name__ == "__main__":
    main()
