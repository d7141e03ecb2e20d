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

--fourier: the other Gaussian of the line-pattern route, with options of its own.  Time the Fourier Gaussian filter (prep.preprocessing._apply_fft_filter, dcp_fourier_gauss_2d: two Toeplitz passes in float64, no FFT) on
device-resident float32 images against the same formula through an FFT library on the same device tensor
(torch.nn.functional.pad, torch.fft.fft2 / ifft2 in complex128, the sign plane and the window made once outside the timed calls), the
two routes alternated in one process, and once per case against the reference's route on the host (scipy.fftpack, restated).
Cases: 2000 x 2000 at (sigma, pad) = (10, 100) and (5, 100), 4096 x 4096 at (10, 100), mode "reflect".

Per case: warm-up calls of both routes, then `--rounds` (at least five) rounds; a round times `--reps` back-to-back calls of the
Toeplitz route between device events, then the same of the FFT route.  Printed in ms per call: the median round of each route with
its range, the ratio FFT / Toeplitz, the largest difference between the two outputs over max|output|, the taps the kernels kept per
axis, the fused multiply-adds that makes and the rate it amounts to; with scipy the host's time, its ratio to the Toeplitz route and
the difference of the outputs.  There is no threshold: the numbers go to DESIGN.md as they are.

    python tools/time_gaussian.py --fourier [--cases 2000:10:100,2000:5:100,4096:10:100] [--rounds 5] [--reps 10] [--no-scipy]

--cross-points: the whole line-pattern route, with options of its own.  Time prep.linepattern.get_cross_points_hor_lines on an
1800 x 2000 float32 line pattern (line distance 90, tilted 1.5 degrees, default arguments) for NumPy and for tensor input (wall clock:
the call ends on the host), and each of its GPU steps on the device tensor between device events: max - mat, normalization_fft(mat, 5),
gaussian_filter(mat, 3), get_tilted_profiles (its host part -- the coordinates -- on the wall clock beside it) and the peak search
(dcp_local_extrema_rows on device-resident profiles; the wrapper on host rows on the wall clock).  Warm-up calls, then `--rounds` (at
least five) rounds of `--reps` calls; the median round and the range are printed in ms per call.  The NumPy restatement of the peak
search (tests/helpers/peaks_reference.py: the reference's loop with the sort of candidate windows only) is timed once on the same
profiles, on this machine's CPU, and its positions are compared with the kernel's.

    python tools/time_gaussian.py --cross-points [--shape 1800x2000] [--dist 90] [--rounds 5] [--reps 5] [--no-numpy]

--radon: the transform in front of that route, with options of its own.  Time the Radon transform (prep.linepattern.radon's call,
dcp_radon_2d: one launch of radon_kernel for all angles) on device-resident planes: 600 x 600 float32 and float64 (the ROI of a
2000-wide image at the default ratio of the slope search) x 61 angles, the coarse grid of calc_slope_distance_ver_lines (around 0
degree: neighbouring lanes read neighbouring elements) and of calc_slope_distance_hor_lines (around 90 degree: neighbouring lanes read
neighbouring ROWS of the source).  Per element type: warm-up calls of both sweeps, then `--rounds` (at least five) rounds; a round times
`--reps` back-to-back calls of the 0-degree sweep between device events, then the same of the 90-degree sweep.  A call copies its angle
table from host memory and waits for that copy before it enqueues the kernel, so a call is more than its kernel: the same call on a
1 x 1 plane (a kernel of one thread and one row per angle) is timed beside it as the floor of a call.  Printed in ms per call: the
median round of each sweep with its range, the floor, the ratio 90 / 0 of the calls and of the calls less the floor, and whether two
calls of a sweep give the same bits.  There is no time to beat: the numbers go to DESIGN.md as they are; the ratio decides whether a
patch of the source staged in LDS is worth its code.

    python tools/time_gaussian.py --radon [--side 600] [--angles 61] [--dtypes float32,float64] [--rounds 5] [--reps 200]

--select-peaks: the selection behind the peak search, with options of its own.  Time dcp_select_peaks_rows (one launch of
select_peaks_kernel, a wave per candidate) on 4096 candidates at radius 11 on device-resident float32 and float64 profiles of 2000
samples: lines 90 apart on a sloping background with noise, three candidates in four on a line, the fourth between two lines.  Warm-up
calls, then `--rounds` (at least five) rounds of `--reps` back-to-back calls between device events.  A call copies its two candidate
tables from host memory and waits for that copy, so the same call on one candidate is timed beside it as the floor of a call.  Printed
in ms per call: the median round with its range, the floor, how many candidates were kept, how many ended with each status, and whether
two calls give the same bits.  There is no time to beat: the numbers go to DESIGN.md as they are.

    python tools/time_gaussian.py --select-peaks [--peaks 4096] [--radius 11] [--length 2000] [--dtypes float32,float64] [--rounds 5] [--reps 20]

--select-peaks --wired: the peak search with select_peaks=True in one call (dcp_extrema_select_rows) against the composition it
replaces, on device-resident float32 and float64 profiles (300 x 2000, lines 90 apart, radius 11).  The composition: dcp_local_extrema_rows
into a device table, that table downloaded, the two candidate tables built in NumPy, dcp_select_peaks_rows on the device-resident plane
max - row (formed once, outside the timed region: a gift to the composition), the kept mask downloaded, the closed-form parabola of the
kept candidates in NumPy on a host copy of the rows.  The two routes alternate in one process: warm-up, then `--rounds` (at least five)
rounds, a round timing `--reps` back-to-back runs of one route between device events and then the same of the other.  Printed in ms per
run: the median round of each route with its range, whether the two give the same positions, and the core clock under the one call.
The bar: the one call is not slower than the composition by more than the composition's own round-to-round spread.  Then the whole of
prep.linecomplete.get_cross_points_hor_lines on an 1800 x 2000 pattern, flag on against flag off, in wall time.

    python tools/time_gaussian.py --select-peaks --wired [--nrows 300] [--radius 11] [--length 2000] [--dtypes float32,float64] [--rounds 5] [--reps 10] [--no-image]
"""
import argparse
import os
import re
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

MODE_NEAREST = 4        # DCP_MODE_NEAREST


def main():
    if "--fourier" in sys.argv[1:]:
        return fourier_main([v for v in sys.argv[1:] if v != "--fourier"])
    if "--cross-points" in sys.argv[1:]:
        return cross_points_main([v for v in sys.argv[1:] if v != "--cross-points"])
    if "--radon" in sys.argv[1:]:
        return radon_main([v for v in sys.argv[1:] if v != "--radon"])
    if "--select-peaks" in sys.argv[1:] and "--wired" in sys.argv[1:]:
        return select_wired_main([v for v in sys.argv[1:] if v not in ("--select-peaks", "--wired")])
    if "--select-peaks" in sys.argv[1:]:
        return select_peaks_main([v for v in sys.argv[1:] if v != "--select-peaks"])
    ap =argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
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


def reference_filter(mat, sigma, pad, mode="reflect"):
    """discorpy/prep/preprocessing.py:102-128 restated on scipy.fftpack."""
    from scipy.fftpack import fft2, ifft2
    mat = np.pad(mat, ((pad, pad), (pad, pad)), mode=mode)
    (height, width) = mat.shape
    xcenter, ycenter = (width - 1.0) / 2.0, (height - 1.0) / 2.0
    y, x = np.ogrid[-ycenter:height - ycenter, -xcenter:width - xcenter]
    num = 2.0 * sigma * sigma
    window = np.exp(-(x * x / num + y * y / num))
    x, y = np.meshgrid(np.arange(0, width), np.arange(0, height))
    matsign = np.power(-1.0, x + y)
    mat = np.real(ifft2(fft2(mat * matsign) * window) * matsign)
    return mat[pad:height - pad, pad:width - pad]


def fourier_main(argv):
    ap = argparse.ArgumentParser(prog="time_gaussian.py --fourier", description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", default="2000:10:100,2000:5:100,4096:10:100", help="side:sigma:pad, comma-separated")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-scipy", action="store_true")
    a = ap.parse_args(argv)
    if a.rounds < 5:
        ap.error("--rounds must be at least 5")
    import torch
    from discorpy_amd import _ffi as F
    from discorpy_amd.prep import preprocessing as prep
    F.require_device()
    rng = np.random.default_rng(11)
    for spec in a.cases.split(","):
        side, sigma, pad = spec.split(":")
        side, sigma, pad = int(side), float(sigma), int(pad)
        # a line-pattern-like image: a smooth illumination gradient under noise, far from 0
        img = ((rng.random((side, side), dtype=np.float32) + np.linspace(0.5, 1.5, side, dtype=np.float32)) * 100.0).astype(np.float32)
        t = torch.from_numpy(img).to("cuda:0")
        n = side + 2 * pad
        idx = torch.arange(n, device=t.device)
        sign = torch.where((idx[:, None] + idx[None, :]) % 2 == 0, 1.0, -1.0).to(torch.float64)
        window = torch.from_numpy(prep._make_window(n, n, sigma)).to(t.device)

        def toeplitz():
            return prep._apply_fft_filter(t, sigma, pad)

        def library():
            m = torch.nn.functional.pad(t[None, None].to(torch.float64), (pad, pad, pad, pad), mode="reflect")[0, 0]
            out = torch.fft.ifft2(torch.fft.fft2(m * sign) * window).real * sign
            return out[pad:n - pad, pad:n - pad]

        routes = {"toeplitz": toeplitz, "fft": library}

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / a.reps
        outs = {}
        for name, fn in routes.items():
            for _ in range(a.warmup):
                outs[name] = fn()
            if name == "toeplitz":
                kernels = F.last_kernel()
        torch.cuda.synchronize()
        rounds = {name: [] for name in routes}
        for _ in range(a.rounds):
            for name, fn in routes.items():
                rounds[name].append(timed(fn))
        med = {name: float(np.median(v)) for name, v in rounds.items()}
        got = {name: v.cpu().numpy() for name, v in outs.items()}
        diff = np.abs(got["toeplitz"] - got["fft"]).max() / np.abs(got["fft"]).max()
        taps = [int(v) for pair in re.findall(r"taps=(\d+) of (\d+)", kernels) for v in pair]
        ky, kx = taps[0], taps[2]

        def steps(kept, whole):          # indices a block of 8 outputs walks: its cyclic window of 2 R + 8, or the whole axis
            return n if kept == whole else min(n, (kept - 1) // 2 + 8)
        fma = 2.0 * side * n * steps(ky, taps[1]) + 2.0 * side * side * steps(kx, taps[3])     # per step and output: re and im
        line = ("float32 %4d x %-4d sigma %-3g pad %-3d toeplitz %8.4f ms (rounds %.4f .. %.4f)  fft library %8.4f ms (rounds %.4f .. %.4f)"
                "  fft / toeplitz %.2f  |difference| / max %.2e  taps %d, %d  %.3g FMA = %.2f TFLOP/s float64" % (
                    side, side, sigma, pad, med["toeplitz"], min(rounds["toeplitz"]), max(rounds["toeplitz"]), med["fft"], min(rounds["fft"]),
                    max(rounds["fft"]), med["fft"] / med["toeplitz"], diff, ky, kx, fma, 2.0 * fma / (med["toeplitz"] * 1e-3) / 1e12))
        if not a.no_scipy:
            t0 = time.perf_counter()
            ref = reference_filter(img, sigma, pad)
            cpu_ms = (time.perf_counter() - t0) * 1e3
            line += "  scipy.fftpack on the host %9.1f ms  ratio %7.1f  |difference| / max %.2e" % (
                cpu_ms, cpu_ms / med["toeplitz"], np.abs(got["toeplitz"] - ref).max() / np.abs(ref).max())
        print(line + "  [%s]" % kernels, flush=True)


def cross_points_main(argv):
    ap = argparse.ArgumentParser(prog="time_gaussian.py --cross-points", description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", default="1800x2000")
    ap.add_argument("--dist", type=float, default=90.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-numpy", action="store_true", help="skip the NumPy restatement of the peak search")
    a = ap.parse_args(argv)
    if a.rounds < 5:
        ap.error("--rounds must be at least 5")
    import torch
    from discorpy_amd import _ffi as F
    from discorpy_amd.prep import linepattern as lp
    from discorpy_amd.prep import preprocessing as prep
    F.require_device()
    height, width = (int(v) for v in a.shape.split("x"))
    rng = np.random.default_rng(13)
    y, x = np.mgrid[0:height, 0:width].astype(np.float64)
    tilt = np.deg2rad(1.5)
    u, v = x * np.cos(tilt) + y * np.sin(tilt) + 7.3, -x * np.sin(tilt) + y * np.cos(tilt) + 11.9
    du, dv = (u + a.dist / 2) % a.dist - a.dist / 2, (v + a.dist / 2) % a.dist - a.dist / 2
    img = 1.0 - 0.8 * np.maximum(np.exp(-du * du / (2 * 2.5 ** 2)), np.exp(-dv * dv / (2 * 2.5 ** 2)))
    img = (img * (0.75 + 0.2 * x / width + 0.1 * y / height) * (1.0 + 0.01 * rng.standard_normal(img.shape))).astype(np.float32)
    slope = float(np.tan(tilt))
    t = torch.from_numpy(img).to("cuda:0")

    def wall(fn):
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.reps

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.reps

    def report(label, timer, fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        rounds = [timer(fn) for _ in range(a.rounds)]
        print("%-74s %9.4f ms (rounds %.4f .. %.4f)" % (label, float(np.median(rounds)), min(rounds), max(rounds)), flush=True)
        return float(np.median(rounds))
    points = lp.get_cross_points_hor_lines(img, slope, a.dist)
    print("float32 %d x %d, line distance %g: %d points" % (height, width, a.dist, len(points)), flush=True)
    report("get_cross_points_hor_lines, NumPy input (wall clock)", wall, lambda: lp.get_cross_points_hor_lines(img, slope, a.dist))
    report("get_cross_points_hor_lines, tensor input (wall clock)", wall, lambda: lp.get_cross_points_hor_lines(t, slope, a.dist))
    inv = t.max() - t
    nrm = prep.normalization_fft(inv, 5)
    den = lp.gaussian_filter(nrm, 3)
    angle = np.rad2deg(np.arctan(slope))
    first, last = lp._calc_index_range(height, width, angle, "vertical")
    indices = np.arange(first, last, 0.3 * a.dist)
    report("max - mat (device events)", events, lambda: t.max() - t)
    report("normalization_fft(mat, 5) (device events)", events, lambda: prep.normalization_fft(inv, 5))
    report("gaussian_filter(mat, 3) (device events)", events, lambda: lp.gaussian_filter(nrm, 3))
    report("get_tilted_profiles, %d profiles of %d (device events)" % (len(indices), height), events,
           lambda: lp.get_tilted_profiles(den, indices, angle, "vertical"))
    kernels = F.last_kernel()
    report("get_tilted_profiles, with its coordinates on the host (wall clock)", wall, lambda: lp.get_tilted_profiles(den, indices, angle, "vertical"))
    profiles = lp.get_tilted_profiles(den, indices, angle, "vertical")[2]
    rows = profiles.max(dim=1, keepdim=True).values - profiles                   # option="max"
    found = torch.empty(rows.shape, dtype=torch.float64, device=rows.device)
    stream = torch.cuda.current_stream().cuda_stream
    report("peak search, %d x %d device-resident rows, radius 11, sub-pixel (device events)" % tuple(rows.shape), events,
           lambda: F.check(F.lib().dcp_local_extrema_rows(rows.data_ptr(), found.data_ptr(), rows.shape[0], rows.shape[1], rows.shape[1],
                                                          F.DTYPE_BY_NAME["float64"], 11, 0.1, 1, F.MEM_DEVICE, -1, stream)))
    kernels += " | " + F.last_kernel()
    host_rows = profiles.cpu().numpy()
    report("get_local_extrema_points on host rows (wall clock)", wall,
           lambda: lp.get_local_extrema_points(host_rows, option="max", radius=11, denoise=False, norm=False))
    if not a.no_numpy:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "helpers"))
        import peaks_reference as PR
        flipped = np.max(host_rows, axis=1, keepdims=True) - host_rows
        t0 = time.perf_counter()
        restated = [PR.local_minima(row, 11, 0.1) for row in flipped]
        cpu_ms = (time.perf_counter() - t0) * 1e3
        got = lp.get_local_extrema_points(host_rows, option="max", radius=11, denoise=False, norm=False, subpixel=False)
        same = all(np.array_equal(g, r) for g, r in zip(got, restated))
        print("%-74s %9.1f ms (once; %d points, equal to the kernel's: %s)" % ("NumPy restatement of the peak search on this machine's CPU", cpu_ms,
                                                                               sum(len(r) for r in restated), same), flush=True)
    print("[%s]" % kernels, flush=True)


def radon_main(argv):
    ap = argparse.ArgumentParser(prog="time_gaussian.py --radon", description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--side", type=int, default=600)
    ap.add_argument("--angles", type=int, default=61)
    ap.add_argument("--dtypes", default="float32,float64")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args(argv)
    if a.rounds < 5:
        ap.error("--rounds must be at least 5")
    from discorpy_amd import _ffi as F
    from discorpy_amd.prep.linepattern import _make_circle_mask, _radon_table
    L = F.lib()
    F.require_device()
    dev, side, nang = -1, a.side, a.angles
    dptr = F.C.POINTER(F.C.c_double)
    rng = np.random.default_rng(11)
    half = (nang - 1) / 2.0
    sweeps = {"0": np.arange(-half, half + 1.0), "90": 90.0 + np.arange(-half, half + 1.0)}
    # a line-pattern-like ROI under the mask of the slope search: lines 30 apart, noise, zero outside the circle
    y, x = np.mgrid[0:side, 0:side]
    roi = (1.0 + np.cos(2 * np.pi * (x + 0.03 * y) / 30.0) + 0.05 * rng.standard_normal((side, side))) * _make_circle_mask(side, 0.92)
    print("radon: %d x %d plane, %d angles per call, %d rounds of %d calls, ms per call" % (side, side, nang, a.rounds, a.reps))
    for name in a.dtypes.split(","):
        dt = np.dtype(name)
        code = F.DTYPE_BY_NAME[dt.name]
        img = roi.astype(dt)
        src = F.DeviceBuffer(img.nbytes, dev).upload(img)
        dst = F.DeviceBuffer(side * nang * 8, dev)
        tables = {k: _radon_table(v, side) for k, v in sweeps.items()}
        floor_table = _radon_table(sweeps["0"], 1)

        def run(key):
            if key == "floor":
                F.check(L.dcp_radon_2d(src.ptr, dst.ptr, 1, 1, code, nang, floor_table.ctypes.data_as(dptr), F.MEM_DEVICE, dev, None))
            else:
                F.check(L.dcp_radon_2d(src.ptr, dst.ptr, side, side, code, nang, tables[key].ctypes.data_as(dptr), F.MEM_DEVICE, dev, None))

        def timed(key):
            e0, e1 = F.Event(dev), F.Event(dev)
            e0.record()
            for _r in range(a.reps):
                run(key)
            e1.record()
            e1.synchronize()
            return e0.elapsed_ms(e1) / a.reps
        same = {}
        for key in ("0", "90"):
            for _ in range(a.warmup):
                run(key)
            first = dst.download((side, nang), np.float64)
            run(key)
            same[key] = np.array_equal(first, dst.download((side, nang), np.float64), equal_nan=True)
        for _ in range(a.warmup):
            run("floor")
        kernel = F.last_kernel()
        F.check(L.dcp_stream_synchronize(dev, None))
        rounds = {"0": [], "90": [], "floor": []}
        for _ in range(a.rounds):
            for key in ("0", "90", "floor"):
                rounds[key].append(timed(key))
        med = {k: float(np.median(v)) for k, v in rounds.items()}
        for key in ("0", "90"):
            print("%-8s around %2s degree  %8.4f ms (rounds %.4f .. %.4f)  less the floor %8.4f ms  two calls equal: %s" % (
                dt.name, key, med[key], min(rounds[key]), max(rounds[key]), med[key] - med["floor"], same[key]), flush=True)
        print("%-8s floor of a call    %8.4f ms (rounds %.4f .. %.4f)  [1 x 1 plane, %d angles: the table's copy, the wait for it, one launch]" % (
            dt.name, med["floor"], min(rounds["floor"]), max(rounds["floor"]), nang))
        print("%-8s ratio 90 / 0       %8.3f of the calls, %.3f less the floor  [%s]" % (
            dt.name, med["90"] / med["0"], (med["90"] - med["floor"]) / (med["0"] - med["floor"]), kernel), flush=True)
    return 0


def select_peaks_main(argv):
    ap = argparse.ArgumentParser(prog="time_gaussian.py --select-peaks", description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--peaks", type=int, default=4096)
    ap.add_argument("--radius", type=int, default=11)
    ap.add_argument("--length", type=int, default=2000)
    ap.add_argument("--dtypes", default="float32,float64")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args(argv)
    if a.rounds < 5:
        ap.error("--rounds must be at least 5")
    from discorpy_amd import _ffi as F
    L = F.lib()
    F.require_device()
    dev, length, radius = -1, a.length, a.radius
    i32p = F.C.POINTER(F.C.c_int32)
    rng = np.random.default_rng(12)
    # profiles of a line pattern as the cross-point route hands them on: lines 90 apart, of width 4, on a sloping background, with noise;
    # three candidates in four on a line's centre, the fourth half-way between two lines (a false peak)
    per_row = (length - 90) // 90
    nrows = -(-a.peaks // per_row)
    x = np.arange(length, dtype=np.float64)
    rows = np.empty((nrows, length))
    peak_row, peak_idx = [], []
    for r in range(nrows):
        centres = 45.0 + 90.0 * np.arange(per_row) + rng.uniform(-3.0, 3.0, per_row)
        rows[r] = 0.2 + 1e-4 * x + np.exp(-0.5 * ((x[:, None] - centres[None, :]) / 4.0) ** 2).sum(axis=1) + 0.02 * rng.standard_normal(length)
        at = np.round(centres).astype(np.int32)
        at[3::4] += 45
        peak_row.append(np.full(per_row, r, np.int32))
        peak_idx.append(np.clip(at, 0, length - 1))
    peak_row, peak_idx = np.concatenate(peak_row)[:a.peaks], np.concatenate(peak_idx)[:a.peaks]
    npeaks = len(peak_idx)
    print("select_good_peaks: %d candidates at radius %d on %d x %d device-resident profiles, %d rounds of %d calls, ms per call" % (
        npeaks, radius, nrows, length, a.rounds, a.reps))
    for name in a.dtypes.split(","):
        dt = np.dtype(name)
        code = F.DTYPE_BY_NAME[dt.name]
        src = F.DeviceBuffer(nrows * length * dt.itemsize, dev).upload(rows.astype(dt))
        keep, fit = F.DeviceBuffer(npeaks, dev), F.DeviceBuffer(npeaks * 48, dev)

        def run(count):
            F.check(L.dcp_select_peaks_rows(src.ptr, nrows, length, length, code, peak_row.ctypes.data_as(i32p), peak_idx.ctypes.data_as(i32p), count,
                                            radius, 0.2, 1, keep.ptr, fit.ptr, F.MEM_DEVICE, dev, None))

        def timed(count):
            e0, e1 = F.Event(dev), F.Event(dev)
            e0.record()
            for _r in range(a.reps):
                run(count)
            e1.record()
            e1.synchronize()
            return e0.elapsed_ms(e1) / a.reps
        for _ in range(a.warmup):
            run(npeaks)
        first = fit.download((npeaks, 6), np.float64)
        run(npeaks)
        again = fit.download((npeaks, 6), np.float64)
        kept = keep.download((npeaks,), np.uint8)
        kernel = F.last_kernel()
        for _ in range(a.warmup):
            run(1)
        F.check(L.dcp_stream_synchronize(dev, None))
        rounds = {npeaks: [], 1: []}
        for _ in range(a.rounds):
            for count in (npeaks, 1):
                rounds[count].append(timed(count))
        med = {k: float(np.median(v)) for k, v in rounds.items()}
        status = first[:, 5].astype(np.int64)
        print("%-8s %d candidates    %8.4f ms (rounds %.4f .. %.4f)  less the floor %8.4f ms  kept %d, status counts %s, two calls equal: %s" % (
            dt.name, npeaks, med[npeaks], min(rounds[npeaks]), max(rounds[npeaks]), med[npeaks] - med[1], int(kept.sum()),
            np.bincount(status, minlength=7).tolist(), np.array_equal(first, again, equal_nan=True)), flush=True)
        print("%-8s floor of a call    %8.4f ms (rounds %.4f .. %.4f)  [one candidate: the tables' copy, the wait for it, one launch]  [%s]" % (
            dt.name, med[1], min(rounds[1]), max(rounds[1]), kernel), flush=True)
    return 0


def select_wired_main(argv):
    ap = argparse.ArgumentParser(prog="time_gaussian.py --select-peaks --wired", description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nrows", type=int, default=300)
    ap.add_argument("--radius", type=int, default=11)
    ap.add_argument("--length", type=int, default=2000)
    ap.add_argument("--dtypes", default="float32,float64")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-image", action="store_true")
    a = ap.parse_args(argv)
    if a.rounds < 5:
        ap.error("--rounds must be at least 5")
    import bench
    from discorpy_amd import _ffi as F
    L = F.lib()
    F.require_device()
    dev, nrows, length, radius = -1, a.nrows, a.length, a.radius
    i32p = F.C.POINTER(F.C.c_int32)
    rng = np.random.default_rng(13)
    per_row = (length - 90) // 90
    x = np.arange(length, dtype=np.float64)
    lines = np.empty((nrows, length))
    for r in range(nrows):
        centres = 45.0 + 90.0 * np.arange(per_row) + rng.uniform(-3.0, 3.0, per_row)
        lines[r] = 0.2 + 1e-4 * x + np.exp(-0.5 * ((x[:, None] - centres[None, :]) / 4.0) ** 2).sum(axis=1) + 0.02 * rng.standard_normal(length)
    print("peak search with select_peaks=True: %d x %d device-resident profiles at radius %d, %d rounds of %d runs, ms per run" % (
        nrows, length, radius, a.rounds, a.reps))
    for name in a.dtypes.split(","):
        dt = np.dtype(name)
        code = F.DTYPE_BY_NAME[dt.name]
        rows = lines.astype(dt)
        rows = np.ascontiguousarray(rows.max(axis=1, keepdims=True) - rows)          # option="max": the lines are minima
        plane = np.ascontiguousarray(rows.max(axis=1, keepdims=True) - rows)
        sens = float(dt.type(0.1))
        src = F.DeviceBuffer(rows.nbytes, dev).upload(rows)
        sel = F.DeviceBuffer(plane.nbytes, dev).upload(plane)
        table, dst = F.DeviceBuffer(nrows * length * 8, dev), F.DeviceBuffer(nrows * length * 8, dev)
        keep_dev = F.DeviceBuffer(nrows * length, dev)
        rows64 = rows.astype(np.float64)

        def one_call():
            F.check(L.dcp_extrema_select_rows(src.ptr, dst.ptr, nrows, length, length, code, radius, sens, 1, None, length, 0.2, 1, None, None,
                                              F.MEM_DEVICE, dev, None))

        def composed():
            F.check(L.dcp_local_extrema_rows(src.ptr, table.ptr, nrows, length, length, code, radius, sens, 0, F.MEM_DEVICE, dev, None))
            found = table.download((nrows, length), np.float64)
            counts = found[:, -1].astype(np.int64)
            peak_row = np.repeat(np.arange(nrows, dtype=np.int32), counts)
            peak_idx = found[np.arange(length)[None, :] < counts[:, None]].astype(np.int32)
            n = len(peak_idx)
            F.check(L.dcp_select_peaks_rows(sel.ptr, nrows, length, length, code, peak_row.ctypes.data_as(i32p), peak_idx.ctypes.data_as(i32p), n, radius,
                                            0.2, 1, keep_dev.ptr, None, F.MEM_DEVICE, dev, None))
            good = keep_dev.download((n,), np.uint8) != 0
            r, p = peak_row[good].astype(np.int64), peak_idx[good].astype(np.int64)
            d0, d1, d2 = rows64[r, p - 1], rows64[r, p], rows64[r, p + 1]
            qa, qb = (d0 - 2.0 * d1 + d2) / 2.0, (-3.0 * d0 + 4.0 * d1 - d2) / 2.0
            off = np.where(d1 < d0, np.where(d2 < d1, 2.0, 1.0), np.where(d2 < d0, 2.0, 0.0))
            with np.errstate(all="ignore"):
                num = -qb / (2.0 * qa)
            off = np.where((qa != 0.0) & (num >= 0.0) & (num < 3.0), num, off)
            return r, (p - 1).astype(np.float64) + off, n

        def timed(route):
            e0, e1 = F.Event(dev), F.Event(dev)
            e0.record()
            for _r in range(a.reps):
                route()
            e1.record()
            e1.synchronize()
            return e0.elapsed_ms(e1) / a.reps
        for _ in range(a.warmup):
            one_call()
            composed()
        one_call()
        kernel = F.last_kernel()
        F.check(L.dcp_stream_synchronize(dev, None))
        got = dst.download((nrows, length), np.float64)
        r, pos, ncand = composed()
        kept = got[:, -1].astype(np.int64)
        equal = int(kept.sum()) == len(pos) and np.array_equal(got[np.arange(length)[None, :] < kept[:, None]], pos) and \
            np.array_equal(np.repeat(np.arange(nrows), kept), r)
        rounds = {"one": [], "composed": []}
        for _ in range(a.rounds):
            rounds["one"].append(timed(one_call))
            rounds["composed"].append(timed(composed))
        med = {k: float(np.median(v)) for k, v in rounds.items()}
        spread = max(rounds["composed"]) - min(rounds["composed"])
        print("%-8s one call          %8.4f ms (rounds %.4f .. %.4f)  [%s]" % (dt.name, med["one"], min(rounds["one"]), max(rounds["one"]), kernel))
        print("%-8s composition       %8.4f ms (rounds %.4f .. %.4f)  spread %.4f ms; %d candidates, %d kept, positions equal: %s" % (
            dt.name, med["composed"], min(rounds["composed"]), max(rounds["composed"]), spread, ncand, len(pos), equal))
        print("%-8s the bar (one call <= composition + its spread): %s  (%.4f against %.4f ms, ratio %.3f)" % (
            dt.name, "met" if med["one"] <= med["composed"] + spread else "MISSED", med["one"], med["composed"] + spread, med["one"] / med["composed"]), flush=True)
        clk = bench.clocks_under_load(one_call, lambda: F.check(L.dcp_stream_synchronize(dev, None)))
        print("%-8s clock under the one call: %s" % (dt.name, clk), flush=True)
    if a.no_image:
        return 0
    # the whole route on an image: 1800 x 2000, lines 90 apart, flag on against flag off
    from discorpy_amd.prep import linecomplete as lc
    h, w, dist = 1800, 2000, 90.0
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    t = np.deg2rad(1.5)
    u, v = xx * np.cos(t) + yy * np.sin(t) + 7.3, -xx * np.sin(t) + yy * np.cos(t) + 11.9
    du, dv = (u + dist / 2) % dist - dist / 2, (v + dist / 2) % dist - dist / 2
    img = (1.0 - 0.8 * np.maximum(np.exp(-du * du / 32.0), np.exp(-dv * dv / 32.0))) * (0.75 + 0.2 * xx / w + 0.1 * yy / h)
    img = (img * (1.0 + 0.01 * rng.standard_normal((h, w)))).astype(np.float32)
    slope = float(np.tan(t))
    for flag in (False, True, False, True):
        lc.get_cross_points_hor_lines(img, slope, dist, select_peaks=flag)
    walls = {False: [], True: []}
    for _ in range(a.rounds):
        for flag in (False, True):
            t0 = time.perf_counter()
            lc.get_cross_points_hor_lines(img, slope, dist, select_peaks=flag)
            walls[flag].append((time.perf_counter() - t0) * 1e3)
    for flag in (False, True):
        print("get_cross_points_hor_lines 1800 x 2000 select_peaks=%-5s %8.2f ms wall (rounds %.2f .. %.2f), %d points" % (
            flag, float(np.median(walls[flag])), min(walls[flag]), max(walls[flag]),
            len(lc.get_cross_points_hor_lines(img, slope, dist, select_peaks=flag))), flush=True)
    return 0


if __name__ == "__main__":
    main()
