"""Frames of dcp_unwarp_image_f32 captured into a HIP graph and replayed (tests/test_frame_plan_coverage.py starts this in a process
of its own, under a time limit; nothing here is retried).

The rule under test (csrc/frame_plan.cpp): while the calling stream is being captured the plan cache builds nothing, queries no
event and waits for none -- the call uses a plan the host already knows to be complete, or none -- and the memory of a replaced
plan outlives any graph that reads it.  One non-blocking stream, global capture mode (any forbidden runtime call of this thread
would invalidate the capture), a graph of one kernel node.

usage: capture_frames.py empty_cache | ready_plan_then_evicted | plan_just_built
Prints one JSON line; exit status 0 only if every check held.
"""
import ctypes as C
import json
import math
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from discorpy_amd import _ffi as hip  # noqa: E402
from oracle import oracle as orc  # noqa: E402

H, W = 1024, 1536
BASE = [1.0, -0.04, 0.03, -0.02, 0.012]
FACT = [BASE[k] / (math.hypot(H, W) / 2) ** k for k in range(5)]
XC, YC = W / 2 + 0.3, H / 2 - 0.4
FULL = 4 * ((W + 127) // 128) * ((H + 31) // 32)


def hip_runtime():
    """The HIP runtime libdiscorpy_hip.so is bound to: the one mapped into this process (never a second copy)."""
    hip.lib()
    with open("/proc/self/maps") as f:
        paths = {ln.split()[-1] for ln in f if "libamdhip64" in ln}
    assert len(paths) == 1, paths
    rt = C.CDLL(paths.pop())
    vp, sz = C.c_void_p, C.c_size_t
    for name, args in {"hipStreamBeginCapture": [vp, C.c_int], "hipStreamEndCapture": [vp, C.POINTER(vp)],
                       "hipGraphInstantiate": [C.POINTER(vp), vp, vp, vp, sz], "hipGraphLaunch": [vp, vp],
                       "hipGraphGetNodes": [vp, vp, C.POINTER(sz)], "hipGraphExecDestroy": [vp], "hipGraphDestroy": [vp],
                       "hipGraphDebugDotPrint": [vp, C.c_char_p, C.c_uint]}.items():
        fn = getattr(rt, name)
        fn.restype, fn.argtypes = C.c_int, args
    return rt


def ok(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed: hipError %d" % (what, rc))


def frame(src, dst, stream, xc=XC):
    fa, nf = hip.fact_array(FACT)
    hip.check(hip.lib().dcp_unwarp_image_f32(src.ptr, dst.ptr, H, W, W, 1, xc, YC, fa, nf, 1, 1, hip.BLEND_F64LERP, hip.MEM_DEVICE, -1,
                                             stream.ptr))


def capture(rt, src, dst, stream):
    """One frame call captured on `stream`: (executable graph, graph, number of nodes, the line of the graph's dump that names its kernel)."""
    graph, gexec, n = C.c_void_p(), C.c_void_p(), C.c_size_t(0)
    ok(rt.hipStreamBeginCapture(stream.ptr, 0), "hipStreamBeginCapture")                # hipStreamCaptureModeGlobal
    try:
        frame(src, dst, stream)
    finally:
        rc = rt.hipStreamEndCapture(stream.ptr, C.byref(graph))
    ok(rc, "hipStreamEndCapture")
    ok(rt.hipGraphGetNodes(graph, None, C.byref(n)), "hipGraphGetNodes")
    name = ""
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "graph.dot")
        if rt.hipGraphDebugDotPrint(graph, path.encode(), 0) == 0 and os.path.exists(path):
            with open(path, errors="replace") as f:
                hits = [ln.strip() for ln in f if "remap_wg_kernel" in ln]
            name = hits[0] if hits else ""
    ok(rt.hipGraphInstantiate(C.byref(gexec), graph, None, None, 0), "hipGraphInstantiate")
    return gexec, graph, int(n.value), name


def replay(rt, gexec, dst, stream, want):
    dst.upload(np.full((H, W), -1.0, np.float32))
    ok(rt.hipGraphLaunch(gexec, stream.ptr), "hipGraphLaunch")
    stream.synchronize()
    return bool(np.array_equal(dst.download((H, W), np.float32), want))


def is_planned(name):
    """Whether the kernel named in the graph's dump is the PLAN = true instantiation of remap_wg_kernel (its last template argument:
    Lb1 in the mangled name); None if the dump names no such kernel."""
    if "remap_wg_kernel" not in name:
        return None
    return "Lb1E" in name or "true>" in name


def main(scenario):
    rt = hip_runtime()
    hip.require_device()
    orc.build()
    img = np.random.default_rng(8500).random((H, W), dtype=np.float32)
    want = orc.unwarp_image_backward(img, XC, YC, FACT, poly=orc.POLY_KERNEL, blend=orc.BLEND_F64LERP)
    src = hip.DeviceBuffer(img.nbytes).upload(img)
    dst, other = hip.DeviceBuffer(img.nbytes), hip.DeviceBuffer(img.nbytes)
    stream = hip.Stream()
    hip.release_scratch()
    hip.set_option("x_frame_plan", 2)
    rep = {"scenario": scenario, "checks": {}}
    chk = rep["checks"]
    if scenario == "empty_cache":
        gexec, graph, n, name = capture(rt, src, dst, stream)
        chk["nothing_built_while_capturing"] = hip.get_option("x_frame_plan_tiles") == 0
        chk["one_node"] = n == 1
        chk["captured_unplanned"] = is_planned(name) is False
        chk["replay_equal"] = replay(rt, gexec, dst, stream, want)
        frame(src, other, stream)                                   # the same call outside a capture does build
        stream.synchronize()
        chk["built_outside_capture"] = hip.get_option("x_frame_plan_tiles") == FULL
        chk["replay_equal_again"] = replay(rt, gexec, dst, stream, want)
    elif scenario == "ready_plan_then_evicted":
        frame(src, other, stream)                                   # builds
        stream.synchronize()
        frame(src, other, stream)                                   # the host sees the build complete
        stream.synchronize()
        chk["built"] = hip.get_option("x_frame_plan_tiles") == FULL
        gexec, graph, n, name = capture(rt, src, dst, stream)
        chk["one_node"] = n == 1
        chk["captured_planned"] = is_planned(name) is True
        chk["replay_equal"] = replay(rt, gexec, dst, stream, want)
        for i in range(16):                                         # sixteen other calibrations: the captured plan is replaced
            frame(src, other, stream, xc=XC + 0.5 * (i + 1))
        stream.synchronize()
        chk["replay_equal_after_eviction"] = replay(rt, gexec, dst, stream, want)
    elif scenario == "plan_just_built":
        frame(src, other, stream)                                   # builds; the host has not seen the build complete
        gexec, graph, n, name = capture(rt, src, dst, stream)
        chk["one_node"] = n == 1
        chk["captured_unplanned"] = is_planned(name) is False
        chk["replay_equal"] = replay(rt, gexec, dst, stream, want)
        chk["first_frame_equal"] = bool(np.array_equal(other.download((H, W), np.float32), want))
    else:
        raise SystemExit("unknown scenario %r" % scenario)
    rep["captured_kernel"] = name
    ok(rt.hipGraphExecDestroy(gexec), "hipGraphExecDestroy")
    ok(rt.hipGraphDestroy(graph), "hipGraphDestroy")
    hip.release_scratch()
    rep["ok"] = all(chk.values())
    print(json.dumps(rep))
    return 0 if rep["ok"] else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else ""))
