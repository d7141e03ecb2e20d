"""The plane entry points (dcp_*_2d: median, Gaussian, labelling, measurements, hole filling, binarization) answer every refused argument
with the code and the message they answered it with before their argument checks were gathered in csrc/api_plane.cpp, character for
character: tests/golden/plane_refusals.json holds (code, dcp_last_error()) of every case of the tables of test_median_cpu.py,
test_gaussian_cpu.py, test_label_cpu.py and test_binarize_cpu.py (which match a fragment of the message only), recorded with the library
as it was by tools/gen_golden.py --plane-refusals.  The buffers are host memory and no case gets as far as a device call."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

from discorpy_amd import _ffi as F

with open(os.path.join(GOLDEN, "plane_refusals.json")) as _f:
    RECORD = json.load(_f)
CASES = RECORD["cases"]

H, W = 8, 10          # the valid frame of the recording: the source has room for rows W + 4 elements of 8 bytes apart
SRC = np.zeros(H * (W + 4) * 8, np.uint8)
DST = np.zeros(H * W * 8, np.uint8)
OUTPUTS = {"num": np.full(1, -7, np.int32), "sums": np.full((5, 4), -7, np.int64), "boxes": np.full((5, 4), -7, np.int32),
           "minmax": np.full(2, -7.0), "bad": np.full(1, -7, np.int64), "counts": np.full(8, -7, np.int64), "count": np.full(1, -7, np.int64)}
EDGES = np.linspace(0, 1, 9)
POINTERS = ("src", "dst", "weights", "labels", "wy", "wx", "edges", "stream") + tuple(OUTPUTS)


def address(value, keep):
    """The address a recorded pointer stands for (None: null); arrays made for the call are parked in `keep`."""
    if value == "null":
        return None
    if isinstance(value, (list, dict)):          # weights of the Gaussian
        keep.append(np.full(value["n"], value["repeat"]) if isinstance(value, dict) else np.array(value, np.float64))
        return keep[-1].ctypes.data
    if value == "edges":
        return EDGES.ctypes.data
    if value in OUTPUTS:
        return OUTPUTS[value].ctypes.data
    name, _, offset = value.partition("+")
    return {"src": SRC, "dst": DST}[name].ctypes.data + int(offset or 0)


def replay(case):
    entry = RECORD["entries"][case["entry"]]
    args, keep, out = dict(entry["valid"], **case["override"]), [], []
    for key, argtype in zip(entry["order"], F.SIGNATURES[case["entry"]][1]):
        value = args[key]
        if key in POINTERS:
            value = address(value, keep)
            if value is not None and argtype is not F.C.c_void_p:
                value = F.C.cast(F.C.c_void_p(value), argtype)
        out.append(value)
    return getattr(F.lib(), case["entry"])(*out), F.last_error()


def test_the_recording_is_whole():
    assert len(CASES) == 178 and len(RECORD["entries"]) == 11
    per_entry = {name: sum(c["entry"] == name for c in CASES) for name in RECORD["entries"]}
    assert per_entry == {"dcp_median_filter_2d": 18, "dcp_correlate_sym_2d": 20, "dcp_label_2d": 18, "dcp_fill_holes_2d": 14,
                         "dcp_label_measures_2d": 18, "dcp_abs_2d": 12, "dcp_minmax_2d": 17, "dcp_histogram_2d": 21, "dcp_threshold_2d": 12,
                         "dcp_clear_border_2d": 16, "dcp_morph_cross_2d": 12}
    assert all(c["code"] in (F.ERR_INVALID_ARG, F.ERR_UNSUPPORTED) and c["message"] for c in CASES)
    assert (H, W) == (RECORD["entries"]["dcp_abs_2d"]["valid"]["height"], RECORD["entries"]["dcp_abs_2d"]["valid"]["width"])


def test_checks_at_their_boundaries_are_clean_under_the_sanitizers(tmp_path):
    """tests/c/plane_checks.cpp: make_plane_call, the per-plane stride check and the measures' 2^47 bound at touching buffers, 2^31 - 1
    pixels and sides of 2^30 - 1, as a host program of its own built with -fsanitize=address,undefined (no device call, no Python)."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="")
    env.setdefault("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "c"), "plane_checks_asan", "OUT=%s" % tmp_path], check=True, env=env, capture_output=True)
    r = subprocess.run([str(tmp_path / "plane_checks_asan")], env=env, stdin=subprocess.DEVNULL, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "\n0 failure(s)" in r.stdout and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, (r.stdout, r.stderr)
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 24 + 1 and all(line.startswith("ok ") for line in lines[:-1]), r.stdout


@pytest.mark.parametrize("case", CASES, ids=["%s-%s" % (c["entry"][4:-3], "-".join("%s=%s" % (k, v if not isinstance(v, (list, dict)) else "x")
                                                                                  for k, v in c["override"].items())) for c in CASES])
def test_refusal_is_the_recorded_one(case):
    code, message = replay(case)
    assert (code, message) == (case["code"], case["message"])
    assert all((buf == -7).all() for buf in OUTPUTS.values()), "a refused call wrote to the caller's outputs"
    assert not SRC.any() and not DST.any()
