"""CPU suite for the Radon transform and the slope and distance search of discorpy_amd.prep.linepattern (radon,
calc_slope_distance_hor_lines / calc_slope_distance_ver_lines, _make_circle_mask; dcp_radon_2d): the names, signatures and defaults are
the reference's; the entry point is exported, declared and bound and refuses what it does not take before any device work; the
wrappers raise for what they do not take before they ask for a device (this machine has none: reaching the device would raise something
else); the NumPy restatement of the transform's definition (tests/helpers/radon_reference.py, the oracle of tests/test_radon_gpu.py) is
held to facts checked by hand; and golden G28 (tools/gen_golden.py) loads with every case off a tie.

Two of the facts hold under the definition only at multiples of 90 degree, where the rotation permutes the samples; at other angles the
bilinear weights of a rotated lattice do not sum to one.  A single 1 at the centre gives ``1 + 2 (1 - |sin a|)(1 - |cos a|)`` at row c0
(the samples one row above and below the centre still touch it: 1.1716 at 45 degree), which is asserted as that closed form; the total
mass of a disc varies with the angle by a few 1e-3 of itself (printed), and is equal to 1e-12 relative at 0, 90, 180 and 270 degree."""
import inspect
import json
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT, golden

from discorpy_amd import _ffi as F

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import radon_reference as RR  # noqa: E402

INV, UNS = F.ERR_INVALID_ARG, F.ERR_UNSUPPORTED
P = inspect.Parameter


@pytest.fixture(scope="module")
def lp():
    from discorpy_amd.prep import linepattern
    return linepattern


def test_names_and_signatures_are_the_references(lp):
    assert set(lp.__all__) == {"gaussian_filter", "convert_chessboard_to_linepattern", "get_tilted_profile"}
    assert lp.RADON == ["radon", "calc_slope_distance_hor_lines", "calc_slope_distance_ver_lines"]
    for name in lp.RADON + ["_make_circle_mask"]:
        assert callable(getattr(lp, name)), name

    def params(fn):
        return [(p.name, p.default, p.kind) for p in inspect.signature(fn).parameters.values()]
    K, V = P.POSITIONAL_OR_KEYWORD, P.VAR_KEYWORD
    assert params(lp.radon) == [("image", P.empty, K), ("theta", None, K), ("circle", True, K)]
    assert params(lp._make_circle_mask) == [("width", P.empty, K), ("ratio", P.empty, K)]
    for fn in (lp.calc_slope_distance_hor_lines, lp.calc_slope_distance_ver_lines):
        assert params(fn) == [("mat", P.empty, K), ("ratio", 0.3, K), ("search_range", 30.0, K), ("radius", 9, K), ("sensitive", 0.1, K),
                              ("bgr", "bright", K), ("denoise", True, K), ("norm", True, K), ("subpixel", True, K), ("chessboard", False, K),
                              ("select_peaks", False, K), ("kwargs", P.empty, V)]


def test_docstrings_say_what_is_here_and_what_is_not(lp):
    from discorpy_amd.prep import preprocessing as prep
    out = lp.__doc__.split("Out of scope")[1].split("\n\n")[0]
    assert "Radon" in out and "peak search" in out and "normalization_fft" not in out
    for word in ("select_good_peaks", "select_peaks=True", "circle=False"):
        assert word in out, word
    assert "calc_slope_distance_hor_lines" not in out
    for word in ("UNVERIFIED", "RADON", "dcp_radon_2d", "calc_slope_distance_ver_lines"):
        assert word in lp.__doc__, word
    assert "UNVERIFIED" in lp.radon.__doc__ and "float64" in lp.radon.__doc__ and "float32" in lp.radon.__doc__
    assert "Radon-based angle search" in prep.__doc__
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "Radon transform" in design and "UNVERIFIED" in design.split("Radon transform")[1]


def test_symbol_is_exported_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "discorpy_hip.h")).read()
    exports = open(os.path.join(ROOT, "discorpy_amd", "csrc", "exports.map")).read()
    makefile = open(os.path.join(ROOT, "discorpy_amd", "csrc", "Makefile")).read()
    assert hasattr(F.lib(), "dcp_radon_2d")
    assert re.search(r"^int dcp_radon_2d\(const void\* src, double\* dst, int side, ", header, re.M)
    assert re.search(r"^\s*dcp_radon_2d;", exports, re.M)
    assert "radon_kernels.o" in makefile and "api_radon.o" in makefile
    restype, argtypes = F.SIGNATURES["dcp_radon_2d"]
    assert restype is F.C.c_int and len(argtypes) == 10


SIDE, NANG = 12, 3
SRC = np.zeros((SIDE, SIDE), np.float32)
SENTINEL = 0xA5
OUT = np.full(SIDE * NANG * 8, SENTINEL, np.uint8)
TABLE = RR.angle_table([0.0, 45.0, 90.0], SIDE)
F32, F64, U16 = (F.DTYPE_BY_NAME[n] for n in ("float32", "float64", "uint16"))
_dp = F.C.POINTER(F.C.c_double)


def bad_table(value):
    t = TABLE.copy()
    t[1, 2] = value
    return t


def radon_abi(**o):
    a = dict(src=SRC.ctypes.data, dst=OUT.ctypes.data, side=SIDE, stride=SIDE, dtype=F32, nangles=NANG, table=TABLE, mem_kind=F.MEM_HOST,
             device=-1, stream=None)
    a.update(o)
    a["table"] = None if a["table"] is None else a["table"].ctypes.data_as(_dp)
    return F.lib().dcp_radon_2d(*a.values())


REFUSALS = [
    (dict(src=None), INV, "null src / dst"),
    (dict(dst=None), INV, "null dst / table pointer"),
    (dict(table=None), INV, "null dst / table pointer"),
    (dict(side=0), INV, "height and width must be at least 1"),
    (dict(side=-3), INV, "height and width must be at least 1"),
    (dict(nangles=0), INV, "nangles must be at least 1"),
    (dict(nangles=-1), INV, "nangles must be at least 1"),
    (dict(side=32769, stride=32769), UNS, "side above 32768"),
    (dict(nangles=65536), UNS, "more than 65535 angles"),
    (dict(stride=SIDE - 1), INV, "src_row_stride 11 is below the width 12"),
    (dict(dtype=U16), UNS, "float32 or float64"),
    (dict(dtype=F.DTYPE_BY_NAME["bool"]), UNS, "float32 or float64"),
    (dict(dtype=99), INV, "unknown dtype 99"),
    (dict(mem_kind=7), INV, "mem_kind"),
    (dict(dst=SRC.ctypes.data + 8), INV, "src and dst overlap"),
    (dict(dst=SRC.ctypes.data - 8), INV, "src and dst overlap"),
    (dict(table=bad_table(np.nan)), INV, "table entry 6 (angle 1) is not finite"),
    (dict(table=bad_table(np.inf)), INV, "table entry 6 (angle 1) is not finite"),
    (dict(table=bad_table(-np.inf)), INV, "table entry 6 (angle 1) is not finite"),
]


@pytest.mark.parametrize("override,code,fragment", REFUSALS, ids=["-".join("%s" % k for k in c[0]) + "-%d" % i for i, c in enumerate(REFUSALS)])
def test_entry_point_refuses_before_any_device_work(override, code, fragment):
    OUT[:] = SENTINEL
    assert radon_abi(**override) == code
    assert fragment in F.last_error(), F.last_error()
    assert (OUT == SENTINEL).all()


def test_wrappers_refuse_before_any_device_work(lp):
    img = np.zeros((40, 60), np.float32)
    with pytest.raises(NotImplementedError, match="circle=False"):
        lp.radon(img, circle=False)
    with pytest.raises(TypeError, match="Complex type not supported"):
        lp.radon(img.astype(np.complex64))
    for dt in (np.uint8, np.int16, np.int64, np.bool_):
        with pytest.raises(NotImplementedError, match="float32 and float64 only"):
            lp.radon(img.astype(dt))
    with pytest.raises(RuntimeError, match="data type not supported"):
        lp.radon(img.astype(np.float16))
    for bad in (np.zeros(7, np.float32), np.zeros((2, 3, 4), np.float32)):
        with pytest.raises(ValueError, match="must be 2-D"):
            lp.radon(bad)
    with pytest.raises(ValueError, match="must not be empty"):
        lp.radon(np.zeros((0, 5), np.float32))
    with pytest.raises(ValueError, match="1D sequence"):
        lp.radon(img, theta=np.zeros((2, 2)))
    with pytest.raises(ValueError, match="theta must be finite"):
        lp.radon(img, theta=[0.0, np.nan])
    with pytest.raises(NotImplementedError, match="more than 65535 angles"):
        lp.radon(img, theta=np.zeros(65536))
    empty = lp.radon(img, theta=[])                           # no angle: nothing for a device to do
    assert isinstance(empty, np.ndarray) and empty.shape == (40, 0) and empty.dtype == np.float64
    for fn in (lp.calc_slope_distance_hor_lines, lp.calc_slope_distance_ver_lines):
        with pytest.raises(NotImplementedError, match="select_peaks"):
            fn(img, select_peaks=True)
        with pytest.raises(TypeError, match="Complex type not supported"):
            fn(img.astype(np.complex128))
        with pytest.raises(ValueError, match="Input must be a 2D array"):
            fn(np.zeros(9, np.float32))


def test_angle_table_is_the_restatements(lp):
    for side in (1, 2, 5, 64, 257):
        for theta in (np.arange(180), 90.0 + np.arange(-5.0, 6.0), np.arange(-1.0, 1.05, 0.05), [359.95, -30.0]):
            got = lp._radon_table(theta, side)
            assert got.dtype == np.float64 and got.flags.c_contiguous and np.array_equal(got, RR.angle_table(theta, side))
    t = RR.angle_table([0.0], 10)[0]
    assert tuple(t) == (1.0, 0.0, 0.0, 0.0)                   # angle 0 is the identity


def test_circle_mask_is_the_references(lp):
    mask = lp._make_circle_mask(9, 0.92)
    assert mask.dtype == np.float32 and mask.shape == (9, 9)
    y, x = np.mgrid[-4:5, -4:5]
    assert np.array_equal(mask, (x * x + y * y <= (0.92 * 4) ** 2).astype(np.float32))
    assert lp._make_circle_mask(8, 1.0)[0, 4] == 1.0 and lp._make_circle_mask(8, 1.0)[0, 3] == 0.0


def test_crop_rule_of_the_helper():
    a = np.arange(7 * 10).reshape(7, 10)
    assert np.array_equal(RR.crop_square(a), a[:, 2:9])      # excess 3: starts at ceil(1.5) = 2
    assert np.array_equal(RR.crop_square(a[:, :9]), a[:, 1:8])
    assert np.array_equal(RR.crop_square(a.T), a.T[2:9, :])
    assert RR.crop_square(a).base is not None


@pytest.mark.parametrize("side", [1, 2, 9, 64, 65])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_helper_angle_zero_is_the_column_sum(side, dtype):
    rng = np.random.default_rng(side)
    c0 = side // 2
    y, x = np.mgrid[:side, :side]
    inside = (y - c0) ** 2 + (x - c0) ** 2 <= c0 ** 2
    img = (rng.integers(-9, 10, (side, side)) * inside).astype(dtype)
    got = RR.radon(img, [0])
    assert got.shape == (side, 1) and got.dtype == np.float64
    assert np.array_equal(got[:, 0], img.astype(np.float64).sum(0))
    outside = img.copy()
    outside[~inside] = np.nan                                # what lies outside the circle is never read
    assert np.array_equal(RR.radon(outside, [0]), got)


def test_helper_point_at_the_centre():
    theta = np.array([0.0, 90.0, 180.0, 270.0, 45.0, -30.0, 359.95, 17.3, 123.4])
    a = np.deg2rad(theta)
    for side in (33, 64):
        c0 = side // 2
        img = np.zeros((side, side))
        img[c0, c0] = 1.0
        sino = RR.radon(img, theta)
        want = 1.0 + 2.0 * (1.0 - np.abs(np.sin(a))) * (1.0 - np.abs(np.cos(a)))
        print("row c0 of a centred point:", sino[c0])
        assert (np.argmax(sino, axis=0) == c0).all()
        assert np.abs(sino[c0] - want).max() <= 1e-12
        assert np.abs(sino[c0, :4] - 1.0).max() <= 1e-12     # 1 where the rotation permutes the samples


def test_helper_total_mass_of_a_disc():
    side = 65
    y, x = np.mgrid[:side, :side]
    disc = ((y - 30.3) ** 2 + (x - 34.1) ** 2 <= 10 ** 2).astype(np.float64)
    axis = RR.radon(disc, [0.0, 90.0, 180.0, 270.0]).sum(0)
    assert np.abs(axis - disc.sum()).max() <= 1e-12 * disc.sum()
    other = RR.radon(disc, np.arange(0.0, 180.0, 7.3)).sum(0)
    # (a figure, not a bound: at these angles the weights of the rotated lattice do not sum to one -- module docstring)
    print("total mass of a disc over the angles: spread %.3g of the mean" % ((other.max() - other.min()) / other.mean()))
    assert np.isfinite(other).all() and (other > 0).all()


def test_g28_loads_and_sits_on_no_tie():
    g = golden("g28_slope_distance")
    names = [str(n) for n in g["case_names"]]
    assert len(names) >= 10 and {"line_hor", "line_ver", "big_ver", "chess_hor", "dark_ver", "float64_hor", "plain_ver"} <= set(names)
    for key in ("line", "big", "chess"):
        assert g["img_" + key].dtype == np.float32
    assert g["img_line"].shape == (160, 200) and g["img_big"].shape == (400, 420)
    for name in names:
        kw = json.loads(str(g["args_" + name]))
        assert {"ratio", "search_range", "radius"} <= set(kw)
        gap1, gap2, e_dist = float(g["gap1_" + name]), float(g["gap2_" + name]), float(g["e_dist_" + name])
        print("%-12s slope %+.7f distance %.4f gaps %.3g %.3g e_dist %.3g" % (name, g["slope_" + name], g["dist_" + name], gap1, gap2, e_dist))
        assert gap1 > 1e-9 and gap2 > 1e-9, name
        assert 0 <= e_dist < 1e-9 and np.isfinite(g["dist_" + name]) and abs(g["slope_" + name]) < 0.2
        if kw.get("subpixel", True) is False:
            assert e_dist == 0
    assert abs(g["slope_line_hor"] - 0.0261859) < 1e-7 and abs(g["slope_line_ver"] + 0.0261859) < 1e-7
    assert abs(g["slope_big_ver"] + 0.0559087) < 1e-7 and abs(g["dist_big_ver"] - 29.8) < 0.1 and abs(g["dist_line_hor"] - 20.1) < 0.1
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g28_slope_distance.npz")) <= 1 << 20
