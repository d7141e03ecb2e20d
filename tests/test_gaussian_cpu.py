"""CPU suite for the Gaussian filter and the line-pattern module: dcp_correlate_sym_2d is exported, declared and bound; every argument
it refuses is refused with its code and a message that names the argument before any device work (the buffers are host memory, no GPU
is visible to these cases); the weights are scipy's; discorpy_amd.prep.linepattern raises for what it does not take; _calc_index_range
and the index errors of get_tilted_profile agree with a restatement of the reference (discorpy/prep/linepattern.py:452-544: its module
cannot be imported without scikit-image)."""
import inspect
import os
import re

import numpy as np
import pytest
from scipy import ndimage as ndi

from conftest import ROOT

from discorpy_amd import _ffi as F

SYMBOL = "dcp_correlate_sym_2d"
INV, UNS = F.ERR_INVALID_ARG, F.ERR_UNSUPPORTED
H, W = 8, 10
SRC = np.zeros(H * (W + 4) * 8, np.uint8)
DST = np.zeros(H * W * 8, np.uint8)
W3 = np.array([0.25, 0.5, 0.25])
W5 = np.array([0.1, 0.2, 0.4, 0.2, 0.1])
ASYM = np.array([0.25, 0.5, np.nextafter(0.25, 1.0)])
SIGNED_ZERO = np.array([0.0, 1.0, -0.0])
_dp = F.C.POINTER(F.C.c_double)


def ptr(w):
    return None if w is None else w.ctypes.data_as(_dp)


VALID = dict(src=SRC.ctypes.data, dst=DST.ctypes.data, height=H, width=W, stride=W, dtype=F.DTYPE_BY_NAME["uint16"], wy=W3, ry=1, wx=W5, rx=2,
             mode=0, cval=0.0, mem_kind=F.MEM_HOST, device=-1, stream=None)
ORDER = "src dst height width stride dtype wy ry wx rx mode cval mem_kind device stream".split()


def call(**override):
    args = dict(VALID, **override)
    args["wy"], args["wx"] = ptr(args["wy"]), ptr(args["wx"])
    return F.lib().dcp_correlate_sym_2d(*[args[k] for k in ORDER])


def test_symbol_is_exported_declared_and_bound():
    assert hasattr(F.lib(), SYMBOL)
    header = open(os.path.join(ROOT, "include", "discorpy_hip.h")).read()
    assert re.search(r"^int %s\(const void\* src, void\* dst, int height, int width, long src_row_stride, int dtype,$" % SYMBOL, header, re.M)
    exports = open(os.path.join(ROOT, "discorpy_amd", "csrc", "exports.map")).read()
    assert re.search(r"^\s*%s;" % SYMBOL, exports, re.M), "not named in csrc/exports.map"
    restype, argtypes = F.SIGNATURES[SYMBOL]
    assert restype is F.C.c_int and len(argtypes) == 15 and argtypes[4] is F.C.c_long and argtypes[11] is F.C.c_double


CASES = [
    (dict(wy=ASYM), INV, "weights_y are not symmetric"),
    (dict(wx=ASYM, rx=1), INV, "weights_x are not symmetric"),
    (dict(wy=SIGNED_ZERO), INV, "weights_y are not symmetric"),             # equal as numbers, not as bits
    (dict(dst=SRC.ctypes.data), INV, "overlap"),
    (dict(dst=SRC.ctypes.data + 2 * (H * W - 1)), INV, "overlap"),           # the last source element is the first of dst
    (dict(stride=W + 4, dst=SRC.ctypes.data + 2 * ((H - 1) * (W + 4) + W - 1)), INV, "overlap"),
    (dict(mode=8), INV, "boundary mode 8"),
    (dict(mode=-1), INV, "boundary mode -1"),
    (dict(height=0), INV, "height"),
    (dict(width=-1), INV, "width"),
    (dict(stride=W - 1), INV, "src_row_stride"),
    (dict(dtype=99), INV, "dtype"),
    (dict(dtype=F.DTYPE_BY_NAME["bool"]), UNS, "bool"),
    (dict(ry=-2), INV, "radius_y"),
    (dict(rx=-7), INV, "radius_x"),
    (dict(ry=193, wy=np.full(387, 1.0 / 387)), UNS, "radius_y / radius_x above 192"),
    (dict(mem_kind=7), INV, "mem_kind"),
    (dict(mem_kind=F.MEM_DEVICE_UNORDERED), INV, "mem_kind"),
    (dict(src=None), INV, "src"),
    (dict(dst=None), INV, "dst"),
]


@pytest.mark.parametrize("override,rc,fragment", CASES, ids=["-".join("%s=%s" % (k, v if k in ("height", "width", "stride", "dtype", "ry", "rx", "mode",
                                                                                                 "mem_kind") else "x")
                                                                       for k, v in sorted(c[0].items())) for c in CASES])
def test_refused_argument(override, rc, fragment):
    got = call(**override)
    assert (got, fragment in F.last_error()) == (rc, True), (got, F.last_error())


def test_buffers_that_touch_and_skipped_axes_pass_the_checks():
    """dst starting right behind the source's last element is legal, and so are a null weight pointer and a radius of -1 (the axis
    is skipped): the call gets past the argument checks (and, with no device here, fails in the device layer -- or succeeds where
    a GPU is visible)."""
    ok = (F.OK, F.ERR_HIP, F.ERR_NO_DEVICE)
    assert call(stride=W + 4, dst=SRC.ctypes.data + 2 * ((H - 1) * (W + 4) + W)) in ok, F.last_error()
    assert call(wy=None) in ok, F.last_error()
    assert call(wx=ASYM, rx=-1) in ok, F.last_error()            # weights of a skipped axis are not looked at


def test_lab_option_round_trips_under_its_prefixed_name_only():
    assert F.get_option("x_gauss_lds") == 1
    for value in (0, 2, 1):
        F.set_option("x_gauss_lds", value)
        assert F.get_option("x_gauss_lds") == value
    for value in (-1, 3):
        with pytest.raises(ValueError, match="gauss_lds must be 0, 1 or 2"):
            F.set_option("x_gauss_lds", value)
    with pytest.raises(ValueError, match="unknown option"):
        F.set_option("gauss_lds", 0)


def test_weights_are_scipys():
    from discorpy_amd.prep import linepattern as lp
    for sigma in (0.5, 1, 3, 5.3, 10, np.float32(2.7)):
        w = lp._gaussian_weights(sigma)
        r = len(w) // 2
        assert w.dtype == np.float64 and r == int(4.0 * float(sigma) + 0.5)
        assert w.tobytes() == w[::-1].tobytes()
        delta = np.zeros(4 * r + 1)
        delta[2 * r] = 1.0
        assert np.array_equal(ndi.gaussian_filter1d(delta, sigma)[r:3 * r + 1], w)
    assert len(lp._gaussian_weights(3, truncate=2.5)) == 2 * 8 + 1 and len(lp._gaussian_weights(3, radius=5)) == 11
    delta = np.zeros(41)
    delta[20] = 1.0
    assert np.array_equal(ndi.gaussian_filter1d(delta, 3, radius=5)[15:26], lp._gaussian_weights(3, radius=5))
    for bad in (-1, 2.5):
        with pytest.raises(ValueError, match="Radius must be a nonnegative integer"):
            lp._gaussian_weights(3, radius=bad)


def test_module_offers_the_reference_signatures():
    from discorpy_amd import prep
    from discorpy_amd.prep import linepattern as lp
    assert prep.linepattern is lp
    P = inspect.Parameter
    sig = inspect.signature(lp.convert_chessboard_to_linepattern)
    assert [(p.name, p.default) for p in sig.parameters.values()] == [("mat", P.empty), ("smooth", True), ("bgr", "bright"), ("sigma", 3)]
    assert list(inspect.signature(lp.get_tilted_profile).parameters) == ["mat", "index", "angle_deg", "direction"]
    assert list(inspect.signature(lp._calc_index_range).parameters) == ["height", "width", "angle_deg", "direction"]
    gsig = inspect.signature(lp.gaussian_filter)
    assert list(gsig.parameters)[:2] == ["mat", "sigma"]
    assert {k: (p.default, p.kind) for k, p in gsig.parameters.items() if k not in ("mat", "sigma")} == {
        "order": (0, P.KEYWORD_ONLY), "mode": ("reflect", P.KEYWORD_ONLY), "cval": (0.0, P.KEYWORD_ONLY), "truncate": (4.0, P.KEYWORD_ONLY),
        "radius": (None, P.KEYWORD_ONLY), "out": (None, P.KEYWORD_ONLY)}
    assert set(lp.__all__) == {"gaussian_filter", "convert_chessboard_to_linepattern", "get_tilted_profile"}
    for word in ("normalization_fft", "Radon", "get_local_extrema_points", "select_good_peaks", "get_cross_points_hor_lines", "Out of scope"):
        assert word in lp.__doc__, word


def test_refused_inputs_of_the_wrapper_need_no_device():
    from discorpy_amd.prep import linepattern as lp
    a = np.zeros((4, 4), np.float32)
    for dt in (np.complex64, np.complex128):
        with pytest.raises(TypeError, match="Complex type not supported"):
            lp.gaussian_filter(np.zeros((4, 4), dt), 3)
    for dt in (np.float16, np.bool_):
        with pytest.raises(RuntimeError, match="data type not supported"):
            lp.gaussian_filter(np.zeros((4, 4), dt), 3)
    for order in (1, 2, (0, 1)):
        with pytest.raises(NotImplementedError, match="order"):
            lp.gaussian_filter(a, 3, order=order)
    with pytest.raises(RuntimeError, match="boundary mode not supported"):
        lp.gaussian_filter(a, 3, mode="periodic")
    with pytest.raises(ValueError, match="2-D"):
        lp.gaussian_filter(np.zeros((2, 3, 4), np.float32), 3)
    with pytest.raises(RuntimeError, match="sequence argument must have length equal to input rank"):
        lp.gaussian_filter(a, (3, 3, 3))
    with pytest.raises(ValueError, match="Radius must be a nonnegative integer"):
        lp.gaussian_filter(a, 3, radius=-1)


def reference_index_range(height, width, angle_deg, direction):
    """discorpy/prep/linepattern.py:475-509 restated: (min_idx, max_idx), or the text of the ValueError."""
    t = np.tan(np.abs(angle_deg * np.pi / 180.0))
    if np.abs(angle_deg) == 90.0:
        return "around 90-degree"
    if direction == "horizontal":
        lo, hi = (int(np.ceil(width * np.tan(angle_deg * np.pi / 180.0))), height - 1) if angle_deg > 0 else (0, height - 1 - int(np.floor(width * t)))
        return (lo, hi) if 0 <= lo < height and 0 <= hi < height else "Row index is out of range, please select the direction correctly !!!"
    lo, hi = (0, width - 1 - int(np.ceil(height * np.tan(angle_deg * np.pi / 180.0)))) if angle_deg > 0 else (int(np.floor(height * t)), width - 1)
    return (lo, hi) if 0 <= lo < width and 0 <= hi < width else "Column index is out of range, please select the direction correctly !!!"


@pytest.mark.parametrize("direction", ["horizontal", "vertical"])
def test_index_range_follows_the_reference(direction):
    from discorpy_amd.prep import linepattern as lp
    for height, width in ((96, 120), (120, 96), (7, 300), (300, 7), (1, 1)):
        for angle in (0.0, 3.0, -3.0, 0.5, -0.5, 44.0, -44.0, 60.0, -60.0, 89.0, 90.0, -90.0, 12):
            want = reference_index_range(height, width, angle, direction)
            if isinstance(want, str):
                with pytest.raises(ValueError) as err:
                    lp._calc_index_range(height, width, angle, direction)
                assert want in str(err.value), (height, width, angle, str(err.value))
                if abs(angle) == 90.0:
                    assert ("use the '%s' option" % ("vertical" if direction == "horizontal" else "horizontal")) in str(err.value)
            else:
                assert lp._calc_index_range(height, width, angle, direction) == want, (height, width, angle)


def test_tilted_profile_refuses_bad_indices_before_any_device_work():
    from discorpy_amd.prep import linepattern as lp
    a = np.zeros((96, 120), np.float32)
    with pytest.raises(ValueError, match="Input must be a 2D array !!!"):
        lp.get_tilted_profile(np.zeros((3, 4, 5), np.float32), 0, 0.0, "horizontal")
    lo, hi = reference_index_range(96, 120, 3.0, "horizontal")
    assert (lo, hi) == (7, 95)
    for index in (lo - 1, hi + 1):
        with pytest.raises(ValueError, match=re.escape("Input index is out of possible range: [7, 95]")):
            lp.get_tilted_profile(a, index, 3.0, "horizontal")
    lo, hi = reference_index_range(96, 120, -3.0, "vertical")
    for index in (lo - 1, hi + 1):
        with pytest.raises(ValueError, match=re.escape("Input index is out of possible range: [%d, %d]" % (lo, hi))):
            lp.get_tilted_profile(a, index, -3.0, "vertical")
    with pytest.raises(ValueError, match="around 90-degree"):
        lp.get_tilted_profile(a, 5, 90.0, "vertical")
