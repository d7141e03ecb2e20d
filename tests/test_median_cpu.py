"""CPU suite for the median filter: dcp_median_filter_2d is exported, declared and bound; every argument it refuses is refused with
its code and a message that names the argument before any device work (the buffers are host memory, no GPU is visible to these
cases); discorpy_amd.prep.preprocessing offers the reference's normalization with the reference's signature and raises for the element
types it does not take."""
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT

from discorpy_amd import _ffi as F

SYMBOL = "dcp_median_filter_2d"
INV, UNS = F.ERR_INVALID_ARG, F.ERR_UNSUPPORTED
H, W = 8, 10
SRC = np.zeros(H * (W + 4) * 8, np.uint8)
DST = np.zeros(H * W * 8, np.uint8)
VALID = dict(src=SRC.ctypes.data, dst=DST.ctypes.data, height=H, width=W, stride=W, dtype=F.DTYPE_BY_NAME["uint16"], size_y=3, size_x=3,
             mem_kind=F.MEM_HOST, device=-1, stream=None)
ORDER = "src dst height width stride dtype size_y size_x mem_kind device stream".split()


def call(**override):
    args = dict(VALID, **override)
    return F.lib().dcp_median_filter_2d(*[args[k] for k in ORDER])


def test_symbol_is_exported_declared_and_bound():
    assert hasattr(F.lib(), SYMBOL)
    header = open(os.path.join(ROOT, "include", "discorpy_hip.h")).read()
    assert re.search(r"^int %s\(const void\* src, void\* dst, int height, int width, long src_row_stride" % SYMBOL, header, re.M)
    exports = open(os.path.join(ROOT, "discorpy_amd", "csrc", "exports.map")).read()
    assert re.search(r"^\s*%s;" % SYMBOL, exports, re.M), "not named in csrc/exports.map"
    restype, argtypes = F.SIGNATURES[SYMBOL]
    assert restype is F.C.c_int and len(argtypes) == 11 and argtypes[4] is F.C.c_long


CASES = [
    (dict(size_y=0), INV, "size_y"),
    (dict(size_x=0), INV, "size_x"),
    (dict(size_y=-3), INV, "size_y"),
    (dict(height=0), INV, "height"),
    (dict(width=0), INV, "width"),
    (dict(height=-1), INV, "height"),
    (dict(stride=W - 1), INV, "src_row_stride"),
    (dict(dtype=99), INV, "dtype"),
    (dict(dtype=-1), INV, "dtype"),
    (dict(mem_kind=7), INV, "mem_kind"),
    (dict(mem_kind=F.MEM_DEVICE_UNORDERED), INV, "mem_kind"),
    (dict(dst=SRC.ctypes.data), INV, "overlap"),
    (dict(dst=SRC.ctypes.data + 2 * (H * W - 1)), INV, "overlap"),           # the last source element is the first of dst
    (dict(stride=W + 4, dst=SRC.ctypes.data + 2 * ((H - 1) * (W + 4) + W - 1)), INV, "overlap"),
    (dict(size_y=65536, size_x=32768), UNS, "size_y * size_x"),
    (dict(size_y=2147483647, size_x=2), UNS, "size_y * size_x"),
    (dict(src=None), INV, "src"),
    (dict(dst=None), INV, "dst"),
]


@pytest.mark.parametrize("override,rc,fragment", CASES, ids=["-".join("%s=%s" % (k, v if k not in ("src", "dst") else "x")
                                                                       for k, v in sorted(c[0].items())) for c in CASES])
def test_refused_argument(override, rc, fragment):
    got = call(**override)
    assert (got, fragment in F.last_error()) == (rc, True), (got, F.last_error())


def test_buffers_that_touch_but_do_not_overlap_pass_the_checks():
    """dst starting right behind the source's last element is legal: the call gets past the argument checks (and, with no device
    here, fails in the device layer -- or succeeds where a GPU is visible)."""
    got = call(stride=W + 4, dst=SRC.ctypes.data + 2 * ((H - 1) * (W + 4) + W))
    assert got in (F.OK, F.ERR_HIP, F.ERR_NO_DEVICE), (got, F.last_error())


def test_lab_option_round_trips_under_its_prefixed_name_only():
    assert F.get_option("x_median_lds") == 1
    F.set_option("x_median_lds", 0)
    assert F.get_option("x_median_lds") == 0
    F.set_option("x_median_lds", 1)
    with pytest.raises(ValueError, match="unknown option"):
        F.set_option("median_lds", 0)


def test_module_offers_the_reference_signature():
    from discorpy_amd.prep import preprocessing as prep
    sig = inspect.signature(prep.normalization)
    assert [(p.name, p.default, p.kind) for p in sig.parameters.values()] == [
        ("mat", inspect.Parameter.empty, inspect.Parameter.POSITIONAL_OR_KEYWORD), ("size", 51, inspect.Parameter.POSITIONAL_OR_KEYWORD)]
    msig = inspect.signature(prep.median_filter)
    assert list(msig.parameters) == ["mat", "size", "out"] and msig.parameters["out"].kind == inspect.Parameter.KEYWORD_ONLY
    assert set(prep.__all__) == {"normalization", "median_filter"}
    assert "scikit-image" in prep.__doc__ and "out of scope" in prep.__doc__


@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
def test_complex_input_raises_scipys_error(dt):
    from discorpy_amd.prep import preprocessing as prep
    with pytest.raises(TypeError, match="Complex type not supported"):
        prep.median_filter(np.zeros((4, 4), dt), 3)
    with pytest.raises(TypeError, match="Complex type not supported"):
        prep.normalization(np.zeros((4, 4), dt))


def test_float16_raises_as_elsewhere_in_the_package():
    from discorpy_amd.prep import preprocessing as prep
    with pytest.raises(RuntimeError, match="data type not supported"):
        prep.median_filter(np.zeros((4, 4), np.float16), 3)
    with pytest.raises(RuntimeError, match="data type not supported"):
        prep.normalization(np.zeros((4, 4), np.float16), 3)


def test_shape_and_size_errors_need_no_device():
    from discorpy_amd.prep import preprocessing as prep
    with pytest.raises(ValueError, match="2-D"):
        prep.median_filter(np.zeros((2, 3, 4), np.float32), 3)
    with pytest.raises(RuntimeError, match="sequence argument must have length equal to input rank"):
        prep.median_filter(np.zeros((4, 4), np.float32), (3, 3, 3))
    with pytest.raises(TypeError):
        prep.median_filter(np.zeros((4, 4), np.float32), 2.5)
