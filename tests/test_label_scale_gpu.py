"""GPU suite for labelling, hole filling, clear_border and the measurements at the sizes where the loops of csrc/label_kernels.hip turn
that one 3 x 4-tile frame never turns (tests/test_label_gpu.py covers the tile's own edges).  Every comparison is np.array_equal with
scipy.ndimage, as there: labels are integers and the measurements are quotients of exact integer sums.

LARGE (tests/helpers/label_cases.py; its conditions are asserted against the kernels' constants by tests/test_label_cpu.py) has 621
blocks of root counts, so label_scan_kernel walks three rounds of 256: the sums of the waves before a lane's own and the carry from one
round to the next decide scipy's number of every component behind the first 64 and the first 256 blocks.  Its 35 x 18 tiles give the
seam kernel some 380 workgroups that race on one parent plane.  MEDIUM (6 x 5 tiles) carries the patterns with image-long chains under
both values of "x_label_lds"; at LARGE the every-pair union runs noise and the checkerboard only.  The measurements take int8 weights
(kWI8), sums at the largest magnitude of either sign, and label and weight planes whose row strides differ from the width and from each
other."""
import functools
import os
import sys

import numpy as np
import pytest
from scipy import ndimage as ndi

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import binarize_reference as bref  # noqa: E402
import label_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu

TH, TW, BIG, MEDIUM, LARGE = cases.TH, cases.TW, cases.BIG, cases.MEDIUM, cases.LARGE
CHAINS = ("serpentine", "comb", "comb_transposed", "double_spiral", "diagonals")
NOISE = ("random_0.3", "random_0.55", "random_0.6", "checkerboard")
FILLS = ("rings", "nested_rings", "open_ring", "diagonal_gap", "random_0.55", "random_0.8")


@pytest.fixture(scope="module")
def prep(hip):
    from discorpy_amd.prep import preprocessing
    return preprocessing


def _set(hip, value):
    old = hip.get_option("x_label_lds")
    hip.set_option("x_label_lds", value)
    return old


@pytest.fixture(params=[1, 0], ids=["lds", "global"])
def lds(request, hip):
    old = _set(hip, request.param)
    try:
        yield request.param
    finally:
        hip.set_option("x_label_lds", old)


@pytest.fixture
def tiles(hip):
    """x_label_lds = 1, whatever the process was left with."""
    old = _set(hip, 1)
    try:
        yield 1
    finally:
        hip.set_option("x_label_lds", old)


@pytest.fixture
def pairs(hip):
    old = _set(hip, 0)
    try:
        yield 0
    finally:
        hip.set_option("x_label_lds", old)


def check_labels(prep, name, shape, conn):
    want, want_num = cases.expected_labels(name, shape, conn)
    got, num = prep.label(cases.pattern(name, shape), cases.STRUCTURES[conn])
    assert got.dtype == np.int32 and got.shape == shape
    assert num == want_num, (name, conn, num, want_num)
    assert np.array_equal(got, want), (name, conn, int((got != want).sum()), np.argwhere(got != want)[:1].tolist())


# ---------------------------------------------------------------------------------------------- label

@pytest.mark.parametrize("name", NOISE + CHAINS)
def test_labels_of_a_large_frame(prep, hip, tiles, name):
    for conn in (4, 8):
        check_labels(prep, name, LARGE, conn)
        assert hip.last_kernel().startswith("label_tile_kernel<bits=8, tile=%dx%d, conn=%d> + label_merge_kernel<seams> + " % (TW, TH, conn))
    if name == "random_0.3":
        assert cases.expected_labels(name, LARGE, 4)[1] > 250000          # roots in every block of the scan
    if name == "checkerboard":
        n = LARGE[0] * LARGE[1]
        assert cases.expected_labels(name, LARGE, 4)[1] == (n + 1) // 2 and cases.expected_labels(name, LARGE, 8)[1] == 1
    if name == "random_0.6":
        lab, num = cases.expected_labels(name, LARGE, 8)
        assert num > 500 and np.bincount(lab.ravel())[1:].max() > 0.5 * lab.size          # one component through every tile


@pytest.mark.parametrize("name", ["random_0.3", "random_0.55", "checkerboard"])
def test_labels_of_a_large_frame_by_the_union_over_every_pair(prep, hip, pairs, name):
    for conn in (4, 8):
        check_labels(prep, name, LARGE, conn)
        assert hip.last_kernel().startswith("label_init_kernel<bits=8> + label_merge_kernel<every pair, conn=%d> + " % conn)


@pytest.mark.parametrize("name", CHAINS)
def test_long_chains_across_six_by_five_tiles(prep, lds, name):
    for conn in (4, 8):
        check_labels(prep, name, MEDIUM, conn)


# ---------------------------------------------------------------------------------------------- hole filling, clear_border

@pytest.mark.parametrize("name", FILLS)
def test_fill_holes_of_a_large_frame(prep, tiles, name):
    got = prep.binary_fill_holes(cases.hole_pattern(name, LARGE))
    want = cases.expected_filled(name, LARGE)
    assert got.dtype == np.bool_ and np.array_equal(got, want), (name, int((got != want).sum()))


def test_fill_holes_across_six_by_five_tiles(prep, lds):
    for name in FILLS:
        got = prep.binary_fill_holes(cases.hole_pattern(name, MEDIUM))
        assert np.array_equal(got, cases.expected_filled(name, MEDIUM)), name


def inner_blocks(h, w):
    """4 x 4 blocks on every corner where four tiles meet.  The first row is set, and in every second tile column a line runs from it
    down through that column's blocks: those touch the border, the others do not."""
    m = cases.zeros(h, w)
    for y in range(TH, h - 2, TH):
        for x in range(TW, w - 2, TW):
            m[y - 2:y + 2, x - 2:x + 2] = 1
    m[0] = 1
    m[:h - 3, 2 * TW::2 * TW] = 1
    return m


BORDER_PLANES = ("random_0.3", "nested_rings", "comb", "inner_blocks")


@functools.lru_cache(maxsize=None)
def border_plane(name, shape):
    if name == "inner_blocks":
        m = inner_blocks(*shape)
    elif name in cases.HOLE_PATTERNS and name not in cases.PATTERNS:
        m = cases.hole_pattern(name, shape)
    else:
        m = cases.pattern(name, shape)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def expected_cleared(name, shape, conn, invert):
    return bref.clear_border(border_plane(name, shape), conn, invert)


def check_clear_border(prep, name, shape):
    m = border_plane(name, shape)
    for conn in (4, 8):
        for invert in (False, True):
            got = prep._clear_border_plane(prep._rows_image(m), invert=invert, conn=conn)
            want = expected_cleared(name, shape, conn, invert)
            assert got.dtype == np.uint8 and np.array_equal(got, want), (name, conn, invert, int((got != want).sum()))
    if name == "comb":
        assert not expected_cleared(name, shape, 4, False).any() and border_plane(name, shape).any()          # everything touches the border
    if name == "inner_blocks":
        kept = expected_cleared(name, shape, 4, False)
        assert kept[TH, TW] == 1 and kept[TH, 2 * TW] == 0 and 0 < kept.sum() < m.sum()


@pytest.mark.parametrize("name", BORDER_PLANES)
def test_clear_border_of_a_large_frame(prep, hip, tiles, name):
    check_clear_border(prep, name, LARGE)
    assert hip.last_kernel().startswith("label_tile_kernel") and hip.last_kernel().endswith("clear_border_kernel")


def test_clear_border_across_six_by_five_tiles(prep, lds):
    for name in BORDER_PLANES:
        check_clear_border(prep, name, MEDIUM)


# ---------------------------------------------------------------------------------------------- measurements

def weights(dtype, shape, seed):
    """Values over the whole range of the type, zero included."""
    rng = np.random.default_rng(seed)
    info = np.iinfo(dtype)
    a = rng.integers(info.min, info.max, size=shape, endpoint=True).astype(dtype)
    a[rng.random(shape) < 0.1] = 0
    return a


def check_measures(prep, mat, labels, index):
    with np.errstate(all="ignore"):
        want_sum, got_sum = ndi.sum_labels(mat, labels, index), prep.sum_labels(mat, labels, index)
        want_com, got_com = ndi.center_of_mass(mat, labels, index), prep.center_of_mass(mat, labels, index)
    assert np.shape(got_sum) == np.shape(want_sum) and np.array_equal(got_sum, want_sum)
    assert type(got_com) is type(want_com) and np.shape(got_com) == np.shape(want_com)
    assert np.array_equal(np.asarray(got_com, np.float64), np.asarray(want_com, np.float64), equal_nan=True)


@functools.lru_cache(maxsize=None)
def expected_objects(name, conn):
    return ndi.find_objects(cases.expected_labels(name, LARGE, conn)[0])


@pytest.mark.parametrize("dtype", ["int8", "uint16"])
@pytest.mark.parametrize("name,conn", [("random_0.3", 4), ("random_0.6", 8)])
def test_measures_of_a_large_frame_equal_scipys(prep, name, conn, dtype):
    labels, num = cases.expected_labels(name, LARGE, conn)
    mat = weights(dtype, LARGE, 510)
    assert mat.min() == np.iinfo(dtype).min and mat.max() == np.iinfo(dtype).max
    index = np.arange(1, num + 1)
    got = prep.sum_labels(mat, labels, index)
    assert np.array_equal(got, ndi.sum_labels(mat, labels, index))
    drawn = np.random.default_rng(520).choice(index, size=min(2000, num), replace=False)
    check_measures(prep, mat, labels, [1] + [int(v) for v in drawn] + [num])
    assert prep.find_objects(labels) == expected_objects(name, conn)


@pytest.mark.parametrize("dtype,value", [("uint16", 65535), ("int16", -32768), ("int8", -128)])
def test_one_component_that_spans_a_large_frame(prep, dtype, value):
    """The largest sums of either sign the types reach; n * max(H, W) * 65535 < 2^53 keeps scipy's float64 sums exact."""
    labels = np.ones(LARGE, np.int32)
    full = np.full(LARGE, value, dtype)
    n, (h, w) = LARGE[0] * LARGE[1], LARGE
    assert ndi.sum_labels(full, labels, 1) == float(n * value)
    for index in (1, [1, 2]):
        check_measures(prep, full, labels, index)
    assert prep.center_of_mass(full, labels, 1) == ((h - 1) / 2, (w - 1) / 2)
    assert prep.find_objects(labels) == [(slice(0, h, None), slice(0, w, None))]


# ---------------------------------------------------------------------------------------------- row-strided planes

def reference_table(mat, labels, num):
    """The (num, 4) int64 sums and int32 boxes of dcp_label_measures_2d from NumPy (every sum below 2^53: exact in bincount's float64)."""
    lab = np.where((labels >= 1) & (labels <= num), labels, 0).ravel()
    y, x = np.mgrid[0:labels.shape[0], 0:labels.shape[1]]
    v = mat.astype(np.float64).ravel()
    sums = np.stack([np.bincount(lab, minlength=num + 1), np.bincount(lab, v, num + 1), np.bincount(lab, v * y.ravel(), num + 1),
                     np.bincount(lab, v * x.ravel(), num + 1)], axis=1)[1:]
    assert np.abs(sums).max() < 2**53
    boxes = np.array([(labels.shape[0], -1, labels.shape[1], -1) if s is None else (s[0].start, s[0].stop - 1, s[1].start, s[1].stop - 1)
                      for s in ndi.find_objects(labels, num)], np.int32).reshape(num, 4)
    return sums.astype(np.int64), boxes


@pytest.mark.parametrize("dtype,fill", [("uint8", 255), ("int16", 32767)])
def test_label_and_weight_planes_with_row_strides_of_their_own(prep, hip, dtype, fill):
    """Column slices of two wider planes with different paddings: w_stride != l_stride != W.  The padding holds label 1 and the type's
    greatest weight, so a kernel that took either stride for the width would sum them in."""
    import torch
    h, w = BIG
    labels, num = cases.expected_labels("random_0.55", BIG, 4)
    mat = weights(dtype, BIG, 530)
    lbase = np.ascontiguousarray(np.pad(labels.astype(np.int32), ((0, 0), (3, 7)), constant_values=1))
    wbase = np.ascontiguousarray(np.pad(mat, ((0, 0), (13, 4)), constant_values=fill))
    lview, wview = lbase[:, 3:-7], wbase[:, 13:-4]
    assert np.array_equal(lview, labels) and np.array_equal(wview, mat) and not lview.flags.c_contiguous and not wview.flags.c_contiguous
    index = np.arange(1, num + 1)
    want_sums, want_boxes = reference_table(mat, labels, num)
    assert np.array_equal(want_sums[:, 1].astype(np.float64), ndi.sum_labels(mat, labels, index))
    # device tensors, through the Python layer
    lt, wt = torch.from_numpy(lbase).to("cuda:0")[:, 3:-7], torch.from_numpy(wbase).to("cuda:0")[:, 13:-4]
    assert lt.stride(0) == w + 10 and wt.stride(0) == w + 17 and not lt.is_contiguous() and not wt.is_contiguous()
    assert np.array_equal(prep.sum_labels(wt, lt, index), ndi.sum_labels(mat, labels, index))
    picked = [1, num, 2, num // 2, num + 1]
    with np.errstate(all="ignore"):
        want_com = ndi.center_of_mass(mat, labels, picked)
        assert np.array_equal(np.asarray(prep.center_of_mass(wt, lt, picked)), np.asarray(want_com), equal_nan=True)
    assert prep.find_objects(lt) == ndi.find_objects(labels)
    # the C ABI with device pointers and the two strides
    sums = torch.full((num, 4), -1, dtype=torch.int64, device="cuda:0")
    boxes = torch.full((num, 4), -1, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    code = hip.DTYPE_BY_NAME[dtype]
    hip.check(hip.lib().dcp_label_measures_2d(wt.data_ptr(), lt.data_ptr(), h, w, w + 17, w + 10, code, num, sums.data_ptr(), boxes.data_ptr(),
                                              hip.MEM_DEVICE, lt.device.index, None))
    torch.cuda.synchronize()
    assert np.array_equal(sums.cpu().numpy(), want_sums) and np.array_equal(boxes.cpu().numpy(), want_boxes)
    # host memory: the two pitches of the copies that pack the rows
    hsums, hboxes = np.full((num, 4), -1, np.int64), np.full((num, 4), -1, np.int32)
    hip.check(hip.lib().dcp_label_measures_2d(wview.ctypes.data, lview.ctypes.data, h, w, w + 17, w + 10, code, num, hsums.ctypes.data,
                                              hboxes.ctypes.data, hip.MEM_HOST, -1, None))
    assert np.array_equal(hsums, want_sums) and np.array_equal(hboxes, want_boxes)
    assert np.array_equal(prep.sum_labels(wview, lview, index), ndi.sum_labels(mat, labels, index))


# ---------------------------------------------------------------------------------------------- the bounds-checking build

def test_bounds_checking_build_counts_no_violation_at_scale(hip):
    """libdiscorpy_hip_bounds.so at LARGE under x_label_lds = 1 and at MEDIUM under 0: label, hole filling, clear_border (site 43, which
    the run of tests/test_label_gpu.py does not reach) and the measurements must count no violation."""
    import subprocess
    lib = os.path.join(ROOT, "discorpy_amd", "lib", "libdiscorpy_hip_bounds.so")
    assert os.path.exists(lib), "build() makes the bounds-checking library; it is missing"
    code = """
import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import label_cases as cases
import binarize_reference as bref
from scipy import ndimage as ndi
from discorpy_amd import _ffi as F
from discorpy_amd.prep import preprocessing as prep
F.require_device()
assert F.debug_bounds()[4] == 1
for value, shape in ((1, cases.LARGE), (0, cases.MEDIUM)):
    F.set_option("x_label_lds", value)
    m = cases.pattern("random_0.55", shape)
    want, want_num = cases.expected_labels("random_0.55", shape, 8)
    lab, num = prep.label(m, cases.BLOCK)
    assert num == want_num and np.array_equal(lab, want)
    assert np.array_equal(prep.binary_fill_holes(m), ndi.binary_fill_holes(m))
    assert np.array_equal(prep._clear_border_plane(prep._rows_image(m), conn=8), bref.clear_border(m))
    assert "clear_border_kernel" in F.last_kernel()
    index = np.arange(1, num + 1)
    assert np.array_equal(prep.sum_labels(m, lab, index), ndi.sum_labels(m, lab, index))
    assert prep.find_objects(lab, num + 3) == ndi.find_objects(lab, num + 3)
b = F.debug_bounds()
assert b[0] == 0 and b[4] == 1, b
print("bounds ok", b)
""" % (ROOT, os.path.join(ROOT, "tests", "helpers"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT, env=dict(os.environ, DCP_LIB_PATH=lib))
    assert r.returncode == 0 and "bounds ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
