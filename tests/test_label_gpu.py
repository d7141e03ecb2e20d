"""GPU suite for labelling, dot measurements and hole filling (discorpy_amd.prep.preprocessing; csrc/label_kernels.hip).  Every comparison
is np.array_equal with scipy.ndimage: labels are integers, the measurements are quotients of exact integer sums, so there is no rounding
to allow for.

The shapes come from the kernels' tile (tests/helpers/label_cases.py, pinned to dcp_internal.h by tests/test_label_cpu.py): one pixel, a
row and a column across three tiles, one tile, one pixel more each way, 3 x 4 ragged tiles.  Every pattern runs at both connectivities
and under "x_label_lds" 1 (a tile per workgroup in LDS, then the seams) and 0 (the global union over every pixel pair)."""
import os
import sys

import numpy as np
import pytest
from scipy import ndimage as ndi

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import dots_reference as dref  # noqa: E402
import label_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu

TH, TW, BIG = cases.TH, cases.TW, cases.BIG


@pytest.fixture(scope="module")
def prep(hip):
    from discorpy_amd.prep import preprocessing
    return preprocessing


@pytest.fixture(params=[1, 0], ids=["lds", "global"])
def lds(request, hip):
    """x_label_lds for the test, restored afterwards."""
    old = hip.get_option("x_label_lds")
    hip.set_option("x_label_lds", request.param)
    try:
        yield request.param
    finally:
        hip.set_option("x_label_lds", old)


def _id(shape):
    return "%dx%d" % shape


# ---------------------------------------------------------------------------------------------- label

@pytest.mark.parametrize("shape", cases.SHAPES, ids=_id)
def test_patterns(prep, lds, shape):
    for name in cases.PATTERNS:
        for conn in (4, 8):
            want, want_num = cases.expected_labels(name, shape, conn)
            got, num = prep.label(cases.pattern(name, shape), cases.STRUCTURES[conn])
            assert got.dtype == np.int32 and got.shape == shape and isinstance(num, int)
            assert num == want_num, (name, conn, num, want_num)
            assert np.array_equal(got, want), (name, conn, int((got != want).sum()))


def test_structure_none_is_the_cross(prep):
    m = cases.pattern("random_0.55", (TH + 1, TW + 1))
    got, num = prep.label(m)
    want, want_num = cases.expected_labels("random_0.55", (TH + 1, TW + 1), 4)
    assert num == want_num and np.array_equal(got, want)


@pytest.mark.parametrize("dtype", cases.REAL_DTYPES)
def test_every_real_element_type(prep, lds, dtype):
    a = cases.typed_image(dtype, (TH + 1, TW + 1), 77)
    for conn in (4, 8):
        want, want_num = ndi.label(a, cases.STRUCTURES[conn])
        got, num = prep.label(a, cases.STRUCTURES[conn])
        assert num == want_num and np.array_equal(got, want), (dtype, conn, num, want_num)


def test_row_strided_view_is_read_in_place(prep, hip, lds):
    base = np.ascontiguousarray(np.pad(cases.pattern("random_0.6", BIG), ((0, 0), (3, 7)), constant_values=1))
    view = base[:, 3:-7]
    assert not view.flags.c_contiguous
    want, want_num = cases.expected_labels("random_0.6", BIG, 8)
    got, num = prep.label(view, cases.BLOCK)
    assert num == want_num and np.array_equal(got, want)
    # the same through the C ABI with the view's own stride: nothing was copied on the way
    out = np.empty(BIG, np.int32)
    n = hip.C.c_int(0)
    hip.check(hip.lib().dcp_label_2d(view.ctypes.data, out.ctypes.data, BIG[0], BIG[1], base.shape[1], hip.DTYPE_BY_NAME["uint8"], 8, hip.C.byref(n),
                                     hip.MEM_HOST, -1, None))
    assert n.value == want_num and np.array_equal(out, want)
    assert np.array_equal(prep.binary_fill_holes(view), ndi.binary_fill_holes(view))


def test_torch_tensor_on_a_stream_of_its_own(prep, lds):
    torch = pytest.importorskip("torch")
    m = cases.pattern("random_0.55", BIG)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        t = torch.from_numpy(m.copy()).to("cuda:0")
        labels, num = prep.label(t)
        view_labels, view_num = prep.label(t[:, 5:-9].to(torch.float32)[:, 2:], cases.BLOCK)          # a row-strided tensor view, in place
        filled = prep.binary_fill_holes(t)
        sums = prep.sum_labels(t, labels, np.arange(1, num + 1))
        cents = prep.center_of_mass(t, labels, [3, 1, 2])
        boxes = prep.find_objects(labels)
    stream.synchronize()
    want, want_num = cases.expected_labels("random_0.55", BIG, 4)
    assert isinstance(labels, torch.Tensor) and labels.dtype == torch.int32 and labels.device == t.device
    assert num == want_num and np.array_equal(labels.cpu().numpy(), want)
    vwant, vnum = ndi.label(m[:, 7:-9], cases.BLOCK)
    assert view_num == vnum and np.array_equal(view_labels.cpu().numpy(), vwant)
    assert filled.dtype == torch.bool and np.array_equal(filled.cpu().numpy(), ndi.binary_fill_holes(m))
    assert np.array_equal(sums, ndi.sum_labels(m, want, np.arange(1, num + 1)))
    assert cents == ndi.center_of_mass(m, want, [3, 1, 2])
    assert boxes == ndi.find_objects(want)


class Wrapped:
    """Nothing but __cuda_array_interface__ (what CuPy or Numba would hand over)."""

    def __init__(self, dev):
        self.dev = dev
        self.__cuda_array_interface__ = dev.__cuda_array_interface__


def test_cuda_array_interface_array(prep, hip, lds):
    m = cases.pattern("random_0.6", (TH + 1, TW + 1))
    dev = Wrapped(hip.DeviceArray(m.shape, np.uint8).copy_from_host(m))
    labels, num = prep.label(dev, cases.BLOCK)
    want, want_num = cases.expected_labels("random_0.6", m.shape, 8)
    assert isinstance(labels, hip.DeviceArray) and labels.dtype == np.int32
    assert num == want_num and np.array_equal(labels.copy_to_host(), want)
    filled = prep.binary_fill_holes(dev)
    assert isinstance(filled, hip.DeviceArray) and filled.dtype == np.bool_
    assert np.array_equal(filled.copy_to_host(), ndi.binary_fill_holes(m))
    index = np.arange(1, num + 1)
    assert np.array_equal(prep.sum_labels(dev, labels, index), ndi.sum_labels(m, want, index))
    assert prep.find_objects(labels, num) == ndi.find_objects(want)


def test_kernels_launched_under_each_option_value(prep, hip):
    """Stage 1 (label_tile_kernel) runs only under x_label_lds = 1; under 0 every pixel starts as its own root and the merge kernel walks
    every pair."""
    m = cases.pattern("random_0.55", BIG)
    old = hip.get_option("x_label_lds")
    seen = {}
    try:
        for value in (1, 0):
            hip.set_option("x_label_lds", value)
            prep.label(m, cases.BLOCK)
            seen[value, "label"] = hip.last_kernel()
            prep.binary_fill_holes(m)
            seen[value, "fill"] = hip.last_kernel()
    finally:
        hip.set_option("x_label_lds", old)
    print("kernel names observed by test_label_gpu.py:")
    for key in sorted(seen):
        print("   ", key, seen[key])
    rest = " + label_flatten_kernel + label_count/scan/rank_kernel + label_relabel_kernel"
    assert seen[1, "label"] == "label_tile_kernel<bits=8, tile=%dx%d, conn=8> + label_merge_kernel<seams>" % (TW, TH) + rest
    assert seen[0, "label"] == "label_init_kernel<bits=8> + label_merge_kernel<every pair, conn=8>" + rest
    assert seen[1, "fill"].startswith("label_tile_kernel<bits=8, tile=%dx%d, conn=4>" % (TW, TH)) and seen[1, "fill"].endswith("fill_holes_kernel")
    assert seen[0, "fill"].startswith("label_init_kernel<bits=8> + label_merge_kernel<every pair, conn=4>")
    assert all(("label_tile_kernel" in name) == (value == 1) for (value, _), name in seen.items())
    # a frame of one tile has no seam to sew
    prep.label(cases.pattern("ones", (TH, TW)))
    assert "label_merge_kernel" not in hip.last_kernel() and hip.last_kernel().startswith("label_tile_kernel")


# ---------------------------------------------------------------------------------------------- measurements

def weights(dtype, shape, seed):
    """Values over the whole range of the type (negative ones for int8 and int16), zero included."""
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype)
    if dt.kind == "b":
        return rng.random(shape) < 0.7
    info = np.iinfo(dt)
    a = rng.integers(info.min, info.max, size=shape, endpoint=True).astype(dt)
    a[rng.random(shape) < 0.1] = 0
    return a


def check_measures(prep, mat, labels, index):
    with np.errstate(all="ignore"):
        want_sum, got_sum = ndi.sum_labels(mat, labels, index), prep.sum_labels(mat, labels, index)
        want_com, got_com = ndi.center_of_mass(mat, labels, index), prep.center_of_mass(mat, labels, index)
    assert np.shape(got_sum) == np.shape(want_sum) and np.array_equal(got_sum, want_sum)
    assert type(got_com) is type(want_com) and np.shape(got_com) == np.shape(want_com)
    assert np.array_equal(np.asarray(got_com, np.float64), np.asarray(want_com, np.float64), equal_nan=True)
    if isinstance(want_com, list) and want_com:
        assert type(got_com[0]) is tuple and len(got_com[0]) == 2


@pytest.mark.parametrize("dtype", ["bool", "uint8", "int8", "int16", "uint16"])
def test_measures_equal_scipys(prep, dtype):
    for k, density in enumerate(cases.DENSITIES):
        name = "random_%g" % density
        labels, num = cases.expected_labels(name, BIG, 4 if k % 2 else 8)
        mat = weights(dtype, BIG, 500 + k)
        rng = np.random.default_rng(600 + k)
        shuffled = [int(v) for v in rng.permutation(np.arange(1, num + 1))]
        for index in (np.arange(1, num + 1), shuffled, 1, num, np.int64(max(num // 2, 1)), [num, 1, 1], [2, num + 3, 1], num + 1,
                      np.array([[1, 2], [num, num + 7]])):
            check_measures(prep, mat, labels, index)
        assert prep.find_objects(labels) == ndi.find_objects(labels)
        assert prep.find_objects(labels, num + 2) == ndi.find_objects(labels, num + 2)
        assert prep.find_objects(labels, max(num - 1, 1)) == ndi.find_objects(labels, max(num - 1, 1))


@pytest.mark.parametrize("dtype", ["bool", "uint8", "int8", "int16", "uint16"])
def test_one_component_that_spans_the_image(prep, dtype):
    labels = np.ones(BIG, np.int32)
    mat = weights(dtype, BIG, 700)
    for index in (1, [1], [1, 2]):
        check_measures(prep, mat, labels, index)
    assert prep.find_objects(labels) == [(slice(0, BIG[0], None), slice(0, BIG[1], None))] == ndi.find_objects(labels)
    if dtype == "uint16":
        full = np.full(BIG, 65535, np.uint16)          # the largest sums the type can reach on this frame
        check_measures(prep, full, labels, 1)


def test_label_plane_with_gaps_in_its_numbering(prep):
    base, num = cases.expected_labels("random_0.3", BIG, 4)
    labels = np.where(base % 5 == 2, 0, base * 3).astype(np.int32)          # only multiples of 3, and some of those missing
    labels[0, :4] = (-4, 0, 2147483647, -2147483648)
    mat = weights("uint8", BIG, 800)
    top = 3 * num
    for index in (np.arange(1, top + 1), [3, 6, 7, 9, top, top + 1], 6, 7):
        check_measures(prep, mat, labels, index)
    assert prep.find_objects(labels, top) == ndi.find_objects(labels, top)
    as64 = labels.astype(np.int64)
    as64[0, :4] = 0
    assert np.array_equal(prep.sum_labels(mat, as64, [3, 6, 9]), ndi.sum_labels(mat, as64, [3, 6, 9]))


def test_index_none_takes_every_labelled_pixel(prep):
    labels, num = cases.expected_labels("random_0.55", BIG, 4)
    mat = weights("uint16", BIG, 900)
    assert prep.sum_labels(mat, labels) == ndi.sum_labels(mat, labels)
    assert prep.center_of_mass(mat, labels) == ndi.center_of_mass(mat, labels)


# ---------------------------------------------------------------------------------------------- hole filling

@pytest.mark.parametrize("shape", cases.SHAPES, ids=_id)
def test_fill_holes_patterns(prep, lds, shape):
    for name in cases.HOLE_PATTERNS:
        got = prep.binary_fill_holes(cases.hole_pattern(name, shape))
        assert got.dtype == np.bool_ and got.shape == shape
        assert np.array_equal(got, cases.expected_filled(name, shape)), (name, int((got != cases.expected_filled(name, shape)).sum()))
    for name in ("zeros", "ones", "checkerboard", "serpentine", "double_spiral", "comb"):
        m = cases.pattern(name, shape)
        assert np.array_equal(prep.binary_fill_holes(m), ndi.binary_fill_holes(m)), name


@pytest.mark.parametrize("dtype", cases.REAL_DTYPES)
def test_fill_holes_of_every_real_element_type(prep, dtype):
    a = cases.typed_image(dtype, (TH + 1, TW + 1), 78)
    assert np.array_equal(prep.binary_fill_holes(a), ndi.binary_fill_holes(a))


# ---------------------------------------------------------------------------------------------- the reference's functions

@pytest.mark.parametrize("dtype", ["float32", "int16"])
def test_reference_functions_on_a_dot_grid(prep, dtype, capsys):
    mat = dref.dot_grid(dtype=dtype)
    _, num = ndi.label(mat)
    assert num == 7 * 9 - 1 + 1                                     # two discs merged, one speck
    points = prep.get_points_dot_pattern(mat, binarize=False)
    want = dref.get_points_dot_pattern(mat)
    assert points.shape == (num, 2) and points.dtype == np.float64 and np.array_equal(points, want)
    assert prep.check_num_dots(mat) is False and dref.check_num_dots(mat) is False and capsys.readouterr().out == ""
    few = mat[:32, :32]
    assert prep.check_num_dots(few) is True and dref.check_num_dots(few) is True
    assert capsys.readouterr().out == "WARNING!!! Number of detected dots: %d\nis not enough for the algorithm to work!\n" % ndi.label(few)[1]
    disc = float(np.median(ndi.sum_labels(mat, *ndi.label(mat)[:1], index=np.arange(1, num + 1))))
    for size, ratio in ((disc, 0.3), (disc, 0.01), (2.2 * disc, 0.3), (1.0, 0.5)):
        got, ref = prep.select_dots_based_size(mat, size, ratio), dref.select_dots_based_size(mat, size, ratio)
        assert got.dtype == ref.dtype == np.int16 and np.array_equal(got, ref), (size, ratio)
    kept = dref.select_dots_based_size(mat, disc, 0.3)
    assert 0 < ndi.label(kept)[1] < num                                                     # the merged pair and the speck went
    for dist, ratio in ((14.0, 0.3), (14.0, 0.02), (9.0, 0.1), (13.0, 0.05)):
        got, ref = prep.select_dots_based_distance(mat, dist, ratio), dref.select_dots_based_distance(mat, dist, ratio)
        assert got.dtype == ref.dtype == np.int16 and np.array_equal(got, ref), (dist, ratio)
    dropped = dref.select_dots_based_distance(mat, 14.0, 0.02)
    assert 0 < ndi.label(dropped)[1] < num


def test_reference_functions_take_a_device_tensor(prep):
    torch = pytest.importorskip("torch")
    mat = dref.dot_grid(dtype=np.float32)
    t = torch.from_numpy(mat).to("cuda:0")
    assert np.array_equal(prep.get_points_dot_pattern(t, binarize=False), dref.get_points_dot_pattern(mat))
    assert prep.check_num_dots(t) is False
    assert np.array_equal(prep.select_dots_based_size(t, 49.0), dref.select_dots_based_size(mat, 49.0))
    with pytest.raises(ValueError, match="Input not a binary image"):
        prep.get_points_dot_pattern(t * 2, binarize=False)


# ---------------------------------------------------------------------------------------------- the bounds-checking build

def test_bounds_checking_build_counts_no_violation(hip):
    """libdiscorpy_hip_bounds.so checks every index into the tile, the parent / root / rank planes and the accumulators (sites 30-42):
    ragged tiles at both connectivities and option values, hole filling and the measurements must count none."""
    import subprocess
    lib = os.path.join(ROOT, "discorpy_amd", "lib", "libdiscorpy_hip_bounds.so")
    assert os.path.exists(lib), "build() makes the bounds-checking library; it is missing"
    code = """
import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import label_cases as cases
from scipy import ndimage as ndi
from discorpy_amd import _ffi as F
from discorpy_amd.prep import preprocessing as prep
F.require_device()
assert F.debug_bounds()[4] == 1
for value in (1, 0):
    F.set_option("x_label_lds", value)
    for name in ("random_0.55", "serpentine", "diagonals"):
        m = cases.pattern(name, cases.BIG)
        for conn in (4, 8):
            lab, num = prep.label(m, cases.STRUCTURES[conn])
            assert num == cases.expected_labels(name, cases.BIG, conn)[1]
        assert np.array_equal(prep.binary_fill_holes(m), ndi.binary_fill_holes(m))
    assert prep.find_objects(lab, num + 3) == ndi.find_objects(lab, num + 3)
    assert np.array_equal(prep.sum_labels(m, lab, np.arange(1, num + 1)), ndi.sum_labels(m, lab, np.arange(1, num + 1)))
b = F.debug_bounds()
assert b[0] == 0 and b[4] == 1, b
print("bounds ok", b)
""" % (ROOT, os.path.join(ROOT, "tests", "helpers"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT, env=dict(os.environ, DCP_LIB_PATH=lib))
    assert r.returncode == 0 and "bounds ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
