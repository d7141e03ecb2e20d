"""The plane entry points of the C ABI (dcp_*_2d: median, Gaussian, labelling, measurements, hole filling, binarization) give one answer
whatever memory the planes are in and whatever the row stride: each is called four times through _ffi -- device memory on a plane
inside a wider allocation (row stride width + 13) on a stream of its own, device memory on a dense copy, host memory on the strided
plane, host memory on the dense copy -- and the four output planes are equal byte for byte, the four sets of host scalars are equal,
and both equal scipy's / NumPy's.  csrc/api_plane.h forks on the memory kind in one place (run_plane); what that place can get wrong is
the stride handed to the launch on each path, the read-back of the scalars and the synchronisation, and that is all this file aims at.

The padding around the strided plane holds values that would change the answer if a kernel read them (set pixels, label 1, the
type's greatest value, a value above the threshold), and it lies inside the allocation, so a wrong stride shows as a wrong result and
not as a fault.  The three entry points that return host scalars (dcp_label_2d, dcp_minmax_2d, dcp_histogram_2d) must have
synchronised the stream themselves: their scalars are read right after the call; for the others the test synchronises before it
reads a plane.

Shapes: 37 x 70 (more than one tile of TH = 32 rows, not a multiple of either side; tests/helpers/label_cases.py), 37 x (TW + 7)
(more than one tile of TW = 128 columns too), and 1 x 70 and 37 x 1, where a caller's row stride is arbitrary."""
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

PAD, LEFT = 13, 5          # row stride = width + PAD; the plane begins LEFT elements into each row of the allocation
SHAPES = [(37, 70), (37, cases.TW + 7), (1, 70), (37, 1)]
assert cases.TH < 37 < 2 * cases.TH and 37 % cases.TH and 70 % cases.TW and cases.TW < cases.TW + 7 < 2 * cases.TW
WAYS = [("device, strided, own stream", True, True), ("device, dense", True, False), ("host, strided", False, True), ("host, dense", False, False)]


class Side:
    """The buffers of one of the four calls, in device memory (DeviceArray) or host memory (NumPy)."""

    def __init__(self, F, device, strided):
        self.F, self.device, self.strided = F, device, strided
        self.mem = F.MEM_DEVICE if device else F.MEM_HOST
        self.own = F.Stream() if device and strided else None
        self.stream = self.own.ptr if self.own else None
        self.keep = []

    def buffer(self, array):
        """(pointer, reader) of a copy of ``array`` in this side's memory."""
        array = np.ascontiguousarray(array)
        if self.device:
            dev = self.F.DeviceArray(array.shape, array.dtype).copy_from_host(array)
            self.keep.append(dev)
            return dev.ptr, dev.copy_to_host
        host = array.copy()
        self.keep.append(host)
        return host.ctypes.data, lambda: host

    def source(self, plane, pad):
        """(pointer, row stride) of ``plane``: dense, or inside an allocation of rows PAD wider that holds ``pad`` everywhere else."""
        if not self.strided:
            return self.buffer(plane)[0], plane.shape[1]
        wide = np.full((plane.shape[0], plane.shape[1] + PAD), pad, plane.dtype)
        wide[:, LEFT:LEFT + plane.shape[1]] = plane
        return self.buffer(wide)[0] + LEFT * plane.itemsize, plane.shape[1] + PAD

    def output(self, shape, dtype, fill=0x5B):
        return self.buffer(np.full(shape, fill, dtype))

    def synchronize(self):
        if self.device:
            self.F.check(self.F.lib().dcp_stream_synchronize(-1, self.stream))


def four_ways(F, call, want_plane, want_scalars):
    """``call(side)`` runs the entry point on one side's buffers and returns (host scalars read at once, reader of the output plane or
    None, readers of scalars that are only good after the stream)."""
    planes, scalars = [], []
    for name, device, strided in WAYS:
        side = Side(F, device, strided)
        at_once, plane, later = call(side)
        at_once = [np.array(v) for v in at_once]          # copied before anything else touches the stream
        side.synchronize()
        planes.append(None if plane is None else plane())
        scalars.append(at_once + [np.array(read()) for read in later])
    for (name, _, _), plane, got in zip(WAYS, planes, scalars):
        if want_plane is not None:
            assert plane.dtype == want_plane.dtype and plane.tobytes() == want_plane.tobytes(), name
        assert len(got) == len(want_scalars), name
        for g, w in zip(got, want_scalars):
            assert np.array_equal(g, np.asarray(w)), (name, g, w)


def image(dtype, shape, seed):
    rng = np.random.default_rng(seed)
    if np.dtype(dtype).kind == "f":
        return (rng.random(shape) * 2 - 1).astype(dtype)
    info = np.iinfo(dtype)
    return rng.integers(info.min, info.max, shape, endpoint=True).astype(dtype)


def greatest(dtype):
    return np.finfo(dtype).max if np.dtype(dtype).kind == "f" else np.iinfo(dtype).max


def dots(dtype, shape, seed=3):
    return (np.random.default_rng(seed).random(shape) < 0.55).astype(dtype)


def options(F, key, values, body):
    old = F.get_option(key)
    try:
        for value in values:
            F.set_option(key, value)
            body()
    finally:
        F.set_option(key, old)


@pytest.fixture(scope="module")
def F(hip):
    return hip


SHAPE_IDS = ["%dx%d" % s for s in SHAPES]


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("dtype", ["uint16", "float32"])
def test_median(F, dtype, shape):
    plane, (h, w), code = image(dtype, shape, 1), shape, F.DTYPE_BY_NAME[dtype]
    want = ndi.median_filter(plane, (3, 5), mode="reflect")

    def call(side):
        src, stride = side.source(plane, greatest(dtype))
        dst, read = side.output(shape, dtype)
        F.check(F.lib().dcp_median_filter_2d(src, dst, h, w, stride, code, 3, 5, side.mem, -1, side.stream))
        return [], read, []
    options(F, "x_median_lds", (0, 1), lambda: four_ways(F, call, want, []))


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("dtype", ["uint16", "float32"])
def test_gaussian(F, dtype, shape):
    from discorpy_amd.post.postprocessing import _MODES
    from discorpy_amd.prep import linepattern as lp
    plane, (h, w), code = image(dtype, shape, 2), shape, F.DTYPE_BY_NAME[dtype]
    want = ndi.gaussian_filter(plane, 1.5, mode="nearest")
    weights = lp._gaussian_weights(1.5)
    wptr, radius = weights.ctypes.data_as(F.C.POINTER(F.C.c_double)), len(weights) // 2

    def call(side):
        src, stride = side.source(plane, greatest(dtype))
        dst, read = side.output(shape, dtype)
        F.check(F.lib().dcp_correlate_sym_2d(src, dst, h, w, stride, code, wptr, radius, wptr, radius, _MODES.index("nearest"), 0.0, side.mem, -1,
                                             side.stream))
        return [], read, []
    options(F, "x_gauss_lds", (0, 1, 2), lambda: four_ways(F, call, want, []))


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("dtype", ["uint16", "float32"])
def test_label(F, dtype, shape):
    plane, (h, w), code = dots(dtype, shape), shape, F.DTYPE_BY_NAME[dtype]
    want, want_num = ndi.label(plane)

    def call(side):
        src, stride = side.source(plane, 1)
        dst, read = side.output(shape, np.int32)
        num = F.C.c_int(-7)
        F.check(F.lib().dcp_label_2d(src, dst, h, w, stride, code, 4, F.C.byref(num), side.mem, -1, side.stream))
        return [num.value], read, []          # (the count without a synchronise of the test's: the call has waited for it)
    options(F, "x_label_lds", (0, 1), lambda: four_ways(F, call, want.astype(np.int32), [want_num]))


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("dtype", ["uint16", "float32"])
def test_fill_holes_and_clear_border(F, dtype, shape):
    plane, (h, w), code = dots(dtype, shape, 4), shape, F.DTYPE_BY_NAME[dtype]

    def fill(side):
        src, stride = side.source(plane, 1)
        dst, read = side.output(shape, np.uint8)
        F.check(F.lib().dcp_fill_holes_2d(src, dst, h, w, stride, code, side.mem, -1, side.stream))
        return [], read, []

    def clear(side):
        src, stride = side.source(plane, 1)
        dst, read = side.output(shape, np.uint8)
        F.check(F.lib().dcp_clear_border_2d(src, dst, h, w, stride, code, 8, 0, side.mem, -1, side.stream))
        return [], read, []
    options(F, "x_label_lds", (0, 1), lambda: (four_ways(F, fill, ndi.binary_fill_holes(plane).astype(np.uint8), []),
                                               four_ways(F, clear, bref.clear_border(plane, 8), [])))


def measure_table(weights, labels, num):
    """(int64 count, sum v, sum y v, sum x v) and (int32 min y, max y, min x, max x) of the labels 1..num, in exact integers."""
    sums, boxes = np.zeros((num, 4), np.int64), np.zeros((num, 4), np.int32)
    for j in range(1, num + 1):
        y, x = np.nonzero(labels == j)
        v = weights[y, x].astype(np.int64)
        sums[j - 1] = (len(y), v.sum(), (y * v).sum(), (x * v).sum())
        boxes[j - 1] = (y.min(), y.max(), x.min(), x.max())
    return sums, boxes


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_label_measures(F, shape):
    """Two source planes with strides of their own: the padding of the labels holds label 1, that of the weights 65535."""
    (h, w), code = shape, F.DTYPE_BY_NAME["uint16"]
    labels, num = ndi.label(dots(np.uint8, shape, 5))
    labels, weights = labels.astype(np.int32), image("uint16", shape, 6)
    want_sums, want_boxes = measure_table(weights, labels, num)
    assert np.array_equal(want_sums[:, 1].astype(np.float64), ndi.sum_labels(weights, labels, np.arange(1, num + 1)))

    def call(side):
        wsrc, wstride = side.source(weights, 65535)
        lsrc, lstride = side.source(labels, 1)
        sums, read_sums = side.output((num, 4), np.int64, -1)
        boxes, read_boxes = side.output((num, 4), np.int32, -1)
        F.check(F.lib().dcp_label_measures_2d(wsrc, lsrc, h, w, wstride, lstride, code, num, sums, boxes, side.mem, -1, side.stream))
        return [], None, [read_sums, read_boxes]
    four_ways(F, call, None, [want_sums, want_boxes])


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_abs_and_minmax(F, dtype, shape):
    plane, (h, w), code = image(dtype, shape, 7), shape, F.DTYPE_BY_NAME[dtype]
    pad = np.inf if dtype == "float32" else greatest(dtype)          # would move the maximum (and the count of non-finite elements)

    def absolute(side):
        src, stride = side.source(plane, pad)
        dst, read = side.output(shape, dtype)
        F.check(F.lib().dcp_abs_2d(src, dst, h, w, stride, code, side.mem, -1, side.stream))
        return [], read, []

    def minmax(side):
        src, stride = side.source(plane, pad)
        out, bad = (F.C.c_double * 2)(-7.0, -7.0), F.C.c_int64(-7)
        F.check(F.lib().dcp_minmax_2d(src, h, w, stride, code, out, F.C.byref(bad), side.mem, -1, side.stream))
        return [out[0], out[1], bad.value], None, []
    four_ways(F, absolute, np.abs(plane), [])
    four_ways(F, minmax, None, [float(plane.min()), float(plane.max()), 0])


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("dtype", ["uint16", "float32"])
def test_histogram(F, dtype, shape):
    (h, w), code, nbins = shape, F.DTYPE_BY_NAME[dtype], 40
    if dtype == "float32":
        plane = image(dtype, shape, 8)
        plane.flat[0], plane.flat[-1] = -1.0, 1.0
        want, edges = np.histogram(plane, nbins)
        assert edges.dtype == np.float32
        eptr, first, pad = edges.ctypes.data, 0, 0.0
    else:
        plane = np.random.default_rng(8).integers(5, 45, shape).astype(dtype)
        want, eptr, first, pad = np.bincount(plane.ravel().astype(np.int64) - 5, minlength=nbins), None, 5, 7

    def call(side):
        src, stride = side.source(plane, pad)
        counts = np.full(nbins, -7, np.int64)
        F.check(F.lib().dcp_histogram_2d(src, h, w, stride, code, eptr, nbins, first, counts.ctypes.data, side.mem, -1, side.stream))
        return [counts], None, []
    options(F, "x_hist_lds", (0, 1), lambda: four_ways(F, call, None, [want.astype(np.int64)]))


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("dtype", ["uint16", "float32"])
def test_threshold(F, dtype, shape):
    """The count is a word of the memory the planes are in, and the call adds to it: a device word for device memory, a host word for
    host memory."""
    plane, (h, w), code = image(dtype, shape, 9), shape, F.DTYPE_BY_NAME[dtype]
    thres = 0.25 if dtype == "float32" else 40000.0
    want = (plane.astype(np.float64) > thres).astype(np.uint8)

    def call(side):
        src, stride = side.source(plane, greatest(dtype))
        dst, read = side.output(shape, np.uint8)
        count, read_count = side.buffer(np.full(1, 100, np.int64))
        F.check(F.lib().dcp_threshold_2d(src, dst, h, w, stride, code, thres, count, side.mem, -1, side.stream))
        return [], read, [read_count]
    four_ways(F, call, want, [[100 + int(want.sum())]])


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_morphology(F, shape):
    plane, (h, w) = image("uint8", shape, 10), shape
    for op, ref, pad in ((0, bref.erosion, 0), (1, bref.dilation, 255), (2, bref.opening, 255)):
        def call(side):
            src, stride = side.source(plane, pad)
            dst, read = side.output(shape, np.uint8)
            F.check(F.lib().dcp_morph_cross_2d(src, dst, h, w, stride, op, side.mem, -1, side.stream))
            return [], read, []
        options(F, "x_morph_fused", (0, 1), lambda: four_ways(F, call, ref(plane), []))
