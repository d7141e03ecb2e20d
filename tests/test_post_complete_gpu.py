"""GPU suite for the completed post module: unwarp_image_forward (forward_winner_kernel + forward_fill_kernel) bit for bit against the
reference's outputs (golden G21) and the NumPy emulation of tests/helpers/forward_emulation.py; unwarp_line_backward (the root of
ru B(ru) = rd, map_points_inverse_kernel) against the reference's minimiser (golden G22); argument checks of the two new entry points."""
import ctypes as C
import os
import sys
import threading

import numpy as np
import pytest

from conftest import ROOT, golden

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import forward_emulation as fe  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g21():
    return golden("g21_forward_images")


@pytest.fixture(scope="module")
def g22():
    return golden("g22_lines_backward")


@pytest.fixture(scope="module")
def post(hip):
    import discorpy_amd.post.postprocessing as pp
    return pp


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


class DeviceView:
    """A strided view of a device allocation through ``__cuda_array_interface__`` (strides in bytes)."""

    def __init__(self, base, shape, strides, offset=0):
        self.base, self.shape, self.dtype = base, tuple(shape), base.dtype
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": base.dtype.str, "data": (base.ptr + offset, False),
                                         "version": 3, "strides": None if strides is None else tuple(strides)}


# ------------------------------------------------------------------------------------------------ forward image unwarp

@pytest.mark.parametrize("name", [n for n in fe.g21_names() if n != "complex64"])
def test_forward_equals_the_reference_host_and_device(hip, post, g21, name):
    mat, xc, yc, fact = fe.g21_input(name)
    want = g21["out_" + name]
    got = post.unwarp_image_forward(mat, xc, yc, fact)
    assert isinstance(got, np.ndarray) and same_bytes(got, want), name
    assert hip.last_kernel() == "forward_winner_kernel<NF=%d> + forward_fill_kernel<%d>" % (len(fact), mat.dtype.itemsize)
    dev = hip.DeviceArray(mat.shape, mat.dtype).copy_from_host(mat)
    res = post.unwarp_image_forward(dev, xc, yc, fact)
    assert isinstance(res, hip.DeviceArray) and res.dtype == mat.dtype
    assert same_bytes(res.copy_to_host(), want), name


def test_forward_complex_goes_through_its_parts(post, g21):
    mat, xc, yc, fact = fe.g21_input("complex64")
    got = post.unwarp_image_forward(mat, xc, yc, fact)
    assert same_bytes(got, g21["out_complex64"])
    out = np.empty_like(mat)
    assert post.unwarp_image_forward(mat, xc, yc, fact, out=out) is out and same_bytes(out, g21["out_complex64"])


def test_forward_strided_views_out_and_overlap(hip, post):
    base = np.random.default_rng(5).random((90, 154), dtype=np.float32) + np.float32(0.25)
    xc, yc, fact = 40.3, 21.9, [1.0, 2.0e-3, -1.0e-5]
    for view in (base[::2], base[:, ::3], base[1::3, 2::2]):                       # row-strided, column-strided, both
        assert fe.half_integer_margin(*view.shape, xc, yc, fact) >= 1e-9
        assert same_bytes(post.unwarp_image_forward(view, xc, yc, fact), fe.unwarp_image_forward(view, xc, yc, fact))
    dev = hip.DeviceArray(base.shape, base.dtype).copy_from_host(base)
    for sl, shape, strides, off in ((np.s_[::2], (45, 154), (2 * 154 * 4, 4), 0), (np.s_[:, ::3], (90, 52), (154 * 4, 12), 0),
                                    (np.s_[1::3, 2::2], (30, 76), (3 * 154 * 4, 8), (154 + 2) * 4)):
        res = post.unwarp_image_forward(DeviceView(dev, shape, strides, off), xc, yc, fact)
        assert same_bytes(res.copy_to_host(), fe.unwarp_image_forward(base[sl], xc, yc, fact))
    want = fe.unwarp_image_forward(base, xc, yc, fact)
    out = np.full_like(base, 7.0)
    assert post.unwarp_image_forward(base, xc, yc, fact, out=out) is out and same_bytes(out, want)
    dout = hip.DeviceArray(base.shape, base.dtype).copy_from_host(np.full_like(base, 7.0))
    assert post.unwarp_image_forward(dev, xc, yc, fact, out=dout) is dout and same_bytes(dout.copy_to_host(), want)
    with pytest.raises(ValueError, match="overlap"):
        post.unwarp_image_forward(base, xc, yc, fact, out=base)
    with pytest.raises(ValueError, match="overlap"):
        post.unwarp_image_forward(dev, xc, yc, fact, out=dev)
    with pytest.raises(ValueError):
        post.unwarp_image_forward(base, xc, yc, fact, out=np.empty((90, 154), np.float64))
    assert same_bytes(dev.copy_to_host(), base)                                    # the refused calls wrote nothing


def test_forward_destination_not_aligned_to_four_elements(hip, post):
    """The fill pass stores four elements at once where the destination allows it; a dense destination at an odd address must not."""
    mat = fe.typed_frame("uint8", (8, 12), 31)
    xc, yc, fact = 5.3, 3.6, [1.0, 2.0e-2]
    assert fe.half_integer_margin(8, 12, xc, yc, fact) >= 1e-9
    src = hip.DeviceArray(mat.shape, mat.dtype).copy_from_host(mat)
    room = hip.DeviceArray((200,), np.uint8).copy_from_host(np.full(200, 9, np.uint8))
    for off in (1, 2, 3, 4):
        out = DeviceView(room, (8, 12), None, off)
        assert post.unwarp_image_forward(src, xc, yc, fact, out=out) is out
        got = room.copy_to_host()
        assert np.array_equal(got[off:off + 96].reshape(8, 12), fe.unwarp_image_forward(mat, xc, yc, fact))
        assert np.all(got[:off] == 9) and np.all(got[off + 96:] == 9)              # nothing written around the frame
        room.copy_from_host(np.full(200, 9, np.uint8))


def test_forward_input_errors(post):
    with pytest.raises(ValueError):                                                # the reference's (height, width) = mat.shape
        post.unwarp_image_forward(np.zeros((3, 4, 5), np.float32), 1.0, 1.0, [1.0])
    with pytest.raises(ValueError):
        post.unwarp_image_forward(np.zeros(7, np.float32), 1.0, 1.0, [1.0])
    img = np.ones((5, 6), np.float32)
    for xc, yc, fact in ((np.nan, 1.0, [1.0]), (1.0, np.inf, [1.0]), (1.0, 1.0, [1.0, np.nan]), (1.0, 1.0, [-np.inf])):
        with pytest.raises(ValueError, match="finite"):
            post.unwarp_image_forward(img, xc, yc, fact)
    with pytest.raises(ValueError, match="nfact"):
        post.unwarp_image_forward(img, 1.0, 1.0, [1.0] * 33)


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (9, 1), (17, 65), (300, 517)])
@pytest.mark.parametrize("dtype", ["float32", "uint8", "int16", "float64"])
def test_forward_shapes_against_the_emulation(post, shape, dtype):
    mat = fe.typed_frame(dtype, shape, 77)
    h, w = shape
    for xc, yc, fact in ((0.45 * w, 0.55 * h, [1.0, 1.5e-3, 2.0e-6]), (0.6 * w + 0.3, 0.4 * h - 0.2, [0.97, -8.0e-4]),
                         (w + 3.2, -2.6, [1.0, 0.0, 1.0e-6, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0e-30, 0.0])):      # 12 terms: the looped polynomial
        assert fe.half_integer_margin(h, w, xc, yc, fact) >= 1e-9
        assert same_bytes(post.unwarp_image_forward(mat, xc, yc, fact), fe.unwarp_image_forward(mat, xc, yc, fact)), (shape, dtype, fact)


def test_forward_every_pixel_onto_one(post):
    """fact = [0.0]: every source pixel lands on the pixel nearest the centre, which keeps the LAST one (all atomics on one word)."""
    mat = np.arange(1, 300 * 517 + 1, dtype=np.uint32).reshape(300, 517)
    got = post.unwarp_image_forward(mat, 200.4, 99.7, [0.0])
    assert np.count_nonzero(got) == 1 and got[100, 200] == 300 * 517
    empty = post.unwarp_image_forward(mat, 200.4, 99.7, [])                        # no coefficients: F = 0 as well
    assert same_bytes(empty, got)


def test_forward_is_deterministic(post):
    mat, xc, yc, fact = fe.g21_input("compress")
    first = post.unwarp_image_forward(mat, xc, yc, fact)
    assert all(same_bytes(post.unwarp_image_forward(mat, xc, yc, fact), first) for _ in range(2))


def test_forward_four_threads_four_streams_four_calibrations(hip):
    L = hip.lib()
    mat = np.random.default_rng(9).random((257, 389), dtype=np.float32) + np.float32(0.5)
    h, w = mat.shape
    cals = [(190.23, 130.41, [1.0, 1.0e-3, 2.0e-6]), (140.7, 100.1, [1.0, -1.2e-3]), (250.3, 60.6, [1.02, 5.0e-4, -1.0e-6, 1.1e-9]),
            (30.9, 200.8, [0.9, 2.0e-3])]
    assert all(fe.half_integer_margin(h, w, *c) >= 1e-9 for c in cals)
    src = hip.DeviceArray(mat.shape, mat.dtype).copy_from_host(mat)
    dsts = [hip.DeviceArray(mat.shape, mat.dtype) for _ in cals]
    fas = [hip.fact_array(c[2]) for c in cals]

    def call(k, stream):
        xc, yc, _ = cals[k]
        return L.dcp_unwarp_image_forward(src.ptr, dsts[k].ptr, hip.DTYPE_F32, h, w, w, 1, xc, yc, fas[k][0], fas[k][1], hip.MEM_DEVICE, -1, stream)

    single = []
    for k in range(4):
        hip.check(call(k, None))
        hip.check(L.dcp_stream_synchronize(-1, None))
        single.append(dsts[k].copy_to_host())
        assert same_bytes(single[k], fe.unwarp_image_forward(mat, *cals[k]))
        dsts[k].copy_from_host(np.zeros_like(mat))
    streams = [hip.Stream() for _ in cals]
    codes = [[] for _ in cals]
    gate = threading.Barrier(4)

    def worker(k):
        gate.wait()
        for _ in range(6):
            codes[k].append(call(k, streams[k].ptr))
        streams[k].synchronize()

    threads = [threading.Thread(target=worker, args=(k,)) for k in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert all(c == [hip.OK] * 6 for c in codes), codes
    for k in range(4):
        assert same_bytes(dsts[k].copy_to_host(), single[k]), k


def test_forward_full_size_frame(hip, post):
    """configs.cfg2() at 4096^2, float32, device-resident, against the emulation.  At most 4 pixels may differ (the margin
    test_gpu_parity.py gives the two polynomial orders at this size); the nearest coordinate lies 2.5e-9 px from a half-integer and a
    Horner evaluation agrees with NumPy's order on every destination index, so 0 are expected."""
    from discorpy_amd import configs
    cfg = configs.cfg2()
    h, w = cfg["shape"]
    mat = np.random.default_rng(cfg["seed"]).random((h, w), dtype=np.float32) + np.float32(0.5)
    want = fe.unwarp_image_forward(mat, cfg["xcenter"], cfg["ycenter"], cfg["list_fact"])
    dev = hip.DeviceArray(mat.shape, mat.dtype).copy_from_host(mat)
    res = post.unwarp_image_forward(dev, cfg["xcenter"], cfg["ycenter"], cfg["list_fact"])
    assert hip.last_kernel() == "forward_winner_kernel<NF=5> + forward_fill_kernel<4>"
    got = res.copy_to_host()
    differing = int(np.count_nonzero(got.view(np.uint32) != want.view(np.uint32)))
    print("forward 4096^2: %d pixels differ from the emulation" % differing)
    assert differing <= 4, "%d pixels differ from the NumPy emulation (expected 0, allowed 4)" % differing


# ------------------------------------------------------------------------------------------------ backward line unwarp

def _split(points, sizes):
    out, pos = [], 0
    for n in sizes:
        out.append(points[pos:pos + int(n)])
        pos += int(n)
    return out


def _residual(points, dpoints, xc, yc, fact):
    """|rd - ru B(ru)| with ru from `points` and rd from the distorted points, in NumPy."""
    ru = np.sqrt((points[:, 1] - xc) ** 2 + (points[:, 0] - yc) ** 2)
    rd = np.sqrt((dpoints[:, 1] - xc) ** 2 + (dpoints[:, 0] - yc) ** 2)
    return np.abs(rd - ru * np.sum(np.asarray([a * ru ** i for i, a in enumerate(fact)]), axis=0))


@pytest.mark.parametrize("name", ["unit", "grid"])
def test_line_backward_solves_the_equation_better_than_the_reference(post, g22, name):
    xc, yc, fact = float(g22[name + "_xcenter"]), float(g22[name + "_ycenter"]), list(g22[name + "_list_fact"])
    dpts, ref, sizes = g22[name + "_dlines"], g22[name + "_ref"], g22[name + "_sizes"]
    got_lines = post.unwarp_line_backward(_split(dpts, sizes), xc, yc, fact)
    assert [len(ln) for ln in got_lines] == [int(n) for n in sizes] and all(ln.dtype == np.float64 for ln in got_lines)
    got = np.concatenate(got_lines)
    ours, theirs = _residual(got, dpts, xc, yc, fact), _residual(ref, dpts, xc, yc, fact)
    print("%s: equation residual ours max %.3g, reference max %.3g" % (name, ours.max(), theirs.max()))
    assert np.all(ours <= theirs), (ours.max(), np.flatnonzero(ours > theirs)[:5])
    bound = theirs / float(g22[name + "_min_dg"]) + 1e-9
    dist = np.sqrt(((got - ref) ** 2).sum(axis=1))
    assert np.all(dist <= bound), (dist.max(), np.flatnonzero(dist > bound)[:5])


@pytest.mark.parametrize("name", ["unit", "grid"])
def test_line_forward_then_backward_returns_the_grid(post, g22, name):
    xc, yc, fact = float(g22[name + "_xcenter"]), float(g22[name + "_ycenter"]), list(g22[name + "_list_fact"])
    grid = _split(g22[name + "_ulines"], g22[name + "_sizes"])
    back = post.unwarp_line_backward(post.unwarp_line_forward(grid, xc, yc, fact), xc, yc, fact)
    assert max(np.abs(b - u).max() for b, u in zip(back, grid)) <= 1e-9


def test_line_backward_centre_dtypes_and_empties(post, g22):
    xc, yc, fact = float(g22["grid_xcenter"]), float(g22["grid_ycenter"]), list(g22["grid_list_fact"])
    assert np.array_equal(g22["grid_dlines"][-1], [yc, xc])                        # the golden's last line is the centre itself
    centre = post.unwarp_line_backward([np.array([[yc, xc]])], xc, yc, fact)[0]
    assert np.array_equal(centre, [[yc, xc]])
    ints = post.unwarp_line_backward([np.array([[10, 20], [300, 700]], dtype=np.int32), np.array([[5.5, 6.5]], dtype=np.float32)], xc, yc, fact)
    assert ints[0].dtype == np.int32 and ints[0].shape == (2, 2) and ints[1].dtype == np.float32
    assert post.unwarp_line_backward([], xc, yc, fact) == []
    res = post.unwarp_line_backward([np.zeros((0, 2)), np.array([[yc + 3.0, xc - 4.0]])], xc, yc, [1.0])
    assert res[0].shape == (0, 2) and np.allclose(res[1], [[yc + 3.0, xc - 4.0]], rtol=0, atol=1e-12)
    assert [ln.shape for ln in post.unwarp_line_backward([np.zeros((0, 2))], xc, yc, fact)] == [(0, 2)]


def test_line_backward_without_a_root_raises_with_the_count(post):
    # ru (1 - 0.01 ru) never exceeds 25: the two points at radius 30 and 40 have no root, the one at radius 10 has
    lines = [np.array([[50.0, 80.0], [50.0, 60.0]]), np.array([[90.0, 50.0]])]
    with pytest.raises(ValueError, match=r"no root for 2 of 3 points"):
        post.unwarp_line_backward(lines, 50.0, 50.0, [1.0, -1.0e-2])
    ok = post.unwarp_line_backward([np.array([[50.0, 60.0]])], 50.0, 50.0, [1.0, -1.0e-2])[0]
    ru = ok[0, 1] - 50.0
    assert abs(ru * (1.0 - 1.0e-2 * ru) - 10.0) < 1e-12 and 11.0 < ru < 12.0          # the root next to the start, not the far one


# ------------------------------------------------------------------------------------------------ argument checks

def test_bad_arguments_are_refused_before_any_launch(hip):
    L = hip.lib()
    img = np.arange(48, dtype=np.float32).reshape(6, 8)
    dst = np.full_like(img, -1.0)
    fa, nf = hip.fact_array([1.0, 1e-3])
    hip.check(L.dcp_unwarp_image_forward(img.ctypes.data, dst.ctypes.data, hip.DTYPE_F32, 6, 8, 8, 1, 3.0, 2.0, fa, nf, hip.MEM_HOST, -1, None))
    before = hip.last_kernel()
    assert before.startswith("forward_winner_kernel")
    good = dict(src=img.ctypes.data, dst=dst.ctypes.data, dtype=hip.DTYPE_F32, h=6, w=8, rs=8, cs=1, fa=fa, nf=nf, mem=hip.MEM_HOST)
    bad = [dict(src=None), dict(dst=None), dict(h=0), dict(w=0), dict(h=-3), dict(rs=7), dict(cs=0), dict(nf=33), dict(nf=-1), dict(fa=None),
           dict(dtype=11), dict(dtype=-1), dict(mem=7), dict(dst=img.ctypes.data), dict(dst=img.ctypes.data + 16)]
    hip.check(L.dcp_unwarp_image_typed(img.ctypes.data, dst.ctypes.data, hip.DTYPE_F32, 6, 8, 8, 1, 3.0, 2.0, fa, nf, 0, 0, hip.MEM_HOST, -1, None))
    marker = hip.last_kernel()                                                       # another kernel's name: a forward launch would replace it
    sentinel = dst.copy()
    for change in bad:
        a = dict(good, **change)
        rc = L.dcp_unwarp_image_forward(a["src"], a["dst"], a["dtype"], a["h"], a["w"], a["rs"], a["cs"], 3.0, 2.0, a["fa"], a["nf"], a["mem"], -1, None)
        assert rc == hip.ERR_INVALID_ARG and len(hip.last_error()) > 3, (change, rc, hip.last_error())
        assert hip.last_kernel() == marker and (a["dst"] != dst.ctypes.data or np.array_equal(dst, sentinel)), change
    # a frame too large for the 32-bit winner plane is unsupported, not invalid (nothing is touched: the check comes first)
    rc = L.dcp_unwarp_image_forward(img.ctypes.data, dst.ctypes.data, hip.DTYPE_BY_NAME["uint8"], 65536, 65536, 65536, 1, 3.0, 2.0, fa, nf, hip.MEM_DEVICE, -1, None)
    assert rc == hip.ERR_UNSUPPORTED and "2^32" in hip.last_error()

    pts = np.array([[1.0, 2.0], [3.0, 4.0]])
    out = np.full_like(pts, -5.0)
    count = C.c_int64(-9)
    pgood = dict(src=pts.ctypes.data, dst=out.ctypes.data, n=2, fa=fa, nf=nf, mem=hip.MEM_HOST)
    for change in (dict(src=None), dict(dst=None), dict(n=-1), dict(nf=33), dict(nf=-2), dict(fa=None), dict(mem=9)):
        a = dict(pgood, **change)
        rc = L.dcp_map_points_inverse_f64(a["src"], a["dst"], a["n"], 3.0, 2.0, a["fa"], a["nf"], C.byref(count), a["mem"], -1, None)
        assert rc == hip.ERR_INVALID_ARG and len(hip.last_error()) > 3, (change, rc, hip.last_error())
        assert np.all(out == -5.0) and count.value == -9, change
    hip.check(L.dcp_map_points_inverse_f64(pts.ctypes.data, out.ctypes.data, 2, 3.0, 2.0, fa, nf, C.byref(count), hip.MEM_HOST, -1, None))
    assert count.value == 0 and np.all(np.isfinite(out))
    hip.check(L.dcp_map_points_inverse_f64(pts.ctypes.data, out.ctypes.data, 2, 3.0, 2.0, fa, nf, None, hip.MEM_HOST, -1, None))      # the count is optional
    hip.check(L.dcp_map_points_inverse_f64(None, None, 0, 3.0, 2.0, fa, nf, C.byref(count), hip.MEM_HOST, -1, None))
    assert count.value == 0
