"""GPU suite for the peak search with select_peaks=True in one call (dcp_extrema_select_rows; extrema_list_kernel, extrema_fit_kernel and
extrema_compact_kernel of csrc/extrema_select_kernels.hip behind peak_rows_kernel; prep.linecomplete on top).  The yardstick is the
composition the call replaces, made of entry points that have suites of their own: dcp_local_extrema_rows for the candidates,
dcp_select_peaks_rows on rows.max(axis=1, keepdims=True) - rows formed by NumPy in the rows' type, and the kept entries of
dcp_local_extrema_rows(subpixel=1).  The one call must give the composition's tables bit for bit -- dst, cand and keep -- whether the
selection's plane is formed by the kernel (sel = NULL) or handed in; on shapes that strain a worklist (the widest window, several
hundred fits over every tile of the search, rows without candidates, rows whose candidates all fail, a NaN or an infinity that empties a
whole row through the row maximum) it must not depend on the order the tickets are drawn in; strided device planes on a stream of their
own must agree with host memory.  The wrappers of prep.linecomplete are compared with the same composition through prep.linepattern,
and with the reference itself through golden G33 (tools/gen_golden.py): what discorpy's own functions return with select_peaks=True,
with every candidate its select_good_peaks judged recorded and marked clear or unclear by G32's rule.  Where every candidate of a row
is clear the positions must be the reference's; unclear ones may go either way and are counted, never asserted."""
import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu

FILL = -777.0
KFILL = 0xA5


@pytest.fixture(scope="module")
def g32():
    g = golden("g32_select_peaks")
    for v in g.values():
        v.setflags(write=False)
    return g


@pytest.fixture(scope="module")
def lc(hip):
    from discorpy_amd.prep import linecomplete
    return linecomplete


@pytest.fixture(scope="module")
def lp(hip):
    from discorpy_amd.prep import linepattern
    return linepattern


def minima_rows(g, dtype):
    """The 27 x 160 rows of G32 (lines, noise, a ramp, a square wave) with option="max" applied: the lines are minima."""
    rows = np.concatenate([g["r7_rows"], g["h7_rows"]]).astype(dtype)
    return np.ascontiguousarray(rows.max(axis=1, keepdims=True) - rows)


def sens_of(dtype, sensitive=0.1):
    return float(np.dtype(dtype).type(sensitive))


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def fused(hip, src, radius, sensitive, subpixel, sel=None, tol=0.2, use_offset=True, want_tables=True):
    """(dst, cand, keep) of one dcp_extrema_select_rows call on host memory; the tables start from FILL / KFILL and carry a guard behind them."""
    n, length = src.shape
    dst, cand, keep = np.full(n * length + 16, FILL), np.full(n * length + 16, FILL), np.full(n * length + 16, KFILL, np.uint8)
    hip.check(hip.lib().dcp_extrema_select_rows(src.ctypes.data, dst.ctypes.data, n, length, length, hip.DTYPE_BY_NAME[src.dtype.name], radius, sensitive,
                                                int(subpixel), None if sel is None else sel.ctypes.data, length, tol, int(use_offset),
                                                cand.ctypes.data if want_tables else None, keep.ctypes.data if want_tables else None,
                                                hip.MEM_HOST, -1, None))
    assert (dst[n * length:] == FILL).all() and (cand[n * length:] == FILL).all() and (keep[n * length:] == KFILL).all()
    if not want_tables:
        assert (cand == FILL).all() and (keep == KFILL).all()
    return dst[:n * length].reshape(n, length), cand[:n * length].reshape(n, length), keep[:n * length].reshape(n, length)


def extrema(hip, src, radius, sensitive, subpixel):
    n, length = src.shape
    out = np.full((n, length), FILL)
    hip.check(hip.lib().dcp_local_extrema_rows(src.ctypes.data, out.ctypes.data, n, length, length, hip.DTYPE_BY_NAME[src.dtype.name], radius, sensitive,
                                               int(subpixel), hip.MEM_HOST, -1, None))
    return out


def composition(hip, src, radius, sensitive, subpixel, tol=0.2, use_offset=True):
    """(dst, cand, keep) as the three calls of the composition define them; what no call defines stays FILL / KFILL."""
    n, length = src.shape
    found = extrema(hip, src, radius, sensitive, 0)
    counts = found[:, -1].astype(np.int64)
    assert (counts >= 0).all() and (counts < length).all()
    with np.errstate(invalid="ignore"):
        plane = np.ascontiguousarray(src.max(axis=1, keepdims=True) - src)
    assert plane.dtype == src.dtype
    peak_row = np.repeat(np.arange(n), counts).astype(np.int32)
    peak_idx = np.concatenate([found[r, :counts[r]] for r in range(n)]).astype(np.int32)
    flags = np.zeros(len(peak_idx), np.uint8)
    if len(peak_idx):
        i32p = hip.C.POINTER(hip.C.c_int32)
        hip.check(hip.lib().dcp_select_peaks_rows(plane.ctypes.data, n, length, length, hip.DTYPE_BY_NAME[src.dtype.name], peak_row.ctypes.data_as(i32p),
                                                  peak_idx.ctypes.data_as(i32p), len(peak_idx), radius, tol, int(use_offset), flags.ctypes.data, None,
                                                  hip.MEM_HOST, -1, None))
    refined = extrema(hip, src, radius, sensitive, 1) if subpixel else found
    assert np.array_equal(refined[:, -1], found[:, -1])
    dst, cand, keep = np.full((n, length), FILL), np.full((n, length), FILL), np.full((n, length), KFILL, np.uint8)
    first = 0
    for r in range(n):
        k = flags[first:first + counts[r]] != 0
        first += counts[r]
        cand[r, :counts[r]], cand[r, -1] = found[r, :counts[r]], counts[r]
        keep[r, :counts[r]] = k
        dst[r, :k.sum()], dst[r, -1] = refined[r, :counts[r]][k], k.sum()
    return dst, cand, keep, plane


def report(tag, cand, dst):
    print("%s: %d candidates, %d kept; rows without candidates %d, rows with all rejected %d" % (
        tag, int(cand[:, -1].sum()), int(dst[:, -1].sum()), int((cand[:, -1] == 0).sum()), int(((cand[:, -1] > 0) & (dst[:, -1] == 0)).sum())))


# --------------------------------------------------------------------------- 1: equal to the composition, bit for bit

@pytest.mark.parametrize("subpixel", [0, 1])
@pytest.mark.parametrize("radius", [3, 7, 11])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_one_call_equals_the_composition(hip, g32, dtype, radius, subpixel):
    src = minima_rows(g32, dtype)
    assert src.shape == (27, 160)
    want_dst, want_cand, want_keep, plane = composition(hip, src, radius, sens_of(dtype), subpixel)
    report("%s radius %d subpixel %d" % (dtype, radius, subpixel), want_cand, want_dst)
    kept, total = int(want_dst[:, -1].sum()), int(want_cand[:, -1].sum())
    assert total >= 60 and 10 <= kept <= total - 10          # the selection keeps and rejects on these rows
    dst, cand, keep = fused(hip, src, radius, sens_of(dtype), subpixel)
    assert same_bits(cand, want_cand) and same_bits(keep, want_keep)
    assert same_bits(dst, want_dst), np.argwhere(dst != want_dst)[:5]
    if subpixel:
        assert (dst[:, :-1][dst[:, :-1] != FILL] % 1 != 0).any()          # (refined positions, not the integers)
    # the selection's plane handed in: the same bits -- a row maximum or a subtraction in another type would show here
    dst_s, cand_s, keep_s = fused(hip, src, radius, sens_of(dtype), subpixel, sel=plane)
    assert same_bits(dst_s, dst) and same_bits(cand_s, cand) and same_bits(keep_s, keep)
    # other criteria than the defaults
    want2 = composition(hip, src, radius, sens_of(dtype), subpixel, tol=0.3, use_offset=False)
    got2 = fused(hip, src, radius, sens_of(dtype), subpixel, tol=0.3, use_offset=False)
    assert all(same_bits(a, b) for a, b in zip(got2, want2[:3]))
    assert want2[0][:, -1].sum() >= kept


# --------------------------------------------------------------------------- 2: shapes that break a worklist

@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_widest_window(hip, g32, dtype):
    """Radius 128 on G32's row of 600 samples: windows of 257 samples, four doubles per lane and one more in lane 0."""
    rows = g32["big_rows"].astype(dtype)
    src = np.ascontiguousarray(rows.max(axis=1, keepdims=True) - rows)
    assert src.shape == (1, 600)
    for subpixel in (0, 1):
        want = composition(hip, src, 128, sens_of(dtype), subpixel)
        got = fused(hip, src, 128, sens_of(dtype), subpixel)
        report("radius 128 %s subpixel %d" % (dtype, subpixel), want[1], want[0])
        assert want[1][0, -1] >= 1
        assert all(same_bits(a, b) for a, b in zip(got, want[:3]))


LENGTH = 1000


def worklist_batch(dtype, bad):
    """(6, 1000): two rows of about 80 narrow lines each (a candidate in every 256-sample tile of the search), two constant rows, a
    sawtooth whose minima all fail the fit, and a copy of the first row with one `bad` sample far behind its last line."""
    x = np.arange(LENGTH, dtype=np.float64)

    def lines(centres, sigma, depth):
        row = np.ones(LENGTH)
        for c in centres:
            row -= depth * np.exp(-0.5 * ((x - c) / sigma) ** 2)
        return row

    first = lines(12.0 + 12 * np.arange(80) + 0.3 * np.sin(np.arange(80)), 1.1, 1.0)
    second = lines(15.5 + 11.9 * np.arange(80), 1.3, 0.8)
    saw = 1.0 - 0.5 * ((x % 23) / 23.0)
    spoiled = first.copy()
    spoiled[990] = bad
    return np.ascontiguousarray(np.stack([first, np.full(LENGTH, 0.25), second, saw, np.full(LENGTH, -3.0), spoiled]).astype(dtype))


@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["nan", "inf"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_worklist_over_many_tiles_and_rows_that_come_back_empty(hip, dtype, bad):
    src = worklist_batch(dtype, bad)
    sens = sens_of(dtype)
    want_dst, want_cand, want_keep, _ = composition(hip, src, 3, sens, 1)
    counts, kept = want_cand[:, -1], want_dst[:, -1]
    print("candidates per row %s, kept %s" % (counts.tolist(), kept.tolist()))
    # what the batch is for, by the composition's own account
    assert counts.sum() > 256 and counts[0] >= 75 and counts[2] >= 75 and kept[0] >= 60 and kept[2] >= 60
    assert counts[1] == 0 and counts[4] == 0
    assert counts[3] >= 30 and kept[3] == 0
    assert counts[5] >= 75 and kept[5] == 0                  # one NaN / infinity far from the lines: np.max spoils every window of the row
    for tile in range(4):
        lo, hi = 3 + 256 * tile, min(3 + 256 * (tile + 1), LENGTH - 4)
        assert ((want_cand[0, :int(counts[0])] >= lo) & (want_cand[0, :int(counts[0])] < hi)).any()
    got = fused(hip, src, 3, sens, 1)
    assert all(same_bits(a, b) for a, b in zip(got, (want_dst, want_cand, want_keep)))
    # again, and with the rows in reverse order: every row's tables, bit for bit, whatever order the tickets were drawn in
    again = fused(hip, src, 3, sens, 1)
    assert all(same_bits(a, b) for a, b in zip(again, got))
    turned = fused(hip, np.ascontiguousarray(src[::-1]), 3, sens, 1)
    assert all(same_bits(np.ascontiguousarray(a[::-1]), b) for a, b in zip(turned, got))
    # the tables are optional
    alone = fused(hip, src, 3, sens, 1, want_tables=False)
    assert same_bits(alone[0], got[0])
    # radius 1: windows of 3 samples are not fitted, nothing is kept, the candidates are still listed
    dst1, cand1, keep1 = fused(hip, src, 1, sens, 1)
    assert (dst1[:, -1] == 0).all() and cand1[0, -1] >= 75 and (dst1[:, :-1] == FILL).all()
    assert same_bits(cand1, composition(hip, src, 1, sens, 0)[1]) and not keep1[0, :int(cand1[0, -1])].any()


# --------------------------------------------------------------------------- 3: containers

@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_strided_device_planes_on_a_stream_of_their_own(hip, g32, dtype):
    import torch
    src = minima_rows(g32, dtype)
    n, length = src.shape
    sens = sens_of(dtype)
    want = fused(hip, src, 7, sens, 1)
    with np.errstate(invalid="ignore"):
        plane = np.ascontiguousarray(src.max(axis=1, keepdims=True) - src)
    # the rows as the [:, 5:5 + L] view of a wider buffer whose margins would spoil the row maximum and every window that reached them
    buf = np.empty((n, length + 13), src.dtype)
    buf[:, :5], buf[:, 5 + length:] = np.nan, 1e30
    buf[:, 5:5 + length] = src
    pbuf = buf.copy()
    pbuf[:, 5:5 + length] = plane
    code = hip.DTYPE_BY_NAME[dtype]
    # the view in host memory
    dst = np.full((n, length), FILL)
    hip.check(hip.lib().dcp_extrema_select_rows(buf[:, 5:].ctypes.data, dst.ctypes.data, n, length, buf.shape[1], code, 7, sens, 1, None, length, 0.2, 1,
                                                None, None, hip.MEM_HOST, -1, None))
    assert same_bits(dst, want[0])
    dst[:] = FILL
    hip.check(hip.lib().dcp_extrema_select_rows(buf[:, 5:].ctypes.data, dst.ctypes.data, n, length, buf.shape[1], code, 7, sens, 1, pbuf[:, 5:].ctypes.data,
                                                pbuf.shape[1], 0.2, 1, None, None, hip.MEM_HOST, -1, None))
    assert same_bits(dst, want[0])
    # the same views in device memory, the outputs there too, on a stream of its own
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        dbuf, dpbuf = torch.from_numpy(buf).to("cuda:0"), torch.from_numpy(pbuf).to("cuda:0")
        ddst = torch.full((n * length + 16,), FILL, dtype=torch.float64, device="cuda:0")
        dcand = torch.full((n * length + 16,), FILL, dtype=torch.float64, device="cuda:0")
        dkeep = torch.full((n * length + 16,), KFILL, dtype=torch.uint8, device="cuda:0")
        hip.check(hip.lib().dcp_extrema_select_rows(dbuf[:, 5:].data_ptr(), ddst.data_ptr(), n, length, dbuf.stride(0), code, 7, sens, 1, None, length, 0.2, 1,
                                                    dcand.data_ptr(), dkeep.data_ptr(), hip.MEM_DEVICE, 0, stream.cuda_stream))
    stream.synchronize()
    for got, ref, fill in ((ddst, want[0], FILL), (dcand, want[1], FILL), (dkeep, want[2], KFILL)):
        host = got.cpu().numpy()
        assert (host[n * length:] == fill).all() and same_bits(host[:n * length].reshape(n, length), ref)
    # sel given, cand and keep null
    with torch.cuda.stream(stream):
        ddst.fill_(FILL)
        hip.check(hip.lib().dcp_extrema_select_rows(dbuf[:, 5:].data_ptr(), ddst.data_ptr(), n, length, dbuf.stride(0), code, 7, sens, 1,
                                                    dpbuf[:, 5:].data_ptr(), dpbuf.stride(0), 0.2, 1, None, None, hip.MEM_DEVICE, 0, stream.cuda_stream))
    stream.synchronize()
    assert same_bits(ddst.cpu().numpy()[:n * length].reshape(n, length), want[0])


# --------------------------------------------------------------------------- 4: the wrappers of prep.linecomplete

def composed_points(lp, rows, radius, subpixel, tol=0.2, sigma=0, use_offset=True):
    """The hand composition of prep.linepattern's docstring on prepared rows, row by row."""
    out = []
    for d in rows:
        points = lp.get_local_extrema_points(d, option="min", radius=radius, denoise=False, norm=False, subpixel=False)
        points = lp.select_good_peaks(np.max(d) - d, points.astype(np.int64), tol=tol, radius=radius, sigma=sigma, use_offset=use_offset)
        if subpixel and len(points):
            points = np.asarray([p - 1 + lp.locate_subpixel_point(d[p - 1:p + 2], option="min") for p in points])
        out.append(points)
    return out


@pytest.mark.parametrize("subpixel", [True, False])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_wrapper_gives_what_the_hand_composition_gives(hip, lc, lp, g32, dtype, subpixel):
    src = minima_rows(g32, dtype)
    for kw in ({}, dict(tol=0.3, use_offset=False), dict(sigma=1.5)):
        want = composed_points(lp, src, 7, subpixel, **kw)
        got = lc.get_local_extrema_points(src, option="min", radius=7, denoise=False, norm=False, subpixel=subpixel, select_peaks=True, **kw)
        assert isinstance(got, list) and len(got) == len(want)
        empty = 0
        for a, b in zip(got, want):
            assert isinstance(a, np.ndarray) and a.ndim == 1
            if len(b) == 0:
                assert a.shape == (0,) and a.dtype == np.float64
                empty += 1
            elif subpixel:
                # (the kernel's closed form against locate_subpixel_point's: the same operations, in float64)
                assert a.dtype == np.float64 and np.array_equal(a, np.asarray(b, np.float64))
            else:
                assert a.dtype == np.int64 and np.array_equal(a, b)
        assert 1 <= empty < len(want)
        # a batch call equals row-by-row calls
        for r in (0, 5, 25):
            one = lc.get_local_extrema_points(src[r], option="min", radius=7, denoise=False, norm=False, subpixel=subpixel, select_peaks=True, **kw)
            assert same_bits(one, got[r])
    # the steps in front of the search: the selection reads the prepared rows
    prepared = lc.get_local_extrema_points(g32["r7_rows"][:4].astype(dtype), option="max", radius=7, denoise=True, norm=True, subpixel=subpixel, select_peaks=True)
    plain = lp.get_local_extrema_points(g32["r7_rows"][:4].astype(dtype), option="max", radius=7, denoise=True, norm=True, subpixel=subpixel)
    for a, b in zip(prepared, plain):
        assert np.isin(a, b).all()                            # selection only removes
    # without the flag kwargs are ignored and the result is prep.linepattern's
    same = lc.get_local_extrema_points(src[:4], radius=7, denoise=False, norm=False, subpixel=subpixel, select_peaks=False, tol=1e-9, nonsense=3)
    for a, b in zip(same, lp.get_local_extrema_points(src[:4], radius=7, denoise=False, norm=False, subpixel=subpixel)):
        assert same_bits(a, b)


def test_cross_points_and_slopes_with_the_flag(hip, lc):
    """Golden G27's line image and G28's: with the flag every returned point is, bit for bit, a point of the call without it (selection
    only removes); an array and a device tensor give the same points within 1e-6 pixel; the slope does not depend on the flag (it comes from the sinogram)."""
    import torch
    g27, g28 = golden("g27_cross_points"), golden("g28_slope_distance")
    img, slope = g27["img_line"], float(g27["slope"])
    for fn in (lc.get_cross_points_hor_lines, lc.get_cross_points_ver_lines):
        plain = fn(img, slope, 20.0)
        for kw in ({}, dict(tol=0.3, use_offset=False)):
            picked = fn(img, slope, 20.0, select_peaks=True, **kw)
            assert picked.ndim == 2 and picked.shape[1] == 2 and 0 < len(picked) <= len(plain)
            assert {p.tobytes() for p in picked} <= {p.tobytes() for p in plain}
            on_device = fn(torch.from_numpy(img).to("cuda:0"), slope, 20.0, select_peaks=True, **kw)
            assert on_device.shape == picked.shape and np.abs(on_device - picked).max() <= 1e-6
            print("%s %s: %d of %d points" % (fn.__name__, kw, len(picked), len(plain)))
    for fn in (lc.calc_slope_distance_hor_lines, lc.calc_slope_distance_ver_lines):
        slope0, dist0 = fn(g28["img_line"], ratio=0.9, search_range=5, radius=5)
        slope1, dist1 = fn(g28["img_line"], ratio=0.9, search_range=5, radius=5, select_peaks=True)
        print("%s: slope %r distance %r, with the flag %r" % (fn.__name__, slope0, dist0, dist1))
        assert slope1 == slope0 and np.isfinite(dist0)


# --------------------------------------------------------------------------- 5: the reference itself (golden G33)

CAP = 1e-6                   # pixel: the position tolerance of tests/test_cross_points_gpu.py


@pytest.fixture(scope="module")
def g33():
    g = golden("g33_select_wired")
    for v in g.values():
        v.setflags(write=False)
    return g


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_wrapper_returns_the_references_positions_on_clear_rows(hip, lc, g33, dtype):
    e_sub = float(golden("g27_cross_points")["e_sub"])
    case = g33["tb_case"]
    case = case[case[:, 3] == (1 if dtype == "float32" else 0)]
    rows = g33["tb_rows"].astype(dtype)
    compared = unclear_rows = 0
    worst = 0.0
    groups = sorted({tuple(int(v) for v in c[[1, 2, 4, 5]]) for c in case})
    assert len(groups) == 12
    for radius, k, dn, nm in groups:
        members = case[(case[:, 1] == radius) & (case[:, 2] == k) & (case[:, 4] == dn) & (case[:, 5] == nm)]
        kw = dict(tol=float(g33["kw_tol"][k]), sigma=float(g33["kw_sigma"][k]), use_offset=bool(g33["kw_use_offset"][k]))
        args = dict(option="max", radius=radius, denoise=bool(dn), norm=bool(nm), select_peaks=True, **kw)
        batch = rows[members[:, 0]]
        ints = lc.get_local_extrema_points(batch, subpixel=False, **args)
        subs = lc.get_local_extrema_points(batch, subpixel=True, **args)
        assert isinstance(ints, list) and len(ints) == len(subs) == len(members)
        for j, (row, _, _, _, _, _, first, n, rfirst, rn, all_clear) in enumerate(members):
            for got in (ints[j], subs[j]):
                assert isinstance(got, np.ndarray) and got.ndim == 1
            assert len(ints[j]) == len(subs[j]) and subs[j].dtype == np.float64 and ints[j].dtype == (np.int64 if len(ints[j]) else np.float64)
            if not all_clear:
                unclear_rows += 1
                continue
            want_int, want_sub = g33["tb_int"][rfirst:rfirst + rn], g33["tb_sub"][rfirst:rfirst + rn]
            assert np.array_equal(ints[j], want_int), (radius, k, dn, nm, int(row), ints[j], want_int)
            if rn:
                worst = max(worst, float(np.abs(subs[j] - want_sub).max()))
            else:
                assert ints[j].shape == (0,) and subs[j].shape == (0,)             # np.asarray([]), as the reference returns
            compared += 1
        # a batch call equals row-by-row calls
        for j in (0, len(members) // 2, len(members) - 1):
            assert same_bits(lc.get_local_extrema_points(batch[j], subpixel=True, **args), subs[j])
            assert same_bits(lc.get_local_extrema_points(batch[j], subpixel=False, **args), ints[j])
    print("%s: %d rows compared with the reference, %d rows with an unclear candidate left out; largest sub-pixel deviation %.3g (e_sub %.3g)" % (
        dtype, compared, unclear_rows, worst, e_sub))
    assert compared >= 100 and worst <= 4 * e_sub


def image_of(g33, key):
    if key == "wide":
        return g33["img_wide"]
    return golden("g28_slope_distance")["img_big"] if key == "big" else golden("g27_cross_points")["img_" + key]


@pytest.mark.parametrize("key", ["line", "tall", "big", "wide"])
def test_cross_points_with_the_flag_against_the_reference(hip, lc, g33, key):
    import torch
    img = image_of(g33, key)
    names = list(g33["im_names"])
    for fn_name, fn in (("hor", lc.get_cross_points_hor_lines), ("ver", lc.get_cross_points_ver_lines)):
        for k in (0, 1):
            idx = names.index("%s_%s_%d" % (key, fn_name, k))
            _, first, n, judged, n_unclear, n_plain = (int(v) for v in g33["im_case"][idx])
            want = g33["im_pts"][first:first + n]
            slope, dist = float(np.tan(np.deg2rad(g33["im_slope_deg"][idx]))), float(g33["im_dist"][idx])
            kw = dict(tol=float(g33["kw_tol"][k]), use_offset=bool(g33["kw_use_offset"][k])) if k else {}
            plain = fn(img, slope, dist)
            got = fn(img, slope, dist, select_peaks=True, **kw)
            assert len(plain) == n_plain == judged and got.ndim == 2 and got.shape[1] == 2
            # selection only removes: every point is, bit for bit, a point of the call without the flag
            assert {p.tobytes() for p in got} <= {p.tobytes() for p in plain} and len({p.tobytes() for p in got}) == len(got)
            # matched to the reference's points within the position tolerance, the two sets differ by unclear candidates at most
            near = (np.abs(got[:, None, :] - want[None, :, :]).max(axis=2) <= CAP) if len(got) and len(want) else np.zeros((len(got), len(want)), bool)
            assert (near.sum(axis=0) <= 1).all() and (near.sum(axis=1) <= 1).all()
            differ = int((~near.any(axis=1)).sum() + (~near.any(axis=0)).sum())
            print("%s %s kwargs %d: %d points (reference %d) of %d, %d differ, %d unclear" % (key, fn_name, k, len(got), len(want), n_plain, differ, n_unclear))
            assert differ <= n_unclear
            # a device tensor gives the same points: as many, in the same order, each within the position tolerance (the steps in front
            # of the profiles are torch's there and agree with NumPy's to rounding, as without the flag, tests/test_cross_points_gpu.py)
            dev = fn(torch.from_numpy(np.array(img)).to("cuda:0"), slope, dist, select_peaks=True, **kw)
            assert isinstance(dev, np.ndarray) and dev.shape == got.shape
            apart = float(np.abs(dev - got).max()) if len(got) else 0.0
            print("%s %s kwargs %d tensor input: %d points, largest deviation from the array's %.3g pixel" % (key, fn_name, k, len(dev), apart))
            assert apart <= CAP


def test_slope_and_distance_with_the_flag_against_the_reference(hip, lc, g33):
    import json
    g28 = golden("g28_slope_distance")
    checked = 0
    for name, (slope, dist, all_clear, ncand, nkept) in zip(g33["sd_names"], g33["sd_vals"]):
        name = str(name)
        mat, prepare, kw = g28["img_" + str(g28["image_" + name])], str(g28["prepare_" + name]), json.loads(str(g28["args_" + name]))
        if prepare == "invert":
            mat = mat.max() - mat
        if prepare == "float64":
            mat = mat.astype(np.float64)
        fn = lc.calc_slope_distance_hor_lines if name.endswith("_hor") else lc.calc_slope_distance_ver_lines
        with np.errstate(all="ignore"):
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                got_slope, got_dist = fn(mat, select_peaks=True, **kw)
        print("%-12s slope %+.7f (reference %+.7f) distance %r (reference %r), %d of %d candidates kept there, all clear %s" % (
            name, got_slope, slope, got_dist, dist, nkept, ncand, bool(all_clear)))
        if not all_clear:
            continue
        assert got_slope == slope
        assert (np.isnan(got_dist) and np.isnan(dist)) or abs(got_dist - dist) <= CAP
        checked += np.isfinite(dist)
    assert checked >= 2
