"""GPU suite for the selection of good peaks (prep.linepattern.select_good_peaks, dcp_select_peaks_rows, select_peaks_kernel of
csrc/select_peaks_kernels.hip) against the reference's own decisions, golden G32 (tools/gen_golden.py): per candidate the reference's
decision with and without use_offset, its four values (check, c, d, num) and the same from a refit at tolerances of 1e-14, for float64
rows and for the same rows as float32.  A candidate is CLEAR where the two fits decide alike and every criterion of a fit that
succeeded keeps `delta` from its threshold (delta: four times the 99th percentile of the difference between the two fits).  On clear
candidates the decision must be the reference's; unclear ones may go either way and are counted against the 15 % the generator
promised.  Rows synthesised from the model itself must come back with their parameters; a candidate's fit must not depend on the
call it is in; strided planes, device tensors and NumPy arrays must agree bit for bit."""
import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu

I32 = None
STATUS = dict(ok=0, short=1, not_finite=2, constant=3, budget=4, diverged=5, gradient=6)


@pytest.fixture(scope="module")
def lp(hip):
    from discorpy_amd.prep import linepattern
    return linepattern


@pytest.fixture(scope="module")
def g32():
    g = golden("g32_select_peaks")
    for v in g.values():
        v.setflags(write=False)
    return g


def select(hip, rows, peak_row, peak_idx, radius, tol=0.2, use_offset=True, view=None):
    """(keep, fit) of one call on host memory; view: (pointer, row stride) of the plane where it is not `rows` itself."""
    i32p = hip.C.POINTER(hip.C.c_int32)
    peak_row, peak_idx = np.ascontiguousarray(peak_row, np.int32), np.ascontiguousarray(peak_idx, np.int32)
    n = len(peak_idx)
    keep, fit = np.full(n + 8, 0xA5, np.uint8), np.full((n + 1, 6), -12345.0)
    ptr, stride = (rows.ctypes.data, rows.shape[1]) if view is None else view
    hip.check(hip.lib().dcp_select_peaks_rows(ptr, rows.shape[0], rows.shape[1], stride, hip.DTYPE_BY_NAME[rows.dtype.name], peak_row.ctypes.data_as(i32p),
                                              peak_idx.ctypes.data_as(i32p), n, radius, tol, int(use_offset), keep.ctypes.data, fit.ctypes.data,
                                              hip.MEM_HOST, -1, None))
    assert (keep[n:] == 0xA5).all() and (fit[n] == -12345.0).all() and set(np.unique(keep[:n]).tolist()) <= {0, 1}
    return keep[:n].astype(bool), fit[:n]


def case_of(g, lp, name, dtype):
    """(rows as the kernel gets them, row of every candidate, its index, radius, tol) of one case of the golden."""
    k = list(g["case_names"]).index(name)
    rows = np.ascontiguousarray(g[name + "_rows"].astype(dtype))
    if g["sigma"][k] > 0:
        rows = lp.gaussian_filter(rows, (0, float(g["sigma"][k])))
    return rows, g[name + "_row_of"], g[name + "_idx"], int(g["radius"][k]), float(g["tol"][k])


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# --------------------------------------------------------------------------- 1, 5: the reference's decisions

@pytest.mark.parametrize("use_offset", [True, False])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_decisions_are_the_references_on_every_clear_peak(hip, lp, g32, dtype, use_offset):
    key, col = "f64" if dtype == "float64" else "f32", 0 if use_offset else 1
    clear_n = unclear_n = total = 0
    wrong = []
    for name in g32["case_names"]:
        if name == "big":
            continue
        rows, row_of, idx, radius, tol = case_of(g32, lp, name, dtype)
        keep, fit = select(hip, rows, row_of, idx, radius, tol, use_offset)
        want, clear = g32["%s_%s_keep" % (name, key)][:, col], g32["%s_%s_clear" % (name, key)][:, col]
        status = fit[:, 5].astype(np.int64)
        assert ((status >= 0) & (status <= 6)).all() and np.isfinite(fit[keep]).all() and (status[keep] == 0).all()
        for i in np.flatnonzero(clear & (keep != want)):
            wrong.append((str(name), int(i), int(row_of[i]), int(idx[i]), bool(keep[i]), fit[i].tolist(), g32["%s_%s_ref" % (name, key)][i].tolist()))
        clear_n += int(clear.sum())
        unclear_n += int((~clear).sum())
        total += len(idx)
        print("%-7s %s use_offset=%s: %d candidates, %d kept (reference %d), %d unclear of which %d decided otherwise, status counts %s" % (
            name, dtype, use_offset, len(idx), keep.sum(), want.sum(), (~clear).sum(), (~clear & (keep != want)).sum(),
            np.bincount(status, minlength=7).tolist()))
    print("clear %d, unclear %d of %d (%.2f %%), wrong decisions on clear candidates: %d" % (clear_n, unclear_n, total, 100.0 * unclear_n / total,
                                                                                           len(wrong)))
    assert unclear_n <= 0.15 * total
    assert not wrong, wrong[:5]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_largest_window(hip, lp, g32, dtype):
    """Radius 128 on the row of 600 samples: windows of 257 samples in the interior, clipped ones near both ends."""
    key = "f64" if dtype == "float64" else "f32"
    rows, row_of, idx, radius, tol = case_of(g32, lp, "big", dtype)
    assert radius == 128 and rows.shape == (1, 600) and idx.min() < 128 and idx.max() > 600 - 129
    for col, use_offset in enumerate((True, False)):
        keep, fit = select(hip, rows, row_of, idx, radius, tol, use_offset)
        want, clear = g32["big_%s_keep" % key][:, col], g32["big_%s_clear" % key][:, col]
        print("radius 128 %s use_offset=%s: kept %d of %d (reference %d), clear %d, status %s" % (dtype, use_offset, keep.sum(), len(idx), want.sum(),
                                                                                                 clear.sum(), fit[:, 5].astype(int).tolist()))
        assert clear.sum() >= 12 and want[clear].any() and not want[clear].all()
        assert np.array_equal(keep[clear], want[clear])
        assert (fit[keep, 5] == 0).all() and np.isfinite(fit[keep]).all()


# --------------------------------------------------------------------------- 2: recovery of exact data

def model(x, a, b, c, d):
    return a * np.exp(-((x - c) / (2 * b ** 2)) ** 2) + d


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_rows_made_from_the_model_come_back(hip, dtype):
    """A line a exp(-((x - c) / (2 b^2))^2) + d around sample `centre`; windows clipped at the row's start and end and whole in the
    interior, with even and odd numbers of samples.  The normalisation keeps b, moves c to the window's own origin (x_i = i - n // 2)
    and maps d to (d - min) / std: fit returns those within 1e-6 (an origin off by one sample would be off by 1; by half, 0.5)."""
    length, radius = 48, 7
    x = np.arange(length, dtype=np.float64)
    # (centre of the line, candidate): start-clipped with n = 10, 11 and 12, interior with n = 15, end-clipped with n = 12, 11 and 10
    cases = [(2.3, 2), (3.4, 3), (3.8, 4), (20.25, 20), (24.0, 24), (27.6, 28), (43.7, 43), (44.4, 44), (45.2, 45)]
    rows = np.stack([model(x, 2.5 + 0.1 * k, 1.1 + 0.03 * k, centre, 0.7 - 0.1 * k) for k, (centre, _) in enumerate(cases)]).astype(dtype)
    peaks = np.array([p for _, p in cases])
    keep, fit = select(hip, rows, np.arange(len(cases)), peaks, radius, 0.2, True)
    sizes = set()
    for k, (centre, p) in enumerate(cases):
        start, stop = max(0, p - radius), min(length, p + radius + 1)
        n = stop - start
        sizes.add(n)
        w = rows[k, start:stop].astype(np.float64)
        # the parameters of the window's own least-squares problem: exact for float64 rows; for float32 rows the data carry 6e-8
        # of rounding, which moves the minimum by about that much
        want_c, want_d, want_b = centre - start - n // 2, (0.7 - 0.1 * k - w.min()) / w.std(), 1.1 + 0.03 * k
        print("n %2d start %2d: status %d c %.9f (want %.9f) d %.9f (want %.9f) b %.9f num %.3g" % (n, start, fit[k, 5], fit[k, 2], want_c, fit[k, 3],
                                                                                                   want_d, fit[k, 1], fit[k, 4]))
        assert fit[k, 5] == 0 and abs(fit[k, 2] - want_c) <= 1e-6 and abs(fit[k, 3] - want_d) <= 1e-6 and abs(abs(fit[k, 1]) - want_b) <= 1e-6
        assert fit[k, 4] <= 1e-6 and keep[k] == (abs(fit[k, 2]) < radius // 2 and abs(fit[k, 3]) < 0.2)
    assert sizes == {10, 11, 12, 15}


# --------------------------------------------------------------------------- 3: independence

def test_a_fit_does_not_depend_on_the_call_it_is_in(hip, lp, g32):
    rows = np.concatenate([g32["r7_rows"], g32["h7_rows"]])                     # 27 rows: lines, noise, a ramp, a square wave
    row_of = np.concatenate([g32["r7_row_of"], g32["h7_row_of"] + 24])
    idx = np.concatenate([g32["r7_idx"], g32["h7_idx"]])
    order = np.random.default_rng(3).permutation(len(idx))
    row_of, idx = np.resize(row_of[order], 1000), np.resize(idx[order], 1000)      # good and hopeless candidates, mixed
    keep_all, fit_all = select(hip, rows, row_of, idx, 7)
    status = fit_all[:, 5].astype(np.int64)
    assert (status == 0).sum() > 300 and (status == STATUS["constant"]).sum() > 5 and (status == STATUS["budget"]).sum() > 5 and 100 < keep_all.sum() < 900
    # a second run, and the batch reversed: every candidate's row of `fit`, bit for bit
    keep_2, fit_2 = select(hip, rows, row_of, idx, 7)
    assert same_bits(fit_2, fit_all) and np.array_equal(keep_2, keep_all)
    keep_r, fit_r = select(hip, rows, row_of[::-1], idx[::-1], 7)
    assert same_bits(np.ascontiguousarray(fit_r[::-1]), fit_all) and np.array_equal(keep_r[::-1], keep_all)
    # one good and one hopeless candidate: alone, and as candidate 0, 63, 64 and 65 of a batch (the last of a wave's block, the first of the next)
    for k in (int(np.flatnonzero(keep_all)[0]), int(np.flatnonzero(status == STATUS["budget"])[0])):
        keep_1, fit_1 = select(hip, rows, row_of[k:k + 1], idx[k:k + 1], 7)
        assert same_bits(fit_1[0], fit_all[k]) and keep_1[0] == keep_all[k]
        for slot in (0, 63, 64, 65):
            r, i = row_of[:130].copy(), idx[:130].copy()
            r[slot], i[slot] = row_of[k], idx[k]
            keep_s, fit_s = select(hip, rows, r, i, 7)
            assert same_bits(fit_s[slot], fit_all[k]) and keep_s[slot] == keep_all[k], (k, slot)


# --------------------------------------------------------------------------- 4: row strides and containers

@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_strided_rows_device_tensors_and_numpy_arrays_agree(hip, lp, g32, dtype):
    import torch
    rows, row_of, idx, radius, tol = case_of(g32, lp, "r11", dtype)
    rows, keepers = rows[:6], np.flatnonzero(row_of < 6)
    row_of, idx = row_of[keepers], idx[keepers]
    keep, fit = select(hip, rows, row_of, idx, radius, tol)
    assert 0 < keep.sum() < len(keep)
    # the rows as the [:, 5:5 + L] view of a wider buffer whose margins would spoil every clipped window
    buf = np.empty((rows.shape[0], rows.shape[1] + 13), rows.dtype)
    buf[:, :5], buf[:, 5 + rows.shape[1]:] = np.nan, 1e30
    buf[:, 5:5 + rows.shape[1]] = rows
    keep_v, fit_v = select(hip, rows, row_of, idx, radius, tol, view=(buf[:, 5:].ctypes.data, buf.shape[1]))
    assert same_bits(fit_v, fit) and np.array_equal(keep_v, keep)
    # the same view in device memory, the outputs there too, on a stream of its own
    i32p = hip.C.POINTER(hip.C.c_int32)
    n = len(idx)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        dbuf = torch.from_numpy(buf).to("cuda:0")
        dkeep = torch.full((n + 8,), 0xA5, dtype=torch.uint8, device="cuda:0")
        dfit = torch.full((n + 1, 6), -12345.0, dtype=torch.float64, device="cuda:0")
        hip.check(hip.lib().dcp_select_peaks_rows(dbuf[:, 5:].data_ptr(), rows.shape[0], rows.shape[1], dbuf.stride(0), hip.DTYPE_BY_NAME[dtype],
                                                  np.ascontiguousarray(row_of, np.int32).ctypes.data_as(i32p),
                                                  np.ascontiguousarray(idx, np.int32).ctypes.data_as(i32p), n, radius, tol, 1, dkeep.data_ptr(),
                                                  dfit.data_ptr(), hip.MEM_DEVICE, 0, stream.cuda_stream))
    stream.synchronize()
    hkeep, hfit = dkeep.cpu().numpy(), dfit.cpu().numpy()
    assert (hkeep[n:] == 0xA5).all() and (hfit[n] == -12345.0).all()
    assert same_bits(np.ascontiguousarray(hfit[:n]), fit) and np.array_equal(hkeep[:n].astype(bool), keep)
    # fit may be null
    with torch.cuda.stream(stream):
        dkeep.fill_(0xA5)
        hip.check(hip.lib().dcp_select_peaks_rows(dbuf[:, 5:].data_ptr(), rows.shape[0], rows.shape[1], dbuf.stride(0), hip.DTYPE_BY_NAME[dtype],
                                                  np.ascontiguousarray(row_of, np.int32).ctypes.data_as(i32p),
                                                  np.ascontiguousarray(idx, np.int32).ctypes.data_as(i32p), n, radius, tol, 1, dkeep.data_ptr(),
                                                  None, hip.MEM_DEVICE, 0, stream.cuda_stream))
    stream.synchronize()
    assert np.array_equal(dkeep.cpu().numpy()[:n].astype(bool), keep)
    # the wrapper: a tensor, a NumPy array and a list give the same selection
    per_row = [idx[row_of == r].astype(np.int64) for r in range(rows.shape[0])]
    want = [p[keep[row_of == r]] for r, p in enumerate(per_row)]
    for data in (rows, torch.from_numpy(rows).to("cuda:0"), rows.tolist() if dtype == "float64" else rows):
        got = lp.select_good_peaks(data, per_row, tol=tol, radius=radius)
        assert len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))


# --------------------------------------------------------------------------- 6: hopeless rows

def test_hopeless_rows_come_back_with_a_status(hip, lp, g32):
    seen = set()
    for name in ("h3", "h7"):
        rows, row_of, idx, radius, tol = case_of(g32, lp, name, "float64")
        keep, fit = select(hip, rows, row_of, idx, radius, tol)
        status = fit[:, 5].astype(np.int64)
        assert (status == fit[:, 5]).all() and ((status >= 0) & (status <= 6)).all()
        assert np.isfinite(fit[keep]).all() and (status[keep] == 0).all()
        assert np.isfinite(fit[status == 0]).all() and np.isnan(fit[status != 0][:, 4]).all() and np.isnan(fit[(status >= 1) & (status <= 3)][:, :5]).all()
        # the square wave (row 2): a window inside one of its flat stretches is constant, and no other window of these rows is
        const = np.array([np.ptp(rows[r, max(0, p - radius):p + radius + 1]) == 0 for r, p in zip(row_of, idx)])
        assert const.any() and np.array_equal(status == STATUS["constant"], const) and (row_of[const] == 2).all()
        seen |= set(status.tolist())
        print("%s: status counts %s, kept %d" % (name, np.bincount(status, minlength=7).tolist(), keep.sum()))
    assert {STATUS["ok"], STATUS["constant"], STATUS["budget"]} <= seen
    # radius 1: windows of 2 samples at the ends, of 3 elsewhere -- none is fitted
    rows, row_of, idx, _, tol = case_of(g32, lp, "h7", "float32")
    keep, fit = select(hip, rows, row_of, idx, 1, tol)
    assert not keep.any() and (fit[:, 5] == STATUS["short"]).all() and np.isnan(fit[:, :5]).all()
    # radius 2: 5 samples in the interior (fitted or constant), 3 at index 0 (row_of, idx hold it for every row)
    keep, fit = select(hip, rows, row_of, idx, 2, tol)
    assert (idx == 0).sum() == 3 and (fit[idx == 0, 5] == STATUS["short"]).all() and (fit[idx > 1, 5] != STATUS["short"]).all()
    # a NaN or an infinity anywhere in the window, and only there
    for bad in (np.nan, np.inf, -np.inf):
        spoiled = rows.copy()
        spoiled[0, 40] = bad
        keep, fit = select(hip, spoiled, row_of, idx, 7, tol)
        hit = (row_of == 0) & (np.abs(idx - 40) <= 7)
        assert hit.sum() >= 2 and np.array_equal(fit[:, 5] == STATUS["not_finite"], hit) and not keep[hit].any()


# --------------------------------------------------------------------------- 7: the wrapper

def reference_selection(g, name, key, use_offset):
    """Per row of a case: (its candidates, the reference's selection, whether every candidate of the row is clear)."""
    col = 0 if use_offset else 1
    row_of, idx = g[name + "_row_of"], g[name + "_idx"].astype(np.int64)
    keep, clear = g["%s_%s_keep" % (name, key)][:, col], g["%s_%s_clear" % (name, key)][:, col]
    out = []
    for r in range(g[name + "_rows"].shape[0]):
        m = row_of == r
        out.append((idx[m], idx[m][keep[m]], bool(clear[m].all())))
    return out


def assert_selection(got, want):
    """np.asarray(good_peaks) of the reference: the candidates' integer type, or the empty float64 array where none is good."""
    assert isinstance(got, np.ndarray) and got.ndim == 1
    if len(want) == 0:
        assert got.shape == (0,) and got.dtype == np.float64
    else:
        assert got.dtype == want.dtype and np.array_equal(got, want), (got, want)


@pytest.mark.parametrize("use_offset", [True, False])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_wrapper_selects_what_the_reference_selects(hip, lp, g32, dtype, use_offset):
    key = "f64" if dtype == "float64" else "f32"
    names = list(g32["case_names"])
    checked = 0
    for name in ("r7", "r11", "smooth", "vec2"):
        k = names.index(name)
        kw = dict(tol=float(g32["tol"][k]), radius=int(g32["radius"][k]), sigma=float(g32["sigma"][k]), use_offset=use_offset)
        rows = g32[name + "_rows"].astype(dtype)
        per_row = reference_selection(g32, name, key, use_offset)
        sure = [r for r, (_, _, clear) in enumerate(per_row) if clear]
        assert sure, name
        # one profile at a time: the first three rows whose candidates are all clear
        for r in sure[:3]:
            assert_selection(lp.select_good_peaks(rows[r], per_row[r][0], **kw), per_row[r][1])
        # the batch, with an empty row among the full ones
        cands = [c for c, _, _ in per_row]
        if len(cands) > 2:
            cands[1] = np.zeros(0, np.int64)
        got = lp.select_good_peaks(rows, cands, **kw)
        assert isinstance(got, list) and len(got) == len(per_row)
        for r in sure:
            assert_selection(got[r], per_row[r][1] if len(cands[r]) else np.zeros(0, np.int64))
        if len(cands) > 2:
            assert got[1].shape == (0,) and got[1].dtype == np.float64
        checked += len(sure)
        print("%-6s %s use_offset=%s: %d of %d rows have only clear candidates" % (name, dtype, use_offset, len(sure), len(per_row)))
    assert checked >= 8
    # other element types are read as float64 before everything: integers give what their float64 copy gives
    ints = np.round(200.0 * g32["r7_rows"][:4]).astype(np.int32)
    cands = [c for c, _, _ in reference_selection(g32, "r7", key, use_offset)[:4]]
    for sigma in (0, 1.5):
        a = lp.select_good_peaks(ints, cands, radius=7, sigma=sigma, use_offset=use_offset)
        b = lp.select_good_peaks(ints.astype(np.float64), cands, radius=7, sigma=sigma, use_offset=use_offset)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_the_references_own_test_vectors(hip, lp, g32):
    """tests/test_linepattern.py:53-67 of the reference.  The second vector is clear; the first one's first peak fits a shift of
    -0.99999919 against a limit of 1 (the golden marks it unclear), so only its second peak is asserted."""
    got = lp.select_good_peaks(np.array([0, 1, 2, 9, 2, 1, 0, 0, 3, 10, 3, 0, 0], np.float64), np.asarray([3, 9]), tol=0.3, radius=3, sigma=1)
    assert g32["vec2_f64_clear"].all() and np.array_equal(got, [3, 9]) and got.dtype == np.asarray([3, 9]).dtype
    got = lp.select_good_peaks(np.array([0, 1.5, 5, 1.5, 0, 0, 3, 10, 3, 0]), np.asarray([2, 7]), tol=0.1, radius=3, sigma=0)
    clear = g32["vec1_f64_clear"][:, 0]
    print("first vector: selected %s, clear %s, the reference's values %s" % (got, clear.tolist(), g32["vec1_f64_ref"].tolist()))
    assert not clear[0] and clear[1] and 7 in got and set(got.tolist()) <= {2, 7}
