"""GPU suite that attacks the structure of peak_rows_kernel and window_slope_kernel (csrc/profile_kernels.hip) with the rows of
tests/helpers/peak_cases.py: rows of one to five steps with minima on every step's first and last sample, steps in which every
sample is a candidate, tails of every length at which NumPy's pairwise sum takes another path with thresholds one ulp away, and
special values.  The oracle is tests/helpers/peaks_reference.py, which tests/test_peak_rows_cpu.py holds to NumPy on these rows.
Every comparison is exact: integer positions as sets, sub-pixel positions and slopes bit for bit.  The entry points are also called
directly: row-strided planes in host and in device memory, a radius of 0 that fills a row of the output to its cap, the grid's
limit of 65535 rows."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import peak_cases as PC  # noqa: E402
import peaks_reference as PR  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0


@pytest.fixture(scope="module")
def lp(hip):
    from discorpy_amd.prep import linepattern
    return linepattern


def search(lp, rows, radius, sensitive, subpixel):
    return lp.get_local_extrema_points(rows, radius=radius, sensitive=sensitive, denoise=False, norm=False, subpixel=subpixel)


@pytest.mark.parametrize("kind", list(PC.BUILDERS))
@pytest.mark.parametrize("dtype", PC.DTYPES)
def test_wrapper_equals_the_oracle_on_every_row(lp, dtype, kind):
    rows = PC.BUILDERS[kind](dtype)
    points = 0
    for k, (row, radius, sensitive) in enumerate(rows):
        want = PC.expected_positions(kind, dtype, k)
        ints = search(lp, row, radius, sensitive, False)
        assert set(ints.tolist()) == set(want.tolist()) and len(ints) == len(want), (kind, k, len(row), radius, sensitive, ints, want)
        subs = search(lp, row, radius, sensitive, True)
        assert np.array_equal(subs, PR.refine(row, want)), (kind, k, len(row), radius, sensitive)
        points += len(want)
    print("%s rows, %s: %d rows, %d points" % (kind, dtype, len(rows), points))
    assert points > 0


@pytest.mark.parametrize("dtype", PC.DTYPES)
def test_constructed_and_crowded_rows_give_what_their_builders_say(lp, dtype):
    for (row, radius, sensitive), expected in PC.constructed_cases(dtype):
        assert np.array_equal(search(lp, row, radius, sensitive, False), expected), (radius, len(row))
    for row, radius, sensitive in PC.crowded_rows(dtype):
        if not (row == 3.0).all():
            continue
        lo, hi = PC.search_range(len(row), radius)
        ints, subs = search(lp, row, radius, sensitive, False), search(lp, row, radius, sensitive, True)
        if sensitive > 0:                             # 256 candidates in every full step, num2 exactly 0: no point
            assert len(ints) == 0 and len(subs) == 0
        else:                                         # every searched sample; a flat triple takes the argmin, its first sample
            assert np.array_equal(ints, np.arange(lo, hi)) and np.array_equal(subs, np.arange(lo, hi) - 1.0), (radius, sensitive)


def groups_of(rows):
    """The rows of one (length, radius, threshold and its kind), in their order."""
    out = {}
    for k, (row, radius, sensitive) in enumerate(rows):
        out.setdefault((len(row), radius, type(sensitive).__name__, float(sensitive)), []).append(k)
    return out


@pytest.mark.parametrize("kind", ["step", "ladder"])
@pytest.mark.parametrize("dtype", PC.DTYPES)
def test_batches_of_rows(lp, dtype, kind):
    """The rows of one (length, radius, threshold) in one call; and one row of every (length, radius) 73 times, rolled by 7 j, of which
    rows 0, 1, 36 and 72 are compared."""
    rows = PC.BUILDERS[kind](dtype)
    groups = groups_of(rows)
    if kind == "step":                                # the cosine row of every (radius, span)
        rolled = [4 * g + 1 for g in range(len(PC.STEP_RADII) * len(PC.STEP_SPANS))]
    else:                                             # every radius at its median threshold
        rolled = [k for k, (_, radius, s) in enumerate(rows) if type(s) is float and s == float(PC.ladder_thresholds(radius, dtype)[2][1])]
        assert len(rolled) == len(PC.LADDER_RADII)
    for key, members in groups.items():
        radius, sensitive = rows[members[0]][1:]
        got = search(lp, np.stack([rows[k][0] for k in members]), radius, sensitive, True)
        assert isinstance(got, list) and len(got) == len(members)
        for k, g in zip(members, got):
            assert np.array_equal(g, PR.refine(rows[k][0], PC.expected_positions(kind, dtype, k))), (key, k)
    for k in rolled:
        row, radius, sensitive = rows[k]
        key = (len(row), radius)
        stack = np.stack([np.roll(row, 7 * j) for j in range(73)])
        got = search(lp, stack, radius, sensitive, False)
        assert len(got) == 73 and np.array_equal(got[0], PC.expected_positions(kind, dtype, k)), key
        for j in (1, 36, 72):
            assert np.array_equal(got[j], PR.local_minima(stack[j], radius, sensitive)), (key, j)


# --------------------------------------------------------------------------- the entry points, called directly

def margin_buffer(rows):
    """``rows`` as the ``[:, 5:5 + L]`` view of an (N, L + 13) buffer whose margins are NaN in front and -1e30 behind."""
    n, length = rows.shape
    buf = np.empty((n, length + 13), rows.dtype)
    buf[:, :5] = np.nan
    buf[:, 5 + length:] = -1e30
    buf[:, 5:5 + length] = rows
    return buf


def extrema_host(hip, src, nrows, length, stride, radius, sensitive, subpixel):
    dst = np.full((nrows + 1, length), SENTINEL)      # one guard row behind the plane
    hip.check(hip.lib().dcp_local_extrema_rows(src.ctypes.data, dst.ctypes.data, nrows, length, stride, hip.DTYPE_BY_NAME[src.dtype.name], radius,
                                               sensitive, subpixel, hip.MEM_HOST, -1, None))
    assert (dst[nrows] == SENTINEL).all()
    return dst[:nrows]


def extrema_device(hip, torch, src, nrows, length, radius, sensitive, subpixel):
    """``src``: the margin buffer; the kernel reads the view in place on a stream of its own.  (dst, what dst held before)."""
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        buf = torch.from_numpy(src).to("cuda:0")
        view = buf[:, 5:5 + length]
        dst = torch.full((nrows + 1, length), SENTINEL, dtype=torch.float64, device="cuda:0")
        hip.check(hip.lib().dcp_local_extrema_rows(view.data_ptr(), dst.data_ptr(), nrows, length, buf.stride(0), hip.DTYPE_BY_NAME[src.dtype.name],
                                                   radius, sensitive, subpixel, hip.MEM_DEVICE, 0, stream.cuda_stream))
    stream.synchronize()
    out = dst.cpu().numpy()
    assert (out[nrows] == SENTINEL).all()
    return out[:nrows]


def found(dst):
    return [dst[r, :int(dst[r, -1])] for r in range(len(dst))]


@pytest.mark.parametrize("nrows", [1, 2, 73])
@pytest.mark.parametrize("dtype", PC.DTYPES)
def test_strided_rows_through_the_entry_points(hip, lp, dtype, nrows):
    """src_row_stride > length, as host memory (the packed round trip) and as device memory on a stream of its own (read in place):
    the positions and slopes of the contiguous rows bit for bit, row r from row r alone, nothing written that is not a result."""
    torch = pytest.importorskip("torch")
    radius, span = 11, 513
    row = PC.step_rows(dtype)[4 * (len(PC.STEP_SPANS) * PC.STEP_RADII.index(radius) + PC.STEP_SPANS.index(span)) + 1][0]
    length = len(row)
    assert length == PC.step_length(radius, span)
    rows = np.stack([np.roll(row, 7 * j) for j in range(nrows)])
    buf = margin_buffer(rows)
    code = hip.DTYPE_BY_NAME[dtype]
    for subpixel in (0, 1):
        packed = found(extrema_host(hip, rows, nrows, length, length, radius, 0.1, subpixel))
        host = found(extrema_host(hip, buf[:, 5:], nrows, length, length + 13, radius, 0.1, subpixel))
        device = extrema_device(hip, torch, buf, nrows, length, radius, 0.1, subpixel)
        for r in sorted({0, 1, 36, 72} & set(range(nrows))):
            alone = found(extrema_host(hip, rows[r:r + 1], 1, length, length, radius, 0.1, subpixel))[0]
            ints = PR.local_minima(rows[r], radius, 0.1)
            assert len(ints) > 5 and np.array_equal(alone, PR.refine(rows[r], ints) if subpixel else ints.astype(np.float64)), r
            assert np.array_equal(packed[r], alone), r
        for r in range(nrows):
            count = len(packed[r])
            assert np.array_equal(host[r], packed[r]) and np.array_equal(device[r, :count], packed[r]) and device[r, -1] == count, (r, subpixel)
            assert (device[r, count:-1] == SENTINEL).all(), r          # (device memory: only the positions and their number are written)
    for size in (5, 255):
        want = np.stack([PR.window_slope(rows[r], size) for r in sorted({0, nrows - 1})])
        packed = np.full((nrows + 1, length), SENTINEL, dtype)
        hip.check(hip.lib().dcp_window_slope_rows(rows.ctypes.data, packed.ctypes.data, nrows, length, length, code, size, hip.MEM_HOST, -1, None))
        host = np.full((nrows + 1, length), SENTINEL, dtype)
        hip.check(hip.lib().dcp_window_slope_rows(buf[:, 5:].ctypes.data, host.ctypes.data, nrows, length, length + 13, code, size, hip.MEM_HOST, -1, None))
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            dbuf = torch.from_numpy(buf).to("cuda:0")
            ddst = torch.full((nrows + 1, length), SENTINEL, dtype=getattr(torch, dtype), device="cuda:0")
            hip.check(hip.lib().dcp_window_slope_rows(dbuf[:, 5:5 + length].data_ptr(), ddst.data_ptr(), nrows, length, dbuf.stride(0), code, size,
                                                      hip.MEM_DEVICE, 0, stream.cuda_stream))
        stream.synchronize()
        assert np.array_equal(packed[[0, nrows - 1]], want[[0, -1]]), size
        assert np.array_equal(host, packed) and np.array_equal(ddst.cpu().numpy(), packed), size
        assert (packed[nrows] == SENTINEL).all()


@pytest.mark.parametrize("length", [1, 2, 257, 600])
@pytest.mark.parametrize("dtype", PC.DTYPES)
def test_a_radius_of_0_fills_every_row_to_its_cap(hip, dtype, length):
    """radius 0, no refinement, sensitive -1: every sample but the last is a point, 0 .. L - 2, and element L - 1 holds their number
    L - 1 -- the most a row of the output takes; the rows behind it and a guard row behind the plane stay what they were.  At
    sensitive 0 nothing is a point: the mean of a window of one sample is the sample, num2 is exactly 0."""
    torch = pytest.importorskip("torch")
    nrows = 3
    rows = (np.random.default_rng(2754).standard_normal((nrows, length)) + 3.0).astype(dtype)
    want = np.concatenate([np.arange(length - 1.0), [length - 1.0]])
    for r, got in enumerate(extrema_host(hip, rows, nrows, length, length, 0, -1.0, 0)):
        assert np.array_equal(got, want), (r, got)
    device = extrema_device(hip, torch, margin_buffer(rows), nrows, length, 0, -1.0, 0)
    for r in range(nrows):
        assert np.array_equal(device[r], want), (r, device[r])
    assert all(row[-1] == 0.0 for row in extrema_host(hip, rows, nrows, length, length, 0, 0.0, 0))
    device = extrema_device(hip, torch, margin_buffer(rows), nrows, length, 0, 0.0, 0)
    assert (device[:, -1] == 0.0).all() and (device[:, :-1] == SENTINEL).all()


@pytest.mark.parametrize("dtype", PC.DTYPES)
def test_window_slope_at_the_clamp_and_the_grid_limit(hip, lp, dtype):
    """Windows wider than the row is long on either side (255, 257 and 601 of 600 samples: the clamp works on both sides at once), rows
    of 3 and 4 samples, a row with a NaN and an inf, and 65535 rows, the most the grid takes: PR.window_slope bit for bit."""
    rng = np.random.default_rng(2755)
    rows = (rng.standard_normal((5, 600)) * 10.0 ** rng.integers(-3, 4, (5, 600))).astype(dtype)
    rows[4, 77], rows[4, 411] = np.nan, np.inf
    for size in (255, 257, 601):
        got = lp.sliding_window_slope(rows, size=size, norm=False)
        assert got.dtype == rows.dtype and got.shape == rows.shape
        with np.errstate(all="ignore"):
            for r in (0, 3, 4):
                want = PR.window_slope(rows[r], size)
                assert np.isnan(want).any() == (r == 4) and np.array_equal(got[r], want, equal_nan=True), (size, r)
    with np.errstate(all="ignore"):
        for size in (3, 11):
            assert np.array_equal(lp.sliding_window_slope(rows[4], size=size, norm=False), PR.window_slope(rows[4], size), equal_nan=True), size
    for n in (3, 4):
        short = rng.standard_normal((2, n)).astype(dtype)
        for size in (3, 5, 7):
            used = int(np.clip(size, 3, n))
            used += 1 - used % 2
            got = lp.sliding_window_slope(short, size=size, norm=False)
            for r in (0, 1):
                assert np.array_equal(got[r], PR.window_slope(short[r], used)), (n, size, r)
    many = rng.standard_normal((65535, 8)).astype(dtype)
    got = lp.sliding_window_slope(many, size=5, norm=False)
    assert got.shape == many.shape
    for r in (0, 32767, 65534):
        assert np.array_equal(got[r], PR.window_slope(many[r], 5)), r


def test_bounds_checking_build_counts_no_tap_in_crowded_and_five_step_rows():
    """libdiscorpy_hip_bounds.so in a process of its own (sites 40 - 42 of peak_rows_kernel): the crowded rows at radius 128 and the
    constructed rows of five steps at radii 1 and 128, both types, refined: the expected number of points, and nothing counted."""
    lib = os.path.join(ROOT, "discorpy_amd", "lib", "libdiscorpy_hip_bounds.so")
    assert os.path.exists(lib), "build() makes the bounds-checking library; it is missing"
    code = """
import sys, numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import peak_cases as PC, peaks_reference as PR
from discorpy_amd import _ffi as F
from discorpy_amd.prep import linepattern as lp
F.require_device()
assert F.debug_bounds()[4] == 1
done = 0
for dtype in PC.DTYPES:
    cases = [(c, len(PR.local_minima(*c))) for c in PC.crowded_rows(dtype) if c[1] == 128]
    for radius in (1, 128):
        for decoys in (True, False):
            row, expected = PC.constructed_row(radius, 1025, dtype, decoys)
            cases.append(((row, radius, 0.1), len(expected)))
    for (row, radius, sensitive), count in cases:
        if (row == 3.0).all():
            assert count == (0 if sensitive > 0 else len(row) - 2 * radius - 1)
        got = lp.get_local_extrema_points(row, radius=radius, sensitive=sensitive, denoise=False, norm=False, subpixel=True)
        assert len(got) == count, (dtype, radius, sensitive, len(got), count)
        done += 1
b = F.debug_bounds()
assert b[0] == 0 and b[4] == 1, b
print("bounds ok", done, b)
""" % (ROOT, os.path.join(ROOT, "tests", "helpers"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT, env=dict(os.environ, DCP_LIB_PATH=lib))
    assert r.returncode == 0 and "bounds ok 16" in r.stdout, (r.stdout + r.stderr)[-3000:]
