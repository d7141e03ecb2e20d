"""GPU suite for the grouping of dcp_tilted_profiles_2d (csrc/profile_kernels.hip: launch_tilted_profiles, the band kernels): a call
whose band planes exceed the 512 MiB of one group and is split by bytes, not by the 256 profiles of the band table; bands of unequal
size in one group; and a row-strided image as the source.  A profile of a batch equals the profile of a call of its own bit for bit;
against scipy.ndimage.map_coordinates on the reference's band the bounds are those of test_cross_points_gpu.test_tilted_profiles
(float32 on [0, 1) data within 1e-6; float64 rtol 1e-12, atol 1e-9)."""
import time

import numpy as np
import pytest
from scipy import ndimage as ndi

from test_cross_points_gpu import reference_line

pytestmark = pytest.mark.gpu

GROUP_BYTES = 512 << 20                               # kProfileWorkCap of csrc/api_profile.cpp: the band planes of one group
GROUP_MAX = 256                                       # kProfileGroupMax: the profiles of one band table
PAD = 12                                              # kBandPad: a band's plane is padded by 12 on every side


@pytest.fixture(scope="module")
def lp(hip):
    from discorpy_amd.prep import linepattern
    return linepattern


def close_to_scipy(profile, ref):
    dev = float(np.abs(profile.astype(np.float64) - ref).max())
    if profile.dtype == np.float32:
        assert np.abs(profile - ref).max() <= 1e-6, dev
    else:
        assert np.allclose(profile, ref, rtol=1e-12, atol=1e-9), dev
    return dev


def first_group(band_n, along):
    """How many profiles the first group takes: planes of (n + 24) (along + 24) doubles, closed before the plane that would not fit
    512 MiB, or at 256 profiles."""
    room, used, g = GROUP_BYTES // 8, 0, 0
    while g < min(len(band_n), GROUP_MAX) and used + (band_n[g] + 2 * PAD) * (along + 2 * PAD) <= room:
        used += (band_n[g] + 2 * PAD) * (along + 2 * PAD)
        g += 1
    return g


def split_by_bytes(lp, mat, direction, to_input, to_numpy):
    height, width = mat.shape
    along = width if direction == "horizontal" else height
    first, last = lp._calc_index_range(height, width, 0.1, direction)
    indices = np.linspace(first, last, 80)
    lines = [reference_line(height, width, index, 0.1, direction) for index in indices]
    band_n = [(band[0] if direction == "horizontal" else band[1]) for _, _, band, _ in lines]
    band_n = [s.stop - s.start for s in band_n]
    assert set(band_n) <= {30, 31}
    total = sum((n + 2 * PAD) * (along + 2 * PAD) * 8 for n in band_n)
    g = first_group(band_n, along)
    print("byte split %s: bands of %d to %d, planes of %.1f MiB in all, first group of %d profiles" % (direction, min(band_n), max(band_n), total / 2.0 ** 20, g))
    assert total > GROUP_BYTES and 0 < g < 80 and g < GROUP_MAX
    src = to_input(mat)
    t0 = time.perf_counter()
    xlists, ylists, profiles = lp.get_tilted_profiles(src, indices, 0.1, direction)
    profiles = to_numpy(profiles)
    print("byte split %s: %d profiles of %d samples in %.2f s" % (direction, len(indices), along, time.perf_counter() - t0))
    assert profiles.shape == (80, along) and profiles.dtype == mat.dtype
    for p, (xlist, ylist, _, _) in enumerate(lines):
        assert np.array_equal(xlists[p], xlist) and np.array_equal(ylists[p], ylist), p
    for p in (0, g - 1, g, g + 1, 79):
        one = lp.get_tilted_profiles(src, [indices[p]], 0.1, direction)
        assert np.array_equal(to_numpy(one[2])[0], profiles[p]), p
        assert np.array_equal(one[0][0], xlists[p]) and np.array_equal(one[1][0], ylists[p]), p
    return lines, profiles, g


def test_groups_split_by_bytes_horizontal(lp):
    """80 bands of 30 or 31 rows of a 64 x 16384 float32 image: 547 MiB of planes, the first group closes on its bytes."""
    mat = np.random.default_rng(2756).random((64, 16384)).astype(np.float32)
    lines, profiles, g = split_by_bytes(lp, mat, "horizontal", lambda a: a, lambda a: a)
    worst = max(close_to_scipy(profiles[p], ndi.map_coordinates(mat[lines[p][2]], lines[p][3], order=3, mode="nearest")) for p in (0, g, 79))
    print("byte split horizontal: largest deviation from scipy %.3g" % worst)


def test_groups_split_by_bytes_vertical(lp):
    """The same bands as columns of a 16384 x 64 float64 image in device memory."""
    torch = pytest.importorskip("torch")
    mat = np.random.default_rng(2757).random((16384, 64))
    lines, profiles, g = split_by_bytes(lp, mat, "vertical", lambda a: torch.from_numpy(a).to("cuda:0"), lambda t: t.cpu().numpy())
    worst = close_to_scipy(profiles[g], ndi.map_coordinates(mat[lines[g][2]], lines[g][3], order=3, mode="nearest"))
    print("byte split vertical: largest deviation from scipy %.3g" % worst)


BANDS = [(0, 1), (0, 96), (95, 1), (40, 7), (0, 41), (0, 42)]      # (padded lines of 65 and 66 samples: either side of the 64-term start sum)


@pytest.mark.parametrize("direction", [0, 1])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_unequal_bands_in_one_group(hip, dtype, direction):
    """Six bands of 1 to 96 rows (columns, of the transposed image) in one call of the entry point: each profile equals a call of its
    own bit for bit, and scipy on its own band."""
    rng = np.random.default_rng(2758)
    mat = rng.random((96, 120)).astype(dtype)
    if direction == 1:
        mat = np.ascontiguousarray(mat.T)
    height, width = mat.shape
    nprof, length = len(BANDS), 300
    lo = np.array([b[0] for b in BANDS], np.int32)
    n = np.array([b[1] for b in BANDS], np.int32)
    across = lo[:, None] + rng.random((nprof, length)) * (n[:, None] - 1)            # inside each band
    along = rng.random((nprof, length)) * ((width if direction == 0 else height) - 1)
    across[:, 0], across[:, 1], along[:, 0], along[:, 1] = lo, lo + n - 1, 0.0, (width if direction == 0 else height) - 1
    yc, xc = (across, along) if direction == 0 else (along, across)
    i32p = hip.C.POINTER(hip.C.c_int32)
    code = hip.DTYPE_BY_NAME[dtype]

    def call(first, count):
        dst = np.full((count + 1, length), -7.0, dtype)
        hip.check(hip.lib().dcp_tilted_profiles_2d(mat.ctypes.data, dst.ctypes.data, height, width, width, code, direction, count, length,
                                                   yc[first:].ctypes.data, xc[first:].ctypes.data, lo[first:].ctypes.data_as(i32p),
                                                   n[first:].ctypes.data_as(i32p), hip.MEM_HOST, -1, None))
        assert (dst[count] == -7.0).all()
        return dst[:count]

    batch = call(0, nprof)
    worst = 0.0
    for p, (b0, bn) in enumerate(BANDS):
        assert np.array_equal(call(p, 1)[0], batch[p]), p
        if direction == 0:
            ref = ndi.map_coordinates(mat[b0:b0 + bn], (yc[p] - b0, xc[p]), order=3, mode="nearest")
        else:
            ref = ndi.map_coordinates(mat[:, b0:b0 + bn], (yc[p], xc[p] - b0), order=3, mode="nearest")
        worst = max(worst, close_to_scipy(batch[p], ref))
    print("unequal bands %s direction %d: largest deviation from scipy %.3g" % (dtype, direction, worst))


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_a_strided_image_as_the_source(lp, dtype):
    """The 96 x 120 image as a view of a 110 x 150 buffer that is NaN elsewhere, as a NumPy view and as a torch view: the profiles of
    the contiguous image bit for bit, all of them finite."""
    torch = pytest.importorskip("torch")
    mat = np.random.default_rng(2759).random((96, 120)).astype(dtype)
    buf = np.full((110, 150), np.nan, dtype)
    buf[9:105, 17:137] = mat
    view = buf[9:105, 17:137]
    tview = torch.from_numpy(buf).to("cuda:0")[9:105, 17:137]
    assert not view.flags.c_contiguous and not tview.is_contiguous()
    for direction in ("horizontal", "vertical"):
        for angle in (3.0, -3.0):
            indices = list(lp._calc_index_range(96, 120, angle, direction))
            want = lp.get_tilted_profiles(mat, indices, angle, direction)
            assert np.isfinite(want[2]).all()
            got = lp.get_tilted_profiles(view, indices, angle, direction)
            dev = lp.get_tilted_profiles(tview, indices, angle, direction)
            assert isinstance(dev[2], torch.Tensor)
            for a, b, c in zip(want, got, (dev[0], dev[1], dev[2].cpu().numpy())):
                assert np.array_equal(a, b) and np.array_equal(a, c), (direction, angle)
