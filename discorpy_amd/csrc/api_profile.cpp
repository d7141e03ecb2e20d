// api_profile.cpp -- dcp_local_extrema_rows, dcp_window_slope_rows, dcp_tilted_profiles_2d and dcp_select_peaks_rows of the C ABI
// (include/discorpy_hip.h): plane calls (api_plane.h) on a plane of profiles or on the image the profiles are taken from, their argument
// checks, the workspace of the bands' coefficient planes and of the peak tables (one lease of the spline workspace) and the launches of
// profile_kernels.hip and select_peaks_kernels.hip.
#include "api_plane.h"

#include <cstring>
#include <memory>
#include <new>
#include <vector>

using namespace dcpapi;

constexpr size_t kProfileWorkCap = (size_t)512 << 20;   // the bands' planes of one group; a single band wider than this still gets its own

static int float_plane_only(int dtype) {
  if (dtype != dcp::kF32 && dtype != dcp::kF64) return fail(DCP_ERR_UNSUPPORTED, "dtype %d: profiles are float32 or float64", dtype);
  return DCP_OK;
}

extern "C" {

int dcp_local_extrema_rows(const void* src, double* dst, int nrows, int length, long src_row_stride, int dtype, int radius, double sensitive,
                           int subpixel, int mem_kind, int device, void* stream) {
  PlaneCall c;
  int rc;
  if ((rc = make_plane_call(&c, src, dst, nrows, length, src_row_stride, dtype, sizeof(double), kPixelLimit, kReadsWindow, mem_kind, device, stream)) != DCP_OK)
    return rc;
  if ((rc = float_plane_only(dtype)) != DCP_OK) return rc;
  if (radius < 0) return fail(DCP_ERR_INVALID_ARG, "radius must be at least 0 (got %d)", radius);
  if (radius > dcp::kPeakMaxRadius) return fail(DCP_ERR_UNSUPPORTED, "radius above %d (got %d)", dcp::kPeakMaxRadius, radius);
  if (subpixel != 0 && subpixel != 1) return fail(DCP_ERR_INVALID_ARG, "subpixel must be 0 or 1 (got %d)", subpixel);
  if (subpixel && radius < 1) return fail(DCP_ERR_INVALID_ARG, "subpixel needs a radius of at least 1");
  if (sensitive != sensitive) return fail(DCP_ERR_INVALID_ARG, "sensitive is NaN");
  return run_plane(c, false, 0, [&](const void* s, void* d, int64_t rs, void*) {
    return dcp::launch_peak_rows(s, static_cast<double*>(d), nrows, length, rs, dtype, radius, sensitive, subpixel != 0, c.stream);
  });
}

int dcp_window_slope_rows(const void* src, void* dst, int nrows, int length, long src_row_stride, int dtype, int size, int mem_kind, int device,
                          void* stream) {
  PlaneCall c;
  int rc;
  if ((rc = make_plane_call(&c, src, dst, nrows, length, src_row_stride, dtype, kSameElem, kPixelLimit, kReadsWindow, mem_kind, device, stream)) != DCP_OK)
    return rc;
  if ((rc = float_plane_only(dtype)) != DCP_OK) return rc;
  if (size < 3 || !(size & 1)) return fail(DCP_ERR_INVALID_ARG, "size must be odd and at least 3 (got %d)", size);
  if (nrows > 65535) return fail(DCP_ERR_UNSUPPORTED, "more than 65535 rows (got %d)", nrows);
  return run_plane(c, false, 0, [&](const void* s, void* d, int64_t rs, void*) {
    return dcp::launch_window_slope(s, d, nrows, length, rs, dtype, size, c.stream);
  });
}

int dcp_tilted_profiles_2d(const void* src, void* dst, int height, int width, long src_row_stride, int dtype, int direction, int nprofiles,
                           int length, const double* ycoords, const double* xcoords, const int32_t* band_lo, const int32_t* band_count,
                           int mem_kind, int device, void* stream) {
  PlaneCall c;
  int rc;
  // (the destination is not a plane of the source's shape: checked here, and the round trip of host memory is this call's own)
  if ((rc = make_plane_call(&c, src, nullptr, height, width, src_row_stride, dtype, 0, kSideLimit, kReadsWindow, mem_kind, device, stream)) != DCP_OK)
    return rc;
  if ((rc = float_plane_only(dtype)) != DCP_OK) return rc;
  if (!dst || !ycoords || !xcoords || !band_lo || !band_count) return fail(DCP_ERR_INVALID_ARG, "null dst / coordinate / band pointer");
  if (direction != 0 && direction != 1) return fail(DCP_ERR_INVALID_ARG, "direction must be 0 (bands of rows) or 1 (bands of columns), got %d", direction);
  if (nprofiles < 1 || length < 1) return fail(DCP_ERR_INVALID_ARG, "nprofiles and length must be at least 1 (got %d, %d)", nprofiles, length);
  if (nprofiles > 65535) return fail(DCP_ERR_UNSUPPORTED, "more than 65535 profiles (got %d)", nprofiles);
  if ((int64_t)nprofiles * (int64_t)length > 2147483647LL) return fail(DCP_ERR_UNSUPPORTED, "nprofiles * length above 2^31 - 1");
  const bool vertical = direction == 1;
  const size_t table = dcp::kProfileGroupMax * 24;      // the band table in front of the planes (profile_kernels.hip)
  size_t all = 0, widest = 0;
  for (int p = 0; p < nprofiles; ++p) {
    if (band_lo[p] < 0 || band_count[p] < 1 || (int64_t)band_lo[p] + band_count[p] > (vertical ? width : height))
      return fail(DCP_ERR_INVALID_ARG, "band %d: [%d, %d + %d) leaves the image", p, band_lo[p], band_lo[p], band_count[p]);
    const size_t bytes = dcp::profile_band_elems(height, width, vertical, band_count[p]) * sizeof(double);
    all += bytes;
    widest = bytes > widest ? bytes : widest;
  }
  const size_t work_bytes = table + (all <= kProfileWorkCap ? all : (widest > kProfileWorkCap ? widest : kProfileWorkCap));
  const size_t out_bytes = (size_t)nprofiles * (size_t)length * c.esz, coord_bytes = (size_t)nprofiles * (size_t)length * sizeof(double);
  {
    const char *d0 = (const char*)dst, *d1 = d0 + out_bytes;
    const char *s0 = (const char*)src, *s1 = s0 + ((size_t)(height - 1) * (size_t)src_row_stride + (size_t)width) * c.esz;
    if (s0 < d1 && d0 < s1) return fail(DCP_ERR_INVALID_ARG, "src and dst overlap: %s", kReadsNeighbourhood);
  }
  PlaneDevice on(c.device);
  if (on.rc != DCP_OK) return on.rc;
  WorkspaceLease lease;
  if ((rc = lease.acquire(work_bytes, c.stream)) != DCP_OK) return rc;
  auto launch = [&](const void* s, void* d, int64_t rs, const void* yc, const void* xc) {
    return dcp::launch_tilted_profiles(s, d, height, width, rs, dtype, vertical, nprofiles, length, static_cast<const double*>(yc),
                                       static_cast<const double*>(xc), band_lo, band_count, lease.buf, work_bytes, c.stream);
  };
  if (!c.host) {
    DCP_HIP(launch(c.src, dst, c.rs, ycoords, xcoords));
    return DCP_OK;
  }
  HostTrip t = packed_rows(c);
  t.y_up = ycoords;
  t.x_up = xcoords;
  t.plane = coord_bytes;
  t.dst = dst;
  t.out_bytes = out_bytes;
  return host_round_trip(t, c.stream, [&](const void* dsrc, void* ddst, void* dy, void* dx) { return launch(dsrc, ddst, (int64_t)c.W, dy, dx); });
}

int dcp_select_peaks_rows(const void* src, int nrows, int length, long src_row_stride, int dtype, const int32_t* peak_row, const int32_t* peak_index,
                          int npeaks, int radius, double tol, int use_offset, unsigned char* keep, double* fit, int mem_kind, int device, void* stream) {
  PlaneCall c;
  int rc;
  // (the outputs are not planes of the source's shape: checked here, and the round trip of host memory is this call's own)
  if ((rc = make_plane_call(&c, src, nullptr, nrows, length, src_row_stride, dtype, 0, kPixelLimit, kReadsWindow, mem_kind, device, stream)) != DCP_OK)
    return rc;
  if ((rc = float_plane_only(dtype)) != DCP_OK) return rc;
  if (!peak_row || !peak_index || !keep) return fail(DCP_ERR_INVALID_ARG, "null peak_row / peak_index / keep pointer");
  if (npeaks < 1) return fail(DCP_ERR_INVALID_ARG, "npeaks must be at least 1 (got %d)", npeaks);
  if (radius < 1) return fail(DCP_ERR_INVALID_ARG, "radius must be at least 1 (got %d)", radius);
  if (radius > dcp::kSelectMaxRadius) return fail(DCP_ERR_UNSUPPORTED, "radius above %d (got %d)", dcp::kSelectMaxRadius, radius);
  if (tol != tol) return fail(DCP_ERR_INVALID_ARG, "tol is NaN");
  if (use_offset != 0 && use_offset != 1) return fail(DCP_ERR_INVALID_ARG, "use_offset must be 0 or 1 (got %d)", use_offset);
  for (int k = 0; k < npeaks; ++k)
    if (peak_row[k] < 0 || peak_row[k] >= nrows || peak_index[k] < 0 || peak_index[k] >= length)
      return fail(DCP_ERR_INVALID_ARG, "peak %d: row %d, index %d lies outside the %d x %d plane", k, peak_row[k], peak_index[k], nrows, length);
  const size_t keep_bytes = (size_t)npeaks, fit_bytes = (size_t)npeaks * 6 * sizeof(double);
  {
    const char *s0 = (const char*)src, *s1 = s0 + ((size_t)(nrows - 1) * (size_t)src_row_stride + (size_t)length) * c.esz;
    const char *k0 = (const char*)keep, *k1 = k0 + keep_bytes;
    const char *f0 = (const char*)fit, *f1 = f0 + fit_bytes;
    if ((s0 < k1 && k0 < s1) || (fit && s0 < f1 && f0 < s1)) return fail(DCP_ERR_INVALID_ARG, "src and keep / fit overlap: %s", kReadsWindow);
    if (fit && k0 < f1 && f0 < k1) return fail(DCP_ERR_INVALID_ARG, "keep and fit overlap");
  }
  PlaneDevice on(c.device);
  if (on.rc != DCP_OK) return on.rc;
  WorkspaceLease lease;
  if ((rc = lease.acquire(dcp::select_peaks_work_bytes(npeaks), c.stream)) != DCP_OK) return rc;
  auto launch = [&](const void* s, int64_t rs, unsigned char* k, double* f) {
    return dcp::launch_select_peaks(s, nrows, length, rs, dtype, peak_row, peak_index, npeaks, radius, tol, use_offset != 0, k, f, lease.buf, c.stream);
  };
  if (!c.host) {
    DCP_HIP(launch(c.src, c.rs, keep, fit));
    return DCP_OK;
  }
  // host memory: both outputs come back in one block, the fit rows (8-byte aligned) in front of the keep bytes
  std::vector<unsigned char> back(fit_bytes + keep_bytes);
  HostTrip t = packed_rows(c);
  t.dst = back.data();
  t.out_bytes = back.size();
  rc = host_round_trip(t, c.stream, [&](const void* dsrc, void* ddst, void*, void*) {
    return launch(dsrc, (int64_t)c.W, static_cast<unsigned char*>(ddst) + fit_bytes, static_cast<double*>(ddst));
  });
  if (rc != DCP_OK) return rc;
  memcpy(keep, back.data() + fit_bytes, keep_bytes);
  if (fit) memcpy(fit, back.data(), fit_bytes);
  return DCP_OK;
}

int dcp_extrema_select_rows(const void* src, double* dst, int nrows, int length, long src_row_stride, int dtype, int radius, double sensitive,
                            int subpixel, const void* sel, long sel_row_stride, double tol, int use_offset, double* cand, unsigned char* keep,
                            int mem_kind, int device, void* stream) {
  PlaneCall c;
  int rc;
  if ((rc = make_plane_call(&c, src, dst, nrows, length, src_row_stride, dtype, sizeof(double), kPixelLimit, kReadsWindow, mem_kind, device, stream)) != DCP_OK)
    return rc;
  if ((rc = float_plane_only(dtype)) != DCP_OK) return rc;
  if (sel && (rc = check_row_stride("sel_row_stride", sel_row_stride, length)) != DCP_OK) return rc;
  if (radius < 1) return fail(DCP_ERR_INVALID_ARG, "radius must be at least 1 (got %d)", radius);
  if (radius > dcp::kSelectMaxRadius) return fail(DCP_ERR_UNSUPPORTED, "radius above %d (got %d)", dcp::kSelectMaxRadius, radius);
  if (subpixel != 0 && subpixel != 1) return fail(DCP_ERR_INVALID_ARG, "subpixel must be 0 or 1 (got %d)", subpixel);
  if (use_offset != 0 && use_offset != 1) return fail(DCP_ERR_INVALID_ARG, "use_offset must be 0 or 1 (got %d)", use_offset);
  if (sensitive != sensitive) return fail(DCP_ERR_INVALID_ARG, "sensitive is NaN");
  if (tol != tol) return fail(DCP_ERR_INVALID_ARG, "tol is NaN");
  const size_t cells = (size_t)nrows * (size_t)length, table_bytes = cells * sizeof(double);
  {
    // two planes read, three tables written: no table may touch a plane or another table
    struct Span {
      const char *lo, *hi;
      const char* name;
    };
    const Span in[2] = {{(const char*)src, (const char*)src + ((size_t)(nrows - 1) * (size_t)src_row_stride + (size_t)length) * c.esz, "src"},
                        {(const char*)sel, (const char*)sel + (sel ? ((size_t)(nrows - 1) * (size_t)sel_row_stride + (size_t)length) * c.esz : 0), "sel"}};
    const Span out[3] = {{(const char*)dst, (const char*)dst + table_bytes, "dst"},
                         {(const char*)cand, (const char*)cand + (cand ? table_bytes : 0), "cand"},
                         {(const char*)keep, (const char*)keep + (keep ? cells : 0), "keep"}};
    for (const Span& a : in)
      for (const Span& b : out)
        if (a.lo && b.lo && a.lo < b.hi && b.lo < a.hi) return fail(DCP_ERR_INVALID_ARG, "%s and %s overlap: %s", a.name, b.name, kReadsWindow);
    for (int i = 0; i < 3; ++i)
      for (int j = i + 1; j < 3; ++j)
        if (out[i].lo && out[j].lo && out[i].lo < out[j].hi && out[j].lo < out[i].hi)
          return fail(DCP_ERR_INVALID_ARG, "%s and %s overlap", out[i].name, out[j].name);
  }
  PlaneDevice on(c.device);
  if (on.rc != DCP_OK) return on.rc;
  WorkspaceLease lease;
  if ((rc = lease.acquire(dcp::extrema_select_work_bytes(nrows, length), c.stream)) != DCP_OK) return rc;
  auto launch = [&](const void* s, int64_t rs, const void* q, int64_t qs, double* d, double* cd, unsigned char* k) {
    return dcp::launch_extrema_select(s, d, nrows, length, rs, dtype, radius, sensitive, subpixel != 0, q, qs, tol, use_offset != 0, cd, k, lease.buf,
                                      c.stream);
  };
  if (!c.host) {
    DCP_HIP(launch(c.src, c.rs, sel, (int64_t)sel_row_stride, dst, cand, keep));
    return DCP_OK;
  }
  // host memory: the rows go up packed (sel behind them, into a staging plane of its own); the tables the caller asked for come back in
  // one block -- dst, then cand (also where only keep is asked for: it carries the rows' counts), then keep -- and only what the call
  // defines is copied out of it: a row's entries up to its count, and the count
  const size_t row_bytes = (size_t)length * c.esz;
  void* dsel = nullptr;
  if (sel) DCP_HIP(g_staging.get(2, (size_t)nrows * row_bytes, &dsel));
  const bool with_cand = cand || keep;
  const size_t back_bytes = table_bytes + (with_cand ? table_bytes : 0) + (keep ? cells : 0);
  const std::unique_ptr<unsigned char[]> back(new (std::nothrow) unsigned char[back_bytes]);
  if (!back) return fail(DCP_ERR_HIP, "out of host memory: %zu bytes for the tables on their way down", back_bytes);
  HostTrip t = packed_rows(c);
  t.dst = back.get();
  t.out_bytes = back_bytes;
  rc = host_round_trip(t, c.stream, [&](const void* dsrc, void* ddst, void*, void*) {
    if (sel) {
      const hipError_t e = hipMemcpy2DAsync(dsel, row_bytes, sel, (size_t)sel_row_stride * c.esz, row_bytes, (size_t)nrows, hipMemcpyHostToDevice, c.stream);
      if (e != hipSuccess) return e;
    }
    unsigned char* const b = static_cast<unsigned char*>(ddst);
    return launch(dsrc, (int64_t)length, dsel, (int64_t)length, reinterpret_cast<double*>(b), with_cand ? reinterpret_cast<double*>(b + table_bytes) : nullptr,
                  keep ? b + 2 * table_bytes : nullptr);
  });
  if (rc != DCP_OK) return rc;
  const double* const bdst = reinterpret_cast<const double*>(back.get());
  const double* const bcand = reinterpret_cast<const double*>(back.get() + table_bytes);
  const unsigned char* const bkeep = back.get() + 2 * table_bytes;
  for (size_t r = 0; r < (size_t)nrows; ++r) {
    const size_t first = r * (size_t)length, last = first + (size_t)length - 1;
    const size_t kept = (size_t)bdst[last];
    memcpy(dst + first, bdst + first, kept * sizeof(double));
    dst[last] = bdst[last];
    if (!with_cand) continue;
    const size_t count = (size_t)bcand[last];
    if (cand) {
      memcpy(cand + first, bcand + first, count * sizeof(double));
      cand[last] = bcand[last];
    }
    if (keep) memcpy(keep + first, bkeep + first, count);
  }
  return DCP_OK;
}

}  // extern "C"
