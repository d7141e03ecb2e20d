// api_gauss.cpp -- dcp_correlate_sym_2d of the C ABI (include/discorpy_hip.h): the argument checks, the plane between the two passes
// (leased from the spline workspace), the staged round trip of host memory and the launch of gauss_kernels.hip.
#include "api_common.h"

#include <cstring>

using namespace dcpapi;

// 2 r + 1 weights that read the same from both ends, compared as bit patterns
static bool symmetric_to_the_bit(const double* w, int r) {
  for (int k = 0; k < r; ++k)
    if (memcmp(&w[k], &w[2 * r - k], sizeof(double)) != 0) return false;
  return true;
}

extern "C" {

int dcp_correlate_sym_2d(const void* src, void* dst, int height, int width, long src_row_stride, int dtype, const double* weights_y,
                         int radius_y, const double* weights_x, int radius_x, int mode, double cval, int mem_kind, int device, void* stream) {
  bool host = false;
  int rc;
  if ((rc = mem_kind_of(mem_kind, &host)) != DCP_OK) return rc;
  if (dtype < 0 || dtype >= dcp::kNumElemTypes) return fail(DCP_ERR_INVALID_ARG, "unknown dtype %d", dtype);
  if (dtype == dcp::kBool) return fail(DCP_ERR_UNSUPPORTED, "dtype bool: scipy's filters do not take it either");
  if (!src || !dst) return fail(DCP_ERR_INVALID_ARG, "null src / dst pointer");
  if (height < 1 || width < 1) return fail(DCP_ERR_INVALID_ARG, "height and width must be at least 1 (got %d x %d)", height, width);
  if (src_row_stride < width) return fail(DCP_ERR_INVALID_ARG, "src_row_stride %ld is below the width %d", src_row_stride, width);
  if (mode < DCP_MODE_REFLECT || mode > DCP_MODE_WRAP) return fail(DCP_ERR_INVALID_ARG, "unknown boundary mode %d", mode);
  if (radius_y < -1 || radius_x < -1) return fail(DCP_ERR_INVALID_ARG, "radius_y and radius_x must be at least -1 (got %d, %d)", radius_y, radius_x);
  if (!weights_y) radius_y = -1;
  if (!weights_x) radius_x = -1;
  if (radius_y > dcp::kGaussMaxRadius || radius_x > dcp::kGaussMaxRadius)
    return fail(DCP_ERR_UNSUPPORTED, "radius_y / radius_x above %d (got %d, %d)", dcp::kGaussMaxRadius, radius_y, radius_x);
  if (radius_y >= 0 && !symmetric_to_the_bit(weights_y, radius_y)) return fail(DCP_ERR_INVALID_ARG, "weights_y are not symmetric to the bit");
  if (radius_x >= 0 && !symmetric_to_the_bit(weights_x, radius_x)) return fail(DCP_ERR_INVALID_ARG, "weights_x are not symmetric to the bit");
  if (height > 1073741823 || width > 1073741823) return fail(DCP_ERR_UNSUPPORTED, "height / width above 2^30 - 1 (got %d x %d)", height, width);
  const size_t esz = (size_t)dcp::elem_size(dtype);
  const char *s0 = (const char*)src, *s1 = s0 + ((size_t)(height - 1) * (size_t)src_row_stride + (size_t)width) * esz;
  const char *d0 = (const char*)dst, *d1 = d0 + (size_t)height * (size_t)width * esz;
  if (s0 < d1 && d0 < s1) return fail(DCP_ERR_INVALID_ARG, "src and dst overlap: every output pixel reads a neighbourhood of the source");
  DeviceScope scope(device);
  if (scope.status != hipSuccess) return fail(DCP_ERR_HIP, "cannot select device %d: %s", device, hipGetErrorString(scope.status));
  const int lds_mode = g_gauss_lds.load();
  hipStream_t st = (hipStream_t)stream;
  // the plane between the passes of the per-axis route
  WorkspaceLease lease;
  if (radius_y >= 0 && radius_x >= 0 && !dcp::gauss_takes_lds(dtype, radius_y, radius_x, lds_mode))
    if ((rc = lease.acquire((size_t)height * (size_t)width * esz, st)) != DCP_OK) return rc;
  if (!host) {
    DCP_HIP(dcp::launch_gauss(src, dst, lease.buf, height, width, (int64_t)src_row_stride, dtype, weights_y, radius_y, weights_x, radius_x, mode,
                              cval, lds_mode, st));
    return DCP_OK;
  }
  HostTrip t;          // the rows are packed on the way up
  t.src = src;
  t.row_bytes = (size_t)width * esz;
  t.rows = (size_t)height;
  t.pitch = (size_t)src_row_stride * esz;
  t.dst = dst;
  t.out_bytes = (size_t)height * (size_t)width * esz;
  return host_round_trip(t, st, [&](const void* dsrc, void* ddst, void*, void*) {
    return dcp::launch_gauss(dsrc, ddst, lease.buf, height, width, (int64_t)width, dtype, weights_y, radius_y, weights_x, radius_x, mode, cval,
                             lds_mode, st);
  });
}

}  // extern "C"
