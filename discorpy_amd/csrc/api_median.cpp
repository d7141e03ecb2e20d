// api_median.cpp -- dcp_median_filter_2d of the C ABI (include/discorpy_hip.h): the argument checks, the staged round trip of host
// memory and the launch of median_kernels.hip.
#include "api_common.h"

using namespace dcpapi;

extern "C" {

int dcp_median_filter_2d(const void* src, void* dst, int height, int width, long src_row_stride, int dtype, int size_y, int size_x,
                         int mem_kind, int device, void* stream) {
  bool host = false;
  int rc;
  if ((rc = mem_kind_of(mem_kind, &host)) != DCP_OK) return rc;
  if (dtype < 0 || dtype >= dcp::kNumElemTypes) return fail(DCP_ERR_INVALID_ARG, "unknown dtype %d", dtype);
  if (!src || !dst) return fail(DCP_ERR_INVALID_ARG, "null src / dst pointer");
  if (height < 1 || width < 1) return fail(DCP_ERR_INVALID_ARG, "height and width must be at least 1 (got %d x %d)", height, width);
  if (size_y < 1 || size_x < 1) return fail(DCP_ERR_INVALID_ARG, "size_y and size_x must be at least 1 (got %d x %d)", size_y, size_x);
  if (src_row_stride < width) return fail(DCP_ERR_INVALID_ARG, "src_row_stride %ld is below the width %d", src_row_stride, width);
  if ((int64_t)size_y * (int64_t)size_x >= 2147483648LL)
    return fail(DCP_ERR_UNSUPPORTED, "size_y * size_x = %lld: a window holds at most 2^31 - 1 elements", (long long)size_y * size_x);
  if (height > 1073741823 || width > 1073741823) return fail(DCP_ERR_UNSUPPORTED, "height / width above 2^30 - 1 (got %d x %d)", height, width);
  const size_t esz = (size_t)dcp::elem_size(dtype);
  const char *s0 = (const char*)src, *s1 = s0 + ((size_t)(height - 1) * (size_t)src_row_stride + (size_t)width) * esz;
  const char *d0 = (const char*)dst, *d1 = d0 + (size_t)height * (size_t)width * esz;
  if (s0 < d1 && d0 < s1) return fail(DCP_ERR_INVALID_ARG, "src and dst overlap: every output pixel reads a window of the source");
  DeviceScope scope(device);
  if (scope.status != hipSuccess) return fail(DCP_ERR_HIP, "cannot select device %d: %s", device, hipGetErrorString(scope.status));
  const bool use_lds = g_median_lds.load() != 0;
  hipStream_t st = (hipStream_t)stream;
  if (!host) {
    DCP_HIP(dcp::launch_median(src, dst, height, width, (int64_t)src_row_stride, dtype, size_y, size_x, use_lds, st));
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
    return dcp::launch_median(dsrc, ddst, height, width, (int64_t)width, dtype, size_y, size_x, use_lds, st);
  });
}

}  // extern "C"
