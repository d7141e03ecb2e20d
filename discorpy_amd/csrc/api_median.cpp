// api_median.cpp -- dcp_median_filter_2d of the C ABI (include/discorpy_hip.h): a plane call (api_plane.h), the window's checks and the
// launch of median_kernels.hip.
#include "api_plane.h"

using namespace dcpapi;

extern "C" {

int dcp_median_filter_2d(const void* src, void* dst, int height, int width, long src_row_stride, int dtype, int size_y, int size_x,
                         int mem_kind, int device, void* stream) {
  PlaneCall c;
  int rc;
  if ((rc = make_plane_call(&c, src, dst, height, width, src_row_stride, dtype, kSameElem, kSideLimit, kReadsWindow, mem_kind, device, stream)) != DCP_OK) return rc;
  if (size_y < 1 || size_x < 1) return fail(DCP_ERR_INVALID_ARG, "size_y and size_x must be at least 1 (got %d x %d)", size_y, size_x);
  if ((int64_t)size_y * (int64_t)size_x >= 2147483648LL)
    return fail(DCP_ERR_UNSUPPORTED, "size_y * size_x = %lld: a window holds at most 2^31 - 1 elements", (long long)size_y * size_x);
  const bool use_lds = g_median_lds.load() != 0;
  return run_plane(c, false, 0, [&](const void* s, void* d, int64_t rs, void*) {
    return dcp::launch_median(s, d, height, width, rs, dtype, size_y, size_x, use_lds, c.stream);
  });
}

}  // extern "C"
