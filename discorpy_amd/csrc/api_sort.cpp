// api_sort.cpp -- dcp_sort_plane_2d and dcp_zoom_cubic_nearest_1d of the C ABI (include/discorpy_hip.h): plane calls (api_plane.h), their own
// checks, the sort's work memory (leased from the spline workspace) and the launches of sort_kernels.hip.
#include "api_plane.h"

#include <cmath>

using namespace dcpapi;

namespace {

constexpr size_t kWorkspaceLimit = (size_t)2 << 30;          // what one lease of the spline workspace may ask for
constexpr const char* kAnyElement = "every output element may come from any source element";

bool sortable(int dtype) { return dtype != dcp::kBool; }

}  // namespace

extern "C" {

int dcp_sort_plane_2d(const void* src, void* dst, int height, int width, long src_row_stride, int dtype, int mem_kind, int device, void* stream) {
  PlaneCall c;
  int rc;
  if ((rc = make_plane_call(&c, src, dst, height, width, src_row_stride, dtype, kSameElem, kPixelLimit, kAnyElement, mem_kind, device, stream)) != DCP_OK)
    return rc;
  if (!sortable(dtype)) return fail(DCP_ERR_UNSUPPORTED, "dtype %d: float32, float64 and the 8- to 64-bit integers only", dtype);
  const size_t work = dcp::sort_work_bytes((int64_t)height * width, dtype);
  if (work > kWorkspaceLimit)
    return fail(DCP_ERR_UNSUPPORTED, "height * width = %lld: the two key buffers and their tables take %zu bytes, above the workspace's limit of 2 GiB",
                (long long)height * width, work);
  const bool skip = g_sort_skip.load() != 0;
  return run_plane(c, false, work, [&](const void* s, void* d, int64_t rs, void* w) { return dcp::launch_sort(s, d, height, width, rs, dtype, w, skip, c.stream); });
}

int dcp_zoom_cubic_nearest_1d(const void* src, int64_t n, void* dst, int64_t out_n, int dtype, int mem_kind, int device, void* stream) {
  PlaneCall c;
  int rc;
  if (n < 1 || n > 2147483647LL) {
    // (the shared checks take an int: a length outside its range gets their words here)
    bool host;
    if ((rc = mem_kind_of(mem_kind, &host)) != DCP_OK) return rc;
    if (dtype < 0 || dtype >= dcp::kNumElemTypes) return fail(DCP_ERR_INVALID_ARG, "unknown dtype %d", dtype);
    if (n < 1) return fail(DCP_ERR_INVALID_ARG, "height and width must be at least 1 (got 1 x %lld)", (long long)n);
    return fail(DCP_ERR_UNSUPPORTED, "height * width = %lld: labels and pixel indices are int32, at most 2^31 - 1 pixels", (long long)n);
  }
  // the line as a plane of one row; the destination has its own length, checked here
  if ((rc = make_plane_call(&c, src, nullptr, 1, (int)n, (long)n, dtype, 0, kPixelLimit, nullptr, mem_kind, device, stream)) != DCP_OK) return rc;
  if (!dst) return fail(DCP_ERR_INVALID_ARG, "null src / dst pointer");
  if (out_n < 1) return fail(DCP_ERR_INVALID_ARG, "out_n must be at least 1 (got %lld)", (long long)out_n);
  if (out_n > 2147483647LL) return fail(DCP_ERR_UNSUPPORTED, "out_n = %lld: at most 2^31 - 1 output points", (long long)out_n);
  if (!sortable(dtype)) return fail(DCP_ERR_UNSUPPORTED, "dtype %d: float32, float64 and the 8- to 64-bit integers only", dtype);
  const char *s0 = (const char*)src, *s1 = s0 + (size_t)n * c.esz, *d0 = (const char*)dst, *d1 = d0 + (size_t)out_n * c.esz;
  if (s0 < d1 && d0 < s1) return fail(DCP_ERR_INVALID_ARG, "src and dst overlap: %s", "every output point reads a window of the source");
  c.dst = dst;
  c.dst_elem = c.esz;
  c.dst_n = out_n;
  const double z_n = std::pow(std::sqrt(3.0) - 2.0, (double)(n + 24));
  return run_plane(c, false, 0, [&](const void* s, void* d, int64_t, void*) { return dcp::launch_zoom_cubic_nearest(s, n, d, out_n, dtype, z_n, c.stream); });
}

}  // extern "C"
