// plane_checks.cpp -- the argument checks of the plane entry points (csrc/api_plane.cpp, and dcp_label_measures_2d of csrc/api_label.cpp
// for its own bound) at their boundaries, as a stand-alone host program: `make -C tests/c plane_checks_asan` builds it with
// -fsanitize=address,undefined and tests/test_plane_refusals_cpu.py runs it.  Nothing here reaches a device: what the two sources need
// of the rest of the library is stubbed below, and every call either is refused or returns before its first device call.
#include "../../discorpy_amd/csrc/api_plane.h"

#include <cstdarg>
#include <cstdio>
#include <cstring>

namespace dcpapi {
static char g_msg[512];
int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_msg, sizeof(g_msg), fmt, ap);
  va_end(ap);
  return code;
}
int mem_kind_of(int mem_kind, bool* host, bool*) {
  *host = mem_kind == DCP_MEM_HOST;
  return mem_kind == DCP_MEM_HOST || mem_kind == DCP_MEM_DEVICE ? DCP_OK : fail(DCP_ERR_INVALID_ARG, "unknown mem_kind %d", mem_kind);
}
std::atomic<int> g_label_lds{1};
thread_local Staging g_staging;
int WorkspaceLease::acquire(size_t, hipStream_t) { return fail(DCP_ERR_HIP, "no workspace in this program"); }
WorkspaceLease::~WorkspaceLease() {}
}  // namespace dcpapi
namespace dcp {
size_t label_count_words(int, int) { return 1; }
hipError_t launch_label(const void*, int32_t*, int32_t*, int32_t*, int, int, int64_t, int, bool, bool, hipStream_t) { return hipErrorUnknown; }
hipError_t launch_fill_holes(const void*, uint8_t*, int32_t*, int32_t*, int, int, int64_t, int, bool, hipStream_t) { return hipErrorUnknown; }
hipError_t launch_clear_border(const void*, uint8_t*, int32_t*, int32_t*, int, int, int64_t, int, bool, bool, bool, hipStream_t) { return hipErrorUnknown; }
hipError_t launch_label_measures(const void*, const int32_t*, int, int, int64_t, int64_t, int, int, long long*, int32_t*, hipStream_t) { return hipErrorUnknown; }
}  // namespace dcp

using namespace dcpapi;

static int failures = 0;
static void expect(const char* what, int got, int want, const char* fragment) {
  const bool ok = got == want && (want == DCP_OK || strstr(g_msg, fragment));
  if (!ok) ++failures;
  printf("%-4s %-66s rc %d%s%s\n", ok ? "ok" : "FAIL", what, got, got == DCP_OK ? "" : ": ", got == DCP_OK ? "" : g_msg);
}

// make_plane_call on a uint16 source whose rows are `stride` elements apart and a destination of dst_elem-byte elements at `dst`
static int plane(const void* src, void* dst, int h, int w, long stride, size_t dst_elem, PlaneLimit limit) {
  PlaneCall c;
  return make_plane_call(&c, src, dst, h, w, stride, dcp::kU16, dst_elem, limit, kComponentReach, DCP_MEM_HOST, -1, nullptr);
}

int main() {
  const int H = 8, W = 10, S = W + 4;
  static uint16_t buf[8 * 14 + 8 * 10 * 2];          // a strided source and, right behind its last element, a destination
  char* end = reinterpret_cast<char*>(buf + (H - 1) * S + W);
  expect("dst begins right behind the source's last element", plane(buf, end, H, W, S, 2, kSideLimit), DCP_OK, "");
  expect("dst begins on the source's last byte", plane(buf, end - 1, H, W, S, 1, kPixelLimit), DCP_ERR_INVALID_ARG, "overlap");
  expect("dst ends right in front of the source", plane(end, end - 2 * W, 1, W, W, 2, kPixelLimit), DCP_OK, "");
  expect("dst ends on the source's first byte", plane(end, end - 2 * W + 1, 1, W, W, 2, kPixelLimit), DCP_ERR_INVALID_ARG, "overlap");
  expect("dst inside the padding of the source's rows overlaps", plane(buf, buf + W, H, 2, S, 2, kPixelLimit), DCP_ERR_INVALID_ARG, "overlap");
  // frames at the limits: addresses far apart that nothing dereferences
  char *lo = reinterpret_cast<char*>(uintptr_t(1) << 20), *hi = reinterpret_cast<char*>(uintptr_t(1) << 44);
  expect("2^31 - 1 pixels in one row", plane(lo, hi, 1, 2147483647, 2147483647L, 4, kPixelLimit), DCP_OK, "");
  expect("2^31 - 1 pixels in one column", plane(lo, hi, 2147483647, 1, 1, 4, kPixelLimit), DCP_OK, "");
  expect("65536 x 32768 = 2^31 pixels", plane(lo, hi, 65536, 32768, 32768, 4, kPixelLimit), DCP_ERR_UNSUPPORTED, "height * width");
  expect("46341 x 46341 > 2^31 - 1 pixels (the product wraps in int32)", plane(lo, hi, 46341, 46341, 46341, 1, kPixelLimit), DCP_ERR_UNSUPPORTED,
         "height * width");
  expect("2^31 - 1 pixels without a destination", plane(lo, nullptr, 1, 2147483647, 2147483647L, 0, kPixelLimit), DCP_OK, "");
  expect("a height of 2^30 - 1", plane(lo, hi, 1073741823, 1, 1, kSameElem, kSideLimit), DCP_OK, "");
  expect("a width of 2^30 - 1", plane(lo, hi, 1, 1073741823, 1073741823L, kSameElem, kSideLimit), DCP_OK, "");
  expect("2^30 - 1 rows of 3 columns (above 2^31 pixels) under the side limit", plane(lo, hi, 1073741823, 3, 3, kSameElem, kSideLimit), DCP_OK, "");
  expect("a height of 2^30", plane(lo, hi, 1073741824, 1, 1, kSameElem, kSideLimit), DCP_ERR_UNSUPPORTED, "2^30 - 1");
  expect("a width of 2^30", plane(lo, hi, 1, 1073741824, 1073741824L, kSameElem, kSideLimit), DCP_ERR_UNSUPPORTED, "2^30 - 1");
  expect("a row stride one below the width", check_row_stride("labels_row_stride", W - 1, W), DCP_ERR_INVALID_ARG, "labels_row_stride 9 is below");
  expect("a row stride of the width", check_row_stride("weights_row_stride", W, W), DCP_OK, "");
  expect("the greatest long as a row stride", check_row_stride("weights_row_stride", 9223372036854775807L, 2147483647), DCP_OK, "");
  expect("a negative row stride", plane(buf, end, H, W, -S, 2, kPixelLimit), DCP_ERR_INVALID_ARG, "src_row_stride -14");
  // the measures' own bound: height * width * max(height, width) < 2^47
  int64_t sums[4];
  int32_t boxes[4], labels[1];
  auto measures = [&](int h, int w) { return dcp_label_measures_2d(nullptr, labels, h, w, w, w, dcp::kU16, 0, sums, boxes, DCP_MEM_HOST, -1, nullptr); };
  expect("measures: 2^17 x (2^13 - 1), 2^47 - 2^34", measures(1 << 17, (1 << 13) - 1), DCP_OK, "");
  expect("measures: 2^17 x 2^13 reaches 2^47", measures(1 << 17, 1 << 13), DCP_ERR_UNSUPPORTED, "max(height, width)");
  expect("measures: 2^13 x 2^17 reaches 2^47", measures(1 << 13, 1 << 17), DCP_ERR_UNSUPPORTED, "max(height, width)");
  expect("measures: 1 x (2^31 - 1) passes the pixel limit, not this one", measures(1, 2147483647), DCP_ERR_UNSUPPORTED, "max(height, width)");
  expect("measures: 2^16 x 2^15 is refused for its pixels first", measures(65536, 32768), DCP_ERR_UNSUPPORTED, "height * width");
  printf("%d failure(s)\n", failures);
  return failures ? 1 : 0;
}
