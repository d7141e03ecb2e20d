// api_label.cpp -- dcp_label_2d, dcp_label_measures_2d, dcp_fill_holes_2d and dcp_clear_border_2d of the C ABI (include/discorpy_hip.h): the
// argument checks (shared with api_binarize.cpp), the working planes (leased from the spline workspace), the staged round trip of host
// memory and the launches of label_kernels.hip.
#include "api_common.h"

using namespace dcpapi;

namespace dcpapi {

int check_plane_call(const void* src, const void* dst, int height, int width, long src_row_stride, int dtype, size_t dst_elem, int mem_kind, bool* host) {
  int rc;
  if ((rc = mem_kind_of(mem_kind, host)) != DCP_OK) return rc;
  if (dtype < 0 || dtype >= dcp::kNumElemTypes) return fail(DCP_ERR_INVALID_ARG, "unknown dtype %d", dtype);
  if (!src || (dst_elem && !dst)) return fail(DCP_ERR_INVALID_ARG, "null src / dst pointer");
  if (height < 1 || width < 1) return fail(DCP_ERR_INVALID_ARG, "height and width must be at least 1 (got %d x %d)", height, width);
  if (src_row_stride < width) return fail(DCP_ERR_INVALID_ARG, "src_row_stride %ld is below the width %d", src_row_stride, width);
  if ((int64_t)height * (int64_t)width > 2147483647LL)
    return fail(DCP_ERR_UNSUPPORTED, "height * width = %lld: labels and pixel indices are int32, at most 2^31 - 1 pixels", (long long)height * width);
  if (!dst_elem) return DCP_OK;
  const size_t esz = (size_t)dcp::elem_size(dtype);
  const char *s0 = (const char*)src, *s1 = s0 + ((size_t)(height - 1) * (size_t)src_row_stride + (size_t)width) * esz;
  const char *d0 = (const char*)dst, *d1 = d0 + (size_t)height * (size_t)width * dst_elem;
  if (s0 < d1 && d0 < s1) return fail(DCP_ERR_INVALID_ARG, "src and dst overlap: a pixel's component reaches across the whole image");
  return DCP_OK;
}

HostTrip packed_rows(const void* src, void* dst, int height, int width, long src_row_stride, size_t esz, size_t dst_elem) {
  HostTrip t;          // the rows are packed on the way up
  t.src = src;
  t.row_bytes = (size_t)width * esz;
  t.rows = (size_t)height;
  t.pitch = (size_t)src_row_stride * esz;
  t.dst = dst;
  t.out_bytes = (size_t)height * (size_t)width * dst_elem;
  return t;
}

}  // namespace dcpapi

extern "C" {

int dcp_label_2d(const void* src, int32_t* dst, int height, int width, long src_row_stride, int dtype, int connectivity, int* num_labels_out,
                 int mem_kind, int device, void* stream) {
  bool host = false;
  int rc;
  if ((rc = check_plane_call(src, dst, height, width, src_row_stride, dtype, sizeof(int32_t), mem_kind, &host)) != DCP_OK) return rc;
  if (connectivity != 4 && connectivity != 8) return fail(DCP_ERR_INVALID_ARG, "connectivity must be 4 or 8 (got %d)", connectivity);
  if (!num_labels_out) return fail(DCP_ERR_INVALID_ARG, "null num_labels_out pointer");
  DeviceScope scope(device);
  if (scope.status != hipSuccess) return fail(DCP_ERR_HIP, "cannot select device %d: %s", device, hipGetErrorString(scope.status));
  const bool use_lds = g_label_lds.load() != 0;
  hipStream_t st = (hipStream_t)stream;
  // the parent plane (the ranks' afterwards) and, behind it, the per-block root counts with the total in their last word
  const size_t n = (size_t)height * (size_t)width, words = dcp::label_count_words(height, width);
  WorkspaceLease lease;
  if ((rc = lease.acquire((n + words) * sizeof(int32_t), st)) != DCP_OK) return rc;
  int32_t *parent = static_cast<int32_t*>(lease.buf), *counts = parent + n;
  const size_t esz = (size_t)dcp::elem_size(dtype);
  int32_t total = 0;
  if (!host) {
    DCP_HIP(dcp::launch_label(src, dst, parent, counts, height, width, (int64_t)src_row_stride, dtype, connectivity == 8, use_lds, st));
    DCP_HIP(hipMemcpyAsync(&total, counts + words - 1, sizeof(total), hipMemcpyDeviceToHost, st));
    DCP_HIP(hipStreamSynchronize(st));
  } else {
    rc = host_round_trip(packed_rows(src, dst, height, width, src_row_stride, esz, sizeof(int32_t)), st, [&](const void* dsrc, void* ddst, void*, void*) {
      hipError_t e = dcp::launch_label(dsrc, static_cast<int32_t*>(ddst), parent, counts, height, width, (int64_t)width, dtype, connectivity == 8,
                                       use_lds, st);
      if (e != hipSuccess) return e;
      return hipMemcpyAsync(&total, counts + words - 1, sizeof(total), hipMemcpyDeviceToHost, st);
    });
    if (rc != DCP_OK) return rc;
  }
  *num_labels_out = (int)total;
  return DCP_OK;
}

int dcp_fill_holes_2d(const void* src, uint8_t* dst, int height, int width, long src_row_stride, int dtype, int mem_kind, int device, void* stream) {
  bool host = false;
  int rc;
  if ((rc = check_plane_call(src, dst, height, width, src_row_stride, dtype, sizeof(uint8_t), mem_kind, &host)) != DCP_OK) return rc;
  DeviceScope scope(device);
  if (scope.status != hipSuccess) return fail(DCP_ERR_HIP, "cannot select device %d: %s", device, hipGetErrorString(scope.status));
  const bool use_lds = g_label_lds.load() != 0;
  hipStream_t st = (hipStream_t)stream;
  const size_t n = (size_t)height * (size_t)width;
  WorkspaceLease lease;          // the parent plane of the complement's components and the plane of their roots
  if ((rc = lease.acquire(2 * n * sizeof(int32_t), st)) != DCP_OK) return rc;
  int32_t *parent = static_cast<int32_t*>(lease.buf), *root = parent + n;
  if (!host) {
    DCP_HIP(dcp::launch_fill_holes(src, dst, parent, root, height, width, (int64_t)src_row_stride, dtype, use_lds, st));
    return DCP_OK;
  }
  return host_round_trip(packed_rows(src, dst, height, width, src_row_stride, (size_t)dcp::elem_size(dtype), sizeof(uint8_t)), st,
                         [&](const void* dsrc, void* ddst, void*, void*) {
                           return dcp::launch_fill_holes(dsrc, static_cast<uint8_t*>(ddst), parent, root, height, width, (int64_t)width, dtype, use_lds, st);
                         });
}

int dcp_clear_border_2d(const void* src, uint8_t* dst, int height, int width, long src_row_stride, int dtype, int connectivity, int invert,
                        int mem_kind, int device, void* stream) {
  bool host = false;
  int rc;
  if ((rc = check_plane_call(src, dst, height, width, src_row_stride, dtype, sizeof(uint8_t), mem_kind, &host)) != DCP_OK) return rc;
  if (connectivity != 4 && connectivity != 8) return fail(DCP_ERR_INVALID_ARG, "connectivity must be 4 or 8 (got %d)", connectivity);
  if (invert != 0 && invert != 1) return fail(DCP_ERR_INVALID_ARG, "invert must be 0 or 1 (got %d)", invert);
  DeviceScope scope(device);
  if (scope.status != hipSuccess) return fail(DCP_ERR_HIP, "cannot select device %d: %s", device, hipGetErrorString(scope.status));
  const bool use_lds = g_label_lds.load() != 0;
  hipStream_t st = (hipStream_t)stream;
  const size_t n = (size_t)height * (size_t)width;
  WorkspaceLease lease;          // the parent plane of the components and the plane of their roots
  if ((rc = lease.acquire(2 * n * sizeof(int32_t), st)) != DCP_OK) return rc;
  int32_t *parent = static_cast<int32_t*>(lease.buf), *root = parent + n;
  if (!host) {
    DCP_HIP(dcp::launch_clear_border(src, dst, parent, root, height, width, (int64_t)src_row_stride, dtype, connectivity == 8, invert != 0, use_lds, st));
    return DCP_OK;
  }
  return host_round_trip(packed_rows(src, dst, height, width, src_row_stride, (size_t)dcp::elem_size(dtype), sizeof(uint8_t)), st,
                         [&](const void* dsrc, void* ddst, void*, void*) {
                           return dcp::launch_clear_border(dsrc, static_cast<uint8_t*>(ddst), parent, root, height, width, (int64_t)width, dtype,
                                                           connectivity == 8, invert != 0, use_lds, st);
                         });
}

int dcp_label_measures_2d(const void* weights, const int32_t* labels, int height, int width, long weights_row_stride, long labels_row_stride,
                          int dtype, int num_labels, int64_t* sums, int32_t* boxes, int mem_kind, int device, void* stream) {
  bool host = false;
  int rc;
  if ((rc = mem_kind_of(mem_kind, &host)) != DCP_OK) return rc;
  if (dtype < 0 || dtype >= dcp::kNumElemTypes) return fail(DCP_ERR_INVALID_ARG, "unknown dtype %d", dtype);
  if (!labels) return fail(DCP_ERR_INVALID_ARG, "null labels pointer");
  if (!sums || !boxes) return fail(DCP_ERR_INVALID_ARG, "null sums / boxes pointer");
  if (height < 1 || width < 1) return fail(DCP_ERR_INVALID_ARG, "height and width must be at least 1 (got %d x %d)", height, width);
  if (labels_row_stride < width) return fail(DCP_ERR_INVALID_ARG, "labels_row_stride %ld is below the width %d", labels_row_stride, width);
  if (weights && weights_row_stride < width) return fail(DCP_ERR_INVALID_ARG, "weights_row_stride %ld is below the width %d", weights_row_stride, width);
  if (num_labels < 0) return fail(DCP_ERR_INVALID_ARG, "num_labels must not be negative (got %d)", num_labels);
  if (weights && dtype != dcp::kBool && dtype != dcp::kU8 && dtype != dcp::kI8 && dtype != dcp::kU16 && dtype != dcp::kI16)
    return fail(DCP_ERR_UNSUPPORTED, "dtype %d of the weights: bool and 8- / 16-bit integers only (their sums are exact in int64)", dtype);
  if ((int64_t)height * (int64_t)width > 2147483647LL)
    return fail(DCP_ERR_UNSUPPORTED, "height * width = %lld: labels and pixel indices are int32, at most 2^31 - 1 pixels", (long long)height * width);
  // |sum x v| <= H W max(H, W) 65535 must stay below 2^63: H W max(H, W) < 2^47
  if ((int64_t)height * (int64_t)width * (int64_t)(height > width ? height : width) >= ((int64_t)1 << 47))
    return fail(DCP_ERR_UNSUPPORTED, "height * width * max(height, width) * 65536 reaches 2^63 (%d x %d): an int64 sum could overflow", height, width);
  DeviceScope scope(device);
  if (scope.status != hipSuccess) return fail(DCP_ERR_HIP, "cannot select device %d: %s", device, hipGetErrorString(scope.status));
  if (num_labels == 0) return DCP_OK;
  hipStream_t st = (hipStream_t)stream;
  if (!host) {
    DCP_HIP(dcp::launch_label_measures(weights, labels, height, width, (int64_t)weights_row_stride, (int64_t)labels_row_stride, dtype, num_labels,
                                       reinterpret_cast<long long*>(sums), boxes, st));
    return DCP_OK;
  }
  // host memory: the weights into staging slot 0 and the labels into slot 2, rows packed; sums and boxes side by side in slot 1
  const size_t esz = (size_t)dcp::elem_size(dtype), num = (size_t)num_labels;
  const size_t sums_bytes = num * 4 * sizeof(int64_t), boxes_bytes = num * 4 * sizeof(int32_t);
  void *dw = nullptr, *dl = nullptr, *dout = nullptr;
  if (weights) DCP_HIP(g_staging.get(0, (size_t)height * width * esz, &dw));
  DCP_HIP(g_staging.get(2, (size_t)height * width * sizeof(int32_t), &dl));
  DCP_HIP(g_staging.get(1, sums_bytes + boxes_bytes, &dout));
  if (weights)
    DCP_HIP(hipMemcpy2DAsync(dw, (size_t)width * esz, weights, (size_t)weights_row_stride * esz, (size_t)width * esz, (size_t)height,
                             hipMemcpyHostToDevice, st));
  DCP_HIP(hipMemcpy2DAsync(dl, (size_t)width * sizeof(int32_t), labels, (size_t)labels_row_stride * sizeof(int32_t), (size_t)width * sizeof(int32_t),
                           (size_t)height, hipMemcpyHostToDevice, st));
  long long* dsums = static_cast<long long*>(dout);
  int32_t* dboxes = reinterpret_cast<int32_t*>(static_cast<char*>(dout) + sums_bytes);
  DCP_HIP(dcp::launch_label_measures(dw, static_cast<const int32_t*>(dl), height, width, (int64_t)width, (int64_t)width, dtype, num_labels, dsums,
                                     dboxes, st));
  DCP_HIP(hipMemcpyAsync(sums, dsums, sums_bytes, hipMemcpyDeviceToHost, st));
  DCP_HIP(hipMemcpyAsync(boxes, dboxes, boxes_bytes, hipMemcpyDeviceToHost, st));
  DCP_HIP(hipStreamSynchronize(st));
  return DCP_OK;
}

}  // extern "C"
