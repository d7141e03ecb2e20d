// api_label.cpp -- dcp_label_2d, dcp_label_measures_2d, dcp_fill_holes_2d and dcp_clear_border_2d of the C ABI (include/discorpy_hip.h): plane
// calls (api_plane.h), their own checks, the working planes (leased from the spline workspace) and the launches of label_kernels.hip.
#include "api_plane.h"

using namespace dcpapi;

extern "C" {

int dcp_label_2d(const void* src, int32_t* dst, int height, int width, long src_row_stride, int dtype, int connectivity, int* num_labels_out,
                 int mem_kind, int device, void* stream) {
  PlaneCall c;
  int rc;
  if ((rc = make_plane_call(&c, src, dst, height, width, src_row_stride, dtype, sizeof(int32_t), kPixelLimit, kComponentReach, mem_kind, device, stream)) != DCP_OK)
    return rc;
  if (connectivity != 4 && connectivity != 8) return fail(DCP_ERR_INVALID_ARG, "connectivity must be 4 or 8 (got %d)", connectivity);
  if (!num_labels_out) return fail(DCP_ERR_INVALID_ARG, "null num_labels_out pointer");
  const bool use_lds = g_label_lds.load() != 0;
  // the parent plane (the ranks' afterwards) and, behind it, the per-block root counts with the total in their last word
  const size_t n = (size_t)height * (size_t)width, words = dcp::label_count_words(height, width);
  int32_t total = 0;
  rc = run_plane(c, true, (n + words) * sizeof(int32_t), [&](const void* s, void* d, int64_t rs, void* work) {
    int32_t *parent = static_cast<int32_t*>(work), *counts = parent + n;
    hipError_t e = dcp::launch_label(s, static_cast<int32_t*>(d), parent, counts, height, width, rs, dtype, connectivity == 8, use_lds, c.stream);
    if (e != hipSuccess) return e;
    return hipMemcpyAsync(&total, counts + words - 1, sizeof(total), hipMemcpyDeviceToHost, c.stream);
  });
  if (rc != DCP_OK) return rc;
  *num_labels_out = (int)total;
  return DCP_OK;
}

int dcp_fill_holes_2d(const void* src, uint8_t* dst, int height, int width, long src_row_stride, int dtype, int mem_kind, int device, void* stream) {
  PlaneCall c;
  int rc;
  if ((rc = make_plane_call(&c, src, dst, height, width, src_row_stride, dtype, sizeof(uint8_t), kPixelLimit, kComponentReach, mem_kind, device, stream)) != DCP_OK)
    return rc;
  const bool use_lds = g_label_lds.load() != 0;
  const size_t n = (size_t)height * (size_t)width;
  // the parent plane of the complement's components and the plane of their roots
  return run_plane(c, false, 2 * n * sizeof(int32_t), [&](const void* s, void* d, int64_t rs, void* work) {
    int32_t *parent = static_cast<int32_t*>(work), *root = parent + n;
    return dcp::launch_fill_holes(s, static_cast<uint8_t*>(d), parent, root, height, width, rs, dtype, use_lds, c.stream);
  });
}

int dcp_clear_border_2d(const void* src, uint8_t* dst, int height, int width, long src_row_stride, int dtype, int connectivity, int invert,
                        int mem_kind, int device, void* stream) {
  PlaneCall c;
  int rc;
  if ((rc = make_plane_call(&c, src, dst, height, width, src_row_stride, dtype, sizeof(uint8_t), kPixelLimit, kComponentReach, mem_kind, device, stream)) != DCP_OK)
    return rc;
  if (connectivity != 4 && connectivity != 8) return fail(DCP_ERR_INVALID_ARG, "connectivity must be 4 or 8 (got %d)", connectivity);
  if (invert != 0 && invert != 1) return fail(DCP_ERR_INVALID_ARG, "invert must be 0 or 1 (got %d)", invert);
  const bool use_lds = g_label_lds.load() != 0;
  const size_t n = (size_t)height * (size_t)width;
  // the parent plane of the components and the plane of their roots
  return run_plane(c, false, 2 * n * sizeof(int32_t), [&](const void* s, void* d, int64_t rs, void* work) {
    int32_t *parent = static_cast<int32_t*>(work), *root = parent + n;
    return dcp::launch_clear_border(s, static_cast<uint8_t*>(d), parent, root, height, width, rs, dtype, connectivity == 8, invert != 0, use_lds, c.stream);
  });
}

// Two source planes with strides of their own: the shared checks piece by piece, and a staging of its own for host memory (HostTrip
// carries one strided source).
int dcp_label_measures_2d(const void* weights, const int32_t* labels, int height, int width, long weights_row_stride, long labels_row_stride,
                          int dtype, int num_labels, int64_t* sums, int32_t* boxes, int mem_kind, int device, void* stream) {
  bool host = false;
  int rc;
  if ((rc = mem_kind_of(mem_kind, &host)) != DCP_OK) return rc;
  if ((rc = check_plane_shape(height, width, dtype, kPixelLimit)) != DCP_OK) return rc;
  if (!labels) return fail(DCP_ERR_INVALID_ARG, "null labels pointer");
  if (!sums || !boxes) return fail(DCP_ERR_INVALID_ARG, "null sums / boxes pointer");
  if ((rc = check_row_stride("labels_row_stride", labels_row_stride, width)) != DCP_OK) return rc;
  if (weights && (rc = check_row_stride("weights_row_stride", weights_row_stride, width)) != DCP_OK) return rc;
  if (num_labels < 0) return fail(DCP_ERR_INVALID_ARG, "num_labels must not be negative (got %d)", num_labels);
  if (weights && dtype != dcp::kBool && dtype != dcp::kU8 && dtype != dcp::kI8 && dtype != dcp::kU16 && dtype != dcp::kI16)
    return fail(DCP_ERR_UNSUPPORTED, "dtype %d of the weights: bool and 8- / 16-bit integers only (their sums are exact in int64)", dtype);
  // |sum x v| <= H W max(H, W) 65535 must stay below 2^63: H W max(H, W) < 2^47
  if ((int64_t)height * (int64_t)width * (int64_t)(height > width ? height : width) >= ((int64_t)1 << 47))
    return fail(DCP_ERR_UNSUPPORTED, "height * width * max(height, width) * 65536 reaches 2^63 (%d x %d): an int64 sum could overflow", height, width);
  PlaneDevice on(device);
  if (on.rc != DCP_OK) return on.rc;
  if (num_labels == 0) return DCP_OK;
  hipStream_t st = (hipStream_t)stream;
  const void* dw = weights;
  const int32_t* dl = labels;
  int64_t w_stride = weights_row_stride, l_stride = labels_row_stride;
  long long* dsums = reinterpret_cast<long long*>(sums);
  int32_t* dboxes = boxes;
  const size_t sums_bytes = (size_t)num_labels * 4 * sizeof(int64_t), boxes_bytes = (size_t)num_labels * 4 * sizeof(int32_t);
  if (host) {          // the weights into staging slot 0 and the labels into slot 2, rows packed; sums and boxes side by side in slot 1
    const size_t esz = (size_t)dcp::elem_size(dtype), wrow = (size_t)width * esz, lrow = (size_t)width * sizeof(int32_t);
    void *up_w = nullptr, *up_l = nullptr, *out = nullptr;
    if (weights) DCP_HIP(g_staging.get(0, (size_t)height * wrow, &up_w));
    DCP_HIP(g_staging.get(2, (size_t)height * lrow, &up_l));
    DCP_HIP(g_staging.get(1, sums_bytes + boxes_bytes, &out));
    if (weights) DCP_HIP(hipMemcpy2DAsync(up_w, wrow, weights, (size_t)weights_row_stride * esz, wrow, (size_t)height, hipMemcpyHostToDevice, st));
    DCP_HIP(hipMemcpy2DAsync(up_l, lrow, labels, (size_t)labels_row_stride * sizeof(int32_t), lrow, (size_t)height, hipMemcpyHostToDevice, st));
    dw = up_w;
    dl = static_cast<const int32_t*>(up_l);
    w_stride = l_stride = width;
    dsums = static_cast<long long*>(out);
    dboxes = reinterpret_cast<int32_t*>(static_cast<char*>(out) + sums_bytes);
  }
  DCP_HIP(dcp::launch_label_measures(dw, dl, height, width, w_stride, l_stride, dtype, num_labels, dsums, dboxes, st));
  if (!host) return DCP_OK;
  DCP_HIP(hipMemcpyAsync(sums, dsums, sums_bytes, hipMemcpyDeviceToHost, st));
  DCP_HIP(hipMemcpyAsync(boxes, dboxes, boxes_bytes, hipMemcpyDeviceToHost, st));
  DCP_HIP(hipStreamSynchronize(st));
  return DCP_OK;
}

}  // extern "C"
