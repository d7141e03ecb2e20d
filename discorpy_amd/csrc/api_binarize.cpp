// api_binarize.cpp -- dcp_abs_2d, dcp_minmax_2d, dcp_histogram_2d, dcp_threshold_2d and dcp_morph_cross_2d of the C ABI
// (include/discorpy_hip.h): plane calls (api_plane.h), their own checks, the scratch (leased from the spline workspace) and the launches
// of binarize_kernels.hip.  (dcp_clear_border_2d is in api_label.cpp, beside the labelling it reuses.)
#include "api_plane.h"

#include <cstring>

using namespace dcpapi;

namespace {

bool reducible(int dtype) {
  return dtype == dcp::kF32 || dtype == dcp::kF64 || dtype == dcp::kU8 || dtype == dcp::kI8 || dtype == dcp::kU16 || dtype == dcp::kI16;
}

}  // namespace

extern "C" {

int dcp_abs_2d(const void* src, void* dst, int height, int width, long src_row_stride, int dtype, int mem_kind, int device, void* stream) {
  PlaneCall c;
  int rc;
  if ((rc = make_plane_call(&c, src, dst, height, width, src_row_stride, dtype, kSameElem, kPixelLimit, kComponentReach, mem_kind, device, stream)) != DCP_OK)
    return rc;
  return run_plane(c, false, 0, [&](const void* s, void* d, int64_t rs, void*) { return dcp::launch_abs(s, d, height, width, rs, dtype, c.stream); });
}

int dcp_minmax_2d(const void* src, int height, int width, long src_row_stride, int dtype, double* minmax_out, int64_t* nonfinite_out, int mem_kind,
                  int device, void* stream) {
  PlaneCall c;
  int rc;
  if ((rc = make_plane_call(&c, src, nullptr, height, width, src_row_stride, dtype, 0, kPixelLimit, nullptr, mem_kind, device, stream)) != DCP_OK) return rc;
  if (!minmax_out || !nonfinite_out) return fail(DCP_ERR_INVALID_ARG, "null minmax_out / nonfinite_out pointer");
  if (!reducible(dtype))
    return fail(DCP_ERR_UNSUPPORTED, "dtype %d: float32, float64 and 8- / 16-bit integers only (a double holds each of their values exactly)", dtype);
  const size_t part = (size_t)3 * dcp::kReduceMaxBlocks;          // the workgroups' triples, then min, max and the count
  double got[3];          // (the third word carries the int64)
  rc = run_plane(c, true, (part + 3) * sizeof(double), [&](const void* s, void*, int64_t rs, void* work) {
    double *partials = static_cast<double*>(work), *out = partials + part;
    hipError_t e = dcp::launch_minmax(s, height, width, rs, dtype, partials, out, reinterpret_cast<long long*>(out + 2), c.stream);
    if (e != hipSuccess) return e;
    return hipMemcpyAsync(got, out, sizeof(got), hipMemcpyDeviceToHost, c.stream);
  });
  if (rc != DCP_OK) return rc;
  minmax_out[0] = got[0];
  minmax_out[1] = got[1];
  long long count;
  memcpy(&count, &got[2], sizeof(count));
  *nonfinite_out = (int64_t)count;
  return DCP_OK;
}

int dcp_histogram_2d(const void* src, int height, int width, long src_row_stride, int dtype, const void* edges, int nbins, int64_t first,
                     int64_t* counts_out, int mem_kind, int device, void* stream) {
  PlaneCall c;
  int rc;
  if ((rc = make_plane_call(&c, src, nullptr, height, width, src_row_stride, dtype, 0, kPixelLimit, nullptr, mem_kind, device, stream)) != DCP_OK) return rc;
  if (!counts_out) return fail(DCP_ERR_INVALID_ARG, "null counts_out pointer");
  if (nbins < 1) return fail(DCP_ERR_INVALID_ARG, "nbins must be at least 1 (got %d)", nbins);
  if (!reducible(dtype)) return fail(DCP_ERR_UNSUPPORTED, "dtype %d: float32, float64 and 8- / 16-bit integers only", dtype);
  if (nbins > 65536) return fail(DCP_ERR_UNSUPPORTED, "nbins %d: at most 65536 bins", nbins);
  const bool is_float = dtype == dcp::kF32 || dtype == dcp::kF64;
  if (is_float && !edges) return fail(DCP_ERR_INVALID_ARG, "null edges pointer: a float plane is counted between nbins + 1 edges");
  if (!is_float && edges) return fail(DCP_ERR_INVALID_ARG, "edges given for an integer plane: it is counted per value from `first`");
  const bool use_lds = g_hist_lds.load() != 0;
  const size_t count_bytes = (size_t)nbins * sizeof(int64_t), edge_bytes = is_float ? (size_t)(nbins + 1) * c.esz : 0;
  // the counts, then the edges
  return run_plane(c, true, count_bytes + edge_bytes + 8, [&](const void* s, void*, int64_t rs, void* work) {
    long long* dcounts = static_cast<long long*>(work);
    void* dedges = is_float ? static_cast<void*>(static_cast<char*>(work) + count_bytes) : nullptr;
    hipError_t e = hipSuccess;
    if (is_float && (e = hipMemcpyAsync(dedges, edges, edge_bytes, hipMemcpyHostToDevice, c.stream)) != hipSuccess) return e;
    if ((e = dcp::launch_histogram(s, height, width, rs, dtype, dedges, nbins, (long long)first, dcounts, use_lds, c.stream)) != hipSuccess) return e;
    return hipMemcpyAsync(counts_out, dcounts, count_bytes, hipMemcpyDeviceToHost, c.stream);
  });
}

// `count`: device memory -- a device word the kernel adds to; host memory -- a host word the call adds to, through a leased device word
int dcp_threshold_2d(const void* src, uint8_t* dst, int height, int width, long src_row_stride, int dtype, double thres, int64_t* count,
                     int mem_kind, int device, void* stream) {
  PlaneCall c;
  int rc;
  if ((rc = make_plane_call(&c, src, dst, height, width, src_row_stride, dtype, sizeof(uint8_t), kPixelLimit, kComponentReach, mem_kind, device, stream)) != DCP_OK)
    return rc;
  long long got = 0;
  rc = run_plane(c, false, c.host ? sizeof(long long) : 0, [&](const void* s, void* d, int64_t rs, void* word) {
    long long* dcount = c.host ? static_cast<long long*>(word) : reinterpret_cast<long long*>(count);
    hipError_t e = c.host ? hipMemsetAsync(dcount, 0, sizeof(long long), c.stream) : hipSuccess;
    if (e != hipSuccess) return e;
    e = dcp::launch_threshold(s, static_cast<uint8_t*>(d), height, width, rs, dtype, thres, dcount, c.stream);
    if (e != hipSuccess || !c.host) return e;
    return hipMemcpyAsync(&got, dcount, sizeof(got), hipMemcpyDeviceToHost, c.stream);
  });
  if (rc != DCP_OK) return rc;
  if (c.host && count) *count += (int64_t)got;
  return DCP_OK;
}

int dcp_morph_cross_2d(const uint8_t* src, uint8_t* dst, int height, int width, long src_row_stride, int op, int mem_kind, int device,
                       void* stream) {
  PlaneCall c;
  int rc;
  if ((rc = make_plane_call(&c, src, dst, height, width, src_row_stride, dcp::kU8, sizeof(uint8_t), kPixelLimit, kComponentReach, mem_kind, device, stream)) != DCP_OK)
    return rc;
  if (op < 0 || op > 2) return fail(DCP_ERR_INVALID_ARG, "op must be 0 (erosion), 1 (dilation) or 2 (opening) (got %d)", op);
  const bool fused = g_morph_fused.load() != 0;
  // the eroded plane of the two-launch opening
  return run_plane(c, false, op == 2 && !fused ? (size_t)height * (size_t)width : 0, [&](const void* s, void* d, int64_t rs, void* tmp) {
    return dcp::launch_morph_cross(static_cast<const uint8_t*>(s), static_cast<uint8_t*>(d), static_cast<uint8_t*>(tmp), height, width, rs, op, fused, c.stream);
  });
}

}  // extern "C"
