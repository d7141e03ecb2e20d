// api_binarize.cpp -- dcp_abs_2d, dcp_minmax_2d, dcp_histogram_2d, dcp_threshold_2d and dcp_morph_cross_2d of the C ABI
// (include/discorpy_hip.h): the argument checks, the scratch (leased from the spline workspace), the staged round trip of host memory
// and the launches of binarize_kernels.hip.  (dcp_clear_border_2d is in api_label.cpp, beside the labelling it reuses.)
#include "api_common.h"

#include <cstring>

using namespace dcpapi;

namespace {

bool reducible(int dtype) {
  return dtype == dcp::kF32 || dtype == dcp::kF64 || dtype == dcp::kU8 || dtype == dcp::kI8 || dtype == dcp::kU16 || dtype == dcp::kI16;
}

}  // namespace

extern "C" {

int dcp_abs_2d(const void* src, void* dst, int height, int width, long src_row_stride, int dtype, int mem_kind, int device, void* stream) {
  bool host = false;
  int rc;
  const size_t esz = dtype >= 0 && dtype < dcp::kNumElemTypes ? (size_t)dcp::elem_size(dtype) : 1;
  if ((rc = check_plane_call(src, dst, height, width, src_row_stride, dtype, esz, mem_kind, &host)) != DCP_OK) return rc;
  DeviceScope scope(device);
  if (scope.status != hipSuccess) return fail(DCP_ERR_HIP, "cannot select device %d: %s", device, hipGetErrorString(scope.status));
  hipStream_t st = (hipStream_t)stream;
  if (!host) {
    DCP_HIP(dcp::launch_abs(src, dst, height, width, (int64_t)src_row_stride, dtype, st));
    return DCP_OK;
  }
  return host_round_trip(packed_rows(src, dst, height, width, src_row_stride, esz, esz), st, [&](const void* dsrc, void* ddst, void*, void*) {
    return dcp::launch_abs(dsrc, ddst, height, width, (int64_t)width, dtype, st);
  });
}

int dcp_minmax_2d(const void* src, int height, int width, long src_row_stride, int dtype, double* minmax_out, int64_t* nonfinite_out, int mem_kind,
                  int device, void* stream) {
  bool host = false;
  int rc;
  if ((rc = check_plane_call(src, nullptr, height, width, src_row_stride, dtype, 0, mem_kind, &host)) != DCP_OK) return rc;
  if (!minmax_out || !nonfinite_out) return fail(DCP_ERR_INVALID_ARG, "null minmax_out / nonfinite_out pointer");
  if (!reducible(dtype))
    return fail(DCP_ERR_UNSUPPORTED, "dtype %d: float32, float64 and 8- / 16-bit integers only (a double holds each of their values exactly)", dtype);
  DeviceScope scope(device);
  if (scope.status != hipSuccess) return fail(DCP_ERR_HIP, "cannot select device %d: %s", device, hipGetErrorString(scope.status));
  hipStream_t st = (hipStream_t)stream;
  WorkspaceLease lease;          // the workgroups' triples, then min, max and the count
  const size_t part = (size_t)3 * dcp::kReduceMaxBlocks;
  if ((rc = lease.acquire((part + 3) * sizeof(double), st)) != DCP_OK) return rc;
  double *partials = static_cast<double*>(lease.buf), *out = partials + part;
  long long* bad = reinterpret_cast<long long*>(out + 2);
  double got[3];          // (the third word carries the int64)
  auto run = [&](const void* dsrc, int64_t stride) {
    hipError_t e = dcp::launch_minmax(dsrc, height, width, stride, dtype, partials, out, bad, st);
    if (e != hipSuccess) return e;
    return hipMemcpyAsync(got, out, sizeof(got), hipMemcpyDeviceToHost, st);
  };
  if (!host) {
    DCP_HIP(run(src, (int64_t)src_row_stride));
    DCP_HIP(hipStreamSynchronize(st));
  } else {
    rc = host_round_trip(packed_rows(src, nullptr, height, width, src_row_stride, (size_t)dcp::elem_size(dtype), 0), st,
                         [&](const void* dsrc, void*, void*, void*) { return run(dsrc, (int64_t)width); });
    if (rc != DCP_OK) return rc;
  }
  minmax_out[0] = got[0];
  minmax_out[1] = got[1];
  long long count;
  memcpy(&count, &got[2], sizeof(count));
  *nonfinite_out = (int64_t)count;
  return DCP_OK;
}

int dcp_histogram_2d(const void* src, int height, int width, long src_row_stride, int dtype, const void* edges, int nbins, int64_t first,
                     int64_t* counts_out, int mem_kind, int device, void* stream) {
  bool host = false;
  int rc;
  if ((rc = check_plane_call(src, nullptr, height, width, src_row_stride, dtype, 0, mem_kind, &host)) != DCP_OK) return rc;
  if (!counts_out) return fail(DCP_ERR_INVALID_ARG, "null counts_out pointer");
  if (nbins < 1) return fail(DCP_ERR_INVALID_ARG, "nbins must be at least 1 (got %d)", nbins);
  if (!reducible(dtype)) return fail(DCP_ERR_UNSUPPORTED, "dtype %d: float32, float64 and 8- / 16-bit integers only", dtype);
  if (nbins > 65536) return fail(DCP_ERR_UNSUPPORTED, "nbins %d: at most 65536 bins", nbins);
  const bool is_float = dtype == dcp::kF32 || dtype == dcp::kF64;
  if (is_float && !edges) return fail(DCP_ERR_INVALID_ARG, "null edges pointer: a float plane is counted between nbins + 1 edges");
  if (!is_float && edges) return fail(DCP_ERR_INVALID_ARG, "edges given for an integer plane: it is counted per value from `first`");
  DeviceScope scope(device);
  if (scope.status != hipSuccess) return fail(DCP_ERR_HIP, "cannot select device %d: %s", device, hipGetErrorString(scope.status));
  hipStream_t st = (hipStream_t)stream;
  const bool use_lds = g_hist_lds.load() != 0;
  WorkspaceLease lease;          // the counts, then the edges
  const size_t count_bytes = (size_t)nbins * sizeof(int64_t), edge_bytes = is_float ? (size_t)(nbins + 1) * (size_t)dcp::elem_size(dtype) : 0;
  if ((rc = lease.acquire(count_bytes + edge_bytes + 8, st)) != DCP_OK) return rc;
  long long* dcounts = static_cast<long long*>(lease.buf);
  void* dedges = is_float ? static_cast<void*>(static_cast<char*>(lease.buf) + count_bytes) : nullptr;
  auto run = [&](const void* dsrc, int64_t stride) {
    hipError_t e = hipSuccess;
    if (is_float && (e = hipMemcpyAsync(dedges, edges, edge_bytes, hipMemcpyHostToDevice, st)) != hipSuccess) return e;
    if ((e = dcp::launch_histogram(dsrc, height, width, stride, dtype, dedges, nbins, (long long)first, dcounts, use_lds, st)) != hipSuccess) return e;
    return hipMemcpyAsync(counts_out, dcounts, count_bytes, hipMemcpyDeviceToHost, st);
  };
  if (!host) {
    DCP_HIP(run(src, (int64_t)src_row_stride));
    DCP_HIP(hipStreamSynchronize(st));
    return DCP_OK;
  }
  return host_round_trip(packed_rows(src, nullptr, height, width, src_row_stride, (size_t)dcp::elem_size(dtype), 0), st,
                         [&](const void* dsrc, void*, void*, void*) { return run(dsrc, (int64_t)width); });
}

int dcp_threshold_2d(const void* src, uint8_t* dst, int height, int width, long src_row_stride, int dtype, double thres, int64_t* count,
                     int mem_kind, int device, void* stream) {
  bool host = false;
  int rc;
  if ((rc = check_plane_call(src, dst, height, width, src_row_stride, dtype, sizeof(uint8_t), mem_kind, &host)) != DCP_OK) return rc;
  DeviceScope scope(device);
  if (scope.status != hipSuccess) return fail(DCP_ERR_HIP, "cannot select device %d: %s", device, hipGetErrorString(scope.status));
  hipStream_t st = (hipStream_t)stream;
  if (!host) {
    DCP_HIP(dcp::launch_threshold(src, dst, height, width, (int64_t)src_row_stride, dtype, thres, reinterpret_cast<long long*>(count), st));
    return DCP_OK;
  }
  WorkspaceLease lease;          // the count of a host call
  if ((rc = lease.acquire(8, st)) != DCP_OK) return rc;
  long long* dcount = static_cast<long long*>(lease.buf);
  long long got = 0;
  rc = host_round_trip(packed_rows(src, dst, height, width, src_row_stride, (size_t)dcp::elem_size(dtype), sizeof(uint8_t)), st,
                       [&](const void* dsrc, void* ddst, void*, void*) {
                         hipError_t e = hipMemsetAsync(dcount, 0, sizeof(long long), st);
                         if (e != hipSuccess) return e;
                         e = dcp::launch_threshold(dsrc, static_cast<uint8_t*>(ddst), height, width, (int64_t)width, dtype, thres, dcount, st);
                         if (e != hipSuccess) return e;
                         return hipMemcpyAsync(&got, dcount, sizeof(got), hipMemcpyDeviceToHost, st);
                       });
  if (rc != DCP_OK) return rc;
  if (count) *count += (int64_t)got;
  return DCP_OK;
}

int dcp_morph_cross_2d(const uint8_t* src, uint8_t* dst, int height, int width, long src_row_stride, int op, int mem_kind, int device,
                       void* stream) {
  bool host = false;
  int rc;
  if ((rc = check_plane_call(src, dst, height, width, src_row_stride, dcp::kU8, sizeof(uint8_t), mem_kind, &host)) != DCP_OK) return rc;
  if (op < 0 || op > 2) return fail(DCP_ERR_INVALID_ARG, "op must be 0 (erosion), 1 (dilation) or 2 (opening) (got %d)", op);
  DeviceScope scope(device);
  if (scope.status != hipSuccess) return fail(DCP_ERR_HIP, "cannot select device %d: %s", device, hipGetErrorString(scope.status));
  hipStream_t st = (hipStream_t)stream;
  const bool fused = g_morph_fused.load() != 0;
  WorkspaceLease lease;          // the eroded plane of the two-launch opening
  uint8_t* tmp = nullptr;
  if (op == 2 && !fused) {
    if ((rc = lease.acquire((size_t)height * (size_t)width, st)) != DCP_OK) return rc;
    tmp = static_cast<uint8_t*>(lease.buf);
  }
  if (!host) {
    DCP_HIP(dcp::launch_morph_cross(src, dst, tmp, height, width, (int64_t)src_row_stride, op, fused, st));
    return DCP_OK;
  }
  return host_round_trip(packed_rows(src, dst, height, width, src_row_stride, 1, 1), st, [&](const void* dsrc, void* ddst, void*, void*) {
    return dcp::launch_morph_cross(static_cast<const uint8_t*>(dsrc), static_cast<uint8_t*>(ddst), tmp, height, width, (int64_t)width, op, fused, st);
  });
}

}  // extern "C"
