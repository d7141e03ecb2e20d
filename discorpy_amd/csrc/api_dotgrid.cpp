// api_dotgrid.cpp -- dcp_radon_padded_2d, dcp_nearest_sq_dists and dcp_box_moments_2d of the C ABI (include/discorpy_hip.h): plane calls
// (api_plane.h; the point table is a plane of two columns), their own checks, the tables' place in the spline workspace and the launches
// of dotgrid_kernels.hip.
#include "api_plane.h"

#include <cmath>

using namespace dcpapi;

namespace {

// [a, a + na) and [b, b + nb) share a byte
bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const char *a0 = (const char*)a, *a1 = a0 + na, *b0 = (const char*)b, *b1 = b0 + nb;
  return a0 < b1 && b0 < a1;
}

size_t plane_extent(const PlaneCall& c) { return ((size_t)(c.H - 1) * (size_t)c.rs + (size_t)c.W) * c.esz; }

}  // namespace

extern "C" {

int dcp_radon_padded_2d(const void* src, double* dst, int height, int width, long src_row_stride, int dtype, int nangles, const double* table,
                        int mem_kind, int device, void* stream) {
  PlaneCall c;
  int rc;
  // (the destination is not a plane of the source's shape: checked here, and the round trip of host memory is this call's own)
  if ((rc = make_plane_call(&c, src, nullptr, height, width, src_row_stride, dtype, 0, kSideLimit, kReadsWindow, mem_kind, device, stream)) != DCP_OK)
    return rc;
  if (dtype != dcp::kF32 && dtype != dcp::kF64) return fail(DCP_ERR_UNSUPPORTED, "dtype %d: the Radon transform takes float32 or float64", dtype);
  if (!dst || !table) return fail(DCP_ERR_INVALID_ARG, "null dst / table pointer");
  if (nangles < 1) return fail(DCP_ERR_INVALID_ARG, "nangles must be at least 1 (got %d)", nangles);
  const int longer = height > width ? height : width;
  if (longer > dcp::kRadonMaxSide) return fail(DCP_ERR_UNSUPPORTED, "padded side above %d (%d x %d): indices are int32", dcp::kRadonMaxSide, height, width);
  const int side = dcp::radon_padded_side(height, width);
  if (side > dcp::kRadonMaxSide)
    return fail(DCP_ERR_UNSUPPORTED, "padded side above %d (got %d for %d x %d): indices are int32", dcp::kRadonMaxSide, side, height, width);
  if (nangles > dcp::kRadonMaxAngles) return fail(DCP_ERR_UNSUPPORTED, "more than %d angles (got %d)", dcp::kRadonMaxAngles, nangles);
  const size_t out_bytes = (size_t)side * (size_t)nangles * sizeof(double);
  if (ranges_overlap(src, plane_extent(c), dst, out_bytes))
    return fail(DCP_ERR_INVALID_ARG, "src and dst overlap: every sample of the sinogram sums a line across the source");
  for (int i = 0; i < 4 * nangles; ++i)
    if (!std::isfinite(table[i])) return fail(DCP_ERR_INVALID_ARG, "table entry %d (angle %d) is not finite", i, i / 4);
  PlaneDevice on(c.device);
  if (on.rc != DCP_OK) return on.rc;
  WorkspaceLease lease;
  if ((rc = lease.acquire(dcp::radon_work_bytes(nangles), c.stream)) != DCP_OK) return rc;
  auto launch = [&](const void* s, void* d, int64_t rs) {
    return dcp::launch_radon_padded(s, static_cast<double*>(d), height, width, rs, dtype, nangles, table, lease.buf, c.stream);
  };
  if (!c.host) {
    DCP_HIP(launch(c.src, dst, c.rs));
    return DCP_OK;
  }
  HostTrip t = packed_rows(c);
  t.dst = dst;
  t.out_bytes = out_bytes;
  return host_round_trip(t, c.stream, [&](const void* dsrc, void* ddst, void*, void*) { return launch(dsrc, ddst, (int64_t)c.W); });
}

// The table of points is a plane of npoints rows and two columns of doubles, dense.
int dcp_nearest_sq_dists(const double* points, double* dst, int npoints, int mem_kind, int device, void* stream) {
  PlaneCall c;
  int rc;
  if (npoints < 1) return fail(DCP_ERR_INVALID_ARG, "npoints must be at least 1 (got %d)", npoints);
  if ((rc = make_plane_call(&c, points, nullptr, npoints, 2, 2, dcp::kF64, 0, kSideLimit, kReadsWindow, mem_kind, device, stream)) != DCP_OK) return rc;
  if (!dst) return fail(DCP_ERR_INVALID_ARG, "null dst pointer");
  if (npoints > dcp::kNearMaxPoints) return fail(DCP_ERR_UNSUPPORTED, "more than %d points (got %d)", dcp::kNearMaxPoints, npoints);
  const size_t out_bytes = (size_t)npoints * 4 * sizeof(double);
  if (ranges_overlap(points, plane_extent(c), dst, out_bytes))
    return fail(DCP_ERR_INVALID_ARG, "points and dst overlap: every row of dst reads every point");
  if (c.host)               // (device memory cannot be read here: its caller vouches for finite coordinates)
    for (int i = 0; i < 2 * npoints; ++i)
      if (!std::isfinite(points[i])) return fail(DCP_ERR_INVALID_ARG, "coordinate %d of point %d is not finite", i % 2, i / 2);
  PlaneDevice on(c.device);
  if (on.rc != DCP_OK) return on.rc;
  if (!c.host) {
    DCP_HIP(dcp::launch_nearest_sq_dists(points, dst, npoints, c.stream));
    return DCP_OK;
  }
  HostTrip t = packed_rows(c);
  t.dst = dst;
  t.out_bytes = out_bytes;
  return host_round_trip(t, c.stream, [&](const void* dsrc, void* ddst, void*, void*) {
    return dcp::launch_nearest_sq_dists(static_cast<const double*>(dsrc), static_cast<double*>(ddst), npoints, c.stream);
  });
}

int dcp_box_moments_2d(const void* src, int height, int width, long src_row_stride, int dtype, const int32_t* boxes, int nboxes, int64_t* sums,
                       int mem_kind, int device, void* stream) {
  PlaneCall c;
  int rc;
  if ((rc = make_plane_call(&c, src, nullptr, height, width, src_row_stride, dtype, 0, kPixelLimit, kReadsWindow, mem_kind, device, stream)) != DCP_OK)
    return rc;
  if (dtype != dcp::kBool && dtype != dcp::kU8 && dtype != dcp::kI8 && dtype != dcp::kU16 && dtype != dcp::kI16)
    return fail(DCP_ERR_UNSUPPORTED, "dtype %d: bool and 8- / 16-bit integers only (the images that are measured)", dtype);
  if (height > dcp::kBoxMaxSide || width > dcp::kBoxMaxSide)
    return fail(DCP_ERR_UNSUPPORTED, "height / width above %d (got %d x %d): a second moment could pass 2^60", dcp::kBoxMaxSide, height, width);
  if (nboxes < 0) return fail(DCP_ERR_INVALID_ARG, "nboxes must not be negative (got %d)", nboxes);
  if (nboxes > dcp::kBoxMaxBoxes) return fail(DCP_ERR_UNSUPPORTED, "more than %d boxes (got %d)", dcp::kBoxMaxBoxes, nboxes);
  if (nboxes == 0) return DCP_OK;
  if (!boxes || !sums) return fail(DCP_ERR_INVALID_ARG, "null boxes / sums pointer");
  const size_t out_bytes = (size_t)nboxes * 6 * sizeof(int64_t);
  if (ranges_overlap(src, plane_extent(c), sums, out_bytes)) return fail(DCP_ERR_INVALID_ARG, "src and sums overlap: every sum reads a box of the source");
  for (int b = 0; b < nboxes; ++b) {
    const int32_t* q = boxes + 4 * (size_t)b;
    if (q[1] < q[0] || q[3] < q[2]) continue;          // empty: zeros, wherever it is said to lie
    if (q[0] < 0 || q[1] >= height || q[2] < 0 || q[3] >= width)
      return fail(DCP_ERR_INVALID_ARG, "box %d (rows %d..%d, columns %d..%d) lies outside the %d x %d plane", b, q[0], q[1], q[2], q[3], height, width);
  }
  PlaneDevice on(c.device);
  if (on.rc != DCP_OK) return on.rc;
  WorkspaceLease lease;
  if ((rc = lease.acquire(dcp::box_work_bytes(nboxes), c.stream)) != DCP_OK) return rc;
  auto launch = [&](const void* s, void* d, int64_t rs) {
    return dcp::launch_box_moments(s, height, width, rs, dtype, boxes, nboxes, static_cast<long long*>(d), lease.buf, c.stream);
  };
  if (!c.host) {
    DCP_HIP(launch(c.src, sums, c.rs));
    return DCP_OK;
  }
  HostTrip t = packed_rows(c);
  t.dst = sums;
  t.out_bytes = out_bytes;
  return host_round_trip(t, c.stream, [&](const void* dsrc, void* ddst, void*, void*) { return launch(dsrc, ddst, (int64_t)c.W); });
}

}  // extern "C"
