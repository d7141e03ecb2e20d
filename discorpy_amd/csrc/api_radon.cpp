// api_radon.cpp -- dcp_radon_2d of the C ABI (include/discorpy_hip.h): a plane call (api_plane.h) on the square plane the sinogram is
// taken from, its argument checks, the angle table's place in the spline workspace and the launch of radon_kernels.hip.
#include "api_plane.h"

#include <cmath>

using namespace dcpapi;

extern "C" {

int dcp_radon_2d(const void* src, double* dst, int side, long src_row_stride, int dtype, int nangles, const double* table, int mem_kind,
                 int device, void* stream) {
  PlaneCall c;
  int rc;
  // (the destination is not a plane of the source's shape: checked here, and the round trip of host memory is this call's own)
  if ((rc = make_plane_call(&c, src, nullptr, side, side, src_row_stride, dtype, 0, kSideLimit, kReadsWindow, mem_kind, device, stream)) != DCP_OK)
    return rc;
  if (dtype != dcp::kF32 && dtype != dcp::kF64) return fail(DCP_ERR_UNSUPPORTED, "dtype %d: the Radon transform takes float32 or float64", dtype);
  if (!dst || !table) return fail(DCP_ERR_INVALID_ARG, "null dst / table pointer");
  if (nangles < 1) return fail(DCP_ERR_INVALID_ARG, "nangles must be at least 1 (got %d)", nangles);
  if (side > dcp::kRadonMaxSide) return fail(DCP_ERR_UNSUPPORTED, "side above %d (got %d): indices are int32", dcp::kRadonMaxSide, side);
  if (nangles > dcp::kRadonMaxAngles) return fail(DCP_ERR_UNSUPPORTED, "more than %d angles (got %d)", dcp::kRadonMaxAngles, nangles);
  const size_t out_bytes = (size_t)side * (size_t)nangles * sizeof(double);
  {
    const char *d0 = (const char*)dst, *d1 = d0 + out_bytes;
    const char *s0 = (const char*)src, *s1 = s0 + ((size_t)(side - 1) * (size_t)src_row_stride + (size_t)side) * c.esz;
    if (s0 < d1 && d0 < s1) return fail(DCP_ERR_INVALID_ARG, "src and dst overlap: every sample of the sinogram sums a line across the source");
  }
  for (int i = 0; i < 4 * nangles; ++i)
    if (!std::isfinite(table[i])) return fail(DCP_ERR_INVALID_ARG, "table entry %d (angle %d) is not finite", i, i / 4);
  PlaneDevice on(c.device);
  if (on.rc != DCP_OK) return on.rc;
  WorkspaceLease lease;
  if ((rc = lease.acquire(dcp::radon_work_bytes(nangles), c.stream)) != DCP_OK) return rc;
  auto launch = [&](const void* s, void* d, int64_t rs) {
    return dcp::launch_radon(s, static_cast<double*>(d), side, rs, dtype, nangles, table, lease.buf, c.stream);
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

}  // extern "C"
