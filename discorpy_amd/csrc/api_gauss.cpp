// api_gauss.cpp -- dcp_correlate_sym_2d of the C ABI (include/discorpy_hip.h): a plane call (api_plane.h), the checks of the weights and
// the boundary mode, the plane between the two passes (leased from the spline workspace) and the launch of gauss_kernels.hip.
#include "api_plane.h"

#include <cstring>

using namespace dcpapi;

// 2 r + 1 weights that read the same from both ends, compared as bit patterns
static bool symmetric_to_the_bit(const double* w, int r) {
  for (int k = 0; k < r; ++k)
    if (memcmp(&w[k], &w[2 * r - k], sizeof(double)) != 0) return false;
  return true;
}

extern "C" {

int dcp_correlate_sym_2d(const void* src, void* dst, int height, int width, long src_row_stride, int dtype, const double* weights_y,
                         int radius_y, const double* weights_x, int radius_x, int mode, double cval, int mem_kind, int device, void* stream) {
  PlaneCall c;
  int rc;
  if ((rc = make_plane_call(&c, src, dst, height, width, src_row_stride, dtype, kSameElem, kSideLimit, kReadsNeighbourhood, mem_kind, device, stream)) != DCP_OK)
    return rc;
  if (dtype == dcp::kBool) return fail(DCP_ERR_UNSUPPORTED, "dtype bool: scipy's filters do not take it either");
  if (mode < DCP_MODE_REFLECT || mode > DCP_MODE_WRAP) return fail(DCP_ERR_INVALID_ARG, "unknown boundary mode %d", mode);
  if (radius_y < -1 || radius_x < -1) return fail(DCP_ERR_INVALID_ARG, "radius_y and radius_x must be at least -1 (got %d, %d)", radius_y, radius_x);
  if (!weights_y) radius_y = -1;
  if (!weights_x) radius_x = -1;
  if (radius_y > dcp::kGaussMaxRadius || radius_x > dcp::kGaussMaxRadius)
    return fail(DCP_ERR_UNSUPPORTED, "radius_y / radius_x above %d (got %d, %d)", dcp::kGaussMaxRadius, radius_y, radius_x);
  if (radius_y >= 0 && !symmetric_to_the_bit(weights_y, radius_y)) return fail(DCP_ERR_INVALID_ARG, "weights_y are not symmetric to the bit");
  if (radius_x >= 0 && !symmetric_to_the_bit(weights_x, radius_x)) return fail(DCP_ERR_INVALID_ARG, "weights_x are not symmetric to the bit");
  const int lds_mode = g_gauss_lds.load();
  // the plane between the passes of the per-axis route
  const bool two_passes = radius_y >= 0 && radius_x >= 0 && !dcp::gauss_takes_lds(dtype, radius_y, radius_x, lds_mode);
  return run_plane(c, false, two_passes ? (size_t)height * (size_t)width * c.esz : 0, [&](const void* s, void* d, int64_t rs, void* tmp) {
    return dcp::launch_gauss(s, d, tmp, height, width, rs, dtype, weights_y, radius_y, weights_x, radius_x, mode, cval, lds_mode, c.stream);
  });
}

}  // extern "C"
