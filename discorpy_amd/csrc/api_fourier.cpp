// api_fourier.cpp -- dcp_fourier_gauss_2d of the C ABI (include/discorpy_hip.h): a plane call (api_plane.h), the checks of the pad, its mode
// and the four tap tables, the support radius of each axis (a bound on what the truncated sums leave out, not a measurement), the
// workspace (the planes between the two passes and the tables' device copies, one lease of the spline workspace) and the launch of
// fourier_kernels.hip.
#include "api_plane.h"

#include <cmath>

using namespace dcpapi;

// The smallest radius r such that the taps left out, r < |d| < n - r, sum to at most 2^-56 of the whole table in |re| + |im|; n / 2 (every
// tap kept) where no smaller one does.  False for a tap that is not finite.  The omission of a pass is then at most
// 2^-56 max|m| sum|a|, an eighth of float64's unit roundoff on the scale of the result.
static bool support_radius(const double* re, const double* im, int n, int* radius) {
  const int len = 2 * n - 1, mid = n - 1;
  double total = 0.0;
  for (int i = 0; i < len; ++i) {
    if (!std::isfinite(re[i]) || !std::isfinite(im[i])) return false;
    total += std::fabs(re[i]) + std::fabs(im[i]);
  }
  auto mag = [&](int d) { return std::fabs(re[mid + d]) + std::fabs(im[mid + d]) + std::fabs(re[mid - d]) + std::fabs(im[mid - d]); };
  const double allowed = std::ldexp(total, -56);
  int r = n / 2;                 // 2 r + 1 >= n: nothing lies strictly between r and n - r
  double dropped = 0.0;
  while (r > 0) {                // r -> r - 1 drops |d| = r and, unless it is the same distance, |d| = n - r
    double more = mag(r);
    if (n - r != r) more += mag(n - r);
    if (!(dropped + more <= allowed)) break;
    dropped += more;
    --r;
  }
  *radius = r;
  return true;
}

extern "C" {

int dcp_fourier_gauss_2d(const void* src, void* dst, int height, int width, long src_row_stride, int dtype, int pad, int pad_mode,
                         const double* taps_y_re, const double* taps_y_im, const double* taps_x_re, const double* taps_x_im, int mem_kind, int device,
                         void* stream) {
  PlaneCall c;
  int rc;
  if ((rc = make_plane_call(&c, src, dst, height, width, src_row_stride, dtype, sizeof(double), kSideLimit, kReadsNeighbourhood, mem_kind, device, stream)) !=
      DCP_OK)
    return rc;
  if (!taps_y_re || !taps_y_im || !taps_x_re || !taps_x_im) return fail(DCP_ERR_INVALID_ARG, "null tap table (taps_y_re, taps_y_im, taps_x_re, taps_x_im)");
  if (pad < 0) return fail(DCP_ERR_INVALID_ARG, "pad must be at least 0 (got %d)", pad);
  if (pad_mode != DCP_MODE_REFLECT && pad_mode != DCP_MODE_MIRROR && pad_mode != DCP_MODE_NEAREST && pad_mode != DCP_MODE_WRAP && pad_mode != DCP_MODE_CONSTANT)
    return fail(DCP_ERR_INVALID_ARG, "unknown pad mode %d", pad_mode);
  const int64_t ny = (int64_t)height + 2 * (int64_t)pad, nx = (int64_t)width + 2 * (int64_t)pad;
  if (ny > dcp::kFourierMaxSide || nx > dcp::kFourierMaxSide)
    return fail(DCP_ERR_UNSUPPORTED, "padded side above %d (got %lld x %lld)", dcp::kFourierMaxSide, (long long)ny, (long long)nx);
  int ry, rx;
  if (!support_radius(taps_y_re, taps_y_im, (int)ny, &ry)) return fail(DCP_ERR_INVALID_ARG, "taps_y hold a value that is not finite");
  if (!support_radius(taps_x_re, taps_x_im, (int)nx, &rx)) return fail(DCP_ERR_INVALID_ARG, "taps_x hold a value that is not finite");
  const double* const taps[4] = {taps_y_re, taps_y_im, taps_x_re, taps_x_im};
  return run_plane(c, false, dcp::fourier_work_bytes(height, width, pad), [&](const void* s, void* d, int64_t rs, void* work) {
    return dcp::launch_fourier(s, static_cast<double*>(d), work, height, width, rs, dtype, pad, pad_mode, taps, ry, rx, c.stream);
  });
}

}  // extern "C"
