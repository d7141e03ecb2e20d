// select_peaks_kernels.hip -- select_good_peaks of the line-pattern route (discorpy.prep.linepattern:75-152) on a batch of candidate peaks:
//   select_peaks_kernel     one wave per candidate: its window, the normalisation, the least-squares fit of
//                           a exp(-((x - c) / (2 b^2))^2) + d from (1, 1, 0, 0), the 80th percentile of |fit - y| and the decision
// The fit is the Levenberg-Marquardt iteration of MINPACK's lmdif as scipy's curve_fit runs it for the reference ("Peak
// selection"): Jacobian by forward differences, columns scaled by the running maximum of their norms, a trust region on the scaled
// step, the tolerances 1.49012e-8 and the budget of 200 (4 + 1) evaluations -- on the normal equations J^T J, J^T r, whose fourteen sums
// and the cost are reduced across the wave in a fixed order.  Everything is float64.  Built with -ffp-contract=off.  The device code
// is fit_window of select_peaks_device.h, which extrema_select_kernels.hip calls too.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include "dcp_device.h"
#include "select_peaks_device.h"

namespace dcp {

// One wave per candidate (fit_window of select_peaks_device.h), four candidates per workgroup.
template <typename T>
__global__ void __launch_bounds__(kFitBlock) select_peaks_kernel(const T* __restrict__ src, int64_t src_stride, int L, const int32_t* __restrict__ peak_row,
                                                                 const int32_t* __restrict__ peak_idx, int npeaks, int radius, double tol, int use_offset,
                                                                 unsigned char* __restrict__ keep, double* __restrict__ fit) {
  __shared__ double s_y[kFitWaves][kFitMaxWindow];
  __shared__ double s_pick[kFitWaves][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int peak = blockIdx.x * kFitWaves + wave;
  const bool active = peak < npeaks;                  // (the same in every lane of a wave)
  int n = 0;
  const T* __restrict__ row = src;
  if (active) {
    const int p = peak_idx[peak];
    const int start = max(0, p - radius), stop = min(L, p + radius + 1);
    n = stop - start;                                 // at most 2 radius + 1 <= kFitMaxWindow
    row = src + (int64_t)peak_row[peak] * src_stride + start;
  }
  const FitResult r = fit_window(active, n, radius, tol, use_offset, s_y[wave], s_pick[wave], lane, [&](int i) { return (double)row[i]; });
  if (active && lane == 0) {
    keep[peak] = r.good ? 1 : 0;
    if (fit) {
      double* __restrict__ o = fit + (int64_t)peak * 6;
      o[0] = r.x[0], o[1] = r.x[1], o[2] = r.x[2], o[3] = r.x[3], o[4] = r.num, o[5] = (double)r.status;
    }
  }
}

DCP_DEFINE_BOUNDS_READER(read_bounds_select)

// ------------------------------------------------------------------ launcher

hipError_t launch_select_peaks(const void* src, int N, int L, int64_t src_stride, int dtype, const int32_t* peak_row, const int32_t* peak_idx, int npeaks,
                               int radius, double tol, bool use_offset, unsigned char* keep, double* fit, void* work, hipStream_t stream) {
  if (N < 1 || L < 1 || src_stride < L || npeaks < 1 || radius < 1 || radius > kSelectMaxRadius || !peak_row || !peak_idx || !keep || !work ||
      (dtype != kF32 && dtype != kF64))
    return hipErrorInvalidValue;
  int32_t* const rows_dev = static_cast<int32_t*>(work);
  int32_t* const idx_dev = rows_dev + npeaks;
  hipError_t e = hipMemcpyAsync(rows_dev, peak_row, (size_t)npeaks * sizeof(int32_t), hipMemcpyHostToDevice, stream);
  if (e == hipSuccess) e = hipMemcpyAsync(idx_dev, peak_idx, (size_t)npeaks * sizeof(int32_t), hipMemcpyHostToDevice, stream);
  // the tables are ordinary host memory of the caller: wait until they have been read
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) return e;
  const dim3 grid((unsigned)((npeaks + kFitWaves - 1) / kFitWaves));
  if (dtype == kF32)
    hipLaunchKernelGGL((select_peaks_kernel<float>), grid, dim3(kFitBlock), 0, stream, static_cast<const float*>(src), src_stride, L, rows_dev, idx_dev,
                       npeaks, radius, tol, use_offset ? 1 : 0, keep, fit);
  else
    hipLaunchKernelGGL((select_peaks_kernel<double>), grid, dim3(kFitBlock), 0, stream, static_cast<const double*>(src), src_stride, L, rows_dev, idx_dev,
                       npeaks, radius, tol, use_offset ? 1 : 0, keep, fit);
  char name[96];
  snprintf(name, sizeof(name), "select_peaks_kernel<%s, radius=%d, peaks=%d>", dtype == kF32 ? "float" : "double", radius, npeaks);
  set_last_kernel_name(name);
  return hipGetLastError();
}

}  // namespace dcp
