// radon_kernels.hip -- the Radon transform of a square plane for a table of angles (discorpy.prep.linepattern: the sinograms of
// calc_slope_distance_hor_lines / calc_slope_distance_ver_lines), one launch for all angles:
//   radon_kernel            sinogram[c, i] = sum over r of the bilinear sample (r, c) of the plane rotated by angle i
// Built with -ffp-contract=off: every expression below is the sequence of IEEE operations DESIGN.md ("Radon transform") names, so the
// result equals the NumPy restatement of that definition (tests/helpers/radon_reference.py) bit for bit.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include "dcp_device.h"

namespace dcp {

constexpr int kRadonBlock = 64;                       // one wave: 64 neighbouring columns of one angle
constexpr int kRadonBatch = 4;                        // rows whose taps are in flight together; they are still added one by one

// One tap g(y, x): where it lies in the plane (`at`) and whether it counts.  g is the element widened to float64, 0.0 outside the plane and
// outside the inscribed circle (an assignment: what lies there, a NaN included, never reaches the result).  yf / xf are floor / ceil
// results; the comparisons in double keep the conversion to int in range.  No branch: a tap outside reads element (0, 0) instead and
// drops it.
struct RadonTap {
  int64_t at;
  bool keep;
};

__device__ __forceinline__ RadonTap radon_tap(int64_t stride, int N, int c0, int rad2, double yf, double xf) {
  const bool in_plane = (yf >= 0.0) & (yf < (double)N) & (xf >= 0.0) & (xf < (double)N);     // (&: no short-circuit, no branch)
  const int yi = in_plane ? (int)yf : 0, xi = in_plane ? (int)xf : 0;      // 0 <= yi, xi < N either way
  const int ey = yi - c0, ex = xi - c0;
  RadonTap t;
  t.at = (int64_t)yi * stride + xi;
  t.keep = in_plane & (ey * ey + ex * ex <= rad2);                         // (|ey|, |ex| <= 2^14: the squares stay far inside int32)
  return t;
}

// The sample (r, c) of one angle in three steps, so that a batch of rows can issue all its loads before it needs any of them:
// where its four taps lie and their weights (xc = ca * c and yc = -sa * c are the thread's own products, the rest is the definition's
// left-to-right order), the loads, the blend.
struct RadonSample {
  RadonTap t00, t01, t10, t11;
  double dx, dy;
};

__device__ __forceinline__ RadonSample radon_locate(int64_t stride, int N, int c0, int rad2, double ca, double sa, double tx, double ty,
                                                    double xc, double yc, int r) {
  const double x = xc + sa * (double)r + tx;
  const double y = yc + ca * (double)r + ty;
  const double x0 = floor(x), x1 = ceil(x), y0 = floor(y), y1 = ceil(y);
  RadonSample s;
  s.dx = x - x0;
  s.dy = y - y0;
  s.t00 = radon_tap(stride, N, c0, rad2, y0, x0);
  s.t01 = radon_tap(stride, N, c0, rad2, y0, x1);
  s.t10 = radon_tap(stride, N, c0, rad2, y1, x0);
  s.t11 = radon_tap(stride, N, c0, rad2, y1, x1);
  return s;
}

template <typename T>
__device__ __forceinline__ double radon_blend(const RadonSample& s, T e00, T e01, T e10, T e11) {
  const double g00 = s.t00.keep ? (double)e00 : 0.0, g01 = s.t01.keep ? (double)e01 : 0.0;
  const double g10 = s.t10.keep ? (double)e10 : 0.0, g11 = s.t11.keep ? (double)e11 : 0.0;
  const double top = (1.0 - s.dx) * g00 + s.dx * g01;
  const double bot = (1.0 - s.dx) * g10 + s.dx * g11;
  return (1.0 - s.dy) * top + s.dy * bot;
}

// `B` consecutive rows from r on: v[j] = the sample (r + j, c)
template <int B, typename T>
__device__ __forceinline__ void radon_rows(const T* __restrict__ src, int64_t stride, int N, int c0, int rad2, double ca, double sa, double tx,
                                           double ty, double xc, double yc, int r, double* v) {
  RadonSample s[B];
  T e[B][4];
#pragma unroll
  for (int j = 0; j < B; ++j) s[j] = radon_locate(stride, N, c0, rad2, ca, sa, tx, ty, xc, yc, r + j);
#pragma unroll
  for (int j = 0; j < B; ++j) {
    e[j][0] = src[s[j].t00.at];
    e[j][1] = src[s[j].t01.at];
    e[j][2] = src[s[j].t10.at];
    e[j][3] = src[s[j].t11.at];
  }
#pragma unroll
  for (int j = 0; j < B; ++j) v[j] = radon_blend(s[j], e[j][0], e[j][1], e[j][2], e[j][3]);
}

// One thread per (angle, column): blockIdx.y is the angle, lanes run along the columns, and the thread walks its rows 0 .. N - 1 and
// adds them in that order (no atomics, no tree: the order is the definition's).  table: {ca, sa, tx, ty} per angle.  out: (N, A).
template <typename T>
__global__ void __launch_bounds__(kRadonBlock) radon_kernel(const T* __restrict__ src, int64_t stride, int N, int A,
                                                            const double* __restrict__ table, double* __restrict__ out) {
  const int c = blockIdx.x * kRadonBlock + threadIdx.x, a = blockIdx.y;
  if (c >= N || a >= A) return;
  const double ca = table[4 * a], sa = table[4 * a + 1], tx = table[4 * a + 2], ty = table[4 * a + 3];
  const int c0 = N / 2, rad2 = c0 * c0;
  const double xc = ca * (double)c, yc = -sa * (double)c;
  double acc, v[kRadonBatch];
  radon_rows<1>(src, stride, N, c0, rad2, ca, sa, tx, ty, xc, yc, 0, &acc);
  int r = 1;
  for (; r + kRadonBatch <= N; r += kRadonBatch) {
    radon_rows<kRadonBatch>(src, stride, N, c0, rad2, ca, sa, tx, ty, xc, yc, r, v);
#pragma unroll
    for (int j = 0; j < kRadonBatch; ++j) acc += v[j];
  }
  for (; r < N; ++r) {
    radon_rows<1>(src, stride, N, c0, rad2, ca, sa, tx, ty, xc, yc, r, v);
    acc += v[0];
  }
  out[(int64_t)c * A + a] = acc;
}

hipError_t launch_radon(const void* src, double* dst, int N, int64_t src_stride, int dtype, int nangles, const double* table, void* work,
                        hipStream_t stream) {
  if (N < 1 || N > kRadonMaxSide || nangles < 1 || nangles > kRadonMaxAngles || src_stride < N || !table || !work || (dtype != kF32 && dtype != kF64))
    return hipErrorInvalidValue;
  hipError_t e = hipMemcpyAsync(work, table, radon_work_bytes(nangles), hipMemcpyHostToDevice, stream);
  // the table is ordinary host memory of the caller: wait until it has been read
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) return e;
  const dim3 grid((unsigned)((N + kRadonBlock - 1) / kRadonBlock), (unsigned)nangles);
  if (dtype == kF32)
    hipLaunchKernelGGL((radon_kernel<float>), grid, dim3(kRadonBlock), 0, stream, static_cast<const float*>(src), src_stride, N, nangles,
                       static_cast<const double*>(work), dst);
  else
    hipLaunchKernelGGL((radon_kernel<double>), grid, dim3(kRadonBlock), 0, stream, static_cast<const double*>(src), src_stride, N, nangles,
                       static_cast<const double*>(work), dst);
  char name[96];
  snprintf(name, sizeof(name), "radon_kernel<%s, angles=%d>", dtype == kF32 ? "float" : "double", nangles);
  set_last_kernel_name(name);
  return hipGetLastError();
}

}  // namespace dcp
