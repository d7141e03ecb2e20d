// spline_device.h -- the arithmetic every user of the spline orders shares (spline_kernels.hip, spline_color_kernels.hip,
// spline_frames_kernels.hip, profile_kernels.hip): the B-spline weights, the folding of a tap index under a boundary mode, the
// LDS-only barrier, and the geometry of the LDS-staged gather.  What only the three gather files share -- box, fill, row table,
// launchers -- is in spline_gather.h, which needs dcp_device.h.
#pragma once
#include "dcp_internal.h"

namespace dcp {

constexpr int kSplBlock = 256;

// x / D, correctly rounded, for the constants of the weight polynomials: q = x * RN(1/D), one exact residual, one
// correction (Markstein) -- three instructions where the compiler's IEEE division takes about twenty, and the weights
// need up to eight divisions per pixel.  |x| is O(1) here: nothing leaves the normal range.
template <int D>
__device__ __forceinline__ double div_c(double x) {
  constexpr double r = 1.0 / (double)D;
  const double q = x * r;
  const double e = __builtin_fma(-(double)D, q, x);
  return __builtin_fma(e, r, q);
}

// centred B-spline weights (the expressions of spline_weights() in the oracle); returns the first tap
// FAST (the factorised gather only, where the sum is not scipy's to the last bit anyway): the cubic weights as fused polynomials,
// y^2 (y / 2 - 1) + 2 / 3 and z^3 / 6 -- 15 operations per axis instead of 27; each weight within one float64 ulp of scipy's form.
template <int ORDER, bool FAST = false>
__device__ __forceinline__ int spline_weights(double x, double* w) {
  double s;
  if constexpr (ORDER & 1) s = __builtin_floor(x);
  else s = __builtin_floor(x + 0.5);
  const double t = x - s;
  const int start = (int)s - ORDER / 2;
  double y = t, z = 1.0 - t, t2;
  if constexpr (ORDER == 3 && FAST) {
    w[1] = __builtin_fma(y * y, __builtin_fma(y, 0.5, -1.0), 2.0 / 3.0);
    w[2] = __builtin_fma(z * z, __builtin_fma(z, 0.5, -1.0), 2.0 / 3.0);
    w[0] = (z * z) * (z * (1.0 / 6.0));
    w[3] = 1.0 - w[0] - w[1] - w[2];
  } else if constexpr (ORDER == 4 && FAST) {
    // (round 6) the quartic and quintic weights as fused Horner chains in the same variables as scipy's expressions: 21 / 29 operations
    // per axis instead of 37 / 53, every weight within a few float64 ulps of scipy's form (the constants 1/6, 1/24, 1/120 rounded once)
    t2 = t * t;
    w[2] = __builtin_fma(t2, __builtin_fma(t2, 0.25, -0.625), 115.0 / 192.0);
    y = 1.0 + t;
    z = 1.0 - t;
    w[1] = __builtin_fma(y, __builtin_fma(y, __builtin_fma(y, __builtin_fma(y, -1.0 / 6.0, 5.0 / 6.0), -1.25), 5.0 / 24.0), 55.0 / 96.0);
    w[3] = __builtin_fma(z, __builtin_fma(z, __builtin_fma(z, __builtin_fma(z, -1.0 / 6.0, 5.0 / 6.0), -1.25), 5.0 / 24.0), 55.0 / 96.0);
    y = 0.5 - t;
    y *= y;
    w[0] = (y * y) * (1.0 / 24.0);
    w[4] = 1.0 - w[0] - w[1] - w[2] - w[3];
  } else if constexpr (ORDER == 5 && FAST) {
    t2 = y * y;
    w[2] = __builtin_fma(t2, __builtin_fma(t2, __builtin_fma(y, -1.0 / 12.0, 0.25), -0.5), 0.55);
    t2 = z * z;
    w[3] = __builtin_fma(t2, __builtin_fma(t2, __builtin_fma(z, -1.0 / 12.0, 0.25), -0.5), 0.55);
    w[0] = (t2 * t2) * (z * (1.0 / 120.0));
    y += 1.0;
    w[1] = __builtin_fma(y, __builtin_fma(y, __builtin_fma(y, __builtin_fma(y, __builtin_fma(y, 1.0 / 24.0, -0.375), 1.25), -1.75), 0.625), 0.425);
    y = z + 1.0;
    w[4] = __builtin_fma(y, __builtin_fma(y, __builtin_fma(y, __builtin_fma(y, __builtin_fma(y, 1.0 / 24.0, -0.375), 1.25), -1.75), 0.625), 0.425);
    w[5] = 1.0 - w[0] - w[1] - w[2] - w[3] - w[4];
  } else if constexpr (ORDER == 2) {
    w[1] = 0.75 - t * t;
    y = 0.5 + t;
    w[2] = 0.5 * y * y;
    w[0] = 1.0 - w[1] - w[2];
  } else if constexpr (ORDER == 3) {
    w[1] = div_c<6>(y * y * (y - 2.0) * 3.0 + 4.0);
    w[2] = div_c<6>(z * z * (z - 2.0) * 3.0 + 4.0);
    w[0] = div_c<6>(z * z * z);
    w[3] = 1.0 - w[0] - w[1] - w[2];
  } else if constexpr (ORDER == 4) {
    t2 = t * t;
    w[2] = t2 * (t2 * 0.25 - 0.625) + 115.0 / 192.0;
    y = 1.0 + t;
    z = 1.0 - t;
    w[1] = y * (y * (div_c<6>(y * (5.0 - y)) - 1.25) + 5.0 / 24.0) + 55.0 / 96.0;
    w[3] = z * (z * (div_c<6>(z * (5.0 - z)) - 1.25) + 5.0 / 24.0) + 55.0 / 96.0;
    y = 0.5 - t;
    y *= y;
    w[0] = div_c<24>(y * y);
    w[4] = 1.0 - w[0] - w[1] - w[2] - w[3];
  } else {
    t2 = y * y;
    w[2] = t2 * (t2 * (0.25 - div_c<12>(y)) - 0.5) + 0.55;
    t2 = z * z;
    w[3] = t2 * (t2 * (0.25 - div_c<12>(z)) - 0.5) + 0.55;
    y += 1.0;
    w[1] = y * (y * (y * (y * (div_c<24>(y) - 0.375) + 1.25) - 1.75) + 0.625) + 0.425;
    y = z + 1.0;
    w[4] = y * (y * (y * (y * (div_c<24>(y) - 0.375) + 1.25) - 1.75) + 0.625) + 0.425;
    t2 = z * z;
    w[0] = div_c<120>(t2 * t2 * z);
    w[5] = 1.0 - w[0] - w[1] - w[2] - w[3] - w[4];
  }
  return start;
}

__device__ __forceinline__ int spline_fold(int i, int n, int mode) {
  if (i >= 0 && i < n) return i;
  if (mode == kModeReflect || mode == kModeGridMirror) {
    const int s2 = 2 * n;
    i %= s2;
    if (i < 0) i += s2;
    return i < n ? i : s2 - 1 - i;
  }
  if (mode == kModeGridWrap) {
    i %= n;
    return i < 0 ? i + n : i;
  }
  if (mode == kModeNearest || mode == kModeGridConstant) return i < 0 ? 0 : n - 1;
  if (n == 1) return 0;
  const int s2 = 2 * n - 2;
  i %= s2;
  if (i < 0) i += s2;
  return i < n ? i : s2 - i;
}

// Workgroup barrier that orders LDS traffic only: the wave's LDS reads and writes are retired, then the workgroup meets -- what was
// written may be read, what was read may be overwritten.  (__syncthreads() also drains the wave's global memory operations; a fill of
// LDS by LDS-DMA is such an operation and needs its own vmcnt wait.)
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

constexpr int kSwTW = 128, kSwTH = 32;             // workgroup tile
constexpr int kSwBoxW = 144, kSwBoxH = 45;         // slab: 144 x 45 float64 = 51 840 B; with the row tables three workgroups per CU
constexpr int kSwCH = kSwBoxW * 8 / 16;            // 16-byte chunks per slab row
constexpr int kSwNJ = (kSwBoxH * kSwCH + 255) / 256;   // loads per wave that cover the slab: 13

}  // namespace dcp
