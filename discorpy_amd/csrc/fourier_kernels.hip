// fourier_kernels.hip -- the Fourier Gaussian filter behind discorpy.prep.preprocessing._apply_fft_filter / normalization_fft (:76-158)
// without an FFT: on the image padded by `pad` on every side (sides Ny x Nx) the reference's
//     real(ifft2(fft2(m s) win) s),   s = (-1)^(x + y),   win a Gaussian centred on ((Ny - 1) / 2, (Nx - 1) / 2),
// is real(A_y m A_x^T) with one complex Toeplitz matrix per axis, A[j, k] = a(j - k) ("Fourier Gaussian filter").
//
//   tables         per axis 2 N - 1 complex taps as two float64 arrays, index d + N - 1 holding a(d), d = -(N - 1) .. N - 1, computed on the
//                  host; on the device each array is followed by kFourierRows - 1 zeros, so that a block of kFourierRows outputs may
//                  read its taps as one contiguous run whatever the block's last outputs are.
//   support        only taps with |d| <= R or |d| >= N - R enter the sums (R per axis, from the host: what is dropped is below 2^-56
//                  of the table's absolute sum); a block of outputs o0 .. o0 + 7 walks the cyclic index window [o0 - R, o0 + 7 + R] of
//                  the summed axis as at most two runs of indices, or all N indices once the window is that long.
//   fourier_rows_kernel<T>   pass 1, along axis 0: P[j, x] = sum_k a_y(j - k) m[k, x] for the cropped rows j and EVERY padded column x,
//                  m read from the source through the pad's index fold (gauss_fold of dcp_device.h; no padded plane) and converted to double.  One thread per
//                  column x (a wave reads 64 consecutive elements of a source row), kFourierRows output rows in registers: per group
//                  of 8 indices k eight elements of m, the 2 x 15 taps a wave-uniform run (scalar loads; the window of a row moves by
//                  one tap per k, so 15 taps serve 64 products), 128 fused multiply-adds.  P is written TRANSPOSED,
//                  p[x * H + j], 64 bytes per thread, so that
//   fourier_cols_kernel      pass 2, along axis 1: bck[j, i] = sum_x a_x,re(i - x) P_re[j, x] - a_x,im(i - x) P_im[j, x], is the same
//                  loop with one thread per row j (a wave reads 64 consecutive elements of p) and kFourierRows output columns in
//                  registers; it writes the result row-major, 64 bytes per thread.
// All arithmetic is float64; the file is compiled with -ffp-contract=off like every other one, the multiply-adds are explicit.
#include "dcp_device.h"

#include <cstdio>

namespace dcp {

constexpr int kFourierBlock = 256;     // threads per workgroup: 256 columns (pass 1) / rows (pass 2)
constexpr int kFourierSteps = 8;       // indices of the summed axis per group: their taps are one run of kFourierSteps + kFourierRows - 1

// The indices of the summed axis (length N) that the outputs o0 .. o0 + kFourierRows - 1 (padded coordinates) need at radius R: the
// cyclic window [o0 - R, o0 + kFourierRows - 1 + R] as the runs [a0, b0] and [a1, b1] (the second one may be empty: a1 > b1).
struct FourierRuns {
  int a0, b0, a1, b1;
};
__device__ __forceinline__ FourierRuns fourier_runs(int o0, int R, int N) {
  const int lo = o0 - R, hi = o0 + kFourierRows - 1 + R;
  FourierRuns r = {lo, hi, 0, -1};
  if (hi - lo + 1 >= N) {
    r.a0 = 0;
    r.b0 = N - 1;
  } else if (lo < 0) {             // the window wraps below 0: [0, hi] and [lo + N, N - 1]
    r.a0 = 0;
    r.a1 = lo + N;
    r.b1 = N - 1;
  } else if (hi > N - 1) {         // it wraps above N - 1: [0, hi - N] and [lo, N - 1]
    r.a0 = 0;
    r.b0 = hi - N;
    r.a1 = lo;
    r.b1 = N - 1;
  }
  return r;
}

template <typename T>
__global__ void __launch_bounds__(kFourierBlock) fourier_rows_kernel(const T* __restrict__ src, int64_t src_stride, int H, int W, int pad, int mode, int N,
                                                                     int NX, int R, const double* __restrict__ t_re, const double* __restrict__ t_im,
                                                                     double* __restrict__ p_re, double* __restrict__ p_im) {
  const int x = (int)blockIdx.x * kFourierBlock + (int)threadIdx.x;
  if (x >= NX) return;
  const int jb = (int)blockIdx.y * kFourierRows;        // first row of the block in the cropped plane
  const int j0 = pad + jb;                              // and in the padded one
  const int sx = gauss_fold(x - pad, W, mode);
  DCP_BOUNDS(sx < 0 ? 0 : sx, 1, W, 50);
  double acc_re[kFourierRows], acc_im[kFourierRows];
#pragma unroll
  for (int b = 0; b < kFourierRows; ++b) acc_re[b] = acc_im[b] = 0.0;
  const FourierRuns runs = fourier_runs(j0, R, N);
  [[maybe_unused]] const uint32_t table = (uint32_t)(2 * N - 1 + kFourierRows - 1);      // (the checking build: entries of a device table)
  auto fetch = [&](int k) -> T {                         // m[k, x] as the source holds it; 0 outside under the constant mode
    const int sy = gauss_fold(k - pad, H, mode);       // the same in every lane
    if (sy < 0 || sx < 0) return (T)0;
    DCP_BOUNDS(sy, 1, H, 50);
    return src[(int64_t)sy * src_stride + sx];
  };
  auto run = [&](int ka, int kb) {
    int k = ka;
    // kFourierSteps steps at a time: their elements are loaded together, and the taps of step s and row b, a(j0 + b - k - s), are
    // entry low + (kFourierSteps - 1 - s) + b of ONE run of kFourierSteps + kFourierRows - 1 entries (the window of a row moves by one
    // tap per step), so a tap is loaded once per group, not once per step
    for (; k + kFourierSteps - 1 <= kb; k += kFourierSteps) {
      int sy[kFourierSteps];                             // the folds first (scalar work), then the loads back to back, then the arithmetic
#pragma unroll
      for (int s = 0; s < kFourierSteps; ++s) {
        sy[s] = gauss_fold(k + s - pad, H, mode);
        DCP_BOUNDS(sy[s] < 0 ? 0 : sy[s], 1, H, 50);
      }
      T v[kFourierSteps];
#pragma unroll
      for (int s = 0; s < kFourierSteps; ++s) v[s] = src[(int64_t)(sy[s] < 0 ? 0 : sy[s]) * src_stride + (sx < 0 ? 0 : sx)];
      const int low = j0 - (k + kFourierSteps - 1) + N - 1;
      DCP_BOUNDS(low, kFourierSteps + kFourierRows - 1, table, 50);
      double tr[kFourierSteps + kFourierRows - 1], ti[kFourierSteps + kFourierRows - 1];
#pragma unroll
      for (int i = 0; i < kFourierSteps + kFourierRows - 1; ++i) {
        tr[i] = t_re[low + i];
        ti[i] = t_im[low + i];
      }
#pragma unroll
      for (int s = 0; s < kFourierSteps; ++s) {
        const double m = (sy[s] < 0 || sx < 0) ? 0.0 : (double)v[s];
#pragma unroll
        for (int b = 0; b < kFourierRows; ++b) {
          acc_re[b] = __builtin_fma(tr[kFourierSteps - 1 - s + b], m, acc_re[b]);
          acc_im[b] = __builtin_fma(ti[kFourierSteps - 1 - s + b], m, acc_im[b]);
        }
      }
    }
    for (; k <= kb; ++k) {                               // the steps left over, one at a time
      const double m = (double)fetch(k);
      const int base = j0 - k + N - 1;                   // a(j0 + b - k) is entry base + b
      DCP_BOUNDS(base, kFourierRows, table, 50);
#pragma unroll
      for (int b = 0; b < kFourierRows; ++b) {
        acc_re[b] = __builtin_fma(t_re[base + b], m, acc_re[b]);
        acc_im[b] = __builtin_fma(t_im[base + b], m, acc_im[b]);
      }
    }
  };
  run(runs.a0, runs.b0);
  run(runs.a1, runs.b1);
  double* out_re = p_re + (int64_t)x * H + jb;
  double* out_im = p_im + (int64_t)x * H + jb;
#pragma unroll
  for (int b = 0; b < kFourierRows; ++b) {
    if (jb + b < H) {
      out_re[b] = acc_re[b];
      out_im[b] = acc_im[b];
    }
  }
}

__global__ void __launch_bounds__(kFourierBlock) fourier_cols_kernel(const double* __restrict__ p_re, const double* __restrict__ p_im, int H, int W, int pad, int N,
                                                                     int R, const double* __restrict__ t_re, const double* __restrict__ t_im,
                                                                     double* __restrict__ dst) {
  const int j = (int)blockIdx.x * kFourierBlock + (int)threadIdx.x;
  if (j >= H) return;
  const int ib = (int)blockIdx.y * kFourierRows;        // first column of the block in the cropped plane
  const int i0 = pad + ib;                              // and in the padded one
  double acc[kFourierRows];
#pragma unroll
  for (int b = 0; b < kFourierRows; ++b) acc[b] = 0.0;
  const FourierRuns runs = fourier_runs(i0, R, N);
  [[maybe_unused]] const uint32_t table = (uint32_t)(2 * N - 1 + kFourierRows - 1);      // (the checking build: entries of a device table)
  auto run = [&](int xa, int xb) {
    if (xa > xb) return;
    DCP_BOUNDS(xa, xb - xa + 1, N, 51);
    int x = xa;
    for (; x + kFourierSteps - 1 <= xb; x += kFourierSteps) {      // groups of steps, as in pass 1
      double vr[kFourierSteps], vi[kFourierSteps];
#pragma unroll
      for (int s = 0; s < kFourierSteps; ++s) {
        vr[s] = p_re[(int64_t)(x + s) * H + j];
        vi[s] = p_im[(int64_t)(x + s) * H + j];
      }
      const int low = i0 - (x + kFourierSteps - 1) + N - 1;
      DCP_BOUNDS(low, kFourierSteps + kFourierRows - 1, table, 51);
      double tr[kFourierSteps + kFourierRows - 1], ti[kFourierSteps + kFourierRows - 1];
#pragma unroll
      for (int i = 0; i < kFourierSteps + kFourierRows - 1; ++i) {
        tr[i] = t_re[low + i];
        ti[i] = t_im[low + i];
      }
#pragma unroll
      for (int s = 0; s < kFourierSteps; ++s) {
#pragma unroll
        for (int b = 0; b < kFourierRows; ++b)
          acc[b] = __builtin_fma(-ti[kFourierSteps - 1 - s + b], vi[s], __builtin_fma(tr[kFourierSteps - 1 - s + b], vr[s], acc[b]));
      }
    }
    for (; x <= xb; ++x) {                               // the steps left over, one at a time
      const double pr = p_re[(int64_t)x * H + j], pi = p_im[(int64_t)x * H + j];
      const int base = i0 - x + N - 1;                   // a(i0 + b - x) is entry base + b
      DCP_BOUNDS(base, kFourierRows, table, 51);
#pragma unroll
      for (int b = 0; b < kFourierRows; ++b) acc[b] = __builtin_fma(-t_im[base + b], pi, __builtin_fma(t_re[base + b], pr, acc[b]));
    }
  };
  run(runs.a0, runs.b0);
  run(runs.a1, runs.b1);
  double* out = dst + (int64_t)j * W + ib;
#pragma unroll
  for (int b = 0; b < kFourierRows; ++b)
    if (ib + b < W) out[b] = acc[b];
}

DCP_DEFINE_BOUNDS_READER(read_bounds_fourier)

// ------------------------------------------------------------------ launcher

size_t fourier_work_bytes(int H, int W, int pad) {
  const size_t ny = (size_t)H + 2 * (size_t)pad, nx = (size_t)W + 2 * (size_t)pad;
  return (2 * (size_t)H * nx + 2 * (2 * ny - 1 + kFourierRows - 1) + 2 * (2 * nx - 1 + kFourierRows - 1)) * sizeof(double);
}

template <typename T>
static void launch_fourier_rows(const void* src, int64_t src_stride, int H, int W, int pad, int mode, int ny, int nx, int ry, const double* ty_re,
                                const double* ty_im, double* p_re, double* p_im, hipStream_t stream) {
  const dim3 grid((unsigned)((nx + kFourierBlock - 1) / kFourierBlock), (unsigned)((H + kFourierRows - 1) / kFourierRows));
  hipLaunchKernelGGL((fourier_rows_kernel<T>), grid, dim3(kFourierBlock), 0, stream, static_cast<const T*>(src), src_stride, H, W, pad, mode, ny, nx, ry,
                     ty_re, ty_im, p_re, p_im);
}

hipError_t launch_fourier(const void* src, double* dst, void* work, int H, int W, int64_t src_stride, int dtype, int pad, int boundary,
                          const double* const taps[4], int ry, int rx, hipStream_t stream) {
  if (H < 1 || W < 1 || pad < 0 || !work || !taps[0] || !taps[1] || !taps[2] || !taps[3]) return hipErrorInvalidValue;
  const int64_t ny64 = (int64_t)H + 2 * (int64_t)pad, nx64 = (int64_t)W + 2 * (int64_t)pad;
  if (ny64 > kFourierMaxSide || nx64 > kFourierMaxSide || ry < 0 || rx < 0) return hipErrorInvalidValue;
  const int ny = (int)ny64, nx = (int)nx64;
  int mode;
  switch (boundary) {
    case kModeReflect: mode = kGaussReflect; break;       // np.pad's "symmetric": period 2 n
    case kModeMirror: mode = kGaussMirror; break;         // "reflect": period 2 n - 2
    case kModeNearest: mode = kGaussNearest; break;       // "edge"
    case kModeWrap: mode = kGaussWrap; break;             // "wrap"
    case kModeConstant: mode = kGaussConstant; break;     // "constant": gauss_fold says -1, the element is 0
    default: return hipErrorInvalidValue;
  }
  // the workspace: the two planes of pass 1, then the four tables, each followed by kFourierRows - 1 zeros
  double* p_re = static_cast<double*>(work);
  double* p_im = p_re + (size_t)H * (size_t)nx;
  const size_t len_y = 2 * (size_t)ny - 1, len_x = 2 * (size_t)nx - 1, tail = kFourierRows - 1;
  double* t[4];
  t[0] = p_im + (size_t)H * (size_t)nx;
  t[1] = t[0] + len_y + tail;
  t[2] = t[1] + len_y + tail;
  t[3] = t[2] + len_x + tail;
  hipError_t e = hipMemsetAsync(t[0], 0, (2 * (len_y + tail) + 2 * (len_x + tail)) * sizeof(double), stream);
  for (int i = 0; i < 4 && e == hipSuccess; ++i)
    e = hipMemcpyAsync(t[i], taps[i], (i < 2 ? len_y : len_x) * sizeof(double), hipMemcpyHostToDevice, stream);
  // the caller's tables are ordinary host memory and may change or go once the call returns: wait until they have been read
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) return e;
#define DCP_FOURIER_CASE(T) launch_fourier_rows<T>(src, src_stride, H, W, pad, mode, ny, nx, ry, t[0], t[1], p_re, p_im, stream); break
  switch (dtype) {
    case kF32: DCP_FOURIER_CASE(float);
    case kF64: DCP_FOURIER_CASE(double);
    case kU8:
    case kBool: DCP_FOURIER_CASE(uint8_t);
    case kI8: DCP_FOURIER_CASE(int8_t);
    case kU16: DCP_FOURIER_CASE(uint16_t);
    case kI16: DCP_FOURIER_CASE(int16_t);
    case kU32: DCP_FOURIER_CASE(uint32_t);
    case kI32: DCP_FOURIER_CASE(int32_t);
    case kI64: DCP_FOURIER_CASE(int64_t);
    case kU64: DCP_FOURIER_CASE(uint64_t);
    default: return hipErrorInvalidValue;
  }
#undef DCP_FOURIER_CASE
  if ((e = hipGetLastError()) != hipSuccess) return e;
  const dim3 grid((unsigned)((H + kFourierBlock - 1) / kFourierBlock), (unsigned)((W + kFourierRows - 1) / kFourierRows));
  hipLaunchKernelGGL(fourier_cols_kernel, grid, dim3(kFourierBlock), 0, stream, p_re, p_im, H, W, pad, nx, rx, t[2], t[3], dst);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  char name[160];
  snprintf(name, sizeof(name), "fourier_rows_kernel<block=%dx%d, taps=%d of %d> + fourier_cols_kernel<taps=%d of %d>", kFourierBlock, kFourierRows,
           2 * ry + 1 >= ny ? 2 * ny - 1 : 4 * ry + 1, 2 * ny - 1, 2 * rx + 1 >= nx ? 2 * nx - 1 : 4 * rx + 1, 2 * nx - 1);
  set_last_kernel_name(name);
  return hipSuccess;
}

}  // namespace dcp
