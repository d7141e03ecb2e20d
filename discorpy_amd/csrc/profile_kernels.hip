// profile_kernels.hip -- the per-profile steps of the line-pattern route (discorpy.prep.linepattern: get_local_extrema_points,
// sliding_window_slope, get_tilted_profile) on batches of profiles:
//   peak_rows_kernel        the local minima of every row of an (N, L) plane, with their sub-pixel refinement
//   window_slope_kernel     the absolute slope of the least-squares line through a sliding window of every row
//   band_filter_cols_kernel / band_filter_rows_kernel / band_sample_kernel
//                           N tilted profiles of one image: the cubic prefilter of every profile's own band, then the samples
// Built with -ffp-contract=off: every sum below is the sequence of IEEE operations the comments name.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include "dcp_device.h"
#include "select_peaks_device.h"
#include "spline_device.h"

namespace dcp {

// ------------------------------------------------------------------ (a) peak search

constexpr int kPeakBlock = 256;                       // four waves
constexpr int kPeakWaves = kPeakBlock / 64;
constexpr int kPeakTile = 256;                        // samples per step of a row's workgroup
constexpr int kPeakSlab = kPeakTile + 2 * kPeakMaxRadius;

// np.add.reduce over n <= 128 contiguous elements: NumPy's pairwise_sum below its recursive split
template <typename T>
__device__ __forceinline__ T numpy_block_sum(const T* a, int n) {
  if (n < 8) {
    T res = (T)0;
    for (int i = 0; i < n; ++i) res += a[i];
    return res;
  }
  T r[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = a[j];
  int i = 8;
  for (; i < n - (n % 8); i += 8) {
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] += a[i + j];
  }
  T res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) res += a[i];
  return res;
}

// One workgroup per row; it walks the row in steps of kPeakTile samples.  Per step: the samples and `radius` more on both sides go to
// LDS; every thread takes the minimum of its sample's window (a sample is a candidate iff min - v == 0 and the window holds no NaN);
// the candidates are listed in ascending order; a wave per candidate ranks the window (rank sort: ties by index, as a stable sort) and
// writes its `ntop` largest elements in ascending order, whose NumPy sum / ntop is the mean the sensitivity test divides by; thread 0
// appends the accepted positions to the row's output.  out: (N, L) doubles, row r = its positions, element L - 1 their number.
template <typename T>
__global__ void __launch_bounds__(kPeakBlock) peak_rows_kernel(const T* __restrict__ src, int64_t src_stride, int L, int radius, double sensitive,
                                                               int subpixel, double* __restrict__ out) {
  __shared__ T s_tile[kPeakSlab];
  __shared__ T s_top[kPeakWaves][kPeakMaxRadius];
  __shared__ int s_cand[kPeakTile];
  __shared__ double s_res[kPeakTile];
  __shared__ int s_wave_n[kPeakWaves];
  const T* __restrict__ row = src + (int64_t)blockIdx.x * src_stride;
  double* __restrict__ orow = out + (int64_t)blockIdx.x * L;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lo = radius, hi = L - radius - 1;          // the samples i of range(radius, L - radius - 1)
  const int n = 2 * radius + 1, ntop = radius > 0 ? radius : 1;   // (list_sort[-0:] is the whole window of one element)
  int count = 0;                                       // thread 0: points written so far
  for (int t0 = lo; t0 < hi; t0 += kPeakTile) {
    // s_tile[j] = row[t0 - radius + j]: the windows of samples t0 .. t0 + kPeakTile - 1 that lie below hi end at hi - 1 + radius <= L - 2
    const int span = min(kPeakTile, hi - t0) + 2 * radius;
    for (int j = tid; j < span; j += kPeakBlock) s_tile[j] = row[t0 - radius + j];
    __syncthreads();
    const int i = t0 + tid;
    bool cand = false;
    if (i < hi) {
      DCP_BOUNDS((uint32_t)tid * sizeof(T), (uint32_t)n * sizeof(T), sizeof(s_tile), 40);
      const T v = s_tile[tid + radius];
      T mn = s_tile[tid];
      bool nan = mn != mn;
      for (int j = 1; j < n; ++j) {
        const T w = s_tile[tid + j];
        nan = nan || w != w;
        mn = w < mn ? w : mn;
      }
      cand = !nan && (mn - v) == (T)0;                 // num1 == 0.0 (an infinite minimum gives inf - inf: no point, as in the reference)
    }
    const unsigned long long mask = __ballot(cand);
    if (lane == 0) s_wave_n[wave] = __popcll(mask);
    __syncthreads();
    int before = 0, ncand = 0;
#pragma unroll
    for (int w = 0; w < kPeakWaves; ++w) {
      before += w < wave ? s_wave_n[w] : 0;
      ncand += s_wave_n[w];
    }
    if (cand) s_cand[before + __popcll(mask & ((1ull << lane) - 1ull))] = tid;
    __syncthreads();
    for (int c0 = 0; c0 < ncand; c0 += kPeakWaves) {   // (ncand is the same in every thread: the barriers below are uniform)
      const int c = c0 + wave;
      const int k = c < ncand ? s_cand[c] : 0;         // the window of sample t0 + k is s_tile[k .. k + n)
      if (c < ncand) {
        for (int e = lane; e < n; e += 64) {
          DCP_BOUNDS((uint32_t)k * sizeof(T), (uint32_t)n * sizeof(T), sizeof(s_tile), 41);
          const T we = s_tile[k + e];
          int rank = 0;
          for (int j = 0; j < n; ++j) {
            const T wj = s_tile[k + j];
            rank += (wj < we || (wj == we && j < e)) ? 1 : 0;
          }
          if (rank >= n - ntop) {
            DCP_BOUNDS((uint32_t)(rank - (n - ntop)) * sizeof(T), sizeof(T), sizeof(s_top[0]), 42);
            s_top[wave][rank - (n - ntop)] = we;
          }
        }
      }
      __syncthreads();
      if (c < ncand && lane == 0) {
        const T v = s_tile[k + radius];
        const T m = numpy_block_sum(s_top[wave], ntop) / (T)ntop;      // np.mean: the sum, then one division, in the row's type
        T num2 = (T)0;
        if (m != (T)0) {
          num2 = (v - m) / m;
          num2 = num2 < (T)0 ? -num2 : num2;
        }
        double pos = -1.0;                             // (positions are never negative)
        if ((double)num2 > sensitive) {
          const int ip = t0 + k;
          pos = (double)ip;
          if (subpixel) {
            // the parabola through the sample and its neighbours, float64: vertex -b / (2 a) where it lies in [0, 3), else the argmin
            // (parabola_position of select_peaks_device.h, which the fused search-and-select call applies to the same three samples)
            pos = parabola_position(ip, (double)s_tile[k + radius - 1], (double)v, (double)s_tile[k + radius + 1]);
          }
        }
        s_res[c] = pos;
      }
      __syncthreads();
    }
    if (tid == 0)
      for (int c = 0; c < ncand; ++c)
        if (s_res[c] >= 0.0) orow[count++] = s_res[c];   // count <= hi - lo <= L - 1: element L - 1 stays free
    __syncthreads();                                   // s_tile, s_cand and s_res are rewritten by the next step
  }
  if (tid == 0) orow[L - 1] = (double)count;
}

// ------------------------------------------------------------------ (b) sliding-window slope

// out[i] = | T( (sum_k (k - r) p[clamp(i + k - r)]) / sum_k (k - r)^2 ) |: the slope of the least-squares line through the `size` = 2 r + 1
// samples around i of the edge-padded row.  The products and the sum (k ascending, from 0.0) are float64, the quotient is rounded
// to the row's type as the reference stores it, then the sign goes.
template <typename T>
__global__ void __launch_bounds__(256) window_slope_kernel(const T* __restrict__ src, int64_t src_stride, int N, int L, int r, double den,
                                                           T* __restrict__ dst) {
  const int i = blockIdx.x * 256 + threadIdx.x, rowi = blockIdx.y;
  if (i >= L || rowi >= N) return;
  const T* __restrict__ row = src + (int64_t)rowi * src_stride;
  double acc = 0.0;
  for (int k = 0; k <= 2 * r; ++k) {
    int j = i + k - r;
    j = j < 0 ? 0 : (j > L - 1 ? L - 1 : j);
    acc += (double)(k - r) * (double)row[j];
  }
  const T s = (T)(acc / den);
  dst[(int64_t)rowi * L + i] = s < (T)0 ? -s : s;
}

// ------------------------------------------------------------------ (c) tilted profiles

// The band of profile p: rows (columns) lo .. lo + n - 1 of the image, and where its coefficients live.  The padded band measures
// (n + 24) x (W + 24) [bands of rows] or (H + 24) x (n + 24) [bands of columns] doubles, row-major, at work + offset.
struct alignas(8) ProfileBand {
  int32_t lo, n;
  int64_t offset;
  double zpow;           // z^(n + 24): the reflect start of the lines across the band
};

static_assert(sizeof(ProfileBand) == 24, "api_profile.cpp sizes the band table by this");

constexpr int kBandPad = 12;                          // scipy edge-pads by 12 under "nearest" and prefilters the padded array
constexpr int kBandBatch = 8;
constexpr int kBandHorizon = 64;                      // terms kept of the start sums (spline_kernels.hip: kHorizon)

// One line of the cubic prefilter in place, scipy's recursion under its "reflect" ends (spline_causal_kernel / spline_anticausal_kernel
// of spline_kernels.hip without their chunking): x(i) -> lam x(i) is read through `ld`, the line's samples are `stride` doubles apart.
template <typename Load>
__device__ __forceinline__ void band_filter_line(double* c, int64_t stride, int n, double z, double z_n, double lam, Load ld) {
  if (n < 2) {
    if (n == 1) c[0] = ld(0);
    return;
  }
  const double x0 = ld(0) * lam;
  double z_i = z;
  double acc = x0 + z_n * (ld(n - 1) * lam);
  const int m = min(n - 1, kBandHorizon);
  for (int k = 1; k <= m; ++k) {
    const double far = n - 1 - k == 0 ? acc : ld(n - 1 - k) * lam;
    acc += z_i * (ld(k) * lam + z_n * far);
    z_i *= z;
  }
  double t = acc * z / (1.0 - z_i * z_i) + x0;
  c[0] = t;
  // kBandBatch loads in flight per thread ahead of the recursion: the lines of a few bands are all the parallelism there is
  int i = 1;
  for (; i + kBandBatch <= n; i += kBandBatch) {
    double v[kBandBatch];
#pragma unroll
    for (int j = 0; j < kBandBatch; ++j) v[j] = ld(i + j);
#pragma unroll
    for (int j = 0; j < kBandBatch; ++j) {
      t = v[j] * lam + z * t;
      c[(int64_t)(i + j) * stride] = t;
    }
  }
  for (; i < n; ++i) {
    t = ld(i) * lam + z * t;
    c[(int64_t)i * stride] = t;
  }
  t = c[(int64_t)(n - 1) * stride] * (z / (z - 1.0));
  c[(int64_t)(n - 1) * stride] = t;
  i = n - 2;
  for (; i - kBandBatch + 1 >= 0; i -= kBandBatch) {
    double v[kBandBatch];
#pragma unroll
    for (int j = 0; j < kBandBatch; ++j) v[j] = c[(int64_t)(i - j) * stride];
#pragma unroll
    for (int j = 0; j < kBandBatch; ++j) {
      t = z * (t - v[j]);
      c[(int64_t)(i - j) * stride] = t;
    }
  }
  for (; i >= 0; --i) {
    t = z * (t - c[(int64_t)i * stride]);
    c[(int64_t)i * stride] = t;
  }
}

struct BandArgs {
  const void* src;
  int64_t src_stride;
  int32_t H, W;
  int32_t vertical;      // 0: bands of rows (profiles run along x), 1: bands of columns (profiles run along y)
  int32_t nprof, maxn;   // profiles of this launch, the widest band among them
  const ProfileBand* bands;
  double* work;
  double z, lam;
  double zpow_along;     // z^(W + 24) / z^(H + 24): the lines along the profile
};

// axis 0: one thread per column of a padded band, reading the image (edge-padded by the clamp) and writing the band's plane
template <typename T>
__global__ void __launch_bounds__(256) band_filter_cols_kernel(const BandArgs a) {
  const int p = blockIdx.y;
  const ProfileBand b = a.bands[p];
  const int Hp = (a.vertical ? a.H : b.n) + 2 * kBandPad, Wp = (a.vertical ? b.n : a.W) + 2 * kBandPad;
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= Wp) return;
  const int y0 = a.vertical ? 0 : b.lo, x0 = a.vertical ? b.lo : 0;      // the band's corner in the image
  const int bh = Hp - 2 * kBandPad, bw = Wp - 2 * kBandPad;
  int sx = col - kBandPad;
  sx = x0 + (sx < 0 ? 0 : (sx > bw - 1 ? bw - 1 : sx));
  const T* __restrict__ scol = static_cast<const T*>(a.src) + sx;
  auto ld = [&](int i) -> double {
    int sy = i - kBandPad;
    sy = y0 + (sy < 0 ? 0 : (sy > bh - 1 ? bh - 1 : sy));
    return (double)scol[(int64_t)sy * a.src_stride];
  };
  band_filter_line(a.work + b.offset + col, (int64_t)Wp, Hp, a.z, a.vertical ? a.zpow_along : b.zpow, a.lam, ld);
}

// axis 1: one thread per row of a padded band, in place
__global__ void __launch_bounds__(256) band_filter_rows_kernel(const BandArgs a) {
  const int p = blockIdx.y;
  const ProfileBand b = a.bands[p];
  const int Hp = (a.vertical ? a.H : b.n) + 2 * kBandPad, Wp = (a.vertical ? b.n : a.W) + 2 * kBandPad;
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= Hp) return;
  double* line = a.work + b.offset + (int64_t)r * Wp;      // read and written in place: no __restrict__
  auto ld = [&](int i) -> double { return line[i]; };
  band_filter_line(line, (int64_t)1, Wp, a.z, a.vertical ? b.zpow : a.zpow_along, a.lam, ld);
}

// the samples: spline_remap_kernel's cubic gather (explicit coordinates, "nearest") on the profile's own coefficient plane
template <typename T>
__global__ void __launch_bounds__(256) band_sample_kernel(const BandArgs a, const double* __restrict__ ycoord, const double* __restrict__ xcoord,
                                                          int len, T* __restrict__ dst) {
  const int p = blockIdx.y;
  const ProfileBand b = a.bands[p];
  const int Hp = (a.vertical ? a.H : b.n) + 2 * kBandPad, Wp = (a.vertical ? b.n : a.W) + 2 * kBandPad;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= len) return;
  // coordinates in the image -> in the band; (tap indices are 32-bit, as in spline_remap_kernel)
  double yc = ycoord[(int64_t)p * len + i] - (a.vertical ? 0.0 : (double)b.lo);
  double xc = xcoord[(int64_t)p * len + i] - (a.vertical ? (double)b.lo : 0.0);
  yc = yc < -1.0e9 ? -1.0e9 : (yc > 1.0e9 ? 1.0e9 : yc);
  xc = xc < -1.0e9 ? -1.0e9 : (xc > 1.0e9 ? 1.0e9 : xc);
  double wy[6], wx[6];
  const int sy = spline_weights<3>(yc + (double)kBandPad, wy);
  const int sx = spline_weights<3>(xc + (double)kBandPad, wx);
  int ix[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) ix[k] = spline_fold(sx + k, Wp, kModeNearest);
  const double* __restrict__ coef = a.work + b.offset;
  double t = 0.0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const double* rowp = coef + (int64_t)spline_fold(sy + j, Hp, kModeNearest) * Wp;
#pragma unroll
    for (int k = 0; k < 4; ++k) t += (rowp[ix[k]] * wy[j]) * wx[k];
  }
  dst[(int64_t)p * len + i] = (T)t;
}

DCP_DEFINE_BOUNDS_READER(read_bounds_profile)

// ------------------------------------------------------------------ launchers

hipError_t launch_peak_rows(const void* src, double* dst, int N, int L, int64_t src_stride, int dtype, int radius, double sensitive, bool subpixel,
                            hipStream_t stream) {
  if (N < 1 || L < 1 || radius < 0 || radius > kPeakMaxRadius || (subpixel && radius < 1) || (dtype != kF32 && dtype != kF64)) return hipErrorInvalidValue;
  if (dtype == kF32)
    hipLaunchKernelGGL((peak_rows_kernel<float>), dim3((unsigned)N), dim3(kPeakBlock), 0, stream, static_cast<const float*>(src), src_stride, L, radius,
                       sensitive, subpixel ? 1 : 0, dst);
  else
    hipLaunchKernelGGL((peak_rows_kernel<double>), dim3((unsigned)N), dim3(kPeakBlock), 0, stream, static_cast<const double*>(src), src_stride, L, radius,
                       sensitive, subpixel ? 1 : 0, dst);
  char name[96];
  snprintf(name, sizeof(name), "peak_rows_kernel<%s, radius=%d%s>", dtype == kF32 ? "float" : "double", radius, subpixel ? ", subpixel" : "");
  set_last_kernel_name(name);
  return hipGetLastError();
}

hipError_t launch_window_slope(const void* src, void* dst, int N, int L, int64_t src_stride, int dtype, int size, hipStream_t stream) {
  if (N < 1 || L < 1 || size < 3 || !(size & 1) || N > 65535 || (dtype != kF32 && dtype != kF64)) return hipErrorInvalidValue;
  const int r = size / 2;
  double den = 0.0;
  for (int k = -r; k <= r; ++k) den += (double)k * (double)k;
  const dim3 grid((unsigned)((L + 255) / 256), (unsigned)N);
  if (dtype == kF32)
    hipLaunchKernelGGL((window_slope_kernel<float>), grid, dim3(256), 0, stream, static_cast<const float*>(src), src_stride, N, L, r, den,
                       static_cast<float*>(dst));
  else
    hipLaunchKernelGGL((window_slope_kernel<double>), grid, dim3(256), 0, stream, static_cast<const double*>(src), src_stride, N, L, r, den,
                       static_cast<double*>(dst));
  char name[96];
  snprintf(name, sizeof(name), "window_slope_kernel<%s, size=%d>", dtype == kF32 ? "float" : "double", size);
  set_last_kernel_name(name);
  return hipGetLastError();
}

size_t profile_band_elems(int H, int W, bool vertical, int n) {
  return vertical ? ((size_t)H + 2 * kBandPad) * ((size_t)n + 2 * kBandPad) : ((size_t)n + 2 * kBandPad) * ((size_t)W + 2 * kBandPad);
}

hipError_t launch_tilted_profiles(const void* src, void* dst, int H, int W, int64_t src_stride, int dtype, bool vertical, int nprof, int len,
                                  const double* ycoord, const double* xcoord, const int32_t* band_lo, const int32_t* band_n, void* work, size_t work_bytes,
                                  hipStream_t stream) {
  if (H < 1 || W < 1 || nprof < 1 || len < 1 || !work || (dtype != kF32 && dtype != kF64)) return hipErrorInvalidValue;
  const double z = sqrt(3.0) - 2.0;
  BandArgs a;
  a.src = src;
  a.src_stride = src_stride;
  a.H = H;
  a.W = W;
  a.vertical = vertical ? 1 : 0;
  a.z = z;
  a.lam = (1.0 - z) * (1.0 - 1.0 / z);
  a.zpow_along = pow(z, (double)((vertical ? H : W) + 2 * kBandPad));
  const size_t esz = dtype == kF32 ? 4 : 8;
  // groups of profiles whose band planes and table fit the workspace: the table first, the planes behind it
  ProfileBand* const table_dev = static_cast<ProfileBand*>(work);
  for (int p0 = 0; p0 < nprof;) {
    ProfileBand table[kProfileGroupMax];
    int g = 0, maxn = 0;
    size_t used = 0;
    const size_t room = (work_bytes - kProfileGroupMax * sizeof(ProfileBand)) / sizeof(double);
    while (p0 + g < nprof && g < kProfileGroupMax) {
      const int lo = band_lo[p0 + g], n = band_n[p0 + g];
      if (lo < 0 || n < 1 || (int64_t)lo + n > (vertical ? W : H)) return hipErrorInvalidValue;
      const size_t elems = profile_band_elems(H, W, vertical, n);
      if (used + elems > room) break;
      table[g].lo = lo;
      table[g].n = n;
      table[g].offset = (int64_t)(kProfileGroupMax * sizeof(ProfileBand) / sizeof(double) + used);
      table[g].zpow = pow(z, (double)(n + 2 * kBandPad));
      used += elems;
      maxn = n > maxn ? n : maxn;
      ++g;
    }
    if (g == 0) return hipErrorInvalidValue;          // (the caller sized the workspace for the widest band)
    hipError_t e = hipMemcpyAsync(table_dev, table, (size_t)g * sizeof(ProfileBand), hipMemcpyHostToDevice, stream);
    // the table is ordinary host memory of this frame: wait until it has been read
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return e;
    a.nprof = g;
    a.maxn = maxn;
    a.bands = table_dev;
    a.work = static_cast<double*>(work);
    const int maxHp = (vertical ? H : maxn) + 2 * kBandPad, maxWp = (vertical ? maxn : W) + 2 * kBandPad;
    const dim3 gcols((unsigned)((maxWp + 255) / 256), (unsigned)g), grows((unsigned)((maxHp + 255) / 256), (unsigned)g);
    const dim3 gsamp((unsigned)((len + 255) / 256), (unsigned)g);
    const double* yc = ycoord + (size_t)p0 * (size_t)len;
    const double* xc = xcoord + (size_t)p0 * (size_t)len;
    char* d = static_cast<char*>(dst) + (size_t)p0 * (size_t)len * esz;
    if (dtype == kF32) {
      hipLaunchKernelGGL((band_filter_cols_kernel<float>), gcols, dim3(256), 0, stream, a);
      hipLaunchKernelGGL(band_filter_rows_kernel, grows, dim3(256), 0, stream, a);
      hipLaunchKernelGGL((band_sample_kernel<float>), gsamp, dim3(256), 0, stream, a, yc, xc, len, reinterpret_cast<float*>(d));
    } else {
      hipLaunchKernelGGL((band_filter_cols_kernel<double>), gcols, dim3(256), 0, stream, a);
      hipLaunchKernelGGL(band_filter_rows_kernel, grows, dim3(256), 0, stream, a);
      hipLaunchKernelGGL((band_sample_kernel<double>), gsamp, dim3(256), 0, stream, a, yc, xc, len, reinterpret_cast<double*>(d));
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
    p0 += g;
    // the next group overwrites the table and the planes: stream order keeps it behind this group's kernels
  }
  char name[128];
  snprintf(name, sizeof(name), "band_filter_cols_kernel + band_filter_rows_kernel + band_sample_kernel<%s, profiles=%d>", dtype == kF32 ? "float" : "double",
           nprof);
  set_last_kernel_name(name);
  return hipSuccess;
}

}  // namespace dcp
