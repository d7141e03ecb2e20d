// binarize_kernels.hip -- the steps of discorpy.prep.preprocessing.binarization (preprocessing.py:216-248) that labelling does not
// cover: np.abs, the minimum / maximum and the histogram behind skimage's threshold_otsu, the comparison with the threshold and the
// 3 x 3-cross morphology behind skimage's opening(mat, disk(1)).  All of them stream a plane once; none waits on another workgroup.
//
//   abs_kernel<U, KIND>        one thread per element.  Floats on their bits (the sign bit cleared, a NaN's too), signed integers
//                              negated in unsigned arithmetic (the minimum wraps to itself as NumPy's does), the rest copied.
//   minmax_kernel<T>           at most kReduceMaxBlocks workgroups stride over the plane; minimum and maximum propagate a NaN as NumPy's
//                              a.min() / a.max() do; per workgroup three doubles (min, max, non-finite count), minmax_final_kernel folds them.
//   histogram_kernel<T, EDGES> EDGES: the bin of an element is found by a binary search of the caller's edges (copied into LDS when
//                              the counts are): the largest j with edges[j] <= a, the last edge closing its bin -- what np.histogram
//                              returns after its two correction steps.  Otherwise bin = a - first.  Lanes of one run of equal bins
//                              along a wave combine first (a ballot of the run heads; the head lane adds the run's length), so a flat
//                              region costs one atomic per wave and not 64 on one LDS word.  Counts are 32-bit in LDS up to
//                              kHistLdsMaxBins bins, flushed with 64-bit atomics; above that (or use_lds = false) the head lanes add to
//                              the int64 counts in global memory directly.  Integer adds: exact in any order.
//   threshold_kernel<T>        four consecutive pixels per thread, (double)a > thres, one 32-bit store where dst is aligned; the set
//                              pixels are counted per wave, per workgroup, then one 64-bit atomic per workgroup.
//   morph_cross_kernel<OP>     a kMorphTW x kMorphTH tile per workgroup; the source box with a halo of 1 (erosion, dilation) or 2
//                              (opening) in LDS, filled with the operation's neutral element outside the image ("ignore what lies
//                              outside").  Opening: the eroded box (halo 1; ZERO outside the image, the dilation's neutral element) in a
//                              second LDS plane, then the dilation -- the plane is read and written once.  Byte planes read along x by
//                              consecutive lanes: 64 lanes touch 16 consecutive banks, whatever the pitch.
#include "dcp_internal.h"

#include <cstdio>
#include <type_traits>

namespace dcp {

constexpr int kBinBlock = 256;
constexpr int kBinWaves = kBinBlock / 64;

static unsigned bin_blocks_of(int64_t n) { return (unsigned)((n + kBinBlock - 1) / kBinBlock); }

// ------------------------------------------------------------------ abs

enum AbsKind : int { kAbsCopy = 0, kAbsFloat = 1, kAbsSigned = 2 };

template <typename U, int KIND>
__global__ void __launch_bounds__(kBinBlock) abs_kernel(const U* __restrict__ src, U* __restrict__ dst, int H, int W, int64_t src_stride) {
  const int64_t n = (int64_t)H * W, i = (int64_t)blockIdx.x * kBinBlock + threadIdx.x;
  if (i >= n) return;
  const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
  U u = src[(int64_t)y * src_stride + x];
  if constexpr (KIND == kAbsFloat) u = (U)(u & (U)~((U)1 << (sizeof(U) * 8 - 1)));
  if constexpr (KIND == kAbsSigned) {
    if (u >> (sizeof(U) * 8 - 1)) u = (U)((U)0 - u);
  }
  dst[i] = u;
}

template <typename U, int KIND>
static hipError_t launch_abs_as(const void* src, void* dst, int H, int W, int64_t src_stride, hipStream_t stream) {
  hipLaunchKernelGGL((abs_kernel<U, KIND>), dim3(bin_blocks_of((int64_t)H * W)), dim3(kBinBlock), 0, stream, static_cast<const U*>(src),
                     static_cast<U*>(dst), H, W, src_stride);
  return hipGetLastError();
}

hipError_t launch_abs(const void* src, void* dst, int H, int W, int64_t src_stride, int dtype, hipStream_t stream) {
  if (H < 1 || W < 1 || (int64_t)H * W > 2147483647LL) return hipErrorInvalidValue;
  hipError_t e;
  switch (dtype) {
    case kF32: e = launch_abs_as<uint32_t, kAbsFloat>(src, dst, H, W, src_stride, stream); break;
    case kF64: e = launch_abs_as<uint64_t, kAbsFloat>(src, dst, H, W, src_stride, stream); break;
    case kI8: e = launch_abs_as<uint8_t, kAbsSigned>(src, dst, H, W, src_stride, stream); break;
    case kI16: e = launch_abs_as<uint16_t, kAbsSigned>(src, dst, H, W, src_stride, stream); break;
    case kI32: e = launch_abs_as<uint32_t, kAbsSigned>(src, dst, H, W, src_stride, stream); break;
    case kI64: e = launch_abs_as<uint64_t, kAbsSigned>(src, dst, H, W, src_stride, stream); break;
    case kU8:
    case kBool: e = launch_abs_as<uint8_t, kAbsCopy>(src, dst, H, W, src_stride, stream); break;
    case kU16: e = launch_abs_as<uint16_t, kAbsCopy>(src, dst, H, W, src_stride, stream); break;
    case kU32: e = launch_abs_as<uint32_t, kAbsCopy>(src, dst, H, W, src_stride, stream); break;
    case kU64: e = launch_abs_as<uint64_t, kAbsCopy>(src, dst, H, W, src_stride, stream); break;
    default: return hipErrorInvalidValue;
  }
  if (e == hipSuccess) set_last_kernel_name("abs_kernel");
  return e;
}

// ------------------------------------------------------------------ minimum, maximum, non-finite count

// NumPy's minimum / maximum: a NaN operand is the result
__device__ __forceinline__ double np_min(double a, double b) { return a != a ? a : (b != b ? b : (b < a ? b : a)); }
__device__ __forceinline__ double np_max(double a, double b) { return a != a ? a : (b != b ? b : (b > a ? b : a)); }

// folds the workgroup's (lo, hi, bad) into thread 0's
__device__ __forceinline__ void block_fold(double& lo, double& hi, double& bad) {
  __shared__ double part[3][kBinWaves];
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    lo = np_min(lo, __shfl_down(lo, d));
    hi = np_max(hi, __shfl_down(hi, d));
    bad += __shfl_down(bad, d);
  }
  if (lane == 0) {
    part[0][wave] = lo;
    part[1][wave] = hi;
    part[2][wave] = bad;
  }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < kBinWaves; ++w) {
      lo = np_min(lo, part[0][w]);
      hi = np_max(hi, part[1][w]);
      bad += part[2][w];
    }
}

template <typename T>
__global__ void __launch_bounds__(kBinBlock) minmax_kernel(const T* __restrict__ src, int H, int W, int64_t src_stride, double* __restrict__ partials) {
  const int64_t n = (int64_t)H * W, step = (int64_t)gridDim.x * kBinBlock;
  const double inf = __builtin_huge_val();
  double lo = inf, hi = -inf, bad = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * kBinBlock + threadIdx.x; i < n; i += step) {
    const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
    const double v = (double)src[(int64_t)y * src_stride + x];
    lo = np_min(lo, v);
    hi = np_max(hi, v);
    if (!(__builtin_fabs(v) < inf)) bad += 1.0;
  }
  block_fold(lo, hi, bad);
  if (threadIdx.x == 0) {
    partials[3 * blockIdx.x + 0] = lo;
    partials[3 * blockIdx.x + 1] = hi;
    partials[3 * blockIdx.x + 2] = bad;          // (a count below 2^31: exact in a double)
  }
}

// one workgroup: nb triples -> out[0] = min, out[1] = max, *nonfinite = the count
__global__ void __launch_bounds__(kBinBlock) minmax_final_kernel(const double* __restrict__ partials, int nb, double* __restrict__ out,
                                                                 long long* __restrict__ nonfinite) {
  const double inf = __builtin_huge_val();
  double lo = inf, hi = -inf, bad = 0.0;
  for (int j = (int)threadIdx.x; j < nb; j += kBinBlock) {
    lo = np_min(lo, partials[3 * j + 0]);
    hi = np_max(hi, partials[3 * j + 1]);
    bad += partials[3 * j + 2];
  }
  block_fold(lo, hi, bad);
  if (threadIdx.x == 0) {
    out[0] = lo;
    out[1] = hi;
    *nonfinite = (long long)bad;
  }
}

static int reduce_blocks(int64_t n) {
  const int64_t want = (n + kBinBlock * 8 - 1) / (kBinBlock * 8);          // about eight elements per thread
  return (int)(want < 1 ? 1 : (want > kReduceMaxBlocks ? kReduceMaxBlocks : want));
}

template <typename T>
static hipError_t launch_minmax_as(const void* src, int H, int W, int64_t src_stride, double* partials, int nb, hipStream_t stream) {
  hipLaunchKernelGGL((minmax_kernel<T>), dim3((unsigned)nb), dim3(kBinBlock), 0, stream, static_cast<const T*>(src), H, W, src_stride, partials);
  return hipGetLastError();
}

hipError_t launch_minmax(const void* src, int H, int W, int64_t src_stride, int dtype, double* partials, double* out, long long* nonfinite,
                         hipStream_t stream) {
  if (H < 1 || W < 1 || (int64_t)H * W > 2147483647LL) return hipErrorInvalidValue;
  const int nb = reduce_blocks((int64_t)H * W);
  hipError_t e;
  switch (dtype) {
    case kF32: e = launch_minmax_as<float>(src, H, W, src_stride, partials, nb, stream); break;
    case kF64: e = launch_minmax_as<double>(src, H, W, src_stride, partials, nb, stream); break;
    case kU8: e = launch_minmax_as<uint8_t>(src, H, W, src_stride, partials, nb, stream); break;
    case kI8: e = launch_minmax_as<int8_t>(src, H, W, src_stride, partials, nb, stream); break;
    case kU16: e = launch_minmax_as<uint16_t>(src, H, W, src_stride, partials, nb, stream); break;
    case kI16: e = launch_minmax_as<int16_t>(src, H, W, src_stride, partials, nb, stream); break;
    default: return hipErrorInvalidValue;
  }
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(minmax_final_kernel, dim3(1), dim3(kBinBlock), 0, stream, partials, nb, out, nonfinite);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  set_last_kernel_name("minmax_kernel + minmax_final_kernel");
  return hipSuccess;
}

// ------------------------------------------------------------------ histogram

struct HistArgs {
  const void* src;
  const void* edges;       // EDGES: nbins + 1 values of the plane's type
  long long* counts;       // nbins, zeroed before the launch
  int64_t src_stride;
  long long first;         // bincount form: the value of bin 0
  int32_t H, W;
  int32_t nbins;
  int32_t use_lds;
};

// EDGES: the largest j in [0, nbins] with e[j] <= a, given e[0] <= a <= e[nbins]; bin nbins belongs to the last one
template <typename T>
__device__ __forceinline__ int edge_bin(const T* e, int nbins, T a) {
  int lo = 0, hi = nbins + 1;          // e[lo] <= a always; hi: a sentinel above every edge
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;          // 1 .. nbins
    if (e[mid] <= a) lo = mid;
    else hi = mid;
  }
  return lo < nbins ? lo : nbins - 1;
}

template <typename T, bool EDGES>
__global__ void __launch_bounds__(kBinBlock) histogram_kernel(const HistArgs a) {
  extern __shared__ unsigned long long hist_lds[];          // use_lds: the edges (EDGES), then nbins 32-bit counts
  const T* __restrict__ src = static_cast<const T*>(a.src);
  const int nbins = a.nbins, tid = (int)threadIdx.x, lane = tid & 63;
  const T* e = static_cast<const T*>(a.edges);
  uint32_t* cnt = nullptr;
  if (a.use_lds) {
    size_t edge_words = 0;
    if constexpr (EDGES) {
      T* le = reinterpret_cast<T*>(hist_lds);
      for (int j = tid; j <= nbins; j += kBinBlock) le[j] = e[j];
      e = le;
      edge_words = ((size_t)(nbins + 1) * sizeof(T) + 7) / 8;
    }
    cnt = reinterpret_cast<uint32_t*>(hist_lds + edge_words);
    for (int j = tid; j < nbins; j += kBinBlock) cnt[j] = 0u;
    __syncthreads();
  }
  const int64_t n = (int64_t)a.H * a.W, step = (int64_t)gridDim.x * kBinBlock;
  // (every thread of a workgroup walks the same number of rounds: the shuffles and the ballot below see whole waves)
  for (int64_t base = (int64_t)blockIdx.x * kBinBlock; base < n; base += step) {
    const int64_t i = base + tid;
    int bin = -1;
    if (i < n) {
      const int y = (int)(i / a.W), x = (int)(i - (int64_t)y * a.W);
      const T v = src[(int64_t)y * a.src_stride + x];
      if constexpr (EDGES) {
        if (v >= e[0] && v <= e[nbins]) bin = edge_bin<T>(e, nbins, v);          // (a NaN fails both comparisons)
      } else {
        const long long d = (long long)v - a.first;
        if (d >= 0 && d < (long long)nbins) bin = (int)d;
      }
    }
    // runs of equal bins along the wave: the head lane of a run adds the run's length
    const int prev = __shfl_up(bin, 1);
    const unsigned long long heads = __ballot(lane == 0 || prev != bin);
    if (bin >= 0 && ((heads >> lane) & 1ull)) {
      const unsigned long long above = lane == 63 ? 0ull : (heads >> (lane + 1));
      const int run = above ? __ffsll((long long)above) : 64 - lane;
      if (cnt) (void)__hip_atomic_fetch_add(&cnt[bin], (uint32_t)run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      else (void)__hip_atomic_fetch_add(&a.counts[bin], (long long)run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  if (cnt) {
    __syncthreads();
    for (int j = tid; j < nbins; j += kBinBlock) {
      const uint32_t c = cnt[j];
      if (c) (void)__hip_atomic_fetch_add(&a.counts[j], (long long)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

template <typename T, bool EDGES>
static hipError_t launch_histogram_as(const HistArgs& a, int nb, size_t lds, hipStream_t stream) {
  hipLaunchKernelGGL((histogram_kernel<T, EDGES>), dim3((unsigned)nb), dim3(kBinBlock), lds, stream, a);
  return hipGetLastError();
}

hipError_t launch_histogram(const void* src, int H, int W, int64_t src_stride, int dtype, const void* edges, int nbins, long long first,
                            long long* counts, bool use_lds, hipStream_t stream) {
  if (H < 1 || W < 1 || (int64_t)H * W > 2147483647LL || nbins < 1 || nbins > 65536) return hipErrorInvalidValue;
  const bool is_float = dtype == kF32 || dtype == kF64;
  if (is_float != (edges != nullptr)) return hipErrorInvalidValue;
  HistArgs a;
  a.src = src;
  a.edges = edges;
  a.counts = counts;
  a.src_stride = src_stride;
  a.first = first;
  a.H = H;
  a.W = W;
  a.nbins = nbins;
  a.use_lds = (use_lds && nbins <= kHistLdsMaxBins) ? 1 : 0;
  size_t lds = 0;          // at most 4097 * 8 + 4096 * 4 bytes = 48 KiB + 8
  if (a.use_lds) lds = (edges ? (((size_t)(nbins + 1) * (size_t)elem_size(dtype) + 7) / 8) * 8 : 0) + (size_t)nbins * sizeof(uint32_t);
  hipError_t e = hipMemsetAsync(counts, 0, (size_t)nbins * sizeof(long long), stream);
  if (e != hipSuccess) return e;
  const int nb = reduce_blocks((int64_t)H * W);
  switch (dtype) {
    case kF32: e = launch_histogram_as<float, true>(a, nb, lds, stream); break;
    case kF64: e = launch_histogram_as<double, true>(a, nb, lds, stream); break;
    case kU8: e = launch_histogram_as<uint8_t, false>(a, nb, lds, stream); break;
    case kI8: e = launch_histogram_as<int8_t, false>(a, nb, lds, stream); break;
    case kU16: e = launch_histogram_as<uint16_t, false>(a, nb, lds, stream); break;
    case kI16: e = launch_histogram_as<int16_t, false>(a, nb, lds, stream); break;
    default: return hipErrorInvalidValue;
  }
  if (e != hipSuccess) return e;
  char name[96];
  snprintf(name, sizeof(name), "histogram_kernel<%s, bins=%d, %s>", edges ? "edges" : "bincount", nbins, a.use_lds ? "lds" : "global");
  set_last_kernel_name(name);
  return hipSuccess;
}

// ------------------------------------------------------------------ threshold

template <typename T>
__global__ void __launch_bounds__(kBinBlock) threshold_kernel(const T* __restrict__ src, uint8_t* __restrict__ dst, int H, int W, int64_t src_stride,
                                                              double thres, long long* count, int dst_aligned) {
  __shared__ int32_t wave_sum[kBinWaves];
  const int64_t n = (int64_t)H * W, i0 = ((int64_t)blockIdx.x * kBinBlock + threadIdx.x) * 4;
  uint32_t packed = 0;
  int32_t mine = 0;
  if (i0 < n) {
    int y = (int)(i0 / W), x = (int)(i0 - (int64_t)y * W);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (i0 + k < n) {
        const uint32_t bit = (double)src[(int64_t)y * src_stride + x] > thres ? 1u : 0u;
        packed |= bit << (8 * k);
        mine += (int32_t)bit;
        if (++x == W) {
          x = 0;
          ++y;
        }
      }
    }
    if (dst_aligned && i0 + 3 < n) *reinterpret_cast<uint32_t*>(dst + i0) = packed;
    else
      for (int k = 0; k < 4 && i0 + k < n; ++k) dst[i0 + k] = (uint8_t)((packed >> (8 * k)) & 0xffu);
  }
  if (!count) return;          // (uniform over the launch)
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) mine += __shfl_down(mine, d);
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    long long s = 0;
    for (int w = 0; w < kBinWaves; ++w) s += wave_sum[w];
    if (s) (void)__hip_atomic_fetch_add(count, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

template <typename T>
static hipError_t launch_threshold_as(const void* src, uint8_t* dst, int H, int W, int64_t src_stride, double thres, long long* count,
                                      hipStream_t stream) {
  const int64_t quads = ((int64_t)H * W + 3) / 4;
  hipLaunchKernelGGL((threshold_kernel<T>), dim3(bin_blocks_of(quads)), dim3(kBinBlock), 0, stream, static_cast<const T*>(src), dst, H, W, src_stride,
                     thres, count, ((uintptr_t)dst & 3u) == 0 ? 1 : 0);
  return hipGetLastError();
}

hipError_t launch_threshold(const void* src, uint8_t* dst, int H, int W, int64_t src_stride, int dtype, double thres, long long* count,
                            hipStream_t stream) {
  if (H < 1 || W < 1 || (int64_t)H * W > 2147483647LL) return hipErrorInvalidValue;
  hipError_t e;
  switch (dtype) {
    case kF32: e = launch_threshold_as<float>(src, dst, H, W, src_stride, thres, count, stream); break;
    case kF64: e = launch_threshold_as<double>(src, dst, H, W, src_stride, thres, count, stream); break;
    case kU8:
    case kBool: e = launch_threshold_as<uint8_t>(src, dst, H, W, src_stride, thres, count, stream); break;
    case kI8: e = launch_threshold_as<int8_t>(src, dst, H, W, src_stride, thres, count, stream); break;
    case kU16: e = launch_threshold_as<uint16_t>(src, dst, H, W, src_stride, thres, count, stream); break;
    case kI16: e = launch_threshold_as<int16_t>(src, dst, H, W, src_stride, thres, count, stream); break;
    case kU32: e = launch_threshold_as<uint32_t>(src, dst, H, W, src_stride, thres, count, stream); break;
    case kI32: e = launch_threshold_as<int32_t>(src, dst, H, W, src_stride, thres, count, stream); break;
    case kU64: e = launch_threshold_as<unsigned long long>(src, dst, H, W, src_stride, thres, count, stream); break;
    case kI64: e = launch_threshold_as<long long>(src, dst, H, W, src_stride, thres, count, stream); break;
    default: return hipErrorInvalidValue;
  }
  if (e == hipSuccess) set_last_kernel_name("threshold_kernel");
  return e;
}

// ------------------------------------------------------------------ morphology by the 3 x 3 cross

constexpr int kMorphPitch = kMorphTW + 8;          // bytes between the rows of an LDS plane (the widest box is kMorphTW + 4)

__device__ __forceinline__ uint8_t u8min(uint8_t a, uint8_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint8_t u8max(uint8_t a, uint8_t b) { return a > b ? a : b; }

// the cross at (ly, lx) of a plane: ERODE the minimum, else the maximum
template <bool ERODE>
__device__ __forceinline__ uint8_t cross_at(const uint8_t* p, int ly, int lx) {
  const uint8_t* c = p + ly * kMorphPitch + lx;
  if constexpr (ERODE) return u8min(u8min(u8min(c[0], c[-1]), u8min(c[1], c[-kMorphPitch])), c[kMorphPitch]);
  return u8max(u8max(u8max(c[0], c[-1]), u8max(c[1], c[-kMorphPitch])), c[kMorphPitch]);
}

// OP 0 erosion, 1 dilation, 2 opening (erosion then dilation)
template <int OP>
__global__ void __launch_bounds__(kBinBlock) morph_cross_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int H, int W,
                                                                int64_t src_stride, int tiles_x) {
  constexpr int R = OP == 2 ? 2 : 1;
  constexpr int BW = kMorphTW + 2 * R, BH = kMorphTH + 2 * R;          // the source box
  constexpr uint8_t kFill = OP == 1 ? 0 : 255;                           // the first step's neutral element
  __shared__ uint8_t box[BH * kMorphPitch];
  __shared__ uint8_t mid[OP == 2 ? (kMorphTH + 2) * kMorphPitch : 4];  // opening: the eroded box, halo 1
  const int tile_y = (int)(blockIdx.x / (unsigned)tiles_x), tile_x = (int)(blockIdx.x - (unsigned)tile_y * (unsigned)tiles_x);
  const int y0 = tile_y * kMorphTH, x0 = tile_x * kMorphTW, tid = (int)threadIdx.x;
  for (int p = tid; p < BH * BW; p += kBinBlock) {
    const int ly = p / BW, lx = p - ly * BW;
    const int y = y0 - R + ly, x = x0 - R + lx;
    box[ly * kMorphPitch + lx] = (y >= 0 && y < H && x >= 0 && x < W) ? src[(int64_t)y * src_stride + x] : kFill;
  }
  __syncthreads();
  const uint8_t* from = box;
  if constexpr (OP == 2) {
    constexpr int MW = kMorphTW + 2, MH = kMorphTH + 2;
    for (int p = tid; p < MH * MW; p += kBinBlock) {
      const int ly = p / MW, lx = p - ly * MW;
      const int y = y0 - 1 + ly, x = x0 - 1 + lx;
      // (outside the image the dilation must see its own neutral element, not an eroded value)
      mid[ly * kMorphPitch + lx] = (y >= 0 && y < H && x >= 0 && x < W) ? cross_at<true>(box, ly + 1, lx + 1) : (uint8_t)0;
    }
    __syncthreads();
    from = mid;
  }
  for (int p = tid; p < kMorphTH * kMorphTW; p += kBinBlock) {
    const int ly = p / kMorphTW, lx = p - ly * kMorphTW;
    const int y = y0 + ly, x = x0 + lx;
    if (y >= H || x >= W) continue;
    dst[(int64_t)y * W + x] = OP == 0 ? cross_at<true>(from, ly + 1, lx + 1) : cross_at<false>(from, ly + 1, lx + 1);
  }
}

template <int OP>
static hipError_t launch_morph_as(const uint8_t* src, uint8_t* dst, int H, int W, int64_t src_stride, hipStream_t stream) {
  const int tiles_x = (W + kMorphTW - 1) / kMorphTW;
  const int64_t tiles = (((int64_t)H + kMorphTH - 1) / kMorphTH) * tiles_x;
  hipLaunchKernelGGL((morph_cross_kernel<OP>), dim3((unsigned)tiles), dim3(kBinBlock), 0, stream, src, dst, H, W, src_stride, tiles_x);
  return hipGetLastError();
}

hipError_t launch_morph_cross(const uint8_t* src, uint8_t* dst, uint8_t* tmp, int H, int W, int64_t src_stride, int op, bool fused,
                              hipStream_t stream) {
  if (H < 1 || W < 1 || (int64_t)H * W > 2147483647LL || op < 0 || op > 2) return hipErrorInvalidValue;
  hipError_t e;
  if (op == 0) e = launch_morph_as<0>(src, dst, H, W, src_stride, stream);
  else if (op == 1) e = launch_morph_as<1>(src, dst, H, W, src_stride, stream);
  else if (fused) e = launch_morph_as<2>(src, dst, H, W, src_stride, stream);
  else {
    if (!tmp) return hipErrorInvalidValue;
    if ((e = launch_morph_as<0>(src, tmp, H, W, src_stride, stream)) != hipSuccess) return e;
    e = launch_morph_as<1>(tmp, dst, H, W, (int64_t)W, stream);
  }
  if (e != hipSuccess) return e;
  set_last_kernel_name(op == 0 ? "morph_cross_kernel<erosion>" : op == 1 ? "morph_cross_kernel<dilation>"
                       : fused ? "morph_cross_kernel<opening>" : "morph_cross_kernel<erosion> + morph_cross_kernel<dilation>");
  return hipSuccess;
}

}  // namespace dcp
