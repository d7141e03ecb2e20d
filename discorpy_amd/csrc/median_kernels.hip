// median_kernels.hip -- the 2-D median filter of discorpy.prep.preprocessing (normalization :50-73 runs
// scipy.ndimage.median_filter(mat, 51, mode="reflect"), binarization's denoise step runs it at size 2).
//
// A median is a SELECTION: the element of rank (size_y size_x) / 2 (0-based, ascending) of the window.  No value is computed with:
//
//   key            every element is loaded as an unsigned integer whose order is the order of the values: unsigned types as they are,
//                  signed integers with the sign bit flipped, floats as u ^ (sign ? ~0 : signbit).  32-bit keys for elements up to 32
//                  bits, 64-bit keys for float64 / int64 / uint64.  The output is the element recovered from the selected key.
//   window         rows y - size_y / 2 .. y - size_y / 2 + size_y - 1 (an even size leans to the lower indices and, with the rank
//                  above, returns the upper median: scipy's origin = 0), columns likewise; an index outside the image is reflected
//                  with period 2 n (i mod 2 n, then 2 n - 1 - i where that is >= n: scipy's "reflect"), any number of folds.
//   selection      per output pixel a binary search on the key from its top bit down: the candidate is prefix | 1 << b, the window's
//                  keys below the candidate are counted (one compare and one add per tap), the bit stays if the count is <= rank.  The
//                  greatest value with at most `rank` keys below it is the key of that rank.  As many steps as the element has bits.
//
//   median_lds_kernel<U, KIND, TH>     a workgroup of 256 threads stages the key box of its 64 x TH output tile,
//                                      (TH + size_y - 1) x (64 + size_x - 1) keys, in LDS (the reflection is applied during the fill)
//                                      and every thread selects for TH / 4 pixels of one column.  The 64 lanes of a wave read 64
//                                      consecutive keys of one box row: free of bank conflicts for 4- and 8-byte keys alike.
//   median_global_kernel<U, KIND>      the same selection with every tap read from global memory (the reflected index is walked, not
//                                      divided for): windows whose box fits no tile, and the lab option "x_median_lds" = 0.
#include "dcp_internal.h"
#include "order_keys.h"

#include <cstdio>

namespace dcp {

constexpr int kMedianTW = 64;           // tile width: one wave per tile row
constexpr int kMedianBlock = 256;       // four waves: four tile rows per pass
constexpr int kMedianRowsPerPass = kMedianBlock / kMedianTW;
constexpr size_t kMedianLdsPlain = 64u << 10, kMedianLdsMax = 160u << 10;      // dynamic LDS without / with the function attribute

// scipy's "reflect" (d c b a | a b c d | d c b a) for any i: position in the period of 2 n, folded
__device__ __forceinline__ int median_reflect(int64_t i, int n) {
  const int64_t p = 2 * (int64_t)n;
  int64_t m = i % p;
  if (m < 0) m += p;
  return (int)(m >= n ? p - 1 - m : m);
}

struct MedianArgs {
  const void* src;
  void* dst;
  int64_t src_stride;      // elements between source rows
  int32_t H, W;
  int32_t size_y, size_x;
  int32_t tiles_x;         // median_lds_kernel: tiles per row of tiles (blockIdx.x = ty * tiles_x + tx)
  uint32_t rank;           // size_y * size_x / 2
};

template <typename U, int KIND, int TH>
__global__ void __launch_bounds__(kMedianBlock) median_lds_kernel(const MedianArgs a) {
  typedef typename MedianKey<U>::type K;
  extern __shared__ __attribute__((aligned(16))) unsigned char median_smem[];
  K* box = reinterpret_cast<K*>(median_smem);
  const U* __restrict__ src = static_cast<const U*>(a.src);
  U* __restrict__ dst = static_cast<U*>(a.dst);
  const int tile_y = (int)(blockIdx.x / (unsigned)a.tiles_x), tile_x = (int)(blockIdx.x - (unsigned)tile_y * (unsigned)a.tiles_x);
  const int y0 = tile_y * TH, x0 = tile_x * kMedianTW;
  const int bw = kMedianTW + a.size_x - 1, bh = TH + a.size_y - 1;
  const int lane = (int)threadIdx.x & (kMedianTW - 1), wave = (int)threadIdx.x / kMedianTW;
  // fill: a wave per box row, lanes along it; rows and columns outside the image come from their reflections
  const int64_t by0 = (int64_t)y0 - a.size_y / 2, bx0 = (int64_t)x0 - a.size_x / 2;
  for (int by = wave; by < bh; by += kMedianRowsPerPass) {
    const U* row = src + (int64_t)median_reflect(by0 + by, a.H) * a.src_stride;
    K* out = box + by * bw;
    for (int bx = lane; bx < bw; bx += kMedianTW) out[bx] = median_key<U, KIND>(row[median_reflect(bx0 + bx, a.W)]);
  }
  __syncthreads();
  const int x = x0 + lane;
  if (x >= a.W) return;
  constexpr int kBits = (int)sizeof(U) * 8;
  for (int ty = wave; ty < TH; ty += kMedianRowsPerPass) {
    const int y = y0 + ty;
    if (y >= a.H) return;
    const K* win = box + ty * bw + lane;
    K prefix = 0;
    for (int b = kBits - 1; b >= 0; --b) {
      const K cand = prefix | ((K)1 << b);
      uint32_t below = 0;
      for (int wy = 0; wy < a.size_y; ++wy) {
        const K* r = win + wy * bw;
#pragma unroll 8
        for (int wx = 0; wx < a.size_x; ++wx) below += r[wx] < cand ? 1u : 0u;
      }
      if (below <= a.rank) prefix = cand;
    }
    dst[(int64_t)y * a.W + x] = median_elem<U, KIND>(prefix);
  }
}

// one thread per output pixel, 64 x 4 pixels per workgroup; blockIdx.x = ty * tiles_x + tx as above
template <typename U, int KIND>
__global__ void __launch_bounds__(kMedianBlock) median_global_kernel(const MedianArgs a) {
  typedef typename MedianKey<U>::type K;
  const U* __restrict__ src = static_cast<const U*>(a.src);
  U* __restrict__ dst = static_cast<U*>(a.dst);
  const int tile_y = (int)(blockIdx.x / (unsigned)a.tiles_x), tile_x = (int)(blockIdx.x - (unsigned)tile_y * (unsigned)a.tiles_x);
  const int x = tile_x * kMedianTW + ((int)threadIdx.x & (kMedianTW - 1));
  const int y = tile_y * kMedianRowsPerPass + (int)threadIdx.x / kMedianTW;
  if (x >= a.W || y >= a.H) return;
  // positions in the reflection's period of the window's first row and column; a step is +1 modulo the period
  const int py = 2 * a.H, px = 2 * a.W;           // (H, W < 2^30: the C ABI checks)
  int my0 = (int)(((int64_t)y - a.size_y / 2) % py), mx0 = (int)(((int64_t)x - a.size_x / 2) % px);
  if (my0 < 0) my0 += py;
  if (mx0 < 0) mx0 += px;
  constexpr int kBits = (int)sizeof(U) * 8;
  K prefix = 0;
  for (int b = kBits - 1; b >= 0; --b) {
    const K cand = prefix | ((K)1 << b);
    uint32_t below = 0;
    int my = my0;
    for (int wy = 0; wy < a.size_y; ++wy) {
      const U* row = src + (int64_t)(my < a.H ? my : py - 1 - my) * a.src_stride;
      my = my + 1 == py ? 0 : my + 1;
      int mx = mx0;
      for (int wx = 0; wx < a.size_x; ++wx) {
        below += median_key<U, KIND>(row[mx < a.W ? mx : px - 1 - mx]) < cand ? 1u : 0u;
        mx = mx + 1 == px ? 0 : mx + 1;
      }
    }
    if (below <= a.rank) prefix = cand;
  }
  dst[(int64_t)y * a.W + x] = median_elem<U, KIND>(prefix);
}

// ------------------------------------------------------------------ launchers

// bytes of the key box of a 64 x th tile
static size_t median_box_bytes(int th, int size_y, int size_x, size_t key_bytes) {
  return (size_t)(th + size_y - 1) * (size_t)(kMedianTW + size_x - 1) * key_bytes;
}

// The tile of a call: the tallest of 16 / 8 / 4 rows whose box fits the 64 KiB any launch may ask for, else the tallest that fits
// the CU's 160 KiB (the launch then raises the kernel's dynamic-LDS limit); 0: no box fits, the taps come from global memory.
static int median_tile_rows(int size_y, int size_x, size_t key_bytes) {
  for (size_t cap : {kMedianLdsPlain, kMedianLdsMax})
    for (int th : {16, 8, 4})
      if (median_box_bytes(th, size_y, size_x, key_bytes) <= cap) return th;
  return 0;
}

template <typename U, int KIND, int TH>
static hipError_t launch_median_lds(MedianArgs a, hipStream_t stream) {
  const size_t lds = median_box_bytes(TH, a.size_y, a.size_x, sizeof(typename MedianKey<U>::type));
  const int64_t tiles_y = ((int64_t)a.H + TH - 1) / TH, tiles = tiles_y * a.tiles_x;
  if (tiles > 2147483647LL) return hipErrorInvalidValue;
  if (lds > kMedianLdsPlain) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&median_lds_kernel<U, KIND, TH>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL((median_lds_kernel<U, KIND, TH>), dim3((unsigned)tiles), dim3(kMedianBlock), lds, stream, a);
  return hipGetLastError();
}

template <typename U, int KIND>
static hipError_t launch_median_typed(MedianArgs a, int th, hipStream_t stream) {
  a.tiles_x = (a.W + kMedianTW - 1) / kMedianTW;
  char name[96];
  hipError_t e;
  if (th == 0) {
    const int64_t tiles = (((int64_t)a.H + kMedianRowsPerPass - 1) / kMedianRowsPerPass) * a.tiles_x;
    if (tiles > 2147483647LL) return hipErrorInvalidValue;
    hipLaunchKernelGGL((median_global_kernel<U, KIND>), dim3((unsigned)tiles), dim3(kMedianBlock), 0, stream, a);
    e = hipGetLastError();
    snprintf(name, sizeof(name), "median_global_kernel<bits=%d>", (int)sizeof(U) * 8);
  } else {
    e = th == 16 ? launch_median_lds<U, KIND, 16>(a, stream) : th == 8 ? launch_median_lds<U, KIND, 8>(a, stream)
                                                                       : launch_median_lds<U, KIND, 4>(a, stream);
    snprintf(name, sizeof(name), "median_lds_kernel<bits=%d, tile=%dx%d>", (int)sizeof(U) * 8, kMedianTW, th);
  }
  if (e == hipSuccess) set_last_kernel_name(name);
  return e;
}

hipError_t launch_median(const void* src, void* dst, int H, int W, int64_t src_stride, int dtype, int size_y, int size_x, bool use_lds,
                         hipStream_t stream) {
  if (H < 1 || W < 1 || H > 1073741823 || W > 1073741823 || size_y < 1 || size_x < 1 || (int64_t)size_y * size_x > 2147483647LL)
    return hipErrorInvalidValue;
  MedianArgs a;
  a.src = src;
  a.dst = dst;
  a.src_stride = src_stride;
  a.H = H;
  a.W = W;
  a.size_y = size_y;
  a.size_x = size_x;
  a.tiles_x = 0;
  a.rank = (uint32_t)(((int64_t)size_y * size_x) / 2);
  const int th = use_lds ? median_tile_rows(size_y, size_x, elem_size(dtype) == 8 ? 8 : 4) : 0;
  switch (dtype) {
    case kU8:
    case kBool: return launch_median_typed<uint8_t, kKeyUnsigned>(a, th, stream);
    case kI8: return launch_median_typed<uint8_t, kKeySigned>(a, th, stream);
    case kU16: return launch_median_typed<uint16_t, kKeyUnsigned>(a, th, stream);
    case kI16: return launch_median_typed<uint16_t, kKeySigned>(a, th, stream);
    case kU32: return launch_median_typed<uint32_t, kKeyUnsigned>(a, th, stream);
    case kI32: return launch_median_typed<uint32_t, kKeySigned>(a, th, stream);
    case kF32: return launch_median_typed<uint32_t, kKeyFloat>(a, th, stream);
    case kU64: return launch_median_typed<uint64_t, kKeyUnsigned>(a, th, stream);
    case kI64: return launch_median_typed<uint64_t, kKeySigned>(a, th, stream);
    case kF64: return launch_median_typed<uint64_t, kKeyFloat>(a, th, stream);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace dcp
