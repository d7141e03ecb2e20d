// gauss_kernels.hip -- the separable symmetric correlation behind scipy.ndimage.gaussian_filter (discorpy.prep.linepattern: the denoise
// step of get_cross_points_hor_lines / _ver_lines, :659,739, and convert_chessboard_to_linepattern, :592), scipy's arithmetic bit for bit.
//
//   weights        2 r + 1 float64 values per axis, symmetric to the bit, computed on the host (scipy's _gaussian_kernel1d); the kernels
//                  get the first r + 1 of them (w[r] is the centre) by value in their argument block and read them with scalar loads.
//   one element    of one pass, e the extended line as doubles:  tmp = e[i] w[r];  for j = -r .. -1:  tmp += (e[i + j] + e[i - j]) w[r + j]
//                  in float64, no fused multiply-add (-ffp-contract=off), then cast to the element type: floats round to nearest,
//                  integers truncate toward zero (scipy's C cast); 64-bit integers are read through a double, as scipy reads them.
//   axes           axis 0 first, then axis 1 on the result of the first pass ROUNDED TO THE ELEMENT TYPE (scipy stores it in the output
//                  array between the passes).
//   extension      position p of a line of length n, any integer p: reflect (p mod 2 n, folded), mirror (p mod (2 n - 2), folded; n = 1:
//                  index 0), nearest (clip), wrap (p mod n), constant (the double `cval`, never cast to the element type; in the
//                  second pass a column outside the image is cval too, not a filtered value).
//
//   gauss_lds_kernel<T>           both passes in one launch: a workgroup of 256 threads stages the source box of its 128 x 32 output tile,
//                                 (32 + 2 ry) x (128 + 2 rx) elements of T, in LDS with both axes folded during the fill (constant mode:
//                                 a position outside holds 0 and is recognised again by its index, which costs one compare per tap
//                                 and only in tiles that reach over an edge), runs the axis-0 pass for the 32 x (128 + 2 rx) positions
//                                 the second pass needs into a second LDS plane as T, then the axis-1 pass from that plane.  In both
//                                 passes the 64 lanes of a wave read 64 consecutive elements of one plane row per tap: no bank conflicts.
//   gauss_axis_kernel<T, AXIS>    one pass per launch with every tap read from global memory: boxes that fit no LDS, a call with one
//                                 axis skipped, radii at which the fused kernel measured slower (gauss_takes_lds), and the lab option
//                                 "x_gauss_lds" = 0.  The same operations in the same order: the same bits.
#include "dcp_device.h"

#include <cstdio>
#include <cstring>

namespace dcp {

constexpr int kGaussTW = 128, kGaussTH = 32;      // output tile of gauss_lds_kernel (the tile of the spline gathers)
constexpr int kGaussBlock = 256;                  // four waves
constexpr int kGaussWaves = kGaussBlock / 64;
constexpr int kGaussAxisTW = 64;                  // gauss_axis_kernel: 64 x 4 pixels per workgroup, one per thread
constexpr size_t kGaussLdsPlain = 64u << 10, kGaussLdsMax = 160u << 10;      // dynamic LDS without / with the function attribute

struct GaussWeights {
  double w[kGaussMaxRadius + 1];      // the first r + 1 weights of the axis: w[r] is the centre
};

struct GaussArgs {
  const void* src;
  void* dst;
  int64_t src_stride, dst_stride;     // elements between rows
  int32_t H, W;
  int32_t ry, rx;                     // gauss_axis_kernel: ry is the radius of its axis, wy its weights
  int32_t mode;                       // GaussExtend
  int32_t tiles_x;                    // blockIdx.x = ty * tiles_x + tx
  uint32_t mid_offset;                // gauss_lds_kernel: byte offset of the second LDS plane
  double cval;
  GaussWeights wy, wx;
};

// scipy's store of a double into the output array: a C cast
template <typename T>
__device__ __forceinline__ T gauss_cast(double v) {
  return static_cast<T>(v);
}

// One output element from an LDS plane: taps `step` elements apart around `c`.  CHECK (constant mode, a tile that reaches over an edge
// of this axis): the tap at distance j is cval where pos + j lies outside [0, n).
template <typename T, bool CHECK>
__device__ __forceinline__ double gauss_lds_taps(const T* c, int step, int r, const GaussWeights& w, int pos, int n, double cval,
                                                 const unsigned char* slab, uint32_t slab_bytes, int site) {
  DCP_BOUNDS((const unsigned char*)(c - r * step) - slab, (size_t)(2 * r * step + 1) * sizeof(T), slab_bytes, site);
  double tmp = (double)c[0] * w.w[r];
  for (int j = -r; j < 0; ++j) {
    double lo = (double)c[j * step], hi = (double)c[-j * step];
    if constexpr (CHECK) {
      if ((unsigned)(pos + j) >= (unsigned)n) lo = cval;
      if ((unsigned)(pos - j) >= (unsigned)n) hi = cval;
    }
    tmp += (lo + hi) * w.w[r + j];
  }
  return tmp;
}

template <typename T>
__global__ void __launch_bounds__(kGaussBlock) gauss_lds_kernel(const GaussArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char gauss_smem[];
  T* box = reinterpret_cast<T*>(gauss_smem);
  T* mid = reinterpret_cast<T*>(gauss_smem + a.mid_offset);
  const T* __restrict__ src = static_cast<const T*>(a.src);
  T* __restrict__ dst = static_cast<T*>(a.dst);
  const int tile_y = (int)(blockIdx.x / (unsigned)a.tiles_x), tile_x = (int)(blockIdx.x - (unsigned)tile_y * (unsigned)a.tiles_x);
  const int y0 = tile_y * kGaussTH, x0 = tile_x * kGaussTW;
  const int bw = kGaussTW + 2 * a.rx, bh = kGaussTH + 2 * a.ry;
  const int lane = (int)threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const uint32_t box_bytes = (uint32_t)(bh * bw) * (uint32_t)sizeof(T), mid_bytes = (uint32_t)(kGaussTH * bw) * (uint32_t)sizeof(T);
  // fill: lanes along a box row, a wave per row; both axes folded here
  const int by0 = y0 - a.ry, bx0 = x0 - a.rx;
  for (int bx = lane; bx < bw; bx += 64) {
    const int sx = gauss_fold(bx0 + bx, a.W, a.mode);
    for (int by = wave; by < bh; by += kGaussWaves) {
      const int sy = gauss_fold(by0 + by, a.H, a.mode);
      box[by * bw + bx] = (sx < 0 || sy < 0) ? (T)0 : src[(int64_t)sy * a.src_stride + sx];
    }
  }
  __syncthreads();
  const bool cst = a.mode == kGaussConstant;
  // axis 0: the rows of the tile at every column of the box, rounded to T
  const bool check_y = cst && (by0 < 0 || y0 + kGaussTH + a.ry > a.H);
  for (int ty = wave; ty < kGaussTH; ty += kGaussWaves) {
    const int y = y0 + ty;
    if (y >= a.H) break;
    for (int bx = lane; bx < bw; bx += 64) {
      const T* c = box + (ty + a.ry) * bw + bx;
      const double tmp = check_y ? gauss_lds_taps<T, true>(c, bw, a.ry, a.wy, y, a.H, a.cval, gauss_smem, box_bytes, 20)
                                 : gauss_lds_taps<T, false>(c, bw, a.ry, a.wy, y, a.H, a.cval, gauss_smem, box_bytes, 20);
      mid[ty * bw + bx] = gauss_cast<T>(tmp);
    }
  }
  __syncthreads();
  // axis 1
  const bool check_x = cst && (bx0 < 0 || x0 + kGaussTW + a.rx > a.W);
  for (int ty = wave; ty < kGaussTH; ty += kGaussWaves) {
    const int y = y0 + ty;
    if (y >= a.H) break;
    for (int tx = lane; tx < kGaussTW; tx += 64) {
      const int x = x0 + tx;
      if (x >= a.W) break;
      const T* c = mid + ty * bw + a.rx + tx;
      const double tmp = check_x ? gauss_lds_taps<T, true>(c, 1, a.rx, a.wx, x, a.W, a.cval, gauss_smem + a.mid_offset, mid_bytes, 21)
                                 : gauss_lds_taps<T, false>(c, 1, a.rx, a.wx, x, a.W, a.cval, gauss_smem + a.mid_offset, mid_bytes, 21);
      dst[(int64_t)y * a.dst_stride + x] = gauss_cast<T>(tmp);
    }
  }
}

// one thread per output pixel, 64 x 4 pixels per workgroup; radius a.ry and weights a.wy along AXIS
template <typename T, int AXIS>
__global__ void __launch_bounds__(kGaussBlock) gauss_axis_kernel(const GaussArgs a) {
  const T* __restrict__ src = static_cast<const T*>(a.src);
  T* __restrict__ dst = static_cast<T*>(a.dst);
  const int tile_y = (int)(blockIdx.x / (unsigned)a.tiles_x), tile_x = (int)(blockIdx.x - (unsigned)tile_y * (unsigned)a.tiles_x);
  const int x = tile_x * kGaussAxisTW + ((int)threadIdx.x & (kGaussAxisTW - 1));
  const int y = tile_y * kGaussWaves + (int)threadIdx.x / kGaussAxisTW;
  if (x >= a.W || y >= a.H) return;
  const int n = AXIS == 0 ? a.H : a.W, i = AXIS == 0 ? y : x, r = a.ry;
  const T* line = AXIS == 0 ? src + x : src + (int64_t)y * a.src_stride;
  const int64_t step = AXIS == 0 ? a.src_stride : 1;
  auto at = [&](int p) -> double {
    const int q = gauss_fold(p, n, a.mode);
    return q < 0 ? a.cval : (double)line[(int64_t)q * step];
  };
  double tmp = (double)line[(int64_t)i * step] * a.wy.w[r];
  for (int j = -r; j < 0; ++j) tmp += (at(i + j) + at(i - j)) * a.wy.w[r + j];
  dst[(int64_t)y * a.dst_stride + x] = gauss_cast<T>(tmp);
}

DCP_DEFINE_BOUNDS_READER(read_bounds_gauss)

// ------------------------------------------------------------------ launchers

// bytes of the two LDS planes of gauss_lds_kernel (the second one starts at a multiple of 16 bytes: *mid_offset)
static size_t gauss_lds_bytes(int ry, int rx, size_t esz, uint32_t* mid_offset) {
  const size_t bw = (size_t)kGaussTW + 2 * (size_t)rx, bh = (size_t)kGaussTH + 2 * (size_t)ry;
  const size_t box = (bh * bw * esz + 15) & ~(size_t)15;
  if (mid_offset) *mid_offset = (uint32_t)box;
  return box + (size_t)kGaussTH * bw * esz;
}

// lds_mode (option "x_gauss_lds"): 0 never; 2 wherever the two planes fit the CU's 160 KiB; 1 where the fused kernel was measured not to
// be slower than one launch per axis (tools/time_gaussian.py: float32 and uint16, radii 12 / 16 / 20 / 24 / 32 / 40): it held the bar in
// every case up to radius 24 whose planes leave room for two workgroups per CU (80 KiB), lost by a factor of two where only one fits
// (float32 from radius 32) and by a tenth at radius 40 in uint16, where the box is 5.7 times the tile.  Element types and radii that
// were not measured follow the same two limits.
bool gauss_takes_lds(int dtype, int ry, int rx, int lds_mode) {
  if (lds_mode <= 0 || ry < 0 || rx < 0) return false;
  const size_t lds = gauss_lds_bytes(ry, rx, (size_t)elem_size(dtype), nullptr);
  if (lds_mode == 1 && (ry > kGaussFusedMaxRadius || rx > kGaussFusedMaxRadius || lds > (size_t)kGaussFusedMaxLds)) return false;
  return lds <= kGaussLdsMax;
}

static const char* gauss_type_name(int dtype) {
  static const char* const names[kNumElemTypes] = {"float32", "float64", "uint8", "int8", "uint16", "int16", "uint32", "int32", "int64", "uint64", "bool"};
  return dtype >= 0 && dtype < kNumElemTypes ? names[dtype] : "?";
}

static void gauss_fill_weights(GaussWeights* g, const double* w, int r) { memcpy(g->w, w, (size_t)(r + 1) * sizeof(double)); }

template <typename T>
static hipError_t launch_gauss_lds(GaussArgs a, hipStream_t stream) {
  const size_t lds = gauss_lds_bytes(a.ry, a.rx, sizeof(T), &a.mid_offset);
  a.tiles_x = (a.W + kGaussTW - 1) / kGaussTW;
  const int64_t tiles = (((int64_t)a.H + kGaussTH - 1) / kGaussTH) * a.tiles_x;
  if (tiles > 2147483647LL) return hipErrorInvalidValue;
  if (lds > kGaussLdsPlain) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&gauss_lds_kernel<T>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL((gauss_lds_kernel<T>), dim3((unsigned)tiles), dim3(kGaussBlock), lds, stream, a);
  return hipGetLastError();
}

template <typename T, int AXIS>
static hipError_t launch_gauss_axis(GaussArgs a, hipStream_t stream) {
  a.tiles_x = (a.W + kGaussAxisTW - 1) / kGaussAxisTW;
  const int64_t tiles = (((int64_t)a.H + kGaussWaves - 1) / kGaussWaves) * a.tiles_x;
  if (tiles > 2147483647LL) return hipErrorInvalidValue;
  hipLaunchKernelGGL((gauss_axis_kernel<T, AXIS>), dim3((unsigned)tiles), dim3(kGaussBlock), 0, stream, a);
  return hipGetLastError();
}

template <typename T>
static hipError_t launch_gauss_typed(const void* src, void* dst, void* tmp, int H, int W, int64_t src_stride, int dtype, const double* wy, int ry,
                                     const double* wx, int rx, int mode, double cval, int lds_mode, hipStream_t stream) {
  GaussArgs a;
  memset(&a, 0, sizeof(a));
  a.H = H;
  a.W = W;
  a.mode = mode;
  a.cval = cval;
  char name[128];
  hipError_t e;
  if (gauss_takes_lds(dtype, ry, rx, lds_mode)) {
    a.src = src;
    a.dst = dst;
    a.src_stride = src_stride;
    a.dst_stride = W;
    a.ry = ry;
    a.rx = rx;
    gauss_fill_weights(&a.wy, wy, ry);
    gauss_fill_weights(&a.wx, wx, rx);
    e = launch_gauss_lds<T>(a, stream);
    snprintf(name, sizeof(name), "gauss_lds_kernel<%s, tile=%dx%d>", gauss_type_name(dtype), kGaussTW, kGaussTH);
  } else {
    const bool both = ry >= 0 && rx >= 0;
    if (both && !tmp) return hipErrorInvalidValue;
    e = hipSuccess;
    if (ry >= 0) {
      a.src = src;
      a.src_stride = src_stride;
      a.dst = both ? tmp : dst;
      a.dst_stride = W;
      a.ry = ry;
      gauss_fill_weights(&a.wy, wy, ry);
      e = launch_gauss_axis<T, 0>(a, stream);
    }
    if (e == hipSuccess && rx >= 0) {
      a.src = both ? tmp : src;
      a.src_stride = both ? (int64_t)W : src_stride;
      a.dst = dst;
      a.dst_stride = W;
      a.ry = rx;
      gauss_fill_weights(&a.wy, wx, rx);
      e = launch_gauss_axis<T, 1>(a, stream);
    }
    if (both) snprintf(name, sizeof(name), "gauss_axis_kernel<%s, axis=0> + gauss_axis_kernel<%s, axis=1>", gauss_type_name(dtype), gauss_type_name(dtype));
    else snprintf(name, sizeof(name), "gauss_axis_kernel<%s, axis=%d>", gauss_type_name(dtype), ry >= 0 ? 0 : 1);
  }
  if (e == hipSuccess) set_last_kernel_name(name);
  return e;
}

hipError_t launch_gauss(const void* src, void* dst, void* tmp, int H, int W, int64_t src_stride, int dtype, const double* wy, int ry,
                        const double* wx, int rx, int boundary, double cval, int lds_mode, hipStream_t stream) {
  if (H < 1 || W < 1 || H > 1073741823 || W > 1073741823 || ry > kGaussMaxRadius || rx > kGaussMaxRadius || (ry >= 0 && !wy) || (rx >= 0 && !wx))
    return hipErrorInvalidValue;
  int mode;
  switch (boundary) {
    case kModeReflect:
    case kModeGridMirror: mode = kGaussReflect; break;
    case kModeConstant:
    case kModeGridConstant: mode = kGaussConstant; break;
    case kModeNearest: mode = kGaussNearest; break;
    case kModeMirror: mode = kGaussMirror; break;
    case kModeGridWrap:
    case kModeWrap: mode = kGaussWrap; break;
    default: return hipErrorInvalidValue;
  }
  if (ry < 0 && rx < 0) {        // both axes skipped: a copy, as scipy's
    const size_t esz = (size_t)elem_size(dtype);
    const hipError_t e = hipMemcpy2DAsync(dst, (size_t)W * esz, src, (size_t)src_stride * esz, (size_t)W * esz, (size_t)H, hipMemcpyDeviceToDevice, stream);
    if (e == hipSuccess) set_last_kernel_name("gauss_copy");
    return e;
  }
#define DCP_GAUSS_CASE(T) return launch_gauss_typed<T>(src, dst, tmp, H, W, src_stride, dtype, wy, ry, wx, rx, mode, cval, lds_mode, stream)
  switch (dtype) {
    case kF32: DCP_GAUSS_CASE(float);
    case kF64: DCP_GAUSS_CASE(double);
    case kU8: DCP_GAUSS_CASE(uint8_t);
    case kI8: DCP_GAUSS_CASE(int8_t);
    case kU16: DCP_GAUSS_CASE(uint16_t);
    case kI16: DCP_GAUSS_CASE(int16_t);
    case kU32: DCP_GAUSS_CASE(uint32_t);
    case kI32: DCP_GAUSS_CASE(int32_t);
    case kI64: DCP_GAUSS_CASE(int64_t);
    case kU64: DCP_GAUSS_CASE(uint64_t);
    default: return hipErrorInvalidValue;
  }
#undef DCP_GAUSS_CASE
}

}  // namespace dcp
