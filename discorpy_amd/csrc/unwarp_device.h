// unwarp_device.h -- the device pieces that the frame kernels (unwarp_kernels.hip) and the stack kernels (stack_kernels.hip) both use:
// the sampler, the tile shapes of the LDS-staged kernels, the corner rule of a workgroup tile, the exact integer blend.  The kernels themselves stay apart (profiles/LAB_NOTEBOOK.md: sharing device functions between
// tuned instantiations moves their register counts).
#pragma once
#include "dcp_internal.h"
#include "dcp_device.h"
#include <type_traits>

namespace dcp {

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

constexpr int kBlock = 256;
#ifndef DCP_STORE_AUX
#define DCP_STORE_AUX 2  // cache-policy bits of the output store: 2 = nt (streamed once, never re-read here)
#endif

// ------------------------------------------------------------------ sampler

struct SrcView {
  __amdgpu_buffer_rsrc_t rsrc;
  int32_t W, H;
  int32_t stride;      // elements
  int32_t cstride;     // elements
};

// One bilinear (or nearest) fetch in flight: the issued loads plus the two fractions.
// PAIR: the x0/x1 taps of a row are one 8-byte load (needs unit column stride, W,H >= 2).
template <int SAMPLER, bool PAIR, typename CT>
struct Fetch {
  u32x2 a, b;          // PAIR: rows y0 / y0+1.  !PAIR: a = (v00, v01), b = (v10, v11)
  CT fx, fy;
};

// Coordinates are already inside [0, W-1] x [0, H-1].  The base tap is held at x0 <= W-2,
// y0 <= H-2: at the far edge the fraction becomes 1 on (len-2, len-1) instead of scipy's 0 on
// (len-1, folded len-1) -- the same value for finite data, and no out-of-range tap exists.
template <int SAMPLER, bool PAIR, typename CT>
__device__ __forceinline__ Fetch<SAMPLER, PAIR, CT> fetch(const SrcView& s, CT xc, CT yc) {
  Fetch<SAMPLER, PAIR, CT> f;
  int xi = (int)xc, yi = (int)yc;   // truncation == floor for non-negative coordinates
  if constexpr (SAMPLER == kNearest) {
    // order 0: index = floor(c + 0.5)  (round half up, not rint)
    xi += (xc - (CT)xi >= (CT)0.5) ? 1 : 0;
    yi += (yc - (CT)yi >= (CT)0.5) ? 1 : 0;
    uint32_t off;
    if constexpr (PAIR) off = (__umul24(yi, s.stride) + (uint32_t)xi) << 2;
    else off = ((uint32_t)yi * (uint32_t)s.stride + (uint32_t)xi * (uint32_t)s.cstride) * 4u;
    f.a.x = __builtin_amdgcn_raw_buffer_load_b32(s.rsrc, off, 0, 0);
    f.fx = f.fy = (CT)0;
    return f;
  } else if constexpr (PAIR) {
    xi = min(xi, s.W - 2);
    yi = min(yi, s.H - 2);
    f.fx = xc - (CT)xi;             // exact
    f.fy = yc - (CT)yi;
    const uint32_t off = (__umul24(yi, s.stride) + (uint32_t)xi) << 2;
    f.a = __builtin_amdgcn_raw_buffer_load_b64(s.rsrc, off, 0, 0);
    f.b = __builtin_amdgcn_raw_buffer_load_b64(s.rsrc, off, s.stride * 4, 0);
    return f;
  } else {
    // any stride, any size: same base-tap rule per axis, four 4-byte loads
    xi = min(xi, max(s.W - 2, 0));
    yi = min(yi, max(s.H - 2, 0));
    f.fx = xc - (CT)xi;
    f.fy = yc - (CT)yi;
    const uint32_t dx = s.W >= 2 ? (uint32_t)s.cstride * 4u : 0u;
    const uint32_t dy = s.H >= 2 ? (uint32_t)s.stride * 4u : 0u;
    const uint32_t off = ((uint32_t)yi * (uint32_t)s.stride + (uint32_t)xi * (uint32_t)s.cstride) * 4u;
    f.a.x = __builtin_amdgcn_raw_buffer_load_b32(s.rsrc, off, 0, 0);
    f.a.y = __builtin_amdgcn_raw_buffer_load_b32(s.rsrc, off + dx, 0, 0);
    f.b.x = __builtin_amdgcn_raw_buffer_load_b32(s.rsrc, off + dy, 0, 0);
    f.b.y = __builtin_amdgcn_raw_buffer_load_b32(s.rsrc, off + dy + dx, 0, 0);
    return f;
  }
}

// The three order-1 arithmetics (same as sample() in oracle/unwarp_oracle.c).
// EDGE = false: the caller knows both fractions are below 1 (tiles strictly inside the image)
template <int SAMPLER, bool PAIR, typename CT, bool EDGE = true>
__device__ __forceinline__ float finish(const Fetch<SAMPLER, PAIR, CT>& f) {
  const float v00 = __uint_as_float(f.a.x), v01 = __uint_as_float(f.a.y);
  const float v10 = __uint_as_float(f.b.x), v11 = __uint_as_float(f.b.y);
  if constexpr (SAMPLER == kNearest) {
    return v00;
  } else if constexpr (SAMPLER == kScipy) {
    // scipy NI_GeometricTransform: w0 = 1 - f, w1 = 1 - w0; ((v*wy)*wx) summed left to right.
    // At the far edge the gather holds the base tap at len - 2 and the fraction is 1, where scipy's taps are (len - 1,
    // len - 1 folded) with fraction 0: the same value for finite data, but scipy's zero-weight tap is the edge pixel itself.
    // Take it too, so that a non-finite pixel at len - 2 does not reach a clipped coordinate (0 * NaN).
    float v00 = __uint_as_float(f.a.x), v01 = __uint_as_float(f.a.y);
    float v10 = __uint_as_float(f.b.x), v11 = __uint_as_float(f.b.y);
    if constexpr (EDGE) {
      if (f.fx == (CT)1) {
        v00 = v01;
        v10 = v11;
      }
      if (f.fy == (CT)1) {
        v00 = v10;
        v01 = v11;
      }
    }
    const double fx = (double)f.fx, fy = (double)f.fy;
    const double wy0 = 1.0 - fy, wy1 = 1.0 - wy0;
    const double wx0 = 1.0 - fx, wx1 = 1.0 - wx0;
    double acc = ((double)v00 * wy0) * wx0;
    acc += ((double)v01 * wy0) * wx1;
    acc += ((double)v10 * wy1) * wx0;
    acc += ((double)v11 * wy1) * wx1;
    return (float)acc;
  } else if constexpr (SAMPLER == kF64Lerp) {
    const double fx = (double)f.fx, fy = (double)f.fy;
    const double a = (double)v00, b = (double)v01, c = (double)v10, d = (double)v11;
    const double top = __builtin_fma(fx, b - a, a);
    const double bot = __builtin_fma(fx, d - c, c);
    return (float)__builtin_fma(fy, bot - top, top);
  } else {
    const float fx = (float)f.fx, fy = (float)f.fy;
    const float top = __builtin_fmaf(fx, v01 - v00, v00);
    const float bot = __builtin_fmaf(fx, v11 - v10, v10);
    return __builtin_fmaf(fy, bot - top, top);
  }
}

__device__ __forceinline__ SrcView make_view(const float* base, uint32_t bytes, int W, int H, int stride,
                                             int cstride) {
  SrcView s;
  s.rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, (int)bytes, 0x00020000);
  s.W = W;
  s.H = H;
  s.stride = stride;
  s.cstride = cstride;
  return s;
}

#ifndef DCP_LDS_TH
#define DCP_LDS_TH 16
#endif
constexpr int kLdsTW = 64, kLdsTH = DCP_LDS_TH;
#ifndef DCP_BOXW
#define DCP_BOXW 80
#endif
#ifndef DCP_BOXH
#define DCP_BOXH 24
#endif
#ifndef DCP_LDS_MARGIN
#define DCP_LDS_MARGIN 0   // extra pixels around the corner hull (0: ~1 tile per 16384 fails the vote on cfg2)
#endif
#ifndef DCP_LDS_WAVES
#define DCP_LDS_WAVES 5
#endif
#ifndef DCP_LDS_BLOCK_WAVES
#define DCP_LDS_BLOCK_WAVES 4   // wave tiles (64 x 16 pixels, stacked vertically) per workgroup
#endif
constexpr int kBoxW = DCP_BOXW, kBoxH = DCP_BOXH;
constexpr int kLdsBW = DCP_LDS_BLOCK_WAVES;

// ------------------------------------------------------------------ integer element types: the exact lerp

// Bilinear blend of 8- / 16-bit integer taps when BOTH coordinates are >= 32: a float32 coordinate in [32, 2^24) is a multiple of
// 2^-18, so the fractions carry at most 18 bits, a tap (or a difference of taps) at most 17, and every product and sum of
// scipy's ((v * wy) * wx) accumulation -- and of the factorised form below -- is EXACTLY representable in a double (<= 53
// bits: 16 + 18 + 18 + 1).  No operation rounds, so the two forms agree bit for bit (and with the true bilinear value), and the
// factorised one costs 13 float64 operations fewer per pixel.  `top` / `bot`: the tap pairs (x0, x0 + 1) of rows y0 / y0 + 1 in
// the low bits of a dword (element 0 in the low half); fx, fy: the fractions.  Tiles whose source box reaches a coordinate
// below 32 keep scipy's operation order (where roundings do occur it is their order that has to be reproduced).
template <typename T>
__device__ __forceinline__ double exact_lerp_pairs(uint32_t top, uint32_t bot, double fx, double fy) {
  constexpr int B = (int)sizeof(T) * 8;
  int a, b, c, d;
  if constexpr (std::is_signed<T>::value) {
    a = __builtin_amdgcn_sbfe(top, 0, B);
    b = __builtin_amdgcn_sbfe(top, B, B);
    c = __builtin_amdgcn_sbfe(bot, 0, B);
    d = __builtin_amdgcn_sbfe(bot, B, B);
  } else {
    a = (int)(top & ((1u << B) - 1u));
    c = (int)(bot & ((1u << B) - 1u));
    if constexpr (B == 16) {
      b = (int)(top >> 16);
      d = (int)(bot >> 16);
    } else {
      b = (int)__builtin_amdgcn_ubfe(top, B, B);
      d = (int)__builtin_amdgcn_ubfe(bot, B, B);
    }
  }
  const double tp = __builtin_fma(fx, (double)(b - a), (double)a);
  const double bt = __builtin_fma(fx, (double)(d - c), (double)c);
  return __builtin_fma(fy, bt - tp, tp);
}

// (exact_lerp_taps -- the same blend on narrow LDS reads -- and to_elem_in_range live in dcp_device.h: the colour kernel shares them)

// ------------------------------------------------------------------ workgroup-shared source box (remap_wg_kernel, stack_wg_kernel)

constexpr int kWgTW = 128, kWgTH = 32;            // outputs per workgroup: 2 x 2 wave tiles of kLdsTW x kLdsTH
constexpr int kWgBoxW = 144, kWgBoxH = 42;        // largest box: 36 chunks of 16 B per row, 42 rows (api_core.cpp: kWgBoxRows / kWgBoxCols)
constexpr int kWgSlabRows = 42;                   // 24 192 B: six workgroups per CU
static_assert(kLdsTW == 64 && kLdsTH == 16, "remap_wg_kernel assumes 64 x 16 wave tiles");

// The rule of wg_corner_tap (unwarp_kernels.hip) on the corner's output pixel (X, Y) of a W x H frame (wmaxf = W - 1, hmaxf = H - 1), for
// stack_wg_kernel under a homography or the fused map (kFused: lanes 0..3 together, corner = lane, as there).  Kept apart from
// wg_corner_tap so that remap_wg_kernel's code does not move.
template <int KIND, int NF>
__device__ __forceinline__ void tile_corner_tap(const MapArgs& map, float wmaxf, float hmaxf, double X, double Y, int corner, int* cxi, int* cyi) {
  double xd, yd;
  if constexpr (KIND == kFused) {
    double px, py;
    corner_coord<kPersp, NF>(map, X, Y, &px, &py);
    const float pxf = round_clip_f32(px, wmaxf), pyf = round_clip_f32(py, hmaxf);
    float qx[4], qy[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      qx[i] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pxf), i));
      qy[i] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pyf), i));
    }
    const float qx0 = fminf(fminf(qx[0], qx[1]), fminf(qx[2], qx[3])), qx1 = fmaxf(fmaxf(qx[0], qx[1]), fmaxf(qx[2], qx[3]));
    const float qy0 = fminf(fminf(qy[0], qy[1]), fminf(qy[2], qy[3])), qy1 = fmaxf(fmaxf(qy[0], qy[1]), fmaxf(qy[2], qy[3]));
    corner_coord<kRadial, NF>(map, (double)((corner & 1) ? qx1 : qx0), (double)((corner & 2) ? qy1 : qy0), &xd, &yd);
  } else {
    corner_coord<KIND, NF>(map, X, Y, &xd, &yd);
  }
  *cxi = (int)round_clip_f32(xd, wmaxf);
  *cyi = (int)round_clip_f32(yd, hmaxf);
}

}  // namespace dcp
