// unwarp_launch.h -- host-side launch decisions that the frame launchers (unwarp_kernels.hip), the stack launchers
// (stack_kernels.hip) and the colour launcher (color_kernels.hip) share: one copy of each.  No device code.
#pragma once
#include "dcp_internal.h"
#include <cstdio>
#include <type_traits>

namespace dcp {

// ------------------------------------------------------------------ the reported kernel name

static const char* kind_name(int k) { return k == kRadial ? "Radial" : k == kPersp ? "Persp" : "Fused"; }
static const char* sampler_name(int s) { return s == kNearest ? "nearest" : s == kScipy ? "scipy" : s == kF64Lerp ? "f64lerp" : "f32lerp"; }
static void note_kernel(const char* kernel, int kind, int nf, int sampler, const char* extra = "") {
  char name[192];
  if (kind >= 0) snprintf(name, sizeof(name), "%s<%s,NF=%d,%s%s>", kernel, kind_name(kind), nf, sampler_name(sampler), extra);
  else snprintf(name, sizeof(name), "%s<NF=%d,%s%s>", kernel, nf, sampler_name(sampler), extra);
  set_last_kernel_name(name);
}

// ------------------------------------------------------------------ the counters of the staged path

// The staged kernels count the tiles that leave the staged path: [0] box did not fit, [1] containment vote failed.  One __device__
// pair per translation unit -- g_lds_stats in unwarp_kernels.hip, g_stack_lds_stats in stack_kernels.hip: without relocatable device
// code a __device__ variable belongs to the code object of its unit (and a `static` one in a shared header changes the code of the
// kernels that count).  Each unit defines its reader with this; dcp_debug_counters sums the units and clears them together.
#define DCP_DEFINE_LDS_STATS_READER(name, stats)                                                             \
  hipError_t name(unsigned long long* out, bool reset) {                                                     \
    hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(stats), sizeof(stats));                               \
    if (e != hipSuccess || !reset) return e;                                                                 \
    const unsigned long long zero[2] = {0, 0};                                                               \
    return hipMemcpyToSymbol(HIP_SYMBOL(stats), zero, sizeof(zero));                                         \
  }

// ------------------------------------------------------------------ run-time value -> template argument

// f(std::integral_constant<int, S>{}) with S the sampler: the four of the frame kernels ...
template <typename F>
static auto with_sampler(int sampler, F&& f) {
  switch (sampler) {
    case kNearest: return f(std::integral_constant<int, kNearest>{});
    case kScipy: return f(std::integral_constant<int, kScipy>{});
    case kF64Lerp: return f(std::integral_constant<int, kF64Lerp>{});
    default: return f(std::integral_constant<int, kF32Lerp>{});
  }
}
// ... and the three order-1 blends of the stack kernels, which have no order-0 instantiation
template <typename F>
static auto with_blend(int sampler, F&& f) {
  switch (sampler) {
    case kScipy: return f(std::integral_constant<int, kScipy>{});
    case kF64Lerp: return f(std::integral_constant<int, kF64Lerp>{});
    default: return f(std::integral_constant<int, kF32Lerp>{});
  }
}

// A coefficient vector shorter than the instantiated length N, padded with zeros: fma(r2, 0, a) = a exactly, so every intermediate of
// the even / odd Horner chains, and the result, is unchanged -- instead of the run-time-length form (coefficients from LDS, more registers).
template <int N>
static MapArgs pad_to(const MapArgs& m) {
  MapArgs p = m;
  for (int i = p.nfact < 0 ? 0 : p.nfact; i < N; ++i) p.fact[i] = 0.0;
  if (p.nfact < N) p.nfact = N;
  return p;
}

// f(std::integral_constant<int, NF>{}, map) for the kernels instantiated at NF = 5, 4 and -1 (run-time length): five coefficients as they
// are, fewer through NF = 4 padded, more -- or any number when `unrolled` is false (option coef_lds) -- with the vector in LDS.
template <typename F>
static auto with_nf_5_4(const MapArgs& map, bool unrolled, F&& f) {
  if (unrolled && map.nfact == 5) return f(std::integral_constant<int, 5>{}, map);
  if (unrolled && map.nfact <= 4) return f(std::integral_constant<int, 4>{}, pad_to<4>(map));
  return f(std::integral_constant<int, -1>{}, map);
}

// ------------------------------------------------------------------ shapes

// The 8-byte pair gather (and every LDS-staged kernel) needs unit column stride and at least a 2 x 2 image; its row offsets are 24-bit
// products (v_mul_u32_u24), so a source whose row stride reaches 2^22 elements (16 MB rows: a column-plane view of a large volume) or
// whose height reaches 2^24 takes the strided kernels with full 32-bit multiplies instead.
static bool pair_gather_ok(const ImageArgs& img) {
  return img.src_col_stride == 1 && img.W >= 2 && img.H >= 2 && img.src_stride < (1 << 22) && img.H < (1 << 24);
}

static int tiles_of(int extent, int tile) { return (extent + tile - 1) / tile; }
// XCD stripes: n tile columns (stack_wg_kernel: tile rows) dealt to the eight XCDs in whole stripes, the grid padded to a multiple of
// eight.  Stripes share source lines inside an L2 (4096 px: 3 % faster than the plain order), but only balance when n divides by eight:
// 20 columns (2560 px) put 3 on four XCDs and 2 on the other four, 7 % slower than the plain order.  Stripes when the widest XCD
// carries at most 7 % more than the average.
static int64_t xcd_padded(int64_t n) { return 8 * ((n + 7) / 8); }
static bool xcd_stripes_balance(int64_t n) { return xcd_padded(n) * 100 <= n * 107; }

// The grid of a frame kernel with one tw x th output tile per workgroup (remap_wg_kernel and its batch, remap_wg_color_kernel): sets
// img->tiles_x / tiles_y, takes stripe order (img->xcd_remap == 2) back to the plain order where the stripes do not balance, and
// returns the grid -- eight times the widest stripe in x under stripe order, blockIdx.z = frame.
static dim3 wg_tile_grid(ImageArgs* img, int tw, int th, int frames = 1) {
  img->tiles_x = tiles_of(img->W, tw);
  img->tiles_y = tiles_of(img->rows_out, th);
  if (img->xcd_remap == 2 && !xcd_stripes_balance(img->tiles_x)) img->xcd_remap = 0;
  return dim3(img->xcd_remap == 2 ? (unsigned)xcd_padded(img->tiles_x) : img->tiles_x, img->tiles_y, frames);
}

}  // namespace dcp
