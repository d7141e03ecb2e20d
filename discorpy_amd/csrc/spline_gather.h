// spline_gather.h -- what the gather kernels of the spline orders share beyond the weights of spline_device.h:
//   spline_wg_kernel / spline_remap_kernel                 (spline_kernels.hip)         one plane
//   spline_wg_color_kernel / spline_remap_color_kernel     (spline_color_kernels.hip)   the channels of an interleaved image
//   spline_wg_frames_kernel / spline_remap_frames_kernel   (spline_frames_kernels.hip)  the frames of a stack
// Device side: the corner hull with the box rule and the `staged` test, the extent and the lane's first chunk of the slab's fill, the
// row table with the staging of a long polynomial.  Host side: the two launch grids, the order / exact dispatch, the polynomial's NF
// instantiations, the choice of staged against fallback with the name it reports.
// Everything here is inlined, and a kernel built from these pieces is byte for byte the kernel that had them written out
// (tools/device_text_hashes.py --per-kernel; profiles/LAB_NOTEBOOK.md, "Spline gathers: shared pieces").  That is the condition for
// a piece to live here.  The tile order, the fill's loads, the tap sum out of the slab and the folding gather do NOT meet it in any
// shape tried -- as functions they move register allocation in all the staged kernels -- and stay written out in the three files;
// spline_kernels.hip holds the commented copy.  Kept apart from spline_device.h, which profile_kernels.hip includes for the weights.
#pragma once
#include "dcp_internal.h"
#include "dcp_device.h"
#include "spline_device.h"
#include <cstdio>
#include <type_traits>

#ifndef DCP_SPLINE_OUT_AUX
#define DCP_SPLINE_OUT_AUX 2   // cache-policy bits of the staged kernels' float32 result store: 2 = nt (0: plain, A/B)
#endif

namespace dcp {

// ------------------------------------------------------------------ corner hull -> box -> staged
// The map at the four corner pixels of the workgroup's 128 x 32 tile (lanes 0..3) gives the hull [cx0, cx1] x [cy0, cy1] of their taps'
// base positions in the padded plane.  Under the host's tile-deviation certificate (MapArgs::tile_dev_ok >= 2: every coordinate of the
// tile within 0.90 px of the bilinear interpolant of the corners) floor(coordinate) lies in [c0 - 1, c1 + 1]; odd orders tap
// floor - ORDER/2 .. + ORDER, even orders floor(coordinate + 0.5) - ORDER/2 .. + ORDER: every tap of every pixel of the tile lies
// inside [c0 - 1 - ORDER/2, c1 + 2 + (ORDER + 1)/2] -- the box.
// staged: the box fits the slab and lies inside the plane (no tap folds); workgroup-uniform, the same for every plane of a launch.
struct SwBox {
  int bx0, bx1, by0, by1;
  bool staged;
};
template <int KIND, int ORDER, int NF>
__device__ __forceinline__ SwBox sw_box(const SplineArgs& a, const MapArgs& map, int tx, int ty, int lane) {
  const float wmaxf = (float)(a.W - 1), hmaxf = (float)(a.H - 1);
  const double X = (double)min(tx * kSwTW + (lane & 1) * (kSwTW - 1), a.W - 1);
  const double Y = (double)min(ty * kSwTH + ((lane >> 1) & 1) * (kSwTH - 1), a.H - 1);
  double xd, yd;
  corner_coord<KIND, NF>(map, X, Y, &xd, &yd);
  const int cxi = (int)round_clip_f32(xd, wmaxf) + a.pad, cyi = (int)round_clip_f32(yd, hmaxf) + a.pad;
  const int xa = __builtin_amdgcn_readlane(cxi, 0), xb = __builtin_amdgcn_readlane(cxi, 1);
  const int xc_ = __builtin_amdgcn_readlane(cxi, 2), xd_ = __builtin_amdgcn_readlane(cxi, 3);
  const int ya = __builtin_amdgcn_readlane(cyi, 0), yb = __builtin_amdgcn_readlane(cyi, 1);
  const int yc_ = __builtin_amdgcn_readlane(cyi, 2), yd_ = __builtin_amdgcn_readlane(cyi, 3);
  const int cx0 = min(min(xa, xb), min(xc_, xd_)), cx1 = max(max(xa, xb), max(xc_, xd_));
  const int cy0 = min(min(ya, yb), min(yc_, yd_)), cy1 = max(max(ya, yb), max(yc_, yd_));
  SwBox b;
  b.bx0 = cx0 - 1 - ORDER / 2, b.bx1 = cx1 + 2 + (ORDER + 1) / 2;
  b.by0 = cy0 - 1 - ORDER / 2, b.by1 = cy1 + 2 + (ORDER + 1) / 2;
  const int bw = b.bx1 - b.bx0 + 1, bh = b.by1 - b.by0 + 1;
  b.staged = bw <= kSwBoxW && bh <= kSwBoxH && b.bx0 >= 0 && b.by0 >= 0 && b.bx1 <= a.Wp - 1 && b.by1 <= a.Hp - 1;
  return b;
}

// ------------------------------------------------------------------ the slab's fill: extent and the lane's first chunk
// The box is copied into the slab by LDS-DMA in 16-byte chunks, kSwCH per slab row, 256 per load of the workgroup, kSwNJ loads (the
// kernels' issue_fill).  A plane's descriptor ends with the box's last row: a chunk of a later row is out of range (zeros, no memory
// access), which replaces a per-lane row test in every load (remap_wg_kernel).  The offsets stay inside ONE plane (spline_wg_takes: a
// plane is smaller than 4 GiB); every plane of a launch gets a descriptor of its own from a 64-bit base.
// One slab serves all the planes of a launch.  Between two planes:
//   RAW  the wave's own loads are retired (vmcnt(0)), then a barrier, then the first read of the slab;
//   WAR  the wave's reads of the slab are retired (lgkmcnt(0)), then a barrier (lds_barrier), then the next plane's first load.
struct SwFill {
  uint32_t rstep;    // bytes per row of the plane
  uint32_t extent;   // of a plane's descriptor
  uint32_t off0;     // the lane's chunk of load 0
  int c160;          // its chunk column
  int nchunk;        // chunks of the box
  bool staged;
};
// (the extent alone, for the kernel that builds its only descriptor before it needs the rest)
__device__ __forceinline__ uint32_t sw_fill_extent(const SplineArgs& a, const SwBox& b) {
  const uint32_t rstep = (uint32_t)a.Wp * 8u;
  const unsigned long long plane_bytes = (unsigned long long)a.Hp * rstep, rows_end = (unsigned long long)(b.by1 + 1) * rstep;
  return (uint32_t)(b.staged && rows_end < plane_bytes ? rows_end : plane_bytes);
}
__device__ __forceinline__ SwFill sw_fill(const SplineArgs& a, const SwBox& b, int wave, int lane) {
  SwFill f;
  f.staged = b.staged;
  f.rstep = (uint32_t)a.Wp * 8u;
  f.extent = sw_fill_extent(a, b);
  const int fc = wave * 64 + lane;
  const int crow0 = fc / kSwCH;
  f.c160 = fc - crow0 * kSwCH;
  f.off0 = ((uint32_t)b.by0 * (uint32_t)a.Wp + (uint32_t)b.bx0) * 8u + (uint32_t)crow0 * f.rstep + (uint32_t)f.c160 * 16u;
  f.nchunk = (b.by1 - b.by0 + 1) * kSwCH;
  return f;
}

// ------------------------------------------------------------------ row table, long polynomials
// NF: length of the radial polynomial (5: coefficients from the kernel arguments, shorter vectors padded with zeros by the launcher --
// fma(r2, 0, a) = a exactly; -1: any length, coefficients staged in LDS; 0: perspective, none).  One row table per wave (lanes 0..15;
// same-wave LDS traffic is ordered, no barrier) for the hoisted evaluation map_coord (dcp_device.h), as remap_wg_kernel's phase 1 --
// round 2 walked the coefficient vector with one scalar load and one wait per coefficient and pixel row.
// (The tables are taken whole and indexed here: handed over as s_row[wave] the address is formed once and the kernels change.)
template <int KIND, int NF, int RW, int NCOEF>
__device__ __forceinline__ void sw_stage_rows(const SplineArgs& a, const MapArgs& map, double (&s_row)[4][16][RW], double (&s_coef)[NCOEF], int wave, int lane,
                                              int y0) {
  if (lane < 16) fill_row<KIND, RW>(map, s_row[wave], lane, (double)min(y0 + lane, a.H - 1));
  if constexpr (NF < 0 && KIND != kPersp) {
    if ((int)threadIdx.x < map.nfact) s_coef[threadIdx.x] = map.fact[threadIdx.x];
    __syncthreads();
  }
}

// ------------------------------------------------------------------ host side: what the three launchers share
// the staged kernels' grid: one workgroup per tile, the x extent a multiple of 8 under the XCD tile order
inline dim3 spline_wg_grid(const SplineArgs& a) {
  const unsigned tiles_x = (unsigned)((a.W + kSwTW - 1) / kSwTW);
  return dim3(a.xcd_remap ? ((tiles_x + 7u) / 8u) * 8u : tiles_x, (unsigned)((a.H + kSwTH - 1) / kSwTH));
}
// the fallback kernels' grid: a thread per pixel, blockIdx.y + 65535 blockIdx.z the row
inline dim3 spline_remap_grid(const SplineArgs& a) {
  return dim3((unsigned)((a.W + kSplBlock - 1) / kSplBlock), (unsigned)(a.H < 65535 ? a.H : 65535), (unsigned)((a.H + 65534) / 65535));
}
// f(integral_constant<int, ORDER>{}) / f(integral_constant<int, ORDER>{}, bool_constant<EXACT>{}) for the call's order and sum
template <class F>
inline void spline_for_order(const SplineArgs& a, F&& f) {
  switch (a.order) {
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    default: f(std::integral_constant<int, 5>{}); break;
  }
}
template <class F>
inline void spline_for_order_exact(const SplineArgs& a, F&& f) {
  spline_for_order(a, [&](auto ord) {
    if (a.exact_sum) f(ord, std::true_type{});
    else f(ord, std::false_type{});
  });
}
// The staged kernels' arguments for this call: f(integral_constant<int, NF>{}, a, map) with the tile order set and the polynomial's
// instantiation chosen -- none for the homography (NF = 0), up to five coefficients zero-padded to NF = 5, longer vectors staged in
// LDS (NF = -1)
template <int KIND, class F>
inline hipError_t spline_wg_with_nf(const SplineArgs& a_in, const MapArgs& map_in, F&& f) {
  SplineArgs a = a_in;
  a.xcd_remap = get_spline_xcd();
  if constexpr (KIND == kPersp) {
    return f(std::integral_constant<int, 0>{}, a, map_in);
  } else {
    if (map_in.nfact > 5) return f(std::integral_constant<int, -1>{}, a, map_in);
    MapArgs map = map_in;
    for (int i = map.nfact < 0 ? 0 : map.nfact; i < 5; ++i) map.fact[i] = 0.0;
    map.nfact = 5;
    return f(std::integral_constant<int, 5>{}, a, map);
  }
}
// Staged or fallback?  Reports "<prefilter> + spline_{wg,remap}<flavour>_kernel<order=N[, <planes>=n]>" as the call's kernel name
// (flavour: "", "_color", "_frames"; planes: nullptr, "channels", "frames") and returns true for the staged kernel.
inline bool spline_pick_gather(const SplineArgs& a, MapKind kind, const MapArgs& map, const char* desc, const char* flavour, const char* planes, int nplanes) {
  const bool wg = spline_wg_takes(a, kind, map);
  char name[200], tail[48] = "";
  if (planes) snprintf(tail, sizeof(tail), ", %s=%d", planes, nplanes);
  snprintf(name, sizeof(name), "%s + spline_%s%s_kernel<order=%d%s>", desc, wg ? "wg" : "remap", flavour, a.order, tail);
  set_last_kernel_name(name);
  return wg;
}

}  // namespace dcp
