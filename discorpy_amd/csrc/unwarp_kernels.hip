// unwarp_kernels.hip -- hand-written gfx950 (CDNA4 / MI355X) kernels for the frames of the backward
// unwarp path of discorpy (reference: discorpy/post/postprocessing.py), and their launchers.
//
//   remap_wg_kernel / remap_lds_kernel / remap_tile_kernel <Radial>  K1  unwarp_image_backward      postprocessing.py:137-148
//   remap_wg_kernel / remap_lds_kernel / remap_tile_kernel <Persp>   K2  correct_perspective_image  postprocessing.py:448-459,486-492
//   remap_lds_kernel / remap_tile_kernel <Fused>   K3  perspective o radial in one pass
//   remap_wg_batch_kernel / box_table_kernel / plan_table_kernel   K1 over many frames, its tile hulls and frame plans
//   remap_coords_kernel         K5  map_index= / _mapping            postprocessing.py:250-251,489-491
//   coord_map_kernel            K6  the float32 (yd, xd) planes      postprocessing.py:144-145,444-459
// (K4, the rows of a stack -- stack_wg_kernel / stack_lds_kernel / stack_rows_kernel / stack_centres_kernel -- is stack_kernels.hip.
// What both units use -- the sampler, the tile shapes, tile_corner_tap, exact_lerp_pairs -- is unwarp_device.h; the launch decisions
// they share are unwarp_launch.h.)
//
// Design (see DESIGN.md section 4 for the selection table and the numbers):
//  * one thread per output pixel column, 64-wide wavefronts along x: a wave's store is 256 B
//    contiguous.  The order-1 frame kernels stage the source in LDS: remap_wg_kernel (certified maps --
//    the host bounds how far a tile's coordinates can stray from the bilinear interpolant of its corner
//    pixels) gives a workgroup of four waves a 128 x 32 output tile and ONE source box, predicted from
//    the tile's four corner pixels and copied with row-contiguous 16-byte LDS-DMA loads that go out
//    between the coordinate rows; remap_lds_kernel gives every wave its own 64 x 16 tile and box
//    (certified, or with every pixel verified against the box: the fused map and uncertified models).
//    The taps of every pixel then come from LDS.  The direct kernel (remap_tile_kernel) gathers tap
//    pairs from global memory with 8-byte buffer loads; it serves float64 coordinates, strided /
//    degenerate sources and the fallback.  stack_wg_kernel (stack_kernels.hip) does the same for the rows of a
//    stack, with two slabs: the box of projection d + 1 streams in while projection d is blended.
//  * the coordinate polynomial is evaluated in fp64 (the reference computes float64 and only
//    then rounds to float32, postprocessing.py:144-145; an fp32 evaluation changes 34 % of the
//    coordinates by one ulp).  Everything that does not depend on x is staged once per
//    workgroup in LDS (yu, yu^2 per row; c*y products for the homography); everything that
//    does not depend on y lives in registers across the row loop; coefficients are SGPR
//    resident (kernarg) for vectors of <= 10 terms and staged in LDS for longer ones.
//  * sqrt is the correctly rounded fp64 result built from v_rsq_f64 + one coupled Newton
//    step + one residual correction (tools/ubench.hip); the two homography divisions share one
//    refined reciprocal and are correctly rounded too (tools/ubench_div.hip).
//  * every global access goes through a buffer descriptor: a 32-bit byte offset per lane, row
//    steps through the scalar offset, hardware bounds checking.
//  * no MFMA: the op is a remap (8 B of HBM traffic per pixel), not a contraction.
//
// Build with -ffp-contract=off: every fused multiply-add below is written explicitly so that
// the arithmetic is the same sequence of IEEE operations as oracle/unwarp_oracle.c.
#include "unwarp_device.h"
#include "unwarp_launch.h"
#include "dcp_lab.h"
#include <cstring>

namespace dcp {

#ifndef DCP_PIPE_DEPTH
#define DCP_PIPE_DEPTH 2
#endif
constexpr int kPipeDepth = DCP_PIPE_DEPTH;
#ifndef DCP_LDS_UNTRACKED_DMA
#define DCP_LDS_UNTRACKED_DMA 1  // 0: remap_lds_kernel's fill through the compiler's LDS-DMA builtin (rounds 1-3; A/B)
#endif
#ifndef DCP_FILL_AUX
#define DCP_FILL_AUX 0   // cache-policy bits of remap_wg_kernel's LDS-DMA fill (2 = nt)
#endif

// ------------------------------------------------------------------ tile bookkeeping

// blockIdx.x -> tile (tx, ty).  The dispatcher places workgroup b on XCD b % 8 (observed, used for
// speed only).  xcd_remap:
//   0  row-major tile order: horizontally adjacent tiles land on different XCDs
//   1  each XCD gets a contiguous run of row-major tiles (a horizontal band of the image)
//   2  each XCD gets a vertical stripe of tile columns and sweeps it row by row: neighbours in x
//      and y share an L2 (their source boxes overlap), while the eight XCDs together still touch
//      one full-width band of rows at a time (even spread over the HBM channels)
__device__ __forceinline__ void logical_tile(int xcd_remap, int tiles_x, int* tx, int* ty) {
  const int b = blockIdx.x;
  if (xcd_remap == 0) {
    *ty = b / tiles_x;
    *tx = b - *ty * tiles_x;
    return;
  }
  const int nb = gridDim.x;
  const int per = nb >> 3, rem = nb & 7;
  const int xcd = b & 7, j = b >> 3;
  const int lin = xcd * per + min(xcd, rem) + j;     // position in the XCD-contiguous enumeration
  if (xcd_remap == 1) {
    *ty = lin / tiles_x;
    *tx = lin - *ty * tiles_x;
    return;
  }
  // enumeration: stripe by stripe; inside a stripe row by row.  Stripe s spans columns
  // [s*wq + min(s, wr), ...) with width wq + (s < wr), wq = tiles_x / 8, wr = tiles_x % 8.
  const int tiles_y = nb / tiles_x;
  const int wq = tiles_x >> 3, wr = tiles_x & 7;
  const int big = (wq + 1) * tiles_y;                 // tiles in one of the first wr (wider) stripes
  int s, off;
  if (lin < wr * big) {
    s = lin / big;
    off = lin - s * big;
  } else {
    const int l2 = lin - wr * big;
    const int small = max(wq, 1) * tiles_y;
    s = wr + l2 / small;
    off = l2 - (s - wr) * small;
  }
  const int w = wq + (s < wr ? 1 : 0);
  const int x0 = s * wq + min(s, wr);
  *ty = off / w;
  *tx = x0 + (off - *ty * w);
}

// ------------------------------------------------------------------ K1 / K2 / K3


// (ColCtx / make_col / fill_row / map_coord -- the hoisted evaluation of the coordinate maps -- live in dcp_device.h: the spline
// gather shares them)

// NF >= 0: polynomial length known at compile time, coefficients read from kernarg (SGPRs).
// NF == -1: runtime length, coefficients staged in LDS.
// PD: rows in flight per thread (software pipeline depth of the gather).
template <int KIND, int NF, int SAMPLER, bool ROUND32, bool PAIR, int PD>
__global__ void __launch_bounds__(kBlock) remap_tile_kernel(const ImageArgs img, const MapArgs map) {
  __shared__ double s_row[kMaxTileRows + PD][4];
  __shared__ double s_coef[kMaxFact];
  using CT = typename std::conditional<ROUND32, float, double>::type;
  using FetchT = Fetch<SAMPLER, PAIR, CT>;

  int tx, ty;
  logical_tile(img.xcd_remap, img.tiles_x, &tx, &ty);
  const int y0 = ty * img.tile_rows;
  const int x = tx * kBlock + (int)threadIdx.x;
  const int rows = min(img.tile_rows, img.rows_out - y0);     // y0: row inside the launch's band of output rows

  // per-row invariants -> LDS.  PD rows past the tile are filled too: the pipeline below runs
  // ahead by PD rows and simply discards what it computed for them.
  if ((int)threadIdx.x < img.tile_rows + PD)
    fill_row<KIND, 4>(map, s_row, threadIdx.x, (double)(img.y_origin + y0 + (int)threadIdx.x));
  if constexpr (NF < 0 && KIND != kPersp) {
    if ((int)threadIdx.x < map.nfact) s_coef[threadIdx.x] = map.fact[threadIdx.x];
  }
  __syncthreads();
  if (x >= img.W) return;

  const SrcView src = make_view(img.src, img.src_bytes, img.W, img.H, img.src_stride, img.src_col_stride);
  const float wmaxf = (float)(img.W - 1), hmaxf = (float)(img.H - 1);
  const double wmaxd = (double)(img.W - 1), hmaxd = (double)(img.H - 1);
  // output rows through one buffer descriptor per row built on the scalar unit: lane offset
  // x*4 in a VGPR; a row past the image gets num_records = 0, i.e. the store is dropped
  const uint32_t row_bytes_out = (uint32_t)img.W * 4u;
  const char* out_base = (const char*)(img.dst + (size_t)y0 * (size_t)img.W);
  const uint32_t xoff = (uint32_t)x * 4u;
  const ColCtx col = make_col<KIND, NF>(map, x);

  // source coordinate of row k of the tile and the gather it starts
  auto issue = [&](int k) -> FetchT {
    double xd, yd;
    map_coord<KIND, NF, 4>(map, s_row, s_coef, col, k, wmaxf, hmaxf, &xd, &yd);
    if constexpr (ROUND32) {
      return fetch<SAMPLER, PAIR, float>(src, round_clip_f32(xd, wmaxf), round_clip_f32(yd, hmaxf));
    } else {
      return fetch<SAMPLER, PAIR, double>(src, clip_f64(xd, wmaxd), clip_f64(yd, hmaxd));
    }
  };

  // software pipeline: PD rows of gathers in flight per thread
  FetchT q[PD];
#pragma unroll
  for (int j = 0; j < PD; ++j) q[j] = issue(j);
  for (int k = 0; k < rows; k += PD) {
#pragma unroll
    for (int j = 0; j < PD; ++j) {
      const float v = finish<SAMPLER, PAIR, CT>(q[j]);
      const __amdgpu_buffer_rsrc_t dst = __builtin_amdgcn_make_buffer_rsrc(
          (void*)(out_base + (size_t)(k + j) * row_bytes_out), 0, (k + j < rows) ? (int)row_bytes_out : 0,
          0x00020000);
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), dst, xoff, 0, DCP_STORE_AUX);
      q[j] = issue(k + j + PD);
    }
  }
}

// ------------------------------------------------------------------ K1 / K2 / K3, LDS-staged gather

// The same maps as remap_tile_kernel, float32-rounded coordinates, order 1, unit column stride.
// Each WAVE owns a 64-wide x 16-tall output tile:
//   phase 1a every lane evaluates the source coordinates of the first and last row of its column;
//            the four corner pixels of the tile predict the bounding box of all its taps;
//   fill     the wave starts copying that box -- at most kBoxW x kBoxH floats -- from HBM/L2 into
//            its own LDS slab with row-contiguous 4-byte-per-lane LDS-DMA loads (one 256 B line
//            pair per instruction, the access shape the vector L1 serves fastest);
//   phase 1b the other 14 rows are evaluated while the fill is in flight, and every lane checks
//            that all its taps lie inside the predicted box (one ballot);
//   phase 2  every lane gathers its four taps from LDS (two ds_read2_b32), blends and stores.
// A box that does not fit (strong minification or skew) or a failed containment vote makes the
// wave fall back to the direct global gather for that tile.  No workgroup barrier is needed after the row table is built:
// slabs are wave-private and a wave's LDS operations execute in order.
// (the tile shapes: unwarp_device.h)
// this unit's statistics of the staged path (see DCP_DEFINE_LDS_STATS_READER): [0] box did not fit, [1] containment vote failed
__device__ unsigned long long g_lds_stats[2];

// VOTE = false: the host has certified (MapArgs::tile_dev_ok, api_core.cpp: tile_deviation_certified) that inside any
// 64 x 16 tile every source coordinate stays within one pixel of the bilinear interpolant of the tile's four corner
// coordinates.  The box is then the corner hull grown by one pixel on every side, it contains every tap by
// construction, and the per-pixel containment vote (two min3/max3 per pixel and a ballot) is not compiled in.
// VOTE = true: no certificate (fused map, strongly curved models): zero margin, every pixel verified.
// (the fused map with runtime-length coefficients needs > 96 VGPRs: three waves per SIMD is what it gets, and what it declares)
template <int KIND, int NF, int SAMPLER, bool VOTE>
__global__ void __launch_bounds__(64 * kLdsBW, NF < 0 ? 3 : DCP_LDS_WAVES) remap_lds_kernel(const ImageArgs img, const MapArgs map) {
  constexpr int kMargin = VOTE ? DCP_LDS_MARGIN : 1;
  // 4 x 7680 B slabs + row table + coefficients <= 32 KB: five workgroups (20 waves) per CU
  __shared__ float s_box[kLdsBW][kBoxH * kBoxW];
  __shared__ double s_row[kLdsBW * kLdsTH][KIND == kRadial ? 2 : 4];
  __shared__ double s_coef[NF < 0 ? kMaxFact : 1];
  using FetchT = Fetch<SAMPLER, true, float>;

  // the wave index is wave-uniform by construction; say so, or every descriptor derived from it
  // is treated as divergent and wrapped in a waterfall loop
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int lane = (int)threadIdx.x & 63;
  DCP_TRACE_WAVE_BEGIN(((unsigned)blockIdx.y * gridDim.x + blockIdx.x) * kLdsBW + (unsigned)wave);
  int tx, ty;
  if (img.xcd_remap == 2) {
    // stripe order without divisions: a 2-D grid whose x extent is 8 * (widest stripe); the
    // linear workgroup id is y * gridDim.x + x, so XCD = blockIdx.x & 7 owns stripe blockIdx.x & 7
    // and all stripes sweep the image row by row together.  Narrower stripes have a few idle
    // workgroups at their right end.
    const int s = blockIdx.x & 7, c = blockIdx.x >> 3;
    const int wq = img.tiles_x >> 3, wr = img.tiles_x & 7;
    if (c >= wq + (s < wr ? 1 : 0)) return;
    tx = s * wq + min(s, wr) + c;
    ty = blockIdx.y;
  } else {
    logical_tile(img.xcd_remap, img.tiles_x, &tx, &ty);
  }
  const int yblk = ty * (kLdsBW * kLdsTH);
  const int y0 = yblk + wave * kLdsTH;            // first row of this wave's tile
  const int x = tx * kLdsTW + lane;

  if ((int)threadIdx.x < kLdsBW * kLdsTH)
    fill_row<KIND, (KIND == kRadial ? 2 : 4)>(map, s_row, threadIdx.x,
                                              (double)(img.y_origin + min(yblk + (int)threadIdx.x, img.rows_out - 1)));
  if constexpr (NF < 0 && KIND != kPersp) {
    if ((int)threadIdx.x < map.nfact) s_coef[threadIdx.x] = map.fact[threadIdx.x];
  }
  __syncthreads();
  DCP_TRACE(1);
  if (y0 >= img.rows_out) return;                 // whole wave past the band of output rows (wave-uniform)
  const int rows = min(kLdsTH, img.rows_out - y0);

  const SrcView src = make_view(img.src, img.src_bytes, img.W, img.H, img.src_stride, 1);
  const float wmaxf = (float)(img.W - 1), hmaxf = (float)(img.H - 1);
  const ColCtx col = make_col<KIND, NF>(map, min(x, img.W - 1));
  const auto* rowtab = s_row + wave * kLdsTH;

  float* box = s_box[wave];
  const uint32_t row_bytes_out = (uint32_t)img.W * 4u;
  const char* out_base = (const char*)(img.dst + (size_t)y0 * (size_t)img.W);
  const uint32_t xoff = (uint32_t)x * 4u;         // lanes with x >= W: the store is out of range and dropped
  const __amdgpu_buffer_rsrc_t dst =
      __builtin_amdgcn_make_buffer_rsrc((void*)out_base, 0, (int)((uint32_t)rows * row_bytes_out), 0x00020000);

  // ---- phase 1a: first and last row of the tile; their end lanes are the tile's four corners
  float xf[kLdsTH], yf[kLdsTH];
  auto eval_row = [&](int k) {
    double xd, yd;
    map_coord<KIND, NF, (KIND == kRadial ? 2 : 4)>(map, rowtab, s_coef, col, k, wmaxf, hmaxf, &xd, &yd);
    xf[k] = round_clip_f32(xd, wmaxf);
    yf[k] = round_clip_f32(yd, hmaxf);
  };
  eval_row(0);
  eval_row(kLdsTH - 1);

  // ---- predicted source box: hull of the corner taps grown by one pixel.  The map is smooth, so
  // the taps of the other 1020 pixels stay inside it (the bulge of a 64-pixel arc is ~0.01 px);
  // phase 1b verifies that for every pixel and the wave falls back to the direct gather if not.
  int cx0, cx1, cy0, cy1;
  {
    const int xa = (int)xf[0], xb = (int)xf[kLdsTH - 1], ya = (int)yf[0], yb = (int)yf[kLdsTH - 1];
    const int xa0 = __builtin_amdgcn_readlane(xa, 0), xa1 = __builtin_amdgcn_readlane(xa, 63);
    const int xb0 = __builtin_amdgcn_readlane(xb, 0), xb1 = __builtin_amdgcn_readlane(xb, 63);
    const int ya0 = __builtin_amdgcn_readlane(ya, 0), ya1 = __builtin_amdgcn_readlane(ya, 63);
    const int yb0 = __builtin_amdgcn_readlane(yb, 0), yb1 = __builtin_amdgcn_readlane(yb, 63);
    cx0 = min(min(xa0, xa1), min(xb0, xb1));
    cx1 = max(max(xa0, xa1), max(xb0, xb1));
    cy0 = min(min(ya0, ya1), min(yb0, yb1));
    cy1 = max(max(ya0, ya1), max(yb0, yb1));
  }
  const int bx0 = max(min(cx0 - kMargin, img.W - 2), 0);
  const int bx1 = min(cx1 + 1 + kMargin, img.W - 1);   // last column held: tap x0+1 of the largest x0 (+ margin)
  const int by0 = max(min(cy0 - kMargin, img.H - 2), 0);
  const int by1 = min(cy1 + 1 + kMargin, img.H - 1);
  const int bw = bx1 - bx0 + 1, bh = by1 - by0 + 1;
  const bool fits = bw <= kBoxW && bh <= kBoxH;
  DCP_TRACE(2);

  // ---- fill: box rows by0..by1 from column bx0, row-contiguous loads that land directly in LDS
  // (buffer_load ... lds, no VGPR round trip).  The row group advances through the scalar offset.
  // All rows are in flight at once and complete underneath phase 1b.  (The slab is filled to its
  // full 80-float pitch: up to 12 columns more than the box needs, from cache lines the
  // neighbouring tile fetches anyway.)
  if (fits) {
    // 16 bytes per lane: 20 lanes cover one slab row (pitch 80 floats), so one instruction fills
    // three consecutive box rows (lanes 0-59) and the LDS image stays lane-linear as LDS-DMA needs
    const uint32_t org = ((uint32_t)by0 * (uint32_t)img.src_stride + (uint32_t)bx0) * 4u;
    const uint32_t rstep = (uint32_t)img.src_stride * 4u;
    typedef __attribute__((address_space(3))) void* lds_ptr;
    static_assert(kBoxW == 80, "the fill maps 20 lanes of 16 bytes to one slab row");
    const int lrow = (int)(__umul24((uint32_t)lane, 13u) >> 8);        // lane / 20 for lane < 64
    const int lcol = lane - lrow * 20;
    const uint32_t voff = (uint32_t)lrow * rstep + (uint32_t)lcol * 16u;   // full 32-bit product: a row stride may exceed 2^24 bytes
    [[maybe_unused]] const dcp_rsrc_words src_words = raw_rsrc_words(img.src, img.src_bytes);
    [[maybe_unused]] const uint32_t box_lds = (uint32_t)(uintptr_t)(lds_ptr)box;
    if (lane < 60) {
      // the whole offset goes through the VGPR so that the descriptor's bounds check sees it: the slab pitch can reach past the last
      // image column / the end of the source buffer, where the load must return zeros instead of touching memory.
      // Radial and perspective maps: hidden from the compiler, which otherwise waits for the fill in front of the first row-table
      // read of phase 1b on the unclipped path -- see lds_dma16_untracked; the wave's own wait is the explicit one below (cfg5
      // 115.3 -> 113.5 us).  The fused map, whose instantiation has no such wait, is 3 % slower that way: it keeps the builtin
      auto three_rows = [&](int r) {
        if (r + lrow < bh) {
          if constexpr (DCP_LDS_UNTRACKED_DMA && KIND != kFused)
            lds_dma16_untracked(src_words, box_lds + (uint32_t)(r * kBoxW * 4), voff + (org + (uint32_t)r * rstep));
          else
            __builtin_amdgcn_raw_ptr_buffer_load_lds(src.rsrc, (lds_ptr)(box + r * kBoxW), 16, voff + (org + (uint32_t)r * rstep), 0, 0, 0);
        }
      };
      if constexpr (DCP_LDS_UNTRACKED_DMA && KIND != kFused) {
        for (int r = 0; r < bh; r += 6) {       // (two loads per turn, by hand: `#pragma unroll` does not unroll around the asm)
          three_rows(r);
          three_rows(r + 3);
        }
      } else {
#pragma unroll 2
        for (int r = 0; r < bh; r += 3) three_rows(r);
      }
    }
  }

  DCP_TRACE(3);
  // ---- phase 1b: the other rows, and this lane's extremes for the containment vote.
  // When the predicted box lies strictly inside the image the clip is skipped: a coordinate that
  // would have been clipped is then outside the box, fails the vote below and the fallback path
  // clips it.  (Border tiles keep the clip: their clipped coordinates are legitimate box members.)
  const bool box_inside = cx0 - kMargin >= 0 && cx1 + 1 + kMargin <= img.W - 1 &&
                          cy0 - kMargin >= 0 && cy1 + 1 + kMargin <= img.H - 1;
  float xmn = 0.f, xmx = 0.f, ymn = 0.f, ymx = 0.f;
  if constexpr (VOTE) {
    xmn = __builtin_fminf(xf[0], xf[kLdsTH - 1]), xmx = __builtin_fmaxf(xf[0], xf[kLdsTH - 1]);
    ymn = __builtin_fminf(yf[0], yf[kLdsTH - 1]), ymx = __builtin_fmaxf(yf[0], yf[kLdsTH - 1]);
  }
  auto rows_1b = [&](auto noclip, auto fastdiv) {
#pragma unroll
    for (int k = 1; k < kLdsTH - 1; ++k) {
      double xd, yd;
      map_coord<KIND, NF, (KIND == kRadial ? 2 : 4), decltype(fastdiv)::value>(map, rowtab, s_coef, col, k, wmaxf,
                                                                               hmaxf, &xd, &yd);
      if constexpr (decltype(noclip)::value) {
        xf[k] = (float)xd;
        yf[k] = (float)yd;
      } else {
        xf[k] = round_clip_f32(xd, wmaxf);
        yf[k] = round_clip_f32(yd, hmaxf);
      }
      if constexpr (VOTE) {
        xmn = __builtin_fminf(xmn, xf[k]);
        xmx = __builtin_fmaxf(xmx, xf[k]);
        ymn = __builtin_fminf(ymn, yf[k]);
        ymx = __builtin_fmaxf(ymx, yf[k]);
      }
    }
  };
  const bool unclipped = box_inside && fits;
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  if (KIND == kRadial || !map.fast_div) {
    if (unclipped) rows_1b(std::true_type{}, I0{});
    else rows_1b(std::false_type{}, I0{});
  } else {
    if (unclipped) rows_1b(std::true_type{}, I1{});
    else rows_1b(std::false_type{}, I1{});
  }
  // tap columns are min(floor(xf), W-2) and +1: inside [bx0, bx1] iff xf >= bx0 and (xf < bx1 or
  // the coordinate was clipped and the box ends at the image edge)
  bool staged = fits;
  if constexpr (VOTE) {
    const bool inside = xmn >= (float)bx0 && (xmx < (float)bx1 || (!unclipped && bx1 == img.W - 1)) &&
                        ymn >= (float)by0 && (ymx < (float)by1 || (!unclipped && by1 == img.H - 1));
    staged = fits && __builtin_amdgcn_ballot_w64(!inside) == 0;
  }
  if (!staged && lane == 0) atomicAdd(&g_lds_stats[fits ? 1 : 0], 1ull);
  DCP_TRACE(4);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");

  DCP_TRACE(5);
  // one descriptor for the rows of the tile that exist; the row offset goes through the scalar
  // offset (not bounds-checked, hence the explicit row and column predicates)
  if (!(x < img.W)) return;                      // no cross-lane work from here on
  if (staged) {
    // ---- phase 2: taps from LDS, blend, store.  Byte address of tap (y0, x0) in the slab:
    // (y0 - by0) * pitch + (x0 - bx0) floats = y0 * (4 pitch) + (4 x0 - 4 (by0 pitch + bx0))
    // the slab's own byte offset inside the workgroup's LDS is folded into the origin term (one scalar add per tile
    // instead of a vector add per pixel)
    const uint32_t negorg4 = (uint32_t)(-(by0 * kBoxW + bx0) * 4) + (uint32_t)(wave * (kBoxH * kBoxW * 4));
    const char* boxb = (const char*)&s_box[0][0];
    // A box that ends before the last image column/row cannot contain the clipped coordinate
    // W-1 / H-1, so interior tiles need no base-tap clamp: floor and fraction are one op each.
    const bool interior = bx1 < img.W - 1 && by1 < img.H - 1;
    // interior tiles form the address in float32 (the only VALU ops that issue a wave in 2 cycles instead of 4):
    // floor = c - fract(c) exactly, address = floor_y * 4 pitch + floor_x * 4 + origin, every term an integer
    // below 2^24 (launch_lds checks H and W), one conversion at the end
    const float negorg4f = (float)(int32_t)negorg4;
    auto tile_rows_loop = [&](auto full, auto inner) {
#pragma unroll
      for (int k = 0; k < kLdsTH; ++k) {
        FetchT f;
        uint32_t addr;
        if constexpr (SAMPLER == kNearest) {
          // order 0: index = floor(c + 0.5); it is one of the two bilinear tap indices, so it lies inside the box
          int xi = (int)xf[k];
          int yi = (int)yf[k];
          xi += (xf[k] - (float)xi >= 0.5f) ? 1 : 0;
          yi += (yf[k] - (float)yi >= 0.5f) ? 1 : 0;
          uint32_t xa;
          asm("v_lshl_add_u32 %0, %1, 2, %2" : "=v"(xa) : "v"(xi), "s"(negorg4));
          asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(addr) : "v"(yi), "s"(kBoxW * 4), "v"(xa));
        } else if constexpr (decltype(inner)::value) {
          f.fx = __builtin_amdgcn_fractf(xf[k]);      // x - floor(x), exact
          f.fy = __builtin_amdgcn_fractf(yf[k]);
          const float flx = xf[k] - f.fx, fly = yf[k] - f.fy;
          const float af = __builtin_fmaf(fly, (float)(kBoxW * 4), __builtin_fmaf(flx, 4.0f, negorg4f));
          addr = (uint32_t)(int32_t)af;
        } else {
          const int xi = min((int)xf[k], img.W - 2);
          const int yi = min((int)yf[k], img.H - 2);
          f.fx = xf[k] - (float)xi;
          f.fy = yf[k] - (float)yi;
          uint32_t xa;
          asm("v_lshl_add_u32 %0, %1, 2, %2" : "=v"(xa) : "v"(xi), "s"(negorg4));
          asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(addr) : "v"(yi), "s"(kBoxW * 4), "v"(xa));
        }
        DCP_BOUNDS(addr - (uint32_t)wave * (uint32_t)(kBoxH * kBoxW * 4), SAMPLER == kNearest ? 4 : kBoxW * 4 + 8, kBoxH * kBoxW * 4, 1);
        const float* t = (const float*)(boxb + addr);
        float v;
        if constexpr (SAMPLER == kNearest) {
          v = t[0];
        } else {
          f.a.x = __float_as_uint(t[0]);
          f.a.y = __float_as_uint(t[1]);
          f.b.x = __float_as_uint(t[kBoxW]);
          f.b.y = __float_as_uint(t[kBoxW + 1]);
          v = finish<SAMPLER, true, float, !decltype(inner)::value>(f);
        }
        if (decltype(full)::value || k < rows)
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), dst, xoff, (uint32_t)k * row_bytes_out,
                                                DCP_STORE_AUX);
      }
    };
    if (rows == kLdsTH && interior) tile_rows_loop(std::true_type{}, std::true_type{});
    else if (rows == kLdsTH) tile_rows_loop(std::true_type{}, std::false_type{});
    else tile_rows_loop(std::false_type{}, std::false_type{});
    DCP_TRACE(6);
    DCP_TRACE_WAVE_END();
  } else {
    // ---- box too large for the slab, or a tap outside the predicted box: direct global gather
#pragma unroll
    for (int k = 0; k < kLdsTH; ++k) {
      const FetchT f = fetch<SAMPLER, true, float>(src, __builtin_amdgcn_fmed3f(xf[k], 0.0f, wmaxf),
                                                   __builtin_amdgcn_fmed3f(yf[k], 0.0f, hmaxf));
      const float v = finish<SAMPLER, true, float>(f);
      if (k < rows)
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), dst, xoff, (uint32_t)k * row_bytes_out,
                                              DCP_STORE_AUX);
    }
  }
}

// ------------------------------------------------------------------ K1 / K2, workgroup-shared source box

// The per-CU rate at which streamed source data can be brought in (vector L1 misses served by the L2: ~10 B/clk per
// CU, ~5 TB/s over the chip -- MI355X_MICROARCH.md, "global_load_dwordx4 (HBM-bound)") is what bounds the staged
// kernels, not HBM: with one box per WAVE tile (64 x 16 outputs, 80 x 21..24 floats fetched, every row segment cut
// into 128-byte lines at both ends) the L2 -> L1 traffic is 8 B per output pixel for 4 B of source.  This kernel
// stages ONE box per WORKGROUP: the four waves own a 2 x 2 arrangement of 64 x 16 sub-tiles (a 128 x 32 output tile),
// the box is the hull of the workgroup tile's four corner pixels grown by one pixel (host certificate for that tile
// shape: MapArgs::tile_dev_ok == 2), and the four waves copy it into one shared slab with 16-byte LDS-DMA loads --
// longer row segments (fewer partial lines) and half the halo rows: ~5.9 B per output pixel.
//   corners   every wave evaluates the workgroup tile's four corner pixels itself (lanes 0..3): no exchange, no barrier;
//   fill      the slab is a linear array of 16-byte chunks, 36 per row of pitch 144 floats; chunk (4 j + wave) 64 + lane
//             belongs to lane `lane` of wave `wave` in its j-th load (at most 6 per wave);
//   phase 1   the source coordinates of the sub-tile's 16 rows while the loads are in flight (row table per wave);
//   barrier   every wave waits for its own loads, then for the other waves' (the only barrier of the kernel);
//   phase 2   taps from the shared slab, blend, store -- as in remap_lds_kernel.
// A box that does not fit the slab (magnification > ~1.1) sends the whole workgroup to the direct global gather.
#ifndef DCP_WG_UNTRACKED_DMA
#define DCP_WG_UNTRACKED_DMA 1   // 0: remap_wg_kernel's fill through the compiler's LDS-DMA builtin (rounds 2-3; A/B)
#endif
#ifndef DCP_WG_FILL_START
#define DCP_WG_FILL_START 0   // phase 1 row in front of which the first load of the fill is issued
#endif
#ifndef DCP_WG_FILL_EVERY
#define DCP_WG_FILL_EVERY 1   // phase 1 rows between two loads of the fill (0: all six loads in one burst in front of phase 1)
#endif
#ifndef DCP_WG_WAVES
#define DCP_WG_WAVES 6      // waves per SIMD the register allocation aims at (six 24 KB workgroups fit a CU's LDS)
#endif
// Corner `corner` (bit 0: right, bit 1: bottom) of workgroup tile (tx, yblk / kWgTH): its source pixel, rounded and clipped as the
// taps are.  Pixels past the image are clamped to the last valid ones, so the corners span exactly the valid part of the tile.
template <int KIND, int NF>
__device__ __forceinline__ void wg_corner_tap(const ImageArgs& img, const MapArgs& map, int tx, int yblk, int corner, int* cxi, int* cyi) {
  const float wmaxf = (float)(img.W - 1), hmaxf = (float)(img.H - 1);
  const double X = (double)min(tx * kWgTW + (corner & 1) * (kWgTW - 1), img.W - 1);
  const double Y = (double)(img.y_origin + min(yblk + ((corner >> 1) & 1) * (kWgTH - 1), img.rows_out - 1));
  double xd, yd;
  if constexpr (KIND == kFused) {
    // Lanes 0..3 together (corner = lane).  The homography maps the tile onto a convex quadrilateral (denominator of one sign: the
    // host's certificate), so the float32-rounded, clipped perspective positions of ALL its pixels -- rounding and clipping are
    // monotone -- lie in the bounding box Q of the four corners' positions.  The radial map is then taken at the corners of Q: its
    // deviation from the bilinear interpolant of those four values over Q is what the certificate bounds, so their hull grown by
    // one pixel holds every tap of the tile -- also of a tile that the inner clip cuts through, where the composed map has a kink.
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

// T: element type of source and result.  float is the tuned float32 path (any blend).  uint8 / int8 / uint16 / int16
// (what detectors and cameras deliver) run the same kernel on narrower slab rows -- 16-bit: 20 chunks of 16 bytes =
// 160 elements, 8-bit: 10 chunks = 160 elements, the box's first column rounded down to a 4-byte boundary -- read their
// taps with ds_read_u16 / _i16 / _u8 / _i8, blend in scipy's exact float64 operation order (SAMPLER = kScipy; the
// integer result depends on it at rounding ties) and convert as scipy does: round half away from zero, saturate.
// ImageArgs::src / dst / src_stride / src_bytes keep their meaning (pointers reinterpreted, stride in ELEMENTS, extent in bytes).
// (the body is a device function: the single-frame kernel and the multi-frame kernel remap_wg_batch_kernel share it)
// PLAN: the launch carries a frame plan (frame_plan.cpp; float32, radial map, NF >= 0): every tile's hull comes from the plan's table, and
// a wave tile whose certificate bit is set takes its twelve non-node coordinate rows from the cubic of radial_rows_interp.
template <int KIND, int NF, int SAMPLER, typename T, bool PLAN = false>
__device__ __forceinline__ void remap_wg_body(const ImageArgs& img, const MapArgs& map) {
  constexpr bool kIsF32 = std::is_same<T, float>::value;
  static_assert(!PLAN || (kIsF32 && KIND == kRadial && NF >= 0), "frame plans: float32, radial map, unrolled polynomial");
  constexpr int ES = (int)sizeof(T);                           // element size in bytes
  constexpr int CH = ES == 4 ? 36 : (ES == 2 ? 20 : 10);       // 16-byte chunks per slab row
  constexpr int PB = CH * 16;                                  // slab pitch in bytes
  constexpr int kBoxWEl = PB / ES;                             // widest box in elements: 144 / 160 / 160
  constexpr int NJ = (kWgBoxH * CH + 255) / 256;               // loads per wave that cover the slab: 6 / 4 / 2
  static_assert(kIsF32 || SAMPLER == kNearest || SAMPLER == kScipy, "integer element types blend in scipy's exact order");
  // (the slab holds every chunk the NJ loads of the four waves can write -- 43 rows of float32, 52 of the narrower types --
  // so that no lane of a load has to be masked: rows past the box are past the fill descriptor's extent and arrive as zeros)
  constexpr int kSlabChunks = NJ * 256;
  __shared__ __attribute__((aligned(16))) unsigned char s_box[kSlabChunks * 16];
  static_assert(kSlabChunks * 16 >= kWgSlabRows * PB, "the slab covers the largest box");
  __shared__ double s_row[4][kLdsTH][KIND == kRadial ? 2 : 4];     // one row table per wave: no barrier before it is read
  __shared__ double s_coef[NF < 0 ? kMaxFact : 1];
  using FetchT = Fetch<SAMPLER, true, float>;
  constexpr int RW = KIND == kRadial ? 2 : 4;
  const T* const srcT = (const T*)img.src;
  T* const dstT = (T*)img.dst;

  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int lane = (int)threadIdx.x & 63;
  const int wx = wave & 1, wy = wave >> 1;
  DCP_TRACE_WAVE_BEGIN((((unsigned)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 4u + (unsigned)wave);
  // tile order: XCD blockIdx.x & 7 owns a vertical stripe of tile columns and sweeps it row by row (see remap_lds_kernel)
  int tx, ty;
  if (img.xcd_remap == 2) {
    const int s = blockIdx.x & 7, c = blockIdx.x >> 3;
    const int wq = img.tiles_x >> 3, wr = img.tiles_x & 7;
    if (c >= wq + (s < wr ? 1 : 0)) return;
    tx = s * wq + min(s, wr) + c;
    ty = blockIdx.y;
  } else {                       // plain row-major order (grid = tiles_x x tiles_y): x-neighbours on different XCDs, every XCD the same load
    tx = blockIdx.x;
    ty = blockIdx.y;
  }
  const int yblk = ty * kWgTH;
  // (wave-uniform by construction; said explicitly, or the store descriptor derived from it lands in VGPRs and every
  // store is wrapped in a waterfall loop)
  const int y0 = __builtin_amdgcn_readfirstlane(yblk + wy * kLdsTH);   // first row of this wave's sub-tile (inside the band of output rows)
  const int x = tx * kWgTW + wx * kLdsTW + lane;
  const float wmaxf = (float)(img.W - 1), hmaxf = (float)(img.H - 1);

  // ---- the workgroup tile's four corner pixels, one per lane 0..3, by every wave for itself (no exchange, no barrier:
  // the fill below can start a few hundred cycles into the wave's life).  Pixels past the image are clamped to the
  // last valid ones, so the corners span exactly the valid part of the tile.  The values may differ from the
  // row-hoisted evaluation of phase 1 in the last bits; the certificate leaves 0.05 px for that.
  int cx0, cx1, cy0, cy1;
  [[maybe_unused]] bool certified = false;       // PLAN: plan_table_kernel found the interpolated rows of this wave tile equal to the exact ones
  if (PLAN || img.boxes != nullptr) {
    // (the hull was computed once per tile by box_table_kernel with the same code: four scalars from one scalar load,
    // instead of ~70 vector instructions in each of the four waves)
    typedef __attribute__((address_space(4))) const int32_t* const_ptr;
    const const_ptr b = (const_ptr)(img.boxes + 4 * ((size_t)blockIdx.z * img.tiles_y * img.tiles_x + (size_t)ty * img.tiles_x + tx));
    cx0 = b[0];
    cx1 = b[1];
    cy0 = b[2];
    cy1 = b[3];
    if constexpr (PLAN) {
      // (the certificate words follow the hulls of the plan's tiles_x * tiles_y tiles)
      const const_ptr c = (const_ptr)(img.boxes + (4 * (size_t)img.tiles_y * img.tiles_x + (size_t)ty * img.tiles_x + tx));
      certified = ((c[0] >> wave) & 1) != 0;      // (wave-uniform: a scalar load and a scalar shift)
    }
  } else {
    int cxi, cyi;
    wg_corner_tap<KIND, NF>(img, map, tx, yblk, lane, &cxi, &cyi);
    const int xa = __builtin_amdgcn_readlane(cxi, 0), xb = __builtin_amdgcn_readlane(cxi, 1);
    const int xc_ = __builtin_amdgcn_readlane(cxi, 2), xd_ = __builtin_amdgcn_readlane(cxi, 3);
    const int ya = __builtin_amdgcn_readlane(cyi, 0), yb = __builtin_amdgcn_readlane(cyi, 1);
    const int yc_ = __builtin_amdgcn_readlane(cyi, 2), yd_ = __builtin_amdgcn_readlane(cyi, 3);
    cx0 = min(min(xa, xb), min(xc_, xd_));
    cx1 = max(max(xa, xb), max(xc_, xd_));
    cy0 = min(min(ya, yb), min(yc_, yd_));
    cy1 = max(max(ya, yb), max(yc_, yd_));
  }
  // hull of the corner taps grown by one pixel (the certified deviation is below one pixel)
  // (narrow element types: the first column rounded down to a 4-byte boundary of the source row, as the 16-byte copies need)
  const int bx0 = max(min(cx0 - 1, img.W - 2), 0) & ~(4 / ES - 1);
  const int bx1 = min(cx1 + 2, img.W - 1);
  const int by0 = max(min(cy0 - 1, img.H - 2), 0);
  const int by1 = min(cy1 + 2, img.H - 1);
  const int bw = bx1 - bx0 + 1, bh = by1 - by0 + 1;
  const bool fits = bw <= kBoxWEl && bh <= kWgBoxH;          // workgroup-uniform
  DCP_TRACE(1);
  DCP_TRACE(2);

  // ---- fill: this wave's share of the box.  The slab is a linear array of 16-byte chunks, 36 per row of pitch 144
  // floats; chunk (4 j + wave) 64 + lane belongs to lane `lane` of wave `wave` in its j-th load (at most 6 per wave).
  // Advancing j adds 256 chunks = 7 rows + 4 chunks: row and byte offset of load j follow from those of load 0 with
  // one wrap test.  (A/B-tested against dealing whole row triples to the waves through per-load descriptors -- no
  // vector arithmetic per load at all, but 5 us slower per frame.)  The loads are not issued in one burst: load j
  // goes out in front of coordinate row DCP_WG_FILL_EVERY * j of phase 1 (a wave stuck at a full memory queue does no arithmetic).
  typedef __attribute__((address_space(3))) void* lds_ptr;
  static_assert(kWgBoxW == 144 && kWgBoxH * 36 <= 6 * 256, "six loads of 64 chunks per wave cover the float32 slab");
  const uint32_t rstep = (uint32_t)img.src_stride * (uint32_t)ES;      // source row pitch in bytes
  // the fill's descriptor ends with the box's last row: a chunk of a later row is out of range -- zeros, and no memory access --
  // which replaces the per-lane row test of every load (7 -> 3 vector instructions per load)
  const unsigned long long rows_end = (unsigned long long)(by1 + 1) * rstep;
  const uint32_t fill_extent = rows_end < (unsigned long long)img.src_bytes ? (uint32_t)rows_end : img.src_bytes;
  [[maybe_unused]] const __amdgpu_buffer_rsrc_t src_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)img.src, 0, (int)fill_extent, 0x00020000);
  [[maybe_unused]] const dcp_rsrc_words src_words = raw_rsrc_words(img.src, fill_extent);
  [[maybe_unused]] const uint32_t box0 = (uint32_t)(uintptr_t)(lds_ptr)&s_box[0];
  const int fc = wave * 64 + lane;
  const int crow0 = fc / CH;                                            // (constant divisor: a multiply and a shift)
  const int c160 = fc - crow0 * CH;
  const uint32_t off0 = ((uint32_t)by0 * (uint32_t)img.src_stride + (uint32_t)bx0) * (uint32_t)ES + (uint32_t)crow0 * rstep + (uint32_t)c160 * 16u;
  const int nchunk = bh * CH;
  auto issue_fill = [&](auto jc) {
    constexpr int j = decltype(jc)::value;
    if constexpr (j < NJ) {
      if (fits && (j * 4 + wave) * 64 < nchunk) {             // wave-uniform: does any chunk of this load lie inside the box?
        // 256 j chunks further on: (256 j) / CH whole rows, and the column wraps into the next row at most once
        constexpr int qrow = (256 * j) / CH, rem = (256 * j) % CH;
        const bool wrap = c160 >= CH - rem;
        // (the two alternatives are scalars: one compare, one select, one add per load)
        const uint32_t step_nowrap = (uint32_t)qrow * rstep + (uint32_t)rem * 16u, step_wrap = step_nowrap + rstep - (uint32_t)PB;
#if DCP_WG_UNTRACKED_DMA
        // (hidden from the compiler, which otherwise puts `s_waitcnt vmcnt(0)` in front of a row-table read in the middle of phase 1
        // on the interior-tile path: see lds_dma16_untracked.  The wait for the fill is the explicit one in front of the barrier below)
        lds_dma16_untracked(src_words, box0 + (uint32_t)((j * 4 + wave) * 1024), off0 + (wrap ? step_wrap : step_nowrap));
#else
        __builtin_amdgcn_raw_ptr_buffer_load_lds(src_rsrc, (lds_ptr)(s_box + (j * 4 + wave) * 1024), 16, off0 + (wrap ? step_wrap : step_nowrap), 0, 0,
                                                 DCP_FILL_AUX);
#endif
      }
    }
  };

  DCP_TRACE(3);
  // ---- row table of this wave's 16 rows (lanes 0..15; same-wave LDS traffic is ordered, no barrier)
  if (lane < kLdsTH)
    fill_row<KIND, RW>(map, s_row[wave], lane, (double)(img.y_origin + min(y0 + lane, img.rows_out - 1)));
  if constexpr (NF < 0 && KIND != kPersp) {
    if ((int)threadIdx.x < map.nfact) s_coef[threadIdx.x] = map.fact[threadIdx.x];
    __syncthreads();
  }
  // (max(0, min(..)) selects v_med3_i32, a VALU-only instruction: without the readfirstlane the value -- and the store
  // descriptor built from it -- would live in VGPRs)
  const int rows = __builtin_amdgcn_readfirstlane(max(0, min(kLdsTH, img.rows_out - y0)));
  const int ybase = __builtin_amdgcn_readfirstlane(min(y0, img.rows_out - 1));
  const ColCtx col = make_col<KIND, NF>(map, min(x, img.W - 1));
  const auto* rowtab = s_row[wave];
  const uint32_t row_bytes_out = (uint32_t)img.W * (uint32_t)ES;
  const char* out_base = (const char*)(dstT + (size_t)ybase * (size_t)img.W);
  const uint32_t xoff = (uint32_t)x * (uint32_t)ES;         // lanes with x >= W: the store is out of range and dropped
  const __amdgpu_buffer_rsrc_t dst =
      __builtin_amdgcn_make_buffer_rsrc((void*)out_base, 0, (int)((uint32_t)rows * row_bytes_out), 0x00020000);

  // ---- phase 1: the source coordinates of the sub-tile's 16 rows, while the loads are in flight.  A box strictly
  // inside the image needs no clip (every coordinate lies inside the box).
  float xf[kLdsTH], yf[kLdsTH];
  const bool box_inside = cx0 - 1 >= 0 && cx1 + 2 <= img.W - 1 && cy0 - 1 >= 0 && cy1 + 2 <= img.H - 1;
  const bool unclipped = box_inside && fits;
  auto rows_1 = [&](auto noclip, auto fastdiv) {
    if constexpr (DCP_WG_FILL_EVERY == 0) {
      issue_fill(std::integral_constant<int, 0>{});
      issue_fill(std::integral_constant<int, 1>{});
      issue_fill(std::integral_constant<int, 2>{});
      issue_fill(std::integral_constant<int, 3>{});
      issue_fill(std::integral_constant<int, 4>{});
      issue_fill(std::integral_constant<int, 5>{});
    }
#pragma unroll
    for (int k = 0; k < kLdsTH; ++k) {
      if constexpr (DCP_WG_FILL_EVERY > 0) {
        if (k == DCP_WG_FILL_START + 0 * DCP_WG_FILL_EVERY) issue_fill(std::integral_constant<int, 0>{});
        if (k == DCP_WG_FILL_START + 1 * DCP_WG_FILL_EVERY) issue_fill(std::integral_constant<int, 1>{});
        if (k == DCP_WG_FILL_START + 2 * DCP_WG_FILL_EVERY) issue_fill(std::integral_constant<int, 2>{});
        if (k == DCP_WG_FILL_START + 3 * DCP_WG_FILL_EVERY) issue_fill(std::integral_constant<int, 3>{});
        if (k == DCP_WG_FILL_START + 4 * DCP_WG_FILL_EVERY) issue_fill(std::integral_constant<int, 4>{});
        if (k == DCP_WG_FILL_START + 5 * DCP_WG_FILL_EVERY) issue_fill(std::integral_constant<int, 5>{});
      }
      double xd, yd;
      map_coord<KIND, NF, RW, decltype(fastdiv)::value>(map, rowtab, s_coef, col, k, wmaxf, hmaxf, &xd, &yd);
      if constexpr (decltype(noclip)::value) {
        xf[k] = (float)xd;
        yf[k] = (float)yd;
      } else {
        xf[k] = round_clip_f32(xd, wmaxf);
        yf[k] = round_clip_f32(yd, hmaxf);
      }
    }
  };
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  if (PLAN && certified) {
    // a whole, unclipped tile (the certificate says so): exact radial factor on the node rows, the cubic through them on the others;
    // the fill's six loads go out in front of the four node rows and the first two interpolated ones
    if constexpr (PLAN) radial_rows_interp<NF>(map, rowtab, col, xf, yf, [&](auto jc) { issue_fill(jc); });
  } else if (rows > 0) {
    if (KIND == kRadial || !map.fast_div) {
      if (unclipped) rows_1(std::true_type{}, I0{});
      else rows_1(std::false_type{}, I0{});
    } else {
      if (unclipped) rows_1(std::true_type{}, I1{});
      else rows_1(std::false_type{}, I1{});
    }
  } else {                                         // nothing to compute for this wave: only its share of the copy
    issue_fill(std::integral_constant<int, 0>{});
    issue_fill(std::integral_constant<int, 1>{});
    issue_fill(std::integral_constant<int, 2>{});
    issue_fill(std::integral_constant<int, 3>{});
    issue_fill(std::integral_constant<int, 4>{});
    issue_fill(std::integral_constant<int, 5>{});
  }
  if (!fits && lane == 0 && wave == 0) atomicAdd(&g_lds_stats[0], 1ull);
  DCP_TRACE(4);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();                                 // every wave's share of the box has landed
  DCP_TRACE(5);

  if (rows == 0 || !(x < img.W)) return;           // no cross-lane work from here on
  if (fits) {
    // ---- phase 2: taps from the shared slab, blend, store
    const uint32_t negorg4 = (uint32_t)(-(by0 * PB + bx0 * ES));
    const char* boxb = (const char*)s_box;
    const bool interior = bx1 < img.W - 1 && by1 < img.H - 1;
    const float negorg4f = (float)(int32_t)negorg4;
    auto tap_addr = [&](int xi, int yi) -> uint32_t {            // yi * pitch + xi * element size + origin, 24-bit multiply
      uint32_t xa, a_;
      if constexpr (ES == 4) asm("v_lshl_add_u32 %0, %1, 2, %2" : "=v"(xa) : "v"(xi), "s"(negorg4));
      else if constexpr (ES == 2) asm("v_lshl_add_u32 %0, %1, 1, %2" : "=v"(xa) : "v"(xi), "s"(negorg4));
      else xa = (uint32_t)xi + negorg4;
      asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(a_) : "v"(yi), "s"(PB), "v"(xa));
      return a_;
    };
    auto tile_rows_loop = [&](auto full, auto inner, auto exact) {
#pragma unroll
      for (int k = 0; k < kLdsTH; ++k) {
        FetchT f;
        uint32_t addr;
        if constexpr (SAMPLER == kNearest) {
          int xi = (int)xf[k];
          int yi = (int)yf[k];
          xi += (xf[k] - (float)xi >= 0.5f) ? 1 : 0;
          yi += (yf[k] - (float)yi >= 0.5f) ? 1 : 0;
          addr = tap_addr(xi, yi);
        } else if constexpr (decltype(inner)::value) {
          f.fx = __builtin_amdgcn_fractf(xf[k]);      // x - floor(x), exact
          f.fy = __builtin_amdgcn_fractf(yf[k]);
          const float flx = xf[k] - f.fx, fly = yf[k] - f.fy;
          const float af = __builtin_fmaf(fly, (float)PB, __builtin_fmaf(flx, (float)ES, negorg4f));
          addr = (uint32_t)(int32_t)af;
        } else {
          const int xi = min((int)xf[k], img.W - 2);
          const int yi = min((int)yf[k], img.H - 2);
          f.fx = xf[k] - (float)xi;
          f.fy = yf[k] - (float)yi;
          addr = tap_addr(xi, yi);
        }
        DCP_BOUNDS(addr, SAMPLER == kNearest ? ES : PB + 2 * ES, kSlabChunks * 16, 2);
        const T* t = (const T*)(boxb + addr);
        if constexpr (kIsF32) {
          float v;
          if constexpr (SAMPLER == kNearest) {
            v = t[0];
          } else {
            f.a.x = __float_as_uint(t[0]);
            f.a.y = __float_as_uint(t[1]);
            f.b.x = __float_as_uint(t[kBoxWEl]);
            f.b.y = __float_as_uint(t[kBoxWEl + 1]);
            v = finish<SAMPLER, true, float, !decltype(inner)::value>(f);
          }
          if (decltype(full)::value || k < rows)
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), dst, xoff, (uint32_t)k * row_bytes_out, DCP_STORE_AUX);
        } else {
          T v;
          if constexpr (SAMPLER == kNearest) {
            v = t[0];
          } else {
            const double fx = (double)f.fx, fy = (double)f.fy;
            double acc;
            if constexpr (decltype(exact)::value) {
              // every coordinate of the tile >= 32: no operation rounds (exact_lerp_pairs), no clamps.  The pairs come as aligned
              // dwords here: four narrow LDS reads (exact_lerp_taps) are 7 % faster in the stack kernel, whose addresses are
              // loop-invariant, and 1.5 % slower in this one (tools/ab_int_exact.py, same box)
              const uint32_t* q = (const uint32_t*)(boxb + (addr & ~3u));
              const uint32_t sh = (addr & 3u) * 8u;
              acc = exact_lerp_pairs<T>(__builtin_amdgcn_alignbit(q[1], q[0], sh), __builtin_amdgcn_alignbit(q[PB / 4 + 1], q[PB / 4], sh), fx, fy);
              v = to_elem_in_range<T>(acc);
            } else {
            // The tap pair (x0, x0 + 1) of a row starts at any multiple of the element size: read the two ALIGNED dwords
            // around it (one ds_read2_b32) and shift the pair down -- a dword read at a 2- or 1-byte boundary works on this
            // hardware but costs 40 us per frame.
            const uint32_t* q = (const uint32_t*)(boxb + (addr & ~3u));
            const uint32_t sh = (addr & 3u) * 8u;
            const uint32_t top = __builtin_amdgcn_alignbit(q[1], q[0], sh), bot = __builtin_amdgcn_alignbit(q[PB / 4 + 1], q[PB / 4], sh);
              // scipy NI_GeometricTransform: w0 = 1 - f, w1 = 1 - w0; ((v*wy)*wx) summed left to right, then its integer store
              const double wy0 = 1.0 - fy, wy1 = 1.0 - wy0;
              const double wx0 = 1.0 - fx, wx1 = 1.0 - wx0;
              auto tap = [](uint32_t w, int i) -> double {            // element i (0 / 1) of the pair, as scipy reads it: a double
                if constexpr (std::is_signed<T>::value) return (double)(int32_t)__builtin_amdgcn_sbfe(w, i * ES * 8, ES * 8);
                else return (double)__builtin_amdgcn_ubfe(w, i * ES * 8, ES * 8);
              };
              acc = (tap(top, 0) * wy0) * wx0;
              acc += (tap(top, 1) * wy0) * wx1;
              acc += (tap(bot, 0) * wy1) * wx0;
              acc += (tap(bot, 1) * wy1) * wx1;
              v = to_elem<T>(acc);
            }
          }
          if (decltype(full)::value || k < rows) {
            if constexpr (ES == 2)
              __builtin_amdgcn_raw_buffer_store_b16((unsigned short)v, dst, xoff, (uint32_t)k * row_bytes_out, DCP_STORE_AUX);
            else
              __builtin_amdgcn_raw_buffer_store_b8((unsigned char)v, dst, xoff, (uint32_t)k * row_bytes_out, DCP_STORE_AUX);
          }
        }
      }
    };
    if constexpr (kIsF32 || SAMPLER == kNearest) {
      if (rows == kLdsTH && interior) tile_rows_loop(std::true_type{}, std::true_type{}, std::false_type{});
      else if (rows == kLdsTH) tile_rows_loop(std::true_type{}, std::false_type{}, std::false_type{});
      else tile_rows_loop(std::false_type{}, std::false_type{}, std::false_type{});
    } else {
      // integer elements, order 1: whole interior tiles whose box lies at coordinates >= 32 take the exact factorised blend
      // (every coordinate of the tile is >= its box origin); the others scipy's operation order
      if (rows == kLdsTH && interior && img.int_exact && bx0 >= (int)kExactLerpMinCoord && by0 >= (int)kExactLerpMinCoord)
        tile_rows_loop(std::true_type{}, std::true_type{}, std::true_type{});
      else tile_rows_loop(std::false_type{}, std::false_type{}, std::false_type{});
    }
    DCP_TRACE(6);
    DCP_TRACE_WAVE_END();
  } else {
    // ---- box too large for the slab: direct global gather
#pragma unroll
    for (int k = 0; k < kLdsTH; ++k) {
      const float xc = __builtin_amdgcn_fmed3f(xf[k], 0.0f, wmaxf), yc = __builtin_amdgcn_fmed3f(yf[k], 0.0f, hmaxf);
      if constexpr (kIsF32) {
        const SrcView src = make_view(img.src, img.src_bytes, img.W, img.H, img.src_stride, 1);
        const FetchT f = fetch<SAMPLER, true, float>(src, xc, yc);
        const float v = finish<SAMPLER, true, float>(f);
        if (k < rows)
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), dst, xoff, (uint32_t)k * row_bytes_out, DCP_STORE_AUX);
      } else {
        T v;
        if constexpr (SAMPLER == kNearest) {
          int xi = (int)xc, yi = (int)yc;
          xi += (xc - (float)xi >= 0.5f) ? 1 : 0;
          yi += (yc - (float)yi >= 0.5f) ? 1 : 0;
          v = srcT[(size_t)yi * (size_t)img.src_stride + (size_t)xi];
        } else {
          const int xi = min((int)xc, img.W - 2), yi = min((int)yc, img.H - 2);
          const double fx = (double)(xc - (float)xi), fy = (double)(yc - (float)yi);
          const T* t = srcT + (size_t)yi * (size_t)img.src_stride + (size_t)xi;
          const double wy0 = 1.0 - fy, wy1 = 1.0 - wy0;
          const double wx0 = 1.0 - fx, wx1 = 1.0 - wx0;
          double acc = ((double)t[0] * wy0) * wx0;
          acc += ((double)t[1] * wy0) * wx1;
          acc += ((double)t[img.src_stride] * wy1) * wx0;
          acc += ((double)t[img.src_stride + 1] * wy1) * wx1;
          v = to_elem<T>(acc);
        }
        if (k < rows) {
          if constexpr (ES == 2)
            __builtin_amdgcn_raw_buffer_store_b16((unsigned short)v, dst, xoff, (uint32_t)k * row_bytes_out, DCP_STORE_AUX);
          else
            __builtin_amdgcn_raw_buffer_store_b8((unsigned char)v, dst, xoff, (uint32_t)k * row_bytes_out, DCP_STORE_AUX);
        }
      }
    }
  }
}

// (runtime-length coefficient vectors -- NF < 0 -- walk the vector in LDS and need more registers than six waves per SIMD leave: at six
// they spilled 116-148 bytes into scratch, and every reload of a spill is a VMEM wait that also waits for the untracked fill;
// tools/isa_hazards.py keeps the shipped instantiations free of scratch)
template <int KIND, int NF, int SAMPLER, typename T = float, bool PLAN = false>
__global__ void __launch_bounds__(256, (NF < 0 ? 4 : (NF == 1 ? 5 : DCP_WG_WAVES))) remap_wg_kernel(const ImageArgs img, const MapArgs map) {
  remap_wg_body<KIND, NF, SAMPLER, T, PLAN>(img, map);
}

// ------------------------------------------------------------------ K1, many frames in one launch

// remap_wg_kernel over a batch of frames of one shape, each with its OWN source, destination, centre and coefficient
// vector: blockIdx.z = frame.  A per-frame launch spends ~3.5 us before its first tile completes and ~9 us draining
// its last workgroups (profiles/rounds_1-4/r02b_phase_timeline_wg_f64lerp.txt: a third of a 4096^2 launch); here the tail of
// frame z runs under the head of frame z + 1.  The per-frame arguments travel in the KERNEL ARGUMENTS (a table of
// BatchEntry<NF>, indexed by the workgroup's frame: scalar loads from the kernarg segment, no device-side table whose
// lifetime would have to outlast the launch), which bounds a launch to BatchTable<NF>::kMax frames; longer batches are
// cut into several launches by the host.  Radial map, float32, certified at level 2 for EVERY frame (the host checks).
template <int NF>
struct BatchEntry {
  const float* src;
  float* dst;
  double xc, yc;
  double fact[NF];
};
template <int NF>
struct BatchTable {
  // kernel arguments are limited to 4 KB: ImageArgs (72 B) + the table
  static constexpr int kMax = (4096 - 128) / (int)sizeof(BatchEntry<NF>) > 64 ? 64 : (4096 - 128) / (int)sizeof(BatchEntry<NF>);
  BatchEntry<NF> e[kMax];
};

template <int NF>
__device__ __forceinline__ void batch_frame_args(const ImageArgs& img0, const BatchTable<NF>& tab, int frame, ImageArgs* img, MapArgs* map) {
  const BatchEntry<NF>& e = tab.e[frame];
  *img = img0;
  img->src = e.src;
  img->dst = e.dst;
  map->xc = e.xc;
  map->yc = e.yc;
#pragma unroll
  for (int i = 0; i < NF; ++i) map->fact[i] = e.fact[i];
  map->nfact = NF;
  map->fast_div = 0;
  map->tile_dev_ok = 2;
}

template <int NF, int SAMPLER>
__global__ void __launch_bounds__(256, DCP_WG_WAVES) remap_wg_batch_kernel(const ImageArgs img0, const BatchTable<NF> tab) {
  ImageArgs img;
  MapArgs map;
  batch_frame_args<NF>(img0, tab, blockIdx.z, &img, &map);
  remap_wg_body<kRadial, NF, SAMPLER, float>(img, map);
}

// The corner hulls of every workgroup tile of every frame of a batch, once per tile (one thread each, the four corners in
// turn) with the code the waves of remap_wg_kernel would otherwise run four times per tile: (x0, x1, y0, y1) of the rounded,
// clipped corner taps.  ~2 us for 24 frames of 4096 tiles; the table lives in stream-ordered scratch of the batch launch.
template <int KIND, int NF>
__device__ __forceinline__ void tile_hull(const ImageArgs& img, const MapArgs& map, int frame, int32_t* boxes) {
  const int ntiles = img.tiles_x * img.tiles_y;
  const int t = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (t >= ntiles) return;
  const int ty = t / img.tiles_x, tx = t - ty * img.tiles_x;
  int x0 = INT32_MAX, x1 = INT32_MIN, y0 = INT32_MAX, y1 = INT32_MIN;
#pragma unroll 1
  for (int c = 0; c < 4; ++c) {
    int cxi, cyi;
    wg_corner_tap<KIND, NF>(img, map, tx, ty * kWgTH, c, &cxi, &cyi);
    x0 = min(x0, cxi);
    x1 = max(x1, cxi);
    y0 = min(y0, cyi);
    y1 = max(y1, cyi);
  }
  int4* const o = (int4*)(boxes + 4 * ((size_t)frame * ntiles + t));
  *o = make_int4(x0, x1, y0, y1);
}

template <int NF>
__global__ void __launch_bounds__(64) box_table_kernel(const ImageArgs img0, const BatchTable<NF> tab, int32_t* boxes) {
  ImageArgs img;
  MapArgs map;
  batch_frame_args<NF>(img0, tab, blockIdx.z, &img, &map);
  tile_hull<kRadial, NF>(img, map, blockIdx.z, boxes);
}

// ------------------------------------------------------------------ K1, frame plans

// The plan of one calibration and frame shape (frame_plan.cpp): workgroups and waves laid out as in remap_wg_body, plain tile order.
// Every wave takes the hull of its workgroup tile exactly as a wave of remap_wg_kernel without a table does (wg_corner_tap) and
// evaluates its 16 coordinate rows twice, with map_coord as phase 1 does and with radial_rows_interp, the function the frame kernel
// calls for a certified tile.  The wave tile's certificate bit is set only if all 2 048 float32 values have the same bit patterns
// AND the tile is one that phase 1 would run unclipped and whole -- the box fits the slab and lies strictly inside the image, 16 rows,
// 64 columns.  Everything else (the frame's border, partial tiles, the tile that holds the centre, where ru has its kink) keeps the
// exact evaluation.  Words [0, 4n): hulls, [4n, 5n): certificate bits (bit w = wave w of the tile).
template <int NF>
__global__ void __launch_bounds__(256) plan_table_kernel(const ImageArgs img, const MapArgs map, int32_t* plan) {
  __shared__ double s_row[4][kLdsTH][2];
  __shared__ int s_ok[4];
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int lane = (int)threadIdx.x & 63;
  const int wx = wave & 1, wy = wave >> 1;
  const int tx = blockIdx.x, ty = blockIdx.y;
  const int yblk = ty * kWgTH;
  const int y0 = yblk + wy * kLdsTH;
  const int x = tx * kWgTW + wx * kLdsTW + lane;
  const float wmaxf = (float)(img.W - 1), hmaxf = (float)(img.H - 1);
  int cxi, cyi;
  wg_corner_tap<kRadial, NF>(img, map, tx, yblk, lane, &cxi, &cyi);
  const int xa = __builtin_amdgcn_readlane(cxi, 0), xb = __builtin_amdgcn_readlane(cxi, 1);
  const int xc_ = __builtin_amdgcn_readlane(cxi, 2), xd_ = __builtin_amdgcn_readlane(cxi, 3);
  const int ya = __builtin_amdgcn_readlane(cyi, 0), yb = __builtin_amdgcn_readlane(cyi, 1);
  const int yc_ = __builtin_amdgcn_readlane(cyi, 2), yd_ = __builtin_amdgcn_readlane(cyi, 3);
  const int cx0 = min(min(xa, xb), min(xc_, xd_)), cx1 = max(max(xa, xb), max(xc_, xd_));
  const int cy0 = min(min(ya, yb), min(yc_, yd_)), cy1 = max(max(ya, yb), max(yc_, yd_));
  // as remap_wg_body<.., float> has them
  const int bx0 = max(min(cx0 - 1, img.W - 2), 0), bx1 = min(cx1 + 2, img.W - 1);
  const int by0 = max(min(cy0 - 1, img.H - 2), 0), by1 = min(cy1 + 2, img.H - 1);
  const bool fits = bx1 - bx0 + 1 <= kWgBoxW && by1 - by0 + 1 <= kWgBoxH;
  const bool box_inside = cx0 - 1 >= 0 && cx1 + 2 <= img.W - 1 && cy0 - 1 >= 0 && cy1 + 2 <= img.H - 1;
  const int rows = max(0, min(kLdsTH, img.rows_out - y0));
  const bool whole = fits && box_inside && rows == kLdsTH && tx * kWgTW + wx * kLdsTW + kLdsTW <= img.W;      // wave-uniform
  int ok = 0;
  if (whole) {
    if (lane < kLdsTH) fill_row<kRadial, 2>(map, s_row[wave], lane, (double)(img.y_origin + min(y0 + lane, img.rows_out - 1)));
    const ColCtx col = make_col<kRadial, NF>(map, min(x, img.W - 1));
    float xi[kLdsTH], yi[kLdsTH];
    radial_rows_interp<NF>(map, s_row[wave], col, xi, yi, [](auto) {});
    bool equal = true;
#pragma unroll
    for (int k = 0; k < kLdsTH; ++k) {
      double xd, yd;
      map_coord<kRadial, NF, 2, 0>(map, s_row[wave], nullptr, col, k, wmaxf, hmaxf, &xd, &yd);
      equal = equal && __float_as_uint((float)xd) == __float_as_uint(xi[k]) && __float_as_uint((float)yd) == __float_as_uint(yi[k]);
    }
    ok = __builtin_amdgcn_ballot_w64(equal) == ~0ull ? 1 : 0;
  }
  if (lane == 0) s_ok[wave] = ok;
  __syncthreads();
  if (threadIdx.x == 0) {
    const size_t ntiles = (size_t)img.tiles_x * img.tiles_y, t = (size_t)ty * img.tiles_x + tx;
    *(int4*)(plan + 4 * t) = make_int4(cx0, cx1, cy0, cy1);
    plan[4 * ntiles + t] = s_ok[0] | (s_ok[1] << 1) | (s_ok[2] << 2) | (s_ok[3] << 3);
  }
}

// ------------------------------------------------------------------ K5: explicit coordinates

template <int SAMPLER, bool PAIR, typename CT>
__global__ void __launch_bounds__(kBlock) remap_coords_kernel(const ImageArgs img, const CoordArgs ca) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= ca.npts) return;
  const SrcView src = make_view(img.src, img.src_bytes, img.W, img.H, img.src_stride, img.src_col_stride);
  CT yc = ((const CT*)ca.ycoord)[i];
  CT xc = ((const CT*)ca.xcoord)[i];
  const CT wmax = (CT)(img.W - 1), hmax = (CT)(img.H - 1);
  if (ca.mode != kModeNearest && (yc < (CT)0 || yc > hmax || xc < (CT)0 || xc > wmax)) {
    // outside the image under a mode other than 'nearest': scipy's coordinate mapping and tap folding, in double and in
    // scipy's operation order whatever the blend (rare points: plain 64-bit addressing)
    const float* base = img.src;
    const int64_t rs = img.src_stride, cs = img.src_col_stride;
    img.dst[i] = (float)mc_sample_outside([&](long long r, long long c) -> double { return (double)base[r * rs + c * cs]; }, img.H, img.W,
                                          (double)yc, (double)xc, SAMPLER == kNearest ? 0 : 1, ca.mode);
    return;
  }
  xc = xc < (CT)0 ? (CT)0 : xc;
  xc = xc > wmax ? wmax : xc;
  yc = yc < (CT)0 ? (CT)0 : yc;
  yc = yc > hmax ? hmax : yc;
  const Fetch<SAMPLER, PAIR, CT> f = fetch<SAMPLER, PAIR, CT>(src, xc, yc);
  img.dst[i] = finish<SAMPLER, PAIR, CT>(f);
}

// ------------------------------------------------------------------ K6: coordinate maps

// The float32 (yd, xd) planes themselves -- _generate_perspective_map (postprocessing.py:444-459)
// and the xd_mat / yd_mat of unwarp_image_backward (:144-145) -- for callers that reuse a map
// (map_index=, cv2.remap).  Same coordinate code as the remap kernels, no sampling.
template <int KIND>
__global__ void __launch_bounds__(kBlock) coord_map_kernel(const ImageArgs img, const MapArgs map, float* ymap,
                                                           float* xmap) {
  __shared__ double s_row[kMaxTileRows][4];
  __shared__ double s_coef[kMaxFact];
  const int ty = blockIdx.x / img.tiles_x;
  const int tx = blockIdx.x - ty * img.tiles_x;
  const int y0 = ty * img.tile_rows;
  const int x = tx * kBlock + (int)threadIdx.x;
  const int rows = min(img.tile_rows, img.H - y0);
  if ((int)threadIdx.x < rows) fill_row<KIND, 4>(map, s_row, threadIdx.x, (double)(y0 + (int)threadIdx.x));
  if constexpr (KIND != kPersp) {
    if ((int)threadIdx.x < map.nfact) s_coef[threadIdx.x] = map.fact[threadIdx.x];
  }
  __syncthreads();
  if (x >= img.W) return;
  const float wmaxf = (float)(img.W - 1), hmaxf = (float)(img.H - 1);
  const ColCtx col = make_col<KIND, -1>(map, x);
  for (int k = 0; k < rows; ++k) {
    double xd, yd;
    map_coord<KIND, -1, 4>(map, s_row, s_coef, col, k, wmaxf, hmaxf, &xd, &yd);
    const size_t o = (size_t)(y0 + k) * (size_t)img.W + (size_t)x;
    ymap[o] = round_clip_f32(yd, hmaxf);
    xmap[o] = round_clip_f32(xd, wmaxf);
  }
}

// ------------------------------------------------------------------ launchers

// Name of the kernel the calling thread launched last (dcp_debug_last_kernel): tests and bench.py use it to state --
// and assert -- which kernel a call really took.  (The longest name is a spline colour call's: a two-kernel prefilter description of
// up to 52 characters, " + " and the gather's 46 -- 101 in all.)  The launchers of every unit write it through set_last_kernel_name
// (those here and in stack_kernels.hip: note_kernel of unwarp_launch.h).
static thread_local char g_last_kernel[192] = "";
const char* last_kernel_name() { return g_last_kernel; }

// Whole-frame launches of the staged kernels.  LaunchOpts::any_order (DCP_MEM_DEVICE_UNORDERED of the C ABI) clears the barrier bit
// of the dispatch packet (hipExtAnyOrderLaunch): the command processor may then start the workgroups of this frame while the last
// workgroups of the previous packet of the SAME stream still run -- the drain of frame z under the ramp of frame z + 1, what
// remap_wg_batch_kernel gets from blockIdx.z, for callers that hand over one frame per call.  Set per launch_image / launch_wg_typed call.
static thread_local int t_any_order = 0;
#include <hip/hip_ext.h>
#define DCP_LAUNCH_FRAME(kernel, grid, block, lds, stream, ...)                                                                  \
  do {                                                                                                                            \
    if (t_any_order) hipExtLaunchKernelGGL(kernel, grid, block, lds, stream, nullptr, nullptr, hipExtAnyOrderLaunch, __VA_ARGS__); \
    else hipLaunchKernelGGL(kernel, grid, block, lds, stream, __VA_ARGS__);                                                       \
  } while (0)
void set_last_kernel_name(const char* name) { snprintf(g_last_kernel, sizeof(g_last_kernel), "%s", name); }

template <int KIND, int NF, int SAMPLER, bool ROUND32, bool PAIR>
static hipError_t launch_one(const ImageArgs& img, const MapArgs& map, hipStream_t stream) {
  const int nb = img.tiles_x * img.tiles_y;
  note_kernel("remap_tile_kernel", KIND, NF, SAMPLER, ROUND32 ? (PAIR ? "" : ",strided") : ",f64coords");
  if constexpr (KIND == kRadial && NF >= 0) {
    // the headline path also exists with 1 and 4 rows in flight (option pipe_depth) for A/B runs
    if (img.pipe_depth == 1) {
      hipLaunchKernelGGL((remap_tile_kernel<KIND, NF, SAMPLER, ROUND32, PAIR, 1>), dim3(nb), dim3(kBlock), 0,
                         stream, img, map);
      return hipGetLastError();
    }
    if (img.pipe_depth >= 4) {
      hipLaunchKernelGGL((remap_tile_kernel<KIND, NF, SAMPLER, ROUND32, PAIR, 4>), dim3(nb), dim3(kBlock), 0,
                         stream, img, map);
      return hipGetLastError();
    }
  }
  hipLaunchKernelGGL((remap_tile_kernel<KIND, NF, SAMPLER, ROUND32, PAIR, kPipeDepth>), dim3(nb), dim3(kBlock),
                     0, stream, img, map);
  return hipGetLastError();
}

// The staged kernel forms LDS addresses in float32: every term must be an integer below 2^24.
static bool lds_addressable(const ImageArgs& img) {
  return (int64_t)img.H * (kWgBoxW * 4) + (int64_t)img.W * 4 + 4 * (int64_t)(kLdsBW * kBoxH * kBoxW * 4) < (1 << 24);
}

template <int KIND, int NF, int SAMPLER, bool VOTE>
static hipError_t launch_lds(const ImageArgs& img_in, const MapArgs& map, hipStream_t stream) {
  ImageArgs img = img_in;
  img.tiles_x = (img.W + kLdsTW - 1) / kLdsTW;
  img.tiles_y = (img.rows_out + kLdsBW * kLdsTH - 1) / (kLdsBW * kLdsTH);
  dim3 grid(img.tiles_x * img.tiles_y);
  if (img.xcd_remap == 2) grid = dim3(8 * ((img.tiles_x + 7) / 8), img.tiles_y);   // see the kernel's tile order
  note_kernel("remap_lds_kernel", KIND, NF, SAMPLER, VOTE ? ",vote" : ",certified");
  DCP_LAUNCH_FRAME((remap_lds_kernel<KIND, NF, SAMPLER, VOTE>), grid, dim3(64 * kLdsBW), 0, stream, img, map);
  return hipGetLastError();
}

// (PlanBuildFn of frame_plan.cpp: img as launch_wg has it -- tiles_x / tiles_y of remap_wg_kernel)
template <int NF>
static hipError_t launch_plan_table(const ImageArgs& img, const MapArgs& map, int32_t* plan, hipStream_t stream) {
  hipLaunchKernelGGL((plan_table_kernel<NF>), dim3(img.tiles_x, img.tiles_y), dim3(256), 0, stream, img, map, plan);
  return hipGetLastError();
}

template <int KIND, int NF, int SAMPLER>
static hipError_t launch_wg(const ImageArgs& img_in, const MapArgs& map, hipStream_t stream) {
  ImageArgs img = img_in;
  const dim3 grid = wg_tile_grid(&img, kWgTW, kWgTH);
  // workgroups per CU capped through unused dynamic LDS (the static 25 608 bytes -- slab, row tables -- allow six): img.wg_per_cu in 1..5.
  // 26 KB stand for the static part, so that static and padding together fit the CU's 160 KB / wg_per_cu: with less set aside
  // wg_per_cu = 1 asks for more LDS than a CU has (the launch is refused) and 2..5 each fit one workgroup fewer than they say.
  unsigned pad = 0;
  if (img.wg_per_cu >= 1 && img.wg_per_cu <= 5) pad = (unsigned)(160 * 1024 / img.wg_per_cu - 26 * 1024) & ~255u;
  note_kernel("remap_wg_kernel", KIND, NF, SAMPLER);
  if constexpr (KIND == kRadial && NF >= 0) {
    // the calibration's frame plan, if it has one by now (frame_plan.cpp): hulls and certificate bits from its table.  While the plan may
    // still be under construction on the device, the launch keeps its barrier bit whatever the caller allows.
    bool ordered = false;
    if (const int32_t* plan = frame_plan_lookup(img, map, stream, &launch_plan_table<NF>, &ordered)) {
      img.boxes = plan;
      if (pad > 32768u) {
        const hipError_t e = hipFuncSetAttribute((const void*)remap_wg_kernel<KIND, NF, SAMPLER, float, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pad);
        if (e != hipSuccess) return e;
      }
      if (ordered) hipLaunchKernelGGL((remap_wg_kernel<KIND, NF, SAMPLER, float, true>), grid, dim3(256), pad, stream, img, map);
      else DCP_LAUNCH_FRAME((remap_wg_kernel<KIND, NF, SAMPLER, float, true>), grid, dim3(256), pad, stream, img, map);
      return hipGetLastError();
    }
  }
  if (pad > 32768u) {        // beyond the 64 KB a launch may ask for by default (static 24.6 KB + the padding)
    const hipError_t e = hipFuncSetAttribute((const void*)remap_wg_kernel<KIND, NF, SAMPLER, float>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pad);
    if (e != hipSuccess) return e;
  }
  DCP_LAUNCH_FRAME((remap_wg_kernel<KIND, NF, SAMPLER>), grid, dim3(256), pad, stream, img, map);
  return hipGetLastError();
}

// Many frames of one shape, each with its own calibration, in as few launches as the 4 KB of kernel arguments allow
// (55 frames of <= 5 coefficients, 35 of <= 10).  Coefficient vectors shorter than the instantiated length are padded with
// zeros: fma(r2, 0, a) = a exactly, so every intermediate of the even / odd Horner chains is unchanged.
static int g_batch_box_table = 1;      // option box_table (A/B switch)
void set_box_table(int v) { g_batch_box_table = v; }
int get_box_table() { return g_batch_box_table; }

template <int NF, int SAMPLER>
static hipError_t launch_wg_batch_t(const ImageArgs& img_in, const BatchFrame* fr, int n, int nfact, hipStream_t stream) {
  using Tab = BatchTable<NF>;
  static_assert(sizeof(ImageArgs) + sizeof(Tab) + 16 <= 4096, "kernel arguments are limited to 4 KB");
  ImageArgs img = img_in;
  dim3 grid = wg_tile_grid(&img, kWgTW, kWgTH);        // (z: the frames of each launch, below)
  note_kernel("remap_wg_batch_kernel", kRadial, NF, SAMPLER);
  for (int f0 = 0; f0 < n; f0 += Tab::kMax) {
    const int m = n - f0 < Tab::kMax ? n - f0 : Tab::kMax;
    Tab tab;
    memset(&tab, 0, sizeof(tab));
    for (int i = 0; i < m; ++i) {
      const BatchFrame& f = fr[f0 + i];
      tab.e[i].src = f.src;
      tab.e[i].dst = f.dst;
      tab.e[i].xc = f.xc;
      tab.e[i].yc = f.yc;
      for (int k = 0; k < nfact; ++k) tab.e[i].fact[k] = f.fact[k];
    }
    grid.z = m;
    // the tiles' corner hulls once per tile instead of in every wave, when there are enough frames to pay for the extra launch
    // (stream-ordered scratch: allocated, written, read and freed in the stream's order; without it the waves evaluate the corners)
    const int ntiles = img.tiles_x * img.tiles_y;
    int32_t* boxes = nullptr;
    if (g_batch_box_table && m >= 4 && hipMallocAsync((void**)&boxes, (size_t)m * ntiles * 16, stream) != hipSuccess) {
      (void)hipGetLastError();
      boxes = nullptr;
    }
    img.boxes = boxes;
    if (boxes) hipLaunchKernelGGL((box_table_kernel<NF>), dim3((ntiles + 63) / 64, 1, m), dim3(64), 0, stream, img, tab, boxes);
    hipLaunchKernelGGL((remap_wg_batch_kernel<NF, SAMPLER>), grid, dim3(256), 0, stream, img, tab);
    const hipError_t e = hipGetLastError();
    if (boxes) (void)hipFreeAsync(boxes, stream);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

template <int NF>
static hipError_t launch_wg_batch_s(const ImageArgs& img, const BatchFrame* fr, int n, int nfact, int sampler, hipStream_t stream) {
  return with_sampler(sampler, [&](auto s) { return launch_wg_batch_t<NF, decltype(s)::value>(img, fr, n, nfact, stream); });
}

hipError_t launch_image_batch(const ImageArgs& img_in, const BatchFrame* frames, int n, int nfact, int sampler, const LaunchOpts& opts,
                              hipStream_t stream, bool* taken) {
  *taken = false;
  ImageArgs img = img_in;
  if (img.rows_out <= 0) {
    img.y_origin = 0;
    img.rows_out = img.H;
  }
  img.xcd_remap = opts.xcd_remap;
  img.wg_box = opts.wg_box;
  img.wg_per_cu = 0;
  // what remap_wg_kernel needs (launch_image / launch_lds_vote): the LDS-staged pair gather with one box per workgroup
  if (n <= 0 || nfact < 0 || nfact > 10 || !opts.wg_box || !opts.lds_gather || opts.coef_lds || opts.xcd_remap == 1 || !pair_gather_ok(img) ||
      !lds_addressable(img))
    return hipSuccess;
  *taken = true;
  if (nfact <= 5) return launch_wg_batch_s<5>(img, frames, n, nfact, sampler, stream);
  return launch_wg_batch_s<10>(img, frames, n, nfact, sampler, stream);
}

// Narrow integer element types on remap_wg_kernel (typed entry points of the C ABI, orders 0 / 1): taken = false when the
// call does not qualify (no level-2 certificate, column-strided or unaligned source, image too wide for float32 LDS
// addresses) and the generic one-thread-per-pixel kernels of typed_kernels.hip must serve it.
template <int KIND, int NF, typename T>
static hipError_t launch_wg_typed_t(const ImageArgs& img_in, const MapArgs& map, int order, hipStream_t stream) {
  ImageArgs img = img_in;
  const dim3 grid = wg_tile_grid(&img, kWgTW, kWgTH);
  if (order == 0) {
    note_kernel("remap_wg_kernel", KIND, NF, kNearest, sizeof(T) == 2 ? ",16-bit" : ",8-bit");
    DCP_LAUNCH_FRAME((remap_wg_kernel<KIND, NF, kNearest, T>), grid, dim3(256), 0, stream, img, map);
  } else {
    note_kernel("remap_wg_kernel", KIND, NF, kScipy, sizeof(T) == 2 ? ",16-bit" : ",8-bit");
    DCP_LAUNCH_FRAME((remap_wg_kernel<KIND, NF, kScipy, T>), grid, dim3(256), 0, stream, img, map);
  }
  return hipGetLastError();
}

template <typename T>
static hipError_t launch_wg_typed_k(MapKind kind, const ImageArgs& img, const MapArgs& map, int order, hipStream_t stream) {
  if (kind == kPersp) return launch_wg_typed_t<kPersp, -1, T>(img, map, order, stream);
  return with_nf_5_4(map, true, [&](auto nf, const MapArgs& m) { return launch_wg_typed_t<kRadial, decltype(nf)::value, T>(img, m, order, stream); });
}

hipError_t launch_wg_typed(MapKind kind, const ImageArgs& img_in, const MapArgs& map, int order, int dtype, const LaunchOpts& opts,
                           hipStream_t stream, bool* taken) {
  *taken = false;
  t_any_order = opts.any_order;
  const int es = elem_size(dtype);
  if ((kind != kRadial && kind != kPersp) || (order != 0 && order != 1) || map.tile_dev_ok < 2 || !opts.wg_box || !opts.lds_gather ||
      opts.xcd_remap != 2 || opts.coef_lds)
    return hipSuccess;
  if (dtype != kU8 && dtype != kI8 && dtype != kU16 && dtype != kI16) return hipSuccess;
  ImageArgs img = img_in;
  if (img.rows_out <= 0) {
    img.y_origin = 0;
    img.rows_out = img.H;
  }
  img.xcd_remap = opts.xcd_remap;       // 2 here (tested above): stripes wherever they balance
  img.int_exact = opts.int_exact;
  // unit column stride, at least 2 x 2, 4-byte aligned rows (the 16-byte LDS-DMA copies), 24-bit products, float32 LDS addresses
  if (!pair_gather_ok(img) || ((uintptr_t)img.src & 3u) || (((int64_t)img.src_stride * es) & 3) || !lds_addressable(img)) return hipSuccess;
  *taken = true;
  switch (dtype) {
    case kU8: return launch_wg_typed_k<uint8_t>(kind, img, map, order, stream);
    case kI8: return launch_wg_typed_k<int8_t>(kind, img, map, order, stream);
    case kU16: return launch_wg_typed_k<uint16_t>(kind, img, map, order, stream);
    default: return launch_wg_typed_k<int16_t>(kind, img, map, order, stream);
  }
}

// VOTE = false needs the host's certificate (MapArgs::tile_dev_ok); without it the runtime-length polynomial
// variant with the per-pixel vote runs (one uncertified instantiation per map kind and sampler instead of eleven).
// The fused map always votes: its inner clip (the perspective position clipped to the frame before the radial model
// is applied) makes the composed map non-smooth, so no curvature bound holds for it.
template <int KIND, int NF, int SAMPLER>
static hipError_t launch_lds_vote(const ImageArgs& img, const MapArgs& map, hipStream_t stream) {
  if constexpr (KIND == kFused) {
    // (round 5) a tame homography in front of a radial model of certified curvature: one box per 128 x 32 workgroup tile from the
    // corners of the tile's perspective bounding box (wg_corner_tap) -- no per-pixel vote.  Anything else votes.
    if constexpr (NF >= 0) {
      if (map.tile_dev_ok >= 2 && img.wg_box && img.xcd_remap != 1) return launch_wg<KIND, NF, SAMPLER>(img, map, stream);
    }
    return launch_lds<KIND, NF, SAMPLER, true>(img, map, stream);
  } else {
    // certificate levels: 2 = holds for 128 x 32 tiles (workgroup-shared box), 1 = for 64 x 16 tiles only
    if (map.tile_dev_ok >= 2 && img.wg_box && img.xcd_remap != 1) return launch_wg<KIND, NF, SAMPLER>(img, map, stream);
    if (map.tile_dev_ok) return launch_lds<KIND, NF, SAMPLER, false>(img, map, stream);
    return launch_lds<KIND, -1, SAMPLER, true>(img, map, stream);
  }
}

template <int KIND, int NF>
static hipError_t launch_lds_any(const ImageArgs& img, const MapArgs& map, int sampler, hipStream_t stream) {
  return with_sampler(sampler, [&](auto s) { return launch_lds_vote<KIND, NF, decltype(s)::value>(img, map, stream); });
}

template <int KIND, int NF>
static hipError_t launch_fast(const ImageArgs& img, const MapArgs& map, int sampler, hipStream_t stream) {
  if (img.lds_gather) return launch_lds_any<KIND, NF>(img, map, sampler, stream);
  return with_sampler(sampler, [&](auto s) { return launch_one<KIND, NF, decltype(s)::value, true, true>(img, map, stream); });
}

template <int KIND, bool ROUND32, bool PAIR>
static hipError_t launch_generic(const ImageArgs& img, const MapArgs& map, int sampler, hipStream_t stream) {
  return with_sampler(sampler, [&](auto s) { return launch_one<KIND, -1, decltype(s)::value, ROUND32, PAIR>(img, map, stream); });
}

hipError_t launch_image(MapKind kind, const ImageArgs& img_in, const MapArgs& map, int sampler, bool round_f32,
                        const LaunchOpts& opts, hipStream_t stream) {
  ImageArgs img = img_in;
  t_any_order = opts.any_order;
  int tr = opts.tile_rows;
  if (tr < 1) tr = 1;
  if (tr > kMaxTileRows) tr = kMaxTileRows;
  img.tile_rows = tr;
  if (img.rows_out <= 0) {          // the whole image
    img.y_origin = 0;
    img.rows_out = img.H;
  }
  img.tiles_x = (img.W + kBlock - 1) / kBlock;
  img.tiles_y = (img.rows_out + tr - 1) / tr;
  img.xcd_remap = opts.xcd_remap;
  img.pipe_depth = opts.pipe_depth;
  img.lds_gather = opts.lds_gather && lds_addressable(img);
  img.wg_box = opts.wg_box;
  img.wg_per_cu = opts.wg_per_cu;
  const bool pair = pair_gather_ok(img);      // else: the strided kernels
  const int nf = map.nfact;

  // order-1 remaps of dense float32 images with float32 coordinates: LDS-staged gather
  const bool lds = pair && round_f32 && img.lds_gather;
  if (kind == kPersp) {
    if (lds) return launch_lds_any<kPersp, -1>(img, map, sampler, stream);
    if (pair) return launch_generic<kPersp, true, true>(img, map, sampler, stream);
    return launch_generic<kPersp, true, false>(img, map, sampler, stream);
  }
  if (kind == kRadial) {
    // a sheared map (the certificate holds, but the boxes of 128 x 32 tiles overflow the slab: a fisheye model far from its
    // centre) on 64 x 32 workgroup tiles under an 80 x 56 box -- color_kernels.hip, one channel -- instead of per-wave boxes
    if (pair && round_f32 && !opts.coef_lds && img.lds_gather && img.wg_box && opts.tall_tiles && map.tile_dev_ok == 1 && map.tall_ok &&
        opts.xcd_remap != 1 && sampler != kF32Lerp) {
      ImageArgs t = img;
      t.tile_rows = 64;
      bool taken = false;
      const hipError_t e = launch_color(kRadial, t, map, 1, kF32, sampler, opts, stream, &taken);
      if (e != hipSuccess || taken) return e;
    }
    if (pair && round_f32 && !opts.coef_lds && img.lds_gather && img.wg_box && opts.tall_tiles == 2 && map.tile_dev_ok >= 2 && opts.xcd_remap != 1 &&
        sampler != kF32Lerp) {        // A/B: the generic interleaved-pixel kernel with one channel on 128 x 16 tiles in remap_wg_kernel's place
      ImageArgs t = img;
      t.tile_rows = 128;
      bool taken = false;
      const hipError_t e = launch_color(kRadial, t, map, 1, kF32, sampler, opts, stream, &taken);
      if (e != hipSuccess || taken) return e;
    }
    if (pair && round_f32 && !opts.coef_lds) {
      switch (nf) {
        case 1: return launch_fast<kRadial, 1>(img, map, sampler, stream);
        case 2: return launch_fast<kRadial, 2>(img, map, sampler, stream);
        case 3: return launch_fast<kRadial, 3>(img, map, sampler, stream);
        case 4: return launch_fast<kRadial, 4>(img, map, sampler, stream);
        case 5: return launch_fast<kRadial, 5>(img, map, sampler, stream);
        case 6: return launch_fast<kRadial, 6>(img, map, sampler, stream);
        case 7: return launch_fast<kRadial, 7>(img, map, sampler, stream);
        case 8: return launch_fast<kRadial, 8>(img, map, sampler, stream);
        case 9: return launch_fast<kRadial, 9>(img, map, sampler, stream);
        case 10: return launch_fast<kRadial, 10>(img, map, sampler, stream);
        default: break;
      }
    }
    if (lds) return launch_lds_any<kRadial, -1>(img, map, sampler, stream);
    if (pair) {
      if (round_f32) return launch_generic<kRadial, true, true>(img, map, sampler, stream);
      return launch_generic<kRadial, false, true>(img, map, sampler, stream);
    }
    if (round_f32) return launch_generic<kRadial, true, false>(img, map, sampler, stream);
    return launch_generic<kRadial, false, false>(img, map, sampler, stream);
  }
  // fused
  if (pair && !opts.coef_lds) {
    switch (nf) {
      case 4: return launch_fast<kFused, 4>(img, map, sampler, stream);
      case 5: return launch_fast<kFused, 5>(img, map, sampler, stream);
      default: break;
    }
  }
  if (lds) return launch_lds_any<kFused, -1>(img, map, sampler, stream);
  if (pair) return launch_generic<kFused, true, true>(img, map, sampler, stream);
  return launch_generic<kFused, true, false>(img, map, sampler, stream);
}

template <int SAMPLER, bool PAIR>
static hipError_t launch_coords_t(const ImageArgs& img, const CoordArgs& ca, hipStream_t stream) {
  const int64_t nb = (ca.npts + kBlock - 1) / kBlock;
  if (nb == 0) return hipSuccess;
  if (ca.is_f64)
    hipLaunchKernelGGL((remap_coords_kernel<SAMPLER, PAIR, double>), dim3((unsigned)nb), dim3(kBlock), 0, stream,
                       img, ca);
  else
    hipLaunchKernelGGL((remap_coords_kernel<SAMPLER, PAIR, float>), dim3((unsigned)nb), dim3(kBlock), 0, stream,
                       img, ca);
  return hipGetLastError();
}

hipError_t launch_coords(const ImageArgs& img, const CoordArgs& ca, int sampler, hipStream_t stream) {
  const bool pair = pair_gather_ok(img);
  return with_sampler(sampler, [&](auto s) {
    constexpr int S = decltype(s)::value;
    return pair ? launch_coords_t<S, true>(img, ca, stream) : launch_coords_t<S, false>(img, ca, stream);
  });
}

hipError_t launch_coord_map(MapKind kind, const ImageArgs& img_in, const MapArgs& map, float* ymap, float* xmap,
                            hipStream_t stream) {
  ImageArgs img = img_in;
  img.tile_rows = 16;
  img.tiles_x = (img.W + kBlock - 1) / kBlock;
  img.tiles_y = (img.H + img.tile_rows - 1) / img.tile_rows;
  const dim3 grid(img.tiles_x * img.tiles_y);
  switch (kind) {
    case kRadial: hipLaunchKernelGGL((coord_map_kernel<kRadial>), grid, dim3(kBlock), 0, stream, img, map, ymap, xmap); break;
    case kPersp: hipLaunchKernelGGL((coord_map_kernel<kPersp>), grid, dim3(kBlock), 0, stream, img, map, ymap, xmap); break;
    default: hipLaunchKernelGGL((coord_map_kernel<kFused>), grid, dim3(kBlock), 0, stream, img, map, ymap, xmap); break;
  }
  return hipGetLastError();
}

DCP_LAB_HOST_DEFINITIONS_UNWARP

DCP_DEFINE_BOUNDS_READER(read_bounds_unwarp)
DCP_DEFINE_LDS_STATS_READER(read_lds_stats_unwarp, g_lds_stats)

}  // namespace dcp
