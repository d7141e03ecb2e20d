// stack_kernels.hip -- hand-written gfx950 (CDNA4 / MI355X) kernels for the stacks of the backward unwarp path of discorpy
// (reference: discorpy/post/postprocessing.py), and their launchers.
//
//   stack_wg_kernel / stack_lds_kernel / stack_rows_kernel   K4  unwarp_slice_backward / unwarp_chunk_slices_backward  :211-229,:281-313
//   stack_centres_kernel        K4 under many centres of distortion in one launch (a grid search over the centre)
//
// The same arithmetic and conventions as the frame kernels of unwarp_kernels.hip (see that file's header and DESIGN.md section 4);
// the sampler, the tile shapes, tile_corner_tap and exact_lerp_pairs come from unwarp_device.h, the launch decisions shared with the
// frame launchers from unwarp_launch.h.  stack_lds_kernel and stack_wg_kernel restate remap_lds_kernel's and remap_wg_kernel's
// staging on purpose: sharing device functions between tuned instantiations moves their register counts.
//
// Build with -ffp-contract=off, as unwarp_kernels.hip.
#include "unwarp_device.h"
#include "unwarp_launch.h"
#include <cstring>

namespace dcp {

// this unit's statistics of the staged path (see DCP_DEFINE_LDS_STATS_READER): [0] box did not fit, [1] containment vote failed
__device__ unsigned long long g_stack_lds_stats[2];

#ifndef DCP_ROWS_NT_STORE
#define DCP_ROWS_NT_STORE 1  // stack_rows_body: nt stores (0: plain, rounds 1-3 -- the 121-centre grid 104 -> 87 us, one sinogram 4.0 -> 3.7)
#endif

// ------------------------------------------------------------------ K4: rows of a (D,H,W) stack

// out[d, r, x] = projection d sampled at the radial source coordinate of (row_start + r, x).
// The coordinate and the tap weights are computed once per (r, x) and reused for d_chunk
// projections; the per-projection work is two 8-byte gathers, the blend and a 4-byte store.
// (body shared by stack_rows_kernel -- one centre, from the kernel arguments -- and stack_centres_kernel -- the centre of
// the workgroup's calibration from a table: xc / yc and the output block of that centre are parameters)
template <int NF, int SAMPLER, bool ROUND32>
__device__ __forceinline__ void stack_rows_body(const StackArgs& st, const MapArgs& map, const double xc_, const double yc_, const int r,
                                                float* __restrict__ out_block) {
  __shared__ double s_coef[kMaxFact];
  if constexpr (NF < 0) {
    if ((int)threadIdx.x < map.nfact) s_coef[threadIdx.x] = map.fact[threadIdx.x];
    __syncthreads();
  }
  const int x = blockIdx.x * kBlock + (int)threadIdx.x;
  const int d0 = blockIdx.z * st.d_chunk;
  const int d1 = min(st.D, d0 + st.d_chunk);
  if (x >= st.W) return;

  const double xu = (double)x - xc_;
  const double yu = (st.row_start + (double)r) - yc_;
  const double r2 = xu * xu + yu * yu;
  const double ru = sqrt_rn(r2);
  double f;
  if constexpr (NF >= 0) {
    double lead_e, lead_o;
    poly_leads<NF>(map.fact, &lead_e, &lead_o);
    f = poly_inline<NF>(map.fact, lead_e, lead_o, r2, ru);
  } else {
    f = poly_lds(s_coef, map.nfact, r2, ru);
  }
  const double xd = __builtin_fma(f, xu, xc_);
  const double yd = __builtin_fma(f, yu, yc_);

  using CT = typename std::conditional<ROUND32, float, double>::type;
  CT xc, yc;
  if constexpr (ROUND32) {
    xc = round_clip_f32(xd, (float)(st.W - 1));
    yc = round_clip_f32(yd, (float)(st.H - 1));
  } else {
    xc = clip_f64(xd, (double)(st.W - 1));
    yc = clip_f64(yd, (double)(st.H - 1));
  }
  if constexpr (ROUND32) {
    if (st.rbh > 0 && (yc < (float)st.rb0 || yc > (float)(st.rb0 + st.rbh - 1))) {
      // a folding model: the row coordinate lies outside the band the reference crops (rows rb0 .. rb0 + rbh - 1); scipy
      // reflects it inside the band (mode='reflect' on the cropped array, postprocessing.py:308-312) -- double arithmetic in
      // scipy's order whatever the blend, 64-bit addressing (rare pixels of a model nobody should use)
      const float yrel = yc - (float)st.rb0;             // float32, exact: the reference subtracts yd_min from the float32 plane
      const float* proj = st.vol + (size_t)d0 * (size_t)st.proj_stride + (size_t)st.rb0 * (size_t)st.row_stride;
      float* o = out_block + ((size_t)d0 * (size_t)st.nrows + (size_t)r) * (size_t)st.W + (size_t)x;
      for (int d = d0; d < d1; ++d) {
        const int64_t rs = st.row_stride;
        *o = (float)mc_sample_outside([&](long long rr, long long cc) -> double { return (double)proj[rr * rs + cc]; }, st.rbh, st.W,
                                      (double)yrel, (double)xc, 1, kModeReflect);
        proj += st.proj_stride;
        o += (size_t)st.nrows * (size_t)st.W;
      }
      return;
    }
  }
  // base tap and fractions once; per projection only the descriptor base moves
  int xi = min((int)xc, st.W - 2), yi = min((int)yc, st.H - 2);
  Fetch<SAMPLER, true, CT> ft;
  ft.fx = xc - (CT)xi;
  ft.fy = yc - (CT)yi;
  const uint32_t off = ((uint32_t)yi * (uint32_t)st.row_stride + (uint32_t)xi) << 2;   // full 32-bit product: a row stride may exceed 2^24
  const int row_bytes = st.row_stride * 4;
  const float* base = st.vol + (size_t)d0 * (size_t)st.proj_stride;
  float* out = out_block + ((size_t)d0 * (size_t)st.nrows + (size_t)r) * (size_t)st.W + (size_t)x;
  const size_t out_step = (size_t)st.nrows * (size_t)st.W;
#pragma unroll 4
  for (int d = d0; d < d1; ++d) {
    const __amdgpu_buffer_rsrc_t rsrc =
        __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, (int)st.proj_bytes, 0x00020000);
    ft.a = __builtin_amdgcn_raw_buffer_load_b64(rsrc, off, 0, 0);
    ft.b = __builtin_amdgcn_raw_buffer_load_b64(rsrc, off, row_bytes, 0);
#if DCP_ROWS_NT_STORE
    __builtin_nontemporal_store(finish<SAMPLER, true, CT>(ft), out);     // (written once, never re-read here)
#else
    *out = finish<SAMPLER, true, CT>(ft);
#endif
    base += st.proj_stride;
    out += out_step;
  }
}

template <int NF, int SAMPLER, bool ROUND32>
__global__ void __launch_bounds__(kBlock) stack_rows_kernel(const StackArgs st, const MapArgs map) {
  stack_rows_body<NF, SAMPLER, ROUND32>(st, map, map.xc, map.yc, (int)blockIdx.y, st.out);
}

// K4 for a grid search over the centre of distortion (examples/example_05.py:62-65 calls unwarp_slice_backward 121 times on
// one stack, each time with another centre): the same rows of the same stack under `ncentres` calibrations that differ in
// (xcenter, ycenter) only, in ONE launch.  blockIdx.y = centre * nrows + row; the centres travel in the kernel arguments
// (scalar loads indexed by the workgroup's centre); out = (ncentres, depth, nrows, width).  The workgroups of one depth chunk
// run back to back over all centres (x fastest, then y), so the two or three source rows every centre needs of each of
// its projections are fetched from HBM once and then served by the L2.
struct CentreTable {
  static constexpr int kMax = 224;                  // 224 x 16 B = 3.5 KB of the 4 KB of kernel arguments
  double xc[kMax], yc[kMax];
};

template <int NF, int SAMPLER, bool ROUND32>
__global__ void __launch_bounds__(kBlock) stack_centres_kernel(const StackArgs st, const MapArgs map, const CentreTable tab, const int k0) {
  const int k = (int)blockIdx.y / st.nrows, r = (int)blockIdx.y - k * st.nrows;
  float* out_block = st.out + (size_t)(k0 + k) * (size_t)st.D * (size_t)st.nrows * (size_t)st.W;
  stack_rows_body<NF, SAMPLER, ROUND32>(st, map, tab.xc[k], tab.yc[k], r, out_block);
}

// K4 with the LDS-staged gather of K1: a wave owns a 64 x 16 tile of (x, row) positions; the coordinates, the
// source box and the per-pixel LDS tap address and fractions are computed ONCE and kept in registers, then for
// each of the d_chunk projections the box is filled by LDS-DMA from that projection and the 1024 pixels are
// blended out of LDS.  Per voxel that leaves two ds_read2, the blend and a store (~15 VALU instructions against
// ~42 for a single frame), and row-contiguous 16-byte fills instead of scattered 8-byte gathers.  A tile whose box
// does not fit the slab, or whose containment vote fails, gathers directly as stack_rows_kernel does.
// float32 coordinates only (unwarp_chunk_slices_backward); the slice path keeps stack_rows_kernel.
template <int NF, int SAMPLER>
__global__ void __launch_bounds__(64 * kLdsBW, (NF < 0 || SAMPLER == kScipy) ? 3 : DCP_LDS_WAVES) stack_lds_kernel(const StackArgs st, const MapArgs map) {
  __shared__ float s_box[kLdsBW][kBoxH * kBoxW];
  __shared__ double s_row[kLdsBW * kLdsTH][2];
  __shared__ double s_coef[NF < 0 ? kMaxFact : 1];
  using FetchT = Fetch<SAMPLER, true, float>;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int lane = (int)threadIdx.x & 63;
  const int rblk = blockIdx.y * (kLdsBW * kLdsTH);
  const int r0 = rblk + wave * kLdsTH;              // first output row (index into the requested rows) of this wave
  const int x = blockIdx.x * kLdsTW + lane;
  const int d0 = blockIdx.z * st.d_chunk, d1 = min(st.D, d0 + st.d_chunk);
  if ((int)threadIdx.x < kLdsBW * kLdsTH)
    fill_row<kRadial, 2>(map, s_row, threadIdx.x, st.row_start + (double)min(rblk + (int)threadIdx.x, st.nrows - 1));
  if constexpr (NF < 0) {
    if ((int)threadIdx.x < map.nfact) s_coef[threadIdx.x] = map.fact[threadIdx.x];
  }
  __syncthreads();
  if (r0 >= st.nrows) return;                       // wave-uniform
  const int rows = min(kLdsTH, st.nrows - r0);
  const float wmaxf = (float)(st.W - 1), hmaxf = (float)(st.H - 1);
  const ColCtx col = make_col<kRadial, NF>(map, min(x, st.W - 1));
  const auto* rowtab = s_row + wave * kLdsTH;

  // ---- coordinates of the tile (once for all projections)
  float xf[kLdsTH], yf[kLdsTH];
#pragma unroll
  for (int k = 0; k < kLdsTH; ++k) {
    double xd, yd;
    map_coord<kRadial, NF, 2>(map, rowtab, s_coef, col, k, wmaxf, hmaxf, &xd, &yd);
    xf[k] = round_clip_f32(xd, wmaxf);
    yf[k] = round_clip_f32(yd, hmaxf);
  }
  // ---- source box: hull of the four corner pixels grown by one pixel, verified for every pixel of the tile
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
  const int bx0 = max(min(cx0 - DCP_LDS_MARGIN, st.W - 2), 0);
  const int bx1 = min(cx1 + 1 + DCP_LDS_MARGIN, st.W - 1);
  const int by0 = max(min(cy0 - DCP_LDS_MARGIN, st.H - 2), 0);
  const int by1 = min(cy1 + 1 + DCP_LDS_MARGIN, st.H - 1);
  const int bw = bx1 - bx0 + 1, bh = by1 - by0 + 1;
  const bool fits = bw <= kBoxW && bh <= kBoxH;
  float xmn = xf[0], xmx = xf[0], ymn = yf[0], ymx = yf[0];
#pragma unroll
  for (int k = 1; k < kLdsTH; ++k) {
    xmn = __builtin_fminf(xmn, xf[k]);
    xmx = __builtin_fmaxf(xmx, xf[k]);
    ymn = __builtin_fminf(ymn, yf[k]);
    ymx = __builtin_fmaxf(ymx, yf[k]);
  }
  const bool inside = xmn >= (float)bx0 && (xmx < (float)bx1 || bx1 == st.W - 1) && ymn >= (float)by0 &&
                      (ymx < (float)by1 || by1 == st.H - 1);
  const bool staged = fits && __builtin_amdgcn_ballot_w64(!inside) == 0;
  if (!staged && lane == 0) atomicAdd(&g_stack_lds_stats[fits ? 1 : 0], 1ull);

  // ---- per-pixel tap address in the slab and fractions (base tap held at x0 <= W-2, y0 <= H-2)
  uint32_t addr[kLdsTH];
  float fx[kLdsTH], fy[kLdsTH];
#pragma unroll
  for (int k = 0; k < kLdsTH; ++k) {
    const int xi = min((int)xf[k], st.W - 2), yi = min((int)yf[k], st.H - 2);
    fx[k] = xf[k] - (float)xi;
    fy[k] = yf[k] - (float)yi;
    // slab byte address when staged, byte offset inside the projection otherwise
    addr[k] = staged ? (uint32_t)(((yi - by0) * kBoxW + (xi - bx0)) * 4) : ((uint32_t)yi * (uint32_t)st.row_stride + (uint32_t)xi) << 2;
  }
  const bool active = x < st.W;
  float* box = s_box[wave];
  const char* boxb = (const char*)box;
  typedef __attribute__((address_space(3))) void* lds_ptr;
  static_assert(kBoxW == 80, "the fill maps 20 lanes of 16 bytes to one slab row");
  const uint32_t org = ((uint32_t)by0 * (uint32_t)st.row_stride + (uint32_t)bx0) * 4u;
  const uint32_t rstep = (uint32_t)st.row_stride * 4u;
  const int lrow = (int)(__umul24((uint32_t)lane, 13u) >> 8);        // lane / 20 for lane < 64
  const int lcol = lane - lrow * 20;
  const uint32_t voff = (uint32_t)lrow * rstep + (uint32_t)lcol * 16u;      // full 32-bit product (rows of 16 MB and more)
  const int row_bytes = st.row_stride * 4;
  const float* base = st.vol + (size_t)d0 * (size_t)st.proj_stride;
  float* out = st.out + ((size_t)d0 * (size_t)st.nrows + (size_t)r0) * (size_t)st.W;
  const size_t out_step = (size_t)st.nrows * (size_t)st.W;
  const uint32_t out_row = (uint32_t)st.W * 4u, xoff = (uint32_t)x * 4u;
  for (int d = d0; d < d1; ++d) {
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, (int)st.proj_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t dst =
        __builtin_amdgcn_make_buffer_rsrc((void*)out, 0, (int)((uint32_t)rows * out_row), 0x00020000);
    if (staged) {
      // the previous projection's taps have been consumed (their values fed the stores): refill the slab
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if (lane < 60) {
#pragma unroll 2
        for (int r = 0; r < bh; r += 3) {
          if (r + lrow < bh)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_ptr)(box + r * kBoxW), 16, voff + (org + (uint32_t)r * rstep), 0,
                                                     0, 0);
        }
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      if (active) {
#pragma unroll
        for (int k = 0; k < kLdsTH; ++k) {
          FetchT f;
          f.fx = fx[k];
          f.fy = fy[k];
          DCP_BOUNDS(addr[k], kBoxW * 4 + 8, kBoxH * kBoxW * 4, 3);
          const float* t = (const float*)(boxb + addr[k]);
          f.a.x = __float_as_uint(t[0]);
          f.a.y = __float_as_uint(t[1]);
          f.b.x = __float_as_uint(t[kBoxW]);
          f.b.y = __float_as_uint(t[kBoxW + 1]);
          const float v = finish<SAMPLER, true, float>(f);
          if (k < rows) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), dst, xoff, (uint32_t)k * out_row, DCP_STORE_AUX);
        }
      }
    } else if (active) {
#pragma unroll
      for (int k = 0; k < kLdsTH; ++k) {
        FetchT f;
        f.fx = fx[k];
        f.fy = fy[k];
        f.a = __builtin_amdgcn_raw_buffer_load_b64(rsrc, addr[k], 0, 0);
        f.b = __builtin_amdgcn_raw_buffer_load_b64(rsrc, addr[k], row_bytes, 0);
        const float v = finish<SAMPLER, true, float>(f);
        if (k < rows) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), dst, xoff, (uint32_t)k * out_row, DCP_STORE_AUX);
      }
    }
    base += st.proj_stride;
    out += out_step;
  }
}

// ------------------------------------------------------------------ K4, workgroup-shared source box

// stack_lds_kernel's scheme with remap_wg_kernel's box: a workgroup owns a 128 x 32 tile of (x, row) positions of the
// requested rows (four waves, 2 x 2 sub-tiles of 64 x 16); corner pixels -> box (certificate level 2), per-pixel slab
// address and fractions ONCE; then for every projection of the depth chunk the four waves copy the box of THAT
// projection into one of two slabs (LDS-DMA, the loads of projection d + 1 issued before projection d is blended, so the
// copy runs under the arithmetic inside the workgroup) and blend their 1024 pixels each out of the other.  One barrier
// per projection.  T as in remap_wg_kernel: float (any blend), an 8- / 16- / 32-bit integer type or double (scipy's blend and its
// store) -- tomography detectors deliver uint16.  float32 coordinates only (unwarp_chunk_slices_backward).
#ifndef DCP_STACK_UNTRACKED_DMA
#define DCP_STACK_UNTRACKED_DMA 1   // 0: the fill through the compiler's LDS-DMA builtin (rounds 2-3; A/B) -- see lds_dma16_untracked
#endif
#ifndef DCP_STACK_UNTRACKED_F32
#define DCP_STACK_UNTRACKED_F32 0   // 1: float32 stacks too (A/B: 1.5 % slower)
#endif
#ifndef DCP_STACK_UNTRACKED_I32
#define DCP_STACK_UNTRACKED_I32 1   // 0: int32 / uint32 stacks through the builtin as float32 ones (A/B)
#endif
#ifndef DCP_STACK_INT_WAVES
#define DCP_STACK_INT_WAVES 4   // waves per SIMD the integer instantiations are allocated for (128 VGPRs; at 5 = 96 VGPRs the projection loop spills: 575 us against 435 per uint16 shard)
#endif
// KIND: the coordinate map.  Only the prologue (corner hull, row table, column context, the sixteen coordinates) depends on it; kPersp /
// kFused: whole frames (row_start = 0, nrows = H) under a tame homography (MapArgs::fast_div = 1: launch_stack_wg_frames declines the
// others), the float32 coordinates those of remap_wg_kernel bit for bit.
template <int KIND, int NF, int SAMPLER, typename T = float>
__global__ void __launch_bounds__(256, (sizeof(T) >= 4 ? 3 : DCP_STACK_INT_WAVES)) stack_wg_kernel(const StackArgs st, const MapArgs map) {
  constexpr bool kIsF32 = std::is_same<T, float>::value;
  constexpr int ES = (int)sizeof(T);
  constexpr int CH = ES == 8 ? 72 : ES == 4 ? 36 : (ES == 2 ? 20 : 10);
  constexpr int PB = CH * 16;
  constexpr int kBoxWEl = PB / ES;
  constexpr int NJ = (kWgBoxH * CH + 255) / 256;
  // float64: ONE slab of 48 KB (two would leave a CU a single workgroup) -- fill, wait, blend, the other two workgroups of the CU
  // covering the wait
  constexpr int NSLAB = ES == 8 ? 1 : 2;
  constexpr int kAlignEl = ES >= 4 ? 1 : 4 / ES;               // the box's first column: a dword-aligned byte offset
  static_assert(kIsF32 || SAMPLER == kScipy, "integer and float64 element types blend in scipy's exact order");
  __shared__ __attribute__((aligned(16))) unsigned char s_box[NSLAB][kWgSlabRows * PB];
  constexpr int RW = KIND == kRadial ? 2 : 4;
  __shared__ double s_row[4][kLdsTH][RW];
  __shared__ double s_coef[NF < 0 ? kMaxFact : 1];
  using FetchT = Fetch<SAMPLER, true, float>;

  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int lane = (int)threadIdx.x & 63;
  const int wx = wave & 1, wy = wave >> 1;
  // ---- which (tile column, tile row, depth chunk) this workgroup owns.  The dispatcher deals workgroups to the eight XCDs round robin
  // by their linear id (see logical_tile): in grid order the tiles left and right of this one stream THEIR boxes -- which share the
  // lines at this box's edges and, above and below, whole rows -- through other L2s.  xcd_order 1: XCD k takes the k-th eighth of the
  // (x fastest, then rows, then depth chunks) enumeration, so that the ~100 workgroups an XCD holds at a time are neighbouring tiles
  // of one depth chunk and walk its projections together; 2: whole tile rows (wg_stack_xcd_order has the measurements)
  int tile_x = (int)blockIdx.x, tile_y = (int)blockIdx.y, tile_z = (int)blockIdx.z;
  if (st.xcd_order) {
    const uint32_t gx = gridDim.x, gxy = gx * gridDim.y, n = gxy * gridDim.z;
    const uint32_t b = blockIdx.x + gx * blockIdx.y + gxy * blockIdx.z;
    const uint32_t xcd = b & 7u;
    if (st.xcd_order == 2) {
      // XCD k takes the tile rows k, k + 8, ... of every depth chunk (gridDim.y is the number of tile rows rounded up to a multiple of
      // eight: the workgroups of the rows that do not exist leave).  Left and right neighbours share an L2, the eight XCDs stay
      // inside one band of rows of one depth chunk as in grid order
      const uint32_t l = b - gxy * blockIdx.z, j = l >> 3, q = j / gx;
      tile_y = (int)(q * 8u + xcd);
      tile_x = (int)(j - q * gx);
      if (tile_y * kWgTH >= st.nrows) return;
    } else {
      uint32_t lin = xcd * (n >> 3) + min(xcd, n & 7u) + (b >> 3);
      tile_z = (int)(lin / gxy);
      lin -= (uint32_t)tile_z * gxy;
      tile_y = (int)(lin / gx);
      tile_x = (int)(lin - (uint32_t)tile_y * gx);
    }
  }
  tile_x = __builtin_amdgcn_readfirstlane(tile_x);
  tile_y = __builtin_amdgcn_readfirstlane(tile_y);
  tile_z = __builtin_amdgcn_readfirstlane(tile_z);
  const int rblk = tile_y * kWgTH;
  const int r0 = __builtin_amdgcn_readfirstlane(rblk + wy * kLdsTH);   // first requested row of this wave's sub-tile
  const int x = tile_x * kWgTW + wx * kLdsTW + lane;
  const int d0 = tile_z * st.d_chunk, d1 = min(st.D, d0 + st.d_chunk);
  const float wmaxf = (float)(st.W - 1), hmaxf = (float)(st.H - 1);
  const T* const volT = (const T*)st.vol;
  T* const outT = (T*)st.out;

  // ---- the tile's four corner pixels (lanes 0..3, every wave for itself) -> box (a homography / the fused map: remap_wg_kernel's rule)
  int cx0, cx1, cy0, cy1;
  {
    const double X = (double)min(tile_x * kWgTW + (lane & 1) * (kWgTW - 1), st.W - 1);
    const double Y = st.row_start + (double)min(rblk + ((lane >> 1) & 1) * (kWgTH - 1), st.nrows - 1);
    int cxi, cyi;
    if constexpr (KIND == kRadial) {
      const double xu = X - map.xc, yu = Y - map.yc;
      const double r2 = xu * xu + yu * yu;
      const double ru = sqrt_rn(r2);
      double f;
      if constexpr (NF >= 0) {
        double le, lo;
        poly_leads<NF>(map.fact, &le, &lo);
        f = poly_inline<NF>(map.fact, le, lo, r2, ru);
      } else {
        f = poly_lds(map.fact, map.nfact, r2, ru);
      }
      cxi = (int)round_clip_f32(__builtin_fma(f, xu, map.xc), wmaxf);
      cyi = (int)round_clip_f32(__builtin_fma(f, yu, map.yc), hmaxf);
    } else {
      tile_corner_tap<KIND, NF>(map, wmaxf, hmaxf, X, Y, lane, &cxi, &cyi);
    }
    const int xa = __builtin_amdgcn_readlane(cxi, 0), xb = __builtin_amdgcn_readlane(cxi, 1);
    const int xc_ = __builtin_amdgcn_readlane(cxi, 2), xd_ = __builtin_amdgcn_readlane(cxi, 3);
    const int ya = __builtin_amdgcn_readlane(cyi, 0), yb = __builtin_amdgcn_readlane(cyi, 1);
    const int yc_ = __builtin_amdgcn_readlane(cyi, 2), yd_ = __builtin_amdgcn_readlane(cyi, 3);
    cx0 = min(min(xa, xb), min(xc_, xd_));
    cx1 = max(max(xa, xb), max(xc_, xd_));
    cy0 = min(min(ya, yb), min(yc_, yd_));
    cy1 = max(max(ya, yb), max(yc_, yd_));
  }
  const int bx0 = max(min(cx0 - 1, st.W - 2), 0) & ~(kAlignEl - 1);
  const int bx1 = min(cx1 + 2, st.W - 1);
  const int by0 = max(min(cy0 - 1, st.H - 2), 0);
  const int by1 = min(cy1 + 2, st.H - 1);
  const int bw = bx1 - bx0 + 1, bh = by1 - by0 + 1;
  const bool fits = bw <= kBoxWEl && bh <= kWgBoxH;          // workgroup-uniform
  if (!fits && lane == 0 && wave == 0) atomicAdd(&g_stack_lds_stats[0], 1ull);
  // integer elements: the tile's coordinates are all >= its box origin; at >= 32 the factorised blend is exact (exact_lerp_pairs)
  // (32-bit integers: the products of the factorised blend do not fit a float64 exactly -- scipy's order, as for float32)
  const bool exact = !kIsF32 && ES < 4 && SAMPLER != kNearest && fits && st.int_exact && bx0 >= (int)kExactLerpMinCoord && by0 >= (int)kExactLerpMinCoord;

  // ---- coordinates of this wave's 16 rows, once for all projections: slab address (or byte offset inside a projection
  // when the box does not fit) and fractions
  if (lane < kLdsTH) fill_row<KIND, RW>(map, s_row[wave], lane, st.row_start + (double)min(r0 + lane, st.nrows - 1));
  if constexpr (NF < 0 && KIND != kPersp) {
    if ((int)threadIdx.x < map.nfact) s_coef[threadIdx.x] = map.fact[threadIdx.x];
    __syncthreads();
  }
  const int rows = __builtin_amdgcn_readfirstlane(max(0, min(kLdsTH, st.nrows - r0)));
  const ColCtx col = make_col<KIND, NF>(map, min(x, st.W - 1));
  uint32_t addr[kLdsTH];
  // the two float32 fractions per pixel stay in registers for all projections.  (Integer element types: round 2 kept scipy's four
  // float64 weights instead -- 128 of 168 VGPRs, three waves per SIMD and spills; the conversions back to float64 cost two
  // instructions per voxel and buy five waves per SIMD.)
  float fx[kLdsTH], fy[kLdsTH];
  const uint32_t negorg = (uint32_t)(-(by0 * PB + bx0 * ES));
#pragma unroll
  for (int k = 0; k < kLdsTH; ++k) {
    double xd, yd;
    // (a homography: the launcher takes tame ones only, MapArgs::fast_div = 1 -- the division remap_wg_kernel then uses, fixed here at
    // compile time; an untame one goes frame by frame)
    map_coord<KIND, NF, RW, (KIND == kRadial ? -1 : 1)>(map, s_row[wave], s_coef, col, k, wmaxf, hmaxf, &xd, &yd);
    const float xc = round_clip_f32(xd, wmaxf), yc = round_clip_f32(yd, hmaxf);
    int xi, yi;
    if constexpr (SAMPLER == kNearest) {
      xi = (int)xc;
      yi = (int)yc;
      xi += (xc - (float)xi >= 0.5f) ? 1 : 0;
      yi += (yc - (float)yi >= 0.5f) ? 1 : 0;
      fx[k] = fy[k] = 0.0f;
    } else {
      xi = min((int)xc, st.W - 2);
      yi = min((int)yc, st.H - 2);
      fx[k] = xc - (float)xi;
      fy[k] = yc - (float)yi;
    }
    addr[k] = fits ? (uint32_t)yi * (uint32_t)PB + (uint32_t)xi * (uint32_t)ES + negorg
                   : ((uint32_t)yi * (uint32_t)st.row_stride + (uint32_t)xi) * (uint32_t)ES;
  }

  // ---- the fill of one projection: this wave's chunks (see remap_wg_kernel)
  typedef __attribute__((address_space(3))) void* lds_ptr;
  const uint32_t rstep = (uint32_t)st.row_stride * (uint32_t)ES;
  const int fc = wave * 64 + lane;
  const int crow0 = fc / CH;
  const int c160 = fc - crow0 * CH;
  const uint32_t off0 = ((uint32_t)by0 * (uint32_t)st.row_stride + (uint32_t)bx0) * (uint32_t)ES + (uint32_t)crow0 * rstep + (uint32_t)c160 * 16u;
  const int nchunk = bh * CH;
  // lds_dma16_untracked: seen by the compiler, the stream of projection d + 1 is waited for before the blend of projection d.  Integer
  // stacks (bound by that chain's latency) gain 3-9 % without the wait; float32 stacks (at the rate the box copies memory at) lose 1 %:
  // they keep the builtin
  // (one slab -- float64: the wait behind the fill is for everything, the builtin says so to the compiler)
  constexpr bool kUntrackedFill = DCP_STACK_UNTRACKED_DMA && NSLAB == 2 && ((!kIsF32 && (ES < 4 || DCP_STACK_UNTRACKED_I32)) || DCP_STACK_UNTRACKED_F32);
  [[maybe_unused]] const uint32_t slab0 = (uint32_t)(uintptr_t)(lds_ptr)&s_box[0][0];
  auto fill = [&](const T* proj, int slab) {
    [[maybe_unused]] const dcp_rsrc_words rs = raw_rsrc_words(proj, st.proj_bytes);
    [[maybe_unused]] const __amdgpu_buffer_rsrc_t rs_seen = __builtin_amdgcn_make_buffer_rsrc((void*)proj, 0, (int)st.proj_bytes, 0x00020000);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      if ((j * 4 + wave) * 64 < nchunk) {
        const int qrow = (256 * j) / CH, rem = (256 * j) % CH;
        const bool wrap = c160 >= CH - rem;
        const int crow = crow0 + qrow + (wrap ? 1 : 0);
        const uint32_t voff = off0 + (wrap ? rstep - (uint32_t)PB : 0u) + (uint32_t)qrow * rstep + (uint32_t)rem * 16u;
        if (crow < bh) {
          if constexpr (kUntrackedFill) lds_dma16_untracked(rs, slab0 + (uint32_t)(slab * (kWgSlabRows * PB) + (j * 4 + wave) * 1024), voff);
          else __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_seen, (lds_ptr)(s_box[slab] + (j * 4 + wave) * 1024), 16, voff, 0, 0, 0);
        }
      }
    }
  };

  const bool active = x < st.W && rows > 0;
  const uint32_t out_row = (uint32_t)st.W * (uint32_t)ES, xoff = (uint32_t)x * (uint32_t)ES;
  const T* proj = volT + (size_t)d0 * (size_t)st.proj_stride;
  T* out = outT + ((size_t)d0 * (size_t)st.nrows + (size_t)min(r0, st.nrows - 1)) * (size_t)st.W;
  const size_t out_step = (size_t)st.nrows * (size_t)st.W;
  // (bounds-checking build: the vector-memory instructions this lane's wave has issued since its share of the last fill -- the lazy
  // wait below is right only if there were at least kLdsTH of them)
  DCP_VM_COUNTER(vm_since_fill);
  auto blend_store = [&](const T* t_lo, const T* t_hi, const __amdgpu_buffer_rsrc_t& dst, int k) {
    // t_lo / t_hi: the tap pairs of the two rows (LDS or global); a_: the byte address (for the aligned-dword extraction)
    if constexpr (kIsF32) {
      FetchT f;
      f.fx = fx[k];
      f.fy = fy[k];
      // (scipy's order needs four float64 weights per pixel: hoisted out of the projection loop they are 128 registers and the
      // kernel spills -- the empty asm keeps their computation inside the loop)
      if constexpr (SAMPLER == kScipy) asm volatile("" : "+v"(f.fx), "+v"(f.fy));
      f.a.x = __float_as_uint(t_lo[0]);
      if constexpr (SAMPLER != kNearest) {
        f.a.y = __float_as_uint(t_lo[1]);
        f.b.x = __float_as_uint(t_hi[0]);
        f.b.y = __float_as_uint(t_hi[1]);
      }
      const float v = finish<SAMPLER, true, float>(f);
      if (k < rows) {
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), dst, xoff, (uint32_t)k * out_row, DCP_STORE_AUX);
        DCP_VM_ISSUED(vm_since_fill);
      }
    } else {
      // scipy NI_GeometricTransform: w0 = 1 - f, w1 = 1 - w0 (not f itself where 1 - f rounds); ((v * wy) * wx) summed left to right
      // (the empty asm keeps the conversions and the weights inside the projection loop: hoisted, they are 128 registers again)
      float fy_ = fy[k], fx_ = fx[k];
      asm volatile("" : "+v"(fy_), "+v"(fx_));
      const double wy0_ = 1.0 - (double)fy_, wy1_ = 1.0 - wy0_, wx0_ = 1.0 - (double)fx_, wx1_ = 1.0 - wx0_;
      double acc = ((double)t_lo[0] * wy0_) * wx0_;
      acc += ((double)t_lo[1] * wy0_) * wx1_;
      acc += ((double)t_hi[0] * wy1_) * wx0_;
      acc += ((double)t_hi[1] * wy1_) * wx1_;
      const T v = to_elem<T>(acc);
      if (k < rows) {
        DCP_VM_ISSUED(vm_since_fill);
        if constexpr (ES == 8) {
          typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));
          const unsigned long long b = (unsigned long long)__double_as_longlong((double)v);
          const u32x2_t pk = {(uint32_t)b, (uint32_t)(b >> 32)};
          __builtin_amdgcn_raw_buffer_store_b64(pk, dst, xoff, (uint32_t)k * out_row, DCP_STORE_AUX);
        } else if constexpr (ES == 4) __builtin_amdgcn_raw_buffer_store_b32((uint32_t)v, dst, xoff, (uint32_t)k * out_row, DCP_STORE_AUX);
        else if constexpr (ES == 2) __builtin_amdgcn_raw_buffer_store_b16((unsigned short)v, dst, xoff, (uint32_t)k * out_row, DCP_STORE_AUX);
        else __builtin_amdgcn_raw_buffer_store_b8((unsigned char)v, dst, xoff, (uint32_t)k * out_row, DCP_STORE_AUX);
      }
    }
  };

  static_assert(kLdsTH == 16, "the partial wait below counts the stores of one projection");
  const bool lazy_wait = kUntrackedFill && st.store_wait && rows == kLdsTH && __builtin_amdgcn_readfirstlane((int)(__ballot(active) != 0ull));
  if (fits) {
    if constexpr (NSLAB == 2) fill(proj, 0);
    for (int d = d0; d < d1; ++d) {
      const int cur = NSLAB == 2 ? ((d - d0) & 1) : 0;
      if constexpr (NSLAB == 1) {
        __syncthreads();                                    // everyone is done with the slab's previous projection
        fill(proj, 0);
      }
      // this wave's share of projection d.  Vector memory operations of a wave complete in issue order (one counter for loads and stores
      // on gfx9-class hardware), and what the wave issued AFTER that share are the stores of projection d - 1: exactly kLdsTH of them
      // when the wave has all its rows and a lane inside the image -- then "at most kLdsTH outstanding" means the fill has landed and
      // the stores stay in flight under the barrier, the next fill and the blend (waiting for them too cost a write round trip per
      // projection).  Fewer stores than that (ragged waves): wait for everything
      if (lazy_wait && d > d0) {
        DCP_VM_CHECK(active, vm_since_fill, kLdsTH);                                     // (checking build only)
        asm volatile("s_waitcnt vmcnt(16)" ::: "memory");        // (d0: no stores behind the first fill yet)
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      __syncthreads();                                      // everyone's share has landed; everyone is done with the other slab
      if constexpr (NSLAB == 2) {
        if (d + 1 < d1) fill(proj + st.proj_stride, cur ^ 1); // projection d + 1 streams in under the blend of d
        DCP_VM_RESET(vm_since_fill);
      }
      if (active) {
        const __amdgpu_buffer_rsrc_t dst = __builtin_amdgcn_make_buffer_rsrc((void*)out, 0, (int)((uint32_t)rows * out_row), 0x00020000);
        const char* boxb = (const char*)s_box[cur];
        // (the pointers advance below, in uniform control flow: advanced inside this per-lane branch they -- and the store descriptor built
        // from them -- become per-lane values and every store a waterfall loop)
        [[maybe_unused]] bool done = false;
        if constexpr (!kIsF32 && ES < 4) {
          if (exact) {
            // every coordinate of the tile >= 32: the factorised blend is exact (exact_lerp_pairs) and scipy's w1 = 1 - (1 - f) IS the fraction
#pragma unroll
            for (int k = 0; k < kLdsTH; ++k) {
              DCP_BOUNDS(addr[k], PB + 2 * ES, kWgSlabRows * PB, 4);
              const T* t = (const T*)(boxb + addr[k]);
              float fy_ = fy[k], fx_ = fx[k];
              asm volatile("" : "+v"(fy_), "+v"(fx_));            // (see blend_store)
              const T v = to_elem_in_range<T>(exact_lerp_taps<T>(t, t + kBoxWEl, (double)fx_, (double)fy_));
              if (k < rows) {
                DCP_VM_ISSUED(vm_since_fill);
                if constexpr (ES == 2) __builtin_amdgcn_raw_buffer_store_b16((unsigned short)v, dst, xoff, (uint32_t)k * out_row, DCP_STORE_AUX);
                else __builtin_amdgcn_raw_buffer_store_b8((unsigned char)v, dst, xoff, (uint32_t)k * out_row, DCP_STORE_AUX);
              }
            }
            done = true;
          }
        }
        if (!done) {
#pragma unroll
        for (int k = 0; k < kLdsTH; ++k) {
          DCP_BOUNDS(addr[k], PB + 2 * ES, kWgSlabRows * PB, 5);
          if constexpr (ES >= 4) {                          // float32, int32, uint32, float64: the taps are aligned elements
            const T* t = (const T*)(boxb + addr[k]);
            blend_store(t, t + kBoxWEl, dst, k);
          } else {
            // tap pairs as the two aligned dwords around them, shifted down (see remap_wg_kernel)
            const uint32_t* q = (const uint32_t*)(boxb + (addr[k] & ~3u));
            const uint32_t sh = (addr[k] & 3u) * 8u;
            const uint32_t top = __builtin_amdgcn_alignbit(q[1], q[0], sh), bot = __builtin_amdgcn_alignbit(q[PB / 4 + 1], q[PB / 4], sh);
            T lo[2], hi[2];
            if constexpr (std::is_signed<T>::value) {
              lo[0] = (T)__builtin_amdgcn_sbfe(top, 0, ES * 8); lo[1] = (T)__builtin_amdgcn_sbfe(top, ES * 8, ES * 8);
              hi[0] = (T)__builtin_amdgcn_sbfe(bot, 0, ES * 8); hi[1] = (T)__builtin_amdgcn_sbfe(bot, ES * 8, ES * 8);
            } else {
              lo[0] = (T)__builtin_amdgcn_ubfe(top, 0, ES * 8); lo[1] = (T)__builtin_amdgcn_ubfe(top, ES * 8, ES * 8);
              hi[0] = (T)__builtin_amdgcn_ubfe(bot, 0, ES * 8); hi[1] = (T)__builtin_amdgcn_ubfe(bot, ES * 8, ES * 8);
            }
            blend_store(lo, hi, dst, k);
          }
        }
        }
      }
      proj += st.proj_stride;
      out += out_step;
    }
  } else if (active) {
    // ---- box too large for the slab: direct global gather, projection by projection
    for (int d = d0; d < d1; ++d) {
      const __amdgpu_buffer_rsrc_t dst = __builtin_amdgcn_make_buffer_rsrc((void*)out, 0, (int)((uint32_t)rows * out_row), 0x00020000);
#pragma unroll
      for (int k = 0; k < kLdsTH; ++k) {
        const T* t = (const T*)((const char*)proj + addr[k]);
        blend_store(t, t + st.row_stride, dst, k);
      }
      proj += st.proj_stride;
      out += out_step;
    }
  }
}

// ------------------------------------------------------------------ launchers

template <int NF, bool ROUND32>
static hipError_t launch_stack_t(const StackArgs& st, const MapArgs& map, int sampler, hipStream_t stream) {
  note_kernel("stack_rows_kernel", -1, NF, sampler, ROUND32 ? "" : ",f64coords");
  const dim3 grid((st.W + kBlock - 1) / kBlock, st.nrows, (st.D + st.d_chunk - 1) / st.d_chunk);
  with_blend(sampler, [&](auto s) { hipLaunchKernelGGL((stack_rows_kernel<NF, decltype(s)::value, ROUND32>), grid, dim3(kBlock), 0, stream, st, map); });
  return hipGetLastError();
}

template <int NF, bool ROUND32>
static hipError_t launch_centres_t(const StackArgs& st, const MapArgs& map, const double* xcs, const double* ycs, int ncentres, int sampler,
                                   hipStream_t stream) {
  static_assert(sizeof(StackArgs) + sizeof(MapArgs) + sizeof(CentreTable) + 16 <= 4096, "kernel arguments are limited to 4 KB");
  note_kernel("stack_centres_kernel", -1, NF, sampler, ROUND32 ? "" : ",f64coords");
  // blockIdx.y = centre * nrows + row stays below 65536
  const int per_launch = st.nrows >= 65535 ? 1 : (65535 / st.nrows < CentreTable::kMax ? 65535 / st.nrows : CentreTable::kMax);
  for (int k0 = 0; k0 < ncentres; k0 += per_launch) {
    const int m = ncentres - k0 < per_launch ? ncentres - k0 : per_launch;
    CentreTable tab;
    memset(&tab, 0, sizeof(tab));
    for (int i = 0; i < m; ++i) {
      tab.xc[i] = xcs[k0 + i];
      tab.yc[i] = ycs[k0 + i];
    }
    const dim3 grid((st.W + kBlock - 1) / kBlock, (unsigned)(m * st.nrows), (st.D + st.d_chunk - 1) / st.d_chunk);
    with_blend(sampler, [&](auto s) {
      hipLaunchKernelGGL((stack_centres_kernel<NF, decltype(s)::value, ROUND32>), grid, dim3(kBlock), 0, stream, st, map, tab, k0);
    });
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_stack_centres(const StackArgs& st_in, const MapArgs& map, const double* xcs, const double* ycs, int ncentres, int sampler,
                                bool round_f32, const LaunchOpts& opts, hipStream_t stream) {
  StackArgs st = st_in;
  if (st.D == 0 || st.nrows == 0 || ncentres == 0) return hipSuccess;
  // one thread keeps its coordinate for d_chunk projections; with many centres the launch is large whatever the chunk
  st.d_chunk = opts.d_chunk < 1 ? 1 : opts.d_chunk;
  while (st.d_chunk < 64 && (int64_t)((st.W + kBlock - 1) / kBlock) * st.nrows * ncentres * ((st.D + 2 * st.d_chunk - 1) / (2 * st.d_chunk)) >= 4096)
    st.d_chunk *= 2;
  if ((st.D + st.d_chunk - 1) / st.d_chunk > 65535) st.d_chunk = (st.D + 65534) / 65535;
  return with_nf_5_4(map, !opts.coef_lds, [&](auto nf, const MapArgs& m) {
    constexpr int NF = decltype(nf)::value;
    return round_f32 ? launch_centres_t<NF, true>(st, m, xcs, ycs, ncentres, sampler, stream)
                     : launch_centres_t<NF, false>(st, m, xcs, ycs, ncentres, sampler, stream);
  });
}

template <int NF>
static hipError_t launch_stack_lds(const StackArgs& st, const MapArgs& map, int sampler, hipStream_t stream) {
  note_kernel("stack_lds_kernel", -1, NF, sampler);
  const dim3 grid((unsigned)((st.W + kLdsTW - 1) / kLdsTW), (unsigned)((st.nrows + kLdsBW * kLdsTH - 1) / (kLdsBW * kLdsTH)),
                  (unsigned)((st.D + st.d_chunk - 1) / st.d_chunk));
  const dim3 block(64 * kLdsBW);
  with_blend(sampler, [&](auto s) { hipLaunchKernelGGL((stack_lds_kernel<NF, decltype(s)::value>), grid, block, 0, stream, st, map); });
  return hipGetLastError();
}

// Depth chunk for stack_wg_kernel: a workgroup streams its projections through two slabs, so it wants several of
// them, and the launch wants a few thousand workgroups (three fit a CU).  0: too little work even at 4 per workgroup.
static int wg_stack_chunk(const StackArgs& st, int d_chunk, bool force = false) {
  const int64_t tiles = (int64_t)tiles_of(st.W, kWgTW) * tiles_of(st.nrows, kWgTH);
  int dc = d_chunk < 4 ? 4 : d_chunk;
  auto wgs = [&](int c) { return tiles * ((st.D + c - 1) / c); };
  while (dc > 4 && wgs(dc) < 3072) dc >>= 1;
  if (dc < 4) dc = 4;
  if ((wgs(dc) < 1024 && !force) || (st.D + dc - 1) / dc > 65535) return 0;
  return dc;
}

// stack_wg_kernel's tile order: 0 grid order, 1 XCD runs, 2 XCD tile rows (see the kernel).  Measured (tools/ab_stack_order.py,
// tools/pmc_stack_order.sh; cfg4 shards of 64 / 256 / 1024 projections, 2560^2): the L2s fetch 1.50 x the algorithmic reads of a
// float32 shard in grid order, 1.10 x by tile rows (what is left is the four rows two vertical neighbours share), 1.07 x by runs;
// uint16: 1.95 / 1.09 / 0.99.  The kernel is not bound by those fetches, so time moves little: float32 by rows 0-1 % faster than grid
// order in every process tried, by runs anywhere between 11 % faster and 9 % slower from process to process (eight XCDs streaming
// eight distant regions); uint16 by runs 3-5 % faster, by rows 2-4 %.  So: float32 by tile rows -- the same speed for a fifth less
// HBM traffic, which the exchange of a sharded stack runs beside -- unless the padding to eight rows costs more than 7 % (then grid
// order); integer element types by runs.  Option xcd_remap: 0 grid order, 1 runs for every type.
static int wg_stack_xcd_order(const StackArgs& st, const LaunchOpts& opts, int es) {
  const int64_t ty = tiles_of(st.nrows, kWgTH), ty8 = xcd_padded(ty);
  const int64_t n = (int64_t)tiles_of(st.W, kWgTW) * ty8 * tiles_of(st.D, st.d_chunk);
  if (opts.xcd_remap == 0 || n >= (int64_t(1) << 31)) return 0;      // (the kernel enumerates the grid in 32 bits)
  if (es < 4 || opts.xcd_remap == 1) return 1;
  return xcd_stripes_balance(ty) && ty8 <= 65535 ? 2 : 0;
}

static bool wg_stack_eligible(const StackArgs& st, const MapArgs& map, const LaunchOpts& opts, int es) {
  return map.tile_dev_ok >= 2 && opts.wg_box && opts.lds_gather && opts.stack_lds && !opts.coef_lds && st.nrows >= 8 && st.W >= 2 && st.H >= 2 &&
         st.row_stride < (1 << 22) && st.H < (1 << 24) && (((uintptr_t)st.vol) & 3u) == 0 && (((int64_t)st.row_stride * es) & 3) == 0 &&
         (((int64_t)st.proj_stride * es) & 3) == 0;
}

// What every stack_wg_kernel launch settles first: does the stack qualify (wg_stack_eligible), and if so its depth chunk, tile order
// and the two A/B options, into *st.  false -- *st untouched -- when it does not, or has too little work: "not taken".
// The depth chunk starts from option d_chunk, halved for elements of 4 bytes and more (an option below 1 ends at 4 per workgroup like
// any other below 4).  float32, measured on cfg4 shards of 64 and 256 projections, five processes: 8 projections per workgroup at
// the default 1-4 % faster than 16 in every one, 4 as fast as 8, 32 and 64 slower by 2 and 4 %; 32-bit integers move float32's bytes
// (tools/ab_int32_stack.py: 8 per workgroup 0-2 % faster than 16 in every process, 32 slower by 2-3 %); the narrower integer
// instantiations, whose fill streams in under the blend, are fastest at 16.
static bool stack_wg_prepare(StackArgs* st, const MapArgs& map, const LaunchOpts& opts, int es) {
  if (!wg_stack_eligible(*st, map, opts, es)) return false;
  const int dc = wg_stack_chunk(*st, es >= 4 ? (opts.d_chunk + 1) / 2 : opts.d_chunk, opts.stack_wg >= 2);
  if (dc == 0) return false;
  st->d_chunk = dc;
  st->xcd_order = wg_stack_xcd_order(*st, opts, es);
  st->store_wait = opts.store_wait;
  st->wg_per_cu = opts.wg_per_cu;
  return true;
}

// would launch_stack() hand this float32 call (float32 coordinates) to stack_wg_kernel?  (dcp_unwarp_images_f32 routes frames of one
// calibration here only when it does: the generic stack kernels are slower than remap_wg_batch_kernel)
bool stack_wg_would_take(const StackArgs& st_in, const MapArgs& map, const LaunchOpts& opts) {
  StackArgs st = st_in;
  return st.D != 0 && st.nrows != 0 && opts.stack_wg && stack_wg_prepare(&st, map, opts, 4);
}

template <int KIND, int NF, typename T>
static hipError_t launch_stack_wg_t(const StackArgs& st, const MapArgs& map, int sampler, hipStream_t stream) {
  // (the tiles of wg_tile_grid, but striped by tile ROWS: wg_stack_xcd_order has applied the balance rule to them)
  dim3 grid(tiles_of(st.W, kWgTW), tiles_of(st.nrows, kWgTH), tiles_of(st.D, st.d_chunk));
  if (st.xcd_order == 2) grid.y = (unsigned)xcd_padded(grid.y);      // see the kernel's tile order
  // (A/B) workgroups per CU capped through unused dynamic LDS
  unsigned pad = 0;
  if (st.wg_per_cu >= 1 && st.wg_per_cu <= 3) pad = (unsigned)(160 * 1024 / st.wg_per_cu - 56 * 1024) & ~255u;
  constexpr int kNoted = KIND == kRadial ? -1 : KIND;                // (the radial kernels keep the name they have always reported)
  if constexpr (std::is_same<T, float>::value) {
    note_kernel("stack_wg_kernel", kNoted, NF, sampler);
    with_blend(sampler, [&](auto s) { hipLaunchKernelGGL((stack_wg_kernel<KIND, NF, decltype(s)::value, float>), grid, dim3(256), pad, stream, st, map); });
  } else {
    note_kernel("stack_wg_kernel", kNoted, NF, kScipy, sizeof(T) == 8 ? ",float64" : sizeof(T) == 4 ? ",32-bit" : sizeof(T) == 2 ? ",16-bit" : ",8-bit");
    hipLaunchKernelGGL((stack_wg_kernel<KIND, NF, kScipy, T>), grid, dim3(256), pad, stream, st, map);
  }
  return hipGetLastError();
}

template <typename T>
static hipError_t launch_stack_wg_n(const StackArgs& st, const MapArgs& map, int sampler, hipStream_t stream) {
  return with_nf_5_4(map, true, [&](auto nf, const MapArgs& m) { return launch_stack_wg_t<kRadial, decltype(nf)::value, T>(st, m, sampler, stream); });
}

// the homography alone (no polynomial), or in front of a radial model: up to five coefficients through the NF = 5 instantiation
// (shorter vectors padded with zeros, see pad_to), longer ones looped with the coefficients in LDS
template <typename T>
static hipError_t launch_stack_wg_kind(MapKind kind, const StackArgs& st, const MapArgs& map, int sampler, hipStream_t stream) {
  if (kind == kPersp) return launch_stack_wg_t<kPersp, 0, T>(st, map, sampler, stream);
  if (map.nfact > 5) return launch_stack_wg_t<kFused, -1, T>(st, map, sampler, stream);
  return launch_stack_wg_t<kFused, 5, T>(st, pad_to<5>(map), sampler, stream);
}

// `st.D` whole frames of one calibration under a homography (kPersp) or the fused perspective o radial map (kFused): float32 (blend
// `sampler`), uint8 and uint16 (scipy's blend), order 1, map certified at level 2 for its kind with a tame homography; st.row_start = 0,
// st.nrows = st.H, st.vol / out reinterpreted, strides in elements, proj_bytes the extent of a frame in bytes.
// *taken = false (and nothing launched): launch the frames one by one.
hipError_t launch_stack_wg_frames(MapKind kind, const StackArgs& st_in, const MapArgs& map, int dtype, int sampler, const LaunchOpts& opts,
                                  hipStream_t stream, bool* taken) {
  *taken = false;
  if ((kind != kPersp && kind != kFused) || (dtype != kF32 && dtype != kU8 && dtype != kU16) || sampler == kNearest) return hipSuccess;
  const int es = elem_size(dtype);
  if (st_in.D == 0 || st_in.nrows != st_in.H || st_in.row_start != 0.0 || !opts.stack_wg || !map.fast_div) return hipSuccess;
  StackArgs st = st_in;
  if (!stack_wg_prepare(&st, map, opts, es)) return hipSuccess;
  st.rb0 = st.rbh = 0;              // whole frames: no row band to reflect into
  st.int_exact = opts.int_exact;
  *taken = true;
  switch (dtype) {
    case kU8: return launch_stack_wg_kind<uint8_t>(kind, st, map, kScipy, stream);
    case kU16: return launch_stack_wg_kind<uint16_t>(kind, st, map, kScipy, stream);
    default: return launch_stack_wg_kind<float>(kind, st, map, sampler, stream);
  }
}

// 8- / 16- / 32-bit integer stacks, float32 coordinates, result of the input's type (unwarp_chunk_slices_backward): st.vol / out
// reinterpreted, strides in elements, proj_bytes the extent of a projection in bytes.  *taken = false: use launch_typed_stack.
hipError_t launch_stack_wg_typed(const StackArgs& st_in, const MapArgs& map, int dtype, const LaunchOpts& opts, hipStream_t stream,
                                 bool* taken) {
  *taken = false;
  if (dtype != kU8 && dtype != kI8 && dtype != kU16 && dtype != kI16 && dtype != kU32 && dtype != kI32 && dtype != kF64) return hipSuccess;
  StackArgs st = st_in;
  // (this route does not ask for option stack_wg, only whether it forces small launches; 32-bit integers, untracked against tracked
  // fill: equal to 1 % better)
  if (st.D == 0 || st.nrows == 0 || !stack_wg_prepare(&st, map, opts, elem_size(dtype))) return hipSuccess;
  st.int_exact = opts.int_exact;
  *taken = true;
  switch (dtype) {
    case kU8: return launch_stack_wg_n<uint8_t>(st, map, kScipy, stream);
    case kI8: return launch_stack_wg_n<int8_t>(st, map, kScipy, stream);
    case kU16: return launch_stack_wg_n<uint16_t>(st, map, kScipy, stream);
    case kI16: return launch_stack_wg_n<int16_t>(st, map, kScipy, stream);
    case kU32: return launch_stack_wg_n<uint32_t>(st, map, kScipy, stream);
    case kF64: return launch_stack_wg_n<double>(st, map, kScipy, stream);
    default: return launch_stack_wg_n<int32_t>(st, map, kScipy, stream);
  }
}

hipError_t launch_stack(const StackArgs& st_in, const MapArgs& map, int sampler, bool round_f32,
                        const LaunchOpts& opts, hipStream_t stream) {
  StackArgs st = st_in;
  st.d_chunk = opts.d_chunk < 1 ? 1 : opts.d_chunk;
  if (st.D == 0 || st.nrows == 0) return hipSuccess;
  // chunks of rows under a certified map: one box per workgroup, two slabs (stack_wg_kernel)
  // (st.int_exact stays the caller's: the float32 instantiations do not read it)
  if (round_f32 && opts.stack_wg && stack_wg_prepare(&st, map, opts, 4)) return launch_stack_wg_n<float>(st, map, sampler, stream);
  // chunks of rows (float32 coordinates): the LDS-staged kernel; a few rows only, or the float64-coordinate
  // slice path: the direct gather
  if (opts.lds_gather && opts.stack_lds && round_f32 && (st.nrows >= 8 || opts.stack_lds == 2) && !opts.coef_lds) {
    // a wave walks its projections one after the other, so the launch needs enough wave tiles to fill the
    // chip (256 CUs x 20 waves): shorten the depth chunk until it does; with too little work even at 4
    // projections per wave the finer-grained direct kernel is the faster one (measured on cfg4: 64 rows of
    // a depth-64 shard 21.8 us direct, 39 us staged; all 2560 rows 876 us direct, 740 us staged)
    const int64_t tiles = (int64_t)((st.W + kLdsTW - 1) / kLdsTW) * ((st.nrows + kLdsTH - 1) / kLdsTH);
    int dc = st.d_chunk;
    auto waves = [&](int c) { return tiles * ((st.D + c - 1) / c); };
    while (dc > 4 && waves(dc) < 8192 && opts.stack_lds == 1 && (st.D + (dc >> 1) - 1) / (dc >> 1) <= 65535) dc >>= 1;
    if (waves(dc) >= 4096 || opts.stack_lds == 2) {
      st.d_chunk = dc;
      return with_nf_5_4(map, true, [&](auto nf, const MapArgs& m) { return launch_stack_lds<decltype(nf)::value>(st, m, sampler, stream); });
    }
  }
  return with_nf_5_4(map, !opts.coef_lds, [&](auto nf, const MapArgs& m) {
    constexpr int NF = decltype(nf)::value;
    return round_f32 ? launch_stack_t<NF, true>(st, m, sampler, stream) : launch_stack_t<NF, false>(st, m, sampler, stream);
  });
}

DCP_DEFINE_BOUNDS_READER(read_bounds_stack)
DCP_DEFINE_LDS_STATS_READER(read_lds_stats_stack, g_stack_lds_stats)

}  // namespace dcp
