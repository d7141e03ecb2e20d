// spline_frames_kernels.hip -- spline orders 2..5 on a stack of frames (n, H, W) under ONE calibration: what the reference's users write
// as a loop of unwarp_image_backward(frame, ..., order=3) over the frames of a video or a detector series
// (examples/readthedocs_demo/demo_07.py:25,60; discorpy/post/postprocessing.py:111-148, 444-492) with ONE evaluation of a pixel's
// coordinate for all the frames of a launch.
//
//   spline_wg_frames_kernel<KIND, ORDER, NF, EXACT>    spline_wg_color_kernel's data path (spline_color_kernels.hip) for any number of planes
//   spline_remap_frames_kernel<MAPKIND, ORDER>         spline_remap_color_kernel with planar stores: everything the staged kernel does not take
//
// The planar counterpart of spline_color_kernels.hip.  The frame count of a launch is a run-time argument; frame f of the launch reads the
// coefficient plane a.coef + f Hp Wp and writes the dense (H, W) plane at dst + f * frame_bytes, through a descriptor (or a 64-bit base)
// of its own: no 32-bit offset spans frames, so a group of frames may exceed 4 GiB where one frame does not.  The coefficient planes come
// from the single-plane prefilter, run once per frame (launch_spline_prefilter), and the gathers keep spline_wg_kernel's staging decision
// (sw_box, spline_gather.h) and its per-pixel arithmetic (spline_device.h): every frame of the result is bit for bit what the
// single-frame entry point returns for it -- under scipy's tap order and under the factorised sum.
//
// Shared with the other two gather files through spline_gather.h: corner hull, box rule and `staged`; the fill's extent and first
// chunk; the row table; the launch grids, dispatch and kernel name.  Written out here as in spline_kernels.hip, which holds the commented
// copy: the tile order, issue_fill with its masked last load, the tap sum out of the slab, the folding gather (why: spline_gather.h).
//
// Staged kernel: corner hull, box and `staged` test once per tile; phase 1 (row table, map_coord, round_clip_f32) once, frame 0's fill
// going out between the coordinate rows; then per frame the slab is refilled from that frame's plane by LDS-DMA and phase 2 reads it.
// A frame's values are stored as they are computed -- nothing is kept across frames, so the registers are spline_wg_kernel's (three
// workgroups per CU, two at order 5).  Between frames the RAW / WAR discipline told in spline_gather.h (the slab's fill).
// Bound: per frame as spline_wg_kernel (LDS reads and float64 VALU); the coordinate chain -- about 20 of the 70 (order 3) to 120
// (order 5) instructions per pixel and plane -- is paid once per launch.  No MFMA: a gather, not a contraction.
#include "spline_gather.h"

namespace dcp {

// a.coef: nframes planes of (Hp x Wp) float64 coefficients, one behind the other; dst: nframes dense (H, W) planes of a.dst_dtype,
// frame_bytes apart (= H W elem_size: passed, not derived, so that the kernel multiplies once in 64 bits)
template <int KIND, int ORDER, int NF, bool EXACT>
__global__ void __launch_bounds__(256, ORDER >= 5 ? 2 : 3)
    spline_wg_frames_kernel(const SplineArgs a, const MapArgs map, const int nframes, const unsigned long long frame_bytes, void* dst) {
  constexpr int RW = KIND == kRadial ? 2 : 4;
  __shared__ __attribute__((aligned(16))) unsigned char s_box[kSwBoxH * kSwBoxW * 8];
  __shared__ double s_row[4][16][RW];                                // one row table per wave: no barrier before it is read
  __shared__ double s_coef[NF < 0 ? kMaxFact : 1];
  static_assert(sizeof(s_box) + sizeof(s_row) + sizeof(s_coef) <= 160 * 1024 / 3, "three workgroups per CU");
  typedef __attribute__((address_space(3))) void* lds_ptr;
  constexpr int PB = kSwBoxW * 8;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int lane = (int)threadIdx.x & 63;
  const int wx = wave & 1, wy = wave >> 1;
  // tile order as spline_wg_kernel: XCD blockIdx.x & 7 owns a run of neighbouring tile columns and sweeps it row by row
  int tx = blockIdx.x;
  const int ty = blockIdx.y;
  if (a.xcd_remap) {
    const int tiles_x = (a.W + kSwTW - 1) / kSwTW;
    const int s_ = (int)blockIdx.x & 7, c_ = (int)blockIdx.x >> 3;
    const int wq = tiles_x >> 3, wr = tiles_x & 7;
    if (c_ >= wq + (s_ < wr ? 1 : 0)) return;                // (workgroup-uniform, before any barrier)
    tx = s_ * wq + min(s_, wr) + c_;
  }
  const int y0 = __builtin_amdgcn_readfirstlane(ty * kSwTH + wy * 16);
  const int x = tx * kSwTW + wx * 64 + lane;
  const float wmaxf = (float)(a.W - 1), hmaxf = (float)(a.H - 1);
  // ---- corner hull -> box of every tap of the tile -> staged (spline_gather.h); the same for every frame
  const SwBox box = sw_box<KIND, ORDER, NF>(a, map, tx, ty, lane);
  const int bx0 = box.bx0, by0 = box.by0;
  const bool staged = box.staged;
  // the fill (spline_gather.h): every plane gets a descriptor of its own, built from a 64-bit base, which ends with the box's last row
  const SwFill fill = sw_fill(a, box, wave, lane);
  const uint32_t rstep = fill.rstep, fill_extent = fill.extent, off0 = fill.off0;
  const int c160 = fill.c160, nchunk = fill.nchunk;
  const size_t plane_elems = (size_t)a.Hp * (size_t)a.Wp;
  auto issue_fill = [&](auto jc, const __amdgpu_buffer_rsrc_t src_rsrc, const uint32_t off0, const int c160) {
    constexpr int j = decltype(jc)::value;
    if constexpr (j < kSwNJ) {
      if (staged && (j * 4 + wave) * 64 < nchunk) {
        constexpr int qrow = (256 * j) / kSwCH, rem = (256 * j) % kSwCH;
        const bool wrap = c160 >= kSwCH - rem;
        const uint32_t step_nowrap = (uint32_t)qrow * rstep + (uint32_t)rem * 16u, step_wrap = step_nowrap + rstep - (uint32_t)PB;
        // (the trailing lanes of the LAST load of a box of full height lie behind the slab, in the row tables: masked, for every
        // frame -- see spline_wg_kernel)
        if constexpr ((j * 4 + 4) * 64 > kSwBoxH * kSwCH) {
          if ((j * 4 + wave) * 64 + lane < kSwBoxH * kSwCH)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(src_rsrc, (lds_ptr)(s_box + (j * 4 + wave) * 1024), 16, off0 + (wrap ? step_wrap : step_nowrap), 0, 0, 0);
        } else {
          __builtin_amdgcn_raw_ptr_buffer_load_lds(src_rsrc, (lds_ptr)(s_box + (j * 4 + wave) * 1024), 16, off0 + (wrap ? step_wrap : step_nowrap), 0, 0, 0);
        }
      }
    }
  };
  auto plane_rsrc = [&](int f) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)(a.coef + (size_t)f * plane_elems), 0, (int)fill_extent, 0x00020000);
  };
  // ---- row table of this wave's 16 rows, a long polynomial into LDS (spline_gather.h)
  sw_stage_rows<KIND, NF, RW>(a, map, s_row, s_coef, wave, lane, y0);
  const int rows = __builtin_amdgcn_readfirstlane(max(0, min(16, a.H - y0)));
  const ColCtx col = make_col<KIND, NF>(map, min(x, a.W - 1));
  // (a wave without rows or a lane past the last column takes part in every barrier below: a predicate, not a return)
  const bool active = rows > 0 && x < a.W;
  const double padd = (double)a.pad;
  if (!staged) {
    // ---- (rare: a box that reaches over the plane's edge or does not fit) spline_wg_kernel's folding global gather, the weights and
    // the folded tap indices once per pixel, the tap sum per frame.  `staged` is workgroup-uniform: no barrier is skipped by part
    // of a workgroup (nothing is loaded into the slab: nothing to wait for but the s_coef barrier above, which all waves passed).
    // It stands IN FRONT of phase 1 -- the colour kernel has it behind --: behind it the sixteen coordinate pairs of phase 1 count as
    // live across this branch and the quartic spills here; the coordinates are evaluated again below either way, to the same values
    if (!active) return;
#pragma unroll 1
    for (int k = 0; k < rows; ++k) {
      double xd, yd;
      map_coord<KIND, NF, RW>(map, s_row[wave], s_coef, col, k, wmaxf, hmaxf, &xd, &yd);
      double wyv[6], wxv[6];
      const int sy = spline_weights<ORDER>((double)round_clip_f32(yd, hmaxf) + padd, wyv);
      const int sx = spline_weights<ORDER>((double)round_clip_f32(xd, wmaxf) + padd, wxv);
      int ix[ORDER + 1];
      size_t iy[ORDER + 1];
#pragma unroll
      for (int q = 0; q <= ORDER; ++q) {
        ix[q] = spline_fold(sx + q, a.Wp, a.mode);
        iy[q] = (size_t)spline_fold(sy + q, a.Hp, a.mode) * (size_t)a.Wp;
      }
      const size_t pix = (size_t)(y0 + k) * (size_t)a.W + (size_t)x;
#pragma unroll 1
      for (int f = 0; f < nframes; ++f) {
        const double* plane = a.coef + (size_t)f * plane_elems;
        double t = 0.0;
#pragma unroll
        for (int j = 0; j <= ORDER; ++j) {
          const double* row = plane + iy[j];
#pragma unroll
          for (int q = 0; q <= ORDER; ++q) t += (row[ix[q]] * wyv[j]) * wxv[q];
        }
        store_any((char*)dst + (size_t)f * (size_t)frame_bytes, a.dst_dtype, pix, t);
      }
    }
    return;
  }
  // ---- phase 1, once for all frames: the float32 coordinates of this wave's 16 rows, the loads of frame 0 going out between them
  float xf[16], yf[16];
  {
    const __amdgpu_buffer_rsrc_t rs0 = plane_rsrc(0);
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      if (k == 0) issue_fill(std::integral_constant<int, 0>{}, rs0, off0, c160);
      if (k == 1) issue_fill(std::integral_constant<int, 1>{}, rs0, off0, c160);
      if (k == 2) issue_fill(std::integral_constant<int, 2>{}, rs0, off0, c160);
      if (k == 3) issue_fill(std::integral_constant<int, 3>{}, rs0, off0, c160);
      if (k == 4) issue_fill(std::integral_constant<int, 4>{}, rs0, off0, c160);
      if (k == 5) issue_fill(std::integral_constant<int, 5>{}, rs0, off0, c160);
      if (k == 6) issue_fill(std::integral_constant<int, 6>{}, rs0, off0, c160);
      if (k == 7) issue_fill(std::integral_constant<int, 7>{}, rs0, off0, c160);
      if (k == 8) issue_fill(std::integral_constant<int, 8>{}, rs0, off0, c160);
      if (k == 9) issue_fill(std::integral_constant<int, 9>{}, rs0, off0, c160);
      if (k == 10) issue_fill(std::integral_constant<int, 10>{}, rs0, off0, c160);
      if (k == 11) issue_fill(std::integral_constant<int, 11>{}, rs0, off0, c160);
      if (k == 12) issue_fill(std::integral_constant<int, 12>{}, rs0, off0, c160);
      static_assert(kSwNJ <= 13, "one load per coordinate row");
      double xd, yd;
      map_coord<KIND, NF, RW>(map, s_row[wave], s_coef, col, k, wmaxf, hmaxf, &xd, &yd);
      xf[k] = round_clip_f32(xd, wmaxf);
      yf[k] = round_clip_f32(yd, hmaxf);
    }
  }
  // ---- phase 2, per frame: spline_wg_kernel's value(), taps from the slab
  const int org = by0 * PB + bx0 * 8;
  auto value = [&](int k) -> double {
    double wyv[6], wxv[6];
    int sy, sx;
    // (the coordinates pass through an empty asm in every round of the frame loop: the weights of all 16 rows are invariant in
    // that loop, and hoisted out of it -- 16 x 2 x (ORDER + 1) doubles -- they spill; the values are unchanged)
    float yk = yf[k], xk = xf[k];
    asm volatile("" : "+v"(yk), "+v"(xk));
    if constexpr (EXACT) {
      sy = spline_weights<ORDER>((double)yk + padd, wyv);
      sx = spline_weights<ORDER>((double)xk + padd, wxv);
    } else {
      sy = spline_weights<ORDER, true>((double)yk + padd, wyv);
      sx = spline_weights<ORDER, true>((double)xk + padd, wxv);
    }
    DCP_BOUNDS(sy * PB + sx * 8 - org, ORDER * PB + (ORDER + 1) * 8, sizeof(s_box), 10);
    const unsigned char* base = s_box + (sy * PB + sx * 8 - org);
    double t = 0.0;
    if constexpr (EXACT) {             // scipy's order: t += (c * wy) * wx, tap by tap
#pragma unroll
      for (int j = 0; j <= ORDER; ++j) {
        const double* row = (const double*)(base + j * PB);
#pragma unroll
        for (int q = 0; q <= ORDER; ++q) t += (row[q] * wyv[j]) * wxv[q];
      }
    } else {                           // factorised: sum_j wy_j (sum_q c_jq wx_q), fused
#pragma unroll
      for (int j = 0; j <= ORDER; ++j) {
        const double* row = (const double*)(base + j * PB);
        double r = row[0] * wxv[0];
#pragma unroll
        for (int q = 1; q <= ORDER; ++q) r = __builtin_fma(row[q], wxv[q], r);
        t = j == 0 ? r * wyv[0] : __builtin_fma(r, wyv[j], t);
      }
    }
    return t;
  };
  // float32 frames within 32-bit byte offsets (the common case): the stores go through a descriptor per frame, as spline_wg_kernel's
  const bool f32_rsrc = a.dst_dtype == kF32 && (uint64_t)a.H * (uint64_t)a.W * 4u < (1ull << 32);
  const uint32_t xoff = ((uint32_t)y0 * (uint32_t)a.W + (uint32_t)x) * 4u, row_bytes = (uint32_t)a.W * 4u;
#pragma unroll 1
  for (int f = 0; f < nframes; ++f) {
    if (f > 0) {                       // the slab's readers are behind the barrier at the end of the previous round
      const __amdgpu_buffer_rsrc_t rs = plane_rsrc(f);
      // (the lane's first offset and chunk column pass through an empty asm: the thirteen load offsets derived from them are
      // invariant in this loop, and kept live across phase 2 they cost thirteen registers that order 5 does not have)
      uint32_t off0c = off0;
      int c160c = c160;
      asm volatile("" : "+v"(off0c), "+v"(c160c));
      issue_fill(std::integral_constant<int, 0>{}, rs, off0c, c160c);
      issue_fill(std::integral_constant<int, 1>{}, rs, off0c, c160c);
      issue_fill(std::integral_constant<int, 2>{}, rs, off0c, c160c);
      issue_fill(std::integral_constant<int, 3>{}, rs, off0c, c160c);
      issue_fill(std::integral_constant<int, 4>{}, rs, off0c, c160c);
      issue_fill(std::integral_constant<int, 5>{}, rs, off0c, c160c);
      issue_fill(std::integral_constant<int, 6>{}, rs, off0c, c160c);
      issue_fill(std::integral_constant<int, 7>{}, rs, off0c, c160c);
      issue_fill(std::integral_constant<int, 8>{}, rs, off0c, c160c);
      issue_fill(std::integral_constant<int, 9>{}, rs, off0c, c160c);
      issue_fill(std::integral_constant<int, 10>{}, rs, off0c, c160c);
      issue_fill(std::integral_constant<int, 11>{}, rs, off0c, c160c);
      issue_fill(std::integral_constant<int, 12>{}, rs, off0c, c160c);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wave's share of frame f has landed ...
    __syncthreads();                                     // ... and every other wave's: the slab may be read
    if (active) {
      char* const fdst = (char*)dst + (size_t)f * (size_t)frame_bytes;        // (64-bit: frame f's plane)
      if (f32_rsrc) {
        const __amdgpu_buffer_rsrc_t drs = __builtin_amdgcn_make_buffer_rsrc((void*)fdst, 0, (int)((uint32_t)a.H * (uint32_t)a.W * 4u), 0x00020000);
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          if (k >= rows) continue;
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint((float)value(k)), drs, xoff, (uint32_t)k * row_bytes, DCP_SPLINE_OUT_AUX);
        }
      } else {
        // every other element type: converted and stored as scipy does (store_any)
        // (the column passes through an empty asm once per frame: the sixteen 64-bit element indices derived from it are invariant
        // in the frame loop and would otherwise stay live across it)
        int xc = x;
        asm volatile("" : "+v"(xc));
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          if (k >= rows) continue;
          store_any(fdst, a.dst_dtype, (size_t)(y0 + k) * (size_t)a.W + (size_t)xc, value(k));
        }
      }
    }
    if (f + 1 < nframes) lds_barrier();                    // every wave's reads of the slab are retired: the next fill may overwrite it
  }
}

// MAPKIND 0 radial, 1 perspective, 3 fused perspective -> radial (spline_remap_kernel's numbering); one thread per pixel: coordinate,
// weights and folded tap indices once, the tap sum in scipy's order per frame from that frame's plane, planar stores.
template <int MAPKIND, int ORDER>
__global__ void __launch_bounds__(kSplBlock)
    spline_remap_frames_kernel(const SplineArgs a, const MapArgs map, const int nframes, const unsigned long long frame_bytes, void* dst) {
  const int x = blockIdx.x * kSplBlock + (int)threadIdx.x;
  const int y = blockIdx.y + blockIdx.z * 65535;       // blockIdx.y walks the rows (no 64-bit division)
  if (x >= a.W || y >= a.H) return;
  const float wmaxf = (float)(a.W - 1), hmaxf = (float)(a.H - 1);
  double xd, yd;
  pixel_coord<MAPKIND == 0 ? kRadial : MAPKIND == 1 ? kPersp : kFused>(map, (double)x, (double)y, wmaxf, hmaxf, &xd, &yd);
  const double xc = (double)round_clip_f32(xd, wmaxf);
  const double yc = (double)round_clip_f32(yd, hmaxf);
  double wy[6], wx[6];
  const int sy = spline_weights<ORDER>(yc + (double)a.pad, wy);
  const int sx = spline_weights<ORDER>(xc + (double)a.pad, wx);
  int ix[ORDER + 1];
  size_t iy[ORDER + 1];
#pragma unroll
  for (int k = 0; k <= ORDER; ++k) {
    ix[k] = spline_fold(sx + k, a.Wp, a.mode);
    iy[k] = (size_t)spline_fold(sy + k, a.Hp, a.mode) * (size_t)a.Wp;
  }
  const size_t plane_elems = (size_t)a.Hp * (size_t)a.Wp;
  const size_t pix = (size_t)y * (size_t)a.W + (size_t)x;
#pragma unroll 1
  for (int f = 0; f < nframes; ++f) {
    const double* plane = a.coef + (size_t)f * plane_elems;
    double t = 0.0;
#pragma unroll
    for (int j = 0; j <= ORDER; ++j) {
      const double* row = plane + iy[j];
#pragma unroll
      for (int k = 0; k <= ORDER; ++k) t += (row[ix[k]] * wy[j]) * wx[k];
    }
    store_any((char*)dst + (size_t)f * (size_t)frame_bytes, a.dst_dtype, pix, t);
  }
}

// ------------------------------------------------------------------ launchers

DCP_DEFINE_BOUNDS_READER(read_bounds_spline_frames)

template <int KIND>
static hipError_t launch_wg_frames(const SplineArgs& a_in, const MapArgs& map_in, int nframes, unsigned long long frame_bytes, void* dst, hipStream_t stream) {
  return spline_wg_with_nf<KIND>(a_in, map_in, [&](auto nf, const SplineArgs& a, const MapArgs& map) {
    spline_for_order_exact(a, [&](auto ord, auto exact) {
      hipLaunchKernelGGL((spline_wg_frames_kernel<KIND, decltype(ord)::value, decltype(nf)::value, decltype(exact)::value>), spline_wg_grid(a), dim3(256), 0,
                         stream, a, map, nframes, frame_bytes, dst);
    });
    return hipGetLastError();
  });
}

template <int MAPKIND>
static hipError_t launch_remap_frames_order(const SplineArgs& a, const MapArgs& map, int nframes, unsigned long long frame_bytes, void* dst, hipStream_t stream) {
  spline_for_order(a, [&](auto ord) {
    hipLaunchKernelGGL((spline_remap_frames_kernel<MAPKIND, decltype(ord)::value>), spline_remap_grid(a), dim3(kSplBlock), 0, stream, a, map, nframes,
                       frame_bytes, dst);
  });
  return hipGetLastError();
}

// `nframes` frames at a.src, `src_frame_stride` elements apart (rows a.src_stride apart, unit column stride) -> dense (nframes, H, W) at
// dst.  a.coef: nframes + 1 planes of Hp x Wp doubles -- the coefficients of frame f in plane f, the last one the prefilter's second
// plane.  The single-plane prefilter runs once per frame, then ONE gather launch.
hipError_t launch_spline_frames(const SplineArgs& a_in, MapKind kind, const MapArgs& map, int nframes, int64_t src_frame_stride, void* dst,
                                hipStream_t stream) {
  if (nframes < 1 || (kind != kRadial && kind != kPersp && kind != kFused)) return hipErrorInvalidValue;
  const size_t plane_elems = (size_t)a_in.Hp * (size_t)a_in.Wp;
  const size_t esz = (size_t)elem_size(a_in.src_dtype);
  char desc[128] = "";
  for (int f = 0; f < nframes; ++f) {
    SplineArgs af = a_in;
    af.src = (const char*)a_in.src + (size_t)f * (size_t)src_frame_stride * esz;
    af.coef = a_in.coef + (size_t)f * plane_elems;
    af.scratch = a_in.coef + (size_t)nframes * plane_elems;
    const hipError_t e = launch_spline_prefilter(af, stream, desc, sizeof(desc));
    if (e != hipSuccess) return e;
  }
  if ((int64_t)a_in.H * a_in.W == 0) return hipSuccess;
  const bool wg = spline_pick_gather(a_in, kind, map, desc, "_frames", "frames", nframes);
  const unsigned long long frame_bytes = (unsigned long long)a_in.H * (unsigned long long)a_in.W * (unsigned long long)elem_size(a_in.dst_dtype);
  if (wg) {
    if (kind == kRadial) return launch_wg_frames<kRadial>(a_in, map, nframes, frame_bytes, dst, stream);
    return launch_wg_frames<kPersp>(a_in, map, nframes, frame_bytes, dst, stream);
  }
  switch (kind) {
    case kRadial: return launch_remap_frames_order<0>(a_in, map, nframes, frame_bytes, dst, stream);
    case kPersp: return launch_remap_frames_order<1>(a_in, map, nframes, frame_bytes, dst, stream);
    default: return launch_remap_frames_order<3>(a_in, map, nframes, frame_bytes, dst, stream);
  }
}

}  // namespace dcp
