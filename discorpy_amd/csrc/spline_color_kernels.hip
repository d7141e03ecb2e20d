// spline_color_kernels.hip -- spline orders 2..5 on interleaved (H, W, C) images, C = 1..4: what the reference writes as a loop of
// map_coordinates(mat[:, :, i], ..., order=3) over the channels of a colour photograph (discorpy/util/utility.py:320-341;
// examples/readthedocs_demo/demo_07.py:60) with ONE evaluation of a pixel's coordinate for all its channels.
//
//   spline_wg_color_kernel<KIND, ORDER, NF, EXACT, NC>   spline_wg_kernel's data path (spline_kernels.hip) for NC coefficient planes
//   spline_remap_color_kernel<MAPKIND, ORDER>            spline_remap_kernel with a channel loop: everything the staged kernel does not take
//
// The coefficient planes come from the single-plane prefilter, run once per channel on the column-strided view of that channel
// (launch_spline_prefilter), so plane c holds bit for bit what the single-plane call on mat[:, :, c] filters.  The gathers keep
// spline_wg_kernel's staging decision (sw_box, spline_gather.h) and its per-pixel arithmetic (spline_device.h), so every channel of
// the result is bit for bit what the single-plane entry point returns for that channel -- under scipy's tap order and under the
// factorised sum.
//
// Shared with the other two gather files through spline_gather.h: corner hull, box rule and `staged`; the fill's extent and first
// chunk; the row table; the launch grids, dispatch and kernel name.  Written out here as in spline_kernels.hip, which holds the commented
// copy: the tile order, issue_fill with its masked last load, the tap sum out of the slab, the folding gather (why: spline_gather.h).
//
// Staged kernel: the tile's corner hull, box and `staged` test are evaluated once; phase 1 (row table, map_coord, round_clip_f32)
// runs once; then per channel the slab is refilled from that channel's plane by LDS-DMA and phase 2 reads it.  Between channels the
// RAW / WAR discipline told in spline_gather.h (the slab's fill).
// Bound: per channel as spline_wg_kernel (LDS reads and float64 VALU); the coordinate chain -- about 20 of the 70 (order 3) to 120
// (order 5) instructions per pixel and plane -- is paid once.  No MFMA: a gather, not a contraction.
#include "spline_gather.h"
#include "dcp_pixel_store.h"

namespace dcp {

// Workgroups per CU the register allocation aims at.  spline_wg_kernel's: three below order 5 (the slab and the row tables fit three
// times into a CU's LDS), two at order 5.  Next to one plane's working set a thread keeps its 16 NC float32 results until its pixels
// are stored: orders 2 and 3 hold them inside the 168 registers of three workgroups per CU for every NC, the quartic with three or
// four channels does not (8-156 bytes of scratch per lane, read back in the channel loop) and takes two workgroups per CU.
template <int ORDER, int NC>
constexpr int spline_color_wg_per_cu() {
  return (ORDER >= 5 || (ORDER == 4 && NC >= 3)) ? 2 : 3;
}

// a.coef: NC planes of (Hp x Wp) float64 coefficients, one behind the other; dst: dense (H, W, NC) elements of a.dst_dtype
template <int KIND, int ORDER, int NF, bool EXACT, int NC>
__global__ void __launch_bounds__(256, (spline_color_wg_per_cu<ORDER, NC>())) spline_wg_color_kernel(const SplineArgs a, const MapArgs map, void* dst) {
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
  // ---- corner hull -> box of every tap of the tile -> staged (spline_gather.h); the same for every channel
  const SwBox box = sw_box<KIND, ORDER, NF>(a, map, tx, ty, lane);
  const int bx0 = box.bx0, by0 = box.by0;
  const bool staged = box.staged;
  // the fill (spline_gather.h): every plane gets a descriptor of its own, which ends with the box's last row
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
        // channel -- see spline_wg_kernel)
        if constexpr ((j * 4 + 4) * 64 > kSwBoxH * kSwCH) {
          if ((j * 4 + wave) * 64 + lane < kSwBoxH * kSwCH)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(src_rsrc, (lds_ptr)(s_box + (j * 4 + wave) * 1024), 16, off0 + (wrap ? step_wrap : step_nowrap), 0, 0, 0);
        } else {
          __builtin_amdgcn_raw_ptr_buffer_load_lds(src_rsrc, (lds_ptr)(s_box + (j * 4 + wave) * 1024), 16, off0 + (wrap ? step_wrap : step_nowrap), 0, 0, 0);
        }
      }
    }
  };
  auto plane_rsrc = [&](int c) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)(a.coef + (size_t)c * plane_elems), 0, (int)fill_extent, 0x00020000);
  };
  // ---- row table of this wave's 16 rows, a long polynomial into LDS (spline_gather.h)
  sw_stage_rows<KIND, NF, RW>(a, map, s_row, s_coef, wave, lane, y0);
  // ---- phase 1, once for all channels: the float32 coordinates of this wave's 16 rows, the loads of channel 0 going out between them
  const int rows = __builtin_amdgcn_readfirstlane(max(0, min(16, a.H - y0)));
  const ColCtx col = make_col<KIND, NF>(map, min(x, a.W - 1));
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
  // (a wave without rows or a lane past the last column takes part in every barrier below: a predicate, not a return)
  const bool active = rows > 0 && x < a.W;
  const double padd = (double)a.pad;
  if (!staged) {
    // ---- (rare: a box that reaches over the plane's edge or does not fit) spline_wg_kernel's folding global gather, the weights and
    // the folded tap indices once per pixel, the tap sum per channel.  `staged` is workgroup-uniform: no barrier is skipped by part
    // of a workgroup (nothing was loaded into the slab: nothing to wait for but the s_coef barrier above, which all waves passed)
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
      const size_t pix = ((size_t)(y0 + k) * (size_t)a.W + (size_t)x) * (size_t)NC;
#pragma unroll 1
      for (int c = 0; c < NC; ++c) {
        const double* plane = a.coef + (size_t)c * plane_elems;
        double t = 0.0;
#pragma unroll
        for (int j = 0; j <= ORDER; ++j) {
          const double* row = plane + iy[j];
#pragma unroll
          for (int q = 0; q <= ORDER; ++q) t += (row[ix[q]] * wyv[j]) * wxv[q];
        }
        store_any(dst, a.dst_dtype, pix + (size_t)c, t);
      }
    }
    return;
  }
  // ---- phase 2, per channel: spline_wg_kernel's value(), taps from the slab
  const int org = by0 * PB + bx0 * 8;
  auto value = [&](int k) -> double {
    double wyv[6], wxv[6];
    int sy, sx;
    // (the coordinates pass through an empty asm in every round of the channel loop: the weights of all 16 rows are invariant in
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
    DCP_BOUNDS(sy * PB + sx * 8 - org, ORDER * PB + (ORDER + 1) * 8, sizeof(s_box), 8);
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
  // The channel loop is rolled (one copy of the 16 unrolled evaluations, as in spline_wg_kernel); `keep(c, k, t)` takes the value of
  // channel c in row k, `c` being wave-uniform.
  auto channels_loop = [&](auto&& keep) {
#pragma unroll 1
    for (int c = 0; c < NC; ++c) {
      if (c > 0) {                     // the slab's readers are behind the barrier at the end of the previous round
        const __amdgpu_buffer_rsrc_t rs = plane_rsrc(c);
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
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wave's share of channel c has landed ...
      __syncthreads();                                     // ... and every other wave's: the slab may be read
      if (active) {
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          if (k >= rows) continue;
          keep(c, k, value(k));
        }
      }
      if (c + 1 < NC) lds_barrier();                       // every wave's reads of the slab are retired: the next fill may overwrite it
    }
  };
  // float32 results (the common case): the NC values of a pixel stay in registers and leave in one store of the pixel -- where the
  // registers allow it: the quintic factorised sum needs 212 of the 256 registers of two workgroups per CU for one plane, and 48 or 64
  // results next to it spill; those instantiations store every channel's value as it is computed, like the other element types
  constexpr bool kWholePixels = !(ORDER == 5 && !EXACT && NC >= 3);
  if (kWholePixels && a.dst_dtype == kF32 && (uint64_t)a.H * (uint64_t)a.W * (uint64_t)(4 * NC) < (1ull << 32)) {
    float res[NC][16];
#pragma unroll
    for (int q = 0; q < NC; ++q)
#pragma unroll
      for (int k = 0; k < 16; ++k) res[q][k] = 0.0f;
    channels_loop([&](int c, int k, double t) {
      float v = (float)t;
      asm volatile("" : "+v"(v));      // (the value is finished HERE: left to itself the compiler sinks the sums of all 16 rows behind the last row's
                                       // loads, where their taps -- 16 x (ORDER + 1)^2 doubles -- are live together and spill)
#pragma unroll
      for (int q = 0; q < NC; ++q) res[q][k] = c == q ? v : res[q][k];      // (selects on a uniform condition: no indexed register array)
    });
    if (!active) return;
    const __amdgpu_buffer_rsrc_t drs = __builtin_amdgcn_make_buffer_rsrc(dst, 0, (int)((uint32_t)a.H * (uint32_t)a.W * (uint32_t)(4 * NC)), 0x00020000);
    const uint32_t xoff = ((uint32_t)y0 * (uint32_t)a.W + (uint32_t)x) * (uint32_t)(4 * NC), row_bytes = (uint32_t)a.W * (uint32_t)(4 * NC);
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      if (k >= rows) continue;
      float v[NC];
#pragma unroll
      for (int q = 0; q < NC; ++q) v[q] = res[q][k];
      store_pixel<float, NC>(v, drs, xoff, (uint32_t)k * row_bytes);
    }
  } else {
    // every other element type: converted and stored as scipy does, channel by channel (store_any)
    // (the pixel index passes through an empty asm once per channel: the sixteen 64-bit element indices derived from it are invariant
    // in the channel loop and would otherwise stay live across it)
    int xc = x;
    int last_c = -1;
    channels_loop([&](int c, int k, double t) {
      if (c != last_c) {
        asm volatile("" : "+v"(xc));
        last_c = c;
      }
      store_any(dst, a.dst_dtype, ((size_t)(y0 + k) * (size_t)a.W + (size_t)xc) * (size_t)NC + (size_t)c, t);
    });
  }
}

// MAPKIND 0 radial, 1 perspective, 3 fused perspective -> radial (spline_remap_kernel's numbering); one thread per pixel: coordinate,
// weights and folded tap indices once, the tap sum in scipy's order per channel from that channel's plane, interleaved stores.
template <int MAPKIND, int ORDER>
__global__ void __launch_bounds__(kSplBlock) spline_remap_color_kernel(const SplineArgs a, const MapArgs map, const int channels, void* dst) {
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
  const size_t pix = ((size_t)y * (size_t)a.W + (size_t)x) * (size_t)channels;
#pragma unroll 1
  for (int c = 0; c < channels; ++c) {
    const double* plane = a.coef + (size_t)c * plane_elems;
    double t = 0.0;
#pragma unroll
    for (int j = 0; j <= ORDER; ++j) {
      const double* row = plane + iy[j];
#pragma unroll
      for (int k = 0; k <= ORDER; ++k) t += (row[ix[k]] * wy[j]) * wx[k];
    }
    store_any(dst, a.dst_dtype, pix + (size_t)c, t);
  }
}

// ------------------------------------------------------------------ launchers

DCP_DEFINE_BOUNDS_READER(read_bounds_spline_color)

template <int KIND>
static hipError_t launch_wg_color(const SplineArgs& a_in, const MapArgs& map_in, int channels, void* dst, hipStream_t stream) {
  return spline_wg_with_nf<KIND>(a_in, map_in, [&](auto nf, const SplineArgs& a, const MapArgs& map) {
    auto launch = [&](auto nc) {
      spline_for_order_exact(a, [&](auto ord, auto exact) {
        hipLaunchKernelGGL((spline_wg_color_kernel<KIND, decltype(ord)::value, decltype(nf)::value, decltype(exact)::value, decltype(nc)::value>), spline_wg_grid(a),
                           dim3(256), 0, stream, a, map, dst);
      });
    };
    switch (channels) {
      case 1: launch(std::integral_constant<int, 1>{}); break;
      case 2: launch(std::integral_constant<int, 2>{}); break;
      case 3: launch(std::integral_constant<int, 3>{}); break;
      default: launch(std::integral_constant<int, 4>{}); break;
    }
    return hipGetLastError();
  });
}

template <int MAPKIND>
static hipError_t launch_remap_color_order(const SplineArgs& a, const MapArgs& map, int channels, void* dst, hipStream_t stream) {
  spline_for_order(a, [&](auto ord) {
    hipLaunchKernelGGL((spline_remap_color_kernel<MAPKIND, decltype(ord)::value>), spline_remap_grid(a), dim3(kSplBlock), 0, stream, a, map, channels, dst);
  });
  return hipGetLastError();
}

// The interleaved image at a.src (a.src_stride elements between rows, a.src_cstride between pixels, `channels` = 1..4 elements per
// pixel) -> dense (H, W, channels) at dst.  a.coef: channels + 1 planes of Hp x Wp doubles -- the coefficients of channel c in plane
// c, the last one the prefilter's second plane.  The single-plane prefilter runs once per channel, then ONE gather launch.
hipError_t launch_spline_color(const SplineArgs& a_in, MapKind kind, const MapArgs& map, int channels, void* dst, hipStream_t stream) {
  if (channels < 1 || channels > 4 || (kind != kRadial && kind != kPersp && kind != kFused)) return hipErrorInvalidValue;
  const size_t plane_elems = (size_t)a_in.Hp * (size_t)a_in.Wp;
  char desc[128] = "";
  for (int c = 0; c < channels; ++c) {
    SplineArgs ac = a_in;
    ac.src = (const char*)a_in.src + (size_t)c * (size_t)elem_size(a_in.src_dtype);
    ac.coef = a_in.coef + (size_t)c * plane_elems;
    ac.scratch = a_in.coef + (size_t)channels * plane_elems;
    const hipError_t e = launch_spline_prefilter(ac, stream, desc, sizeof(desc));
    if (e != hipSuccess) return e;
  }
  if ((int64_t)a_in.H * a_in.W == 0) return hipSuccess;
  const bool wg = spline_pick_gather(a_in, kind, map, desc, "_color", "channels", channels);
  if (wg) {
    if (kind == kRadial) return launch_wg_color<kRadial>(a_in, map, channels, dst, stream);
    return launch_wg_color<kPersp>(a_in, map, channels, dst, stream);
  }
  switch (kind) {
    case kRadial: return launch_remap_color_order<0>(a_in, map, channels, dst, stream);
    case kPersp: return launch_remap_color_order<1>(a_in, map, channels, dst, stream);
    default: return launch_remap_color_order<3>(a_in, map, channels, dst, stream);
  }
}

}  // namespace dcp
