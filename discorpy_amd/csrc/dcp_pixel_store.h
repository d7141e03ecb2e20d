// dcp_pixel_store.h -- one store of a whole interleaved pixel (color_kernels.hip, spline_color_kernels.hip).
#pragma once
#include "dcp_internal.h"
#include <type_traits>

namespace dcp {

#ifndef DCP_COLOR_STORE_AUX
#define DCP_COLOR_STORE_AUX 2   // nt: the result is streamed once
#endif

typedef unsigned int u32x3 __attribute__((ext_vector_type(3)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2c __attribute__((ext_vector_type(2)));

// A buffer store of MORE than 64 bits whose data registers are overwritten by the very next VALU instruction stored the NEW
// contents on gfx950 (seen with buffer_store_dwordx3 ... sN offen nt: 500-700 of 4.6e6 values of a frame carried the next row's
// v_cvt_i32_f32 result, differently from run to run).  LLVM's hazard recognizer pads this case only when soffset is NOT a
// register (GCNHazardRecognizer::createsVALUHazard), hipcc therefore left no gap behind the stores with an SGPR row offset.
// The pad keeps the data registers live across one `s_nop 1` (two wait states) behind the store.
#ifndef DCP_WIDE_STORE_PAD_ON
#define DCP_WIDE_STORE_PAD_ON 1
#endif
#if DCP_WIDE_STORE_PAD_ON
#define DCP_WIDE_STORE_PAD(p) asm volatile("s_nop 1" : "+v"(p))
#else
#define DCP_WIDE_STORE_PAD(p) do { } while (0)
#endif

// NC elements of type T to dst + voff (bytes) + soff: one store of the pixel where the hardware has one of that width
template <typename T, int NC>
__device__ __forceinline__ void store_pixel(const T (&v)[NC], __amdgpu_buffer_rsrc_t dst, uint32_t voff, uint32_t soff) {
  constexpr int PS = (int)sizeof(T) * NC;
  if constexpr (std::is_same<T, float>::value && NC == 3) {
    u32x3 p = {__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2])};
    __builtin_amdgcn_raw_buffer_store_b96(p, dst, voff, soff, DCP_COLOR_STORE_AUX);
    DCP_WIDE_STORE_PAD(p);
  } else if constexpr (std::is_same<T, float>::value && NC == 4) {
    u32x4 p = {__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])};
    __builtin_amdgcn_raw_buffer_store_b128(p, dst, voff, soff, DCP_COLOR_STORE_AUX);
    DCP_WIDE_STORE_PAD(p);
  } else if constexpr (std::is_same<T, float>::value && NC == 2) {
    u32x2c p = {__float_as_uint(v[0]), __float_as_uint(v[1])};
    __builtin_amdgcn_raw_buffer_store_b64(p, dst, voff, soff, DCP_COLOR_STORE_AUX);
  } else if constexpr (std::is_same<T, double>::value && NC == 1) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v[0]);
    u32x2c p = {(uint32_t)b, (uint32_t)(b >> 32)};
    __builtin_amdgcn_raw_buffer_store_b64(p, dst, voff, soff, DCP_COLOR_STORE_AUX);
  } else if constexpr (std::is_same<T, float>::value && NC == 1) {
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[0]), dst, voff, soff, DCP_COLOR_STORE_AUX);
  } else if constexpr (sizeof(T) == 4 && NC == 1) {                      // int32 / uint32
    __builtin_amdgcn_raw_buffer_store_b32((uint32_t)v[0], dst, voff, soff, DCP_COLOR_STORE_AUX);
  } else if constexpr (PS == 4) {                                        // 4 x 8-bit, 2 x 16-bit
    uint32_t p = 0;
#pragma unroll
    for (int c = 0; c < NC; ++c) p |= ((uint32_t)v[c] & ((1u << (8 * sizeof(T))) - 1u)) << (8 * sizeof(T) * c);
    __builtin_amdgcn_raw_buffer_store_b32(p, dst, voff, soff, DCP_COLOR_STORE_AUX);
  } else if constexpr (PS == 8) {                                        // 4 x 16-bit
    u32x2c p;
    p.x = ((uint32_t)v[0] & 0xffffu) | (((uint32_t)v[1] & 0xffffu) << 16);
    p.y = ((uint32_t)v[2] & 0xffffu) | (((uint32_t)v[3] & 0xffffu) << 16);
    __builtin_amdgcn_raw_buffer_store_b64(p, dst, voff, soff, DCP_COLOR_STORE_AUX);
  } else {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      if constexpr (sizeof(T) == 1)
        __builtin_amdgcn_raw_buffer_store_b8((unsigned char)v[c], dst, voff + (uint32_t)c, soff, DCP_COLOR_STORE_AUX);
      else if constexpr (sizeof(T) == 2)
        __builtin_amdgcn_raw_buffer_store_b16((unsigned short)v[c], dst, voff + 2u * (uint32_t)c, soff, DCP_COLOR_STORE_AUX);
      else
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint((float)v[c]), dst, voff + 4u * (uint32_t)c, soff, DCP_COLOR_STORE_AUX);
    }
  }
}

}  // namespace dcp
