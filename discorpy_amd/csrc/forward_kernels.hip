// forward_kernels.hip -- the forward scatter of unwarp_image_forward (discorpy/post/postprocessing.py:151-185).
//
// The reference moves every source pixel (y, x) to (yu, xu) = round(clip(centre + F(rd) (p - centre))) with one fancy assignment,
// mat_unw[yu_mat, xu_mat] = mat.  NumPy assigns in row-major order of the source, so a destination keeps the source pixel with the
// GREATEST index s = y W + x that lands on it, and destinations nobody reaches stay zero.  That rule does not depend on any order
// of execution:
//
//   forward_winner_kernel<NF>    one thread per source pixel, lanes along x: the destination index d in float64 (corner_coord's
//                                chain: correctly rounded sqrt, even / odd Horner, fma(F, xd, xc); clip; rint = half to even) and
//                                a no-return 32-bit atomic maximum winner[d] = max(winner[d], s + 1) -- 0 means vacant
//   forward_fill_kernel<U>       one thread per destination pixel (or per four of them): k = winner[d]; out[d] = k ? src[k - 1] : 0.
//                                U is an unsigned integer of the element's size: elements are moved, never computed with (NaN
//                                payloads and -0.0 arrive unchanged)
//
// The winner plane holds H W words and is zeroed by the launcher on the stream; H W < 2^32 - 1 (the C ABI refuses larger frames).
// Plain 64-bit addressing: sources above 4 GiB are fine.
#include "dcp_internal.h"
#include "dcp_device.h"

#include <cstdio>

namespace dcp {

constexpr int kForwardBlock = 256;

// np.round(np.clip(v, 0, hi)) as an index.  A NaN coordinate (the reference's np.intp(nan) is undefined) goes to 0: whatever the
// coefficients, the index stays inside the frame.
__device__ __forceinline__ int64_t forward_index(double v, double hi) {
  v = v >= 0.0 ? v : 0.0;
  v = v > hi ? hi : v;
  return (int64_t)__builtin_rint(v);
}

template <int NF>
__global__ void __launch_bounds__(kForwardBlock) forward_winner_kernel(uint32_t* __restrict__ winner, int H, int W, const MapArgs map) {
  const int x = blockIdx.x * kForwardBlock + (int)threadIdx.x;
  const int y = blockIdx.y + blockIdx.z * 65535;
  if (x >= W || y >= H) return;
  double xu, yu;
  corner_coord<kRadial, NF>(map, (double)x, (double)y, &xu, &yu);
  const int64_t d = forward_index(yu, (double)(H - 1)) * W + forward_index(xu, (double)(W - 1));
  const int64_t s = (int64_t)y * W + x;
  atomicMax(winner + d, (uint32_t)(s + 1));
}

// VEC destination pixels per thread, flat over the dense destination: VEC = 4 reads its winners with one 16-byte load and stores its
// elements as one vector (H W a multiple of 4, dst aligned to four elements), VEC = 1 serves everything else.  DENSE: the source is
// dense as well, src[s]; otherwise s is split into its row and column (a 32-bit division per occupied pixel).
template <typename U>
struct alignas(sizeof(U) * 4 > 16 ? 16 : sizeof(U) * 4) ForwardVec4 {
  U v[4];
};

template <typename U, int VEC, bool DENSE>
__global__ void __launch_bounds__(kForwardBlock) forward_fill_kernel(const U* __restrict__ src, U* __restrict__ dst,
                                                                    const uint32_t* __restrict__ winner, int64_t rs, int64_t cs, int W, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kForwardBlock + threadIdx.x;      // n = H W / VEC threads
  if (i >= n) return;
  auto fetch = [&](uint32_t k) -> U {
    if (!k) return (U)0;
    const uint32_t s = k - 1u;
    if constexpr (DENSE) return src[s];
    const uint32_t sy = s / (uint32_t)W, sx = s - sy * (uint32_t)W;
    return src[(int64_t)sy * rs + (int64_t)sx * cs];
  };
  if constexpr (VEC == 4) {
    const uint4 k = reinterpret_cast<const uint4*>(winner)[i];
    ForwardVec4<U> out;
    out.v[0] = fetch(k.x);
    out.v[1] = fetch(k.y);
    out.v[2] = fetch(k.z);
    out.v[3] = fetch(k.w);
    reinterpret_cast<ForwardVec4<U>*>(dst)[i] = out;
  } else {
    dst[i] = fetch(winner[i]);
  }
}

// ------------------------------------------------------------------ launchers

// x tiles of 256 pixels, one row per blockIdx.y (65535 per grid.z slice)
static dim3 forward_grid(int H, int W) {
  return dim3((unsigned)((W + kForwardBlock - 1) / kForwardBlock), (unsigned)(H < 65535 ? H : 65535), (unsigned)((H + 65534) / 65535));
}

template <int NF>
static void launch_winner(const ForwardArgs& a, const MapArgs& map, hipStream_t stream) {
  hipLaunchKernelGGL((forward_winner_kernel<NF>), forward_grid(a.H, a.W), dim3(kForwardBlock), 0, stream, a.winner, a.H, a.W, map);
}

template <typename U, int VEC, bool DENSE>
static void launch_fill_v(const ForwardArgs& a, hipStream_t stream) {
  const int64_t n = (int64_t)a.H * a.W / VEC;
  hipLaunchKernelGGL((forward_fill_kernel<U, VEC, DENSE>), dim3((unsigned)((n + kForwardBlock - 1) / kForwardBlock)), dim3(kForwardBlock), 0, stream,
                     (const U*)a.src, (U*)a.dst, a.winner, a.src_stride, a.src_cstride, a.W, n);
}

template <typename U>
static void launch_fill(const ForwardArgs& a, hipStream_t stream) {
  // (the winner plane is the workspace's own allocation: aligned far beyond 16 bytes)
  const bool vec = ((int64_t)a.H * a.W) % 4 == 0 && (uintptr_t)a.dst % (sizeof(U) * 4) == 0;
  const bool dense = a.src_cstride == 1 && (a.src_stride == a.W || a.H == 1);
  if (vec && dense) launch_fill_v<U, 4, true>(a, stream);
  else if (vec) launch_fill_v<U, 4, false>(a, stream);
  else if (dense) launch_fill_v<U, 1, true>(a, stream);
  else launch_fill_v<U, 1, false>(a, stream);
}

hipError_t launch_forward(const ForwardArgs& a, const MapArgs& map, hipStream_t stream) {
  if (a.H <= 0 || a.W <= 0 || (double)a.H * (double)a.W >= 4294967295.0) return hipErrorInvalidValue;
  if (a.esize != 1 && a.esize != 2 && a.esize != 4 && a.esize != 8) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(a.winner, 0, (size_t)a.H * (size_t)a.W * sizeof(uint32_t), stream);
  if (e != hipSuccess) return e;
  // lengths 0..kInlineFact: coefficients straight from the kernel arguments, fully unrolled; longer vectors loop over them
  const int nf = map.nfact <= kInlineFact ? map.nfact : -1;
  switch (nf) {
    case 0: launch_winner<0>(a, map, stream); break;
    case 1: launch_winner<1>(a, map, stream); break;
    case 2: launch_winner<2>(a, map, stream); break;
    case 3: launch_winner<3>(a, map, stream); break;
    case 4: launch_winner<4>(a, map, stream); break;
    case 5: launch_winner<5>(a, map, stream); break;
    case 6: launch_winner<6>(a, map, stream); break;
    case 7: launch_winner<7>(a, map, stream); break;
    case 8: launch_winner<8>(a, map, stream); break;
    case 9: launch_winner<9>(a, map, stream); break;
    case 10: launch_winner<10>(a, map, stream); break;
    default: launch_winner<-1>(a, map, stream); break;
  }
  if ((e = hipGetLastError()) != hipSuccess) return e;
  switch (a.esize) {
    case 1: launch_fill<uint8_t>(a, stream); break;
    case 2: launch_fill<uint16_t>(a, stream); break;
    case 4: launch_fill<uint32_t>(a, stream); break;
    default: launch_fill<uint64_t>(a, stream); break;
  }
  char name[96];
  snprintf(name, sizeof(name), "forward_winner_kernel<NF=%d> + forward_fill_kernel<%d>", nf, a.esize);
  set_last_kernel_name(name);
  return hipGetLastError();
}

}  // namespace dcp
