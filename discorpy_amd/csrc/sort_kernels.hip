// sort_kernels.hip -- the two image-sized steps of discorpy.prep.preprocessing.calculate_threshold (:816-853): np.sort of every pixel
// and the cubic-spline scipy.ndimage.zoom of the sorted list down to max(mat.shape) points.
//
// SORT: a least-significant-digit radix sort of order-preserving keys (order_keys.h) on 8-bit digits.  Floats order as np.sort orders
// them: a NaN loses its sign bit before it is keyed, so NaNs of either sign are the largest keys (among themselves in the order of
// their payloads, and a negative NaN comes out positive); -0.0 comes before +0.0.  No kernel waits on another workgroup: launch
// boundaries are the only synchronisation.
//
//   sort_count_kernel<U, KIND>    reads the plane once through its row stride: writes the dense keys to buffer 0 and counts the 256 bins
//                                 of every digit position in LDS (runs of equal digits along a wave add once), flushed with atomics
//   sort_plan_kernel              one workgroup: per position the exclusive prefix of the bins, whether one bin holds every key (the pass
//                                 is then the identity and is SKIPPED, unless the lab option "x_sort_skip" = 0), and which of the two key
//                                 buffers each pass that runs reads.  The plan stays on the device: the host enqueues every pass, and
//                                 the kernels of a skipped pass return at once
//   per pass  sort_tile_count_kernel   workgroup b counts the digits of its run of 4096-key tiles into column b of the (digit, workgroup) table
//             sort_scan_kernel         a workgroup per digit: exclusive prefix along its row of the table, plus the digit's base
//             sort_scatter_kernel      STABLE scatter: a workgroup walks its tiles in order; in a tile wave w owns keys [1024 w, 1024 w +
//                                      1024) and takes them 64 at a time, lane = key order.  The rank of a key among the keys of its
//                                      digit is: the digit's running offset of the workgroup, plus the earlier waves' counts, plus
//                                      the wave's earlier rounds' count, plus the lanes below it with the same digit (eight ballots)
//   sort_decode_kernel<U, KIND>   keys of the last buffer written -> elements of dst
//
// ZOOM: zoom_cubic_nearest_kernel<T>, one thread per output point, restates scipy 1.15's zoom(order=3, mode="nearest") of a 1-D array:
// the line extended by 12 edge samples per side (an index clamp), multiplied by the gain, filtered by the causal and anticausal
// recursions of the pole sqrt(3) - 2 with the reflect boundary's initial values (what scipy uses for "nearest"), sampled at
// j (n - 1) / (out_n - 1) + 12 with scipy's four weights, t = 0; t += c w in tap order, stored through to_elem.  A point does NOT filter the
// line: its causal recursion starts kZoomWindow = 64 samples in front of its first tap (from scipy's initial value where that reaches
// the line's start), its anticausal one 64 samples behind its last tap (from scipy's value at the line's end).  A start-up error decays
// by |sqrt(3) - 2| per sample: after 64 samples it is below 2^-121 of the window's largest magnitude, far below one float64 rounding
// (2^-53).  The initial sum at the line's start stops after kZoomHorizon = 128 terms (2^-243); lines of up to 129 extended samples are
// summed whole, as scipy sums them.
#include "dcp_device.h"
#include "dcp_internal.h"
#include "order_keys.h"
#include "spline_device.h"

#include <cstdio>

namespace dcp {

constexpr int kSortBlock = 256, kSortWaves = kSortBlock / 64;
constexpr int kSortItems = 16;                                   // keys per thread and tile
constexpr int kSortTile = kSortBlock * kSortItems;               // 4096 keys
constexpr int kSortSeg = 64 * kSortItems;                        // a wave's share of a tile
constexpr int kSortMaxPos = 8;                                   // digit positions of a 64-bit key
constexpr int kSortCountBlocks = 1024;

// What sort_plan_kernel leaves for the passes
struct SortPlan {
  uint32_t skip[kSortMaxPos];          // 1: the pass at this position does not run
  uint32_t from[kSortMaxPos];          // the key buffer (0 / 1) the pass at this position reads
  uint32_t last;                       // the buffer that holds the sorted keys
  uint32_t pad[3];
  uint32_t base[kSortMaxPos][256];     // exclusive prefix of the bins of every position
};

static size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
static int sort_key_bytes(int dtype) { return elem_size(dtype) == 8 ? 8 : 4; }

// tiles, workgroups of a pass and tiles per workgroup
static void sort_geometry(int64_t n, int64_t* tiles, int* nb, int* tpw) {
  *tiles = (n + kSortTile - 1) / kSortTile;
  const int64_t per = (*tiles + kSortMaxBlocks - 1) / kSortMaxBlocks;
  *tpw = (int)per;
  *nb = (int)((*tiles + per - 1) / per);
}

size_t sort_work_bytes(int64_t n, int dtype) {
  int64_t tiles;
  int nb, tpw;
  sort_geometry(n, &tiles, &nb, &tpw);
  return 2 * align256((size_t)n * (size_t)sort_key_bytes(dtype)) + align256(kSortMaxPos * 256 * sizeof(uint32_t)) + align256(sizeof(SortPlan)) +
         align256((size_t)256 * (size_t)nb * sizeof(uint32_t));
}

// the lanes of the wave that are valid and hold the digit of this lane
__device__ __forceinline__ unsigned long long digit_peers(uint32_t d, bool valid) {
  unsigned long long peers = __ballot(valid ? 1 : 0);
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const bool bit = ((d >> b) & 1u) != 0;
    const unsigned long long m = __ballot(valid && bit ? 1 : 0);
    peers &= bit ? m : ~m;
  }
  return peers;
}

// adds the runs of equal bins along the wave to the LDS counters (bin < 0: nothing), as histogram_kernel does; every lane of the wave calls
__device__ __forceinline__ void count_runs(uint32_t* cnt, int bin, int lane) {
  const int prev = __shfl_up(bin, 1);
  const unsigned long long heads = __ballot(lane == 0 || prev != bin);
  if (bin >= 0 && ((heads >> lane) & 1ull)) {
    const unsigned long long above = lane == 63 ? 0ull : (heads >> (lane + 1));
    const int run = above ? __ffsll((long long)above) : 64 - lane;
    (void)__hip_atomic_fetch_add(&cnt[bin], (uint32_t)run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
}

template <typename U, int KIND>
__global__ void __launch_bounds__(kSortBlock) sort_count_kernel(const U* __restrict__ src, int H, int W, int64_t src_stride,
                                                                typename MedianKey<U>::type* __restrict__ keys, uint32_t* __restrict__ hist) {
  typedef typename MedianKey<U>::type K;
  constexpr int kPos = (int)sizeof(U);
  __shared__ uint32_t cnt[kPos * 256];
  const int tid = (int)threadIdx.x, lane = tid & 63;
  for (int j = tid; j < kPos * 256; j += kSortBlock) cnt[j] = 0u;
  __syncthreads();
  const int64_t n = (int64_t)H * W, step = (int64_t)gridDim.x * kSortBlock;
  // (every thread of a workgroup walks the same number of rounds: the shuffles and ballots see whole waves)
  for (int64_t base = (int64_t)blockIdx.x * kSortBlock; base < n; base += step) {
    const int64_t i = base + tid;
    const bool valid = i < n;
    K key = 0;
    if (valid) {
      const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
      U u = src[(int64_t)y * src_stride + x];
      if constexpr (KIND == kKeyFloat) {
        constexpr U kSign = (U)1 << (sizeof(U) * 8 - 1);
        constexpr U kInf = sizeof(U) == 8 ? (U)0x7ff0000000000000ull : (U)0x7f800000u;
        if ((u & ~kSign) > kInf) u &= ~kSign;          // a NaN of either sign sorts last
      }
      key = median_key<U, KIND>(u);
      keys[i] = key;
    }
#pragma unroll
    for (int p = 0; p < kPos; ++p) count_runs(cnt + p * 256, valid ? (int)((key >> (8 * p)) & 255u) : -1, lane);
  }
  __syncthreads();
  for (int j = tid; j < kPos * 256; j += kSortBlock) {
    const uint32_t c = cnt[j];
    if (c) (void)__hip_atomic_fetch_add(&hist[j], c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ void __launch_bounds__(256) sort_plan_kernel(const uint32_t* __restrict__ hist, uint32_t n, int npos, int skip_enabled, SortPlan* plan) {
  __shared__ uint32_t h[kSortMaxPos * 256];
  __shared__ uint32_t one_bin[kSortMaxPos];
  const int tid = (int)threadIdx.x;
  if (tid < kSortMaxPos) one_bin[tid] = 0u;
  for (int p = 0; p < npos; ++p) h[p * 256 + tid] = hist[p * 256 + tid];
  __syncthreads();
  for (int p = 0; p < npos; ++p) {
    uint32_t below = 0;
    for (int d = 0; d < tid; ++d) below += h[p * 256 + d];
    plan->base[p][tid] = below;
    if (h[p * 256 + tid] == n) one_bin[p] = 1u;
  }
  __syncthreads();
  if (tid == 0) {
    uint32_t cur = 0;
    for (int p = 0; p < kSortMaxPos; ++p) {
      const uint32_t skip = p >= npos || (skip_enabled && one_bin[p]) ? 1u : 0u;
      plan->skip[p] = skip;
      plan->from[p] = cur;
      if (!skip) cur ^= 1u;
    }
    plan->last = cur;
  }
}

template <typename K>
__global__ void __launch_bounds__(kSortBlock) sort_tile_count_kernel(const K* __restrict__ buf0, const K* __restrict__ buf1, const SortPlan* __restrict__ plan,
                                                                     int pos, int64_t n, int nb, int tpw, uint32_t* __restrict__ table) {
  if (plan->skip[pos]) return;
  __shared__ uint32_t cnt[256];
  const K* __restrict__ in = plan->from[pos] ? buf1 : buf0;
  const int tid = (int)threadIdx.x, lane = tid & 63, shift = 8 * pos;
  cnt[tid] = 0u;
  __syncthreads();
  const int64_t first = (int64_t)blockIdx.x * tpw * kSortTile;
  int64_t end = first + (int64_t)tpw * kSortTile;
  end = end < n ? end : n;
  for (int64_t base = first; base < end; base += kSortBlock) {
    const int64_t i = base + tid;
    count_runs(cnt, i < end ? (int)((in[i] >> shift) & 255u) : -1, lane);
  }
  __syncthreads();
  table[(size_t)tid * nb + blockIdx.x] = cnt[tid];
}

// row d of the table: counts per workgroup -> the first output index of digit d in every workgroup
__global__ void __launch_bounds__(256) sort_scan_kernel(uint32_t* __restrict__ table, const SortPlan* __restrict__ plan, int pos, int nb) {
  if (plan->skip[pos]) return;
  __shared__ uint32_t part[256];
  const int tid = (int)threadIdx.x;
  uint32_t* row = table + (size_t)blockIdx.x * nb;
  const int per = (nb + 255) / 256, j0 = tid * per;
  uint32_t sum = 0;
  for (int j = j0; j < j0 + per && j < nb; ++j) sum += row[j];
  part[tid] = sum;
  __syncthreads();
  uint32_t run = plan->base[pos][blockIdx.x];
  for (int t = 0; t < tid; ++t) run += part[t];
  for (int j = j0; j < j0 + per && j < nb; ++j) {
    const uint32_t c = row[j];
    row[j] = run;
    run += c;
  }
}

template <typename K>
__global__ void __launch_bounds__(kSortBlock) sort_scatter_kernel(K* __restrict__ buf0, K* __restrict__ buf1, const SortPlan* __restrict__ plan, int pos,
                                                                  int64_t n, int64_t tiles, int nb, int tpw, const uint32_t* __restrict__ table) {
  if (plan->skip[pos]) return;
  __shared__ uint32_t next[256];                          // the workgroup's next output index per digit
  __shared__ uint32_t wave_cnt[kSortWaves][256];          // a wave's count per digit so far in the tile; after the prefix, its first index
  const K* __restrict__ in = plan->from[pos] ? buf1 : buf0;
  K* __restrict__ out = plan->from[pos] ? buf0 : buf1;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, shift = 8 * pos;
  const unsigned long long below = (1ull << lane) - 1ull;
  volatile uint32_t* mine = wave_cnt[wave];
  next[tid] = table[(size_t)tid * nb + blockIdx.x];
  const int64_t tile0 = (int64_t)blockIdx.x * tpw;
  int64_t tile1 = tile0 + tpw;
  tile1 = tile1 < tiles ? tile1 : tiles;
  for (int64_t tile = tile0; tile < tile1; ++tile) {
#pragma unroll
    for (int w = 0; w < kSortWaves; ++w) wave_cnt[w][tid] = 0u;
    __syncthreads();
    const int64_t seg = tile * kSortTile + (int64_t)wave * kSortSeg;
    K key[kSortItems];
    uint32_t rank[kSortItems];
#pragma unroll
    for (int r = 0; r < kSortItems; ++r) {
      const int64_t i = seg + r * 64 + lane;
      const bool valid = i < n;
      key[r] = valid ? in[i] : (K)0;
      const uint32_t d = (uint32_t)((key[r] >> shift) & 255u);
      const unsigned long long peers = digit_peers(d, valid);
      // the keys of this digit in the wave's earlier rounds, then the lanes below: the order the previous pass left
      const uint32_t before = valid ? mine[d] : 0u;
      rank[r] = before + (uint32_t)__popcll(peers & below);
      __builtin_amdgcn_wave_barrier();
      if (valid && (peers & below) == 0ull) mine[d] = before + (uint32_t)__popcll(peers);
      __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    {
      uint32_t run = next[tid];
#pragma unroll
      for (int w = 0; w < kSortWaves; ++w) {
        const uint32_t c = wave_cnt[w][tid];
        wave_cnt[w][tid] = run;
        run += c;
      }
      next[tid] = run;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kSortItems; ++r) {
      const int64_t i = seg + r * 64 + lane;
      if (i < n) {
        const uint32_t at = wave_cnt[wave][(key[r] >> shift) & 255u] + rank[r];
        if ((int64_t)at < n) out[at] = key[r];          // (always true for a consistent table: no store can leave the buffer)
      }
    }
    __syncthreads();
  }
}

template <typename U, int KIND>
__global__ void __launch_bounds__(kSortBlock) sort_decode_kernel(const typename MedianKey<U>::type* __restrict__ buf0,
                                                                 const typename MedianKey<U>::type* __restrict__ buf1,
                                                                 const SortPlan* __restrict__ plan, U* __restrict__ dst, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kSortBlock + threadIdx.x;
  if (i >= n) return;
  dst[i] = median_elem<U, KIND>((plan->last ? buf1 : buf0)[i]);
}

template <typename U, int KIND>
static hipError_t launch_sort_typed(const void* src, void* dst, int H, int W, int64_t src_stride, void* work, bool skip, hipStream_t stream) {
  typedef typename MedianKey<U>::type K;
  constexpr int kPos = (int)sizeof(U);
  const int64_t n = (int64_t)H * W;
  int64_t tiles;
  int nb, tpw;
  sort_geometry(n, &tiles, &nb, &tpw);
  char* w = static_cast<char*>(work);
  const size_t key_bytes = align256((size_t)n * sizeof(K));
  K* buf0 = reinterpret_cast<K*>(w);
  K* buf1 = reinterpret_cast<K*>(w + key_bytes);
  uint32_t* hist = reinterpret_cast<uint32_t*>(w + 2 * key_bytes);
  SortPlan* plan = reinterpret_cast<SortPlan*>(w + 2 * key_bytes + align256(kSortMaxPos * 256 * sizeof(uint32_t)));
  uint32_t* table = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(plan) + align256(sizeof(SortPlan)));
  hipError_t e = hipMemsetAsync(hist, 0, kSortMaxPos * 256 * sizeof(uint32_t), stream);
  if (e != hipSuccess) return e;
  const int64_t rounds = (n + kSortBlock - 1) / kSortBlock;
  const int cb = (int)(rounds < kSortCountBlocks ? rounds : kSortCountBlocks);
  hipLaunchKernelGGL((sort_count_kernel<U, KIND>), dim3((unsigned)cb), dim3(kSortBlock), 0, stream, static_cast<const U*>(src), H, W, src_stride, buf0, hist);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(sort_plan_kernel, dim3(1), dim3(256), 0, stream, hist, (uint32_t)n, kPos, skip ? 1 : 0, plan);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  for (int pos = 0; pos < kPos; ++pos) {
    hipLaunchKernelGGL((sort_tile_count_kernel<K>), dim3((unsigned)nb), dim3(kSortBlock), 0, stream, buf0, buf1, plan, pos, n, nb, tpw, table);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(sort_scan_kernel, dim3(256), dim3(256), 0, stream, table, plan, pos, nb);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL((sort_scatter_kernel<K>), dim3((unsigned)nb), dim3(kSortBlock), 0, stream, buf0, buf1, plan, pos, n, tiles, nb, tpw, table);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  hipLaunchKernelGGL((sort_decode_kernel<U, KIND>), dim3((unsigned)rounds), dim3(kSortBlock), 0, stream, buf0, buf1, plan, static_cast<U*>(dst), n);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  char name[96];
  snprintf(name, sizeof(name), "sort_scatter_kernel<bits=%d, digits=%d, skip=%d>", (int)sizeof(U) * 8, kPos, skip ? 1 : 0);
  set_last_kernel_name(name);
  return hipSuccess;
}

hipError_t launch_sort(const void* src, void* dst, int H, int W, int64_t src_stride, int dtype, void* work, bool skip, hipStream_t stream) {
  if (H < 1 || W < 1 || (int64_t)H * W > 2147483647LL || !work) return hipErrorInvalidValue;
  switch (dtype) {
    case kU8: return launch_sort_typed<uint8_t, kKeyUnsigned>(src, dst, H, W, src_stride, work, skip, stream);
    case kI8: return launch_sort_typed<uint8_t, kKeySigned>(src, dst, H, W, src_stride, work, skip, stream);
    case kU16: return launch_sort_typed<uint16_t, kKeyUnsigned>(src, dst, H, W, src_stride, work, skip, stream);
    case kI16: return launch_sort_typed<uint16_t, kKeySigned>(src, dst, H, W, src_stride, work, skip, stream);
    case kU32: return launch_sort_typed<uint32_t, kKeyUnsigned>(src, dst, H, W, src_stride, work, skip, stream);
    case kI32: return launch_sort_typed<uint32_t, kKeySigned>(src, dst, H, W, src_stride, work, skip, stream);
    case kF32: return launch_sort_typed<uint32_t, kKeyFloat>(src, dst, H, W, src_stride, work, skip, stream);
    case kU64: return launch_sort_typed<uint64_t, kKeyUnsigned>(src, dst, H, W, src_stride, work, skip, stream);
    case kI64: return launch_sort_typed<uint64_t, kKeySigned>(src, dst, H, W, src_stride, work, skip, stream);
    case kF64: return launch_sort_typed<uint64_t, kKeyFloat>(src, dst, H, W, src_stride, work, skip, stream);
    default: return hipErrorInvalidValue;
  }
}

// ------------------------------------------------------------------ zoom

constexpr int kZoomPad = 12, kZoomWindow = 64, kZoomHorizon = 128, kZoomBlock = 64;
constexpr int kZoomSpan = 4 + kZoomWindow;          // causal values a point keeps: its taps and the window behind them

template <typename T>
__global__ void __launch_bounds__(kZoomBlock) zoom_cubic_nearest_kernel(const T* __restrict__ src, int64_t n, T* __restrict__ dst, int64_t out_n, double zoom,
                                                                        double z_n) {
  __shared__ double causal[kZoomSpan][kZoomBlock];          // column `tid` belongs to this thread alone: no barrier
  const int tid = (int)threadIdx.x;
  const int64_t j = (int64_t)blockIdx.x * kZoomBlock + tid;
  if (j >= out_n) return;
  const double z = __builtin_sqrt(3.0) - 2.0, gain = (1.0 - z) * (1.0 - 1.0 / z);
  const int64_t N = n + 2 * kZoomPad;
  auto x = [&](int64_t i) -> double {          // the gained sample at index i of the extended line
    int64_t k = i - kZoomPad;
    k = k < 0 ? 0 : (k > n - 1 ? n - 1 : k);
    return (double)src[k] * gain;
  };
  const double cc = (double)j * zoom + (double)kZoomPad;
  const int64_t s = (int64_t)__builtin_floor(cc) - 1;          // first tap: 11 <= s, s + 3 <= N - 11
  const int64_t lo = s - kZoomWindow > 0 ? s - kZoomWindow : 0;
  const int64_t hi = s + 3 + kZoomWindow < N - 1 ? s + 3 + kZoomWindow : N - 1;
  double t = 0.0;
  int64_t i = lo;
  if (lo == 0) {
    // scipy's initial value of the reflect boundary (_init_causal_reflect), its sum cut after kZoomHorizon terms
    const double x0 = x(0);
    double z_i = z, acc = x0 + z_n * x(N - 1);
    const int64_t m = N - 1 < kZoomHorizon ? N - 1 : kZoomHorizon;
    for (int64_t k = 1; k <= m; ++k) {
      const double far = N - 1 - k == 0 ? acc : x(N - 1 - k);          // (scipy sums in place: its last term reads the partial sum)
      acc += z_i * (x(k) + z_n * far);
      z_i *= z;
    }
    t = acc * (z / (1.0 - z_n * z_n)) + x0;
    i = 1;
  }
  for (; i <= hi; ++i) {
    t = x(i) + z * t;
    if (i >= s) causal[i - s][tid] = t;
  }
  double c0 = 0.0, c1 = 0.0, c2 = 0.0, c3 = 0.0;
  int k = (int)(hi - s);          // 3 <= k < kZoomSpan
  if (hi == N - 1) {
    t = causal[k][tid] * (z / (z - 1.0));
    if (k == 3) c3 = t;
    --k;
  } else {
    t = 0.0;
  }
  for (; k >= 0; --k) {
    t = z * (t - causal[k][tid]);
    if (k == 3) c3 = t;
    if (k == 2) c2 = t;
    if (k == 1) c1 = t;
    if (k == 0) c0 = t;
  }
  double w[4];
  (void)spline_weights<3>(cc, w);
  double v = 0.0;
  v += c0 * w[0];
  v += c1 * w[1];
  v += c2 * w[2];
  v += c3 * w[3];
  dst[j] = to_elem<T>(v);
}

template <typename T>
static hipError_t launch_zoom_as(const void* src, int64_t n, void* dst, int64_t out_n, double zoom, double z_n, hipStream_t stream) {
  const int64_t blocks = (out_n + kZoomBlock - 1) / kZoomBlock;
  hipLaunchKernelGGL((zoom_cubic_nearest_kernel<T>), dim3((unsigned)blocks), dim3(kZoomBlock), 0, stream, static_cast<const T*>(src), n, static_cast<T*>(dst),
                     out_n, zoom, z_n);
  return hipGetLastError();
}

hipError_t launch_zoom_cubic_nearest(const void* src, int64_t n, void* dst, int64_t out_n, int dtype, double z_n, hipStream_t stream) {
  if (n < 1 || out_n < 1 || n > 2147483647LL || out_n > 2147483647LL) return hipErrorInvalidValue;
  const double zoom = out_n > 1 ? (double)(n - 1) / (double)(out_n - 1) : 1.0;
  hipError_t e;
  switch (dtype) {
    case kF32: e = launch_zoom_as<float>(src, n, dst, out_n, zoom, z_n, stream); break;
    case kF64: e = launch_zoom_as<double>(src, n, dst, out_n, zoom, z_n, stream); break;
    case kU8: e = launch_zoom_as<uint8_t>(src, n, dst, out_n, zoom, z_n, stream); break;
    case kI8: e = launch_zoom_as<int8_t>(src, n, dst, out_n, zoom, z_n, stream); break;
    case kU16: e = launch_zoom_as<uint16_t>(src, n, dst, out_n, zoom, z_n, stream); break;
    case kI16: e = launch_zoom_as<int16_t>(src, n, dst, out_n, zoom, z_n, stream); break;
    case kU32: e = launch_zoom_as<uint32_t>(src, n, dst, out_n, zoom, z_n, stream); break;
    case kI32: e = launch_zoom_as<int32_t>(src, n, dst, out_n, zoom, z_n, stream); break;
    case kI64: e = launch_zoom_as<long long>(src, n, dst, out_n, zoom, z_n, stream); break;
    case kU64: e = launch_zoom_as<unsigned long long>(src, n, dst, out_n, zoom, z_n, stream); break;
    default: return hipErrorInvalidValue;
  }
  if (e == hipSuccess) set_last_kernel_name("zoom_cubic_nearest_kernel");
  return e;
}

}  // namespace dcp
