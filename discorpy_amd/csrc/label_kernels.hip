// label_kernels.hip -- connected-component labelling, dot measurements and hole filling of discorpy.prep.preprocessing
// (scipy.ndimage.label / sum / center_of_mass / find_objects / binary_fill_holes: preprocessing.py:247-445, 966-997).
//
// A foreground pixel's working value is the linear index y W + x of an ancestor of its component, background is -1, and
// parent[i] <= i always: a component's root is its smallest linear index.  scipy numbers the components 1..n in the raster order of
// their first pixels, so a component's label is 1 + the number of roots with a smaller index: an exclusive prefix sum over the root
// flags.  No sort, no host pass.  The stages, each a launch of its own and each correct with its workgroups running in any order (no
// kernel waits on another workgroup):
//
//   label_tile_kernel<U, FLT>   a workgroup labels one kLabelTW x kLabelTH tile in LDS: union-find with ds atomics on the tile's
//                               pairs (left, up and, at connectivity 8, the two upper diagonals), then every pixel writes the
//                               GLOBAL index of its tile-local root into the parent plane.  Reads only the source.
//   label_init_kernel<U, FLT>   option "x_label_lds" = 0 instead: every foreground pixel its own root.
//   label_merge_kernel          one thread per pixel pair that straddles a tile edge (tiles of 1 x 1 after label_init_kernel: every
//                               pair of the image), the four-tile corners' diagonal pairs included.  find both roots, atomicMin the
//                               larger root's slot to the smaller, repeat until they agree.  Other workgroups write the parent
//                               plane during this launch, so EVERY read of it is an agent-scope relaxed atomic load (a plain load
//                               may be served from a stale line of this CU's L1 or this XCD's L2) and every write an agent-scope
//                               atomic min.  Values only ever decrease, to another ancestor: a lost race is another round.
//   label_flatten_kernel        parent plane (now read-only: plain loads behind the launch boundary) -> the root of every pixel,
//                               written to the second plane.
//   label_count / _scan / _rank_kernel   root flags (root[i] == i), their count per block of kLabelScanChunk pixels, one workgroup
//                               scanning the counts (the total behind them: the number of labels), then each root's rank written to
//                               the parent plane's slot of that root.
//   label_relabel_kernel        dst[i] = rank[root[i]] + 1, 0 for background.
//
// Hole filling (scipy.ndimage.binary_fill_holes = the input OR the components of its complement, 4-neighbour structure, that
// touch no border): the first three stages on the predicate "zero", label_border_kernel stores -2 into the parent slot of every
// border pixel's root (all stores write the same value; it is read in the next launch only), fill_holes_kernel writes
// dst = foreground || parent[root] != -2.
//
// Border components (skimage.segmentation.clear_border of a binary image, dcp_clear_border_2d): the same with the predicate and the
// connectivity turned round -- the first three stages on the SET pixels (or, `invert`, the zero ones) at connectivity 8 or 4,
// label_border_kernel, then clear_border_kernel writes dst = foreground && parent[root] != -2.
//
// Measurements: label_measure_kernel, a wave per 64 pixels of a row.  Lanes of one run of equal labels combine by a segmented
// shuffle scan (count, sum v, sum lane v; y is the wave's), the run's last lane adds to the label's four int64 sums and to its box
// with 32-bit min / max.  Integer atomics: the result does not depend on arrival order.
#include "dcp_device.h"

#include <cstdio>

namespace dcp {

constexpr int kLabelBlock = 256;
constexpr int kLabelTilePixels = kLabelTW * kLabelTH;
constexpr int kLabelPerThread = kLabelTilePixels / kLabelBlock;
constexpr int kLabelScanPerThread = kLabelScanChunk / kLabelBlock;
constexpr int kLabelFlagged = -2;          // label_border_kernel's mark in a root's parent slot
static_assert((kLabelTW & (kLabelTW - 1)) == 0 && kLabelTilePixels % kLabelBlock == 0, "tile");
static_assert(kLabelScanPerThread <= 32, "a thread keeps its flags in one word");

// bounds-checking build: element `i` of a plane (or table) of `n` elements
#define LABEL_AT(i, n, site) DCP_BOUNDS((uint32_t)(i), 1u, (uint32_t)(n), (site))

// nonzero as scipy tests it: NaN and denormals are, -0.0 is not (on the bits: no flush-to-zero mode can change the answer)
template <typename U, bool FLT>
__device__ __forceinline__ bool label_nonzero(U u) {
  if constexpr (FLT) return (U)(u << 1) != (U)0;
  return u != (U)0;
}

__device__ __forceinline__ int32_t ld_agent(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int32_t min_agent(int32_t* p, int32_t v) {
  return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct LabelArgs {
  const void* src;
  int64_t src_stride;      // elements between source rows
  int32_t* parent;         // dense H x W
  int32_t H, W;
  int32_t tiles_x;
  int32_t invert;          // 1: the foreground is where the source is zero (hole filling)
  int32_t conn8;
};

// ------------------------------------------------------------------ stage 1: a tile in LDS

__device__ __forceinline__ int32_t tile_find(int32_t* lab, int32_t a) {
  for (;;) {
    LABEL_AT(a, kLabelTilePixels, 30);
    const int32_t p = __hip_atomic_load(&lab[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (p == a) return a;
    a = p;
  }
}

__device__ __forceinline__ void tile_unite(int32_t* lab, int32_t a, int32_t b) {
  for (;;) {
    a = tile_find(lab, a);
    b = tile_find(lab, b);
    if (a == b) return;
    if (a < b) {
      const int32_t t = a;
      a = b;
      b = t;
    }
    const int32_t old = __hip_atomic_fetch_min(&lab[a], b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (old == a) return;          // a was still a root and now hangs below b
    a = old;                       // somebody else linked a meanwhile: go on from there
  }
}

__device__ __forceinline__ bool tile_fg(int32_t* lab, int32_t p) {
  LABEL_AT(p, kLabelTilePixels, 31);
  return __hip_atomic_load(&lab[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >= 0;
}

template <typename U, bool FLT>
__global__ void __launch_bounds__(kLabelBlock) label_tile_kernel(const LabelArgs a) {
  __shared__ int32_t lab[kLabelTilePixels];
  const U* __restrict__ src = static_cast<const U*>(a.src);
  const int tile_y = (int)(blockIdx.x / (unsigned)a.tiles_x), tile_x = (int)(blockIdx.x - (unsigned)tile_y * (unsigned)a.tiles_x);
  const int y0 = tile_y * kLabelTH, x0 = tile_x * kLabelTW;
  const int tid = (int)threadIdx.x;
  [[maybe_unused]] const int64_t n = (int64_t)a.H * a.W;
#pragma unroll
  for (int k = 0; k < kLabelPerThread; ++k) {
    const int p = k * kLabelBlock + tid, ly = p / kLabelTW, lx = p & (kLabelTW - 1);
    const int y = y0 + ly, x = x0 + lx;
    bool fg = false;
    if (y < a.H && x < a.W) fg = label_nonzero<U, FLT>(src[(int64_t)y * a.src_stride + x]) != (a.invert != 0);
    lab[p] = fg ? p : -1;
  }
  __syncthreads();
  for (int k = 0; k < kLabelPerThread; ++k) {
    const int p = k * kLabelBlock + tid, ly = p / kLabelTW, lx = p & (kLabelTW - 1);
    if (!tile_fg(lab, p)) continue;
    if (lx > 0 && tile_fg(lab, p - 1)) tile_unite(lab, p, p - 1);
    if (ly > 0) {
      if (tile_fg(lab, p - kLabelTW)) tile_unite(lab, p, p - kLabelTW);
      if (a.conn8) {
        if (lx > 0 && tile_fg(lab, p - kLabelTW - 1)) tile_unite(lab, p, p - kLabelTW - 1);
        if (lx < kLabelTW - 1 && tile_fg(lab, p - kLabelTW + 1)) tile_unite(lab, p, p - kLabelTW + 1);
      }
    }
  }
  __syncthreads();
  // (nothing writes `lab` any more)
  for (int k = 0; k < kLabelPerThread; ++k) {
    const int p = k * kLabelBlock + tid, ly = p / kLabelTW, lx = p & (kLabelTW - 1);
    const int y = y0 + ly, x = x0 + lx;
    if (y >= a.H || x >= a.W) continue;
    int32_t out = -1;
    if (lab[p] >= 0) {
      const int32_t r = tile_find(lab, p);
      out = (int32_t)((int64_t)(y0 + r / kLabelTW) * a.W + x0 + (r & (kLabelTW - 1)));
    }
    const int64_t i = (int64_t)y * a.W + x;
    LABEL_AT(i, n, 32);
    a.parent[i] = out;
  }
}

// "x_label_lds" = 0: every foreground pixel starts as its own root; one thread per pixel
template <typename U, bool FLT>
__global__ void __launch_bounds__(kLabelBlock) label_init_kernel(const LabelArgs a) {
  const U* __restrict__ src = static_cast<const U*>(a.src);
  const int64_t n = (int64_t)a.H * a.W, i = (int64_t)blockIdx.x * kLabelBlock + threadIdx.x;
  if (i >= n) return;
  const int y = (int)(i / a.W), x = (int)(i - (int64_t)y * a.W);
  const bool fg = label_nonzero<U, FLT>(src[(int64_t)y * a.src_stride + x]) != (a.invert != 0);
  a.parent[i] = fg ? (int32_t)i : -1;
}

// ------------------------------------------------------------------ stage 2: the seams

__device__ __forceinline__ int32_t plane_find(int32_t* parent, int32_t a, int64_t n) {
  for (;;) {
    LABEL_AT(a, n, 33);
    const int32_t p = ld_agent(parent + a);
    if (p == a) return a;
    a = p;
  }
}

__device__ __forceinline__ void plane_unite(int32_t* parent, int32_t a0, int32_t b0, int64_t n) {
  int32_t a = plane_find(parent, a0, n), b = plane_find(parent, b0, n);
  // the two pixels now point at the roots just found (a value only ever decreases to another ancestor): shorter walks for whoever
  // comes through them next
  if (a != a0) (void)min_agent(parent + a0, a);
  if (b != b0) (void)min_agent(parent + b0, b);
  for (;;) {
    if (a == b) return;
    if (a < b) {
      const int32_t t = a;
      a = b;
      b = t;
    }
    LABEL_AT(a, n, 34);
    const int32_t old = min_agent(parent + a, b);
    if (old == a) return;          // a was still a root and now hangs below b
    a = plane_find(parent, old, n);          // somebody else linked a meanwhile (to `old`, below a): go on from there
    b = plane_find(parent, b, n);
  }
}

__device__ __forceinline__ bool plane_fg(int32_t* parent, int64_t i, int64_t n) {
  LABEL_AT(i, n, 35);
  return ld_agent(parent + i) >= 0;
}

struct MergeArgs {
  int32_t* parent;
  int32_t H, W;
  int32_t tw, th;          // the tiles whose edges are sewn (1 x 1: every pair of the image)
  int32_t conn8;
  int32_t seam_cols;       // ceil(W / tw) - 1
  int64_t n_rows;          // threads of the horizontal seams: (ceil(H / th) - 1) W; the vertical seams' H seam_cols follow
  int64_t n_threads;
};

__global__ void __launch_bounds__(kLabelBlock) label_merge_kernel(const MergeArgs a) {
  int64_t t = (int64_t)blockIdx.x * kLabelBlock + threadIdx.x;
  if (t >= a.n_threads) return;
  const int64_t n = (int64_t)a.H * a.W;
  int32_t* parent = a.parent;
  if (t < a.n_rows) {
    // pixel (y, x) of a tile's first row against the row above: up and, at connectivity 8, up-left and up-right
    const int k = (int)(t / a.W), x = (int)(t - (int64_t)k * a.W), y = (k + 1) * a.th;
    const int64_t i = (int64_t)y * a.W + x, up = i - a.W;
    if (!plane_fg(parent, i, n)) return;
    if (plane_fg(parent, up, n)) plane_unite(parent, (int32_t)i, (int32_t)up, n);
    if (a.conn8) {
      if (x > 0 && plane_fg(parent, up - 1, n)) plane_unite(parent, (int32_t)i, (int32_t)(up - 1), n);
      if (x < a.W - 1 && plane_fg(parent, up + 1, n)) plane_unite(parent, (int32_t)i, (int32_t)(up + 1), n);
    }
    return;
  }
  // pixel (y, x) of a tile's first column against its left neighbour; at connectivity 8 the two diagonals that cross the edge
  // between rows y - 1 and y: (y, x) - (y - 1, x - 1) and (y, x - 1) - (y - 1, x)
  t -= a.n_rows;
  const int y = (int)(t / a.seam_cols), k = (int)(t - (int64_t)y * a.seam_cols), x = (k + 1) * a.tw;
  const int64_t i = (int64_t)y * a.W + x;
  const bool fi = plane_fg(parent, i, n), fl = plane_fg(parent, i - 1, n);
  if (fi && fl) plane_unite(parent, (int32_t)i, (int32_t)(i - 1), n);
  if (a.conn8 && y > 0) {
    if (fi && plane_fg(parent, i - a.W - 1, n)) plane_unite(parent, (int32_t)i, (int32_t)(i - a.W - 1), n);
    if (fl && plane_fg(parent, i - a.W, n)) plane_unite(parent, (int32_t)(i - 1), (int32_t)(i - a.W), n);
  }
}

// ------------------------------------------------------------------ stage 3: every pixel's root

__global__ void __launch_bounds__(kLabelBlock) label_flatten_kernel(const int32_t* __restrict__ parent, int32_t* __restrict__ root, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kLabelBlock + threadIdx.x;
  if (i >= n) return;
  int32_t p = parent[i];
  if (p >= 0)
    for (;;) {
      LABEL_AT(p, n, 36);
      const int32_t q = parent[p];
      if (q == p) break;
      p = q;
    }
  root[i] = p;
}

// ------------------------------------------------------------------ stage 4: the roots' ranks

// this thread's root flags of its block's chunk (bit k: pixel chunk + k * kLabelBlock + tid)
__device__ __forceinline__ uint32_t root_flags(const int32_t* __restrict__ root, int64_t n) {
  const int64_t base = (int64_t)blockIdx.x * kLabelScanChunk + threadIdx.x;
  uint32_t flags = 0;
#pragma unroll
  for (int k = 0; k < kLabelScanPerThread; ++k) {
    const int64_t i = base + k * kLabelBlock;
    if (i < n && root[i] == (int32_t)i) flags |= 1u << k;
  }
  return flags;
}

__global__ void __launch_bounds__(kLabelBlock) label_count_kernel(const int32_t* __restrict__ root, int32_t* __restrict__ counts, int64_t n) {
  __shared__ int32_t wave_sum[kLabelBlock / 64];
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  int32_t mine = __popc(root_flags(root, n));
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) mine += __shfl_down(mine, d);
  if (lane == 0) wave_sum[wave] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t s = 0;
    for (int w = 0; w < kLabelBlock / 64; ++w) s += wave_sum[w];
    counts[blockIdx.x] = s;
  }
}

// one workgroup: counts[0 .. nb) -> their exclusive prefix sums in place, counts[nb] = the total
__global__ void __launch_bounds__(kLabelBlock) label_scan_kernel(int32_t* __restrict__ counts, int32_t nb) {
  __shared__ int32_t wave_sum[kLabelBlock / 64];
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  int32_t carry = 0;
  for (int32_t base = 0; base < nb; base += kLabelBlock) {
    const int32_t j = base + (int32_t)threadIdx.x;
    const int32_t v = j < nb ? counts[j] : 0;
    int32_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int32_t o = __shfl_up(incl, d);
      if (lane >= d) incl += o;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    int32_t before = 0, all = 0;
    for (int w = 0; w < kLabelBlock / 64; ++w) {
      if (w < wave) before += wave_sum[w];
      all += wave_sum[w];
    }
    if (j < nb) counts[j] = carry + before + incl - v;
    carry += all;
    __syncthreads();
  }
  if (threadIdx.x == 0) counts[nb] = carry;
}

// rank[i] = the number of roots before pixel i, for every root i
__global__ void __launch_bounds__(kLabelBlock) label_rank_kernel(const int32_t* __restrict__ root, const int32_t* __restrict__ counts,
                                                                 int32_t* __restrict__ rank, int64_t n) {
  __shared__ int32_t part[kLabelScanPerThread][kLabelBlock / 64];
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const uint32_t flags = root_flags(root, n);
#pragma unroll
  for (int k = 0; k < kLabelScanPerThread; ++k) {
    const unsigned long long m = __ballot((flags >> k) & 1u);
    if (lane == 0) part[k][wave] = __popcll(m);
  }
  __syncthreads();
  int32_t run = counts[blockIdx.x];
  const int64_t base = (int64_t)blockIdx.x * kLabelScanChunk + threadIdx.x;
#pragma unroll
  for (int k = 0; k < kLabelScanPerThread; ++k) {
    int32_t before = run;
    for (int w = 0; w < kLabelBlock / 64; ++w) {
      if (w < wave) before += part[k][w];
      run += part[k][w];
    }
    const unsigned long long m = __ballot((flags >> k) & 1u);
    if ((flags >> k) & 1u) {
      const int64_t i = base + k * kLabelBlock;
      LABEL_AT(i, n, 37);
      rank[i] = before + __popcll(m & ((1ull << lane) - 1ull));
    }
  }
}

// ------------------------------------------------------------------ stage 5

__global__ void __launch_bounds__(kLabelBlock) label_relabel_kernel(int32_t* __restrict__ dst, const int32_t* __restrict__ rank, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kLabelBlock + threadIdx.x;
  if (i >= n) return;
  const int32_t r = dst[i];
  if (r >= 0) LABEL_AT(r, n, 38);
  dst[i] = r < 0 ? 0 : rank[r] + 1;
}

// ------------------------------------------------------------------ hole filling

// border pixel t of the frame (top row, bottom row, left column, right column): its root's parent slot becomes kLabelFlagged
__global__ void __launch_bounds__(kLabelBlock) label_border_kernel(const int32_t* __restrict__ root, int32_t* __restrict__ parent, int H, int W) {
  const int64_t t = (int64_t)blockIdx.x * kLabelBlock + threadIdx.x;
  if (t >= 2 * ((int64_t)W + H)) return;
  int64_t i;
  if (t < W) i = t;
  else if (t < 2 * (int64_t)W) i = (int64_t)(H - 1) * W + (t - W);
  else if (t < 2 * (int64_t)W + H) i = (t - 2 * (int64_t)W) * W;
  else i = (t - 2 * (int64_t)W - H) * W + (W - 1);
  LABEL_AT(i, (int64_t)H * W, 39);
  const int32_t r = root[i];
  if (r < 0) return;
  LABEL_AT(r, (int64_t)H * W, 40);
  parent[r] = kLabelFlagged;
}

__global__ void __launch_bounds__(kLabelBlock) fill_holes_kernel(const int32_t* __restrict__ root, const int32_t* __restrict__ parent,
                                                                 uint8_t* __restrict__ dst, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kLabelBlock + threadIdx.x;
  if (i >= n) return;
  const int32_t r = root[i];          // of the complement: -1 where the source is set
  if (r >= 0) LABEL_AT(r, n, 41);
  dst[i] = (r < 0 || parent[r] != kLabelFlagged) ? 1 : 0;
}

// clear_border: the foreground's own components; a pixel stays where its root's slot was not flagged by label_border_kernel
__global__ void __launch_bounds__(kLabelBlock) clear_border_kernel(const int32_t* __restrict__ root, const int32_t* __restrict__ parent,
                                                                   uint8_t* __restrict__ dst, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kLabelBlock + threadIdx.x;
  if (i >= n) return;
  const int32_t r = root[i];          // -1 where the pixel is background
  if (r >= 0) LABEL_AT(r, n, 43);
  dst[i] = (r >= 0 && parent[r] != kLabelFlagged) ? 1 : 0;
}

// ------------------------------------------------------------------ measurements

enum WeightKind : int { kWNone = 0, kWU8, kWI8, kWU16, kWI16 };

struct MeasureArgs {
  const void* weights;     // may be null: every pixel weighs 1
  const int32_t* labels;
  int64_t w_stride, l_stride;
  int32_t H, W;
  int32_t wkind;
  int32_t num;
  int32_t tiles_x;
  long long* sums;         // [num][4]: count, sum v, sum y v, sum x v
  int32_t* boxes;          // [num][4]: y0, y1, x0, x1
};

__global__ void __launch_bounds__(kLabelBlock) label_measure_init_kernel(long long* sums, int32_t* boxes, int num, int H, int W) {
  const int j = (int)(blockIdx.x * kLabelBlock + threadIdx.x);
  if (j >= num) return;
  for (int c = 0; c < 4; ++c) sums[4 * (int64_t)j + c] = 0;
  boxes[4 * (int64_t)j + 0] = H;
  boxes[4 * (int64_t)j + 1] = -1;
  boxes[4 * (int64_t)j + 2] = W;
  boxes[4 * (int64_t)j + 3] = -1;
}

__device__ __forceinline__ void add_i64(long long* p, long long v) { (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// 64 x 4 pixels per workgroup, a wave per row; blockIdx.x = ty * tiles_x + tx
__global__ void __launch_bounds__(kLabelBlock) label_measure_kernel(const MeasureArgs a) {
  const int tile_y = (int)(blockIdx.x / (unsigned)a.tiles_x), tile_x = (int)(blockIdx.x - (unsigned)tile_y * (unsigned)a.tiles_x);
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const int xb = tile_x * 64, x = xb + lane, y = tile_y * (kLabelBlock / 64) + wave;
  int32_t lab = 0, v = 0;
  if (x < a.W && y < a.H) {
    lab = a.labels[(int64_t)y * a.l_stride + x];
    if (lab < 1 || lab > a.num) lab = 0;
    if (lab) {
      const int64_t wi = (int64_t)y * a.w_stride + x;
      switch (a.wkind) {
        case kWU8: v = static_cast<const uint8_t*>(a.weights)[wi]; break;
        case kWI8: v = static_cast<const int8_t*>(a.weights)[wi]; break;
        case kWU16: v = static_cast<const uint16_t*>(a.weights)[wi]; break;
        case kWI16: v = static_cast<const int16_t*>(a.weights)[wi]; break;
        default: v = 1; break;
      }
    }
  }
  // runs of equal labels along the wave: `start` = the first lane of this lane's run
  const int32_t prev = __shfl_up(lab, 1);
  const unsigned long long heads = __ballot(lane == 0 || prev != lab);
  const int start = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));
  int32_t cnt = 1, sv = v, sl = lane * v;          // |sl| <= 63 * 65535 * 64
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int32_t c = __shfl_up(cnt, d), s = __shfl_up(sv, d), l = __shfl_up(sl, d);
    if (lane - d >= start) {
      cnt += c;
      sv += s;
      sl += l;
    }
  }
  const bool tail = lane == 63 || ((heads >> (lane + 1)) & 1ull);
  if (!tail || !lab) return;
  const int64_t j = lab - 1;
  LABEL_AT(j, a.num, 42);
  long long* s = a.sums + 4 * j;
  int32_t* b = a.boxes + 4 * j;
  add_i64(s + 0, cnt);
  add_i64(s + 1, sv);
  add_i64(s + 2, (long long)y * sv);
  add_i64(s + 3, (long long)xb * sv + sl);
  (void)__hip_atomic_fetch_min(b + 0, y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  (void)__hip_atomic_fetch_max(b + 1, y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  (void)__hip_atomic_fetch_min(b + 2, xb + start, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  (void)__hip_atomic_fetch_max(b + 3, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

DCP_DEFINE_BOUNDS_READER(read_bounds_label)

// ------------------------------------------------------------------ launchers

static unsigned blocks_of(int64_t n) { return (unsigned)((n + kLabelBlock - 1) / kLabelBlock); }

template <typename U, bool FLT>
static hipError_t launch_label_first(const LabelArgs& a, bool use_lds, hipStream_t stream) {
  if (use_lds) {
    const int64_t tiles = (((int64_t)a.H + kLabelTH - 1) / kLabelTH) * a.tiles_x;
    hipLaunchKernelGGL((label_tile_kernel<U, FLT>), dim3((unsigned)tiles), dim3(kLabelBlock), 0, stream, a);
  } else {
    hipLaunchKernelGGL((label_init_kernel<U, FLT>), dim3(blocks_of((int64_t)a.H * a.W)), dim3(kLabelBlock), 0, stream, a);
  }
  return hipGetLastError();
}

// stages 1 to 3: the root of every pixel of the predicate's foreground in `root`, -1 elsewhere; `parent` holds parent[r] == r at
// every root r afterwards
static hipError_t launch_label_roots(const void* src, int32_t* parent, int32_t* root, int H, int W, int64_t src_stride, int dtype, bool conn8,
                                     bool invert, bool use_lds, hipStream_t stream, char* desc, size_t desc_len) {
  if (H < 1 || W < 1 || (int64_t)H * W > 2147483647LL) return hipErrorInvalidValue;
  const int64_t n = (int64_t)H * W;
  LabelArgs a;
  a.src = src;
  a.src_stride = src_stride;
  a.parent = parent;
  a.H = H;
  a.W = W;
  a.tiles_x = (W + kLabelTW - 1) / kLabelTW;
  a.invert = invert ? 1 : 0;
  a.conn8 = conn8 ? 1 : 0;
  hipError_t e;
  switch (dtype) {
    case kU8:
    case kI8:
    case kBool: e = launch_label_first<uint8_t, false>(a, use_lds, stream); break;
    case kU16:
    case kI16: e = launch_label_first<uint16_t, false>(a, use_lds, stream); break;
    case kU32:
    case kI32: e = launch_label_first<uint32_t, false>(a, use_lds, stream); break;
    case kU64:
    case kI64: e = launch_label_first<uint64_t, false>(a, use_lds, stream); break;
    case kF32: e = launch_label_first<uint32_t, true>(a, use_lds, stream); break;
    case kF64: e = launch_label_first<uint64_t, true>(a, use_lds, stream); break;
    default: return hipErrorInvalidValue;
  }
  if (e != hipSuccess) return e;
  MergeArgs m;
  m.parent = parent;
  m.H = H;
  m.W = W;
  m.tw = use_lds ? kLabelTW : 1;
  m.th = use_lds ? kLabelTH : 1;
  m.conn8 = a.conn8;
  m.seam_cols = (W + m.tw - 1) / m.tw - 1;
  m.n_rows = (int64_t)((H + m.th - 1) / m.th - 1) * W;
  m.n_threads = m.n_rows + (int64_t)m.seam_cols * H;
  if (m.n_threads > 0) {
    hipLaunchKernelGGL(label_merge_kernel, dim3(blocks_of(m.n_threads)), dim3(kLabelBlock), 0, stream, m);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  hipLaunchKernelGGL(label_flatten_kernel, dim3(blocks_of(n)), dim3(kLabelBlock), 0, stream, parent, root, n);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  const int bits = elem_size(dtype) * 8;
  if (use_lds)
    snprintf(desc, desc_len, "label_tile_kernel<bits=%d, tile=%dx%d, conn=%d> + %slabel_flatten_kernel", bits, kLabelTW, kLabelTH, conn8 ? 8 : 4,
             m.n_threads > 0 ? "label_merge_kernel<seams> + " : "");
  else
    snprintf(desc, desc_len, "label_init_kernel<bits=%d> + %slabel_flatten_kernel", bits,
             m.n_threads > 0 ? (conn8 ? "label_merge_kernel<every pair, conn=8> + " : "label_merge_kernel<every pair, conn=4> + ") : "");
  return hipSuccess;
}

size_t label_count_words(int H, int W) { return (size_t)(((int64_t)H * W + kLabelScanChunk - 1) / kLabelScanChunk) + 1; }

hipError_t launch_label(const void* src, int32_t* dst, int32_t* parent, int32_t* counts, int H, int W, int64_t src_stride, int dtype, bool conn8,
                        bool use_lds, hipStream_t stream) {
  char desc[192], name[256];
  hipError_t e = launch_label_roots(src, parent, dst, H, W, src_stride, dtype, conn8, false, use_lds, stream, desc, sizeof(desc));
  if (e != hipSuccess) return e;
  const int64_t n = (int64_t)H * W;
  const int32_t nb = (int32_t)(label_count_words(H, W) - 1);
  hipLaunchKernelGGL(label_count_kernel, dim3((unsigned)nb), dim3(kLabelBlock), 0, stream, dst, counts, n);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(label_scan_kernel, dim3(1), dim3(kLabelBlock), 0, stream, counts, nb);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(label_rank_kernel, dim3((unsigned)nb), dim3(kLabelBlock), 0, stream, dst, counts, parent, n);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(label_relabel_kernel, dim3(blocks_of(n)), dim3(kLabelBlock), 0, stream, dst, parent, n);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  snprintf(name, sizeof(name), "%s + label_count/scan/rank_kernel + label_relabel_kernel", desc);
  set_last_kernel_name(name);
  return hipSuccess;
}

hipError_t launch_fill_holes(const void* src, uint8_t* dst, int32_t* parent, int32_t* root, int H, int W, int64_t src_stride, int dtype,
                             bool use_lds, hipStream_t stream) {
  char desc[192], name[256];
  hipError_t e = launch_label_roots(src, parent, root, H, W, src_stride, dtype, false, true, use_lds, stream, desc, sizeof(desc));
  if (e != hipSuccess) return e;
  const int64_t n = (int64_t)H * W;
  hipLaunchKernelGGL(label_border_kernel, dim3(blocks_of(2 * ((int64_t)W + H))), dim3(kLabelBlock), 0, stream, root, parent, H, W);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(fill_holes_kernel, dim3(blocks_of(n)), dim3(kLabelBlock), 0, stream, root, parent, dst, n);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  snprintf(name, sizeof(name), "%s + label_border_kernel + fill_holes_kernel", desc);
  set_last_kernel_name(name);
  return hipSuccess;
}

hipError_t launch_clear_border(const void* src, uint8_t* dst, int32_t* parent, int32_t* root, int H, int W, int64_t src_stride, int dtype,
                               bool conn8, bool invert, bool use_lds, hipStream_t stream) {
  char desc[192], name[256];
  hipError_t e = launch_label_roots(src, parent, root, H, W, src_stride, dtype, conn8, invert, use_lds, stream, desc, sizeof(desc));
  if (e != hipSuccess) return e;
  const int64_t n = (int64_t)H * W;
  hipLaunchKernelGGL(label_border_kernel, dim3(blocks_of(2 * ((int64_t)W + H))), dim3(kLabelBlock), 0, stream, root, parent, H, W);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(clear_border_kernel, dim3(blocks_of(n)), dim3(kLabelBlock), 0, stream, root, parent, dst, n);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  snprintf(name, sizeof(name), "%s + label_border_kernel + clear_border_kernel", desc);
  set_last_kernel_name(name);
  return hipSuccess;
}

hipError_t launch_label_measures(const void* weights, const int32_t* labels, int H, int W, int64_t w_stride, int64_t l_stride, int dtype, int num,
                                 long long* sums, int32_t* boxes, hipStream_t stream) {
  if (H < 1 || W < 1 || num < 0) return hipErrorInvalidValue;
  if (num == 0) return hipSuccess;
  MeasureArgs a;
  a.weights = weights;
  a.labels = labels;
  a.w_stride = w_stride;
  a.l_stride = l_stride;
  a.H = H;
  a.W = W;
  a.num = num;
  a.tiles_x = (W + 63) / 64;
  a.sums = sums;
  a.boxes = boxes;
  if (!weights) a.wkind = kWNone;
  else
    switch (dtype) {
      case kBool:
      case kU8: a.wkind = kWU8; break;
      case kI8: a.wkind = kWI8; break;
      case kU16: a.wkind = kWU16; break;
      case kI16: a.wkind = kWI16; break;
      default: return hipErrorInvalidValue;
    }
  const int64_t tiles = (((int64_t)H + kLabelBlock / 64 - 1) / (kLabelBlock / 64)) * a.tiles_x;
  if (tiles > 2147483647LL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(label_measure_init_kernel, dim3(blocks_of(num)), dim3(kLabelBlock), 0, stream, sums, boxes, num, H, W);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(label_measure_kernel, dim3((unsigned)tiles), dim3(kLabelBlock), 0, stream, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  set_last_kernel_name("label_measure_init_kernel + label_measure_kernel");
  return hipSuccess;
}

}  // namespace dcp
