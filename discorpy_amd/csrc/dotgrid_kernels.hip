// dotgrid_kernels.hip -- the image-sized and the quadratic work of the dot-grid route (discorpy.prep.preprocessing: calc_size_distance,
// select_dots_based_ratio, calc_hor_slope / calc_ver_slope), DESIGN.md ("Dot grid"):
//   radon_padded_kernel     the sinogram of an H x W plane embedded in a square of zeros of side S, without the circle and without the square
//   nearest_sq_kernel       the four smallest squared distances from every point of a table to the points of the table
//   box_moments_kernel      count and first and second coordinate sums of the nonzero elements inside each box of a table
// Built with -ffp-contract=off: every float expression below is the sequence of IEEE operations DESIGN.md names, so the sinogram equals
// the NumPy restatement (tests/helpers/radon_padded_reference.py) and the distances equal NumPy's bit for bit; the moments are integers.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include "dcp_device.h"

namespace dcp {

// ---------------------------------------------------------------------------------------------------------------- padded Radon

constexpr int kPadRadonBlock = 64;                    // one wave: 64 neighbouring columns of one angle
constexpr int kPadRadonBatch = 4;                     // rows whose taps are in flight together; they are still added one by one

// The source rectangle inside the square: rows py .. py + H - 1, columns px .. px + W - 1 of the square are the plane's, the rest is 0.0
struct PadRect {
  int64_t stride;
  int H, W, py, px;
};

// One tap g(y, x) of the square: where it lies in the SOURCE (`at`) and whether it lies in it at all.  yf / xf are floor / ceil results;
// the comparisons in double keep the conversion to int in range.  No branch: a tap outside reads element (0, 0) instead and drops it,
// so nothing outside the H x W view is ever read.  (The rectangle lies inside the square: a tap outside the square is outside it too.)
struct PadTap {
  int64_t at;
  bool keep;
};

__device__ __forceinline__ PadTap pad_tap(const PadRect& q, double yf, double xf) {
  const bool in = (yf >= (double)q.py) & (yf < (double)(q.py + q.H)) & (xf >= (double)q.px) & (xf < (double)(q.px + q.W));
  const int yi = in ? (int)yf - q.py : 0, xi = in ? (int)xf - q.px : 0;    // 0 <= yi < H, 0 <= xi < W either way
  PadTap t;
  t.at = (int64_t)yi * q.stride + xi;
  t.keep = in;
  return t;
}

struct PadSample {
  PadTap t00, t01, t10, t11;
  double dx, dy;
};

// (xc = ca * c and yc = -sa * c are the thread's own products, the rest is the definition's left-to-right order)
__device__ __forceinline__ PadSample pad_locate(const PadRect& q, double ca, double sa, double tx, double ty, double xc, double yc, int r) {
  const double x = xc + sa * (double)r + tx;
  const double y = yc + ca * (double)r + ty;
  const double x0 = floor(x), x1 = ceil(x), y0 = floor(y), y1 = ceil(y);
  PadSample s;
  s.dx = x - x0;
  s.dy = y - y0;
  s.t00 = pad_tap(q, y0, x0);
  s.t01 = pad_tap(q, y0, x1);
  s.t10 = pad_tap(q, y1, x0);
  s.t11 = pad_tap(q, y1, x1);
  return s;
}

template <typename T>
__device__ __forceinline__ double pad_blend(const PadSample& s, T e00, T e01, T e10, T e11) {
  const double g00 = s.t00.keep ? (double)e00 : 0.0, g01 = s.t01.keep ? (double)e01 : 0.0;
  const double g10 = s.t10.keep ? (double)e10 : 0.0, g11 = s.t11.keep ? (double)e11 : 0.0;
  const double top = (1.0 - s.dx) * g00 + s.dx * g01;
  const double bot = (1.0 - s.dx) * g10 + s.dx * g11;
  return (1.0 - s.dy) * top + s.dy * bot;
}

// `B` consecutive rows from r on: v[j] = the sample (r + j, c); all loads of the batch are issued before any is needed
template <int B, typename T>
__device__ __forceinline__ void pad_rows(const T* __restrict__ src, const PadRect& q, double ca, double sa, double tx, double ty, double xc,
                                         double yc, int r, double* v) {
  PadSample s[B];
  T e[B][4];
#pragma unroll
  for (int j = 0; j < B; ++j) s[j] = pad_locate(q, ca, sa, tx, ty, xc, yc, r + j);
#pragma unroll
  for (int j = 0; j < B; ++j) {
    e[j][0] = src[s[j].t00.at];
    e[j][1] = src[s[j].t01.at];
    e[j][2] = src[s[j].t10.at];
    e[j][3] = src[s[j].t11.at];
  }
#pragma unroll
  for (int j = 0; j < B; ++j) v[j] = pad_blend(s[j], e[j][0], e[j][1], e[j][2], e[j][3]);
}

// One thread per (angle, column of the square): blockIdx.y is the angle, lanes run along the columns, and the thread walks the rows
// 0 .. S - 1 of the square and adds them in that order (no atomics, no tree).  table: {ca, sa, tx, ty} per angle, for side S.  out: (S, A).
template <typename T>
__global__ void __launch_bounds__(kPadRadonBlock) radon_padded_kernel(const T* __restrict__ src, PadRect q, int S, int A,
                                                                      const double* __restrict__ table, double* __restrict__ out) {
  const int c = blockIdx.x * kPadRadonBlock + threadIdx.x, a = blockIdx.y;
  if (c >= S || a >= A) return;
  const double ca = table[4 * a], sa = table[4 * a + 1], tx = table[4 * a + 2], ty = table[4 * a + 3];
  const double xc = ca * (double)c, yc = -sa * (double)c;
  double acc, v[kPadRadonBatch];
  pad_rows<1>(src, q, ca, sa, tx, ty, xc, yc, 0, &acc);
  int r = 1;
  for (; r + kPadRadonBatch <= S; r += kPadRadonBatch) {
    pad_rows<kPadRadonBatch>(src, q, ca, sa, tx, ty, xc, yc, r, v);
#pragma unroll
    for (int j = 0; j < kPadRadonBatch; ++j) acc += v[j];
  }
  for (; r < S; ++r) {
    pad_rows<1>(src, q, ca, sa, tx, ty, xc, yc, r, v);
    acc += v[0];
  }
  out[(int64_t)c * A + a] = acc;
}

hipError_t launch_radon_padded(const void* src, double* dst, int H, int W, int64_t src_stride, int dtype, int nangles, const double* table,
                               void* work, hipStream_t stream) {
  if (H < 1 || W < 1 || nangles < 1 || nangles > kRadonMaxAngles || src_stride < W || !table || !work || (dtype != kF32 && dtype != kF64))
    return hipErrorInvalidValue;
  const int S = radon_padded_side(H, W);
  if (S < H || S < W || S > kRadonMaxSide) return hipErrorInvalidValue;
  hipError_t e = hipMemcpyAsync(work, table, radon_work_bytes(nangles), hipMemcpyHostToDevice, stream);
  // the table is ordinary host memory of the caller: wait until it has been read
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) return e;
  PadRect q;
  q.stride = src_stride;
  q.H = H;
  q.W = W;
  q.py = S / 2 - H / 2;
  q.px = S / 2 - W / 2;
  const dim3 grid((unsigned)((S + kPadRadonBlock - 1) / kPadRadonBlock), (unsigned)nangles);
  if (dtype == kF32)
    hipLaunchKernelGGL((radon_padded_kernel<float>), grid, dim3(kPadRadonBlock), 0, stream, static_cast<const float*>(src), q, S, nangles,
                       static_cast<const double*>(work), dst);
  else
    hipLaunchKernelGGL((radon_padded_kernel<double>), grid, dim3(kPadRadonBlock), 0, stream, static_cast<const double*>(src), q, S, nangles,
                       static_cast<const double*>(work), dst);
  char name[96];
  snprintf(name, sizeof(name), "radon_padded_kernel<%s, angles=%d>", dtype == kF32 ? "float" : "double", nangles);
  set_last_kernel_name(name);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------- nearest distances

constexpr int kNearBlock = 64;                        // one wave of query points: a grid of a few dots is one workgroup, one launch
constexpr int kNearTile = 256;                        // points of the table in LDS at a time: 4 KiB, read by every lane at one address

// One thread per query point i; the table passes through LDS in tiles of kNearTile points, and every lane reads the same point of the
// tile at a time (a broadcast: no bank conflict).  d2 = (yi - yj) * (yi - yj) + (xi - xj) * (xi - xj), each operation rounded; the four
// smallest are kept ascending in registers (j = i included: its 0 is one of them).  The result is a multiset, so the order the tiles
// come in does not matter.  out: (N, 4), +inf where the table has fewer than four points.
__global__ void __launch_bounds__(kNearBlock) nearest_sq_kernel(const double* __restrict__ pts, int N, double* __restrict__ out) {
  __shared__ double ty[kNearTile], tx[kNearTile];
  const int i = blockIdx.x * kNearBlock + threadIdx.x;
  const bool live = i < N;
  const double yi = live ? pts[2 * (int64_t)i] : 0.0, xi = live ? pts[2 * (int64_t)i + 1] : 0.0;
  const double inf = __longlong_as_double(0x7ff0000000000000LL);
  double d0 = inf, d1 = inf, d2 = inf, d3 = inf;
  for (int base = 0; base < N; base += kNearTile) {
    const int n = min(kNearTile, N - base);
    __syncthreads();                                  // the previous tile has been read by every lane
    for (int k = threadIdx.x; k < n; k += kNearBlock) {
      ty[k] = pts[2 * (int64_t)(base + k)];
      tx[k] = pts[2 * (int64_t)(base + k) + 1];
    }
    __syncthreads();
    for (int k = 0; k < n; ++k) {
      const double ey = yi - ty[k], ex = xi - tx[k];
      const double d = ey * ey + ex * ex;
      if (d < d3) {                                   // rarely true once the list has settled; then one pass of an insertion sort
        d3 = d;
        double lo;
        lo = d3 < d2 ? d3 : d2; d3 = d3 < d2 ? d2 : d3; d2 = lo;
        lo = d2 < d1 ? d2 : d1; d2 = d2 < d1 ? d1 : d2; d1 = lo;
        lo = d1 < d0 ? d1 : d0; d1 = d1 < d0 ? d0 : d1; d0 = lo;
      }
    }
  }
  if (!live) return;
  double* o = out + 4 * (int64_t)i;
  o[0] = d0;
  o[1] = d1;
  o[2] = d2;
  o[3] = d3;
}

hipError_t launch_nearest_sq_dists(const double* pts, double* dst, int N, hipStream_t stream) {
  if (N < 1 || N > kNearMaxPoints || !pts || !dst) return hipErrorInvalidValue;
  hipLaunchKernelGGL(nearest_sq_kernel, dim3((unsigned)((N + kNearBlock - 1) / kNearBlock)), dim3(kNearBlock), 0, stream, pts, N, dst);
  set_last_kernel_name("nearest_sq_kernel");
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------- box moments

constexpr int kBoxBlock = 64;                         // one wave per box

// One wave per box (min y, max y, min x, max x; inclusive): lane l takes the elements l, l + 64, ... of the box in raster order (its
// coordinates advance by 64 = qy rows and qx columns at a time: no division per element), sums count, y, x, y y, x y, x x of the
// nonzero ones in int64 with (y, x) relative to the box's corner, and the wave adds the lanes' sums.  Integers: exact in any order.
// E: an unsigned type of the element's size (an element is set where any of its bits is).  An empty box (max < min) gives zeros.
template <typename E>
__global__ void __launch_bounds__(kBoxBlock) box_moments_kernel(const E* __restrict__ src, int64_t stride, const int32_t* __restrict__ boxes,
                                                                int n, long long* __restrict__ sums) {
  const int b = blockIdx.x, lane = threadIdx.x;
  if (b >= n) return;
  const int y0 = boxes[4 * b], y1 = boxes[4 * b + 1], x0 = boxes[4 * b + 2], x1 = boxes[4 * b + 3];
  long long s[6] = {0, 0, 0, 0, 0, 0};
  if (y1 >= y0 && x1 >= x0) {
    const int bh = y1 - y0 + 1, bw = x1 - x0 + 1;
    const int qy = kBoxBlock / bw, qx = kBoxBlock % bw;
    int y = lane / bw, x = lane % bw;
    const E* corner = src + (int64_t)y0 * stride + x0;
    while (y < bh) {
      if (corner[(int64_t)y * stride + x] != 0) {
        const long long yy = y, xx = x;
        s[0] += 1;
        s[1] += yy;
        s[2] += xx;
        s[3] += yy * yy;
        s[4] += xx * yy;
        s[5] += xx * xx;
      }
      y += qy;
      x += qx;
      if (x >= bw) {
        x -= bw;
        y += 1;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 6; ++k)
    for (int off = kBoxBlock / 2; off > 0; off >>= 1) s[k] += __shfl_down(s[k], off, kBoxBlock);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k) sums[6 * (int64_t)b + k] = s[k];
  }
}

hipError_t launch_box_moments(const void* src, int H, int W, int64_t src_stride, int dtype, const int32_t* boxes, int n, long long* sums,
                              void* work, hipStream_t stream) {
  if (H < 1 || W < 1 || src_stride < W || n < 1 || n > kBoxMaxBoxes || !boxes || !sums || !work) return hipErrorInvalidValue;
  const int esz = elem_size(dtype);
  if (esz != 1 && esz != 2) return hipErrorInvalidValue;
  hipError_t e = hipMemcpyAsync(work, boxes, box_work_bytes(n), hipMemcpyHostToDevice, stream);
  // the boxes are ordinary host memory of the caller: wait until they have been read
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) return e;
  if (esz == 1)
    hipLaunchKernelGGL((box_moments_kernel<uint8_t>), dim3((unsigned)n), dim3(kBoxBlock), 0, stream, static_cast<const uint8_t*>(src), src_stride,
                       static_cast<const int32_t*>(work), n, sums);
  else
    hipLaunchKernelGGL((box_moments_kernel<uint16_t>), dim3((unsigned)n), dim3(kBoxBlock), 0, stream, static_cast<const uint16_t*>(src), src_stride,
                       static_cast<const int32_t*>(work), n, sums);
  set_last_kernel_name(esz == 1 ? "box_moments_kernel<8 bit>" : "box_moments_kernel<16 bit>");
  return hipGetLastError();
}

}  // namespace dcp
