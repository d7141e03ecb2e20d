// extrema_select_kernels.hip -- get_local_extrema_points(select_peaks=True) of the line-pattern route (discorpy.prep.linepattern:195-274) on an
// (N, L) plane of profiles in one call that never leaves the device: the search (peak_rows_kernel of profile_kernels.hip, integer
// positions, into the workspace), then
//   extrema_list_kernel     one workgroup per row: the row's candidates appended to the call's worklist, and the row's maximum
//   extrema_fit_kernel      a grid of fixed size; a workgroup draws four candidates at a time from a ticket counter and fits them, one
//                           wave each (fit_window of select_peaks_device.h: the code select_peaks_kernel runs), into the keep table
//   extrema_compact_kernel  one workgroup per row: the kept candidates in ascending order, refined by the parabola, into the output
// The number of candidates is known on the device only, so nothing here is sized by it: the worklist holds one entry per candidate in
// the order the rows' workgroups happened to reserve their stretches, a ticket past its end ends the workgroup that drew it, and no
// workgroup ever waits for another.  Every candidate has its own byte of the keep table and every fit is reduced inside its wave in a
// fixed order, so no result depends on which workgroup drew which ticket.  Built with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <limits>
#include "dcp_device.h"
#include "select_peaks_device.h"

namespace dcp {

constexpr int kListBlock = 256;
constexpr int kFitGroupsPerCu = 2;                    // the fit holds 195 VGPRs: two waves per SIMD, one of each of two workgroups

// the call's two counters in front of its workspace
struct ExtremaCounters {
  uint32_t total;      // candidates listed so far; after extrema_list_kernel: of the call
  uint32_t ticket;     // candidates drawn so far (past `total` once every workgroup has drawn its last)
};

// wcand: (N, L) doubles as peak_rows_kernel writes them (row r: its positions, their number in element L - 1).  list[k]: the flat
// index r L + j of a candidate in wcand.  rowmax (null where the caller gives the selection's plane): np.max of every row, in the
// row's type: a NaN anywhere in the row makes it NaN.
template <typename T>
__global__ void __launch_bounds__(kListBlock) extrema_list_kernel(const T* __restrict__ src, int64_t src_stride, int L, const double* __restrict__ wcand,
                                                                  uint32_t* __restrict__ list, ExtremaCounters* __restrict__ counters,
                                                                  T* __restrict__ rowmax) {
  __shared__ uint32_t s_base;
  __shared__ T s_max[kListBlock / 64];
  __shared__ int s_nan[kListBlock / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t first = (int64_t)blockIdx.x * L;
  const int count = min(max((int)wcand[first + L - 1], 0), L - 1);
  if (tid == 0) s_base = count ? atomicAdd(&counters->total, (uint32_t)count) : 0u;
  __syncthreads();
  const uint32_t base = s_base;
  for (int j = tid; j < count; j += kListBlock) list[base + (uint32_t)j] = (uint32_t)(first + j);
  if (!rowmax) return;                                // (the same in every thread)
  const T* __restrict__ row = src + (int64_t)blockIdx.x * src_stride;
  T m = -std::numeric_limits<T>::infinity();
  bool nan = false;
  for (int i = tid; i < L; i += kListBlock) {
    const T v = row[i];
    nan = nan || v != v;
    m = v > m ? v : m;
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    const T o = __shfl_xor(m, s, 64);
    m = o > m ? o : m;
  }
  nan = __any(nan);
  if (lane == 0) {
    DCP_BOUNDS((uint32_t)wave * sizeof(T), sizeof(T), sizeof(s_max), 44);
    DCP_BOUNDS((uint32_t)wave * sizeof(int), sizeof(int), sizeof(s_nan), 45);
    s_max[wave] = m;
    s_nan[wave] = nan ? 1 : 0;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kListBlock / 64; ++w) {
      m = s_max[w] > m ? s_max[w] : m;
      nan = nan || s_nan[w] != 0;
    }
    rowmax[blockIdx.x] = nan ? std::numeric_limits<T>::quiet_NaN() : m;
  }
}

// The window of candidate p of row r is sel[r, p - radius .. p + radius], or, without sel, (T)(max(row) - row[i]) formed in the row's
// type as NumPy forms np.max(list_data) - list_data; whole, because the search takes its candidates from range(radius, L - radius - 1).
// The loop runs the same number of times in every wave of a workgroup (the ticket is drawn for all four): fit_window's barriers are uniform.
template <typename T>
__global__ void __launch_bounds__(kFitBlock) extrema_fit_kernel(const T* __restrict__ src, int64_t src_stride, const T* __restrict__ sel, int64_t sel_stride,
                                                                int L, int radius, double tol, int use_offset, const double* __restrict__ wcand,
                                                                const uint32_t* __restrict__ list, ExtremaCounters* __restrict__ counters,
                                                                const T* __restrict__ rowmax, unsigned char* __restrict__ wkeep) {
  __shared__ double s_y[kFitWaves][kFitMaxWindow];
  __shared__ double s_pick[kFitWaves][2];
  __shared__ uint32_t s_first;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t total = counters->total;             // (final: extrema_list_kernel ended before this kernel began)
  const int n = 2 * radius + 1;
  for (;;) {
    if (threadIdx.x == 0) s_first = atomicAdd(&counters->ticket, (uint32_t)kFitWaves);
    __syncthreads();
    const uint32_t first = s_first;                   // (rewritten behind fit_window's barriers only)
    if (first >= total) break;
    DCP_BOUNDS((uint32_t)wave * sizeof(s_y[0]), sizeof(s_y[0]), sizeof(s_y), 47);
    const uint32_t item = first + (uint32_t)wave;
    bool active = item < total;
    uint32_t flat = 0;
    const T* __restrict__ win = src;
    T mx = (T)0;
    if (active) {
      flat = list[item];
      const int r = (int)(flat / (uint32_t)L), p = (int)wcand[flat];
      active = p >= radius && p + radius < L;         // (what the search guarantees)
      if (active) {
        win = sel ? sel + (int64_t)r * sel_stride + (p - radius) : src + (int64_t)r * src_stride + (p - radius);
        if (!sel) mx = rowmax[r];
      } else if (lane == 0) {
        wkeep[flat] = 0;
      }
    }
    const FitResult res = fit_window(active, n, radius, tol, use_offset, s_y[wave], s_pick[wave], lane,
                                     [&](int i) { return sel ? (double)win[i] : (double)(T)(mx - win[i]); });
    if (active && lane == 0) wkeep[flat] = res.good ? 1 : 0;
  }
}

// dst: row r = the kept candidates' positions in ascending order (subpixel: refined on src), their number in element L - 1.  cand and
// keep (either may be null): the candidates before selection as peak_rows_kernel wrote them, and a byte 0 / 1 for each.
template <typename T>
__global__ void __launch_bounds__(kListBlock) extrema_compact_kernel(const T* __restrict__ src, int64_t src_stride, int L, int subpixel,
                                                                     const double* __restrict__ wcand, const unsigned char* __restrict__ wkeep,
                                                                     double* __restrict__ dst, double* __restrict__ cand, unsigned char* __restrict__ keep) {
  __shared__ int s_wave_n[kListBlock / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t first = (int64_t)blockIdx.x * L;
  const T* __restrict__ row = src + (int64_t)blockIdx.x * src_stride;
  const int count = min(max((int)wcand[first + L - 1], 0), L - 1);
  int kept = 0;                                        // (the same in every thread)
  for (int j0 = 0; j0 < count; j0 += kListBlock) {
    const int j = j0 + tid;
    bool good = false;
    int p = 0;
    if (j < count) {
      const double c = wcand[first + j];
      p = (int)c;
      good = wkeep[first + j] != 0 && p >= 1 && p + 1 < L;
      if (cand) cand[first + j] = c;
      if (keep) keep[first + j] = good ? 1 : 0;
    }
    const unsigned long long mask = __ballot(good);
    DCP_BOUNDS((uint32_t)wave * sizeof(int), sizeof(int), sizeof(s_wave_n), 46);
    if (lane == 0) s_wave_n[wave] = __popcll(mask);
    __syncthreads();
    int before = 0, ngood = 0;
#pragma unroll
    for (int w = 0; w < kListBlock / 64; ++w) {
      before += w < wave ? s_wave_n[w] : 0;
      ngood += s_wave_n[w];
    }
    if (good) {
      const int slot = kept + before + __popcll(mask & ((1ull << lane) - 1ull));      // < count <= L - 1: element L - 1 stays free
      dst[first + slot] = subpixel ? parabola_position(p, (double)row[p - 1], (double)row[p], (double)row[p + 1]) : (double)p;
    }
    kept += ngood;
    __syncthreads();                                   // s_wave_n is rewritten by the next step
  }
  if (tid == 0) {
    dst[first + L - 1] = (double)kept;
    if (cand) cand[first + L - 1] = (double)count;
  }
}

DCP_DEFINE_BOUNDS_READER(read_bounds_extrema_select)

// ------------------------------------------------------------------ launcher

// counters | wcand (N L doubles) | rowmax (N doubles' room) | list (N L words) | wkeep (N L bytes)
size_t extrema_select_work_bytes(int N, int L) {
  const size_t nl = (size_t)N * (size_t)L;
  return 64 + nl * sizeof(double) + (size_t)N * sizeof(double) + nl * sizeof(uint32_t) + nl;
}

template <typename T>
static hipError_t run_extrema_select(const void* src, double* dst, int N, int L, int64_t src_stride, int dtype, int radius, double sensitive, bool subpixel,
                                     const void* sel, int64_t sel_stride, double tol, bool use_offset, double* cand, unsigned char* keep, void* work,
                                     int fit_groups, hipStream_t stream) {
  const size_t nl = (size_t)N * (size_t)L;
  char* const w = static_cast<char*>(work);
  ExtremaCounters* const counters = reinterpret_cast<ExtremaCounters*>(w);
  double* const wcand = reinterpret_cast<double*>(w + 64);
  T* const rowmax = reinterpret_cast<T*>(w + 64 + nl * sizeof(double));
  uint32_t* const list = reinterpret_cast<uint32_t*>(w + 64 + nl * sizeof(double) + (size_t)N * sizeof(double));
  unsigned char* const wkeep = reinterpret_cast<unsigned char*>(list + nl);
  // the ticket and the count start from zero in every call, in stream order
  hipError_t e = hipMemsetAsync(counters, 0, sizeof(ExtremaCounters), stream);
  if (e == hipSuccess) e = launch_peak_rows(src, wcand, N, L, src_stride, dtype, radius, sensitive, false, stream);
  if (e != hipSuccess) return e;
  const T* const s = static_cast<const T*>(src);
  const T* const q = static_cast<const T*>(sel);
  hipLaunchKernelGGL((extrema_list_kernel<T>), dim3((unsigned)N), dim3(kListBlock), 0, stream, s, src_stride, L, wcand, list, counters, q ? nullptr : rowmax);
  hipLaunchKernelGGL((extrema_fit_kernel<T>), dim3((unsigned)fit_groups), dim3(kFitBlock), 0, stream, s, src_stride, q, sel_stride, L, radius, tol,
                     use_offset ? 1 : 0, wcand, list, counters, rowmax, wkeep);
  hipLaunchKernelGGL((extrema_compact_kernel<T>), dim3((unsigned)N), dim3(kListBlock), 0, stream, s, src_stride, L, subpixel ? 1 : 0, wcand, wkeep, dst, cand,
                     keep);
  return hipGetLastError();
}

hipError_t launch_extrema_select(const void* src, double* dst, int N, int L, int64_t src_stride, int dtype, int radius, double sensitive, bool subpixel,
                                 const void* sel, int64_t sel_stride, double tol, bool use_offset, double* cand, unsigned char* keep, void* work,
                                 hipStream_t stream) {
  if (N < 1 || L < 1 || src_stride < L || (sel && sel_stride < L) || radius < 1 || radius > kSelectMaxRadius || radius > kPeakMaxRadius || !src || !dst ||
      !work || (dtype != kF32 && dtype != kF64))
    return hipErrorInvalidValue;
  // the fit grid: a few workgroups per CU, and no more than the candidates the rows can hold at all, four to a workgroup
  int device = 0, cus = 0;
  hipError_t e = hipGetDevice(&device);
  if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
  if (e != hipSuccess) return e;
  const int64_t per_row = (int64_t)L - 2 * radius - 1;
  const int64_t most = per_row > 0 ? ((int64_t)N * per_row + kFitWaves - 1) / kFitWaves : 1;
  const int64_t room = (int64_t)(cus > 0 ? cus : 1) * kFitGroupsPerCu;
  const int fit_groups = (int)(most < room ? most : room);
  if (dtype == kF32)
    e = run_extrema_select<float>(src, dst, N, L, src_stride, dtype, radius, sensitive, subpixel, sel, sel_stride, tol, use_offset, cand, keep, work,
                                  fit_groups, stream);
  else
    e = run_extrema_select<double>(src, dst, N, L, src_stride, dtype, radius, sensitive, subpixel, sel, sel_stride, tol, use_offset, cand, keep, work,
                                   fit_groups, stream);
  char name[160];
  snprintf(name, sizeof(name), "peak_rows_kernel + extrema_list_kernel + extrema_fit_kernel + extrema_compact_kernel<%s, radius=%d%s, groups=%d>",
           dtype == kF32 ? "float" : "double", radius, subpixel ? ", subpixel" : "", fit_groups);
  set_last_kernel_name(name);
  return e;
}

}  // namespace dcp
