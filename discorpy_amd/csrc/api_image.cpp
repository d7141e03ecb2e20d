// api_image.cpp -- single-frame entry points of the C ABI: radial / perspective / fused remaps, explicit coordinates,
// interleaved channels, the forward scatter, points and coordinate maps, on float32 and the other element types, orders 0..5.  Every frame call
// is described once (FrameCall, make_frame_call) and executed by run_frame; spline orders by api_spline.cpp's run_spline.
#include "api_common.h"

#include <cmath>
#include <cstring>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>

using namespace dcpapi;

namespace {

// The float32 kernels address their source with 32-bit byte offsets (buffer instructions).  A source that
// needs more -- a 40 000 x 40 000 frame fits this GPU's memory many times over -- goes to the generic
// kernels of typed_kernels.hip (64-bit addressing, scipy's exact blend) instead of being refused.
bool beyond_32bit_offsets(int64_t H, int64_t W, int64_t rs, int64_t cs) {
  if (H <= 0 || W <= 0 || rs < 1 || cs < 1) return false;
  const double extent = ((double)(H - 1) * (double)rs + (double)(W - 1) * (double)cs + 1.0) * 4.0;
  return extent > 4294967040.0 && H <= 1073741823LL && W <= 1073741823LL;
}

// Does this HIP runtime move pageable data in both PCIe directions at once when two host threads copy on two
// streams?  ROCm 7.2's does (45 GB/s each way); the runtime bundled with PyTorch-ROCm 2.10 serialises the two
// directions, and the banded path then only adds overhead.  Measured once per process on 32 MiB buffers.
bool runtime_overlaps_directions() {
  static std::once_flag once;
  static bool overlaps = false;
  std::call_once(once, []() {
    const size_t n = 32u << 20;
    void *d0 = nullptr, *d1 = nullptr;
    hipStream_t s_up = nullptr, s_down = nullptr;
    if (g_host_streams.get(&s_up, &s_down) != hipSuccess) return;
    if (g_staging.get(2, n, &d0) != hipSuccess || g_staging.get(3, n, &d1) != hipSuccess) return;
    std::vector<char> up(n, 1), down(n, 2);
    int dev = 0;
    (void)hipGetDevice(&dev);
    auto copy_up = [&]() { (void)hipMemcpyAsync(d0, up.data(), n, hipMemcpyHostToDevice, s_up); (void)hipStreamSynchronize(s_up); };
    auto copy_down = [&]() { (void)hipMemcpyAsync(down.data(), d1, n, hipMemcpyDeviceToHost, s_down); (void)hipStreamSynchronize(s_down); };
    auto now = []() { return std::chrono::steady_clock::now(); };
    copy_up();
    copy_down();                                   // first use of the host pages
    double serial = 1e30, parallel = 1e30;
    for (int rep = 0; rep < 3; ++rep) {
      auto t0 = now();
      copy_up();
      copy_down();
      serial = std::min(serial, std::chrono::duration<double>(now() - t0).count());
      t0 = now();
      std::thread th([&]() { (void)hipSetDevice(dev); copy_down(); });
      copy_up();
      th.join();
      parallel = std::min(parallel, std::chrono::duration<double>(now() - t0).count());
    }
    overlaps = parallel < 0.85 * serial;
  });
  return overlaps;
}

// Row boundaries of the bands a host frame of H rows travels in (run_host_banded, run_host_direct): start[k] .. start[k + 1].
// Nominal height = H / nbands rounded up to 64 rows; the first bands grow 128, 256, 512 .. up to it and the last ones shrink the same
// way, so that the stretch during which only ONE direction of the link is busy -- the first upload, the last download -- is short.
// Frames too small for that (fewer than four nominal bands' worth of rows) are cut evenly.
static std::vector<int64_t> band_plan(int64_t H, int64_t nbands) {
  if (nbands < 1) nbands = 1;
  int64_t big = ((H + nbands - 1) / nbands + 63) / 64 * 64;
  if (big > 65535) big = 65535 / 64 * 64;
  std::vector<int64_t> head;
  for (int64_t r = 128; r < big; r *= 2) head.push_back(r);
  int64_t ramp = 0;
  for (int64_t r : head) ramp += r;
  std::vector<int64_t> start{0};
  if (nbands < 3 || 2 * ramp + 2 * big > H) {
    for (int64_t r = big; r < H; r += big) start.push_back(r);
    start.push_back(H);
    return start;
  }
  int64_t r = 0;
  for (int64_t h : head) start.push_back(r += h);
  const int64_t tail0 = (H - ramp) / 64 * 64;          // where the closing ramp begins (every boundary a multiple of 64 rows)
  while (r + big <= tail0) start.push_back(r += big);
  if (tail0 - r >= 64) start.push_back(r = tail0);     // (a short band in front of the ramp; under 64 rows the ramp's first band takes them)
  for (size_t i = head.size(); i-- > 0;) {
    r = H;
    for (size_t j = 0; j < i; ++j) r -= head[j];
    if (i > 0) r = r / 64 * 64;
    if (r > start.back()) start.push_back(r);
  }
  if (start.back() != H) start.push_back(H);
  return start;
}

// Host frame, radial map, order 1: the frame goes through the GPU in bands of output rows so that PCIe carries data
// in both directions at once.  Output rows [r, r + n) only need the source rows host_row_band() reports, so while
// this thread uploads the source top to bottom and launches one stack-kernel band (depth 1: a band of image rows is
// a chunk of rows of a one-projection stack, bit-identical to the image kernels) as soon as its source rows have
// arrived, a second thread copies finished bands back.  With a runtime that overlaps the two directions (ROCm 7.2's)
// a 4096 x 4096 frame takes ~1.5 ms instead of 2.45 ms; with one that serialises them it costs the same as before.
// `pix` = bytes per pixel (all channels), `rs_bytes` = host row stride in bytes, source_rows(r0, n, &b0, &b1) = source rows
// [b0, b1) that output rows [r0, r0 + n) can reach, launch_band(dsrc, dband, r0, n, stream) enqueues the kernel for
// those output rows reading the whole-frame device copy `dsrc`.
template <typename Hull, typename LaunchBand>
int run_host_banded(const void* src, void* dst, int64_t H, int64_t W, size_t pix, size_t rs_bytes, Hull&& source_rows,
                    LaunchBand&& launch_band) {
  const size_t row_bytes = (size_t)W * pix;
  const size_t frame = (size_t)H * row_bytes;
  void *dsrc = nullptr, *ddst = nullptr;
  DCP_HIP(g_staging.get(0, frame, &dsrc));
  DCP_HIP(g_staging.get(1, frame, &ddst));
  hipStream_t s_up = nullptr, s_down = nullptr;
  DCP_HIP(g_host_streams.get(&s_up, &s_down));
  int cur_dev = 0;
  DCP_HIP(hipGetDevice(&cur_dev));
  // bands of output rows: `host_bands` equal ones would leave the first band's upload and the last band's download uncovered by the
  // other direction (2 / host_bands of the transfer time); the plan below opens with 128, 256, 512 .. rows, runs at the nominal band
  // height and closes .., 512, 256, 128 -- head and tail shrink to ~3 % of a 4096-row frame each
  // (twice `host_bands` nominal bands here: 1.77-1.85 ms against 1.85-1.87 per 4096^2 frame on /opt/rocm's runtime, profiles/r06g_host_bands.txt;
  // the direct-write path, whose bands are kernels storing over PCIe, is best at `host_bands` itself)
  const std::vector<int64_t> start = band_plan(H, 2 * (int64_t)g_host_bands.load());
  const int64_t nb = (int64_t)start.size() - 1;
  // one event per band, recorded behind its kernel: the downloader's stream waits for it on the device, this thread goes straight
  // on to the next upload (round 6; it used to synchronise the stream after every band: ~25 us x bands on the upload's critical path)
  thread_local std::vector<hipEvent_t> ev;
  thread_local int ev_dev = -1;
  if (ev_dev != cur_dev) {
    for (auto e : ev) (void)hipEventDestroy(e);
    ev.clear();
    ev_dev = cur_dev;
  }
  while ((int64_t)ev.size() < nb) {
    hipEvent_t e = nullptr;
    DCP_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    ev.push_back(e);
  }
  hipEvent_t* const band_done = ev.data();      // (the downloader thread must not name `ev`: a thread_local is ITS OWN, empty, vector there)

  std::mutex mu;
  std::condition_variable cv;
  int64_t computed = 0;
  bool abort_down = false;
  hipError_t down_err = hipSuccess;
  std::thread downloader([&]() {
    hipError_t e = hipSetDevice(cur_dev);
    for (int64_t k = 0; k < nb && e == hipSuccess; ++k) {
      {
        std::unique_lock<std::mutex> lock(mu);
        cv.wait(lock, [&] { return computed > k || abort_down; });
        if (abort_down) break;
      }
      const int64_t r0 = start[(size_t)k], n = start[(size_t)k + 1] - r0;
      e = hipStreamWaitEvent(s_down, band_done[k], 0);             // band k's kernel has finished (recorded before `computed` moved)
      if (e == hipSuccess)
        e = hipMemcpyAsync((char*)dst + (size_t)r0 * row_bytes, (const char*)ddst + (size_t)r0 * row_bytes, (size_t)n * row_bytes,
                           hipMemcpyDeviceToHost, s_down);
      if (e == hipSuccess) e = hipStreamSynchronize(s_down);
    }
    std::lock_guard<std::mutex> lock(mu);
    down_err = e;
  });
  hipError_t up_err = hipSuccess;
  int64_t uploaded = 0;      // source rows [0, uploaded) are on the device
  for (int64_t k = 0; k < nb && up_err == hipSuccess; ++k) {
    const int64_t r0 = start[(size_t)k], n = start[(size_t)k + 1] - r0;
    int64_t b0 = 0, b1 = H;
    source_rows(r0, n, &b0, &b1);
    // the source arrives top to bottom; a band whose rows reach further down simply waits for more of it
    // (for the last band everything is uploaded whatever the hull says)
    const int64_t need = (k == nb - 1) ? H : b1;
    if (need > uploaded) {
      up_err = hipMemcpy2DAsync((char*)dsrc + (size_t)uploaded * row_bytes, row_bytes, (const char*)src + (size_t)uploaded * rs_bytes,
                                rs_bytes, row_bytes, (size_t)(need - uploaded), hipMemcpyHostToDevice, s_up);
      uploaded = need;
      if (up_err != hipSuccess) break;
    }
    if (b0 < 0 || b1 > uploaded) { up_err = hipErrorInvalidValue; break; }   // cannot happen: need >= b1
    up_err = launch_band(dsrc, (char*)ddst + (size_t)r0 * row_bytes, r0, n, s_up);
    if (up_err == hipSuccess) up_err = hipEventRecord(band_done[k], s_up);
    if (up_err == hipSuccess && g_host_band_sync.load()) up_err = hipStreamSynchronize(s_up);      // (A/B: rounds 1-5 waited here for every band)
    if (up_err != hipSuccess) break;
    {
      std::lock_guard<std::mutex> lock(mu);
      computed = k + 1;
    }
    cv.notify_all();
  }
  if (up_err != hipSuccess) {
    std::lock_guard<std::mutex> lock(mu);
    abort_down = true;
    cv.notify_all();
  }
  downloader.join();
  // (whatever happened, nothing of this call is left running: the kernels read the staging buffer the next call reuses)
  const hipError_t drain = hipStreamSynchronize(s_up);
  if (up_err != hipSuccess) return fail(DCP_ERR_HIP, "banded frame upload / kernel failed: %s", hipGetErrorString(up_err));
  if (down_err != hipSuccess) return fail(DCP_ERR_HIP, "banded frame download failed: %s", hipGetErrorString(down_err));
  if (drain != hipSuccess) return fail(DCP_ERR_HIP, "banded frame: %s", hipGetErrorString(drain));
  return DCP_OK;
}

// Is [p, p + bytes) host memory the GPU can address (hipHostRegister / hipHostMalloc)?  Returns its device-visible address, or
// nullptr.  BOTH ends are asked about: a view that starts inside a registered range shorter than the frame (a C caller's partly
// registered buffer, a NumPy view past a pinned block) must take the staged path, or the kernels would store to unmapped memory.
void* registered_host_alias(const void* p, size_t bytes) {
  if (!bytes) return nullptr;
  hipPointerAttribute_t first, last;
  memset(&first, 0, sizeof(first));
  memset(&last, 0, sizeof(last));
  if (hipPointerGetAttributes(&first, p) != hipSuccess || hipPointerGetAttributes(&last, (const char*)p + (bytes - 1)) != hipSuccess) {
    (void)hipGetLastError();            // plain pageable memory: not an error
    return nullptr;
  }
  if (first.type != hipMemoryTypeHost || last.type != hipMemoryTypeHost || !first.devicePointer || !last.devicePointer) return nullptr;
  // one mapping from end to end: the device alias advances exactly as the host pointer does
  if ((const char*)last.devicePointer - (const char*)first.devicePointer != (ptrdiff_t)(bytes - 1)) return nullptr;
  return first.devicePointer;
}

// Host frame whose DESTINATION is registered host memory (the recycled outputs of the Python front end are; so is anything a C
// caller got from hipHostMalloc / hipHostRegister): the kernels write their rows straight into it over PCIe -- no device result,
// no download.  The source goes up in bands on one stream; the kernel of band k, on a second stream behind an event, writes band k
// of the result while band k + 1 is uploaded: the upload is the copy engine's, the result the shader's stores, and the two
// directions overlap whatever the runtime does with two copies (the runtime bundled with PyTorch-ROCm serialises those: 2.45 ms
// per 4096^2 frame; this path: see DESIGN.md section 6, round 3).
template <typename Hull, typename LaunchBand>
int run_host_direct(const void* src, void* dst_alias, int64_t H, int64_t W, size_t pix, size_t rs_bytes, Hull&& source_rows,
                    LaunchBand&& launch_band) {
  const size_t row_bytes = (size_t)W * pix;
  void* dsrc = nullptr;
  DCP_HIP(g_staging.get(0, (size_t)H * row_bytes, &dsrc));
  hipStream_t s_up = nullptr, s_k = nullptr;
  DCP_HIP(g_host_streams.get(&s_up, &s_k));
  thread_local hipEvent_t ev[2] = {nullptr, nullptr};
  thread_local int ev_dev = -1;
  int cur = 0;
  DCP_HIP(hipGetDevice(&cur));
  if (ev_dev != cur) {
    for (auto& e : ev) {
      if (e) (void)hipEventDestroy(e);
      e = nullptr;
      DCP_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    ev_dev = cur;
  }
  const int64_t nbands = g_host_bands.load();
  int64_t rows_per = ((H + nbands - 1) / nbands + 63) / 64 * 64;
  if (rows_per > 65535) rows_per = 65535 / 64 * 64;
  const int64_t nb = (H + rows_per - 1) / rows_per;
  // (an error in the middle leaves work queued on both streams that reads the staging buffer and writes the caller's memory:
  // whatever happens, both streams are drained before this function returns)
  const char* what = "";
  auto enqueue = [&]() -> hipError_t {
    int64_t uploaded = 0;
    for (int64_t k = 0; k < nb; ++k) {
      const int64_t r0 = k * rows_per, n = (r0 + rows_per > H ? H - r0 : rows_per);
      int64_t b0 = 0, b1 = H;
      source_rows(r0, n, &b0, &b1);
      const int64_t need = (k == nb - 1) ? H : b1;
      hipError_t e;
      if (need > uploaded) {
        what = "upload of a band";
        e = hipMemcpy2DAsync((char*)dsrc + (size_t)uploaded * row_bytes, row_bytes, (const char*)src + (size_t)uploaded * rs_bytes, rs_bytes, row_bytes,
                             (size_t)(need - uploaded), hipMemcpyHostToDevice, s_up);
        if (e != hipSuccess) return e;
        uploaded = need;
      }
      what = "band hull outside the uploaded rows";
      if (b0 < 0 || b1 > uploaded) return hipErrorInvalidValue;      // cannot happen: need >= b1
      what = "event between the upload and the kernel of a band";
      if ((e = hipEventRecord(ev[k & 1], s_up)) != hipSuccess) return e;
      if ((e = hipStreamWaitEvent(s_k, ev[k & 1], 0)) != hipSuccess) return e;
      what = "kernel of a band";
      if ((e = launch_band(dsrc, (char*)dst_alias + (size_t)r0 * row_bytes, r0, n, s_k)) != hipSuccess) return e;
    }
    return hipSuccess;
  };
  const hipError_t e_enq = enqueue();
  const hipError_t e_up = hipStreamSynchronize(s_up), e_k = hipStreamSynchronize(s_k);
  if (e_enq != hipSuccess) return fail(DCP_ERR_HIP, "host frame written in place: %s failed: %s", what, hipGetErrorString(e_enq));
  if (e_up != hipSuccess || e_k != hipSuccess)
    return fail(DCP_ERR_HIP, "host frame written in place: %s", hipGetErrorString(e_up != hipSuccess ? e_up : e_k));
  return DCP_OK;
}

// Source rows [*b0, *b1) that output rows [r0, r0 + n) of a radial, perspective or fused map can reach (the bands of
// run_host_banded / run_host_direct).  The homography of a banded frame has a denominator of one sign over the frame ("tame",
// MapArgs::fast_div): its position is monotone along every segment, so over a band of output rows it takes its extremes at the
// band's four corners; the fused map then evaluates the radial model inside that clipped rectangle of positions.
void band_source_rows(dcp::MapKind kind, const dcp::MapArgs& map, int64_t H, int64_t W, int64_t r0, int64_t n, int64_t* b0,
                      int64_t* b1) {
  if (kind == dcp::kRadial) {
    host_row_band(map, H, W, (double)r0, n, b0, b1);
    return;
  }
  double ylo = 1e300, yhi = -1e300, xlo = 1e300, xhi = -1e300;
  for (double y : {(double)r0, (double)(r0 + n - 1)})
    for (double x : {0.0, (double)(W - 1)}) {
      const double den = (map.coef[6] * x + map.coef[7] * y) + 1.0;
      double yd = ((map.coef[3] * x + map.coef[4] * y) + map.coef[5]) / den;
      double xd = ((map.coef[0] * x + map.coef[1] * y) + map.coef[2]) / den;
      if (!(yd >= 0.0)) yd = 0.0;
      if (yd > (double)(H - 1)) yd = (double)(H - 1);
      if (!(xd >= 0.0)) xd = 0.0;
      if (xd > (double)(W - 1)) xd = (double)(W - 1);
      ylo = std::min(ylo, yd);
      yhi = std::max(yhi, yd);
      xlo = std::min(xlo, xd);
      xhi = std::max(xhi, xd);
    }
  if (kind == dcp::kFused) {
    // float32 rounding of the perspective position moves it by < 1e-3 px: widen the rectangle a little
    host_row_band_rect(map, H, xlo - 0.01, xhi + 0.01, ylo - 0.01, yhi + 0.01, b0, b1);
    return;
  }
  *b0 = std::max<int64_t>(0, (int64_t)std::floor(ylo) - 1);
  *b1 = std::min<int64_t>(H, (int64_t)std::floor(yhi) + 3);
}

// How a DCP_MEM_HOST frame goes through the GPU.  A large one -- at least kBandRows rows and kBandBytes -- that its executor can run
// in bands of rows travels in bands with uploads and downloads overlapped (run_host_banded, `banded_ok`) where the runtime runs the
// two directions at once (/opt/rocm's: 1.78 ms against 2.15 for the direct path per 4096^2 frame); where it cannot (the one
// bundled with PyTorch-ROCm: 2.16 ms against 2.44) the kernels write into a registered destination directly (run_host_direct,
// `direct_ok`).  "host_direct" / "host_duplex" = 2 force these paths, 0 forbid them.  Everything else is staged whole.
// *alias = the device address of `dst` for kDirect; alias == nullptr asks whether a registered destination would be written directly.
enum HostPath { kStaged, kBanded, kDirect };
constexpr int64_t kBandRows = 512;
constexpr double kBandBytes = 16.0 * 1048576.0;
bool large_host_frame(int64_t H, double bytes) { return H >= kBandRows && bytes >= kBandBytes; }
HostPath host_path(int64_t H, double bytes, bool direct_ok, bool banded_ok, const void* dst, void** alias) {
  if (!large_host_frame(H, bytes)) return kStaged;
  if (direct_ok && g_host_direct.load() && (g_host_direct.load() == 2 || !g_host_duplex.load() || !runtime_overlaps_directions()) &&
      (!alias || (*alias = registered_host_alias(dst, (size_t)bytes))))
    return kDirect;
  if (banded_ok && g_host_duplex.load() && (g_host_duplex.load() == 2 || runtime_overlaps_directions())) return kBanded;
  return kStaged;
}

// The map of a frame call: a perspective or fused map needs its homography, flagged tame (fast_div) over an H x W frame;
// a perspective map takes no radial coefficients, kCoords no map at all.
int frame_map(dcp::MapArgs* m, dcp::MapKind kind, double xc, double yc, const double* fact, int nfact, const double* coef, int64_t H,
              int64_t W) {
  const bool homography = kind == dcp::kPersp || kind == dcp::kFused, radial = kind == dcp::kRadial || kind == dcp::kFused;
  if (homography && !coef) return fail(DCP_ERR_INVALID_ARG, "null homography pointer");
  if (const int rc = fill_map(m, xc, yc, radial ? fact : nullptr, radial ? nfact : 0, homography ? coef : nullptr)) return rc;
  if (homography && H > 0 && W > 0) m->fast_div = homography_is_tame(coef, H, W);
  return DCP_OK;
}

int check_coords(const FrameCall& c) {
  if (c.kind != dcp::kCoords) return DCP_OK;
  if (c.npts < 0) return fail(DCP_ERR_INVALID_ARG, "npts < 0");
  if (c.npts > 0 && (!c.ycoord || !c.xcoord)) return fail(DCP_ERR_INVALID_ARG, "null coordinate pointer");
  if (c.coord_dtype != DCP_COORD_F32 && c.coord_dtype != DCP_COORD_F64) return fail(DCP_ERR_INVALID_ARG, "unknown coord_dtype %d", c.coord_dtype);
  if (c.exec != kExecSpline && c.npts > 2147483647LL * 256) return fail(DCP_ERR_UNSUPPORTED, "too many points");
  return DCP_OK;
}

struct Points {      // kCoords: npts source coordinates (y, x), float32 or float64 (dtype = DCP_COORD_*)
  const void* y;
  const void* x;
  int dtype;
  int64_t npts;
};

// Fills and validates *c, before any device work.  `exec` is the executor the entry point names; a tuned float32 call whose source
// lies beyond 32-bit offsets moves to the generic kernels, a generic call of order 2..5 to the spline path.
int make_frame_call(FrameCall* c, FrameExec exec, dcp::MapKind kind, const void* src, void* dst, int dtype, int64_t H, int64_t W,
                    int64_t rs, int64_t cs, int channels, double xc, double yc, const double* fact, int nfact, const double* coef,
                    Points pts, int order, int blend_mode, int mode, int round_f32, int mem_kind, int device, void* stream) {
  int rc;
  // DCP_MEM_DEVICE_UNORDERED: the tuned whole-image entry points only.  A launch leaves unordered only on device memory: a host
  // call's kernels sit right behind its own uploads, whatever the lab switch "x_any_order" says
  bool unordered = false;
  if ((rc = mem_kind_of(mem_kind, &c->host, exec == kExecTuned && kind != dcp::kCoords ? &unordered : nullptr)) != DCP_OK) return rc;
  c->opts = current_opts();
  if (c->host || unordered) c->opts.any_order = unordered;
  if ((rc = frame_map(&c->map, kind, xc, yc, fact, nfact, coef, H, W)) != DCP_OK) return rc;
  c->exec = exec;
  c->kind = kind;
  c->src = src;
  c->dst = dst;
  c->dtype = dtype;
  c->H = H;
  c->W = W;
  c->rs = rs;
  c->cs = cs;
  c->channels = channels;
  c->ycoord = pts.y;
  c->xcoord = pts.x;
  c->coord_dtype = pts.dtype;
  c->npts = pts.npts;
  c->order = order;
  c->sampler = dcp::kScipy;
  c->mode = mode;
  c->exact_sum = 0;
  c->round_f32 = round_f32 != 0;
  c->device = device;
  c->stream = (hipStream_t)stream;
  const bool cert = g_tile_cert.load() != 0;
  if (exec == kExecForward) {
    // the scatter moves elements of any type; its winner plane indexes pixels with 32 bits (0 = vacant)
    if ((rc = check_image_typed(src, dst, dtype, H, W, rs, cs)) != DCP_OK) return rc;
    if ((double)H * (double)W >= 4294967295.0)
      return fail(DCP_ERR_UNSUPPORTED, "forward unwarp of %lld x %lld pixels: the winner plane indexes at most 2^32 - 2 of them", (long long)H,
                  (long long)W);
    const char *s0 = (const char*)src, *s1 = s0 + extent_bytes_typed(H, W, rs, cs, dtype);
    const char *d0 = (const char*)dst, *d1 = d0 + (size_t)H * (size_t)W * (size_t)dcp::elem_size(dtype);
    if (s0 < d1 && d0 < s1) return fail(DCP_ERR_INVALID_ARG, "source and destination overlap: a scatter cannot run in place");
    return DCP_OK;
  }
  if (exec == kExecColour) {
    if (channels < 1 || channels > 64) return fail(DCP_ERR_INVALID_ARG, "channels = %d outside [1, 64]", channels);
    if (order < 0 || order > 1) return fail(DCP_ERR_UNSUPPORTED, "the interleaved-channel kernels take orders 0 and 1 (got %d)", order);
    if (blend_mode != DCP_BLEND_SCIPY && blend_mode != DCP_BLEND_F64LERP)
      return fail(DCP_ERR_UNSUPPORTED, "interleaved channels blend as scipy does (DCP_BLEND_SCIPY) or within one ulp of it (DCP_BLEND_F64LERP); got %d", blend_mode);
    if (cs < channels) return fail(DCP_ERR_INVALID_ARG, "pixel stride %lld smaller than %d channels", (long long)cs, channels);
    if ((rc = check_image_typed(src, dst, dtype, H, W, rs, cs)) != DCP_OK) return rc;
    if (rs < (W - 1) * cs + channels && H > 1)
      return fail(DCP_ERR_INVALID_ARG, "row stride %lld overlaps rows of %lld pixels", (long long)rs, (long long)W);
    // float32 only: the one-ulp factorisation; integer types always blend in scipy's exact order (their rounding ties depend on it)
    c->sampler = order == 0 ? dcp::kNearest : (blend_mode == DCP_BLEND_F64LERP && dtype == dcp::kF32 ? dcp::kF64Lerp : dcp::kScipy);
    if (kind == dcp::kRadial) c->map.tile_dev_ok = cert ? tile_deviation_certified(dcp::kRadial, c->map, H, W) : 0;
    else c->map.tile_dev_ok = cert && (kind != dcp::kFused || g_fused_wg.load()) && colour_boxes_fit(kind, c->map, H, W) ? 2 : 0;
    return DCP_OK;
  }
  if (exec == kExecColourSpline) {
    // interleaved channels at orders 2..5: the ranges of the colour entry points and of the typed spline entry points together; the
    // element type, order, boundary mode and size checks of the single-plane spline call follow below
    if (channels < 1 || channels > 4) return fail(DCP_ERR_INVALID_ARG, "channels = %d outside [1, 4] (the spline orders on interleaved channels)", channels);
    if (cs < channels) return fail(DCP_ERR_INVALID_ARG, "pixel stride %lld smaller than %d channels", (long long)cs, channels);
    if ((rc = check_image_typed(src, dst, dtype, H, W, rs, cs)) != DCP_OK) return rc;
    if (rs < (W - 1) * cs + channels && H > 1)
      return fail(DCP_ERR_INVALID_ARG, "row stride %lld overlaps rows of %lld pixels", (long long)rs, (long long)W);
  }
  if (exec == kExecTuned) {
    if (kind == dcp::kCoords && (mode < 0 || mode > 7)) return fail(DCP_ERR_INVALID_ARG, "unknown boundary mode %d", mode);
    if ((rc = sampler_of(order, blend_mode, &c->sampler)) != DCP_OK) return rc;
    if (!(round_f32 && beyond_32bit_offsets(H, W, rs, cs))) {
      if ((rc = check_image(src, dst, H, W, rs, cs)) != DCP_OK) return rc;
      if (cert && kind != dcp::kCoords && (kind != dcp::kFused || g_fused_wg.load())) {
        int tall = 0;
        c->map.tile_dev_ok = tile_deviation_certified(kind, c->map, H, W, kind == dcp::kRadial ? &tall : nullptr);
        c->map.tall_ok = tall;
      }
      return check_coords(*c);
    }
    c->exec = exec = kExecTyped;
  }
  if (exec == kExecTyped) {
    if (order < 0 || order > 5) return fail(DCP_ERR_INVALID_ARG, "spline order %d outside [0, 5]", order);
    if (mode < 0 || (mode & ~DCP_SPLINE_SCIPY_SUM) > 7) return fail(DCP_ERR_INVALID_ARG, "unknown boundary mode %d", mode);
    if (order < 2) {
      c->mode = mode & ~DCP_SPLINE_SCIPY_SUM;        // (orders 0 / 1 of the typed entry points always blend in scipy's order)
      if ((rc = check_image_typed(src, dst, dtype, H, W, rs, cs)) != DCP_OK) return rc;
      return check_coords(*c);
    }
    c->exec = kExecSpline;
  }
  if ((rc = check_image_typed(src, dst, dtype, H, W, rs, cs)) != DCP_OK) return rc;
  if (order < 2 || order > 5) return fail(DCP_ERR_INVALID_ARG, "spline order %d outside [2, 5]", order);
  // bit 8 of boundary_mode (DCP_SPLINE_SCIPY_SUM): accumulate the taps in scipy's operation order instead of the factorised sum
  c->exact_sum = (mode >= 0 && (mode & DCP_SPLINE_SCIPY_SUM)) ? 1 : 0;
  if (mode >= 0) c->mode = mode &= ~DCP_SPLINE_SCIPY_SUM;
  if (mode < 0 || mode > 7) return fail(DCP_ERR_INVALID_ARG, "unknown boundary mode %d", mode);
  if ((rc = check_coords(*c)) != DCP_OK) return rc;
  if (H > 1000000 || W > 1000000) return fail(DCP_ERR_UNSUPPORTED, "image too large for the spline path");
  // the host's tile-deviation certificate lets the gather stage its taps in LDS (spline_wg_kernel)
  if (cert && (kind == dcp::kRadial || kind == dcp::kPersp)) c->map.tile_dev_ok = tile_deviation_certified(kind, c->map, H, W);
  return DCP_OK;
}

// Output rows [y0, y0 + rows) of the frame (rows = 0: all of it) from the source at `src` (strides rs / cs in elements; kCoords:
// the points at y / x) into `dst` on stream `s`: the launch of every memory path of run_frame.
hipError_t launch_frame(const FrameCall& c, const void* src, void* dst, const void* y, const void* x, int64_t rs, int64_t cs, int64_t y0,
                        int64_t rows, hipStream_t s) {
  dcp::ImageArgs img;
  memset(&img, 0, sizeof(img));
  img.H = (int32_t)c.H;
  img.W = (int32_t)c.W;
  img.src = (const float*)src;
  img.dst = (float*)dst;
  img.src_stride = (int32_t)rs;
  img.src_col_stride = (int32_t)cs;
  dcp::CoordArgs ca;
  memset(&ca, 0, sizeof(ca));
  ca.ycoord = y;
  ca.xcoord = x;
  ca.npts = c.npts;
  ca.is_f64 = c.coord_dtype == DCP_COORD_F64;
  ca.mode = c.mode;
  if (c.exec == kExecTuned) {
    img.src_bytes = extent_bytes(c.H, c.W, rs, cs);
    img.y_origin = (int32_t)y0;
    img.rows_out = (int32_t)rows;
    if (c.kind == dcp::kCoords) return dcp::launch_coords(img, ca, c.sampler, s);
    return dcp::launch_image(c.kind, img, c.map, c.sampler, c.round_f32 != 0, c.opts, s);
  }
  dcp::TypedImageArgs a;
  memset(&a, 0, sizeof(a));
  a.src = src;
  a.dst = dst;
  a.H = (int32_t)c.H;
  a.W = (int32_t)c.W;
  a.src_stride = rs;
  a.src_cstride = cs;
  a.order = c.order;
  a.dtype = c.dtype;
  bool taken = false;
  if (c.exec == kExecColour) {
    // the workgroup-box kernel (remap_wg_color_kernel) where the call qualifies -- dense pixels of 3 / 4 channels, float32 / uint8 /
    // uint16, map of any kind certified --, else one thread per pixel
    const double ext = ((double)(c.H - 1) * (double)rs + (double)(c.W - 1) * (double)cs + (double)c.channels) * (double)dcp::elem_size(c.dtype);
    a.blend = c.sampler;
    a.y0 = (int32_t)y0;
    a.rows = (int32_t)(rows ? rows : c.H);
    if (ext <= 4294900000.0 && rs < (1ll << 31)) {
      img.src_bytes = (uint32_t)ext;
      img.y_origin = a.y0;
      img.rows_out = a.rows;
      const hipError_t e = dcp::launch_color(c.kind, img, c.map, c.channels, c.dtype, c.sampler, c.opts, s, &taken);
      if (e != hipSuccess || taken) return e;
    }
    return dcp::launch_typed_channels(c.kind, a, c.map, c.channels, s);
  }
  // 8- / 16-bit integers, radial or perspective map, certified: the workgroup-box kernel (same arithmetic, LDS-staged); 4- and
  // 8-byte element types under a radial map: the interleaved-pixel kernel with one channel (color_kernels.hip)
  if ((c.kind == dcp::kRadial || c.kind == dcp::kPersp) && cs == 1 && (double)extent_bytes_typed(c.H, c.W, rs, 1, c.dtype) <= 4294900000.0) {
    dcp::MapArgs mapc = c.map;
    mapc.tile_dev_ok = g_tile_cert.load() ? tile_deviation_certified(c.kind, mapc, c.H, c.W) : 0;
    if (c.kind == dcp::kPersp) mapc.fast_div = homography_is_tame(mapc.coef, c.H, c.W);
    img.src_bytes = (uint32_t)extent_bytes_typed(c.H, c.W, rs, 1, c.dtype);
    img.xcd_remap = c.opts.xcd_remap;
    const hipError_t e = c.kind == dcp::kRadial && (c.dtype == dcp::kF64 || c.dtype == dcp::kI32 || c.dtype == dcp::kU32)
                             ? dcp::launch_color(dcp::kRadial, img, mapc, 1, c.dtype, c.order == 0 ? dcp::kNearest : dcp::kScipy, c.opts, s, &taken)
                             : dcp::launch_wg_typed(c.kind, img, mapc, c.order, c.dtype, c.opts, s, &taken);
    if (e != hipSuccess || taken) return e;
  }
  return dcp::launch_typed_image(c.kind, a, c.map, ca, s);
}

// Executes a validated FrameCall: device memory in one launch on the caller's stream; host memory in bands (large dense frames
// of the tuned image kernels and of interleaved channels, host_path) or staged whole.
int run_frame(const FrameCall& c) {
  if (c.kind == dcp::kCoords && c.npts == 0) return DCP_OK;
  DeviceScope scope(c.device);
  if (scope.status != hipSuccess) return fail(DCP_ERR_HIP, "cannot select device %d: %s", c.device, hipGetErrorString(scope.status));
  if (c.exec == kExecSpline) return run_spline(c);
  if (c.exec == kExecColourSpline) return run_spline_color(c);
  if (c.exec == kExecFramesSpline) return run_spline_frames(c);
  if (c.exec == kExecForward) return run_forward(c);
  if (!c.host) {
    DCP_HIP(launch_frame(c, c.src, c.dst, c.ycoord, c.xcoord, c.rs, c.cs, 0, 0, c.stream));
    return DCP_OK;
  }
  const size_t esz = (size_t)dcp::elem_size(c.dtype), pix = (size_t)c.channels * esz;
  const bool tuned_image = c.exec == kExecTuned && c.kind != dcp::kCoords;
  if (tuned_image || c.exec == kExecColour) {
    const bool dense = tuned_image ? c.cs == 1 && c.W >= 2 : c.cs == c.channels;
    // radial float32 bands go through the stack kernel (a band of image rows = a chunk of rows of a one-projection stack)
    // (interleaved channels under a homography travel in bands only when it is tame: band_source_rows takes the band's hull from its corners)
    const bool stack_bands = tuned_image && c.kind == dcp::kRadial && c.sampler != dcp::kNearest && c.round_f32;
    void* alias = nullptr;
    const HostPath path = host_path(c.H, (double)c.H * (double)c.W * (double)pix, dense && tuned_image && (c.kind == dcp::kRadial || c.map.fast_div),
                                    dense && (tuned_image ? stack_bands || (c.kind != dcp::kRadial && c.map.fast_div) : c.kind == dcp::kRadial || c.map.fast_div),
                                    c.dst, &alias);
    auto hull = [&](int64_t r0, int64_t n, int64_t* b0, int64_t* b1) { band_source_rows(c.kind, c.map, c.H, c.W, r0, n, b0, b1); };
    auto band = [&](void* dsrc, void* dband, int64_t r0, int64_t n, hipStream_t s) {
      return launch_frame(c, dsrc, dband, nullptr, nullptr, c.W * c.channels, c.channels, r0, n, s);
    };
    if (path == kDirect) return run_host_direct(c.src, alias, c.H, c.W, pix, (size_t)c.rs * esz, hull, band);
    if (path == kBanded && stack_bands)
      return run_host_banded(c.src, c.dst, c.H, c.W, pix, (size_t)c.rs * esz, hull, [&](void* dsrc, void* dband, int64_t r0, int64_t n, hipStream_t s) {
        dcp::StackArgs st;
        memset(&st, 0, sizeof(st));
        st.D = 1;
        st.H = (int32_t)c.H;
        st.W = (int32_t)c.W;
        st.row_start = (double)r0;
        st.nrows = (int32_t)n;
        st.vol = (const float*)dsrc;
        st.out = (float*)dband;
        st.proj_stride = c.H * c.W;
        st.row_stride = (int32_t)c.W;
        st.proj_bytes = (uint32_t)((size_t)c.H * (size_t)c.W * 4);
        return dcp::launch_stack(st, c.map, c.sampler, true, c.opts, s);
      });
    if (path == kBanded) return run_host_banded(c.src, c.dst, c.H, c.W, pix, (size_t)c.rs * esz, hull, band);
  }
  // staged whole: dense float32 rows packed on the way in, anything else as the extent it spans (the kernel's strided gather picks
  // a column-strided view's elements: one channel of an interleaved image)
  const bool pack = tuned_image && c.cs == 1;
  HostTrip t;
  t.src = c.src;
  t.row_bytes = pack ? (size_t)c.W * esz : (size_t)((c.H - 1) * c.rs + (c.W - 1) * c.cs + c.channels) * esz;
  t.rows = pack ? (size_t)c.H : 1;
  t.pitch = pack ? (size_t)c.rs * esz : t.row_bytes;
  if (c.kind == dcp::kCoords) {
    t.y_up = c.ycoord;
    t.x_up = c.xcoord;
    t.plane = (size_t)c.npts * (c.coord_dtype == DCP_COORD_F64 ? 8 : 4);
  }
  t.dst = c.dst;
  t.out_bytes = (size_t)(c.kind == dcp::kCoords ? c.npts : c.H * c.W * c.channels) * esz;
  return host_round_trip(t, c.stream, [&](const void* dsrc, void* ddst, void* dy, void* dx) {
    return launch_frame(c, dsrc, ddst, dy, dx, pack ? c.W : c.rs, pack ? 1 : c.cs, 0, 0, c.stream);
  });
}

// the two dcp_map_points_* entry points: npts (y, x) pairs through a radial or perspective map, float64
int map_points(dcp::MapKind kind, const double* yx_in, double* yx_out, int64_t npts, double xc, double yc, const double* fact, int nfact,
               const double* coef, int mem_kind, int device, void* stream) {
  int rc;
  bool host = false;
  if ((rc = mem_kind_of(mem_kind, &host)) != DCP_OK) return rc;
  if (npts < 0) return fail(DCP_ERR_INVALID_ARG, "npts < 0");
  if (npts > 0 && (!yx_in || !yx_out)) return fail(DCP_ERR_INVALID_ARG, "null point pointer");
  dcp::MapArgs map;
  if ((rc = frame_map(&map, kind, xc, yc, fact, nfact, coef, 0, 0)) != DCP_OK) return rc;
  if (npts == 0) return DCP_OK;
  DeviceScope scope(device);
  if (scope.status != hipSuccess) return fail(DCP_ERR_HIP, "cannot select device %d: %s", device, hipGetErrorString(scope.status));
  hipStream_t st = (hipStream_t)stream;
  auto launch = [&](const void* in, void* out) {
    return kind == dcp::kRadial ? dcp::launch_map_points((const double*)in, (double*)out, npts, map, st)
                                : dcp::launch_map_points_persp((const double*)in, (double*)out, npts, map, st);
  };
  if (!host) {
    DCP_HIP(launch(yx_in, yx_out));
    return DCP_OK;
  }
  HostTrip t;
  t.src = yx_in;
  t.row_bytes = t.pitch = t.out_bytes = (size_t)npts * 16;
  t.dst = yx_out;
  return host_round_trip(t, st, [&](const void* din, void* dout, void*, void*) { return launch(din, dout); });
}

// dcp_map_points_inverse_f64: as map_points, with the count of points without a root delivered where the points live
int map_points_inverse(const double* yx_in, double* yx_out, int64_t npts, double xc, double yc, const double* fact, int nfact,
                       int64_t* n_unsolved, int mem_kind, int device, void* stream) {
  int rc;
  bool host = false;
  if ((rc = mem_kind_of(mem_kind, &host)) != DCP_OK) return rc;
  if (npts < 0) return fail(DCP_ERR_INVALID_ARG, "npts < 0");
  if (npts > 0 && (!yx_in || !yx_out)) return fail(DCP_ERR_INVALID_ARG, "null point pointer");
  dcp::MapArgs map;
  if ((rc = frame_map(&map, dcp::kRadial, xc, yc, fact, nfact, nullptr, 0, 0)) != DCP_OK) return rc;
  if (npts == 0 && (host || !n_unsolved)) {
    if (n_unsolved) *n_unsolved = 0;
    return DCP_OK;
  }
  DeviceScope scope(device);
  if (scope.status != hipSuccess) return fail(DCP_ERR_HIP, "cannot select device %d: %s", device, hipGetErrorString(scope.status));
  hipStream_t st = (hipStream_t)stream;
  static_assert(sizeof(unsigned long long) == sizeof(int64_t), "counter width");
  auto launch = [&](const void* in, void* out, void* count) -> hipError_t {
    if (count) {
      const hipError_t e = hipMemsetAsync(count, 0, sizeof(int64_t), st);
      if (e != hipSuccess) return e;
    }
    return dcp::launch_map_points_inverse((const double*)in, (double*)out, npts, map, (unsigned long long*)count, st);
  };
  if (!host) {
    DCP_HIP(launch(yx_in, yx_out, n_unsolved));
    return DCP_OK;
  }
  int64_t count = 0, unused = 0;
  HostTrip t;
  t.src = yx_in;
  t.row_bytes = t.pitch = t.out_bytes = (size_t)npts * 16;
  t.dst = yx_out;
  t.y_down = &count;                     // the counter travels as an 8-byte plane (slot 2; slot 3 comes back unread)
  t.x_down = &unused;
  t.plane = sizeof(int64_t);
  rc = host_round_trip(t, st, [&](const void* din, void* dout, void* dcount, void*) { return launch(din, dout, dcount); });
  if (rc == DCP_OK && n_unsolved) *n_unsolved = count;
  return rc;
}

}  // namespace

namespace dcpapi {
bool host_direct_applies() { return host_path(kBandRows, kBandBytes, true, false, nullptr, nullptr) == kDirect; }
}  // namespace dcpapi

extern "C" {

int dcp_unwarp_image_f32(const float* src, float* dst, int64_t height, int64_t width, int64_t src_row_stride,
                         int64_t src_col_stride, double xcenter, double ycenter, const double* list_fact,
                         int nfact, int order, int coord_round_f32, int blend_mode, int mem_kind, int device,
                         void* stream) {
  FrameCall c;
  const int rc = make_frame_call(&c, kExecTuned, dcp::kRadial, src, dst, dcp::kF32, height, width, src_row_stride, src_col_stride, 1,
                                 xcenter, ycenter, list_fact, nfact, nullptr, Points{}, order, blend_mode, 0, coord_round_f32, mem_kind,
                                 device, stream);
  return rc != DCP_OK ? rc : run_frame(c);
}

int dcp_unwarp_images_f32(const float* const* srcs, float* const* dsts, int nframes, int64_t height, int64_t width,
                          int64_t src_row_stride, int64_t src_col_stride, const double* xcenters, const double* ycenters,
                          const double* list_facts, int nfact, int order, int coord_round_f32, int blend_mode, int mem_kind,
                          int device, void* stream) {
  int rc, sampler;
  bool host = false, unordered = false;     // (DCP_MEM_DEVICE_UNORDERED: frame by frame, every launch unordered)
  if ((rc = mem_kind_of(mem_kind, &host, &unordered)) != DCP_OK) return rc;
  if (nframes < 0) return fail(DCP_ERR_INVALID_ARG, "nframes < 0");
  if (nframes == 0) return DCP_OK;
  if (!srcs || !dsts || !xcenters || !ycenters) return fail(DCP_ERR_INVALID_ARG, "null frame / centre array");
  if (nfact < 0 || nfact > dcp::kMaxFact)
    return fail(DCP_ERR_INVALID_ARG, "nfact = %d outside [0, %d] (DCP_MAX_FACT is a limit of this library, not of the reference)", nfact, dcp::kMaxFact);
  if (nfact > 0 && !list_facts) return fail(DCP_ERR_INVALID_ARG, "null coefficient pointer");
  if ((rc = sampler_of(order, blend_mode, &sampler)) != DCP_OK) return rc;
  auto one_by_one = [&](int first) {      // frames first .. nframes-1 through the single-frame entry point
    for (int i = first; i < nframes; ++i) {
      const int r = dcp_unwarp_image_f32(srcs[i], dsts[i], height, width, src_row_stride, src_col_stride, xcenters[i], ycenters[i],
                                         list_facts ? list_facts + (size_t)i * (size_t)nfact : nullptr, nfact, order, coord_round_f32,
                                         blend_mode, mem_kind, device, stream);
      if (r != DCP_OK) return r;
    }
    return DCP_OK;
  };
  // host frames are bound by PCIe: each goes through the single-frame host path (bands of rows, uploads and downloads
  // overlapped); float64 coordinates and sources beyond 32-bit offsets have no multi-frame kernel either
  if (host || unordered || !coord_round_f32 || nframes == 1 || nfact > 10 ||
      beyond_32bit_offsets(height, width, src_row_stride, src_col_stride))
    return one_by_one(0);
  for (int i = 0; i < nframes; ++i)
    if ((rc = check_image(srcs[i], dsts[i], height, width, src_row_stride, src_col_stride)) != DCP_OK) return rc;
  // Frames of ONE calibration, evenly spaced, results dense -- a (n, height, width) array, which is what the reference's callers
  // loop over (the channels of demo_06.py:111-113, the frames of demo_07.py:25,60): the projections of a stack, every row wanted.
  if (order == 1 && src_col_stride == 1) {
    bool same = true;
    const ptrdiff_t pitch = srcs[1] - srcs[0];
    const int64_t extent = (height - 1) * src_row_stride + width;
    for (int i = 1; i < nframes && same; ++i)
      same = xcenters[i] == xcenters[0] && ycenters[i] == ycenters[0] && srcs[i] - srcs[i - 1] == pitch &&
             dsts[i] - dsts[i - 1] == (ptrdiff_t)(height * width) &&
             (nfact == 0 || memcmp(list_facts + (size_t)i * (size_t)nfact, list_facts, (size_t)nfact * sizeof(double)) == 0);
    if (same && (int64_t)pitch >= extent) {
      bool taken = false;
      rc = frames_as_stack(srcs[0], dsts[0], nframes, height, width, (int64_t)pitch, src_row_stride, xcenters[0], ycenters[0],
                           list_facts, nfact, blend_mode, device, stream, &taken);
      if (rc != DCP_OK || taken) return rc;
    }
  }
  // every frame's calibration must hold the level-2 tile certificate (one box per 128 x 32 workgroup tile)
  std::vector<dcp::BatchFrame> fr((size_t)nframes);
  bool all_certified = g_tile_cert.load() != 0;
  for (int i = 0; i < nframes && all_certified; ++i) {
    dcp::MapArgs map;
    const double* f = list_facts ? list_facts + (size_t)i * (size_t)nfact : nullptr;
    if ((rc = fill_map(&map, xcenters[i], ycenters[i], f, nfact, nullptr)) != DCP_OK) return rc;
    all_certified = tile_deviation_certified(dcp::kRadial, map, height, width) >= 2;
    fr[(size_t)i] = dcp::BatchFrame{srcs[i], dsts[i], xcenters[i], ycenters[i], f};
  }
  if (!all_certified) return one_by_one(0);
  DeviceScope scope(device);
  if (scope.status != hipSuccess) return fail(DCP_ERR_HIP, "cannot select device %d: %s", device, hipGetErrorString(scope.status));
  dcp::ImageArgs img;
  memset(&img, 0, sizeof(img));
  img.H = (int32_t)height;
  img.W = (int32_t)width;
  img.src_stride = (int32_t)src_row_stride;
  img.src_col_stride = (int32_t)src_col_stride;
  img.src_bytes = extent_bytes(height, width, src_row_stride, src_col_stride);
  bool taken = false;
  DCP_HIP(dcp::launch_image_batch(img, fr.data(), nframes, nfact, sampler, current_opts(), (hipStream_t)stream, &taken));
  return taken ? DCP_OK : one_by_one(0);
}

int dcp_perspective_image_f32(const float* src, float* dst, int64_t height, int64_t width,
                              int64_t src_row_stride, int64_t src_col_stride, const double* list_coef,
                              int order, int blend_mode, int mem_kind, int device, void* stream) {
  FrameCall c;
  const int rc = make_frame_call(&c, kExecTuned, dcp::kPersp, src, dst, dcp::kF32, height, width, src_row_stride, src_col_stride, 1, 0.0,
                                 0.0, nullptr, 0, list_coef, Points{}, order, blend_mode, 0, 1, mem_kind, device, stream);
  return rc != DCP_OK ? rc : run_frame(c);
}

int dcp_unwarp_fused_f32(const float* src, float* dst, int64_t height, int64_t width, int64_t src_row_stride,
                         int64_t src_col_stride, double xcenter, double ycenter, const double* list_fact,
                         int nfact, const double* list_coef, int order, int blend_mode, int mem_kind,
                         int device, void* stream) {
  FrameCall c;
  const int rc = make_frame_call(&c, kExecTuned, dcp::kFused, src, dst, dcp::kF32, height, width, src_row_stride, src_col_stride, 1,
                                 xcenter, ycenter, list_fact, nfact, list_coef, Points{}, order, blend_mode, 0, 1, mem_kind, device, stream);
  return rc != DCP_OK ? rc : run_frame(c);
}

int dcp_remap_coords_f32(const float* src, float* dst, int64_t height, int64_t width, int64_t src_row_stride,
                         int64_t src_col_stride, const void* ycoord, const void* xcoord, int coord_dtype,
                         int64_t npts, int order, int blend_mode, int mem_kind, int device, void* stream) {
  return dcp_remap_coords_mode_f32(src, dst, height, width, src_row_stride, src_col_stride, ycoord, xcoord, coord_dtype, npts, order,
                                   dcp::kModeNearest, blend_mode, mem_kind, device, stream);
}

int dcp_remap_coords_mode_f32(const float* src, float* dst, int64_t height, int64_t width, int64_t src_row_stride,
                              int64_t src_col_stride, const void* ycoord, const void* xcoord, int coord_dtype,
                              int64_t npts, int order, int boundary_mode, int blend_mode, int mem_kind, int device, void* stream) {
  FrameCall c;
  const int rc = make_frame_call(&c, kExecTuned, dcp::kCoords, src, dst, dcp::kF32, height, width, src_row_stride, src_col_stride, 1, 0.0,
                                 0.0, nullptr, 0, nullptr, Points{ycoord, xcoord, coord_dtype, npts}, order, blend_mode, boundary_mode, 1,
                                 mem_kind, device, stream);
  return rc != DCP_OK ? rc : run_frame(c);
}

int dcp_unwarp_image_typed(const void* src, void* dst, int dtype, int64_t height, int64_t width, int64_t src_row_stride,
                           int64_t src_col_stride, double xcenter, double ycenter, const double* list_fact, int nfact,
                           int order, int boundary_mode, int mem_kind, int device, void* stream) {
  // a large dense host frame, orders 0 / 1: the one-channel case of the interleaved entry point, whose host path moves
  // the frame in bands of rows with uploads and downloads overlapped (same arithmetic: scipy's exact blend)
  if (mem_kind == DCP_MEM_HOST && order >= 0 && order <= 1 && boundary_mode >= 0 && boundary_mode <= 7 && src_col_stride == 1 && dtype >= 0 &&
      dtype < dcp::kNumElemTypes && large_host_frame(height, (double)height * (double)width * (double)dcp::elem_size(dtype)))
    return dcp_unwarp_image_channels(src, dst, dtype, height, width, 1, src_row_stride, 1, xcenter, ycenter, list_fact, nfact,
                                     order, mem_kind, device, stream);
  FrameCall c;
  const int rc = make_frame_call(&c, kExecTyped, dcp::kRadial, src, dst, dtype, height, width, src_row_stride, src_col_stride, 1, xcenter,
                                 ycenter, list_fact, nfact, nullptr, Points{}, order, DCP_BLEND_SCIPY, boundary_mode, 1, mem_kind, device,
                                 stream);
  return rc != DCP_OK ? rc : run_frame(c);
}

int dcp_perspective_image_typed(const void* src, void* dst, int dtype, int64_t height, int64_t width,
                                int64_t src_row_stride, int64_t src_col_stride, const double* list_coef, int order,
                                int boundary_mode, int mem_kind, int device, void* stream) {
  FrameCall c;
  const int rc = make_frame_call(&c, kExecTyped, dcp::kPersp, src, dst, dtype, height, width, src_row_stride, src_col_stride, 1, 0.0, 0.0,
                                 nullptr, 0, list_coef, Points{}, order, DCP_BLEND_SCIPY, boundary_mode, 1, mem_kind, device, stream);
  return rc != DCP_OK ? rc : run_frame(c);
}

int dcp_unwarp_fused_typed(const void* src, void* dst, int dtype, int64_t height, int64_t width, int64_t src_row_stride,
                           int64_t src_col_stride, double xcenter, double ycenter, const double* list_fact, int nfact,
                           const double* list_coef, int order, int boundary_mode, int mem_kind, int device, void* stream) {
  FrameCall c;
  const int rc = make_frame_call(&c, kExecTyped, dcp::kFused, src, dst, dtype, height, width, src_row_stride, src_col_stride, 1, xcenter,
                                 ycenter, list_fact, nfact, list_coef, Points{}, order, DCP_BLEND_SCIPY, boundary_mode, 1, mem_kind, device,
                                 stream);
  return rc != DCP_OK ? rc : run_frame(c);
}

int dcp_remap_coords_typed(const void* src, void* dst, int dtype, int64_t height, int64_t width, int64_t src_row_stride,
                           int64_t src_col_stride, const void* ycoord, const void* xcoord, int coord_dtype, int64_t npts,
                           int order, int boundary_mode, int mem_kind, int device, void* stream) {
  FrameCall c;
  const int rc = make_frame_call(&c, kExecTyped, dcp::kCoords, src, dst, dtype, height, width, src_row_stride, src_col_stride, 1, 0.0, 0.0,
                                 nullptr, 0, nullptr, Points{ycoord, xcoord, coord_dtype, npts}, order, DCP_BLEND_SCIPY, boundary_mode, 1,
                                 mem_kind, device, stream);
  return rc != DCP_OK ? rc : run_frame(c);
}

int dcp_unwarp_image_channels(const void* src, void* dst, int dtype, int64_t height, int64_t width, int channels,
                              int64_t src_row_stride, int64_t src_pixel_stride, double xcenter, double ycenter,
                              const double* list_fact, int nfact, int order, int mem_kind, int device, void* stream) {
  return dcp_unwarp_color_image(src, dst, dtype, height, width, channels, src_row_stride, src_pixel_stride, xcenter, ycenter, list_fact, nfact,
                                order, DCP_BLEND_SCIPY, mem_kind, device, stream);
}

int dcp_unwarp_color_image(const void* src, void* dst, int dtype, int64_t height, int64_t width, int channels, int64_t src_row_stride,
                           int64_t src_pixel_stride, double xcenter, double ycenter, const double* list_fact, int nfact, int order,
                           int blend_mode, int mem_kind, int device, void* stream) {
  FrameCall c;
  const int rc = make_frame_call(&c, kExecColour, dcp::kRadial, src, dst, dtype, height, width, src_row_stride, src_pixel_stride, channels,
                                 xcenter, ycenter, list_fact, nfact, nullptr, Points{}, order, blend_mode, 0, 1, mem_kind, device, stream);
  return rc != DCP_OK ? rc : run_frame(c);
}

int dcp_perspective_color_image(const void* src, void* dst, int dtype, int64_t height, int64_t width, int channels, int64_t src_row_stride,
                                int64_t src_pixel_stride, const double* list_coef, int order, int blend_mode, int mem_kind, int device,
                                void* stream) {
  FrameCall c;
  const int rc = make_frame_call(&c, kExecColour, dcp::kPersp, src, dst, dtype, height, width, src_row_stride, src_pixel_stride, channels, 0.0,
                                 0.0, nullptr, 0, list_coef, Points{}, order, blend_mode, 0, 1, mem_kind, device, stream);
  return rc != DCP_OK ? rc : run_frame(c);
}

int dcp_unwarp_fused_color_image(const void* src, void* dst, int dtype, int64_t height, int64_t width, int channels, int64_t src_row_stride,
                                 int64_t src_pixel_stride, double xcenter, double ycenter, const double* list_fact, int nfact,
                                 const double* list_coef, int order, int blend_mode, int mem_kind, int device, void* stream) {
  FrameCall c;
  const int rc = make_frame_call(&c, kExecColour, dcp::kFused, src, dst, dtype, height, width, src_row_stride, src_pixel_stride, channels,
                                 xcenter, ycenter, list_fact, nfact, list_coef, Points{}, order, blend_mode, 0, 1, mem_kind, device, stream);
  return rc != DCP_OK ? rc : run_frame(c);
}

// The three colour entry points at spline orders 2..5.  Each channel's result is that of the single-plane call on its view, down to the
// homography's division: the float32 single-plane spline entry point divides plainly, the typed one with the refined reciprocal where
// the homography is tame (dcp_perspective_image_spline_f32 above) -- the same choice is made here from the element type.
int dcp_unwarp_color_image_spline(const void* src, void* dst, int dtype, int64_t height, int64_t width, int channels, int64_t src_row_stride,
                                  int64_t src_pixel_stride, double xcenter, double ycenter, const double* list_fact, int nfact, int order,
                                  int boundary_mode, int mem_kind, int device, void* stream) {
  FrameCall c;
  const int rc = make_frame_call(&c, kExecColourSpline, dcp::kRadial, src, dst, dtype, height, width, src_row_stride, src_pixel_stride, channels,
                                 xcenter, ycenter, list_fact, nfact, nullptr, Points{}, order, DCP_BLEND_SCIPY, boundary_mode, 1, mem_kind, device,
                                 stream);
  return rc != DCP_OK ? rc : run_frame(c);
}

int dcp_perspective_color_image_spline(const void* src, void* dst, int dtype, int64_t height, int64_t width, int channels,
                                       int64_t src_row_stride, int64_t src_pixel_stride, const double* list_coef, int order, int boundary_mode,
                                       int mem_kind, int device, void* stream) {
  FrameCall c;
  const int rc = make_frame_call(&c, kExecColourSpline, dcp::kPersp, src, dst, dtype, height, width, src_row_stride, src_pixel_stride, channels,
                                 0.0, 0.0, nullptr, 0, list_coef, Points{}, order, DCP_BLEND_SCIPY, boundary_mode, 1, mem_kind, device, stream);
  if (dtype == dcp::kF32) c.map.fast_div = 0;
  return rc != DCP_OK ? rc : run_frame(c);
}

int dcp_unwarp_fused_color_image_spline(const void* src, void* dst, int dtype, int64_t height, int64_t width, int channels,
                                        int64_t src_row_stride, int64_t src_pixel_stride, double xcenter, double ycenter,
                                        const double* list_fact, int nfact, const double* list_coef, int order, int boundary_mode, int mem_kind,
                                        int device, void* stream) {
  FrameCall c;
  const int rc = make_frame_call(&c, kExecColourSpline, dcp::kFused, src, dst, dtype, height, width, src_row_stride, src_pixel_stride, channels,
                                 xcenter, ycenter, list_fact, nfact, list_coef, Points{}, order, DCP_BLEND_SCIPY, boundary_mode, 1, mem_kind,
                                 device, stream);
  return rc != DCP_OK ? rc : run_frame(c);
}

// Frames of one calibration at spline orders 2..5.  Every frame's result is that of the single-frame call on it, down to the homography's
// division (see the colour entry points above: float32 divides plainly, the other element types as the typed entry point does).
int dcp_remap_frames_spline(const void* src, void* dst, int dtype, int map_kind, int64_t nframes, int64_t height, int64_t width,
                            int64_t frame_stride, int64_t row_stride, double xcenter, double ycenter, const double* list_fact,
                            int nfact, const double* list_coef, int order, int mode, int mem_kind, int device, void* stream) {
  if (map_kind != DCP_MAP_RADIAL && map_kind != DCP_MAP_PERSPECTIVE && map_kind != DCP_MAP_FUSED)
    return fail(DCP_ERR_INVALID_ARG, "unknown map_kind %d", map_kind);
  if (nframes < 0) return fail(DCP_ERR_INVALID_ARG, "nframes < 0");
  if (nframes > 2147483647LL) return fail(DCP_ERR_UNSUPPORTED, "too many frames");
  const dcp::MapKind kind = (dcp::MapKind)map_kind;
  // (an empty stack checks everything but its pointers)
  static const char nothing = 0;
  const void* s = nframes == 0 && !src ? (const void*)&nothing : src;
  void* d = nframes == 0 && !dst ? (void*)&nothing : dst;
  FrameCall c;
  const int rc = make_frame_call(&c, kExecFramesSpline, kind, s, d, dtype, height, width, row_stride, 1, 1, xcenter, ycenter, list_fact, nfact,
                                 list_coef, Points{}, order, DCP_BLEND_SCIPY, mode, 1, mem_kind, device, stream);
  if (rc != DCP_OK) return rc;
  if (nframes > 1 && frame_stride < (height - 1) * row_stride + width)
    return fail(DCP_ERR_INVALID_ARG, "frame stride %lld overlaps frames of %lld rows, %lld elements apart", (long long)frame_stride, (long long)height,
                (long long)row_stride);
  if (nframes == 0) return DCP_OK;
  if (kind == dcp::kPersp && dtype == dcp::kF32) c.map.fast_div = 0;
  c.nframes = nframes;
  c.fs = nframes > 1 ? frame_stride : 0;
  return run_frame(c);
}

int dcp_unwarp_image_forward(const void* src, void* dst, int dtype, int64_t height, int64_t width, int64_t src_row_stride,
                             int64_t src_col_stride, double xcenter, double ycenter, const double* list_fact, int nfact, int mem_kind,
                             int device, void* stream) {
  FrameCall c;
  const int rc = make_frame_call(&c, kExecForward, dcp::kRadial, src, dst, dtype, height, width, src_row_stride, src_col_stride, 1, xcenter,
                                 ycenter, list_fact, nfact, nullptr, Points{}, 0, DCP_BLEND_SCIPY, 0, 0, mem_kind, device, stream);
  return rc != DCP_OK ? rc : run_frame(c);
}

int dcp_unwarp_image_spline_f32(const float* src, float* dst, int64_t height, int64_t width, int64_t src_row_stride,
                                int64_t src_col_stride, double xcenter, double ycenter, const double* list_fact,
                                int nfact, int order, int boundary_mode, int mem_kind, int device, void* stream) {
  FrameCall c;
  const int rc = make_frame_call(&c, kExecSpline, dcp::kRadial, src, dst, dcp::kF32, height, width, src_row_stride, src_col_stride, 1,
                                 xcenter, ycenter, list_fact, nfact, nullptr, Points{}, order, DCP_BLEND_SCIPY, boundary_mode, 1, mem_kind,
                                 device, stream);
  return rc != DCP_OK ? rc : run_frame(c);
}

int dcp_perspective_image_spline_f32(const float* src, float* dst, int64_t height, int64_t width,
                                     int64_t src_row_stride, int64_t src_col_stride, const double* list_coef, int order,
                                     int boundary_mode, int mem_kind, int device, void* stream) {
  FrameCall c;
  const int rc = make_frame_call(&c, kExecSpline, dcp::kPersp, src, dst, dcp::kF32, height, width, src_row_stride, src_col_stride, 1, 0.0,
                                 0.0, nullptr, 0, list_coef, Points{}, order, DCP_BLEND_SCIPY, boundary_mode, 1, mem_kind, device, stream);
  c.map.fast_div = 0;        // (this entry point has always divided the homography plainly; the typed one, at orders 2..5 too, does not)
  return rc != DCP_OK ? rc : run_frame(c);
}

int dcp_unwarp_fused_spline_f32(const float* src, float* dst, int64_t height, int64_t width, int64_t src_row_stride,
                                int64_t src_col_stride, double xcenter, double ycenter, const double* list_fact,
                                int nfact, const double* list_coef, int order, int boundary_mode, int mem_kind, int device,
                                void* stream) {
  FrameCall c;
  const int rc = make_frame_call(&c, kExecSpline, dcp::kFused, src, dst, dcp::kF32, height, width, src_row_stride, src_col_stride, 1,
                                 xcenter, ycenter, list_fact, nfact, list_coef, Points{}, order, DCP_BLEND_SCIPY, boundary_mode, 1, mem_kind,
                                 device, stream);
  return rc != DCP_OK ? rc : run_frame(c);
}

int dcp_remap_coords_spline_f32(const float* src, float* dst, int64_t height, int64_t width, int64_t src_row_stride,
                                int64_t src_col_stride, const void* ycoord, const void* xcoord, int coord_dtype,
                                int64_t npts, int order, int boundary_mode, int mem_kind, int device, void* stream) {
  bool host = false;
  if (npts == 0 && order >= 2 && order <= 5) return mem_kind_of(mem_kind, &host);     // (an empty call checks nothing else)
  FrameCall c;
  const int rc = make_frame_call(&c, kExecSpline, dcp::kCoords, src, dst, dcp::kF32, height, width, src_row_stride, src_col_stride, 1, 0.0,
                                 0.0, nullptr, 0, nullptr, Points{ycoord, xcoord, coord_dtype, npts}, order, DCP_BLEND_SCIPY, boundary_mode,
                                 1, mem_kind, device, stream);
  return rc != DCP_OK ? rc : run_frame(c);
}

int dcp_map_points_f64(const double* yx_in, double* yx_out, int64_t npts, double xcenter, double ycenter,
                       const double* list_fact, int nfact, int mem_kind, int device, void* stream) {
  return map_points(dcp::kRadial, yx_in, yx_out, npts, xcenter, ycenter, list_fact, nfact, nullptr, mem_kind, device, stream);
}

int dcp_map_points_inverse_f64(const double* yx_in, double* yx_out, int64_t npts, double xcenter, double ycenter,
                               const double* list_fact, int nfact, int64_t* n_unsolved, int mem_kind, int device, void* stream) {
  return map_points_inverse(yx_in, yx_out, npts, xcenter, ycenter, list_fact, nfact, n_unsolved, mem_kind, device, stream);
}

int dcp_map_points_perspective_f64(const double* yx_in, double* yx_out, int64_t npts, const double* list_coef, int mem_kind, int device,
                                   void* stream) {
  return map_points(dcp::kPersp, yx_in, yx_out, npts, 0.0, 0.0, nullptr, 0, list_coef, mem_kind, device, stream);
}

int dcp_coordinate_map_f32(float* ymap, float* xmap, int64_t height, int64_t width, int map_kind, double xcenter,
                           double ycenter, const double* list_fact, int nfact, const double* list_coef, int mem_kind,
                           int device, void* stream) {
  int rc;
  bool host = false;
  if ((rc = mem_kind_of(mem_kind, &host)) != DCP_OK) return rc;
  if (!ymap || !xmap) return fail(DCP_ERR_INVALID_ARG, "null map pointer");
  if (height <= 0 || width <= 0 || height > 1073741823LL || width > 1073741823LL)
    return fail(DCP_ERR_INVALID_ARG, "map must be non-empty (got %lld x %lld)", (long long)height, (long long)width);
  if (map_kind < DCP_MAP_RADIAL || map_kind > DCP_MAP_FUSED) return fail(DCP_ERR_INVALID_ARG, "unknown map_kind %d", map_kind);
  const dcp::MapKind kind = (dcp::MapKind)map_kind;
  dcp::MapArgs map;
  if ((rc = frame_map(&map, kind, xcenter, ycenter, list_fact, nfact, list_coef, height, width)) != DCP_OK) return rc;
  DeviceScope scope(device);
  if (scope.status != hipSuccess) return fail(DCP_ERR_HIP, "cannot select device %d: %s", device, hipGetErrorString(scope.status));
  dcp::ImageArgs img;
  memset(&img, 0, sizeof(img));
  img.H = (int32_t)height;
  img.W = (int32_t)width;
  hipStream_t st = (hipStream_t)stream;
  if (!host) {
    DCP_HIP(dcp::launch_coord_map(kind, img, map, ymap, xmap, st));
    return DCP_OK;
  }
  HostTrip t;
  t.y_down = ymap;
  t.x_down = xmap;
  t.plane = (size_t)height * (size_t)width * 4;
  return host_round_trip(t, st, [&](const void*, void*, void* dy, void* dx) { return dcp::launch_coord_map(kind, img, map, (float*)dy, (float*)dx, st); });
}

}  // extern "C"
