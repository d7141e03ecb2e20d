// api_spline.cpp -- spline orders 2..5 (scipy's prefiltered B-spline interpolation, spline_kernels.hip): the
// per-device coefficient workspace and the spline executors of FrameCall -- one plane (run_spline), interleaved channels
// (run_spline_color), frames of one calibration in groups (run_spline_frames); api_image.cpp holds the entry points.  The forward
// scatter (forward_kernels.hip) leases its winner plane from the same workspace: run_forward.
#include "api_common.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include <mutex>

using namespace dcpapi;

namespace {

// Per-device float64 coefficient workspaces (grow-only): kSlots of them, so that spline calls on TWO streams -- independent frames
// handed over alternately, INTEGRATION.md section 7 -- each keep their planes and the prefilter of one frame (memory-bound) runs
// under the gather of the other (LDS- and VALU-bound) instead of waiting for the device (rounds 2-5: one workspace, and a call on
// another stream than the last one synchronised the device first).  A slot remembers the stream that used it last and an event
// recorded behind that use; a call on another stream waits for the event ON THE DEVICE (hipStreamWaitEvent), never on the host.
// A slot's mutex is held by run_spline from acquire() until its last kernel is enqueued (host callers: until the result is back),
// so two host threads never interleave their passes over one slot's planes; calls on different GPUs run side by side.
struct SplineWorkspace {
  static constexpr int kSlots = 2;
  struct Slot {
    std::mutex use;
    void* buf = nullptr;
    size_t cap = 0;
    hipStream_t last = nullptr;
    bool used = false;
    hipEvent_t done = nullptr;
    unsigned long long tick = 0;
  };
  std::mutex mu;                     // the tables below (never held while waiting for a slot)
  Slot slot[64][kSlots];
  unsigned long long clock = 0;

  // The slot for a call on `stream` of the current device, LOCKED (release() unlocks), its planes grown to `bytes` and ordered behind
  // the slot's previous use.  Preference: the slot this stream used last; a slot never used; the least recently used one.
  hipError_t acquire(size_t bytes, hipStream_t stream, int dev, Slot** out) {
    int order[kSlots];
    bool own = false;                  // the preferred slot was last used by this very stream (read under `mu`, like every table entry)
    {
      std::lock_guard<std::mutex> lock(mu);
      int n = 0;
      for (int k = 0; k < kSlots; ++k)
        if (slot[dev][k].used && slot[dev][k].last == stream) order[n++] = k;
      for (int k = 0; k < kSlots; ++k)
        if (!slot[dev][k].used) order[n++] = k;
      for (int pass = 0; pass < kSlots; ++pass) {          // the rest, least recently used first
        int best = -1;
        for (int k = 0; k < kSlots; ++k) {
          bool taken = false;
          for (int i = 0; i < n; ++i) taken = taken || order[i] == k;
          if (!taken && (best < 0 || slot[dev][k].tick < slot[dev][best].tick)) best = k;
        }
        if (best >= 0) order[n++] = best;
      }
      own = slot[dev][order[0]].used && slot[dev][order[0]].last == stream;
    }
    Slot* s = nullptr;
    // a slot of this stream is taken even if another thread holds it right now (calls on one stream are ordered anyway); otherwise
    // the first free one in preference order, and if every slot is busy, wait for the preferred one
    if (own) {
      s = &slot[dev][order[0]];
      s->use.lock();
    } else {
      for (int i = 0; i < kSlots && !s; ++i)
        if (slot[dev][order[i]].use.try_lock()) s = &slot[dev][order[i]];
      if (!s) {
        s = &slot[dev][order[0]];
        s->use.lock();
      }
    }
    hipError_t e = hipSuccess;
    if (!s->done) e = hipEventCreateWithFlags(&s->done, hipEventDisableTiming);
    if (e == hipSuccess && s->cap < bytes) {
      if (s->buf) {                                          // the previous user must be done before its planes go away
        e = hipEventSynchronize(s->done);
        if (e == hipSuccess) e = hipFree(s->buf);
        s->buf = nullptr;
        s->cap = 0;
      }
      if (e == hipSuccess) e = hipMalloc(&s->buf, bytes);
      if (e == hipSuccess) s->cap = bytes;
    }
    // another stream used these planes last: this call's kernels start behind that use (nothing to wait for on the same stream).
    // (`used` / `last` of a slot whose `use` mutex this thread holds change only under that mutex)
    if (e == hipSuccess && s->used && s->last != stream) e = hipStreamWaitEvent(stream, s->done, 0);
    if (e != hipSuccess) {
      s->use.unlock();
      return e;
    }
    {
      std::lock_guard<std::mutex> lock(mu);
      s->used = true;
      s->last = stream;
      s->tick = ++clock;
    }
    *out = s;
    return hipSuccess;
  }
  // every kernel of the call has been enqueued on `stream`: mark the end of the use and let the next caller in
  void release(Slot* s, hipStream_t stream) {
    (void)hipEventRecord(s->done, stream);
    s->use.unlock();
  }
};
SplineWorkspace g_spline_ws;
struct SlotGuard {           // releases the slot on every return path of run_spline
  SplineWorkspace::Slot* s;
  hipStream_t st;
  ~SlotGuard() { g_spline_ws.release(s, st); }
};

int spline_poles(int order, double* z) {
  switch (order) {
    case 2: z[0] = std::sqrt(8.0) - 3.0; return 1;
    case 3: z[0] = std::sqrt(3.0) - 2.0; return 1;
    case 4:
      z[0] = std::sqrt(664.0 - std::sqrt(438976.0)) + std::sqrt(304.0) - 19.0;
      z[1] = std::sqrt(664.0 + std::sqrt(438976.0)) - std::sqrt(304.0) - 19.0;
      return 2;
    case 5:
      z[0] = std::sqrt(67.5 - std::sqrt(4436.25)) + std::sqrt(26.25) - 6.5;
      z[1] = std::sqrt(67.5 + std::sqrt(4436.25)) - std::sqrt(26.25) - 6.5;
      return 2;
    default: return 0;
  }
}

}  // namespace

namespace dcpapi {

int release_spline_workspace() {
  int prev = 0;
  if (hipGetDevice(&prev) != hipSuccess) return DCP_OK;      // no runtime / no device: nothing was ever allocated
  for (int dev = 0; dev < 64; ++dev)
    for (int k = 0; k < SplineWorkspace::kSlots; ++k) {
      SplineWorkspace::Slot& sl = g_spline_ws.slot[dev][k];
      std::lock_guard<std::mutex> exclusive(sl.use);
      if (!sl.buf) continue;
      DCP_HIP(hipSetDevice(dev));
      DCP_HIP(hipDeviceSynchronize());
      (void)hipFree(sl.buf);
      std::lock_guard<std::mutex> lock(g_spline_ws.mu);
      sl.buf = nullptr;
      sl.cap = 0;
      sl.used = false;
      sl.last = nullptr;
    }
  (void)hipSetDevice(prev);
  return DCP_OK;
}

int WorkspaceLease::acquire(size_t bytes, hipStream_t stream) {
  int cur_dev = 0;
  DCP_HIP(hipGetDevice(&cur_dev));
  if (cur_dev < 0 || cur_dev >= 64) return fail(DCP_ERR_UNSUPPORTED, "device index %d", cur_dev);
  SplineWorkspace::Slot* s = nullptr;
  DCP_HIP(g_spline_ws.acquire(bytes, stream, cur_dev, &s));
  slot = s;
  buf = s->buf;
  st = stream;
  return DCP_OK;
}

WorkspaceLease::~WorkspaceLease() {
  if (slot) g_spline_ws.release(static_cast<SplineWorkspace::Slot*>(slot), st);
}

// The SplineArgs of a validated spline call, all but the workspace planes and the source pointer.
static dcp::SplineArgs spline_args_of(const FrameCall& c) {
  dcp::SplineArgs a;
  memset(&a, 0, sizeof(a));
  a.H = (int32_t)c.H;
  a.W = (int32_t)c.W;
  a.src_dtype = a.dst_dtype = c.dtype;
  a.order = c.order;
  a.mode = c.mode;
  a.exact_sum = c.exact_sum;
  a.pad = (c.mode == dcp::kModeNearest || c.mode == dcp::kModeGridConstant) ? 12 : 0;
  a.Hp = a.H + 2 * a.pad;
  a.Wp = a.W + 2 * a.pad;
  // ('nearest': scipy prefilters the edge-padded array with the reflect boundary -- see spline_filter_kind() in the oracle)
  a.filter_kind = (c.mode == dcp::kModeReflect || c.mode == dcp::kModeGridMirror || c.mode == dcp::kModeNearest) ? dcp::kSplReflect
                  : c.mode == dcp::kModeGridWrap                                       ? dcp::kSplWrap
                                                                                       : dcp::kSplMirror;
  a.npoles = spline_poles(c.order, a.poles);
  for (int axis = 0; axis < 2; ++axis) {
    const double n = axis == 0 ? (double)a.Hp : (double)a.Wp;
    for (int p = 0; p < a.npoles; ++p)
      a.zpow[axis][p] = std::pow(a.poles[p], a.filter_kind == dcp::kSplMirror ? n - 1.0 : n);
  }
  a.src_stride = (int32_t)c.rs;
  a.src_cstride = (int32_t)c.cs;
  return a;
}

int run_spline(const FrameCall& c) {
  hipStream_t st = c.stream;
  dcp::SplineArgs a = spline_args_of(c);
  const size_t plane = (size_t)a.Hp * (size_t)a.Wp * sizeof(double);
  int cur_dev = 0;
  DCP_HIP(hipGetDevice(&cur_dev));                           // (run_frame has selected it)
  if (cur_dev < 0 || cur_dev >= 64) return fail(DCP_ERR_UNSUPPORTED, "device index %d", cur_dev);
  SplineWorkspace::Slot* slot = nullptr;
  DCP_HIP(g_spline_ws.acquire(2 * plane, st, cur_dev, &slot));
  SlotGuard guard{slot, st};
  a.coef = (double*)slot->buf;
  a.scratch = a.coef + (size_t)a.Hp * (size_t)a.Wp;
  dcp::CoordArgs ca;
  memset(&ca, 0, sizeof(ca));
  ca.npts = c.npts;
  ca.is_f64 = c.coord_dtype == DCP_COORD_F64;
  if (!c.host) {
    a.src = c.src;
    ca.ycoord = c.ycoord;
    ca.xcoord = c.xcoord;
    DCP_HIP(dcp::launch_spline(a, c.kind, c.map, ca, c.dst, st));
    return DCP_OK;
  }
  HostTrip t;
  t.src = c.src;
  t.row_bytes = t.pitch = extent_bytes_typed(c.H, c.W, c.rs, c.cs, c.dtype);
  if (c.kind == dcp::kCoords) {
    t.y_up = c.ycoord;
    t.x_up = c.xcoord;
    t.plane = (size_t)c.npts * (ca.is_f64 ? 8 : 4);
  }
  t.dst = c.dst;
  t.out_bytes = (size_t)(c.kind == dcp::kCoords ? c.npts : c.H * c.W) * (size_t)dcp::elem_size(c.dtype);
  return host_round_trip(t, st, [&](const void* dsrc, void* ddst, void* dy, void* dx) {
    a.src = dsrc;
    ca.ycoord = dy;
    ca.xcoord = dx;
    return dcp::launch_spline(a, c.kind, c.map, ca, ddst, st);
  });
}

// Interleaved (H, W, channels) image at orders 2..5: the workspace slot holds channels + 1 planes -- the coefficients of every channel
// and the prefilter's second plane --, the single-plane prefilter runs once per channel on that channel's column-strided view, one
// gather launch follows.  Host memory: the interleaved extent goes up once, the dense result comes back once.
int run_spline_color(const FrameCall& c) {
  hipStream_t st = c.stream;
  dcp::SplineArgs a = spline_args_of(c);
  const size_t plane = (size_t)a.Hp * (size_t)a.Wp * sizeof(double);
  int cur_dev = 0;
  DCP_HIP(hipGetDevice(&cur_dev));                           // (run_frame has selected it)
  if (cur_dev < 0 || cur_dev >= 64) return fail(DCP_ERR_UNSUPPORTED, "device index %d", cur_dev);
  SplineWorkspace::Slot* slot = nullptr;
  DCP_HIP(g_spline_ws.acquire((size_t)(c.channels + 1) * plane, st, cur_dev, &slot));
  SlotGuard guard{slot, st};
  a.coef = (double*)slot->buf;
  a.scratch = a.coef + (size_t)c.channels * (size_t)a.Hp * (size_t)a.Wp;
  if (!c.host) {
    a.src = c.src;
    DCP_HIP(dcp::launch_spline_color(a, c.kind, c.map, c.channels, c.dst, st));
    return DCP_OK;
  }
  const size_t esz = (size_t)dcp::elem_size(c.dtype);
  HostTrip t;
  t.src = c.src;
  t.row_bytes = t.pitch = (size_t)((c.H - 1) * c.rs + (c.W - 1) * c.cs + c.channels) * esz;
  t.dst = c.dst;
  t.out_bytes = (size_t)c.H * (size_t)c.W * (size_t)c.channels * esz;
  return host_round_trip(t, st, [&](const void* dsrc, void* ddst, void*, void*) {
    a.src = dsrc;
    return dcp::launch_spline_color(a, c.kind, c.map, c.channels, ddst, st);
  });
}

// c.nframes frames of one calibration (c.fs elements apart, unit column stride) at orders 2..5, in groups of G frames: the workspace slot
// holds G + 1 planes -- the coefficients of every frame of a group and the prefilter's second plane --, per group the single-plane
// prefilter runs once per frame and ONE gather launch follows, all on the call's stream.  G = min(frames left, option "x_spline_frames",
// the largest G with (G + 1) planes <= 2 GiB), at least 1: the 2 GiB keep the two slots of a device at 4 GiB at most.  The slot is held
// from the first group to the last.  Host memory: per group the source extent goes up once and the dense result comes back once.
// "x_spline_frames" = 0: every frame through the single-frame executor (run_spline).
int run_spline_frames(const FrameCall& c) {
  hipStream_t st = c.stream;
  const size_t esz = (size_t)dcp::elem_size(c.dtype);
  const size_t frame_out = (size_t)c.H * (size_t)c.W * esz;
  const int cap = g_spline_frames.load();
  if (cap <= 0) {
    FrameCall one = c;
    one.exec = kExecSpline;
    one.nframes = 1;
    for (int64_t f = 0; f < c.nframes; ++f) {
      one.src = (const char*)c.src + (size_t)f * (size_t)c.fs * esz;
      one.dst = (char*)c.dst + (size_t)f * frame_out;
      if (const int rc = run_spline(one)) return rc;
    }
    return DCP_OK;
  }
  dcp::SplineArgs a = spline_args_of(c);
  const size_t plane_elems = (size_t)a.Hp * (size_t)a.Wp, plane = plane_elems * sizeof(double);
  int64_t group = (int64_t)(((size_t)2 << 30) / plane) - 1;
  if (group > cap) group = cap;
  if (group > c.nframes) group = c.nframes;
  if (group < 1) group = 1;
  int cur_dev = 0;
  DCP_HIP(hipGetDevice(&cur_dev));                           // (run_frame has selected it)
  if (cur_dev < 0 || cur_dev >= 64) return fail(DCP_ERR_UNSUPPORTED, "device index %d", cur_dev);
  SplineWorkspace::Slot* slot = nullptr;
  DCP_HIP(g_spline_ws.acquire((size_t)(group + 1) * plane, st, cur_dev, &slot));
  SlotGuard guard{slot, st};
  a.coef = (double*)slot->buf;
  for (int64_t f0 = 0; f0 < c.nframes; f0 += group) {
    const int g = (int)(c.nframes - f0 < group ? c.nframes - f0 : group);
    const char* gsrc = (const char*)c.src + (size_t)f0 * (size_t)c.fs * esz;
    char* gdst = (char*)c.dst + (size_t)f0 * frame_out;
    a.scratch = a.coef + (size_t)g * plane_elems;
    if (!c.host) {
      a.src = gsrc;
      DCP_HIP(dcp::launch_spline_frames(a, c.kind, c.map, g, c.fs, gdst, st));
      continue;
    }
    HostTrip t;
    t.src = gsrc;
    t.row_bytes = t.pitch = (size_t)((g - 1) * c.fs + (c.H - 1) * c.rs + c.W) * esz;
    t.dst = gdst;
    t.out_bytes = (size_t)g * frame_out;
    const int rc = host_round_trip(t, st, [&](const void* dsrc, void* ddst, void*, void*) {
      a.src = dsrc;
      return dcp::launch_spline_frames(a, c.kind, c.map, g, c.fs, ddst, st);
    });
    if (rc != DCP_OK) return rc;
  }
  return DCP_OK;
}

// unwarp_image_forward: the winner plane (H W words) comes from the spline workspace -- a slot per stream, so calls on different streams
// scatter into different planes --, then the two launches on the call's stream.  Host memory: the source goes up whole (a scatter
// reaches any row: no bands), the dense result comes back.
int run_forward(const FrameCall& c) {
  hipStream_t st = c.stream;
  int cur_dev = 0;
  DCP_HIP(hipGetDevice(&cur_dev));                           // (run_frame has selected it)
  if (cur_dev < 0 || cur_dev >= 64) return fail(DCP_ERR_UNSUPPORTED, "device index %d", cur_dev);
  SplineWorkspace::Slot* slot = nullptr;
  DCP_HIP(g_spline_ws.acquire((size_t)c.H * (size_t)c.W * sizeof(uint32_t), st, cur_dev, &slot));
  SlotGuard guard{slot, st};
  dcp::ForwardArgs a;
  memset(&a, 0, sizeof(a));
  a.winner = (uint32_t*)slot->buf;
  a.H = (int32_t)c.H;
  a.W = (int32_t)c.W;
  a.esize = dcp::elem_size(c.dtype);
  a.src_stride = c.rs;
  a.src_cstride = c.cs;
  if (!c.host) {
    a.src = c.src;
    a.dst = c.dst;
    DCP_HIP(dcp::launch_forward(a, c.map, st));
    return DCP_OK;
  }
  const size_t esz = (size_t)a.esize;
  const bool pack = c.cs == 1;                                // unit column stride: the rows are packed on the way up
  HostTrip t;
  t.src = c.src;
  t.row_bytes = pack ? (size_t)c.W * esz : extent_bytes_typed(c.H, c.W, c.rs, c.cs, c.dtype);
  t.rows = pack ? (size_t)c.H : 1;
  t.pitch = pack ? (size_t)c.rs * esz : t.row_bytes;
  t.dst = c.dst;
  t.out_bytes = (size_t)c.H * (size_t)c.W * esz;
  return host_round_trip(t, st, [&](const void* dsrc, void* ddst, void*, void*) {
    a.src = dsrc;
    a.dst = ddst;
    if (pack) a.src_stride = c.W;
    return dcp::launch_forward(a, c.map, st);
  });
}

}  // namespace dcpapi
