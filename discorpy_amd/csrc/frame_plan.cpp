// frame_plan.cpp -- the per-calibration tile plans of remap_wg_kernel (dcp_internal.h, "Frame plans").
//
// The coordinate map of a frame depends on the calibration and the frame shape only, and a caller applies one calibration to
// thousands of frames (the projections of a scan).  Two things every wave of remap_wg_kernel works out per frame are therefore
// worked out once and kept: the hull of its workgroup tile's corner taps, and whether the cubic of radial_rows_interp reproduces
// the exact float32 coordinates of its wave tile (plan_table_kernel decides that by evaluating both).  20 bytes per 128 x 32
// tile, read by scalar loads: no plane per pixel, no extra pass over memory.
//
// Rules of the cache:
//  * one cache per device, shared by the host threads, behind one mutex; kPlans plans, least recently used replaced;
//  * a calibration seen for the first time only leaves its key behind (a centre search, or a batch of distinct calibrations dealt
//    frame by frame, never pays for plans it does not reuse); the second sighting builds (option frame_plan = 2: the first);
//  * the build is one small launch on the calling stream followed by an event.  Until the host has seen that event complete, a
//    call on another stream waits for it on the device, and every launch that reads the plan keeps its barrier bit (an any-order
//    packet may start while earlier packets of its own stream still run).  Afterwards no call touches the event;
//  * nothing is built, queried or waited for while the calling stream is being captured: such a call uses a plan the host already
//    knows to be complete, or none;
//  * the memory of a replaced plan is never handed out again and is freed only by frame_plan_release (dcp_release_scratch, after the
//    devices have been synchronised): a launch still in flight -- or a captured graph -- may read it.  At most kRetired replaced
//    plans are kept per device; past that no further plan is built on that device until the release;
//  * any HIP error on the way means "no plan": the error is cleared and the call takes the path without one.
#include "dcp_internal.h"

#include <string.h>

#include <mutex>
#include <vector>

namespace dcp {
namespace {

constexpr int kPlans = 16;       // plans per device
constexpr int kSeen = 16;        // keys seen once per device (round-robin)
constexpr int kRetired = 64;     // replaced plans kept until the release, per device
constexpr int kDevices = 64;

struct PlanKey {
  int32_t nfact = -1, H = 0, W = 0, y_origin = 0, rows_out = 0;
  double xc = 0, yc = 0, fact[kInlineFact];
};
// (bit for bit: -0.0 and 0.0, or two NaN payloads, are different calibrations here -- never the other way round)
bool same(const PlanKey& a, const PlanKey& b) {
  return a.nfact == b.nfact && a.H == b.H && a.W == b.W && a.y_origin == b.y_origin && a.rows_out == b.rows_out &&
         memcmp(&a.xc, &b.xc, sizeof(double)) == 0 && memcmp(&a.yc, &b.yc, sizeof(double)) == 0 &&
         memcmp(a.fact, b.fact, sizeof(double) * (size_t)a.nfact) == 0;
}

struct Plan {
  PlanKey key;
  int32_t* dev = nullptr;          // 5 * ntiles words
  int ntiles = 0;
  hipEvent_t built = nullptr;      // recorded behind the build
  hipStream_t build_stream = nullptr;
  bool ready = false;              // the host has seen `built` complete
  unsigned long long tick = 0;
};

struct DeviceCache {
  Plan plan[kPlans];
  PlanKey seen[kSeen];
  int seen_next = 0;
  std::vector<int32_t*> retired;
  std::vector<hipEvent_t> retired_events;
  unsigned long long clock = 0;
  int last = -1;                   // the plan built last (lab keys frame_plan_tiles / frame_plan_exact_tiles)
};

std::mutex g_mu;
DeviceCache* g_cache[kDevices];    // allocated on first use, never moved
int g_mode = 1;

}  // namespace

void set_frame_plan(int v) {
  std::lock_guard<std::mutex> lock(g_mu);
  g_mode = v;
}
int get_frame_plan() {
  std::lock_guard<std::mutex> lock(g_mu);
  return g_mode;
}

const int32_t* frame_plan_lookup(const ImageArgs& img, const MapArgs& map, hipStream_t stream, PlanBuildFn build, bool* ordered) {
  *ordered = false;
  if (map.nfact < 0 || map.nfact > kInlineFact) return nullptr;
  std::lock_guard<std::mutex> lock(g_mu);
  if (g_mode <= 0) return nullptr;
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kDevices) {
    (void)hipGetLastError();
    return nullptr;
  }
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(stream, &cap) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  const bool capturing = cap != hipStreamCaptureStatusNone;
  if (!g_cache[dev]) {
    if (capturing) return nullptr;
    g_cache[dev] = new DeviceCache();
  }
  DeviceCache& c = *g_cache[dev];

  PlanKey key;
  memset(&key, 0, sizeof(key));
  key.nfact = map.nfact;
  key.H = img.H;
  key.W = img.W;
  key.y_origin = img.y_origin;
  key.rows_out = img.rows_out;
  key.xc = map.xc;
  key.yc = map.yc;
  memcpy(key.fact, map.fact, sizeof(double) * (size_t)map.nfact);

  for (int i = 0; i < kPlans; ++i) {
    Plan& p = c.plan[i];
    if (!p.dev || !same(p.key, key)) continue;
    if (!p.ready) {
      if (capturing) return nullptr;
      const hipError_t q = hipEventQuery(p.built);
      if (q == hipSuccess) {
        p.ready = true;
      } else if (q == hipErrorNotReady) {
        (void)hipGetLastError();     // (not an error: must not resurface as the launch's hipGetLastError)
        if (stream != p.build_stream && hipStreamWaitEvent(stream, p.built, 0) != hipSuccess) {
          (void)hipGetLastError();
          return nullptr;
        }
        *ordered = true;
      } else {
        (void)hipGetLastError();
        return nullptr;
      }
    }
    p.tick = ++c.clock;
    return p.dev;
  }
  if (capturing) return nullptr;

  if (g_mode < 2) {                // build on the second sighting
    bool was_seen = false;
    for (int i = 0; i < kSeen; ++i) was_seen = was_seen || same(c.seen[i], key);
    if (!was_seen) {
      c.seen[c.seen_next] = key;
      c.seen_next = (c.seen_next + 1) % kSeen;
      return nullptr;
    }
  }

  // a free slot, else the least recently used plan, whose memory retires
  int slot = -1;
  for (int i = 0; i < kPlans && slot < 0; ++i)
    if (!c.plan[i].dev) slot = i;
  if (slot < 0) {
    if ((int)c.retired.size() >= kRetired) return nullptr;
    slot = 0;
    for (int i = 1; i < kPlans; ++i)
      if (c.plan[i].tick < c.plan[slot].tick) slot = i;
  }
  const int ntiles = img.tiles_x * img.tiles_y;
  int32_t* mem = nullptr;
  hipEvent_t ev = nullptr;
  if (ntiles <= 0 || hipMalloc((void**)&mem, (size_t)ntiles * 20) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess || build(img, map, mem, stream) != hipSuccess ||
      hipEventRecord(ev, stream) != hipSuccess) {
    (void)hipGetLastError();
    // (a build that was launched may still write `mem`: it retires with the rest)
    c.retired.push_back(mem);
    if (ev) c.retired_events.push_back(ev);
    return nullptr;
  }
  Plan& p = c.plan[slot];
  if (p.dev) {
    c.retired.push_back(p.dev);
    c.retired_events.push_back(p.built);
  }
  p.key = key;
  p.dev = mem;
  p.ntiles = ntiles;
  p.built = ev;
  p.build_stream = stream;
  p.ready = false;
  p.tick = ++c.clock;
  c.last = slot;
  for (int i = 0; i < kSeen; ++i)
    if (same(c.seen[i], key)) c.seen[i].nfact = -1;
  *ordered = true;
  return mem;
}

hipError_t frame_plan_last_counts(int* wave_tiles, int* exact_tiles) {
  *wave_tiles = 0;
  *exact_tiles = 0;
  int dev = -1;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  const int32_t* mem = nullptr;
  hipEvent_t ev = nullptr;
  int ntiles = 0;
  {
    std::lock_guard<std::mutex> lock(g_mu);
    if (dev < 0 || dev >= kDevices || !g_cache[dev] || g_cache[dev]->last < 0) return hipSuccess;
    const Plan& p = g_cache[dev]->plan[g_cache[dev]->last];
    mem = p.dev;
    ev = p.built;
    ntiles = p.ntiles;
  }
  if (!mem) return hipSuccess;
  if ((e = hipEventSynchronize(ev)) != hipSuccess) return e;
  std::vector<int32_t> bits((size_t)ntiles);
  if ((e = hipMemcpy(bits.data(), mem + 4 * (size_t)ntiles, (size_t)ntiles * 4, hipMemcpyDeviceToHost)) != hipSuccess) return e;
  int certified = 0;
  for (int32_t b : bits) certified += __builtin_popcount((unsigned)b & 15u);
  *wave_tiles = 4 * ntiles;
  *exact_tiles = 4 * ntiles - certified;
  return hipSuccess;
}

void frame_plan_release() {
  std::lock_guard<std::mutex> lock(g_mu);
  int prev = 0;
  if (hipGetDevice(&prev) != hipSuccess) {
    (void)hipGetLastError();
    return;
  }
  for (int dev = 0; dev < kDevices; ++dev) {
    DeviceCache* c = g_cache[dev];
    if (!c) continue;
    if (hipSetDevice(dev) == hipSuccess && hipDeviceSynchronize() == hipSuccess) {
      for (Plan& p : c->plan) {
        if (p.dev) (void)hipFree(p.dev);
        if (p.built) (void)hipEventDestroy(p.built);
      }
      for (int32_t* m : c->retired) (void)hipFree(m);
      for (hipEvent_t ev : c->retired_events) (void)hipEventDestroy(ev);
    }
    (void)hipGetLastError();
    delete c;
    g_cache[dev] = nullptr;
  }
  (void)hipSetDevice(prev);
}

}  // namespace dcp
