// api_plane.h -- the plane entry points of the C ABI (dcp_*_2d of api_median.cpp, api_gauss.cpp, api_label.cpp, api_binarize.cpp): one
// description of such a call (PlaneCall), the only reading of its arguments (make_plane_call, api_plane.cpp) and the only place that
// forks on the memory kind (run_plane) -- what FrameCall / make_frame_call / run_frame are to the frame entry points.  Not installed.
#pragma once
#include "api_common.h"

namespace dcpapi {

// One source plane of H x W elements of `dtype`, its rows `rs` elements apart, and (dst_elem != 0) one packed destination plane of
// H x W elements of dst_elem bytes.
struct PlaneCall {
  const void* src;
  void* dst;                 // null where the call has no destination plane
  int H, W;
  int64_t rs;                // the source's row stride in elements
  int dtype;
  size_t esz, dst_elem;      // element sizes in bytes; dst_elem = 0: no destination
  int64_t dst_n;             // elements of the destination: H * W unless the entry point says otherwise (dcp_zoom_cubic_nearest_1d)
  bool host;                 // DCP_MEM_HOST
  int device;
  hipStream_t stream;
};

// What a plane may measure: each side at most 2^30 - 1 (the filters), or at most 2^31 - 1 pixels (whatever labels or indexes pixels in int32).
enum PlaneLimit : int { kSideLimit, kPixelLimit };
// The clause of the message behind "src and dst overlap: ".
constexpr const char* kReadsWindow = "every output pixel reads a window of the source";
constexpr const char* kReadsNeighbourhood = "every output pixel reads a neighbourhood of the source";
constexpr const char* kComponentReach = "a pixel's component reaches across the whole image";

constexpr size_t kSameElem = ~(size_t)0;   // dst_elem of make_plane_call: the destination's elements are the source's
// The checks every plane call shares, before any device call, and the call they describe: mem_kind, dtype, null pointers, height and
// width, the row stride, `limit`, and that src and dst do not overlap.
int make_plane_call(PlaneCall* c, const void* src, void* dst, int height, int width, long src_row_stride, int dtype, size_t dst_elem, PlaneLimit limit,
                    const char* overlap_clause, int mem_kind, int device, void* stream);
// The pieces of it that dcp_label_measures_2d applies to its two source planes: `name` is the stride argument's.
int check_plane_shape(int height, int width, int dtype, PlaneLimit limit);
int check_row_stride(const char* name, long row_stride, int width);
// The round trip of a DCP_MEM_HOST call: the rows packed on the way up, H * W * dst_elem bytes back (none without dst).
HostTrip packed_rows(const PlaneCall& c);

// The call's device selected for the calling thread while the object lives; rc carries the failure.
struct PlaneDevice {
  DeviceScope scope;
  int rc;
  explicit PlaneDevice(int device)
      : scope(device), rc(scope.status == hipSuccess ? DCP_OK : fail(DCP_ERR_HIP, "cannot select device %d: %s", device, hipGetErrorString(scope.status))) {}
};

// Executes a plane call: selects the device, leases `work_bytes` of the spline workspace (none for 0: work = null) and enqueues
// launch(src, dst, row_stride, work) -- on the caller's planes for device memory, after which the stream is synchronised iff the entry
// point returns host scalars (launch enqueues their read-back); on the packed staging planes (row_stride = W) inside the round trip of
// host memory (c.dst_n elements come back), which always ends synchronised.  The lease ends before the previous device is selected again.
template <typename Launch>
int run_plane(const PlaneCall& c, bool returns_host_scalars, size_t work_bytes, Launch&& launch) {
  PlaneDevice on(c.device);
  if (on.rc != DCP_OK) return on.rc;
  WorkspaceLease lease;
  int rc;
  if (work_bytes && (rc = lease.acquire(work_bytes, c.stream)) != DCP_OK) return rc;
  if (c.host)
    return host_round_trip(packed_rows(c), c.stream,
                           [&](const void* dsrc, void* ddst, void*, void*) { return launch(dsrc, ddst, (int64_t)c.W, lease.buf); });
  DCP_HIP(launch(c.src, c.dst, c.rs, lease.buf));
  if (returns_host_scalars) DCP_HIP(hipStreamSynchronize(c.stream));
  return DCP_OK;
}

}  // namespace dcpapi
