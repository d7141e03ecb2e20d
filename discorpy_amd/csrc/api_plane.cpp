// api_plane.cpp -- the argument checks of the plane entry points (api_plane.h), every one of them before any device call.
#include "api_plane.h"

namespace dcpapi {

int check_plane_shape(int height, int width, int dtype, PlaneLimit limit) {
  if (dtype < 0 || dtype >= dcp::kNumElemTypes) return fail(DCP_ERR_INVALID_ARG, "unknown dtype %d", dtype);
  if (height < 1 || width < 1) return fail(DCP_ERR_INVALID_ARG, "height and width must be at least 1 (got %d x %d)", height, width);
  if (limit == kSideLimit && (height > 1073741823 || width > 1073741823))
    return fail(DCP_ERR_UNSUPPORTED, "height / width above 2^30 - 1 (got %d x %d)", height, width);
  if (limit == kPixelLimit && (int64_t)height * (int64_t)width > 2147483647LL)
    return fail(DCP_ERR_UNSUPPORTED, "height * width = %lld: labels and pixel indices are int32, at most 2^31 - 1 pixels", (long long)height * width);
  return DCP_OK;
}

int check_row_stride(const char* name, long row_stride, int width) {
  if (row_stride < width) return fail(DCP_ERR_INVALID_ARG, "%s %ld is below the width %d", name, row_stride, width);
  return DCP_OK;
}

int make_plane_call(PlaneCall* c, const void* src, void* dst, int height, int width, long src_row_stride, int dtype, size_t dst_elem, PlaneLimit limit,
                    const char* overlap_clause, int mem_kind, int device, void* stream) {
  int rc;
  if ((rc = mem_kind_of(mem_kind, &c->host)) != DCP_OK) return rc;
  if ((rc = check_plane_shape(height, width, dtype, limit)) != DCP_OK) return rc;
  if (dst_elem == kSameElem) dst_elem = (size_t)dcp::elem_size(dtype);
  if (!src || (dst_elem && !dst)) return fail(DCP_ERR_INVALID_ARG, "null src / dst pointer");
  if ((rc = check_row_stride("src_row_stride", src_row_stride, width)) != DCP_OK) return rc;
  c->src = src;
  c->dst = dst_elem ? dst : nullptr;
  c->H = height;
  c->W = width;
  c->rs = (int64_t)src_row_stride;
  c->dtype = dtype;
  c->esz = (size_t)dcp::elem_size(dtype);
  c->dst_elem = dst_elem;
  c->dst_n = (int64_t)height * (int64_t)width;
  c->device = device;
  c->stream = (hipStream_t)stream;
  if (!dst_elem) return DCP_OK;
  const char *s0 = (const char*)src, *s1 = s0 + ((size_t)(height - 1) * (size_t)src_row_stride + (size_t)width) * c->esz;
  const char *d0 = (const char*)dst, *d1 = d0 + (size_t)height * (size_t)width * dst_elem;
  if (s0 < d1 && d0 < s1) return fail(DCP_ERR_INVALID_ARG, "src and dst overlap: %s", overlap_clause);
  return DCP_OK;
}

HostTrip packed_rows(const PlaneCall& c) {
  HostTrip t;
  t.src = c.src;
  t.row_bytes = (size_t)c.W * c.esz;
  t.rows = (size_t)c.H;
  t.pitch = (size_t)c.rs * c.esz;
  t.dst = c.dst;
  t.out_bytes = (size_t)c.dst_n * c.dst_elem;
  return t;
}

}  // namespace dcpapi
