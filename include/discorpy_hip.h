/*
 * discorpy_hip.h -- C ABI of libdiscorpy_hip.so: the MI355X (gfx950) implementation of the
 * backward-unwarp path of discorpy.post.postprocessing.
 *
 * The reference is pure Python (no FFI of its own); each entry point below replaces the body of
 * one reference function, cited as file:line under /root/reference.  INTEGRATION.md shows the
 * ctypes stub a discorpy maintainer would add to call them.
 *
 * Conventions
 *   - every function returns DCP_OK (0) or a negative DCP_ERR_* code; dcp_last_error() returns a
 *     thread-local, human-readable message for the last failure on the calling thread.
 *   - images are float32, row-major; `src_row_stride` / `src_col_stride` are in ELEMENTS, the
 *     output is always dense (height x width).  x = column index, y = row index.
 *   - mem_kind DCP_MEM_HOST: pointers are host memory, the library stages H2D/D2H itself and
 *     returns after the result is in `dst`.  DCP_MEM_DEVICE: pointers are device memory on
 *     `device`, the kernel is enqueued on `stream` (a hipStream_t, NULL = default stream) and the
 *     call returns without synchronising; the caller owns the memory and its lifetime.
 *   - device < 0 means "the calling thread's current HIP device".
 *   - order: 0 nearest (floor(c + 0.5)), 1 bilinear; orders 2..5 go through the *_spline_* entry points.
 *   - blend_mode (order 1 only): DCP_BLEND_SCIPY reproduces scipy.ndimage.map_coordinates'
 *     float64 arithmetic bit for bit; DCP_BLEND_F64LERP is the factorised float64 form (equal to
 *     it to <= 1 float32 ulp, in practice bit-equal); DCP_BLEND_F32LERP is float32 arithmetic
 *     (<= 2 float32 ulp of the largest tap; opt-in).
 */
#ifndef DISCORPY_HIP_H
#define DISCORPY_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden and an export list (csrc/exports.map): exactly these entry points are visible */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define DCP_OK 0
#define DCP_ERR_INVALID_ARG (-1)
#define DCP_ERR_HIP (-2)
#define DCP_ERR_UNSUPPORTED (-3)
#define DCP_ERR_NO_DEVICE (-4)

#define DCP_MEM_HOST 0
#define DCP_MEM_DEVICE 1
/* DCP_MEM_DEVICE for callers that hand over INDEPENDENT frames one call at a time (a camera loop, the channels of demo_06.py:111-113):
 * the kernel is enqueued on `stream` with the barrier bit of its dispatch packet cleared (hipExtAnyOrderLaunch), so its first
 * workgroups may start while the last workgroups of the PREVIOUS kernel on that stream still run -- the drain of one frame under
 * the ramp of the next, which is what dcp_unwarp_images_f32 gets from one launch (profiles/r06a_dispatch_modes.txt).  The caller
 * vouches that the call reads nothing an unfinished earlier call on the stream writes and writes nothing it reads or writes;
 * events, copies and synchronisations on the stream still wait for every earlier launch.  Accepted by dcp_unwarp_image_f32,
 * dcp_perspective_image_f32 and dcp_unwarp_fused_f32 (orders 0 / 1), and by dcp_unwarp_images_f32, whose frames then go one by
 * one, each unordered; DCP_ERR_INVALID_ARG elsewhere. */
#define DCP_MEM_DEVICE_UNORDERED 0x101

#define DCP_BLEND_SCIPY 0
#define DCP_BLEND_F64LERP 1
#define DCP_BLEND_F32LERP 2

#define DCP_COORD_F32 0
#define DCP_COORD_F64 1

#define DCP_MAX_FACT 32

/* ---- library / device ---- */
int dcp_version(void);                 /* major*10000 + minor*100 + patch */
int dcp_device_count(void);            /* number of HIP devices, 0 if none / no driver */
const char* dcp_last_error(void);

/* Device scratch the library keeps between calls -- the calling thread's staging buffers and streams for
 * DCP_MEM_HOST calls (grow-only, otherwise freed when the thread ends) and the per-device float64 planes of the
 * spline path, and the per-calibration frame plans of every device (the devices are synchronised first) -- is released; the next
 * call allocates again.  For long-running services. */
int dcp_release_scratch(void);

/* Options (process-wide).  The documented ones:
 *   "stack_chunk_kb"  KiB of one projection chunk when a HOST stack is streamed through the GPU (device scratch = 4 chunks; default 24576)
 *   "host_duplex"     host frames of the radial map through the GPU in bands of rows, uploads and downloads at the same time:
 *                     0 never, 1 (default) when a one-off probe finds that the HIP runtime overlaps the two directions, 2 always
 *   "host_bands"      number of those bands (default 6; where uploads and downloads are both runtime copies the frame travels in twice as
 *                     many, the first and last ones shorter -- 128, 256, 512 .. rows -- so that the stretch with one direction idle is short)
 *   "host_direct"     0: never write a host frame's result straight into registered host memory; 1 (default): when the runtime
 *                     cannot overlap an upload with a download; 2: whenever the destination is registered
 *   "host_direct_applies"   read-only: 1 if "host_direct" = 1 takes effect on this runtime (measured once; needs a device)
 *   "tile_cert"       0: never trust the host's tile-deviation certificate -- every staged kernel then verifies every pixel's taps
 *                     against its source box (default 1)
 *   "lds_gather"      0: no LDS-staged kernels at all: every tap a global load (default 1)
 * Every other switch of the library (which kernel takes a call, tile orders, chunk sizes: what the A/B runs under tools/ and the
 * parity campaigns flip) answers only to its name prefixed with "x_"; those are not part of this interface and may change
 * (list: csrc/api_core.cpp, dcp_set_option).  Returns DCP_ERR_INVALID_ARG for an unknown key. */
int dcp_set_option(const char* key, int value);
int dcp_get_option(const char* key, int* value);

/* ---- the hot path ---- */

/* discorpy/post/postprocessing.py:111-148  unwarp_image_backward
 * dst[y,x] = sample(src, clip(yc + B*yu), clip(xc + B*xu)),  B = sum_i list_fact[i] * ru^i,
 * xu = x - xcenter, yu = y - ycenter, ru = sqrt(xu^2 + yu^2), evaluated in float64.
 * coord_round_f32 = 1 rounds the clipped coordinates to float32 as :144-145 does. */
int dcp_unwarp_image_f32(const float* src, float* dst, int64_t height, int64_t width,
                         int64_t src_row_stride, int64_t src_col_stride, double xcenter, double ycenter,
                         const double* list_fact, int nfact, int order, int coord_round_f32, int blend_mode,
                         int mem_kind, int device, void* stream);

/* unwarp_image_backward (discorpy/post/postprocessing.py:111-148) over `nframes` images of ONE shape in one call, every
 * frame with its own source, destination, centre and coefficient vector -- the reference's callers loop over channels
 * (examples/readthedocs_demo/demo_06.py:111-113, demo_07.py:58-60), cameras or candidate calibrations (example_05.py:62-65),
 * one call per image.  srcs[i] / dsts[i]: the frames (all with the strides given); xcenters[i], ycenters[i]; list_facts:
 * nframes x nfact, row-major (pad shorter vectors with zeros: the result does not change).  Device-resident dense
 * float32 frames (unit column stride, coord_round_f32 = 1, nfact <= 10) whose calibrations all hold the tile certificate
 * run as ONE launch per 55 frames (35 above 5 coefficients) with the workgroup's frame in blockIdx.z, so that the drain of
 * one frame overlaps the ramp of the next (a 4096 x 4096 frame: ~25 us instead of ~31 us per frame); anything else is
 * processed frame by frame through dcp_unwarp_image_f32.  Results are bit-identical to nframes separate calls. */
int dcp_unwarp_images_f32(const float* const* srcs, float* const* dsts, int nframes, int64_t height, int64_t width,
                          int64_t src_row_stride, int64_t src_col_stride, const double* xcenters, const double* ycenters,
                          const double* list_facts, int nfact, int order, int coord_round_f32, int blend_mode, int mem_kind,
                          int device, void* stream);

/* discorpy/post/postprocessing.py:444-459 (_generate_perspective_map) + :486-492
 * (correct_perspective_image, map_index=None).  list_coef = c1..c8 of the backward homography in
 * (x, y) convention (discorpy/proc/processing.py:1254-1270). */
int dcp_perspective_image_f32(const float* src, float* dst, int64_t height, int64_t width,
                              int64_t src_row_stride, int64_t src_col_stride, const double* list_coef,
                              int order, int blend_mode, int mem_kind, int device, void* stream);

/* One-pass composition (BASELINE config 3): the float32-rounded perspective coordinate of
 * :453-457 is fed to the radial map of :141-145 and the source is sampled once.  NOT equal to
 * calling the two functions above in sequence (that is two resamplings, demo_05.py:127,147). */
int dcp_unwarp_fused_f32(const float* src, float* dst, int64_t height, int64_t width, int64_t src_row_stride,
                         int64_t src_col_stride, double xcenter, double ycenter, const double* list_fact,
                         int nfact, const double* list_coef, int order, int blend_mode, int mem_kind,
                         int device, void* stream);

/* discorpy/post/postprocessing.py:489-491 (map_index given) and :250-251 (_mapping):
 * dst[i] = sample(src, ycoord[i], xcoord[i]) for npts caller-supplied coordinates of type
 * coord_dtype (DCP_COORD_F32 / DCP_COORD_F64), clamped to the image (scipy's mode='nearest'). */
int dcp_remap_coords_f32(const float* src, float* dst, int64_t height, int64_t width, int64_t src_row_stride,
                         int64_t src_col_stride, const void* ycoord, const void* xcoord, int coord_dtype,
                         int64_t npts, int order, int blend_mode, int mem_kind, int device, void* stream);

/* The same with the reference's `mode` argument honoured for coordinates OUTSIDE the image, as
 * scipy.ndimage.map_coordinates -- which postprocessing.py:489-491 hands `map_index` and `mode` to -- treats them at
 * orders 0 and 1: boundary_mode is the index of the mode in the reference's docstring order (0 reflect, 1 grid-mirror,
 * 2 constant, 3 grid-constant, 4 nearest, 5 mirror, 6 grid-wrap, 7 wrap; cval = 0).  Such points are computed in double
 * in scipy's operation order whatever blend_mode says; points inside the image are what dcp_remap_coords_f32 returns. */
int dcp_remap_coords_mode_f32(const float* src, float* dst, int64_t height, int64_t width, int64_t src_row_stride,
                              int64_t src_col_stride, const void* ycoord, const void* xcoord, int coord_dtype,
                              int64_t npts, int order, int boundary_mode, int blend_mode, int mem_kind, int device,
                              void* stream);

/* discorpy/post/postprocessing.py:188-229 (unwarp_slice_backward: nrows = 1, coord_round_f32 = 0)
 * and :255-313 (unwarp_chunk_slices_backward: coord_round_f32 = 1) over a (depth, height, width)
 * stack: out[d, r, x] (dense, depth x nrows x width) = projection d sampled bilinearly at the
 * radial source coordinate of output pixel (row_start + r, x).  proj_stride / row_stride are the
 * element strides of `vol` between projections / rows.
 * coord_round_f32 = 2: float32 coordinates under unwarp_image_backward's semantics (:141-148) -- the projections are the FRAMES of a
 * (n, height, width) array corrected with one calibration: every coordinate is clipped to the whole frame and the chunk function's
 * row band [yd_min, yd_max) (:289-301) plays no part, so a model that folds rows gives exactly what n calls of
 * dcp_unwarp_image_f32 give.  The requested rows must lie inside the frame.  (dcp_unwarp_images_f32 routes frames of one
 * calibration this way by itself; dcp_unwarp_stack_rows_typed accepts the value too.) */
int dcp_unwarp_stack_rows_f32(const float* vol, float* out, int64_t depth, int64_t height, int64_t width,
                              int64_t proj_stride, int64_t row_stride, double xcenter, double ycenter,
                              const double* list_fact, int nfact, double row_start, int64_t nrows,
                              int coord_round_f32, int blend_mode, int mem_kind, int device, void* stream);

/* dcp_unwarp_stack_rows_f32 under `ncentres` calibrations that differ in the centre of distortion only, in one call -- the grid
 * search of examples/example_05.py:62-65 (unwarp_slice_backward 11 x 11 = 121 times on one stack of 600 projections, one call per
 * candidate centre).  out = (ncentres, depth, nrows, width), dense; block k is what dcp_unwarp_stack_rows_f32 returns for
 * (xcenters[k], ycenters[k]), bit for bit.  One launch per 224 centres: the two or three source rows a sinogram needs of each
 * projection are fetched from HBM once and served to every centre by the L2 (device-resident stacks); a host stack is shipped
 * once -- the union of the centres' row bands -- instead of once per centre.  coord_round_f32 = 1 under a model that may fold
 * rows out of the reference's band is processed centre by centre. */
int dcp_unwarp_stack_rows_centres_f32(const float* vol, float* out, int64_t depth, int64_t height, int64_t width, int64_t proj_stride,
                                      int64_t row_stride, const double* xcenters, const double* ycenters, int ncentres,
                                      const double* list_fact, int nfact, double row_start, int64_t nrows, int coord_round_f32,
                                      int blend_mode, int mem_kind, int device, void* stream);

/* The same over a HOST-resident stack sharded across `ndev` GPUs of this process (SURVEY.md section
 * 8(e): projections are independent).  devices[i] takes the i-th contiguous depth shard (sizes as
 * numpy.array_split), stages it, runs the kernel and copies its block of `out` (depth x nrows x width,
 * host) back; the shards run concurrently on one host thread each.  For DEVICE-resident shards use one
 * process per GPU and an RCCL all-gather (discorpy_amd/stack.py). */
int dcp_unwarp_stack_rows_multi_f32(const float* vol, float* out, int64_t depth, int64_t height, int64_t width,
                                    int64_t proj_stride, int64_t row_stride, double xcenter, double ycenter,
                                    const double* list_fact, int nfact, double row_start, int64_t nrows,
                                    int coord_round_f32, int blend_mode, const int* devices, int ndev);

/* Device-resident depth shards on the GPUs of ONE process and the exchange by direct peer copies (no torch, no RCCL):
 * slot g holds projections [d0_g, d1_g) -- the split of numpy.array_split(range(depth), ndev) -- at vol[g] on
 * devices[g]; its kernel writes its (d1_g - d0_g, nrows, width) block, and with gather != 0 every slot's block is
 * pushed into the depth-outer (depth, nrows, width) result out[h] of every other slot with hipMemcpyPeerAsync (on an
 * 8-GPU node: seven pushes per device, one per xGMI link).  out[g] holds (depth, nrows, width) floats when gathering
 * (slot g writes at depth offset d0_g), (d1_g - d0_g, nrows, width) otherwise.  A device may appear in several slots.
 * Returns after every stream has drained.  Reference: the loops over depth of postprocessing.py:226-228, 310-312 carry no
 * state, so the projections may be split anywhere; the reference itself has no multi-device code. */
int dcp_unwarp_stack_rows_peer_f32(const float* const* vol, float* const* out, int64_t depth, int64_t height, int64_t width,
                                   int64_t proj_stride, int64_t row_stride, double xcenter, double ycenter,
                                   const double* list_fact, int nfact, double row_start, int64_t nrows, int coord_round_f32,
                                   int blend_mode, const int* devices, int ndev, int gather);

/* ---- one process per GPU: the depth-sharded stack and ONE RCCL all-gather over xGMI, without torch ----
 * (north star / SURVEY.md section 8(e); the reference has no multi-device code: its loops over depth,
 * discorpy/post/postprocessing.py:226-228 and 310-312, carry no state, so the projections may be split anywhere.)
 * librccl.so is loaded on first use from the directory of the HIP runtime the process runs on (DCP_RCCL_PATH overrides);
 * every function below returns DCP_ERR_UNSUPPORTED when it cannot be loaded.
 *   dcp_rccl_unique_id      ncclGetUniqueId: 128 bytes that ONE rank creates and the caller ships to the others (MPI, a file, a socket)
 *   dcp_rccl_comm_create    ncclCommInitRank on `device` (collective: every rank of the world calls it), plus the side stream of the
 *                           pipelined exchange; dcp_rccl_comm_destroy releases both
 *   dcp_unwarp_stack_rows_rccl_f32
 *       COLLECTIVE: every rank of the communicator makes the call.  This rank holds `depth_local` projections at `vol` and a
 *       result buffer `out` of (sum of all ranks' depth_local, nrows, width) floats on the communicator's device.  The ranks first
 *       agree on their shard shapes (one all-gather of 40 bytes per rank on the communicator's side stream; the caller's stream is
 *       not waited for): nrows, width and pipeline must be the same everywhere, depth_local may differ from rank to rank and may
 *       be 0 (the shards are laid down in rank order), and a rank whose own arguments are unusable says so there -- a
 *       disagreement makes EVERY rank return DCP_ERR_INVALID_ARG from this call, none is left waiting in a collective.  Then the
 *       stack kernel (dcp_unwarp_stack_rows_f32) writes this rank's block in place at its depth offset and the exchange fills in
 *       the other ranks' blocks -- depth is the outer axis of the result, so every contribution is one contiguous block: equal
 *       shards, pipeline <= 1: ONE ncclAllGather in place on `stream` behind the kernel; ragged shards: one group of
 *       ncclBroadcasts with per-rank counts.  pipeline > 1: every shard is cut into that many depth sub-blocks and the exchange of
 *       sub-block s (grouped ncclBroadcasts on the side stream) overlaps the kernel of sub-block s + 1.  Stream-ordered: returns
 *       without waiting for the result, `stream` is complete when the whole (depth, nrows, width) result is.  After a HIP / RCCL
 *       failure on one rank the others may be blocked in their collectives: destroy the communicator (the caller's stream is
 *       re-joined to the side stream on every path, so nothing is left running behind the caller's back).
 *       The agreement is a HOST wait on the side stream, and RCCL serialises the operations of one communicator: a call therefore also
 *       waits for the previous call's exchange (back-to-back calls do not overlap) -- unless
 *   dcp_rccl_comm_fixed_shards(comm, 1)
 *       has been set, by which the caller vouches ON EVERY RANK that the following calls repeat the depth_local / nrows / width /
 *       pipeline of the last agreed call: the agreement is skipped (no collective, no host wait) and the call is stream-ordered end to
 *       end.  A rank that then passes other shapes gets DCP_ERR_INVALID_ARG; its peers are not told (destroy the communicator).
 *   dcp_rccl_comm_info
 *       what the communicator ITSELF reports, so that a multi-GPU run can prove what RCCL saw rather than what the launcher claimed:
 *       info[0] ncclCommCount, [1] ncclCommUserRank, [2] ncclCommCuDevice, [3] ncclGetVersion (-1 each where the loaded library lacks
 *       the query), [4] / [5] the world size / rank given to dcp_rccl_comm_create, [6] the HIP device, [7] 1 if a shard agreement is
 *       in force, [8] exchanges done, [9] agreements done (up to `ninfo` values are written); shard_depths[r] = depth_local of rank r
 *       as agreed in the last exchange (-1 without one; up to `nshards`); librccl_path = the file the ncclXxx symbols were bound
 *       from (DCP_RCCL_PATH, the librccl.so next to the loaded HIP runtime, or the search path).  Not a collective. */
int dcp_rccl_available(void);
int dcp_rccl_unique_id(void* id, size_t bytes);
int dcp_rccl_comm_create(void** comm, int world_size, int rank, const void* id, int device);
int dcp_rccl_comm_destroy(void* comm);
int dcp_rccl_comm_fixed_shards(void* comm, int on);
int dcp_rccl_comm_info(void* comm, int64_t* info, int ninfo, int64_t* shard_depths, int nshards, char* librccl_path, size_t path_bytes);
int dcp_unwarp_stack_rows_rccl_f32(const float* vol, float* out, int64_t depth_local, int64_t height, int64_t width, int64_t proj_stride,
                                   int64_t row_stride, double xcenter, double ycenter, const double* list_fact, int nfact, double row_start,
                                   int64_t nrows, int coord_round_f32, int blend_mode, void* comm, int pipeline, void* stream);

/* ---- spline orders 2..5 (scipy.ndimage.map_coordinates with its B-spline prefilter) ----
 * The same maps as dcp_unwarp_image_f32 / dcp_perspective_image_f32 / dcp_remap_coords_f32 for
 * `order` in 2..5 -- what the reference computes when a caller passes order >= 2
 * (discorpy/post/postprocessing.py:147, 491; examples/readthedocs_demo/demo_07.py:60 uses 3).  Here the
 * boundary mode matters (prefilter boundary condition, tap folding, 12-sample padding for 'nearest'
 * and 'grid-constant'):  0 reflect, 1 grid-mirror, 2 constant, 3 grid-constant, 4 nearest, 5 mirror,
 * 6 grid-wrap, 7 wrap.  Results are within one float32 ulp of scipy's.  A float64 coefficient plane
 * of (height + 2 pad) x (width + 2 pad) is kept per device by the library. */
/* OR-ed into `boundary_mode` of the spline entry points (and of the *_typed ones at orders >= 2): accumulate the (order + 1)^2 taps
 * of a point in scipy's operation order, t += (c * wy) * wx tap by tap.  Without it the LDS-staged gather of certified maps on
 * whole frames sums them factorised and fused -- sum_j wy_j (sum_q c_jq wx_q): 20 float64 operations instead of 48 at order 3 --,
 * which differs from scipy's sum in the last bits of the float64 value, i.e. in the float32 result of ~1 pixel in 1e8 (the
 * spline orders' contract is "within one float32 ulp of scipy's" either way).  Python: blend="scipy". */
#define DCP_SPLINE_SCIPY_SUM 0x100
#define DCP_MODE_REFLECT 0
#define DCP_MODE_GRID_MIRROR 1
#define DCP_MODE_CONSTANT 2
#define DCP_MODE_GRID_CONSTANT 3
#define DCP_MODE_NEAREST 4
#define DCP_MODE_MIRROR 5
#define DCP_MODE_GRID_WRAP 6
#define DCP_MODE_WRAP 7
int dcp_unwarp_image_spline_f32(const float* src, float* dst, int64_t height, int64_t width, int64_t src_row_stride,
                                int64_t src_col_stride, double xcenter, double ycenter, const double* list_fact,
                                int nfact, int order, int boundary_mode, int mem_kind, int device, void* stream);
int dcp_perspective_image_spline_f32(const float* src, float* dst, int64_t height, int64_t width,
                                     int64_t src_row_stride, int64_t src_col_stride, const double* list_coef, int order,
                                     int boundary_mode, int mem_kind, int device, void* stream);
int dcp_remap_coords_spline_f32(const float* src, float* dst, int64_t height, int64_t width, int64_t src_row_stride,
                                int64_t src_col_stride, const void* ycoord, const void* xcoord, int coord_dtype,
                                int64_t npts, int order, int boundary_mode, int mem_kind, int device, void* stream);
/* the one-pass perspective -> radial map of dcp_unwarp_fused_f32 at a spline order */
int dcp_unwarp_fused_spline_f32(const float* src, float* dst, int64_t height, int64_t width, int64_t src_row_stride,
                                int64_t src_col_stride, double xcenter, double ycenter, const double* list_fact,
                                int nfact, const double* list_coef, int order, int boundary_mode, int mem_kind, int device,
                                void* stream);

/* ---- element types other than float32 ----
 * The reference hands `mat` to scipy.ndimage.map_coordinates whatever its dtype
 * (discorpy/post/postprocessing.py:147, 227, 251, 491): every element is read as a double, the blend
 * runs in double in scipy's operation order, and the result is converted to the INPUT's type -- a C
 * cast for floats; for integers round-half-away-from-zero and saturation.  The *_typed entry points
 * do that for `dtype` = DCP_DTYPE_*, orders 0..5 (`boundary_mode` matters for orders >= 2 only); `src` and `dst` hold elements of `dtype`, strides in elements.
 * DCP_DTYPE_F32 is accepted too (exact scipy blend; the *_f32 entry points are the fast path).
 * dcp_unwarp_stack_rows_typed: out_float32 = 1 stores float32 values of the result already converted
 * to `dtype`, as unwarp_slice_backward assigns into its float32 sinogram (:224-227). */
#define DCP_DTYPE_F32 0
#define DCP_DTYPE_F64 1
#define DCP_DTYPE_U8 2
#define DCP_DTYPE_I8 3
#define DCP_DTYPE_U16 4
#define DCP_DTYPE_I16 5
#define DCP_DTYPE_U32 6
#define DCP_DTYPE_I32 7
#define DCP_DTYPE_I64 8  /* read as a double (rounds above 2^53), stored as scipy's cast does on x86-64: see dcp_device.h to_elem */
#define DCP_DTYPE_U64 9
#define DCP_DTYPE_BOOL 10 /* numpy bool_: one byte, 0 / 1; the double result is truncated on the way out */
int dcp_unwarp_image_typed(const void* src, void* dst, int dtype, int64_t height, int64_t width, int64_t src_row_stride,
                           int64_t src_col_stride, double xcenter, double ycenter, const double* list_fact, int nfact,
                           int order, int boundary_mode, int mem_kind, int device, void* stream);
/* discorpy/post/postprocessing.py:151-185 (unwarp_image_forward): every source pixel (y, x) is MOVED to
 *   (yu, xu) = rint(clip(centre + F(rd) * (p - centre), 0, size - 1)),  F(rd) = sum_i list_fact[i] * rd^i,
 * float64 throughout, rint rounding half to even as np.round does.  Where several source pixels meet, the one with the greatest
 * row-major index y * width + x stays (NumPy's assignment order); destinations nobody reaches are all-zero bytes.  Elements are
 * copied, never computed with: any DCP_DTYPE_*, NaN payloads and -0.0 included.  dst is dense (height x width) and must not overlap
 * src.  A coordinate that is not a number goes to index 0.  Two launches (forward_winner_kernel: one 32-bit atomic maximum per source
 * pixel into a height * width word plane of the library's per-stream workspace; forward_fill_kernel) on `stream`; host memory is
 * staged whole.  height * width >= 2^32 - 1: DCP_ERR_UNSUPPORTED. */
int dcp_unwarp_image_forward(const void* src, void* dst, int dtype, int64_t height, int64_t width, int64_t src_row_stride,
                             int64_t src_col_stride, double xcenter, double ycenter, const double* list_fact, int nfact,
                             int mem_kind, int device, void* stream);
int dcp_perspective_image_typed(const void* src, void* dst, int dtype, int64_t height, int64_t width,
                                int64_t src_row_stride, int64_t src_col_stride, const double* list_coef, int order,
                                int boundary_mode, int mem_kind, int device, void* stream);
int dcp_unwarp_fused_typed(const void* src, void* dst, int dtype, int64_t height, int64_t width, int64_t src_row_stride,
                           int64_t src_col_stride, double xcenter, double ycenter, const double* list_fact, int nfact,
                           const double* list_coef, int order, int boundary_mode, int mem_kind, int device, void* stream);
int dcp_remap_coords_typed(const void* src, void* dst, int dtype, int64_t height, int64_t width, int64_t src_row_stride,
                           int64_t src_col_stride, const void* ycoord, const void* xcoord, int coord_dtype, int64_t npts,
                           int order, int boundary_mode, int mem_kind, int device, void* stream);
int dcp_unwarp_stack_rows_typed(const void* vol, void* out, int dtype, int out_float32, int64_t depth, int64_t height,
                                int64_t width, int64_t proj_stride, int64_t row_stride, double xcenter, double ycenter,
                                const double* list_fact, int nfact, double row_start, int64_t nrows, int coord_round_f32,
                                int mem_kind, int device, void* stream);

/* discorpy/util/utility.py:278-342 (unwarp_color_image_backward), the part after np.pad: an interleaved
 * (height, width, channels) image of `dtype`, every channel sampled at the same radial coordinate
 * (:320-341 loops map_coordinates over mat_pad[:, :, i]) -- one coordinate evaluation and `channels`
 * blends per pixel, orders 0 / 1.  src_pixel_stride = elements between pixels (>= channels); dst is dense
 * (height, width, channels).
 *   dcp_unwarp_color_image     blend_mode DCP_BLEND_SCIPY (scipy's exact arithmetic: bit-equal to the reference) or, for
 *                              float32 pixels, DCP_BLEND_F64LERP (within one float32 ulp of it: what dcp_unwarp_image_f32 computes
 *                              per plane by default); integer element types always blend in scipy's order.  Dense pixels of 3 or 4
 *                              float32 / uint8 / uint16 channels under a certified calibration take the workgroup-box kernel
 *                              (remap_wg_color_kernel: the source box of a 128 x 16 tile staged in LDS once for all channels),
 *                              everything else one thread per pixel -- the same values either way
 *   dcp_unwarp_image_channels  the same with DCP_BLEND_SCIPY (kept for callers of the earlier ABI) */
int dcp_unwarp_color_image(const void* src, void* dst, int dtype, int64_t height, int64_t width, int channels, int64_t src_row_stride,
                           int64_t src_pixel_stride, double xcenter, double ycenter, const double* list_fact, int nfact, int order,
                           int blend_mode, int mem_kind, int device, void* stream);
int dcp_unwarp_image_channels(const void* src, void* dst, int dtype, int64_t height, int64_t width, int channels,
                              int64_t src_row_stride, int64_t src_pixel_stride, double xcenter, double ycenter,
                              const double* list_fact, int nfact, int order, int mem_kind, int device, void* stream);

/* Interleaved pixels under the homography, and under the one-pass perspective -> radial map.  The reference's demos loop
 * post.correct_perspective_image(mat[:, :, i], list_coef) over the channels of a colour photograph
 * (examples/readthedocs_demo/demo_07.py:25,60; demo_05.py:127,147 corrects the radial distortion and then the perspective of the
 * same image): per channel the coordinates of discorpy/post/postprocessing.py:444-459 and the map_coordinates call of :462-492.
 * Here one coordinate evaluation and `channels` blends per pixel, orders 0 / 1; arguments, blend_mode rule and kernel choice as
 * dcp_unwarp_color_image (the staged kernel under the level-2 certificate of the map's kind, else one thread per pixel -- the same
 * values either way, and the same as dcp_perspective_image_f32 / _typed and dcp_unwarp_fused_f32 / _typed give per plane). */
int dcp_perspective_color_image(const void* src, void* dst, int dtype, int64_t height, int64_t width, int channels, int64_t src_row_stride,
                                int64_t src_pixel_stride, const double* list_coef, int order, int blend_mode, int mem_kind, int device,
                                void* stream);
int dcp_unwarp_fused_color_image(const void* src, void* dst, int dtype, int64_t height, int64_t width, int channels, int64_t src_row_stride,
                                 int64_t src_pixel_stride, double xcenter, double ycenter, const double* list_fact, int nfact,
                                 const double* list_coef, int order, int blend_mode, int mem_kind, int device, void* stream);

/* The same three interleaved-pixel calls at spline orders 2..5 (the reference's examples/readthedocs_demo/demo_07.py:60 corrects a
 * colour photograph channel by channel with order=3): every channel of the result is bit for bit what the single-plane spline
 * entry point (dcp_unwarp_image_spline_f32 / _typed and their perspective and fused siblings) returns for that channel's
 * column-strided view.  Arguments as dcp_unwarp_color_image / dcp_perspective_color_image / dcp_unwarp_fused_color_image with
 * boundary_mode in place of blend_mode: DCP_MODE_* (0..7), optionally OR-ed with DCP_SPLINE_SCIPY_SUM.  Any DCP_DTYPE_*, order 2..5,
 * channels 1..4, src_pixel_stride >= channels, rows that do not overlap; anything else is DCP_ERR_INVALID_ARG or
 * DCP_ERR_UNSUPPORTED before any device call.  mem_kind: DCP_MEM_HOST or DCP_MEM_DEVICE (a call of several kernels cannot honour
 * DCP_MEM_DEVICE_UNORDERED).  The single-plane prefilter runs once per channel, reading the channel in place, into a workspace of
 * channels + 1 float64 planes; ONE gather follows, which evaluates a pixel's coordinate once for all its channels --
 * spline_wg_color_kernel (the coefficient box of a 128 x 32 tile staged in LDS, channel after channel) under the level-2
 * certificate of a radial or perspective map on frames of at least one tile, else spline_remap_color_kernel (one thread per pixel).
 * Host memory: the interleaved extent goes up once, the dense (height, width, channels) result comes back once.  dcp_last_kernel
 * reports the prefilter's kernels followed by "+ spline_wg_color_kernel<order=N, channels=C>" or
 * "+ spline_remap_color_kernel<order=N, channels=C>".  Timings against the plane-by-plane route: not measured. */
int dcp_unwarp_color_image_spline(const void* src, void* dst, int dtype, int64_t height, int64_t width, int channels, int64_t src_row_stride,
                                  int64_t src_pixel_stride, double xcenter, double ycenter, const double* list_fact, int nfact, int order,
                                  int boundary_mode, int mem_kind, int device, void* stream);
int dcp_perspective_color_image_spline(const void* src, void* dst, int dtype, int64_t height, int64_t width, int channels,
                                       int64_t src_row_stride, int64_t src_pixel_stride, const double* list_coef, int order, int boundary_mode,
                                       int mem_kind, int device, void* stream);
int dcp_unwarp_fused_color_image_spline(const void* src, void* dst, int dtype, int64_t height, int64_t width, int channels,
                                        int64_t src_row_stride, int64_t src_pixel_stride, double xcenter, double ycenter,
                                        const double* list_fact, int nfact, const double* list_coef, int order, int boundary_mode, int mem_kind,
                                        int device, void* stream);

/* ---- out-of-core stacks ----
 * The reference never touches more of a projection than mat3D[i, yd_min:yd_max, :]
 * (discorpy/post/postprocessing.py:221-228, 295-301), which is what lets it run on an HDF5 dataset
 * larger than memory.  dcp_stack_row_band reports that band for a request (rows row_start ..
 * row_start + nrows - 1): source rows [band_start, band_start + band_rows).  dcp_unwarp_stack_band is
 * dcp_unwarp_stack_rows_f32 / _typed for a buffer that holds ONLY the rows [band_start, band_start +
 * band_rows) of each of `depth` projections (row_stride / proj_stride: element strides inside that
 * buffer); it fails with DCP_ERR_INVALID_ARG if the request needs rows outside the band.  dtype
 * DCP_DTYPE_F32 with out_float32 = 0 runs the tuned kernel with `blend_mode`; every other combination
 * uses scipy's exact blend. */
int dcp_stack_row_band(int64_t height, int64_t width, double xcenter, double ycenter, const double* list_fact, int nfact,
                       double row_start, int64_t nrows, int64_t* band_start, int64_t* band_rows);
int dcp_unwarp_stack_band(const void* band, void* out, int dtype, int out_float32, int64_t depth, int64_t height,
                          int64_t width, int64_t band_start, int64_t band_rows, int64_t proj_stride, int64_t row_stride,
                          double xcenter, double ycenter, const double* list_fact, int nfact, double row_start,
                          int64_t nrows, int coord_round_f32, int blend_mode, int mem_kind, int device, void* stream);

/* The float32 source-coordinate planes themselves, ymap / xmap of height*width floats each:
 * DCP_MAP_RADIAL       yd_mat / xd_mat of unwarp_image_backward, discorpy/post/postprocessing.py:141-145
 * DCP_MAP_PERSPECTIVE  _generate_perspective_map, :444-459 (list_fact ignored)
 * DCP_MAP_FUSED        the composed map of dcp_unwarp_fused_f32
 * for callers that reuse a map (map_index= of correct_perspective_image :478-479, cv2.remap as in
 * discorpy/util/utility.py:425-435).  Feeding the planes to dcp_remap_coords_f32 reproduces the
 * corresponding image entry point bit for bit. */
#define DCP_MAP_RADIAL 0
#define DCP_MAP_PERSPECTIVE 1
#define DCP_MAP_FUSED 2
int dcp_coordinate_map_f32(float* ymap, float* xmap, int64_t height, int64_t width, int map_kind, double xcenter,
                           double ycenter, const double* list_fact, int nfact, const double* list_coef, int mem_kind,
                           int device, void* stream);

/* `nframes` frames of ONE calibration under the homography (map_kind DCP_MAP_PERSPECTIVE: the coordinates of
 * discorpy/post/postprocessing.py:444-459 and the map_coordinates call of :486-492; xcenter, ycenter and list_fact ignored) or under the
 * one-pass perspective -> radial map of dcp_unwarp_fused_f32 (DCP_MAP_FUSED: both) -- the loop a caller writes around
 * examples/readthedocs_demo/demo_05.py:127,147 for every frame of a run, a detector stack or a video.  DCP_MAP_RADIAL is refused: frames
 * under the radial map alone are the projections of a stack (dcp_unwarp_stack_rows_f32 / _typed).
 *   src   frames `frame_stride` elements apart (not overlapping), rows `row_stride` elements apart, unit column stride
 *   dst   dense (nframes, height, width), elements of `dtype` (any DCP_DTYPE_*) like the source
 *   order 0 or 1; blend_mode applies to DCP_DTYPE_F32 only (every other type blends in scipy's order)
 * Device frames of float32, uint8 or uint16 at order 1 whose map holds the level-2 tile certificate of its kind run in ONE launch
 * (stack_wg_kernel: the coordinates of a 128 x 32 tile evaluated once for all frames of a depth chunk) when the launch is large enough;
 * everything else -- order 0, other element types, an uncertified or untame homography, few small frames, host memory -- goes through
 * the single-frame entry point frame by frame on the same stream.  Every frame equals what dcp_perspective_image_f32 / _typed or
 * dcp_unwarp_fused_f32 / _typed give for it bit for bit either way; dcp_debug_last_kernel() names the path taken.  nframes = 0 is DCP_OK. */
int dcp_remap_frames_typed(const void* src, void* dst, int dtype, int map_kind, int64_t nframes, int64_t height, int64_t width,
                           int64_t frame_stride, int64_t row_stride, double xcenter, double ycenter, const double* list_fact,
                           int nfact, const double* list_coef, int order, int blend_mode, int mem_kind, int device, void* stream);

/* `nframes` frames of ONE calibration at spline orders 2..5 -- the loop a caller writes around unwarp_image_backward(frame, ..., order=3)
 * (discorpy/post/postprocessing.py:111-148; examples/readthedocs_demo/demo_07.py:25,60 per frame of a series), around
 * correct_perspective_image (:444-459, 462-492) or around both corrections (demo_05.py:127,147) -- with ONE evaluation of a pixel's
 * source coordinate for all frames of a launch.  Every frame of the result is bit for bit what the single-frame spline entry point
 * (dcp_unwarp_image_spline_f32 / dcp_unwarp_image_typed and their perspective and fused siblings) returns for it.
 *   map_kind  DCP_MAP_RADIAL, DCP_MAP_PERSPECTIVE or DCP_MAP_FUSED; arguments the map does not use are ignored and may be null
 *   src       frames `frame_stride` elements apart (not overlapping, unless nframes = 1), rows `row_stride` elements apart, unit column stride
 *   dst       dense (nframes, height, width), elements of `dtype` (any DCP_DTYPE_*) like the source
 *   order     2..5;  mode: DCP_MODE_* (0..7), optionally OR-ed with DCP_SPLINE_SCIPY_SUM
 *   mem_kind  DCP_MEM_HOST or DCP_MEM_DEVICE
 * Anything else is DCP_ERR_INVALID_ARG or DCP_ERR_UNSUPPORTED before any device call; nframes = 0 is DCP_OK with no launch.  The frames
 * are processed in groups: per group the single-plane prefilter runs once per frame, reading the frame in place, into a workspace of
 * (frames of the group + 1) float64 planes of at most 2 GiB, and ONE gather follows -- spline_wg_frames_kernel (the coefficient box of a
 * 128 x 32 tile staged in LDS, frame after frame) under the level-2 certificate of a radial or perspective map on frames of at least
 * one tile, else spline_remap_frames_kernel (one thread per pixel).  Host memory: per group the source extent goes up once and the
 * dense result comes back once.  dcp_debug_last_kernel() reports the last group's prefilter kernels followed by
 * "+ spline_wg_frames_kernel<order=N, frames=G>" or "+ spline_remap_frames_kernel<order=N, frames=G>". */
int dcp_remap_frames_spline(const void* src, void* dst, int dtype, int map_kind, int64_t nframes, int64_t height, int64_t width,
                            int64_t frame_stride, int64_t row_stride, double xcenter, double ycenter, const double* list_fact,
                            int nfact, const double* list_coef, int order, int mode, int mem_kind, int device, void* stream);

/* ---- preprocessing: the median filter ----
 * discorpy/prep/preprocessing.py:66 (normalization: scipy.ndimage.median_filter(mat, 51, mode="reflect")) and the 2 x 2 denoise step of
 * binarization: dst[y, x] = the element of rank (size_y * size_x) / 2 (0-based, ascending) among the size_y x size_x elements of src in
 * rows y - size_y / 2 .. y - size_y / 2 + size_y - 1 and the columns likewise (an even size leans to the lower indices and yields the
 * upper median, as scipy's does); an index i outside the image is reflected with period 2 n (i mod 2 n, then 2 n - 1 - i where that is
 * >= n), any number of times: the image may be smaller than the window.  A selection, not a computation: the result is one of the
 * window's elements, bit for bit, for every DCP_DTYPE_* (64-bit integers are compared exactly; -0.0 sorts below +0.0; NaNs are
 * undefined, as in scipy).  size_y = size_x = 1 copies.
 *   src   rows `src_row_stride` elements apart (>= width), unit column stride;  dst  dense (height, width), not overlapping src
 *   mem_kind  DCP_MEM_HOST (staged up and down by the library) or DCP_MEM_DEVICE (enqueued on `stream`)
 * A size, height or width below 1, a stride below the width, an unknown dtype or mem_kind and overlapping buffers are
 * DCP_ERR_INVALID_ARG, size_y * size_x >= 2^31 is DCP_ERR_UNSUPPORTED, all before any device call.  One launch: median_lds_kernel
 * (the order-preserving integer keys of a 64 x 16 / 8 / 4 tile's window box staged in LDS, a binary search on the key per pixel) where
 * such a box fits the CU's 160 KiB, else median_global_kernel (the same search, taps from global memory); dcp_debug_last_kernel()
 * names the one that ran.  A device-resident 2048 x 2048 float32 image at size 51: 22 ms (uint16 11 ms, uint8 5.5 ms). */
int dcp_median_filter_2d(const void* src, void* dst, int height, int width, long src_row_stride, int dtype, int size_y, int size_x,
                         int mem_kind, int device, void* stream);

/* ---- line and chessboard patterns: the Gaussian filter ----
 * discorpy/prep/linepattern.py:592,659,739 (scipy.ndimage.gaussian_filter): a symmetric 1-D correlation along axis 0 (weights_y, radius_y),
 * then along axis 1 (weights_x, radius_x) of the first pass's result ROUNDED TO THE ELEMENT TYPE, with scipy's arithmetic bit for bit.
 * One element of one pass, e the extended line read as doubles, w the 2 r + 1 weights:
 *     tmp = e[i] * w[r];   for j = -r .. -1:  tmp += (e[i + j] + e[i - j]) * w[r + j];      (float64, no fused multiply-add)
 * then a C cast to the element type (floats round to nearest, integers truncate toward zero; 64-bit integers are read through a
 * double; defined where the double lies within the type's range).  Position p of a line of length n, any integer p, under `mode`
 * (a DCP_MODE_*): REFLECT / GRID_MIRROR  q = p mod 2 n, 2 n - 1 - q where q >= n;  MIRROR  index 0 if n == 1, else q = p mod (2 n - 2),
 * 2 n - 2 - q where q >= n;  NEAREST  clipped;  WRAP / GRID_WRAP  p mod n;  CONSTANT / GRID_CONSTANT  the double `cval`, not cast to
 * the element type (in the second pass a column outside the image is cval too, not a filtered value).
 *   weights_*  HOST pointers to 2 * radius + 1 doubles, symmetric to the bit; NULL or radius -1 skips the axis (both: dst = src);
 *              radius <= 192 (sigma 48 at scipy's truncate = 4)
 *   src   rows `src_row_stride` elements apart (>= width), unit column stride;  dst  dense (height, width), not overlapping src
 *   dtype any DCP_DTYPE_* but BOOL;  mem_kind  DCP_MEM_HOST (staged up and down by the library) or DCP_MEM_DEVICE (enqueued on `stream`)
 * Asymmetric weights, a height or width below 1, a stride below the width, a radius below -1, an unknown dtype, mode or mem_kind and
 * overlapping buffers are DCP_ERR_INVALID_ARG, DCP_DTYPE_BOOL and a radius above 192 are DCP_ERR_UNSUPPORTED, all before any device
 * call.  One launch of gauss_lds_kernel (the source box of a 128 x 32 tile and the first pass's plane both in LDS) where both axes are
 * filtered with radii up to 24 and the planes take at most 80 KiB -- the range in which it measured no slower: 0.30 against 0.41 ms for a
 * device-resident 4096 x 4096 float32 image at sigma 3 --, else one launch of gauss_axis_kernel per axis (taps from global memory, the plane between the passes in the
 * library's scratch: dcp_release_scratch frees it; 1.05 ms at sigma 10); dcp_debug_last_kernel() names what ran. */
int dcp_correlate_sym_2d(const void* src, void* dst, int height, int width, long src_row_stride, int dtype,
                         const double* weights_y, int radius_y, const double* weights_x, int radius_x,
                         int mode, double cval, int mem_kind, int device, void* stream);

/* ---- line patterns: the Fourier Gaussian background filter ----
 * discorpy/prep/preprocessing.py:76-158 (_apply_fft_filter behind normalization_fft): on the image padded by `pad` on every side
 * (np.pad, sides Ny x Nx) the reference computes real(ifft2(fft2(m s) win) s) with s = (-1)^(x + y) and win a Gaussian centred on
 * ((Ny - 1) / 2, (Nx - 1) / 2), and crops the pad again.  s and win are products of a factor per axis, so the operator is
 * real(A_y m A_x^T) with one complex Toeplitz matrix per axis, A[j, k] = a(j - k); the call evaluates exactly that, without an FFT:
 *     P[j, x]  = sum_k a_y(j - k) m[k, x]                                   (cropped rows j, every padded column x; complex)
 *     dst[j, i] = sum_x a_x,re(i - x) P_re[j, x] - a_x,im(i - x) P_im[j, x]   (cropped columns i)
 * in float64 with fused multiply-adds, m read from src through the pad's index fold (no padded plane exists).
 *   taps_*   HOST pointers, per axis 2 N - 1 doubles each for the real and the imaginary part, N = side + 2 pad: entry d + N - 1 holds
 *            a(d), d = -(N - 1) .. N - 1, with a(d) = (-1)^d c[d mod N] and c the inverse DFT of the window's factor along the axis.
 *            The sums run over the taps with |d| <= R or |d| >= N - R only, R the smallest radius at which the taps left out sum to at
 *            most 2^-56 of the table's sum of |re| + |im| (an eighth of float64's unit roundoff on the result's scale); a narrow
 *            window keeps every tap.  The tables are read before the call returns.
 *   pad_mode np.pad's mode as a DCP_MODE_*, a position p of a line of length n folded as dcp_correlate_sym_2d folds it:
 *            DCP_MODE_MIRROR = "reflect" (period 2 n - 2; n = 1: index 0), DCP_MODE_REFLECT = "symmetric" (period 2 n),
 *            DCP_MODE_NEAREST = "edge", DCP_MODE_WRAP = "wrap" (p mod n), DCP_MODE_CONSTANT = "constant" with value 0; any number of
 *            folds (the pad may exceed the side).  The other DCP_MODE_* codes are refused.
 *   src      rows `src_row_stride` elements apart (>= width), unit column stride, any DCP_DTYPE_*, each element converted to double as
 *            NumPy converts it;  dst  dense (height, width) FLOAT64 whatever `dtype` is, not overlapping src
 *   mem_kind DCP_MEM_HOST (staged up and down by the library) or DCP_MEM_DEVICE (enqueued on `stream`)
 * A null table, pad < 0, an unknown pad_mode, a tap that is not finite and the refusals of every plane call are DCP_ERR_INVALID_ARG,
 * a padded side above 16384 is DCP_ERR_UNSUPPORTED, all before any device call.  The planes of P (2 * height * (width + 2 pad) doubles)
 * and the tables' device copies live in the library's scratch (dcp_release_scratch frees it).  The tables are copied to the device on
 * `stream` and THE CALL WAITS FOR THAT COPY (so for the work enqueued on `stream` before it) before it enqueues its two kernels: it cannot be captured
 * into a graph.  Kernels: fourier_rows_kernel<T> then fourier_cols_kernel (csrc/fourier_kernels.hip); dcp_debug_last_kernel() names
 * them with the number of taps kept per axis. */
int dcp_fourier_gauss_2d(const void* src, void* dst, int height, int width, long src_row_stride, int dtype,
                         int pad, int pad_mode,
                         const double* taps_y_re, const double* taps_y_im,   /* 2 * (height + 2 * pad) - 1 each */
                         const double* taps_x_re, const double* taps_x_im,   /* 2 * (width + 2 * pad) - 1 each */
                         int mem_kind, int device, void* stream);

/* ---- dot patterns: connected components, their measurements, hole filling ----
 * discorpy/prep/preprocessing.py:247-445 and :966-997 (scipy.ndimage.label, sum, center_of_mass, find_objects, binary_fill_holes).
 *
 * dcp_label_2d: dst[y, x] = the number of the connected component of src's nonzero pixels that holds (y, x), 0 where src is zero.
 * Components are numbered 1..n in the raster order of their first pixels, as scipy.ndimage.label numbers them; `connectivity` 4 is
 * scipy's default structure (the 3 x 3 cross), 8 the full 3 x 3 block.  A float is nonzero by its bits: NaN and denormals are, -0.0
 * is not.
 *   src   rows `src_row_stride` elements apart (>= width), unit column stride, any DCP_DTYPE_*
 *   dst   dense (height, width) int32, not overlapping src;  *num_labels_out (a HOST int) receives n
 *   mem_kind  DCP_MEM_HOST (staged up and down by the library) or DCP_MEM_DEVICE (enqueued on `stream`)
 * THE CALL SYNCHRONISES `stream` BEFORE IT RETURNS, for device memory too: *num_labels_out is valid on return.
 * Kernels (label_kernels.hip; dcp_debug_last_kernel() lists them): a 128 x 32 tile per workgroup labelled in LDS, the pixel pairs across
 * tile edges united by atomic min on a parent plane, every pixel's root, the roots' ranks by a three-launch prefix sum, the relabel.  No
 * kernel waits on another workgroup.  Scratch: 4 bytes per pixel and a count per 4096 pixels (dcp_release_scratch frees them).
 *
 * dcp_label_measures_2d: for every label j = 1..num_labels of `labels` (int32, rows `labels_row_stride` apart; other values are ignored)
 *   sums[j - 1]  = { pixel count, sum v, sum y v, sum x v } over the label's pixels, int64, exact in any order of arrival
 *   boxes[j - 1] = { min y, max y, min x, max x }, int32; { height, -1, width, -1 } for a label without pixels
 * with v the element of `weights` at the pixel (DCP_DTYPE_BOOL, UINT8, INT8, UINT16 or INT16, rows `weights_row_stride` apart), or 1
 * everywhere where weights is NULL (dtype is then only range-checked).  All four arrays are of one mem_kind.
 *
 * dcp_fill_holes_2d: dst[y, x] = 1 where src is nonzero or (y, x) lies in a component of src's ZERO pixels (4-neighbour structure) that
 * touches no image border, else 0: scipy.ndimage.binary_fill_holes.  dst is dense (height, width) bytes.  Scratch: 8 bytes per pixel.
 *
 * All three: a null pointer, a height or width below 1, a stride below the width, an unknown dtype or mem_kind, a connectivity other
 * than 4 or 8, a negative num_labels and src overlapping dst are DCP_ERR_INVALID_ARG; height * width above 2^31 - 1 (labels and pixel
 * indices are int32), weights of another type and height * width * max(height, width) * 65536 >= 2^63 (an int64 sum could overflow)
 * are DCP_ERR_UNSUPPORTED; all before any device call. */
int dcp_label_2d(const void* src, int32_t* dst, int height, int width, long src_row_stride, int dtype, int connectivity,
                 int* num_labels_out, int mem_kind, int device, void* stream);
int dcp_label_measures_2d(const void* weights, const int32_t* labels, int height, int width, long weights_row_stride,
                          long labels_row_stride, int dtype, int num_labels, int64_t* sums, int32_t* boxes, int mem_kind, int device,
                          void* stream);
int dcp_fill_holes_2d(const void* src, uint8_t* dst, int height, int width, long src_row_stride, int dtype, int mem_kind, int device,
                      void* stream);

/* ---- binarization of a dot image: absolute value, range, histogram, threshold, border components, 3 x 3-cross morphology ----
 * discorpy/prep/preprocessing.py:216-248 (binarization) and what it calls: np.abs, skimage.filters.threshold_otsu (np.histogram /
 * np.bincount), `mat > thres`, skimage.segmentation.clear_border, skimage.morphology.opening(mat, disk(1)).  Every entry takes src rows
 * `src_row_stride` elements apart (>= width, unit column stride), a dense dst that does not overlap src, and the mem_kind / device /
 * stream triple of dcp_label_2d (DCP_MEM_HOST: staged up and down by the library; DCP_MEM_DEVICE: enqueued on `stream`).
 *
 * dcp_abs_2d: dst = np.abs(src), same dtype, any DCP_DTYPE_*.  Floats lose their sign bit (a NaN's too), signed integers wrap at their
 * minimum as NumPy's do, unsigned integers and bool are copied.
 *
 * dcp_minmax_2d: minmax_out[0] / [1] = src.min() / src.max() as NumPy returns them (NaN where any element is NaN), *nonfinite_out = the
 * number of elements that are NaN or infinite.  DCP_DTYPE_FLOAT32 / FLOAT64 and the 8- / 16-bit integers (a double holds each value
 * exactly).  Both outputs are HOST memory and THE CALL SYNCHRONISES `stream` BEFORE IT RETURNS, for device memory too.
 *
 * dcp_histogram_2d: counts_out[nbins] (HOST int64; the call synchronises `stream`).  Float planes, the edges form: `edges` = nbins + 1
 * ascending HOST values of the plane's own type; bin i counts edges[i] <= a < edges[i + 1] and the last bin a == edges[nbins] too --
 * np.histogram(a, nbins)'s counts when the edges are its own (np.linspace(a.min(), a.max(), nbins + 1)); elements outside
 * [edges[0], edges[nbins]] and NaN are not counted; `first` is ignored.  8- / 16-bit integer planes, the bincount form: edges = NULL,
 * bin a - first, elements outside [first, first + nbins) are not counted.  1 <= nbins <= 65536.  Up to 4096 bins a workgroup counts in LDS
 * and flushes with 64-bit atomics, above that (or with the lab option "x_hist_lds" = 0) runs of equal bins add to global memory directly.
 *
 * dcp_threshold_2d: dst[y, x] = (double)src[y, x] > thres as a byte 0 / 1 (NaN compares false; 64-bit integers are rounded to double to
 * nearest-even, as NumPy's cast does), any DCP_DTYPE_*.  `count` may be NULL; otherwise the number of set pixels is ADDED to *count, an
 * int64 that lives where the planes live (device memory: the caller zeroes it on `stream`; no synchronisation).
 *
 * dcp_clear_border_2d: dst[y, x] = 1 where src is nonzero (invert = 1: where src is ZERO) and the component of such pixels that holds
 * (y, x) -- connectivity 4 or 8 as for dcp_label_2d -- has no pixel in row 0, row height - 1, column 0 or column width - 1; else 0.
 * skimage.segmentation.clear_border of a binary image (connectivity 8); invert = 1 clears the complement instead, so a contrast
 * inversion needs no pass of its own.  The union-find, scratch (8 bytes per pixel) and lab option of dcp_fill_holes_2d.
 *
 * dcp_morph_cross_2d: grey erosion (op 0), dilation (op 1) or opening (op 2: erosion then dilation) of a uint8 plane by the 3 x 3 cross;
 * what lies outside the image is ignored (minimum / maximum over the in-image neighbours only), which is both skimage's border rule and
 * scipy.ndimage.grey_erosion / grey_dilation / grey_opening(footprint=cross, mode="reflect").  The opening is one launch (a 128 x 32
 * tile with a halo of 2 in LDS); the lab option "x_morph_fused" = 0 makes it two, through a plane of scratch.
 *
 * All six: a null pointer, a height or width below 1, a stride below the width, an unknown dtype or mem_kind, src overlapping dst,
 * nbins below 1, edges missing for a float plane or given for an integer one, a connectivity other than 4 or 8, an invert other than 0
 * or 1 and an op outside 0..2 are DCP_ERR_INVALID_ARG; height * width above 2^31 - 1, a dtype the entry does not take and nbins above
 * 65536 are DCP_ERR_UNSUPPORTED; all before any device call. */
int dcp_abs_2d(const void* src, void* dst, int height, int width, long src_row_stride, int dtype, int mem_kind, int device, void* stream);
int dcp_minmax_2d(const void* src, int height, int width, long src_row_stride, int dtype, double* minmax_out, int64_t* nonfinite_out,
                  int mem_kind, int device, void* stream);
int dcp_histogram_2d(const void* src, int height, int width, long src_row_stride, int dtype, const void* edges, int nbins, int64_t first,
                     int64_t* counts_out, int mem_kind, int device, void* stream);
int dcp_threshold_2d(const void* src, uint8_t* dst, int height, int width, long src_row_stride, int dtype, double thres, int64_t* count,
                     int mem_kind, int device, void* stream);
int dcp_clear_border_2d(const void* src, uint8_t* dst, int height, int width, long src_row_stride, int dtype, int connectivity, int invert,
                        int mem_kind, int device, void* stream);
int dcp_morph_cross_2d(const uint8_t* src, uint8_t* dst, int height, int width, long src_row_stride, int op, int mem_kind, int device,
                       void* stream);

/* ---- the image-sized steps of calculate_threshold: the sort of every pixel and the cubic zoom of the sorted list ----
 * discorpy/prep/preprocessing.py:816-853: np.sort(mat.flatten()), scipy.ndimage.zoom(sorted, size / len, mode="nearest").  Both take
 * the mem_kind / device / stream triple of dcp_label_2d, DCP_DTYPE_FLOAT32 / FLOAT64 and the 8- to 64-bit integers, and a dst that does
 * not overlap src; neither synchronises a device call.
 *
 * dcp_sort_plane_2d: dst (dense, height * width elements of the source's type, living where the plane lives) = the plane's elements
 * (rows `src_row_stride` elements apart) in ascending order: np.sort(a, axis=None).  Floats order by value with NaNs of either sign
 * last.  What NumPy leaves open is fixed here: -0.0 comes before +0.0, NaNs come in the order of their payloads, and a negative NaN comes
 * out as the positive NaN of the same payload (it loses its sign bit on the way in).  A least-significant-digit radix sort on the eight
 * bits of a digit over order-preserving integer keys; a pass whose digit is the same in every element is skipped (lab option
 * "x_sort_skip" = 0: never), so uint8 values stored as float32 cost what their entropy costs.  Work memory: two key buffers (4 bytes per
 * element up to 32 bits, else 8) and about 2 MiB of tables, leased from the spline workspace; more than its 2 GiB is DCP_ERR_UNSUPPORTED.
 *
 * dcp_zoom_cubic_nearest_1d: dst[0 .. out_n) = scipy.ndimage.zoom(src, out_n / n, order=3, mode="nearest") of the 1-D array of n
 * elements at src; the caller gives the output length scipy would compute (round(n * zoom)).  scipy 1.15's definition: the line
 * extended by 12 edge samples per side, times the gain, the causal and anticausal recursions of the pole sqrt(3) - 2 with the reflect
 * boundary's initial values, sampled at j (n - 1) / (out_n - 1) + 12 with scipy's weights in scipy's order, stored as scipy stores a
 * double into the element type.  Every output point filters a window of 64 samples on either side of its four taps instead of the line:
 * the start-up error is below 2^-121 of the window's largest magnitude.
 *
 * Both: a null pointer, a height, width, n or out_n below 1, a stride below the width, an unknown dtype or mem_kind and src overlapping
 * dst are DCP_ERR_INVALID_ARG; more than 2^31 - 1 elements, DCP_DTYPE_BOOL and a sort beyond the workspace are DCP_ERR_UNSUPPORTED; all
 * before any device call. */
int dcp_sort_plane_2d(const void* src, void* dst, int height, int width, long src_row_stride, int dtype, int mem_kind, int device, void* stream);
int dcp_zoom_cubic_nearest_1d(const void* src, int64_t n, void* dst, int64_t out_n, int dtype, int mem_kind, int device, void* stream);

/* ---- the per-profile steps of the line-pattern route on batches of profiles (discorpy/prep/linepattern.py:46-274, 512-567) ----
 * The first two take `nrows` profiles of `length` samples as the rows of a DCP_DTYPE_FLOAT32 / FLOAT64 plane (rows `src_row_stride`
 * elements apart) and the mem_kind / device / stream triple of dcp_label_2d.
 *
 * dcp_local_extrema_rows: the minima search of get_local_extrema_points (after its denoise / option / norm steps).  Sample i of
 * range(radius, length - radius - 1) is a point iff it equals the minimum of its window [i - radius, i + radius], the window holds no
 * NaN, and |(v - m) / m| > sensitive, m = np.mean(np.sort(window)[-radius:]) bit for bit (NumPy's pairwise sum in ascending order, then
 * one division; the quotient counts as 0 where m == 0); all in the profiles' own type, the last comparison in double (`sensitive`
 * rounded to float32 by the caller gives NumPy's float32 comparison).  dst: (nrows, length) doubles; row r holds its positions in
 * ascending order and their number in element length - 1 (there are at most length - 1).  subpixel = 1: each position i becomes
 * i - 1 + (-b / (2 a)) with a = (d0 - 2 d1 + d2) / 2, b = (-3 d0 + 4 d1 - d2) / 2 over d = profile[i - 1 .. i + 1] in double, where a != 0
 * and the vertex lies in [0, 3), else i - 1 + argmin(d) -- the closed form of the reference's np.polyfit; needs radius >= 1.
 * 0 <= radius <= 128 (above: DCP_ERR_UNSUPPORTED).
 *
 * dcp_window_slope_rows: sliding_window_slope before its division by the mean: dst ((nrows, length), the profiles' type) = the absolute
 * slope of the least-squares line through the `size` samples (odd, >= 3) around every sample of the edge-padded row,
 * sum_k (k - r) p[i + k - r] / sum_k (k - r)^2 with products and sum in double (k ascending), rounded to the type.  nrows <= 65535.
 *
 * dcp_tilted_profiles_2d: `nprofiles` calls of get_tilted_profile on one height x width plane (FLOAT32 / FLOAT64) in one.  Profile p is
 * scipy.ndimage.map_coordinates(band_p, ..., order=3, mode="nearest") of its own band -- rows (direction 0) or columns (direction 1)
 * band_lo[p] .. band_lo[p] + band_count[p] - 1 of the plane -- at the `length` IMAGE coordinates (ycoords, xcoords)[p][i]: doubles that
 * live where the plane lives, (nprofiles, length) each.  band_lo / band_count are host arrays.  dst: (nprofiles, length) of the plane's
 * type.  The coefficient planes of the bands come from the library's workspace; above 512 MiB the profiles run in groups.  For
 * DCP_MEM_DEVICE the call synchronises `stream` once per group (the band table is copied from host memory). */
int dcp_local_extrema_rows(const void* src, double* dst, int nrows, int length, long src_row_stride, int dtype, int radius, double sensitive,
                           int subpixel, int mem_kind, int device, void* stream);
int dcp_window_slope_rows(const void* src, void* dst, int nrows, int length, long src_row_stride, int dtype, int size, int mem_kind, int device,
                          void* stream);
int dcp_tilted_profiles_2d(const void* src, void* dst, int height, int width, long src_row_stride, int dtype, int direction, int nprofiles,
                           int length, const double* ycoords, const double* xcoords, const int32_t* band_lo, const int32_t* band_count,
                           int mem_kind, int device, void* stream);

/* ---- the selection of good peaks behind the peak search (discorpy/prep/linepattern.py:75-152) ----
 * dcp_select_peaks_rows: select_good_peaks (after its smoothing step) on `npeaks` candidate peaks of a plane of profiles as
 * dcp_local_extrema_rows takes it (`nrows` rows of `length` samples, DCP_DTYPE_FLOAT32 / FLOAT64, rows `src_row_stride` elements
 * apart, the mem_kind / device / stream triple of dcp_label_2d).  Candidate k is sample peak_index[k] of row peak_row[k]: two HOST
 * int32 arrays.  One wave per candidate, everything in double:
 *   window   w = row[start .. stop), start = max(0, p - radius), stop = min(length, p + radius + 1), n = stop - start;
 *   no fit   for n <= 3 (status 1), a NaN or an infinity in the window (status 2) and max(w) == min(w) (status 3; the reference tests
 *            np.std(w) != 0.0, which on a constant window hangs on the rounding of np.mean);
 *   y        = (w - min(w)) / std(w), the population standard deviation; x_i = i - n / 2 (integer division);
 *   fit      a exp(-((x - c) / (2 b^2))^2) + d to (x, y) from (a, b, c, d) = (1, 1, 0, 0) by the Levenberg-Marquardt iteration of MINPACK's
 *            lmdif as scipy.optimize.curve_fit runs it by default: forward-difference Jacobian (relative step 2^-26), columns scaled by
 *            the running maximum of their norms, a trust region of 100 |D x| at first, stop on the relative decrease of the cost
 *            (actual and predicted) or on the trust region against |D x|, both at 1.49012e-8, at most 1000 evaluations of the model
 *            (a Jacobian counts 4).  A fit that runs out of them (status 4), whose sums, step or parameters stop being finite (status 5)
 *            or whose residuals stand at right angles to the Jacobian's columns to 2^-52 first (status 6) has failed;
 *   num      = np.percentile(|fit - y|, 80): linear interpolation at 0.8 (n - 1) of the sorted values;
 *   keep[k]  = 1 iff status 0 and |c| < radius / 2 (integer division) and num < tol and (use_offset == 0 or |d| < tol), else 0.
 * The sums of a fit are reduced across the wave in a fixed order: a candidate's result does not depend on the others of the call.
 * keep: npeaks bytes; fit: npeaks x 6 doubles (a, b, c, d, num, status; NaN for what was not computed), or null.  Both live where the
 * plane lives.  A null pointer other than fit, nrows, length or npeaks below 1, a stride below the length, a candidate outside the
 * plane, radius below 1, a NaN tol, use_offset other than 0 or 1, an unknown dtype or mem_kind and src overlapping keep or fit are
 * DCP_ERR_INVALID_ARG; radius above 128 and other dtypes are DCP_ERR_UNSUPPORTED; all before any device call.  For DCP_MEM_DEVICE the call
 * synchronises `stream` once (the two tables are copied from host memory). */
int dcp_select_peaks_rows(const void* src, int nrows, int length, long src_row_stride, int dtype, const int32_t* peak_row, const int32_t* peak_index,
                          int npeaks, int radius, double tol, int use_offset, unsigned char* keep, double* fit, int mem_kind, int device, void* stream);

/* dcp_extrema_select_rows: get_local_extrema_points(select_peaks=True) in one call -- the search of dcp_local_extrema_rows, the selection of
 * dcp_select_peaks_rows on every candidate the search finds, and the sub-pixel step on the candidates that survive.  src, dst, nrows,
 * length, src_row_stride, dtype, radius, sensitive, subpixel: as dcp_local_extrema_rows defines them; dst row r holds the positions of the
 * SURVIVING candidates in ascending order and their number in element length - 1 (nothing else of dst is written).
 *   sel      the plane the fits read: the type and shape of src, rows `sel_row_stride` elements apart.  NULL: the reference's own
 *            np.max(list_data) - list_data, formed as (T)(max(row) - row[i]) in the rows' type T and then converted to double; max(row)
 *            is NaN where the row holds a NaN (np.max), so every window of such a row is non-finite and nothing of it is kept;
 *   fit      candidate p (an integer position of the search: radius <= p < length - radius - 1) is judged on the whole window
 *            sel[p - radius .. p + radius] with `tol` and `use_offset` exactly as dcp_select_peaks_rows judges that window, bit for bit;
 *   cand     (may be NULL) (nrows, length) doubles: every candidate before selection, as dcp_local_extrema_rows(subpixel = 0) writes them;
 *   keep     (may be NULL) (nrows, length) bytes: keep[r, j] = 0 / 1 for candidate j of row r; bytes beyond a row's count are not written;
 *   subpixel 1: the closed form of dcp_local_extrema_rows on src, for the kept candidates.
 * sel, cand and keep live where the plane lives.  1 <= radius <= 128; at radius 1 every window has 3 samples and nothing is kept.
 * DCP_MEM_DEVICE: the call never synchronises `stream` and reads no count on the host -- the candidates go through a worklist in the
 * library's workspace (8 + 4 + 1 bytes per sample of the plane); a workgroup of the fit grid draws four candidates at a time from a
 * ticket counter the call zeroes on `stream`; no result depends on the order of the draws.  DCP_MEM_HOST: one upload (two with sel), one
 * download.  A null src or dst, nrows or length below 1, a stride below the length, radius below 1, subpixel or use_offset other
 * than 0 or 1, a NaN sensitive or tol, an unknown dtype or mem_kind, and src or sel overlapping an output or two outputs overlapping
 * are DCP_ERR_INVALID_ARG; radius above 128 and other dtypes are DCP_ERR_UNSUPPORTED; all before any device call. */
int dcp_extrema_select_rows(const void* src, double* dst, int nrows, int length, long src_row_stride, int dtype, int radius, double sensitive,
                            int subpixel, const void* sel, long sel_row_stride, double tol, int use_offset, double* cand, unsigned char* keep,
                            int mem_kind, int device, void* stream);

/* ---- the Radon transform behind the slope search of the line-pattern route (discorpy/prep/linepattern.py:302-449) ----
 * dcp_radon_2d: the sinogram of a side x side plane (DCP_DTYPE_FLOAT32 / FLOAT64, rows `src_row_stride` elements apart, read in place)
 * for `nangles` angles in one launch; dst: (side, nangles) doubles, row-major.  With c0 = side / 2 (integer division):
 *   g(y, x)  = (double)src[y, x], and 0.0 where y or x lies outside [0, side) or (y - c0)^2 + (x - c0)^2 > c0^2 (an assignment: a NaN there does not reach dst);
 *   for angle i, table[4 i .. 4 i + 3] = {ca, sa, tx, ty} (HOST doubles; for an angle a: cos a, sin a, -c0 (ca + sa - 1),
 *   -c0 (ca - sa - 1)), the sample (r, c) reads x = ca c + sa r + tx, y = -sa c + ca r + ty (left to right, no fused multiply-add),
 *   x0 = floor x, x1 = ceil x, y0 = floor y, y1 = ceil y, dx = x - x0, dy = y - y0,
 *   v = (1 - dy) ((1 - dx) g(y0, x0) + dx g(y0, x1)) + dy ((1 - dx) g(y1, x0) + dx g(y1, x1));
 *   dst[c, i] = v(0, c) + v(1, c) + ... + v(side - 1, c), added in that order.
 * All float64 for both element types: equal bit for bit to that sequence of IEEE operations evaluated anywhere.  This restates
 * skimage.transform.radon(image, theta, circle=True) from its documentation (agreement with scikit-image itself: UNVERIFIED).
 * The mem_kind / device / stream triple of dcp_label_2d; for DCP_MEM_DEVICE the call synchronises `stream` once (the table is copied
 * from host memory).  A null pointer, side or nangles below 1, a stride below the side, an unknown dtype or mem_kind, src overlapping
 * dst and a table entry that is not finite are DCP_ERR_INVALID_ARG; another dtype, side above 32768 and nangles above 65535 (so that
 * every index fits 32 bits) are DCP_ERR_UNSUPPORTED; all before any device call. */
int dcp_radon_2d(const void* src, double* dst, int side, long src_row_stride, int dtype, int nangles, const double* table, int mem_kind,
                 int device, void* stream);

/* ---- the dot-grid route (discorpy/prep/preprocessing.py:274-558: calc_size_distance, select_dots_based_ratio, calc_hor_slope,
 * calc_ver_slope) ----
 * dcp_radon_padded_2d: the sinogram of a height x width plane (FLOAT32 / FLOAT64, rows `src_row_stride` elements apart, read in place)
 * embedded in a square of zeros: S = (int)ceil(sqrt(2.0) * max(height, width)) in double, the plane's first element at
 * (S / 2 - height / 2, S / 2 - width / 2) (integer divisions).  That square is transformed as dcp_radon_2d transforms a plane of side S
 * -- the same table {ca, sa, tx, ty} per angle MADE FOR SIDE S, the same samples, weights and ascending row sum -- but WITHOUT the
 * circle: g(y, x) is 0.0 exactly where (y, x) lies outside the plane's rectangle and the element, a NaN included, everywhere inside.
 * No padded plane is made and nothing outside the height x width view is read.  dst: (S, nangles) doubles, row-major.  This restates
 * skimage.transform.radon(image, theta, circle=False) from its documentation (agreement with scikit-image itself: UNVERIFIED).
 * Refusals as for dcp_radon_2d, with S (at most 32768, so max(height, width) <= 23170) in the place of its side.
 *
 * dcp_nearest_sq_dists: for `npoints` points (y, x) -- dense (npoints, 2) doubles -- dst[i][0..3] = the four smallest of
 *   (y_i - y_j) * (y_i - y_j) + (x_i - x_j) * (x_i - x_j)     (two differences, two products, one sum, each rounded; no fused multiply-add)
 * over ALL j, j = i included, in ascending order; +inf where npoints < 4.  dst: dense (npoints, 4) doubles where the points live.  SQUARED
 * distances: the caller takes the root.  One launch.  1 <= npoints <= 2^20.  Coordinates must be finite: host memory is checked
 * (DCP_ERR_INVALID_ARG), device memory is the caller's word.
 *
 * dcp_box_moments_2d: per box b of `boxes` (HOST array of nboxes x {min y, max y, min x, max x}, inclusive, as dcp_label_measures_2d writes
 * them), sums[b][0..5] = count, sum y, sum x, sum y y, sum x y, sum x x over EVERY nonzero element of the plane inside the box -- whatever
 * label it carries -- each weighing 1, with (y, x) relative to the box's corner.  The plane: BOOL or an 8- / 16-bit integer type, sides at
 * most 32768 (every sum then stays below 2^60).  An empty box (max < min) gives zeros; a box that is not empty and reaches outside the
 * plane is DCP_ERR_INVALID_ARG.  sums: dense (nboxes, 6) int64 where the plane lives.  nboxes = 0 returns at once.  For DCP_MEM_DEVICE
 * the call synchronises `stream` once (the boxes are copied from host memory).
 * All three: the mem_kind / device / stream triple of dcp_label_2d; null pointers, sizes below 1, a stride below the width, an unknown
 * dtype or mem_kind and an output that overlaps the source are DCP_ERR_INVALID_ARG; all before any device call. */
int dcp_radon_padded_2d(const void* src, double* dst, int height, int width, long src_row_stride, int dtype, int nangles, const double* table,
                        int mem_kind, int device, void* stream);
int dcp_nearest_sq_dists(const double* points, double* dst, int npoints, int mem_kind, int device, void* stream);
int dcp_box_moments_2d(const void* src, int height, int width, long src_row_stride, int dtype, const int32_t* boxes, int nboxes, int64_t* sums,
                       int mem_kind, int device, void* stream);

/* discorpy/post/postprocessing.py:36-64 (unwarp_line_forward) and discorpy/util/utility.py:192-230
 * (find_point_to_point): the radial model applied to npts points given as (y, x) pairs of doubles,
 * out = centre + B(r) * (p - centre) with B(r) = sum_i list_fact[i] * r^i.  Float64; agrees with the
 * reference's numpy/libm evaluation to a few units in the last place. */
int dcp_map_points_f64(const double* yx_in, double* yx_out, int64_t npts, double xcenter, double ycenter,
                       const double* list_fact, int nfact, int mem_kind, int device, void* stream);

/* discorpy/post/postprocessing.py:72-108 (unwarp_line_backward): the INVERSE of the mapping above for npts points given as (y, x)
 * pairs of doubles -- out = centre + (ru / rd) * (p - centre), where rd = |p - centre| and ru solves ru * B(ru) = rd with
 * B(r) = sum_i list_fact[i] * r^i (Newton from ru = rd, bisection once a sign change is bracketed, a fixed iteration budget; the
 * centre maps to itself).  The reference minimises the squared difference with scipy.optimize.minimize and leaves ~1e-6 px of the
 * equation unsolved; this is the root to rounding.  A point for which no root >= 0 is found (the model folds there, or has no
 * solution) is written as NaN and counted: *n_unsolved (optional) receives the count and lives where the points live -- host memory
 * for DCP_MEM_HOST, device memory (written on `stream`) for DCP_MEM_DEVICE. */
int dcp_map_points_inverse_f64(const double* yx_in, double* yx_out, int64_t npts, double xcenter, double ycenter,
                               const double* list_fact, int nfact, int64_t* n_unsolved, int mem_kind, int device, void* stream);

/* discorpy/post/postprocessing.py:414-441 (correct_perspective_line): the homography applied to npts points given as (y, x) pairs of
 * doubles -- xn = (c1 x + c2 y + c3) / (c7 x + c8 y + 1), yn = (c4 x + c5 y + c6) / (c7 x + c8 y + 1) in numpy's operation order with
 * IEEE divisions: bit-equal to the reference. */
int dcp_map_points_perspective_f64(const double* yx_in, double* yx_out, int64_t npts, const double* list_coef, int mem_kind, int device,
                                   void* stream);

/* Diagnostics of the LDS-staged gather on the current device: out[0] = wave tiles whose source
 * box did not fit the LDS slab, out[1] = wave tiles whose containment vote failed (both fall back
 * to the direct gather).  Synchronises the device. */
int dcp_debug_counters(uint64_t* out, int n, int reset);

/* The bounds-checking debug build (make -C discorpy_amd/csrc bounds -> lib/libdiscorpy_hip_bounds.so, loaded through DCP_LIB_PATH;
 * SURVEY.md section 5): every tap the staged kernels read from LDS is checked against its slab.  out[0] = taps outside their
 * slab since the last reset (must be 0: the tile certificate says so), out[1..3] = byte offset, slab size and site number of the
 * first one, out[4] = 1 if this library IS the checking build (0: the product build, which compiles no check and reports zeros).
 * n >= 5.  Synchronises the device. */
int dcp_debug_bounds(uint64_t* out, int n, int reset);

/* Name of the float32 image / stack kernel the calling thread launched last, e.g.
 * "remap_wg_kernel<Radial,NF=5,f64lerp>" (empty before the first launch).  For tests and benchmarks that must say
 * -- and assert -- which kernel a call took; the reference has no counterpart. */
const char* dcp_debug_last_kernel(void);

/* The host's tile-deviation certificate for a calibration on a height x width frame (needs no GPU): 0 = none (the staged
 * kernels verify every pixel), 1 = holds for 64 x 16 wave tiles, 2 = also for 128 x 32 workgroup tiles (remap_wg_kernel,
 * stack_wg_kernel, remap_wg_batch_kernel).  map_kind DCP_MAP_RADIAL (list_fact), DCP_MAP_PERSPECTIVE (list_coef) or DCP_MAP_FUSED (both:
 * 0 or 2).
 * Negative: a DCP_ERR_* code.  For tests and for callers that want to know which kernel their calibration will take. */
int dcp_debug_tile_certificate(int map_kind, int64_t height, int64_t width, double xcenter, double ycenter, const double* list_fact,
                               int nfact, const double* list_coef);

/* ---- device memory / stream / event helpers (so a host language needs no other GPU runtime) ---- */
int dcp_malloc(void** ptr, size_t bytes, int device);
int dcp_free(void* ptr, int device);
#define DCP_COPY_H2D 0
#define DCP_COPY_D2H 1
#define DCP_COPY_D2D 2
int dcp_memcpy(void* dst, const void* src, size_t bytes, int kind, int device, void* stream);
/* Host memory the GPU can address (hipHostRegister): a DCP_MEM_HOST frame call whose `dst` lies in registered memory -- these, or
 * anything from hipHostMalloc -- has its result written straight into it by the kernels, band by band while the source is still
 * uploading (no device copy of the result, no download; option "host_direct" = 0 switches that off).  Registration costs ~0.8 ms
 * per 64 MiB: for buffers that are reused.  Unregister before the memory is freed.  Register WHOLE PAGES that nothing else lives in
 * (an mmap'ed or page-aligned allocation): a malloc'ed block shares its edge pages with other heap objects, and a pageable copy of
 * one of those is pinned and unpinned by the runtime under the registration (GPU memory access faults, round 4). */
int dcp_host_register(void* ptr, size_t bytes, int device);
int dcp_host_unregister(void* ptr);
int dcp_stream_create(void** stream, int device);   /* a non-blocking stream for DCP_MEM_DEVICE calls */
int dcp_stream_destroy(void* stream);
int dcp_stream_synchronize(int device, void* stream);
int dcp_event_create(void** event, int device);
int dcp_event_record(void* event, void* stream);
/* work enqueued on `stream` after this call starts only when `event` (recorded on any stream of the device) has completed --
 * hipStreamWaitEvent: how a caller who spreads independent frames over two streams (two frames in flight: the drain of one under the
 * ramp of the other, profiles/r06a_dispatch_modes.txt) forks from and joins back into one stream without a host synchronisation */
int dcp_stream_wait_event(void* stream, void* event);
int dcp_event_synchronize(void* event);
int dcp_event_elapsed_ms(void* start, void* stop, float* ms);
int dcp_event_destroy(void* event);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* DISCORPY_HIP_H */
