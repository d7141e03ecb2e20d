// dcp_internal.h -- shared between the HIP kernels (unwarp_kernels.hip, stack_kernels.hip, ...) and the
// C-ABI layer (api_*.cpp).  Not installed; the public surface is
// include/discorpy_hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dcp {

constexpr int kMaxFact = 32;       // longest radial coefficient vector accepted
constexpr int kInlineFact = 10;    // lengths 1..kInlineFact get a fully unrolled, SGPR-resident polynomial
constexpr int kMaxTileRows = 64;   // rows one workgroup walks (runtime option tile_rows <= this)

// sampler selector: order 0, or order 1 with one of the three blend arithmetics
enum Sampler : int { kNearest = 0, kScipy = 1, kF64Lerp = 2, kF32Lerp = 3 };

// what maps an output pixel to a source coordinate (kCoords: explicit coordinates, one output value per point)
// (DCP_MAP_RADIAL / _PERSPECTIVE / _FUSED of include/discorpy_hip.h are the first three)
enum MapKind : int { kRadial = 0, kPersp = 1, kFused = 2, kCoords = 3 };

struct ImageArgs {
  const float* src;
  float* dst;
  int32_t H, W;            // output == source shape
  int32_t src_stride;      // elements between source rows
  int32_t src_col_stride;  // elements between source columns (1 on the fast path)
  uint32_t src_bytes;      // extent of the source for the buffer descriptor
  int32_t tiles_x, tiles_y;
  int32_t tile_rows;       // rows per workgroup
  int32_t xcd_remap;       // 1: contiguous band of tiles per XCD
  int32_t pipe_depth;      // rows of gathers in flight per thread (1, 2 or 4)
  int32_t lds_gather;      // 1: stage the source box of each wave tile in LDS (remap_lds_kernel)
  int32_t wg_box;          // 1: one box per workgroup (remap_wg_kernel) when the certificate allows it
  int32_t wg_per_cu;       // remap_wg_kernel: workgroups resident per CU (0 = as many as fit: 6)
  int32_t y_origin;        // a launch may cover only output rows [y_origin, y_origin + rows_out) of the H x W map;
  int32_t rows_out;        // dst then points at row y_origin (0 / 0 = the whole image)
  int32_t int_exact;       // integer element types: 1 = tiles at coordinates >= 32 take the exact factorised blend (exact_lerp_pairs)
  const int32_t* boxes = nullptr;   // remap_wg_kernel: corner hulls (x0, x1, y0, y1) of every 128 x 32 tile, frame-major, from box_table_kernel
                                    // (nullptr: every wave evaluates its workgroup's corners itself)
                                    // remap_wg_kernel<.., PLAN>: a frame plan (frame_plan.cpp) -- the hulls of the tiles_x * tiles_y tiles, then one
                                    // word per tile, bit w set = wave tile w of the tile may take its coordinate rows from radial_rows_interp
};

struct MapArgs {
  double xc, yc;
  double fact[kMaxFact];
  double coef[8];          // perspective c1..c8
  int32_t nfact;
  int32_t fast_div;        // 1: operands of the homography division stay in the normal range over the image
  int32_t tall_ok;         // host certificate for 64 x 32 tiles under an 80 x 56 box (sheared maps: remap_wg_color_kernel's second tile
                           // shape): the deviation bound holds for that tile and (nearly) every such tile's box fits
  int32_t tile_dev_ok;     // host certificate -- inside any output tile every source coordinate stays within 0.95 px of
                           // the bilinear interpolant of the tile's corner coordinates: 1 for 64 x 16 tiles, 2 also
                           // for 128 x 32 tiles (radial and perspective maps; api_core.cpp tile_deviation_certified)
};

struct StackArgs {
  const float* vol;
  float* out;
  int64_t proj_stride;     // elements between projections
  int32_t D, H, W;
  int32_t row_stride;      // elements between rows of a projection
  double row_start;
  int32_t nrows;
  int32_t d_chunk;         // projections walked by one thread
  uint32_t proj_bytes;
  int32_t rb0, rbh;        // the reference's row band [rb0, rb0 + rbh) of unwarp_chunk_slices_backward (postprocessing.py:289-312):
                           // a row coordinate outside it is reflected inside it, as scipy does with the cropped band.  rbh = 0:
                           // the host has shown that no coordinate can leave the band (or the call is not a chunk): no check
  int32_t int_exact;       // as ImageArgs::int_exact (stack_wg_kernel on integer element types)
  int32_t store_wait = 0;  // stack_wg_kernel: LaunchOpts::store_wait
  int32_t wg_per_cu = 0;   // stack_wg_kernel: LaunchOpts::wg_per_cu (1..3: workgroups per CU capped through unused dynamic LDS; A/B)
  int32_t xcd_order = 0;   // stack_wg_kernel: tiles dealt to the XCDs in contiguous runs (LaunchOpts::xcd_remap != 0)
};

struct CoordArgs {
  const void* ycoord;
  const void* xcoord;
  int64_t npts;
  int32_t is_f64;
  int32_t mode;            // BoundaryMode applied to coordinates OUTSIDE the image at orders 0 / 1 (kModeNearest = clamp)
};

// scipy boundary modes in the order of the reference's docstrings (postprocessing.py:128-130)
enum BoundaryMode : int { kModeReflect = 0, kModeGridMirror, kModeConstant, kModeGridConstant, kModeNearest, kModeMirror,
                          kModeGridWrap, kModeWrap };
enum SplineFilterKind : int { kSplMirror = 0, kSplReflect = 1, kSplWrap = 2 };

// element types of the *_typed entry points (DCP_DTYPE_* of include/discorpy_hip.h)
enum ElemType : int { kF32 = 0, kF64, kU8, kI8, kU16, kI16, kU32, kI32, kI64, kU64, kBool, kNumElemTypes };
__host__ __device__ inline int elem_size(int dtype) {
  return (dtype == kF64 || dtype == kI64 || dtype == kU64) ? 8 : (dtype == kF32 || dtype == kU32 || dtype == kI32) ? 4 : (dtype == kU16 || dtype == kI16) ? 2 : 1;
}
// numpy's bool_: one byte holding 0 or 1, read as a double and stored by a C cast of the double (scipy CASE_INTERP_OUT(NPY_BOOL))
struct Bool8 {
  uint8_t v;
  __host__ __device__ operator double() const { return (double)v; }
};

// orders 0 / 1 on any element type (typed_kernels.hip); strides in elements
struct TypedImageArgs {
  const void* src;
  void* dst;
  int64_t src_stride, src_cstride;
  int32_t H, W;
  int32_t order;           // 0 or 1
  int32_t dtype;
  int32_t blend;           // interleaved-channel kernel, float32: kF64Lerp = the one-ulp factorisation (else scipy's exact order)
  int32_t y0, rows;        // interleaved-channel kernel only: output rows [y0, y0 + rows), dst = first row of that band
};

struct TypedStackArgs {
  const void* vol;
  void* out;
  int64_t proj_stride, row_stride;
  int32_t D, H, W;
  int32_t nrows, d_chunk;
  int32_t dtype;
  int32_t out_f32;         // 1: out is float32 holding the value already converted to `dtype` (unwarp_slice_backward)
  int32_t round_f32;       // 1: coordinates rounded to float32 (unwarp_chunk_slices_backward)
  int32_t rb0, rbh;        // as in StackArgs
  double row_start;
};

struct SplineArgs {
  const void* src;
  int32_t src_dtype, dst_dtype;
  double* coef;            // (Hp x Wp) float64 workspace: padded image -> B-spline coefficients
  double* scratch;         // second plane of the same size (out-of-place filter passes, transposes)
  int32_t H, W, src_stride, src_cstride;
  int32_t Hp, Wp, pad;     // pad = 12 for 'nearest' / 'grid-constant', else 0
  int32_t order, mode, filter_kind, npoles;
  double poles[2];
  double zpow[2][2];       // [axis][pole]: z^n (reflect) or z^(n-1) (mirror), evaluated on the host
  int32_t exact_sum;       // 1: the taps are accumulated in scipy's order, t += (c wy) wx; 0: factorised and fused (the LDS-staged gather only)
  int32_t xcd_remap;       // spline_wg_kernel: 1 = every XCD owns a run of neighbouring tile columns (set by launch_spline; option "spline_xcd")
};

struct LaunchOpts {
  int tile_rows = 16;
  int xcd_remap = 2;
  int pipe_depth = 2;
  int lds_gather = 1;
  int coef_lds = 0;        // 1: force the LDS-staged coefficient path even for short vectors
  int d_chunk = 16;
  int stack_lds = 1;       // LDS-staged stack kernel: 0 never, 1 when the launch has enough wave tiles, 2 always
  int wg_box = 1;          // 1: remap_wg_kernel (one source box per 128 x 32 workgroup tile) for certified maps
  int wg_per_cu = 0;       // remap_wg_kernel: cap on resident workgroups per CU (0 = none)
  int store_wait = 1;      // stack_wg_kernel: 1 waits for the fill only (the stores of the previous projection stay in flight), 0 for everything
  int tall_tiles = 0;      // (A/B option, off: slower on config 5) sheared radial maps (level-1 certificate, MapArgs::tall_ok): 64 x 32 workgroup tiles (remap_wg_color_kernel) instead of per-wave boxes
  int int_exact = 1;       // integer element types: the exact factorised blend where it is provably exact (0: scipy's operation order everywhere)
  int stack_wg = 1;        // stack_wg_kernel (one box per workgroup, two slabs) for chunks of rows under a certified map: 0 never,
                           // 1 when the launch has enough workgroups (float32 and 8- / 16-bit integers), 2 whenever eligible
  int any_order = 0;       // 1: whole-frame launches leave with the AQL barrier bit cleared (hipExtAnyOrderLaunch): the packet may start
                           // while earlier packets of its stream still run (DCP_MEM_DEVICE_UNORDERED; the caller vouches for independence)
};

// launchers: frames (unwarp_kernels.hip) and stacks (stack_kernels.hip: launch_stack*, stack_wg_would_take)
hipError_t launch_image(MapKind kind, const ImageArgs& img, const MapArgs& map, int sampler,
                        bool round_f32, const LaunchOpts& opts, hipStream_t stream);
// one frame of launch_image_batch (host side): its own source, destination, centre and coefficient vector
struct BatchFrame {
  const float* src;
  float* dst;
  double xc, yc;
  const double* fact;
};
// n dense float32 frames of ONE shape (img: H, W, src_stride, src_bytes; src / dst ignored), radial map, float32 coordinates, every
// frame with its own calibration of `nfact` <= 10 coefficients, through remap_wg_batch_kernel (blockIdx.z = frame) in
// ceil(n / 55) launches (35 per launch above 5 coefficients).  The caller has certified every frame at level 2
// (tile_deviation_certified).  *taken = false: the shape / options do not qualify, launch the frames one by one
hipError_t launch_image_batch(const ImageArgs& img, const BatchFrame* frames, int n, int nfact, int sampler, const LaunchOpts& opts,
                              hipStream_t stream, bool* taken);
// 8- and 16-bit integer images on remap_wg_kernel (img.src / dst reinterpreted, src_stride in elements, src_bytes the extent
// in bytes); *taken = false: the call does not qualify, use launch_typed_image
hipError_t launch_wg_typed(MapKind kind, const ImageArgs& img, const MapArgs& map, int order, int dtype, const LaunchOpts& opts,
                           hipStream_t stream, bool* taken);
hipError_t launch_stack_wg_typed(const StackArgs& st, const MapArgs& map, int dtype, const LaunchOpts& opts, hipStream_t stream, bool* taken);
// whole frames of one calibration under a homography / the fused map on stack_wg_kernel (float32, uint8, uint16; order 1; level-2
// certificate of the map's kind); st as for launch_stack_wg_typed with row_start = 0, nrows = H; *taken = false: frame by frame
hipError_t launch_stack_wg_frames(MapKind kind, const StackArgs& st, const MapArgs& map, int dtype, int sampler, const LaunchOpts& opts,
                                  hipStream_t stream, bool* taken);
hipError_t launch_coords(const ImageArgs& img, const CoordArgs& ca, int sampler, hipStream_t stream);
hipError_t launch_coord_map(MapKind kind, const ImageArgs& img, const MapArgs& map, float* ymap, float* xmap,
                            hipStream_t stream);
bool stack_wg_would_take(const StackArgs& st, const MapArgs& map, const LaunchOpts& opts);
hipError_t launch_stack(const StackArgs& st, const MapArgs& map, int sampler, bool round_f32,
                        const LaunchOpts& opts, hipStream_t stream);

// the rows of `st` under `ncentres` calibrations that differ in the centre only (map.xc / map.yc ignored), one launch per 224
// centres; st.out = (ncentres, D, nrows, W).  st.rbh must be 0 (no band check: the caller sends folding models call by call)
hipError_t launch_stack_centres(const StackArgs& st, const MapArgs& map, const double* xcs, const double* ycs, int ncentres, int sampler,
                                bool round_f32, const LaunchOpts& opts, hipStream_t stream);

// tiles that left the staged path (box did not fit, containment vote failed), per translation unit: dcp_debug_counters adds them up
hipError_t read_lds_stats_unwarp(unsigned long long* out, bool reset);
hipError_t read_lds_stats_stack(unsigned long long* out, bool reset);
// -DDCP_DEBUG_BOUNDS builds: LDS taps outside their slab (count, first byte offset, slab bytes, site) per translation unit; zeros otherwise
hipError_t read_bounds_unwarp(unsigned long long* out, bool reset);
hipError_t read_bounds_stack(unsigned long long* out, bool reset);
hipError_t read_bounds_color(unsigned long long* out, bool reset);
hipError_t read_bounds_spline(unsigned long long* out, bool reset);
hipError_t read_bounds_spline_color(unsigned long long* out, bool reset);
hipError_t read_bounds_spline_frames(unsigned long long* out, bool reset);
hipError_t read_bounds_gauss(unsigned long long* out, bool reset);
hipError_t read_bounds_label(unsigned long long* out, bool reset);
hipError_t read_bounds_fourier(unsigned long long* out, bool reset);
hipError_t read_bounds_profile(unsigned long long* out, bool reset);
hipError_t read_bounds_select(unsigned long long* out, bool reset);
hipError_t read_bounds_extrema_select(unsigned long long* out, bool reset);
void set_last_kernel_name(const char* name);   // for the launchers of the other translation units
const char* last_kernel_name();   // unwarp_kernels.hip: the kernel the calling thread launched last (float32 image / stack launchers)
void set_spline_wg(int v);      // 0: spline taps always from global memory (option "spline_wg")
// Frame plans (frame_plan.cpp): per calibration and frame shape, the hull of every 128 x 32 tile and a certificate bit per 64 x 16 wave
// tile, built once on the device by plan_table_kernel and kept for the frames that follow.  Layout of a plan of n tiles, in int32 words:
// [0, 4n) hulls (x0, x1, y0, y1) as box_table_kernel writes them, [4n, 5n) certificate words (bit w = wave tile w of the tile).
typedef hipError_t (*PlanBuildFn)(const ImageArgs& img, const MapArgs& map, int32_t* plan, hipStream_t stream);
// The plan for this launch (img: H, W, y_origin, rows_out, tiles_x, tiles_y of remap_wg_kernel; the current device), or nullptr: the
// launch goes without one.  *ordered = true: the plan may still be under construction on the device -- the launch that reads it must keep its barrier bit.
const int32_t* frame_plan_lookup(const ImageArgs& img, const MapArgs& map, hipStream_t stream, PlanBuildFn build, bool* ordered);
void set_frame_plan(int v);     // option "frame_plan": 0 never, 1 build on the second sighting of a calibration, 2 on the first
int get_frame_plan();
hipError_t frame_plan_last_counts(int* wave_tiles, int* exact_tiles);    // of the plan built last (waits for its build; not on a frame's path)
void frame_plan_release();      // frees every plan of every device (each device that holds plans is synchronised first)
void set_box_table(int v);      // option "box_table": remap_wg_kernel reads its tile hulls from box_table_kernel's table (0 never, 1 where it pays)
int get_box_table();
int get_spline_wg();
void set_spline_tiled(int v);   // 0: chunked prefilter passes + transposes even where the one-pass tiles qualify (option "spline_tiled")
int get_spline_tiled();
void set_pf2d_chunk(int v);     // rows per chunk of spline_prefilter2d_kernel (option "pf2d_chunk"; 0 = automatic)
int get_pf2d_chunk();
void set_pf2d_xcd(int v);       // 0: spline_prefilter2d_kernel's tiles in plain launch order (option "pf2d_xcd")
int get_pf2d_xcd();
void set_pf2d_two_pole(int v);  // 0: the two-pole spline orders (4, 5) on spline_tile_filter_kernel, one launch per axis (option "pf2d_two_pole")
int get_pf2d_two_pole();
void set_spline_xcd(int v);     // 0: spline_wg_kernel's tiles in plain launch order (option "spline_xcd")
int get_spline_xcd();
// spline_kernels.hip: any MapKind (kCoords: ca.npts points into dst)
hipError_t launch_spline(const SplineArgs& a, MapKind kind, const MapArgs& map, const CoordArgs& ca, void* dst,
                         hipStream_t stream);
// spline_kernels.hip: the prefilter half of launch_spline -- the plane at a.src (strides a.src_stride / a.src_cstride) -> coefficients in
// a.coef, a.scratch the second plane; `desc`: the kernels' names as dcp_last_kernel reports them in front of the gather's
hipError_t launch_spline_prefilter(const SplineArgs& a, hipStream_t stream, char* desc, size_t desc_len);
// does the LDS-staged gather (spline_wg_kernel / spline_wg_color_kernel / spline_wg_frames_kernel) take this frame under this map?
bool spline_wg_takes(const SplineArgs& a, MapKind kind, const MapArgs& map);
// spline_color_kernels.hip: interleaved (H, W, channels) image, channels = 1..4, radial / perspective / fused map, orders 2..5.
// a.src_cstride = elements between pixels; a.coef = channels + 1 planes of Hp x Wp doubles (a.scratch is ignored); dst dense
hipError_t launch_spline_color(const SplineArgs& a, MapKind kind, const MapArgs& map, int channels, void* dst, hipStream_t stream);
// spline_frames_kernels.hip: `nframes` frames of one calibration, `src_frame_stride` elements apart (unit column stride), radial /
// perspective / fused map, orders 2..5.  a.coef = nframes + 1 planes of Hp x Wp doubles (a.scratch is ignored); dst dense (nframes, H, W)
hipError_t launch_spline_frames(const SplineArgs& a, MapKind kind, const MapArgs& map, int nframes, int64_t src_frame_stride, void* dst,
                                hipStream_t stream);
// typed_kernels.hip: any MapKind (kCoords: ca.npts points into img.dst)
hipError_t launch_typed_image(MapKind kind, const TypedImageArgs& img, const MapArgs& map, const CoordArgs& ca,
                              hipStream_t stream);
hipError_t launch_typed_stack(const TypedStackArgs& st, const MapArgs& map, hipStream_t stream);
// n points (y, x) -> centre + B(r) (p - centre), float64
hipError_t launch_map_points(const double* yx_in, double* yx_out, int64_t n, const MapArgs& map, hipStream_t stream);
// n points (y, x) through the homography map.coef (numpy's operation order), float64
hipError_t launch_map_points_persp(const double* yx_in, double* yx_out, int64_t n, const MapArgs& map, hipStream_t stream);
// n points (y, x) -> centre + (ru / rd) (p - centre), ru the root of ru B(ru) = rd (safeguarded Newton, float64); a point without a
// root becomes NaN and adds one to *n_unsolved (device memory, zeroed by the caller on `stream`; nullptr: not counted)
hipError_t launch_map_points_inverse(const double* yx_in, double* yx_out, int64_t n, const MapArgs& map, unsigned long long* n_unsolved,
                                     hipStream_t stream);
// forward_kernels.hip: the forward scatter of unwarp_image_forward (discorpy/post/postprocessing.py:151-185).  Source pixel s = y W + x
// goes to d = yu W + xu; `winner` (H W words, zeroed by the launcher on `stream`) keeps the greatest s + 1 per destination, the fill
// pass moves the winners' elements (esize = 1, 2, 4 or 8 bytes; source strides in elements, dense destination).  H W < 2^32 - 1.
struct ForwardArgs {
  const void* src;
  void* dst;
  uint32_t* winner;
  int64_t src_stride, src_cstride;
  int32_t H, W;
  int32_t esize;
};
hipError_t launch_forward(const ForwardArgs& a, const MapArgs& map, hipStream_t stream);
// median_kernels.hip: the size_y x size_x median (rank size_y size_x / 2) of every pixel's window under scipy's "reflect", any ElemType;
// rows of src `src_stride` elements apart, dst dense, the two not overlapping.  use_lds = false: every tap from global memory
// (median_global_kernel) even where a key box fits LDS (median_lds_kernel)
hipError_t launch_median(const void* src, void* dst, int H, int W, int64_t src_stride, int dtype, int size_y, int size_x, bool use_lds,
                         hipStream_t stream);
// gauss_kernels.hip: the symmetric correlation of scipy.ndimage.gaussian_filter, axis 0 (weights wy, radius ry) then axis 1 (wx, rx) on the
// result rounded to the element type; w*: 2 r + 1 host doubles, symmetric (only the first r + 1 are read); a radius of -1 skips its
// axis (both: a copy).  `boundary` is a BoundaryMode (the grid- spellings are scipy's aliases here), cval the value outside under
// kModeConstant.  Rows of src `src_stride` elements apart, dst dense, the two not overlapping.  One launch (gauss_lds_kernel) where
// gauss_takes_lds() says so, else one launch of gauss_axis_kernel per axis; with both axes that route writes the first pass to `tmp`
// (H W elements of the type, device memory; unused and may be null otherwise).  Any ElemType but kBool.
constexpr int kGaussMaxRadius = 192;     // the weights travel in the kernels' argument block: 2 x 193 doubles
constexpr int kGaussFusedMaxRadius = 24; // "x_gauss_lds" = 1: gauss_lds_kernel is the default up to this radius and
constexpr int kGaussFusedMaxLds = 80 << 10;  // this many bytes of LDS, two workgroups per CU (see gauss_takes_lds)
bool gauss_takes_lds(int dtype, int ry, int rx, int lds_mode);
hipError_t launch_gauss(const void* src, void* dst, void* tmp, int H, int W, int64_t src_stride, int dtype, const double* wy, int ry,
                        const double* wx, int rx, int boundary, double cval, int lds_mode, hipStream_t stream);
// fourier_kernels.hip: the Fourier Gaussian filter of _apply_fft_filter as two Toeplitz passes in float64: dst (dense H x W doubles) from
// the H x W plane at src (any ElemType, rows `src_stride` elements apart) padded by `pad` under `boundary` (np.pad's mode as a
// BoundaryMode: kModeMirror "reflect", kModeReflect "symmetric", kModeNearest "edge", kModeWrap "wrap", kModeConstant zeros).
// taps = {y re, y im, x re, x im}: HOST arrays of 2 N - 1 doubles, N the padded side of the axis; ry / rx: the support radius per axis
// (only |d| <= r and |d| >= N - r are summed).  `work`: fourier_work_bytes() of device memory.  THE STREAM IS SYNCHRONISED once, after
// the tables have been copied and before the kernels are enqueued.
constexpr int kFourierRows = 8;          // outputs per thread along the summed axis' output index (rows in pass 1, columns in pass 2)
constexpr int kFourierMaxSide = 16384;   // padded side: the tables stay below 2^15 entries, every index far inside int32
size_t fourier_work_bytes(int H, int W, int pad);
hipError_t launch_fourier(const void* src, double* dst, void* work, int H, int W, int64_t src_stride, int dtype, int pad, int boundary,
                          const double* const taps[4], int ry, int rx, hipStream_t stream);
// profile_kernels.hip: the per-profile steps of the line-pattern route on an (N, L) plane of float32 / float64 profiles (kF32, kF64), rows of
// src `src_stride` elements apart, every dst dense.
// The local minima of get_local_extrema_points: sample i of range(radius, L - radius - 1) is a point iff it equals the minimum of its window
// [i - radius, i + radius], the window holds no NaN and |(v - m) / m| > sensitive (0 where m == 0), m = np.mean of the `radius` largest
// window elements in ascending order (NumPy's pairwise sum, then one division), all in the row's type; the comparison with `sensitive`
// is made in float64.  dst: (N, L) doubles; row r holds its positions in ascending order and, in element L - 1, their number.
// subpixel: every position refined by the parabola through d[i - 1], d[i], d[i + 1] in float64 (needs radius >= 1).
constexpr int kPeakMaxRadius = 128;            // the sorted tail stays inside one block of NumPy's pairwise sum
hipError_t launch_peak_rows(const void* src, double* dst, int N, int L, int64_t src_stride, int dtype, int radius, double sensitive, bool subpixel,
                            hipStream_t stream);
// sliding_window_slope before its normalisation: |slope| of the least-squares line through the `size` (odd, >= 3) samples around every sample
// of the edge-padded row; products and sum in float64 (k ascending), the quotient rounded to the row's type.  dst of src's type; N <= 65535
hipError_t launch_window_slope(const void* src, void* dst, int N, int L, int64_t src_stride, int dtype, int size, hipStream_t stream);
// `nprof` tilted profiles of `len` samples of the H x W plane at src: profile p is the cubic spline (scipy's prefilter and weights, mode
// "nearest") of its own band -- rows (vertical: columns) band_lo[p] .. band_lo[p] + band_n[p] - 1 -- sampled at the image coordinates
// (ycoord, xcoord)[p][i] (device doubles).  band_lo / band_n are HOST arrays.  dst: (nprof, len) of src's type.  `work`: work_bytes of
// device memory: kProfileGroupMax * 24 bytes for the band table, then room for profile_band_elems() doubles of the widest band at least;
// profiles whose planes do not fit together run in groups.
// THE STREAM IS SYNCHRONISED once per group, after the group's band table has been copied.
constexpr int kProfileGroupMax = 256;          // profiles per group: their band table travels in one copy
size_t profile_band_elems(int H, int W, bool vertical, int n);
hipError_t launch_tilted_profiles(const void* src, void* dst, int H, int W, int64_t src_stride, int dtype, bool vertical, int nprof, int len,
                                  const double* ycoord, const double* xcoord, const int32_t* band_lo, const int32_t* band_n, void* work, size_t work_bytes,
                                  hipStream_t stream);
// select_peaks_kernels.hip: select_good_peaks on `npeaks` candidates of an (N, L) plane of kF32 / kF64 profiles: candidate k is sample
// peak_idx[k] of row peak_row[k] (HOST arrays, every entry inside the plane).  keep[k] = 1 where the fit of the window of `radius`
// samples on either side succeeded with |c| < radius / 2, the 80th percentile of |fit - y| below tol and (use_offset) |d| < tol;
// fit (may be null): per candidate a, b, c, d, that percentile and the status below.  keep and fit are device memory.  `work`:
// select_peaks_work_bytes(npeaks) of device memory.  THE STREAM IS SYNCHRONISED once, after the two tables have been copied.
constexpr int kSelectMaxRadius = 128;          // the window of one wave: 257 doubles of LDS
enum FitStatus : int {
  kFitOk = 0,
  kFitShort = 1,          // a window of 3 samples or fewer: no fit
  kFitNotFinite = 2,      // a NaN or an infinity in the window: no fit
  kFitConstant = 3,       // max == min: no fit
  kFitBudget = 4,         // the evaluations ran out before a stopping rule held
  kFitDiverged = 5,       // a sum, a step or a parameter stopped being finite
  kFitGradient = 6        // the residuals at right angles to the Jacobian's columns to machine precision before a stopping rule held
};
inline size_t select_peaks_work_bytes(int npeaks) { return (size_t)npeaks * 2 * sizeof(int32_t); }
hipError_t launch_select_peaks(const void* src, int N, int L, int64_t src_stride, int dtype, const int32_t* peak_row, const int32_t* peak_idx, int npeaks,
                               int radius, double tol, bool use_offset, unsigned char* keep, double* fit, void* work, hipStream_t stream);
// extrema_select_kernels.hip: the search of launch_peak_rows, select_good_peaks on every candidate it finds and the sub-pixel step on the kept
// ones, on an (N, L) plane of kF32 / kF64 profiles.  The fits read sel (the plane's type and shape, rows `sel_stride` elements apart) or, where
// sel is null, (T)(max(row) - row[i]) of src.  dst: (N, L) doubles, row r = the kept positions in ascending order and, in element L - 1,
// their number.  cand (may be null): the same table of the candidates before selection, integer positions; keep (may be null): (N, L)
// bytes, keep[r, j] = 0 / 1 for candidate j of row r.  All device memory.  `work`: extrema_select_work_bytes(N, L) of device memory.
// 1 <= radius <= kSelectMaxRadius.  NOTHING HERE SYNCHRONISES THE STREAM OR READS A COUNT ON THE HOST.
size_t extrema_select_work_bytes(int N, int L);
hipError_t launch_extrema_select(const void* src, double* dst, int N, int L, int64_t src_stride, int dtype, int radius, double sensitive, bool subpixel,
                                 const void* sel, int64_t sel_stride, double tol, bool use_offset, double* cand, unsigned char* keep, void* work,
                                 hipStream_t stream);
// radon_kernels.hip: the sinogram of the N x N plane at src (kF32 / kF64, rows `src_stride` elements apart) for `nangles` angles, as
// DESIGN.md ("Radon transform") defines it: the plane zeroed outside its inscribed circle, rotated about (N / 2, N / 2) by bilinear
// interpolation with zeros outside, and summed over the rows in ascending order, all in float64.  table: HOST array of {cos a, sin a,
// tx, ty} per angle.  dst: dense (N, nangles) doubles.  `work`: radon_work_bytes(nangles) of device memory.
// THE STREAM IS SYNCHRONISED once, after the table has been copied and before the kernel is enqueued.
constexpr int kRadonMaxSide = 32768;           // with kRadonMaxAngles: N * nangles < 2^31, (N / 2)^2 * 2 < 2^31, every index fits int32
constexpr int kRadonMaxAngles = 65535;         // one angle per blockIdx.y
inline size_t radon_work_bytes(int nangles) { return (size_t)nangles * 4 * sizeof(double); }
hipError_t launch_radon(const void* src, double* dst, int N, int64_t src_stride, int dtype, int nangles, const double* table, void* work,
                        hipStream_t stream);
// dotgrid_kernels.hip, DESIGN.md ("Dot grid").  The sinogram of the H x W plane at src (kF32 / kF64, rows `src_stride` elements apart)
// embedded in a square of zeros of side S = radon_padded_side(H, W) with its first element at (S / 2 - H / 2, S / 2 - W / 2): the square
// transformed as launch_radon transforms its plane but without the circle; no padded plane exists, and nothing outside the H x W view is
// read.  table: HOST array of {cos a, sin a, tx, ty} per angle FOR SIDE S.  dst: dense (S, nangles) doubles.  `work`:
// radon_work_bytes(nangles) of device memory.  THE STREAM IS SYNCHRONISED once, after the table has been copied.
inline int radon_padded_side(int H, int W) { return (int)__builtin_ceil(__builtin_sqrt(2.0) * (double)(H > W ? H : W)); }
hipError_t launch_radon_padded(const void* src, double* dst, int H, int W, int64_t src_stride, int dtype, int nangles, const double* table,
                               void* work, hipStream_t stream);
// dst[i][0..3] (dense (N, 4) doubles) = the four smallest of (y_i - y_j) * (y_i - y_j) + (x_i - x_j) * (x_i - x_j) over all j (j = i
// included), ascending, +inf where N < 4; pts: dense (N, 2) doubles (y, x), device memory.  One launch.
constexpr int kNearMaxPoints = 1 << 20;
hipError_t launch_nearest_sq_dists(const double* pts, double* dst, int N, hipStream_t stream);
// sums[n][6] = count, sum y, sum x, sum y y, sum x y, sum x x over the nonzero elements of src (kBool or an 8- / 16-bit integer type) inside
// box b = boxes[b][4] = min y, max y, min x, max x (inclusive, INSIDE THE PLANE or empty: max < min), (y, x) relative to the box's corner.
// boxes: HOST array; `work`: box_work_bytes(n) of device memory.  THE STREAM IS SYNCHRONISED once, after the boxes have been copied.
constexpr int kBoxMaxSide = 32768;             // every sum stays below 2^60
constexpr int kBoxMaxBoxes = 1 << 24;
inline size_t box_work_bytes(int n) { return (size_t)n * 4 * sizeof(int32_t); }
hipError_t launch_box_moments(const void* src, int H, int W, int64_t src_stride, int dtype, const int32_t* boxes, int n, long long* sums,
                              void* work, hipStream_t stream);
// label_kernels.hip: connected components of the nonzero pixels (any ElemType; floats by their bits: NaN is set, -0.0 is not) numbered
// as scipy.ndimage.label numbers them, into dst (dense H x W int32, 0 = background).  conn8: the full 3 x 3 structure, else the cross.
// `parent`: H W int32 of device scratch, `counts`: label_count_words(H, W) more; the number of labels is left in the LAST word of
// counts.  use_lds = false: no tile-local stage, the global union over every pixel pair (option "x_label_lds" = 0).  H W < 2^31.
constexpr int kLabelTW = 128, kLabelTH = 32;   // label_tile_kernel's tile: kLabelTW * kLabelTH int32 = 16 KiB of LDS
constexpr int kLabelScanChunk = 4096;          // pixels per workgroup of the root count and rank
size_t label_count_words(int H, int W);
hipError_t launch_label(const void* src, int32_t* dst, int32_t* parent, int32_t* counts, int H, int W, int64_t src_stride, int dtype, bool conn8,
                        bool use_lds, hipStream_t stream);
// scipy.ndimage.binary_fill_holes into dst (dense H x W bytes of 0 / 1); `parent` and `root`: H W int32 of device scratch each
hipError_t launch_fill_holes(const void* src, uint8_t* dst, int32_t* parent, int32_t* root, int H, int W, int64_t src_stride, int dtype,
                             bool use_lds, hipStream_t stream);
// skimage.segmentation.clear_border on a binary image into dst (dense H x W bytes of 0 / 1): the set pixels (invert: the ZERO pixels)
// whose component (conn8: full 3 x 3 structure, else the cross) has no pixel on the image border.  Scratch as for launch_fill_holes
hipError_t launch_clear_border(const void* src, uint8_t* dst, int32_t* parent, int32_t* root, int H, int W, int64_t src_stride, int dtype,
                               bool conn8, bool invert, bool use_lds, hipStream_t stream);
// binarize_kernels.hip: the steps of discorpy.prep.preprocessing.binarization that labelling does not cover.  Rows of src `src_stride`
// elements apart, every dst dense.
constexpr int kHistLdsMaxBins = 4096;          // up to this many bins a workgroup counts in LDS (32-bit, flushed with 64-bit atomics);
                                               // above it (a 16-bit bincount has up to 65536) every element adds to global memory
constexpr int kMorphTW = 128, kMorphTH = 32;   // morph_cross_kernel's output tile; its LDS planes carry a halo of 1 (one op) or 2 (opening)
constexpr int kReduceMaxBlocks = 1024;         // workgroups of minmax_kernel / histogram_kernel (they stride over the rows)
// np.abs: floats lose their sign bit, signed integers wrap at their minimum, unsigned / bool are copied.  Any ElemType
hipError_t launch_abs(const void* src, void* dst, int H, int W, int64_t src_stride, int dtype, hipStream_t stream);
// out[0] = minimum, out[1] = maximum as NumPy's a.min() / a.max() give them (NaN if any element is), nonfinite[0] = elements that are NaN
// or infinite; kF32, kF64 and the 8- / 16-bit integers.  `partials`: 3 * kReduceMaxBlocks doubles of device scratch
hipError_t launch_minmax(const void* src, int H, int W, int64_t src_stride, int dtype, double* partials, double* out, long long* nonfinite,
                         hipStream_t stream);
// counts[nbins] (int64, zeroed here).  edges != null (device memory, nbins + 1 ascending values of the plane's float type): bin i holds
// edges[i] <= a < edges[i + 1], the last one a == edges[nbins] too, anything else (NaN included) is not counted.  edges == null (8- / 16-bit
// integers): bin a - first, elements outside [first, first + nbins) are not counted.  use_lds = false: global atomics at any bin count
hipError_t launch_histogram(const void* src, int H, int W, int64_t src_stride, int dtype, const void* edges, int nbins, long long first,
                            long long* counts, bool use_lds, hipStream_t stream);
// dst = (double)a > thres (NaN: 0) as bytes; *count (device int64, may be null) += the number of set pixels.  Any ElemType
hipError_t launch_threshold(const void* src, uint8_t* dst, int H, int W, int64_t src_stride, int dtype, double thres, long long* count,
                            hipStream_t stream);
// grey erosion (op 0), dilation (op 1) or opening (op 2) of a uint8 plane by the 3 x 3 cross over the in-image neighbours only.  Opening:
// one launch (both steps on a tile with a halo of 2 in LDS) when fused, else erosion into `tmp` (H W bytes of device scratch) and dilation
hipError_t launch_morph_cross(const uint8_t* src, uint8_t* dst, uint8_t* tmp, int H, int W, int64_t src_stride, int op, bool fused,
                              hipStream_t stream);
// per label 1..num of `labels` (rows l_stride apart; other values are ignored): sums[num][4] = pixel count, sum v, sum y v, sum x v over
// its pixels and boxes[num][4] = min y, max y, min x, max x ((H, -1, W, -1) for an absent label); v from `weights` (kBool, kU8, kI8, kU16
// or kI16; rows w_stride apart) or 1 everywhere where weights is null
hipError_t launch_label_measures(const void* weights, const int32_t* labels, int H, int W, int64_t w_stride, int64_t l_stride, int dtype, int num,
                                 long long* sums, int32_t* boxes, hipStream_t stream);
// sort_kernels.hip: dst (dense, H W elements of the type) = the plane's elements in ascending order -- an 8-bit-digit radix sort of
// order-preserving keys; floats as np.sort orders them (NaNs of either sign last, a negative NaN comes out positive; -0.0 before +0.0).
// Any ElemType but kBool.  `work`: sort_work_bytes() of device memory (two key buffers, the bins, the plan, the (digit, workgroup)
// table).  skip = false: the passes whose digit is the same in every key run too (option "x_sort_skip" = 0).  H W < 2^31.
constexpr int kSortMaxBlocks = 2048;           // workgroups of a pass: the columns of the (digit, workgroup) table
size_t sort_work_bytes(int64_t n, int dtype);
hipError_t launch_sort(const void* src, void* dst, int H, int W, int64_t src_stride, int dtype, void* work, bool skip, hipStream_t stream);
// dst[0 .. out_n) = scipy.ndimage.zoom(src, out_n / n, order=3, mode="nearest") of the n elements at src, both of `dtype` (any ElemType
// but kBool); z_n = pow(sqrt(3) - 2, n + 24) from the host's C library, as scipy computes it.  One launch, no scratch.
hipError_t launch_zoom_cubic_nearest(const void* src, int64_t n, void* dst, int64_t out_n, int dtype, double z_n, hipStream_t stream);
// interleaved (H, W, C) image, radial / perspective / fused map, orders 0 / 1; src_cstride = elements between pixels
hipError_t launch_typed_channels(MapKind kind, const TypedImageArgs& img, const MapArgs& map, int channels, hipStream_t stream);
// color_kernels.hip: the same on remap_wg_kernel's data path (3 / 4 dense channels of float32 / uint8 / uint16, level-2 certificate of
// the map's kind); img as for launch_wg_typed with src_col_stride = channels; *taken = false: does not qualify, use launch_typed_channels
hipError_t launch_color(MapKind kind, const ImageArgs& img, const MapArgs& map, int channels, int dtype, int sampler, const LaunchOpts& opts,
                        hipStream_t stream, bool* taken);

}  // namespace dcp
