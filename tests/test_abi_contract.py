"""CPU suite: the error contract of the 19 single-frame entry points of the C ABI.  Every case makes ONE argument of a valid call
invalid and checks the return code and a fragment of dcp_last_error().  Every call is refused before any device work, so the
answers are the same with or without a GPU (and no case reaches a kernel: the buffers are host memory)."""
import ctypes as C

import numpy as np
import pytest

from discorpy_amd import _ffi as F

INV, UNS = F.ERR_INVALID_ARG, F.ERR_UNSUPPORTED
H, W = 8, 10
_keep = []


def _buf(nbytes):
    a = np.zeros(max(int(nbytes), 16), np.uint8)
    _keep.append(a)
    return a.ctypes.data


def _dbl(vals):
    a = np.array(vals, np.float64)
    _keep.append(a)
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ptrs(vals):
    a = (C.c_void_p * len(vals))(*vals)
    _keep.append(a)
    return a


SRC, DST = _buf(H * W * 8 * 4), _buf(H * W * 8 * 4)
YC, XC = _buf(64 * 8), _buf(64 * 8)
FACT = _dbl([1.0, -1e-4, 0.0, 0.0] * 40)
COEF = _dbl([1.0, 0.0, 0.5, 0.0, 1.0, -0.5, 0.0, 0.0])
IMG = dict(src=SRC, dst=DST, height=H, width=W, rs=W, cs=1)
RAD = dict(xc=5.0, yc=4.0, fact=FACT, nfact=3)
COORDS = dict(y=YC, x=XC, coord_dtype=F.COORD_F32, npts=64)
TAIL = dict(mem_kind=F.MEM_HOST, device=-1, stream=None)

# entry point -> (argument names in declaration order, a valid call)
ENTRIES = {
    "dcp_unwarp_image_f32": ("src dst height width rs cs xc yc fact nfact order round blend mem_kind device stream",
                             dict(IMG, **RAD, order=1, round=1, blend=F.BLEND_F64LERP, **TAIL)),
    "dcp_unwarp_images_f32": ("srcs dsts nframes height width rs cs xcs ycs fact nfact order round blend mem_kind device stream",
                              dict(srcs=_ptrs([SRC, SRC]), dsts=_ptrs([DST, _buf(H * W * 4)]), nframes=2, height=H, width=W, rs=W, cs=1,
                                   xcs=_dbl([5.0, 5.0]), ycs=_dbl([4.0, 4.0]), fact=FACT, nfact=3, order=1, round=1,
                                   blend=F.BLEND_F64LERP, **TAIL)),
    "dcp_perspective_image_f32": ("src dst height width rs cs coef order blend mem_kind device stream",
                                  dict(IMG, coef=COEF, order=1, blend=F.BLEND_SCIPY, **TAIL)),
    "dcp_unwarp_fused_f32": ("src dst height width rs cs xc yc fact nfact coef order blend mem_kind device stream",
                             dict(IMG, **RAD, coef=COEF, order=1, blend=F.BLEND_SCIPY, **TAIL)),
    "dcp_remap_coords_f32": ("src dst height width rs cs y x coord_dtype npts order blend mem_kind device stream",
                             dict(IMG, **COORDS, order=1, blend=F.BLEND_SCIPY, **TAIL)),
    "dcp_remap_coords_mode_f32": ("src dst height width rs cs y x coord_dtype npts order mode blend mem_kind device stream",
                                  dict(IMG, **COORDS, order=1, mode=0, blend=F.BLEND_SCIPY, **TAIL)),
    "dcp_unwarp_image_typed": ("src dst dtype height width rs cs xc yc fact nfact order mode mem_kind device stream",
                               dict(IMG, dtype=4, **RAD, order=1, mode=0, **TAIL)),
    "dcp_perspective_image_typed": ("src dst dtype height width rs cs coef order mode mem_kind device stream",
                                    dict(IMG, dtype=4, coef=COEF, order=1, mode=0, **TAIL)),
    "dcp_unwarp_fused_typed": ("src dst dtype height width rs cs xc yc fact nfact coef order mode mem_kind device stream",
                               dict(IMG, dtype=4, **RAD, coef=COEF, order=1, mode=0, **TAIL)),
    "dcp_remap_coords_typed": ("src dst dtype height width rs cs y x coord_dtype npts order mode mem_kind device stream",
                               dict(IMG, dtype=4, **COORDS, order=1, mode=0, **TAIL)),
    "dcp_unwarp_image_channels": ("src dst dtype height width channels rs cs xc yc fact nfact order mem_kind device stream",
                                  dict(IMG, dtype=2, channels=3, rs=3 * W, cs=3, **RAD, order=1, **TAIL)),
    "dcp_unwarp_color_image": ("src dst dtype height width channels rs cs xc yc fact nfact order blend mem_kind device stream",
                               dict(IMG, dtype=2, channels=3, rs=3 * W, cs=3, **RAD, order=1, blend=F.BLEND_SCIPY, **TAIL)),
    "dcp_map_points_f64": ("y x npts xc yc fact nfact mem_kind device stream",
                           dict(y=YC, x=XC, npts=16, **RAD, **TAIL)),
    "dcp_map_points_perspective_f64": ("y x npts coef mem_kind device stream", dict(y=YC, x=XC, npts=16, coef=COEF, **TAIL)),
    "dcp_coordinate_map_f32": ("src dst height width map_kind xc yc fact nfact coef mem_kind device stream",
                               dict(src=SRC, dst=DST, height=H, width=W, map_kind=F.MAP_FUSED, **RAD, coef=COEF, **TAIL)),
    "dcp_unwarp_image_spline_f32": ("src dst height width rs cs xc yc fact nfact order mode mem_kind device stream",
                                    dict(IMG, **RAD, order=3, mode=0, **TAIL)),
    "dcp_perspective_image_spline_f32": ("src dst height width rs cs coef order mode mem_kind device stream",
                                         dict(IMG, coef=COEF, order=3, mode=0, **TAIL)),
    "dcp_unwarp_fused_spline_f32": ("src dst height width rs cs xc yc fact nfact coef order mode mem_kind device stream",
                                    dict(IMG, **RAD, coef=COEF, order=3, mode=0, **TAIL)),
    "dcp_remap_coords_spline_f32": ("src dst height width rs cs y x coord_dtype npts order mode mem_kind device stream",
                                    dict(IMG, **COORDS, order=3, mode=0, **TAIL)),
}

# (entry point, the one invalid argument(s), return code, fragment of dcp_last_error()).  Recorded from the library before the
# frame calls were routed through one call description (no GPU visible), except the rows marked "was": an unknown mem_kind is
# now refused before any device work everywhere -- the spline entry points used to lock and grow their workspace first
# (DCP_ERR_HIP without a GPU), empty calls used to return DCP_OK without looking at it.
CASES = [
    ('dcp_unwarp_image_f32', {'src': None}, INV, 'null image pointer'),
    ('dcp_unwarp_image_f32', {'dst': None}, INV, 'null image pointer'),
    ('dcp_unwarp_image_f32', {'height': 0}, INV, 'image must be non-empty (got 0 x 10)'),
    ('dcp_unwarp_image_f32', {'height': -1}, INV, 'image must be non-empty (got -1 x 10)'),
    ('dcp_unwarp_image_f32', {'width': 0}, INV, 'image must be non-empty (got 8 x 0)'),
    ('dcp_unwarp_image_f32', {'rs': 0}, INV, 'strides must be positive (row 0, col 1)'),
    ('dcp_unwarp_image_f32', {'cs': 0}, INV, 'strides must be positive (row 10, col 0)'),
    ('dcp_unwarp_image_f32', {'fact': None}, INV, 'null coefficient pointer'),
    ('dcp_unwarp_image_f32', {'nfact': 33}, INV, 'nfact = 33 outside [0, 32] (DCP_MAX_FACT is a li'),
    ('dcp_unwarp_image_f32', {'nfact': -1}, INV, 'nfact = -1 outside [0, 32] (DCP_MAX_FACT is a li'),
    ('dcp_unwarp_image_f32', {'order': 7}, UNS, 'spline order 7 is not implemented on the GPU pat'),
    ('dcp_unwarp_image_f32', {'order': -1}, UNS, 'spline order -1 is not implemented on the GPU pa'),
    ('dcp_unwarp_image_f32', {'order': 2}, UNS, 'spline order 2 is not implemented on the GPU pat'),
    ('dcp_unwarp_image_f32', {'blend': 9}, INV, 'unknown blend_mode 9'),
    ('dcp_unwarp_image_f32', {'mem_kind': 7}, INV, 'unknown mem_kind 7'),
    ('dcp_unwarp_image_f32', {'rs': 9}, INV, 'row stride 9 overlaps rows of width 10'),
    ('dcp_unwarp_images_f32', {'srcs': None}, INV, 'null frame / centre array'),
    ('dcp_unwarp_images_f32', {'nframes': -1}, INV, 'nframes < 0'),
    ('dcp_unwarp_images_f32', {'height': 0}, INV, 'image must be non-empty (got 0 x 10)'),
    ('dcp_unwarp_images_f32', {'height': -1}, INV, 'image must be non-empty (got -1 x 10)'),
    ('dcp_unwarp_images_f32', {'width': 0}, INV, 'image must be non-empty (got 8 x 0)'),
    ('dcp_unwarp_images_f32', {'rs': 0}, INV, 'strides must be positive (row 0, col 1)'),
    ('dcp_unwarp_images_f32', {'cs': 0}, INV, 'strides must be positive (row 10, col 0)'),
    ('dcp_unwarp_images_f32', {'xcs': None}, INV, 'null frame / centre array'),
    ('dcp_unwarp_images_f32', {'fact': None}, INV, 'null coefficient pointer'),
    ('dcp_unwarp_images_f32', {'nfact': 33}, INV, 'nfact = 33 outside [0, 32] (DCP_MAX_FACT is a li'),
    ('dcp_unwarp_images_f32', {'nfact': -1}, INV, 'nfact = -1 outside [0, 32] (DCP_MAX_FACT is a li'),
    ('dcp_unwarp_images_f32', {'order': 7}, UNS, 'spline order 7 is not implemented on the GPU pat'),
    ('dcp_unwarp_images_f32', {'order': -1}, UNS, 'spline order -1 is not implemented on the GPU pa'),
    ('dcp_unwarp_images_f32', {'order': 2}, UNS, 'spline order 2 is not implemented on the GPU pat'),
    ('dcp_unwarp_images_f32', {'blend': 9}, INV, 'unknown blend_mode 9'),
    ('dcp_unwarp_images_f32', {'mem_kind': 7}, INV, 'unknown mem_kind 7'),
    ('dcp_unwarp_images_f32', {'rs': 9}, INV, 'row stride 9 overlaps rows of width 10'),
    ('dcp_unwarp_images_f32', {'nframes': 0, 'mem_kind': 7}, INV, 'unknown mem_kind 7'),  # was DCP_OK
    ('dcp_perspective_image_f32', {'src': None}, INV, 'null image pointer'),
    ('dcp_perspective_image_f32', {'dst': None}, INV, 'null image pointer'),
    ('dcp_perspective_image_f32', {'height': 0}, INV, 'image must be non-empty (got 0 x 10)'),
    ('dcp_perspective_image_f32', {'height': -1}, INV, 'image must be non-empty (got -1 x 10)'),
    ('dcp_perspective_image_f32', {'width': 0}, INV, 'image must be non-empty (got 8 x 0)'),
    ('dcp_perspective_image_f32', {'rs': 0}, INV, 'strides must be positive (row 0, col 1)'),
    ('dcp_perspective_image_f32', {'cs': 0}, INV, 'strides must be positive (row 10, col 0)'),
    ('dcp_perspective_image_f32', {'coef': None}, INV, 'null homography pointer'),
    ('dcp_perspective_image_f32', {'order': 7}, UNS, 'spline order 7 is not implemented on the GPU pat'),
    ('dcp_perspective_image_f32', {'order': -1}, UNS, 'spline order -1 is not implemented on the GPU pa'),
    ('dcp_perspective_image_f32', {'order': 2}, UNS, 'spline order 2 is not implemented on the GPU pat'),
    ('dcp_perspective_image_f32', {'blend': 9}, INV, 'unknown blend_mode 9'),
    ('dcp_perspective_image_f32', {'mem_kind': 7}, INV, 'unknown mem_kind 7'),
    ('dcp_perspective_image_f32', {'rs': 9}, INV, 'row stride 9 overlaps rows of width 10'),
    ('dcp_unwarp_fused_f32', {'src': None}, INV, 'null image pointer'),
    ('dcp_unwarp_fused_f32', {'dst': None}, INV, 'null image pointer'),
    ('dcp_unwarp_fused_f32', {'height': 0}, INV, 'image must be non-empty (got 0 x 10)'),
    ('dcp_unwarp_fused_f32', {'height': -1}, INV, 'image must be non-empty (got -1 x 10)'),
    ('dcp_unwarp_fused_f32', {'width': 0}, INV, 'image must be non-empty (got 8 x 0)'),
    ('dcp_unwarp_fused_f32', {'rs': 0}, INV, 'strides must be positive (row 0, col 1)'),
    ('dcp_unwarp_fused_f32', {'cs': 0}, INV, 'strides must be positive (row 10, col 0)'),
    ('dcp_unwarp_fused_f32', {'fact': None}, INV, 'null coefficient pointer'),
    ('dcp_unwarp_fused_f32', {'nfact': 33}, INV, 'nfact = 33 outside [0, 32] (DCP_MAX_FACT is a li'),
    ('dcp_unwarp_fused_f32', {'nfact': -1}, INV, 'nfact = -1 outside [0, 32] (DCP_MAX_FACT is a li'),
    ('dcp_unwarp_fused_f32', {'coef': None}, INV, 'null homography pointer'),
    ('dcp_unwarp_fused_f32', {'order': 7}, UNS, 'spline order 7 is not implemented on the GPU pat'),
    ('dcp_unwarp_fused_f32', {'order': -1}, UNS, 'spline order -1 is not implemented on the GPU pa'),
    ('dcp_unwarp_fused_f32', {'order': 2}, UNS, 'spline order 2 is not implemented on the GPU pat'),
    ('dcp_unwarp_fused_f32', {'blend': 9}, INV, 'unknown blend_mode 9'),
    ('dcp_unwarp_fused_f32', {'mem_kind': 7}, INV, 'unknown mem_kind 7'),
    ('dcp_unwarp_fused_f32', {'rs': 9}, INV, 'row stride 9 overlaps rows of width 10'),
    ('dcp_remap_coords_f32', {'src': None}, INV, 'null image pointer'),
    ('dcp_remap_coords_f32', {'dst': None}, INV, 'null image pointer'),
    ('dcp_remap_coords_f32', {'height': 0}, INV, 'image must be non-empty (got 0 x 10)'),
    ('dcp_remap_coords_f32', {'height': -1}, INV, 'image must be non-empty (got -1 x 10)'),
    ('dcp_remap_coords_f32', {'width': 0}, INV, 'image must be non-empty (got 8 x 0)'),
    ('dcp_remap_coords_f32', {'rs': 0}, INV, 'strides must be positive (row 0, col 1)'),
    ('dcp_remap_coords_f32', {'cs': 0}, INV, 'strides must be positive (row 10, col 0)'),
    ('dcp_remap_coords_f32', {'y': None}, INV, 'null coordinate pointer'),
    ('dcp_remap_coords_f32', {'x': None}, INV, 'null coordinate pointer'),
    ('dcp_remap_coords_f32', {'coord_dtype': 5}, INV, 'unknown coord_dtype 5'),
    ('dcp_remap_coords_f32', {'npts': -1}, INV, 'npts < 0'),
    ('dcp_remap_coords_f32', {'order': 7}, UNS, 'spline order 7 is not implemented on the GPU pat'),
    ('dcp_remap_coords_f32', {'order': -1}, UNS, 'spline order -1 is not implemented on the GPU pa'),
    ('dcp_remap_coords_f32', {'order': 2}, UNS, 'spline order 2 is not implemented on the GPU pat'),
    ('dcp_remap_coords_f32', {'blend': 9}, INV, 'unknown blend_mode 9'),
    ('dcp_remap_coords_f32', {'mem_kind': 7}, INV, 'unknown mem_kind 7'),
    ('dcp_remap_coords_f32', {'mem_kind': 0x101}, INV, 'unknown mem_kind 257'),
    ('dcp_remap_coords_f32', {'rs': 9}, INV, 'row stride 9 overlaps rows of width 10'),
    ('dcp_remap_coords_f32', {'npts': 0, 'mem_kind': 7}, INV, 'unknown mem_kind 7'),  # was DCP_OK
    ('dcp_remap_coords_mode_f32', {'src': None}, INV, 'null image pointer'),
    ('dcp_remap_coords_mode_f32', {'dst': None}, INV, 'null image pointer'),
    ('dcp_remap_coords_mode_f32', {'height': 0}, INV, 'image must be non-empty (got 0 x 10)'),
    ('dcp_remap_coords_mode_f32', {'height': -1}, INV, 'image must be non-empty (got -1 x 10)'),
    ('dcp_remap_coords_mode_f32', {'width': 0}, INV, 'image must be non-empty (got 8 x 0)'),
    ('dcp_remap_coords_mode_f32', {'rs': 0}, INV, 'strides must be positive (row 0, col 1)'),
    ('dcp_remap_coords_mode_f32', {'cs': 0}, INV, 'strides must be positive (row 10, col 0)'),
    ('dcp_remap_coords_mode_f32', {'y': None}, INV, 'null coordinate pointer'),
    ('dcp_remap_coords_mode_f32', {'x': None}, INV, 'null coordinate pointer'),
    ('dcp_remap_coords_mode_f32', {'coord_dtype': 5}, INV, 'unknown coord_dtype 5'),
    ('dcp_remap_coords_mode_f32', {'npts': -1}, INV, 'npts < 0'),
    ('dcp_remap_coords_mode_f32', {'order': 7}, UNS, 'spline order 7 is not implemented on the GPU pat'),
    ('dcp_remap_coords_mode_f32', {'order': -1}, UNS, 'spline order -1 is not implemented on the GPU pa'),
    ('dcp_remap_coords_mode_f32', {'order': 2}, UNS, 'spline order 2 is not implemented on the GPU pat'),
    ('dcp_remap_coords_mode_f32', {'mode': 9}, INV, 'unknown boundary mode 9'),
    ('dcp_remap_coords_mode_f32', {'mode': -1}, INV, 'unknown boundary mode -1'),
    ('dcp_remap_coords_mode_f32', {'blend': 9}, INV, 'unknown blend_mode 9'),
    ('dcp_remap_coords_mode_f32', {'mem_kind': 7}, INV, 'unknown mem_kind 7'),
    ('dcp_remap_coords_mode_f32', {'mem_kind': 0x101}, INV, 'unknown mem_kind 257'),
    ('dcp_remap_coords_mode_f32', {'rs': 9}, INV, 'row stride 9 overlaps rows of width 10'),
    ('dcp_remap_coords_mode_f32', {'npts': 0, 'mem_kind': 7}, INV, 'unknown mem_kind 7'),  # was DCP_OK
    ('dcp_unwarp_image_typed', {'src': None}, INV, 'null image pointer'),
    ('dcp_unwarp_image_typed', {'dst': None}, INV, 'null image pointer'),
    ('dcp_unwarp_image_typed', {'dtype': 99}, INV, 'unknown element type 99'),
    ('dcp_unwarp_image_typed', {'height': 0}, INV, 'image must be non-empty (got 0 x 10)'),
    ('dcp_unwarp_image_typed', {'height': -1}, INV, 'image must be non-empty (got -1 x 10)'),
    ('dcp_unwarp_image_typed', {'width': 0}, INV, 'image must be non-empty (got 8 x 0)'),
    ('dcp_unwarp_image_typed', {'rs': 0}, INV, 'strides must be positive (row 0, col 1)'),
    ('dcp_unwarp_image_typed', {'cs': 0}, INV, 'strides must be positive (row 10, col 0)'),
    ('dcp_unwarp_image_typed', {'fact': None}, INV, 'null coefficient pointer'),
    ('dcp_unwarp_image_typed', {'nfact': 33}, INV, 'nfact = 33 outside [0, 32] (DCP_MAX_FACT is a li'),
    ('dcp_unwarp_image_typed', {'nfact': -1}, INV, 'nfact = -1 outside [0, 32] (DCP_MAX_FACT is a li'),
    ('dcp_unwarp_image_typed', {'order': 7}, INV, 'spline order 7 outside [0, 5]'),
    ('dcp_unwarp_image_typed', {'order': -1}, INV, 'spline order -1 outside [0, 5]'),
    ('dcp_unwarp_image_typed', {'mode': 9}, INV, 'unknown boundary mode 9'),
    ('dcp_unwarp_image_typed', {'mode': -1}, INV, 'unknown boundary mode -1'),
    ('dcp_unwarp_image_typed', {'mem_kind': 7}, INV, 'unknown mem_kind 7'),
    ('dcp_unwarp_image_typed', {'mem_kind': 0x101}, INV, 'unknown mem_kind 257'),
    ('dcp_unwarp_image_typed', {'rs': 9}, INV, 'row stride 9 overlaps rows of width 10'),
    ('dcp_perspective_image_typed', {'src': None}, INV, 'null image pointer'),
    ('dcp_perspective_image_typed', {'dst': None}, INV, 'null image pointer'),
    ('dcp_perspective_image_typed', {'dtype': 99}, INV, 'unknown element type 99'),
    ('dcp_perspective_image_typed', {'height': 0}, INV, 'image must be non-empty (got 0 x 10)'),
    ('dcp_perspective_image_typed', {'height': -1}, INV, 'image must be non-empty (got -1 x 10)'),
    ('dcp_perspective_image_typed', {'width': 0}, INV, 'image must be non-empty (got 8 x 0)'),
    ('dcp_perspective_image_typed', {'rs': 0}, INV, 'strides must be positive (row 0, col 1)'),
    ('dcp_perspective_image_typed', {'cs': 0}, INV, 'strides must be positive (row 10, col 0)'),
    ('dcp_perspective_image_typed', {'coef': None}, INV, 'null homography pointer'),
    ('dcp_perspective_image_typed', {'order': 7}, INV, 'spline order 7 outside [0, 5]'),
    ('dcp_perspective_image_typed', {'order': -1}, INV, 'spline order -1 outside [0, 5]'),
    ('dcp_perspective_image_typed', {'mode': 9}, INV, 'unknown boundary mode 9'),
    ('dcp_perspective_image_typed', {'mode': -1}, INV, 'unknown boundary mode -1'),
    ('dcp_perspective_image_typed', {'mem_kind': 7}, INV, 'unknown mem_kind 7'),
    ('dcp_perspective_image_typed', {'mem_kind': 0x101}, INV, 'unknown mem_kind 257'),
    ('dcp_perspective_image_typed', {'rs': 9}, INV, 'row stride 9 overlaps rows of width 10'),
    ('dcp_unwarp_fused_typed', {'src': None}, INV, 'null image pointer'),
    ('dcp_unwarp_fused_typed', {'dst': None}, INV, 'null image pointer'),
    ('dcp_unwarp_fused_typed', {'dtype': 99}, INV, 'unknown element type 99'),
    ('dcp_unwarp_fused_typed', {'height': 0}, INV, 'image must be non-empty (got 0 x 10)'),
    ('dcp_unwarp_fused_typed', {'height': -1}, INV, 'image must be non-empty (got -1 x 10)'),
    ('dcp_unwarp_fused_typed', {'width': 0}, INV, 'image must be non-empty (got 8 x 0)'),
    ('dcp_unwarp_fused_typed', {'rs': 0}, INV, 'strides must be positive (row 0, col 1)'),
    ('dcp_unwarp_fused_typed', {'cs': 0}, INV, 'strides must be positive (row 10, col 0)'),
    ('dcp_unwarp_fused_typed', {'fact': None}, INV, 'null coefficient pointer'),
    ('dcp_unwarp_fused_typed', {'nfact': 33}, INV, 'nfact = 33 outside [0, 32] (DCP_MAX_FACT is a li'),
    ('dcp_unwarp_fused_typed', {'nfact': -1}, INV, 'nfact = -1 outside [0, 32] (DCP_MAX_FACT is a li'),
    ('dcp_unwarp_fused_typed', {'coef': None}, INV, 'null homography pointer'),
    ('dcp_unwarp_fused_typed', {'order': 7}, INV, 'spline order 7 outside [0, 5]'),
    ('dcp_unwarp_fused_typed', {'order': -1}, INV, 'spline order -1 outside [0, 5]'),
    ('dcp_unwarp_fused_typed', {'mode': 9}, INV, 'unknown boundary mode 9'),
    ('dcp_unwarp_fused_typed', {'mode': -1}, INV, 'unknown boundary mode -1'),
    ('dcp_unwarp_fused_typed', {'mem_kind': 7}, INV, 'unknown mem_kind 7'),
    ('dcp_unwarp_fused_typed', {'mem_kind': 0x101}, INV, 'unknown mem_kind 257'),
    ('dcp_unwarp_fused_typed', {'rs': 9}, INV, 'row stride 9 overlaps rows of width 10'),
    ('dcp_remap_coords_typed', {'src': None}, INV, 'null image pointer'),
    ('dcp_remap_coords_typed', {'dst': None}, INV, 'null image pointer'),
    ('dcp_remap_coords_typed', {'dtype': 99}, INV, 'unknown element type 99'),
    ('dcp_remap_coords_typed', {'height': 0}, INV, 'image must be non-empty (got 0 x 10)'),
    ('dcp_remap_coords_typed', {'height': -1}, INV, 'image must be non-empty (got -1 x 10)'),
    ('dcp_remap_coords_typed', {'width': 0}, INV, 'image must be non-empty (got 8 x 0)'),
    ('dcp_remap_coords_typed', {'rs': 0}, INV, 'strides must be positive (row 0, col 1)'),
    ('dcp_remap_coords_typed', {'cs': 0}, INV, 'strides must be positive (row 10, col 0)'),
    ('dcp_remap_coords_typed', {'y': None}, INV, 'null coordinate pointer'),
    ('dcp_remap_coords_typed', {'x': None}, INV, 'null coordinate pointer'),
    ('dcp_remap_coords_typed', {'coord_dtype': 5}, INV, 'unknown coord_dtype 5'),
    ('dcp_remap_coords_typed', {'npts': -1}, INV, 'npts < 0'),
    ('dcp_remap_coords_typed', {'order': 7}, INV, 'spline order 7 outside [0, 5]'),
    ('dcp_remap_coords_typed', {'order': -1}, INV, 'spline order -1 outside [0, 5]'),
    ('dcp_remap_coords_typed', {'mode': 9}, INV, 'unknown boundary mode 9'),
    ('dcp_remap_coords_typed', {'mode': -1}, INV, 'unknown boundary mode -1'),
    ('dcp_remap_coords_typed', {'mem_kind': 7}, INV, 'unknown mem_kind 7'),
    ('dcp_remap_coords_typed', {'mem_kind': 0x101}, INV, 'unknown mem_kind 257'),
    ('dcp_remap_coords_typed', {'rs': 9}, INV, 'row stride 9 overlaps rows of width 10'),
    ('dcp_remap_coords_typed', {'npts': 0, 'mem_kind': 7}, INV, 'unknown mem_kind 7'),  # was DCP_OK
    ('dcp_unwarp_image_channels', {'src': None}, INV, 'null image pointer'),
    ('dcp_unwarp_image_channels', {'dst': None}, INV, 'null image pointer'),
    ('dcp_unwarp_image_channels', {'dtype': 99}, INV, 'unknown element type 99'),
    ('dcp_unwarp_image_channels', {'height': 0}, INV, 'image must be non-empty (got 0 x 10)'),
    ('dcp_unwarp_image_channels', {'height': -1}, INV, 'image must be non-empty (got -1 x 10)'),
    ('dcp_unwarp_image_channels', {'width': 0}, INV, 'image must be non-empty (got 8 x 0)'),
    ('dcp_unwarp_image_channels', {'channels': 0}, INV, 'channels = 0 outside [1, 64]'),
    ('dcp_unwarp_image_channels', {'channels': 65}, INV, 'channels = 65 outside [1, 64]'),
    ('dcp_unwarp_image_channels', {'rs': 0}, INV, 'strides must be positive (row 0, col 3)'),
    ('dcp_unwarp_image_channels', {'cs': 0}, INV, 'pixel stride 0 smaller than 3 channels'),
    ('dcp_unwarp_image_channels', {'fact': None}, INV, 'null coefficient pointer'),
    ('dcp_unwarp_image_channels', {'nfact': 33}, INV, 'nfact = 33 outside [0, 32] (DCP_MAX_FACT is a li'),
    ('dcp_unwarp_image_channels', {'nfact': -1}, INV, 'nfact = -1 outside [0, 32] (DCP_MAX_FACT is a li'),
    ('dcp_unwarp_image_channels', {'order': 7}, UNS, 'the interleaved-channel kernels take orders 0 an'),
    ('dcp_unwarp_image_channels', {'order': -1}, UNS, 'the interleaved-channel kernels take orders 0 an'),
    ('dcp_unwarp_image_channels', {'order': 2}, UNS, 'the interleaved-channel kernels take orders 0 an'),
    ('dcp_unwarp_image_channels', {'mem_kind': 7}, INV, 'unknown mem_kind 7'),
    ('dcp_unwarp_image_channels', {'mem_kind': 0x101}, INV, 'unknown mem_kind 257'),
    ('dcp_unwarp_image_channels', {'rs': 29}, INV, 'row stride 29 overlaps rows of 10 pixels'),
    ('dcp_unwarp_color_image', {'src': None}, INV, 'null image pointer'),
    ('dcp_unwarp_color_image', {'dst': None}, INV, 'null image pointer'),
    ('dcp_unwarp_color_image', {'dtype': 99}, INV, 'unknown element type 99'),
    ('dcp_unwarp_color_image', {'height': 0}, INV, 'image must be non-empty (got 0 x 10)'),
    ('dcp_unwarp_color_image', {'height': -1}, INV, 'image must be non-empty (got -1 x 10)'),
    ('dcp_unwarp_color_image', {'width': 0}, INV, 'image must be non-empty (got 8 x 0)'),
    ('dcp_unwarp_color_image', {'channels': 0}, INV, 'channels = 0 outside [1, 64]'),
    ('dcp_unwarp_color_image', {'channels': 65}, INV, 'channels = 65 outside [1, 64]'),
    ('dcp_unwarp_color_image', {'rs': 0}, INV, 'strides must be positive (row 0, col 3)'),
    ('dcp_unwarp_color_image', {'cs': 0}, INV, 'pixel stride 0 smaller than 3 channels'),
    ('dcp_unwarp_color_image', {'fact': None}, INV, 'null coefficient pointer'),
    ('dcp_unwarp_color_image', {'nfact': 33}, INV, 'nfact = 33 outside [0, 32] (DCP_MAX_FACT is a li'),
    ('dcp_unwarp_color_image', {'nfact': -1}, INV, 'nfact = -1 outside [0, 32] (DCP_MAX_FACT is a li'),
    ('dcp_unwarp_color_image', {'order': 7}, UNS, 'the interleaved-channel kernels take orders 0 an'),
    ('dcp_unwarp_color_image', {'order': -1}, UNS, 'the interleaved-channel kernels take orders 0 an'),
    ('dcp_unwarp_color_image', {'order': 2}, UNS, 'the interleaved-channel kernels take orders 0 an'),
    ('dcp_unwarp_color_image', {'blend': 9}, UNS, 'interleaved channels blend as scipy does (DCP_BL'),
    ('dcp_unwarp_color_image', {'mem_kind': 7}, INV, 'unknown mem_kind 7'),
    ('dcp_unwarp_color_image', {'mem_kind': 0x101}, INV, 'unknown mem_kind 257'),
    ('dcp_unwarp_color_image', {'rs': 29}, INV, 'row stride 29 overlaps rows of 10 pixels'),
    ('dcp_map_points_f64', {'y': None}, INV, 'null point pointer'),
    ('dcp_map_points_f64', {'x': None}, INV, 'null point pointer'),
    ('dcp_map_points_f64', {'npts': -1}, INV, 'npts < 0'),
    ('dcp_map_points_f64', {'fact': None}, INV, 'null coefficient pointer'),
    ('dcp_map_points_f64', {'nfact': 33}, INV, 'nfact = 33 outside [0, 32] (DCP_MAX_FACT is a li'),
    ('dcp_map_points_f64', {'nfact': -1}, INV, 'nfact = -1 outside [0, 32] (DCP_MAX_FACT is a li'),
    ('dcp_map_points_f64', {'mem_kind': 7}, INV, 'unknown mem_kind 7'),
    ('dcp_map_points_f64', {'mem_kind': 0x101}, INV, 'unknown mem_kind 257'),
    ('dcp_map_points_f64', {'npts': 0, 'mem_kind': 7}, INV, 'unknown mem_kind 7'),  # was DCP_OK
    ('dcp_map_points_perspective_f64', {'y': None}, INV, 'null point pointer'),
    ('dcp_map_points_perspective_f64', {'x': None}, INV, 'null point pointer'),
    ('dcp_map_points_perspective_f64', {'npts': -1}, INV, 'npts < 0'),
    ('dcp_map_points_perspective_f64', {'coef': None}, INV, 'null homography pointer'),
    ('dcp_map_points_perspective_f64', {'mem_kind': 7}, INV, 'unknown mem_kind 7'),
    ('dcp_map_points_perspective_f64', {'mem_kind': 0x101}, INV, 'unknown mem_kind 257'),
    ('dcp_map_points_perspective_f64', {'npts': 0, 'mem_kind': 7}, INV, 'unknown mem_kind 7'),  # was DCP_OK
    ('dcp_coordinate_map_f32', {'src': None}, INV, 'null map pointer'),
    ('dcp_coordinate_map_f32', {'dst': None}, INV, 'null map pointer'),
    ('dcp_coordinate_map_f32', {'height': 0}, INV, 'map must be non-empty (got 0 x 10)'),
    ('dcp_coordinate_map_f32', {'height': -1}, INV, 'map must be non-empty (got -1 x 10)'),
    ('dcp_coordinate_map_f32', {'width': 0}, INV, 'map must be non-empty (got 8 x 0)'),
    ('dcp_coordinate_map_f32', {'map_kind': 5}, INV, 'unknown map_kind 5'),
    ('dcp_coordinate_map_f32', {'fact': None}, INV, 'null coefficient pointer'),
    ('dcp_coordinate_map_f32', {'nfact': 33}, INV, 'nfact = 33 outside [0, 32] (DCP_MAX_FACT is a li'),
    ('dcp_coordinate_map_f32', {'nfact': -1}, INV, 'nfact = -1 outside [0, 32] (DCP_MAX_FACT is a li'),
    ('dcp_coordinate_map_f32', {'coef': None}, INV, 'null homography pointer'),
    ('dcp_coordinate_map_f32', {'mem_kind': 7}, INV, 'unknown mem_kind 7'),
    ('dcp_coordinate_map_f32', {'mem_kind': 0x101}, INV, 'unknown mem_kind 257'),
    ('dcp_unwarp_image_spline_f32', {'src': None}, INV, 'null image pointer'),
    ('dcp_unwarp_image_spline_f32', {'dst': None}, INV, 'null image pointer'),
    ('dcp_unwarp_image_spline_f32', {'height': 0}, INV, 'image must be non-empty (got 0 x 10)'),
    ('dcp_unwarp_image_spline_f32', {'height': -1}, INV, 'image must be non-empty (got -1 x 10)'),
    ('dcp_unwarp_image_spline_f32', {'width': 0}, INV, 'image must be non-empty (got 8 x 0)'),
    ('dcp_unwarp_image_spline_f32', {'rs': 0}, INV, 'strides must be positive (row 0, col 1)'),
    ('dcp_unwarp_image_spline_f32', {'cs': 0}, INV, 'strides must be positive (row 10, col 0)'),
    ('dcp_unwarp_image_spline_f32', {'fact': None}, INV, 'null coefficient pointer'),
    ('dcp_unwarp_image_spline_f32', {'nfact': 33}, INV, 'nfact = 33 outside [0, 32] (DCP_MAX_FACT is a li'),
    ('dcp_unwarp_image_spline_f32', {'nfact': -1}, INV, 'nfact = -1 outside [0, 32] (DCP_MAX_FACT is a li'),
    ('dcp_unwarp_image_spline_f32', {'order': 7}, INV, 'spline order 7 outside [2, 5]'),
    ('dcp_unwarp_image_spline_f32', {'order': -1}, INV, 'spline order -1 outside [2, 5]'),
    ('dcp_unwarp_image_spline_f32', {'mode': 9}, INV, 'unknown boundary mode 9'),
    ('dcp_unwarp_image_spline_f32', {'mode': -1}, INV, 'unknown boundary mode -1'),
    ('dcp_unwarp_image_spline_f32', {'mem_kind': 7}, INV, 'unknown mem_kind 7'),  # was DCP_ERR_HIP
    ('dcp_unwarp_image_spline_f32', {'mem_kind': 0x101}, INV, 'unknown mem_kind 257'),  # was DCP_ERR_HIP
    ('dcp_unwarp_image_spline_f32', {'rs': 9}, INV, 'row stride 9 overlaps rows of width 10'),
    ('dcp_perspective_image_spline_f32', {'src': None}, INV, 'null image pointer'),
    ('dcp_perspective_image_spline_f32', {'dst': None}, INV, 'null image pointer'),
    ('dcp_perspective_image_spline_f32', {'height': 0}, INV, 'image must be non-empty (got 0 x 10)'),
    ('dcp_perspective_image_spline_f32', {'height': -1}, INV, 'image must be non-empty (got -1 x 10)'),
    ('dcp_perspective_image_spline_f32', {'width': 0}, INV, 'image must be non-empty (got 8 x 0)'),
    ('dcp_perspective_image_spline_f32', {'rs': 0}, INV, 'strides must be positive (row 0, col 1)'),
    ('dcp_perspective_image_spline_f32', {'cs': 0}, INV, 'strides must be positive (row 10, col 0)'),
    ('dcp_perspective_image_spline_f32', {'coef': None}, INV, 'null homography pointer'),
    ('dcp_perspective_image_spline_f32', {'order': 7}, INV, 'spline order 7 outside [2, 5]'),
    ('dcp_perspective_image_spline_f32', {'order': -1}, INV, 'spline order -1 outside [2, 5]'),
    ('dcp_perspective_image_spline_f32', {'mode': 9}, INV, 'unknown boundary mode 9'),
    ('dcp_perspective_image_spline_f32', {'mode': -1}, INV, 'unknown boundary mode -1'),
    ('dcp_perspective_image_spline_f32', {'mem_kind': 7}, INV, 'unknown mem_kind 7'),  # was DCP_ERR_HIP
    ('dcp_perspective_image_spline_f32', {'mem_kind': 0x101}, INV, 'unknown mem_kind 257'),  # was DCP_ERR_HIP
    ('dcp_perspective_image_spline_f32', {'rs': 9}, INV, 'row stride 9 overlaps rows of width 10'),
    ('dcp_unwarp_fused_spline_f32', {'src': None}, INV, 'null image pointer'),
    ('dcp_unwarp_fused_spline_f32', {'dst': None}, INV, 'null image pointer'),
    ('dcp_unwarp_fused_spline_f32', {'height': 0}, INV, 'image must be non-empty (got 0 x 10)'),
    ('dcp_unwarp_fused_spline_f32', {'height': -1}, INV, 'image must be non-empty (got -1 x 10)'),
    ('dcp_unwarp_fused_spline_f32', {'width': 0}, INV, 'image must be non-empty (got 8 x 0)'),
    ('dcp_unwarp_fused_spline_f32', {'rs': 0}, INV, 'strides must be positive (row 0, col 1)'),
    ('dcp_unwarp_fused_spline_f32', {'cs': 0}, INV, 'strides must be positive (row 10, col 0)'),
    ('dcp_unwarp_fused_spline_f32', {'fact': None}, INV, 'null coefficient pointer'),
    ('dcp_unwarp_fused_spline_f32', {'nfact': 33}, INV, 'nfact = 33 outside [0, 32] (DCP_MAX_FACT is a li'),
    ('dcp_unwarp_fused_spline_f32', {'nfact': -1}, INV, 'nfact = -1 outside [0, 32] (DCP_MAX_FACT is a li'),
    ('dcp_unwarp_fused_spline_f32', {'coef': None}, INV, 'null homography pointer'),
    ('dcp_unwarp_fused_spline_f32', {'order': 7}, INV, 'spline order 7 outside [2, 5]'),
    ('dcp_unwarp_fused_spline_f32', {'order': -1}, INV, 'spline order -1 outside [2, 5]'),
    ('dcp_unwarp_fused_spline_f32', {'mode': 9}, INV, 'unknown boundary mode 9'),
    ('dcp_unwarp_fused_spline_f32', {'mode': -1}, INV, 'unknown boundary mode -1'),
    ('dcp_unwarp_fused_spline_f32', {'mem_kind': 7}, INV, 'unknown mem_kind 7'),  # was DCP_ERR_HIP
    ('dcp_unwarp_fused_spline_f32', {'mem_kind': 0x101}, INV, 'unknown mem_kind 257'),  # was DCP_ERR_HIP
    ('dcp_unwarp_fused_spline_f32', {'rs': 9}, INV, 'row stride 9 overlaps rows of width 10'),
    ('dcp_remap_coords_spline_f32', {'src': None}, INV, 'null image pointer'),
    ('dcp_remap_coords_spline_f32', {'dst': None}, INV, 'null image pointer'),
    ('dcp_remap_coords_spline_f32', {'height': 0}, INV, 'image must be non-empty (got 0 x 10)'),
    ('dcp_remap_coords_spline_f32', {'height': -1}, INV, 'image must be non-empty (got -1 x 10)'),
    ('dcp_remap_coords_spline_f32', {'width': 0}, INV, 'image must be non-empty (got 8 x 0)'),
    ('dcp_remap_coords_spline_f32', {'rs': 0}, INV, 'strides must be positive (row 0, col 1)'),
    ('dcp_remap_coords_spline_f32', {'cs': 0}, INV, 'strides must be positive (row 10, col 0)'),
    ('dcp_remap_coords_spline_f32', {'y': None}, INV, 'null coordinate pointer'),
    ('dcp_remap_coords_spline_f32', {'x': None}, INV, 'null coordinate pointer'),
    ('dcp_remap_coords_spline_f32', {'coord_dtype': 5}, INV, 'unknown coord_dtype 5'),
    ('dcp_remap_coords_spline_f32', {'npts': -1}, INV, 'npts < 0'),
    ('dcp_remap_coords_spline_f32', {'order': 7}, INV, 'spline order 7 outside [2, 5]'),
    ('dcp_remap_coords_spline_f32', {'order': -1}, INV, 'spline order -1 outside [2, 5]'),
    ('dcp_remap_coords_spline_f32', {'mode': 9}, INV, 'unknown boundary mode 9'),
    ('dcp_remap_coords_spline_f32', {'mode': -1}, INV, 'unknown boundary mode -1'),
    ('dcp_remap_coords_spline_f32', {'mem_kind': 7}, INV, 'unknown mem_kind 7'),  # was DCP_ERR_HIP
    ('dcp_remap_coords_spline_f32', {'mem_kind': 0x101}, INV, 'unknown mem_kind 257'),  # was DCP_ERR_HIP
    ('dcp_remap_coords_spline_f32', {'rs': 9}, INV, 'row stride 9 overlaps rows of width 10'),
    ('dcp_remap_coords_spline_f32', {'npts': 0, 'mem_kind': 7}, INV, 'unknown mem_kind 7'),  # was DCP_OK
]


def call(name, **override):
    names, base = ENTRIES[name]
    args = dict(base, **override)
    return getattr(F.lib(), name)(*[args[k] for k in names.split()])


def test_every_frame_entry_point_is_covered():
    assert len(ENTRIES) == 19
    assert {c[0] for c in CASES} == set(ENTRIES)


@pytest.mark.parametrize("name,override,rc,fragment", CASES, ids=["%s-%s" % (c[0][4:], "-".join("%s=%s" % kv for kv in sorted(c[1].items())))
                                                                  for c in CASES])
def test_invalid_argument_is_refused(name, override, rc, fragment):
    got = call(name, **override)
    assert (got, fragment in F.last_error()) == (rc, True), (got, F.last_error())
