"""Colour / padded unwarp on the GPU path.

``unwarp_color_image_backward`` has the signature and semantics of the reference
(``/root/reference/discorpy/util/utility.py:278-342``): optional padding, then the backward radial
unwarp of every channel at the SAME float32 coordinates -- one launch on the interleaved image for
orders 0 / 1, one gather launch behind a prefilter per channel for orders 2..5 on up to four channels
(``dcp_unwarp_color_image_spline``), plane by plane through :mod:`discorpy_amd.post.postprocessing` otherwise.

``correct_perspective_color_image`` and ``unwarp_perspective_fused_color_image`` do the same for the homography and for the
one-pass perspective -> radial map: what the reference's demos write as a loop of ``post.correct_perspective_image`` over
``mat[:, :, i]`` (``examples/readthedocs_demo/demo_07.py:25,60``; ``demo_05.py:127,147``) is one call on the interleaved image.

``find_point_to_point`` is the closed-form point mapping of ``utility.py:192-230`` (host, NumPy);
``transform_coef_backward_and_forward`` the small least-squares model reversal ``pad=True`` needs
(``proc/processing.py:615-674``; host, NumPy -- the north star keeps the one-off fits on the CPU).
"""
import numpy as np

from ..post import postprocessing as _pp

__all__ = ["unwarp_color_image_backward", "find_point_to_point", "transform_coef_backward_and_forward",
           "correct_perspective_color_image", "unwarp_perspective_fused_color_image"]


def find_point_to_point(points, xcenter, ycenter, list_fact, output_order="xy"):
    """
    The radial model applied to ONE point (reference ``utility.py:192-230``): the point moves along its ray
    from the centre by the factor ``B(r) = sum_i list_fact[i] * r**i``.  With a forward model a distorted
    point goes to the undistorted space, with a backward model the other way.  ``points`` is
    ``(row_index, column_index)``; returns ``(x, y)``, or ``(y, x)`` for ``output_order="yx"``.
    """
    row, col = points[0], points[1]
    dx = col - xcenter
    dy = row - ycenter
    radius = np.sqrt(dx * dx + dy * dy)
    coefs = np.asarray(list_fact, dtype=np.float64)
    scale = np.float64(np.sum(coefs * radius ** np.arange(coefs.size)))
    moved = (xcenter + scale * dx, ycenter + scale * dy)
    return moved if output_order == "xy" else moved[::-1]


def transform_coef_backward_and_forward(list_fact, mapping="backward", ref_points=None):
    """
    Coefficients of the reversed radial model (reference ``proc/processing.py:615-674``, the one-off CPU fit the
    north star leaves on the host).  A model maps a radius ``r`` to ``r * F(r)``, ``F(r) = sum_i list_fact[i] r**i``;
    the reversed model ``G`` satisfies ``G(r F(r)) = 1 / F(r)``, and its coefficients are the least-squares solution
    of that identity over the radii of ``ref_points`` (``(y, x)`` offsets from the centre; a 40 x 40 grid of
    +-1000 px in steps of 50 when not given).  ``mapping`` only names which of the two directions ``list_fact``
    is -- the arithmetic is the same.  Points where ``F`` vanishes are left out.
    """
    coefs = np.asarray(list_fact, dtype=np.float64)
    if ref_points is None:
        ticks = np.arange(-1000, 1000, 50)
        pts = np.stack(np.meshgrid(ticks, ticks, indexing="ij"), axis=-1).reshape(-1, 2).astype(np.float64)
    else:
        if len(ref_points) < coefs.size:
            raise ValueError("Number of reference-points must be equal or "
                             "larger than the number of coefficients!!!")
        pts = np.asarray(ref_points, dtype=np.float64).reshape(-1, 2)
    if mapping not in ("backward", "forward"):
        raise ValueError("mapping must be 'backward' or 'forward'")
    expo = np.arange(coefs.size, dtype=np.int16)
    radius = np.sqrt(pts[:, 1] * pts[:, 1] + pts[:, 0] * pts[:, 0])
    scale = np.sum(coefs[None, :] * np.power(radius[:, None], expo[None, :]), axis=1)
    keep = scale != 0.0
    moved = scale[keep] * radius[keep]
    design = np.power(moved[:, None], expo[None, :])
    return np.linalg.lstsq(design, 1.0 / scale[keep], rcond=1e-64)[0]


def _auto_pad(height, width, xcenter, ycenter, list_fact):
    """pad=True (reference ``utility.py:238-263``): how far the four image corners land outside the frame once the
    forward model -- fitted from the backward one on a 40 x 40 grid over the frame -- is applied to them."""
    grid = [[gy - ycenter, gx - xcenter] for gy in np.linspace(0, height, 40) for gx in np.linspace(0, width, 40)]
    forward = transform_coef_backward_and_forward(list_fact, ref_points=grid)
    corners = {name: find_point_to_point(rc, xcenter, ycenter, forward)
               for name, rc in (("tl", (0, 0)), ("tr", (0, width - 1)), ("br", (height - 1, width - 1)),
                                ("bl", (height - 1, 0)))}
    left = min(corners["tl"][0], corners["bl"][0])
    right = max(corners["tr"][0], corners["br"][0])
    top = min(corners["tl"][1], corners["tr"][1])
    bottom = max(corners["bl"][1], corners["br"][1])
    return (int(-top) if top < 0 else 0, int(bottom - height) if bottom > height else 0,
            int(-left) if left < 0 else 0, int(right - width) if right > width else 0)


def _calc_pad(pad, height, width, xcenter, ycenter, list_fact):
    """(top, bottom, left, right) pad widths from the ``pad`` argument of the reference (``utility.py:233-275``):
    False -> none, True -> automatic, an int -> that width on every side, four values -> as given."""
    if isinstance(pad, bool):
        return _auto_pad(height, width, xcenter, ycenter, list_fact) if pad else (0, 0, 0, 0)
    if isinstance(pad, int):
        return (pad,) * 4
    if isinstance(pad, (tuple, list)):
        if len(pad) != 4:
            raise ValueError("Incorrect format!!! Please use a tuple/list of "
                             "(top_pad, bottom_pad, left_pad, right_pad)")
        return tuple(pad)
    raise ValueError("Invalid format of the 'pad' parameter!!!")


def _pad_device(t, pad_width, mode):
    """numpy.pad for a ROCm tensor: source indices come from numpy.pad on an index ramp, so the
    'edge', 'reflect', 'symmetric' and 'wrap' modes follow numpy's definition exactly."""
    import torch
    if all(p == (0, 0) for p in pad_width):
        return t
    if mode == "constant":
        out = torch.zeros([s + a + b for s, (a, b) in zip(t.shape, pad_width)], dtype=t.dtype, device=t.device)
        sl = tuple(slice(a, a + s) for s, (a, _) in zip(t.shape, pad_width))
        out[sl] = t
        return out
    if mode not in ("edge", "reflect", "symmetric", "wrap"):
        raise NotImplementedError("pad_mode %r is not implemented for device tensors (use a NumPy array, "
                                  "or one of constant/edge/reflect/symmetric/wrap)" % mode)
    for axis, (a, b) in enumerate(pad_width):
        if a or b:
            idx = np.pad(np.arange(t.shape[axis]), (a, b), mode=mode)
            t = t.index_select(axis, torch.as_tensor(idx, device=t.device))
    return t


def _interleaved_image(mat):
    """The (H, W, C) image as the interleaved-channel entry points address it -- unit channel stride, pixel stride >= C, rows that
    do not overlap --, after ONE contiguous copy where the layout is another; returns (image, row stride, pixel stride)."""
    img = _pp._Image(mat, 3)
    h, w, c = img.shape
    rs, ps, cs = img.strides
    if cs != 1 or ps < c or (h > 1 and rs < (w - 1) * ps + c):
        img = _pp._Image(img.keep.contiguous() if img.torch else np.ascontiguousarray(img.keep), 3)
        rs, ps, cs = img.strides
    return img, rs, ps


def _unwarp_interleaved(mat_pad, xcenter, ycenter, list_fact, order, blend=None):
    """(H, W, C) interleaved image in one launch of dcp_unwarp_color_image: one coordinate per pixel, C blends in the
    arithmetic `blend` names (the default of unwarp_image_backward when None; integer pixels always in scipy's exact order),
    no per-channel planes on the host.  3 / 4 channels of float32 / uint8 / uint16 under a certified calibration run
    remap_wg_color_kernel (the source box of a tile staged in LDS once for all channels)."""
    F = _pp.F
    img, rs, ps = _interleaved_image(mat_pad)
    h, w, c = img.shape
    fa, nf = F.fact_array(_pp._coefs(list_fact, "list_fact"))
    out, optr = img.empty((h, w, c))
    F.require_device()
    F.check(F.lib().dcp_unwarp_color_image(img.ptr, optr, img.code, h, w, c, rs, ps, float(xcenter), float(ycenter),
                                           fa, nf, order, _pp._blend_code(blend, img.mem == F.MEM_HOST), img.mem, img.device, img.stream))
    return out


def _homography_interleaved(mat, radial, list_coef, order, blend=None):
    """As _unwarp_interleaved under the homography `list_coef` (dcp_perspective_color_image) or, with radial = (xcenter, ycenter,
    list_fact), under the one-pass perspective -> radial map (dcp_unwarp_fused_color_image)."""
    F = _pp.F
    img, rs, ps = _interleaved_image(mat)
    h, w, c = img.shape
    ca, _ = F.fact_array(_pp._coefs(list_coef, "list_coef"))
    bcode = _pp._blend_code(blend, img.mem == F.MEM_HOST)
    if radial is not None:
        fa, nf = F.fact_array(_pp._coefs(radial[2], "list_fact"))
    out, optr = img.empty((h, w, c))
    F.require_device()
    if radial is None:
        F.check(F.lib().dcp_perspective_color_image(img.ptr, optr, img.code, h, w, c, rs, ps, ca, order, bcode, img.mem, img.device,
                                                    img.stream))
    else:
        F.check(F.lib().dcp_unwarp_fused_color_image(img.ptr, optr, img.code, h, w, c, rs, ps, float(radial[0]), float(radial[1]), fa, nf,
                                                     ca, order, bcode, img.mem, img.device, img.stream))
    return out


def _spline_interleaved(mat, radial, list_coef, order, mode, blend):
    """(H, W, C) interleaved image, C = 1..4, at spline orders 2..5 in one call: the single-plane prefilter once per channel, then
    one gather that evaluates a pixel's coordinate once for all its channels.  radial = (xcenter, ycenter, list_fact) or None,
    list_coef the homography or None: the radial map (dcp_unwarp_color_image_spline), the homography
    (dcp_perspective_color_image_spline) or the one-pass perspective -> radial map (dcp_unwarp_fused_color_image_spline).
    Every channel equals the single-plane function on ``mat[:, :, c]`` bit for bit."""
    F = _pp.F
    img, rs, ps = _interleaved_image(mat)
    h, w, c = img.shape
    mcode = _pp._spline_mode(mode, blend)
    if list_coef is not None:
        ca, _ = F.fact_array(_pp._coefs(list_coef, "list_coef"))
    if radial is not None:
        fa, nf = F.fact_array(_pp._coefs(radial[2], "list_fact"))
    out, optr = img.empty((h, w, c))
    F.require_device()
    if list_coef is None:
        F.check(F.lib().dcp_unwarp_color_image_spline(img.ptr, optr, img.code, h, w, c, rs, ps, float(radial[0]), float(radial[1]), fa, nf,
                                                      order, mcode, img.mem, img.device, img.stream))
    elif radial is None:
        F.check(F.lib().dcp_perspective_color_image_spline(img.ptr, optr, img.code, h, w, c, rs, ps, ca, order, mcode, img.mem, img.device,
                                                           img.stream))
    else:
        F.check(F.lib().dcp_unwarp_fused_color_image_spline(img.ptr, optr, img.code, h, w, c, rs, ps, float(radial[0]), float(radial[1]),
                                                            fa, nf, ca, order, mcode, img.mem, img.device, img.stream))
    return out


def _spline_one_call(order, channels):
    """Do the interleaved-channel spline entry points take this call?  Orders 2..5, 1 to 4 channels (and an image that is not empty:
    the single-plane functions keep their own answer to that)."""
    return 2 <= order <= 5 and 1 <= channels <= 4


def _one_launch(order, blend, channels):
    """Do the interleaved-channel entry points take this call?  Orders 0 / 1, scipy's blend or its one-ulp factorisation
    (names are case-insensitive), 1 to 64 channels."""
    return order <= 1 and (blend is None or str(blend).lower() in ("scipy", "exact", "f64lerp", "f64")) and 1 <= channels <= 64


def _plane_by_plane(mat, plane_call):
    """The reference's loop over mat[:, :, i] (demo_07.py:25,60): every channel through the single-plane function."""
    is_torch = _pp._is_torch(mat)
    if mat.shape[2] == 0:
        return mat.clone() if is_torch else np.array(mat)
    planes = [plane_call(mat[:, :, i]) for i in range(mat.shape[2])]
    if is_torch:
        import torch
        return torch.stack(planes, dim=2)
    return np.stack([np.asarray(p) for p in planes], axis=2)


def _complex_split(mat, call):
    """scipy interpolates a complex array as its real and imaginary parts: `call` on each, joined; None for real data."""
    parts = _pp._complex_parts(mat)
    if parts is None:
        return None
    dense = (lambda t: t.contiguous()) if _pp._is_torch(mat) else np.ascontiguousarray
    return parts[2](call(dense(parts[0])), call(dense(parts[1])))


def correct_perspective_color_image(mat, list_coef, order=1, mode="reflect", map_index=None, *, blend=None):
    """
    Apply perspective correction to a colour image: ``post.correct_perspective_image`` (reference
    ``postprocessing.py:462-492``) on every channel of an interleaved image, as the loop of
    ``examples/readthedocs_demo/demo_07.py:25,60`` does, at ONE evaluation of the coordinates of ``:444-459``.

    Parameters
    ----------
    mat : array_like
        2D/3D array (H, W) or (H, W, C); NumPy array or ROCm torch tensor.  A 2D array is handed to
        ``post.correct_perspective_image``.
    list_coef : list of floats
        Coefficients of the backward-mapping matrix (c1..c8, (x, y) convention).
    order : int, optional.
        The order of the spline interpolation (0..5); orders 2..5 take one call for up to four channels (a prefilter per
        channel, one gather), more channels and ``map_index=`` go plane by plane.
    mode : str, optional
        Boundary mode of scipy's spline interpolation; inert for order <= 1.
    map_index : array_like
        Indices for mapping, (ycoords, xcoords) with height*width points: every plane is remapped at them.

    Returns
    -------
    array_like
        Corrected image: the input's shape, element type and container.
    """
    if len(list_coef) != 8:
        raise ValueError("!!! Eight coefficients are required !!!")
    if len(mat.shape) == 2:
        return _pp.correct_perspective_image(mat, list_coef, order=order, mode=mode, map_index=map_index, blend=blend)
    order = _pp._check_order_mode(order, mode)
    res = _complex_split(mat, lambda part: correct_perspective_color_image(part, list_coef, order, mode, map_index, blend=blend))
    if res is not None:
        return res
    if map_index is None and _one_launch(order, blend, mat.shape[2]):
        return _homography_interleaved(mat, None, list_coef, order, blend)
    if map_index is None and _spline_one_call(order, mat.shape[2]) and mat.shape[0] > 0 and mat.shape[1] > 0:
        return _spline_interleaved(mat, None, list_coef, order, mode, blend)
    return _plane_by_plane(mat, lambda plane: _pp.correct_perspective_image(plane, list_coef, order=order, mode=mode,
                                                                            map_index=map_index, blend=blend))


def unwarp_perspective_fused_color_image(mat, xcenter, ycenter, list_fact, list_coef, order=1, mode="reflect", *, blend=None):
    """
    Perspective and radial correction of a colour image in ONE resampling: ``post.unwarp_perspective_fused`` on every
    channel of an interleaved image at one evaluation of the composed coordinates (the reference resamples twice,
    ``examples/readthedocs_demo/demo_05.py:127,147``; see there for the definition of the one-pass map).

    Parameters
    ----------
    mat : array_like
        2D/3D array (H, W) or (H, W, C); NumPy array or ROCm torch tensor.  A 2D array is handed to
        ``post.unwarp_perspective_fused``.
    xcenter, ycenter : float
        Center of distortion.
    list_fact : list of float
        Polynomial coefficients of the backward radial model.
    list_coef : list of floats
        Coefficients of the backward-mapping matrix (c1..c8, (x, y) convention).
    order : int, optional.
        The order of the spline interpolation (0..5); orders 2..5 take one call for up to four channels (a prefilter per
        channel, one gather), more channels go plane by plane.
    mode : str, optional
        Boundary mode of scipy's spline interpolation; inert for order <= 1.

    Returns
    -------
    array_like
        Corrected image: the input's shape, element type and container.
    """
    if len(list_coef) != 8:
        raise ValueError("!!! Eight coefficients are required !!!")
    if len(mat.shape) == 2:
        return _pp.unwarp_perspective_fused(mat, xcenter, ycenter, list_fact, list_coef, order=order, mode=mode, blend=blend)
    order = _pp._check_order_mode(order, mode)
    res = _complex_split(mat, lambda part: unwarp_perspective_fused_color_image(part, xcenter, ycenter, list_fact, list_coef, order,
                                                                                mode, blend=blend))
    if res is not None:
        return res
    if _one_launch(order, blend, mat.shape[2]):
        return _homography_interleaved(mat, (xcenter, ycenter, list_fact), list_coef, order, blend)
    if _spline_one_call(order, mat.shape[2]) and mat.shape[0] > 0 and mat.shape[1] > 0:
        return _spline_interleaved(mat, (xcenter, ycenter, list_fact), list_coef, order, mode, blend)
    return _plane_by_plane(mat, lambda plane: _pp.unwarp_perspective_fused(plane, xcenter, ycenter, list_fact, list_coef, order=order,
                                                                           mode=mode, blend=blend))


def unwarp_color_image_backward(mat, xcenter, ycenter, list_fact, order=1, mode="reflect", pad=False,
                                pad_mode='constant', *, blend=None):
    """
    Unwarp a color image using a backward model (reference ``utility.py:278-342``).

    Parameters
    ----------
    mat : array_like
        2D/3D array (H, W) or (H, W, C); NumPy array or ROCm torch tensor.
    xcenter, ycenter : float
        Center of distortion (of the UNPADDED image, as in the reference).
    list_fact : list of float
        Polynomial coefficients of the backward model.
    order : int, optional.
        The order of the spline interpolation (0..5); orders 2..5 take one call for up to four channels (a prefilter per
        channel, one gather), more channels go plane by plane.
    mode : str, optional
        Boundary mode of scipy's spline interpolation; inert for order <= 1.
    pad : bool, int, or tuple of int.
        Use to keep the original view.  ``True``: the width is calculated automatically.
    pad_mode : str
        numpy.pad mode ('constant', 'reflect', 'edge', 'mean', 'linear_ramp', 'symmetric', ...).

    Returns
    -------
    array_like
        2D/3D array. Distortion-corrected image, shape of the padded input.
    """
    (height, width) = mat.shape[:2]
    t_pad, b_pad, l_pad, r_pad = _calc_pad(pad, height, width, xcenter, ycenter, list_fact)
    num_dim = len(mat.shape)
    if num_dim == 2:
        pad_width = [(t_pad, b_pad), (l_pad, r_pad)]
    else:
        pad_width = [(t_pad, b_pad), (l_pad, r_pad), (0, 0)]
    is_torch = _pp._is_torch(mat) and mat.is_cuda
    if is_torch:
        mat_pad = _pad_device(mat, pad_width, pad_mode)
    elif t_pad == b_pad == l_pad == r_pad == 0:
        mat_pad = np.asarray(mat)                     # np.pad would copy the image for nothing
    else:
        mat_pad = np.pad(np.asarray(mat), pad_width, mode=pad_mode)
    xcenter = xcenter + l_pad
    ycenter = ycenter + t_pad
    if num_dim == 2:
        return _pp.unwarp_image_backward(mat_pad, xcenter, ycenter, list_fact, order=order, mode=mode, blend=blend)
    order = _pp._check_order_mode(order, mode)
    parts = _pp._complex_parts(mat_pad)
    if parts is not None:         # scipy interpolates a complex array as its real and imaginary parts
        dense = (lambda t: t.contiguous()) if is_torch else np.ascontiguousarray
        return parts[2](unwarp_color_image_backward(dense(parts[0]), xcenter, ycenter, list_fact, order, mode, blend=blend),
                        unwarp_color_image_backward(dense(parts[1]), xcenter, ycenter, list_fact, order, mode, blend=blend))
    # (`blend` names are case-insensitive everywhere, here too: "SciPy" must not fall to the plane-by-plane path -- ADVICE r4)
    if order <= 1 and (blend is None or str(blend).lower() in ("scipy", "exact", "f64lerp", "f64")) and 1 <= mat_pad.shape[2] <= 64:
        return _unwarp_interleaved(mat_pad, xcenter, ycenter, list_fact, order, blend)
    if _spline_one_call(order, mat_pad.shape[2]) and mat_pad.shape[0] > 0 and mat_pad.shape[1] > 0:
        return _spline_interleaved(mat_pad, (xcenter, ycenter, list_fact), None, order, mode, blend)
    # more than four channels at orders 2..5, other blends at orders 0 / 1: channels as dense planes through the batched entry point
    # (the reference's loop over mat_pad[:, :, i], utility.py:320-341): device-resident float32 planes at order 0 / 1 share ONE
    # launch, the other cases go plane by plane inside it
    # (at orders 2..5 the planes are handed over as a SEQUENCE: this route stays plane by plane, as it was before a 3-D array at a
    # spline order became one call of dcp_remap_frames_spline in post.unwarp_images_backward)
    if is_torch:
        planes = mat_pad.permute(2, 0, 1).contiguous()
        if order >= 2 and planes.shape[0] > 0:
            import torch
            out = torch.stack(_pp.unwarp_images_backward([planes[i] for i in range(planes.shape[0])], xcenter, ycenter, list_fact, order=order,
                                                         mode=mode, blend=blend))
        else:
            out = _pp.unwarp_images_backward(planes, xcenter, ycenter, list_fact, order=order, mode=mode, blend=blend)
        return out.permute(1, 2, 0)
    planes = np.ascontiguousarray(np.moveaxis(mat_pad, 2, 0))
    if order >= 2 and planes.shape[0] > 0:
        mat_corr = np.stack(_pp.unwarp_images_backward([planes[i] for i in range(planes.shape[0])], xcenter, ycenter, list_fact, order=order,
                                                       mode=mode, blend=blend))
    else:
        mat_corr = _pp.unwarp_images_backward(planes, xcenter, ycenter, list_fact, order=order, mode=mode, blend=blend)
    return np.moveaxis(np.asarray(mat_corr), 0, 2)
