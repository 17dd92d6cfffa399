"""3-D binary morphology on the device (csrc/morph.hip through hv_morph_ball / hv_morph_struct / hv_morph_merge).

The generator writes a vertebra label one 2-D slice at a time, so across slices the label shows one-voxel gaps, slits and thin bridges to the
neighbouring vertebra.  A closing (and an opening for the bridges) with a ball given in millimetres mends them before the component rules of
components.py run.  The definitions are scipy.ndimage.binary_dilation / binary_erosion / binary_opening / binary_closing, bit for bit, on
volumes that stay resident:
  ball(radius, spacing)                                          the structuring element as a numpy bool array
  binary_dilation / binary_erosion / binary_opening / binary_closing(vol, value=None, radius=None, spacing=(1, 1, 1), connectivity=None,
      iterations=1, border_value=0, out=None)                    -> a uint8 mask (0 / 1) on the device
  close_label / open_label(vol, value, radius, spacing=(1, 1, 1), background=0, fill=0, out=None)
                                                                 the operation on vol == value, written back into the label volume
Exactly one of radius (a ball, in the spacing's units) and connectivity (generate_binary_structure(3, c), `iterations` times) is given.
Volumes are 3-D with any strides, uint8 / float32 / float64 (bool masks become uint8, other dtypes float64), device tensors or numpy arrays
(uploaded).  Nothing is read back."""
import ctypes
import math

import numpy as np
import torch

from . import lib as _lib
from . import ops
from .components import _DT, _EQ, _NE, _check_connectivity, _check_value, _check_volume, _device, _ll, _out_for, _stored_dtype, _upload

DILATE, ERODE, OPEN, CLOSE = 0, 1, 2, 3                      # HV_MORPH_* of include/hvgan.h
GROW, SHRINK = 0, 1


def _check_radius(radius):
    if isinstance(radius, bool) or not isinstance(radius, (int, float, np.integer, np.floating)):
        raise ValueError('radius: a non-negative number expected, got %r' % (radius,))
    r = float(radius)
    if not (math.isfinite(r) and r >= 0.0 and math.isfinite(r * r)):
        raise ValueError('radius: a non-negative finite number expected, got %r' % (radius,))
    return r


def _check_spacing(spacing):
    if isinstance(spacing, (int, float, np.integer, np.floating)) and not isinstance(spacing, bool):
        spacing = (spacing,) * 3
    try:
        sp = tuple(float(s) for s in spacing)
    except (TypeError, ValueError):
        sp = ()
    if len(sp) != 3 or not all(math.isfinite(s) and s > 0.0 for s in sp):
        raise ValueError('spacing: three positive finite numbers expected, got %r' % (spacing,))
    return sp


def ball(radius, spacing=(1, 1, 1)):
    """The structuring element of the radius-given operations: the integer offsets o with ((s0 o0)^2 + (s1 o1)^2) + (s2 o2)^2 <= radius *
    radius, float64 in this order, as a numpy bool array of odd extents centred on the origin (radius 0: the origin alone)."""
    r = _check_radius(radius)
    sp = _check_spacing(spacing)
    r2 = np.float64(r) * np.float64(r)
    sq = []
    for s in sp:
        n = 0
        while (np.float64(s) * np.float64(n + 1)) * (np.float64(s) * np.float64(n + 1)) <= r2:
            n += 1
        t = np.float64(s) * np.arange(-n, n + 1, dtype=np.float64)
        sq.append(t * t)
    return ((sq[0][:, None, None] + sq[1][None, :, None]) + sq[2][None, None, :]) <= r2


def _check_border(border_value):
    if border_value not in (0, 1, False, True):
        raise ValueError('border_value: 0 or 1 expected, got %r' % (border_value,))
    return int(border_value)


def _check_iterations(iterations):
    if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or int(iterations) < 1:
        raise ValueError('iterations: an integer >= 1 expected (scipy\'s "until nothing changes" would need a readback per step), got %r'
                         % (iterations,))
    return int(iterations)


def _check_mask_out(out, meta):
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != tuple(meta.shape)):
        raise ValueError('out: a uint8 tensor of shape %s expected' % (tuple(meta.shape),))


def _element(radius, spacing, connectivity, iterations):
    """-> ('ball', radius, spacing) or ('struct', connectivity, iterations), checked."""
    if (radius is None) == (connectivity is None):
        raise ValueError('exactly one of radius (a ball) and connectivity (generate_binary_structure(3, c)) must be given')
    if radius is not None:
        if iterations != 1:
            raise ValueError('iterations applies to connectivity only (a ball is applied once), got %r' % (iterations,))
        return 'ball', _check_radius(radius), _check_spacing(spacing)
    return 'struct', _check_connectivity(connectivity), _check_iterations(iterations)


def _launch(op, v, val, mode, elem, border, out):
    """Queue one hv_morph_ball / hv_morph_struct on the current stream: the mask of `op` on the device volume v into the uint8 tensor out."""
    L = _lib.get()
    A = tuple(int(s) for s in v.shape)
    if elem[0] == 'ball':
        csp = (ctypes.c_double * 3)(*elem[2])
        ws, wsz = ops._ws(L.size('hv_morph_workspace_bytes', *A, ctypes.c_double(elem[1]), csp), v.device, slot=3)
        L.call('hv_morph_ball', _lib.ptr(v), _DT[v.dtype], *_ll(v.stride()), *A, ctypes.c_double(val), mode, op, ctypes.c_double(elem[1]), csp,
               border, _lib.ptr(out), *_ll(out.stride()), _lib.ptr(ws), wsz, _lib.stream())
    else:
        ws, wsz = ops._ws(L.size('hv_morph_workspace_bytes', *A, ctypes.c_double(0.0), None), v.device, slot=3)
        L.call('hv_morph_struct', _lib.ptr(v), _DT[v.dtype], *_ll(v.stride()), *A, ctypes.c_double(val), mode, op, elem[1], elem[2], border,
               _lib.ptr(out), *_ll(out.stride()), _lib.ptr(ws), wsz, _lib.stream())
    return out


def _mask_op(op, vol, value, radius, spacing, connectivity, iterations, border_value, out):
    meta = _check_volume(vol)
    val = 0.0 if value is None else _check_value(value)
    elem = _element(radius, spacing, connectivity, iterations)
    border = _check_border(border_value)
    _check_mask_out(out, meta)
    dev = _device(vol, out)
    v = _upload(vol, dev)
    _lib.require_gpu(out)
    if out is None:
        out = torch.empty(tuple(v.shape), dtype=torch.uint8, device=dev)
    elif out.data_ptr() == v.data_ptr():
        raise ValueError('out: a tensor that does not share the input\'s memory expected')
    return _launch(op, v, val, _NE if value is None else _EQ, elem, border, out)


def binary_dilation(vol, value=None, radius=None, spacing=(1, 1, 1), connectivity=None, iterations=1, border_value=0, out=None):
    """scipy.ndimage.binary_dilation(vol == value, ball(radius, spacing), border_value=...) -- or (vol != 0 for value=None;
    generate_binary_structure(3, connectivity), iterations=... with connectivity) -- as a uint8 device mask."""
    return _mask_op(DILATE, vol, value, radius, spacing, connectivity, iterations, border_value, out)


def binary_erosion(vol, value=None, radius=None, spacing=(1, 1, 1), connectivity=None, iterations=1, border_value=0, out=None):
    """scipy.ndimage.binary_erosion with the same arguments as binary_dilation."""
    return _mask_op(ERODE, vol, value, radius, spacing, connectivity, iterations, border_value, out)


def binary_opening(vol, value=None, radius=None, spacing=(1, 1, 1), connectivity=None, iterations=1, border_value=0, out=None):
    """scipy.ndimage.binary_opening: the erosion (`iterations` times), then the dilation (`iterations` times), both with border_value."""
    return _mask_op(OPEN, vol, value, radius, spacing, connectivity, iterations, border_value, out)


def binary_closing(vol, value=None, radius=None, spacing=(1, 1, 1), connectivity=None, iterations=1, border_value=0, out=None):
    """scipy.ndimage.binary_closing: the dilation, then the erosion, both with border_value."""
    return _mask_op(CLOSE, vol, value, radius, spacing, connectivity, iterations, border_value, out)


def _check_label_args(vol, value, radius, spacing, background, fill, out):
    meta = _check_volume(vol)
    dtype = _stored_dtype(meta)
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != dtype or tuple(out.shape) != tuple(meta.shape)):
        raise ValueError('out: a %s tensor of shape %s expected' % (str(dtype).replace('torch.', ''), tuple(meta.shape)))
    return (_check_value(value), _check_radius(radius), _check_spacing(spacing), _check_value(background, 'background'),
            _check_value(fill, 'fill'))


def _label_op(op, v, val, radius, sp, background, fill, out):
    """The opening / closing of v == val with the ball (border_value 0), merged into `out` (v itself: in place) by the shrink / grow rule.
    v and out are device tensors; everything is queued on the current stream."""
    mask = torch.empty(tuple(v.shape), dtype=torch.uint8, device=v.device)
    _launch(op, v, val, _EQ, ('ball', radius, sp), 0, mask)
    A = tuple(int(s) for s in v.shape)
    _lib.get().call('hv_morph_merge', _lib.ptr(v), _DT[v.dtype], *_ll(v.stride()), *A, _lib.ptr(mask), *_ll(mask.stride()),
                    GROW if op == CLOSE else SHRINK, ctypes.c_double(val), ctypes.c_double(background), ctypes.c_double(fill), _lib.ptr(out),
                    *_ll(out.stride()), _lib.stream())
    return out


def close_label(vol, value, radius, spacing=(1, 1, 1), background=0, fill=0, out=None):
    """The closing of vol == value by ball(radius, spacing) (border_value 0) written back into the label volume: a voxel of the closing that
    holds `background` becomes `value`; every other voxel -- other labels, and the label's own voxels the closing loses at the volume's faces
    -- is copied.  -> the device volume in the volume's dtype (`out`: a device tensor of that dtype and shape, `vol` itself for in place)."""
    val, r, sp, bg, fl = _check_label_args(vol, value, radius, spacing, background, fill, out)
    v = _upload(vol, _device(vol, out))
    return _label_op(CLOSE, v, val, r, sp, bg, fl, _out_for(v, out))


def open_label(vol, value, radius, spacing=(1, 1, 1), background=0, fill=0, out=None):
    """The opening of vol == value by ball(radius, spacing) (border_value 0) written back: a voxel that holds `value` and is not in the
    opening becomes `fill`; every other voxel is copied.  Arguments and result as close_label."""
    val, r, sp, bg, fl = _check_label_args(vol, value, radius, spacing, background, fill, out)
    v = _upload(vol, _device(vol, out))
    return _label_op(OPEN, v, val, r, sp, bg, fl, _out_for(v, out))
