"""3-D affine resampling of resident volumes (csrc/resample.hip through hv_resample).

A scan and its label are brought to the spacing a model was trained at (0.3 x 0.3 x 5 mm next to 1 mm isotropic) and carried back, a
synthesized vertebra is aligned rigidly with the original, a resident training volume gets a small rigid augmentation -- without a trip through
the host.  The definitions are scipy.ndimage's, on volumes that stay resident:
  affine_transform(vol, matrix, offset=0.0, output_shape=None, output=None, order=3, mode='constant', cval=0.0, prefilter=True)
  zoom(vol, zoom, output=None, order=3, mode='constant', cval=0.0, prefilter=True)            grid_mode=False only
  shift(vol, shift, output=None, order=3, mode='constant', cval=0.0, prefilter=True)
  spline_filter(vol)                                             the order-3 coefficients (straighten.spline_coefficients)
  rigid_matrix(rotation, centre_in, centre_out)                  (matrix, offset) of a rotation about a centre              (host, no device)
  rigid_transform(vol, rotation, centre=None, output_shape=None, ...)
  resample_to_spacing(vol, spacing, new_spacing, order=3, mode='constant', cval=0.0)          -> (volume, plan)
  resample_label_to_spacing(label, spacing, new_spacing, mode='constant', cval=0)             order 0 -> (label, plan)
  resample_back(vol, plan, order=3, mode='constant', cval=0.0)   onto the original grid
  points_to_resampled(points, plan) / points_from_resampled(points, plan)                     centroid lists                (host, no device)
Volumes are 3-D device tensors with any strides (a permuted view or a sub-box passes as it lies: nothing is copied, except that order 3 makes
the float64 coefficient volume), uint8 / int16 / float32 / float64; bool becomes uint8, numpy arrays are uploaded, any other dtype is refused.
The result has the input's dtype, or output=torch.float64 (any of the four dtypes, or a tensor to write into).  Nothing is read back.

Orders 0, 1 and 3; mode 'constant' at every order and 'nearest' at order 0.  'nearest' at order 1 is refused because scipy's edge rule there is
not a clamp of the coordinate (the results differ in the last bit at edge voxels), at order 3 because scipy pre-pads by 12 voxels; 'mirror',
'reflect', 'wrap' and 'grid-*' are not offered.  cval must be a value of an integer output dtype.  rotate() is not offered: scipy rotates a
3-D array plane by plane with a 2-D prefilter, which a 3-D order-3 path cannot reproduce; rigid_transform takes a rotation matrix instead.

The bytes are scipy's for orders 0 and 1 and for the order-3 sample of given coefficients (prefilter=False).  The order-3 prefilter is
hv_spline_prefilter, within SPLINE_TOL of scipy's (row f8), so a float64 order-3 result is scipy's to that tolerance; the rounding of a uint8 /
int16 / float32 output absorbs it on CT-like data."""
import ctypes
import math

import numpy as np
import torch

from . import lib as _lib
from .components import _check_value, _check_volume, _device, _ll
from .filters import _overlaps

_DT = {torch.uint8: 0, torch.int16: 1, torch.float32: 4, torch.float64: 5}      # HV_DT_* of include/hvgan.h
_NP_DT = {np.dtype(np.uint8): torch.uint8, np.dtype(np.int16): torch.int16, np.dtype(np.float32): torch.float32,
          np.dtype(np.float64): torch.float64}
MODES = {'constant': 1, 'nearest': 2}                                            # HV_FILT_* of the modes offered
_REFUSED_MODES = ('reflect', 'mirror', 'wrap', 'grid-constant', 'grid-mirror', 'grid-wrap')
MATRIX, ZOOMSHIFT = 0, 1                                                         # HV_RESAMPLE_*
ORDERS = (0, 1, 3)


# ------------------------------------------------------------------------------------------------ host: checks
def _check_order_mode(order, mode):
    if isinstance(order, bool) or not isinstance(order, (int, np.integer)) or int(order) not in ORDERS:
        raise ValueError('order: 0, 1 or 3 expected, got %r' % (order,))
    order = int(order)
    if mode in _REFUSED_MODES:
        raise ValueError('mode %r is not offered: constant (any order) or nearest (order 0)' % (mode,))
    if mode not in MODES:
        raise ValueError('mode: constant or nearest expected, got %r' % (mode,))
    if mode == 'nearest' and order != 0:
        raise ValueError('mode nearest is offered at order 0 only: at order 1 scipy\'s edge rule is not a clamp of the coordinate, at order 3 '
                         'it pre-pads the volume by 12 voxels')
    return order, MODES[mode]


def _check_cval(cval, dtype):
    c = _check_value(cval, 'cval')
    ok = math.isfinite(c)
    if ok and dtype in (torch.uint8, torch.int16):
        lo, hi = (0, 255) if dtype == torch.uint8 else (-32768, 32767)
        ok = c == math.floor(c) and lo <= c <= hi
    if not ok:
        raise ValueError('cval: a finite number, and a value of an integer output dtype (%s), expected, got %r'
                         % (str(dtype).replace('torch.', ''), cval))
    return c


def _vector(v, name, scalar_ok=True):
    a = np.asarray(v, dtype=np.float64)
    if a.ndim == 0 and scalar_ok:
        a = np.full(3, float(a))
    if a.shape != (3,):
        raise ValueError('%s: %sthree numbers expected, got shape %s' % (name, 'a number or ' if scalar_ok else '', a.shape))
    if not np.isfinite(a).all():
        raise ValueError('%s: finite numbers expected, got %r' % (name, v))
    return a


def _check_shape(shape, name):
    s = tuple(shape)
    if len(s) != 3 or any(isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1 for n in s):
        raise ValueError('%s: three positive integers expected, got %r' % (name, shape))
    return tuple(int(n) for n in s)


def _upload(vol, dev):
    t = torch.as_tensor(vol)
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    if t.dtype not in _DT:
        raise TypeError('resample: a uint8 / int16 / float32 / float64 (or bool) volume expected, got %s' % (t.dtype,))
    t = t.to(dev)
    _lib.require_gpu(t)
    return t


def _out_dtype(output, v):
    """-> (dtype, tensor or None) of the `output` argument: None, a dtype (torch or numpy) or a device tensor."""
    if output is None:
        return v.dtype, None
    if isinstance(output, torch.Tensor):
        if output.dtype not in _DT:
            raise TypeError('output: a uint8 / int16 / float32 / float64 tensor expected, got %s' % (output.dtype,))
        return output.dtype, output
    dt = output if isinstance(output, torch.dtype) else _NP_DT.get(np.dtype(output))
    if dt not in _DT:
        raise TypeError('output: uint8, int16, float32 or float64 expected, got %r' % (output,))
    return dt, None


# ------------------------------------------------------------------------------------------------ the launch
def spline_filter(vol):
    """scipy.ndimage.spline_filter(vol, 3, mode='mirror') in float64: the coefficients order 3 samples (prefilter=False takes them)."""
    _check_volume(vol)
    v = _upload(vol, _device(vol))
    from .straighten import spline_coefficients
    return spline_coefficients(v.to(torch.int16) if v.dtype == torch.uint8 else v)


def _resample(vol, out_shape, form, a, b, output, order, mode, cval, prefilter):
    _check_volume(vol)
    order, m = _check_order_mode(order, mode)
    out_shape = _check_shape(out_shape, 'output_shape')
    meta = torch.as_tensor(vol) if not isinstance(vol, torch.Tensor) else vol
    if 0 in tuple(meta.shape):
        raise ValueError('resample: a non-empty volume expected, got shape %s' % (tuple(meta.shape),))
    v = _upload(vol, _device(vol, output if isinstance(output, torch.Tensor) else None))
    dtype, out = _out_dtype(output, v)
    c = _check_cval(cval, dtype)
    if max(v.numel(), out_shape[0] * out_shape[1] * out_shape[2]) > 2 ** 30:
        raise ValueError('resample: at most 2^30 voxels on either side are supported')
    if out is None:
        out = torch.empty(out_shape, dtype=dtype, device=v.device)
    else:
        if tuple(out.shape) != out_shape:
            raise ValueError('output: a tensor of shape %s expected, got %s' % (out_shape, tuple(out.shape)))
        _lib.require_gpu(out)
        if _overlaps(v, out):
            raise ValueError('output: a tensor that does not share the input\'s memory expected')
    src = v
    if order == 3:
        if prefilter:
            src = spline_filter(v)
        elif v.dtype != torch.float64:
            raise TypeError('prefilter=False at order 3: the float64 coefficients of spline_filter() expected, got %s' % (v.dtype,))
    L = _lib.get()
    d = L.hv_resample_desc()
    d.form, d.order, d.mode, d.cval = form, order, m, c
    mat, off = (a, b) if form == MATRIX else (np.eye(3), np.zeros(3))
    zm, sh = (a, b) if form == ZOOMSHIFT else (np.ones(3), np.zeros(3))
    for i, x in enumerate(np.asarray(mat, dtype=np.float64).reshape(9)):
        d.matrix[i] = float(x)
    for i in range(3):
        d.offset[i], d.zoom[i], d.shift[i] = float(off[i]), float(zm[i]), float(sh[i])
    with torch.cuda.device(v.device):
        L.call('hv_resample', _lib.ptr(src), _DT[src.dtype], *_ll(src.stride()), *(int(s) for s in src.shape), _lib.ptr(out), _DT[out.dtype],
               *_ll(out.stride()), *out_shape, ctypes.byref(d), _lib.stream())
    return out


# ------------------------------------------------------------------------------------------------ scipy's front ends
def affine_arguments(matrix, offset=0.0):
    """(form, a, b) of scipy.ndimage.affine_transform's matrix and offset for a 3-D input: a 3 x 3 matrix, a 3 x 4 / 4 x 4 homogeneous one
    (its last column is the offset, and `offset` is ignored, as in scipy), or a length-3 diagonal, which scipy runs as zoom_shift with zoom =
    matrix and shift = offset / matrix.  Host only."""
    m = np.asarray(matrix, dtype=np.float64)
    if not np.isfinite(m).all():
        raise ValueError('matrix: finite numbers expected')
    if m.ndim == 2 and m.shape in ((3, 4), (4, 4)):
        if m.shape == (4, 4) and not np.array_equal(m[3], (0.0, 0.0, 0.0, 1.0)):
            raise ValueError('matrix: the last row of a homogeneous matrix must be [0, 0, 0, 1]')
        return MATRIX, m[:3, :3].copy(), _vector(m[:3, 3], 'offset')
    off = _vector(offset, 'offset')
    if m.shape == (3,):
        if (m == 0.0).any():
            raise ValueError('matrix: a diagonal without zeros expected')
        return ZOOMSHIFT, m, _vector(off / m, 'offset / matrix')
    if m.shape != (3, 3):
        raise ValueError('matrix: shape (3, 3), (3, 4), (4, 4) or (3,) expected, got %s' % (m.shape,))
    return MATRIX, m, off


def affine_transform(vol, matrix, offset=0.0, output_shape=None, output=None, order=3, mode='constant', cval=0.0, prefilter=True):
    """scipy.ndimage.affine_transform(vol, matrix, offset, output_shape, output, order, mode, cval, prefilter) as a device volume: output voxel
    o reads the input at matrix @ o + offset."""
    form, a, b = affine_arguments(matrix, offset)
    meta = _check_volume(vol)
    shape = tuple(meta.shape) if output_shape is None else output_shape
    return _resample(vol, shape, form, a, b, output, order, mode, cval, prefilter)


def zoom_arguments(in_shape, zoom):
    """(output shape, step per axis) of scipy.ndimage.zoom(grid_mode=False): extents round(A * zoom), the end voxels on the end voxels -- step
    (A - 1) / (O - 1), and 1.0 where O == 1.  Host only."""
    z = _vector(zoom, 'zoom')
    out_shape = tuple(int(round(n * f)) for n, f in zip(in_shape, z))
    if min(out_shape) < 1:
        raise ValueError('zoom: the output shape %s has an empty axis' % (out_shape,))
    return out_shape, np.array([(n - 1) / (o - 1) if o != 1 else 1.0 for n, o in zip(in_shape, out_shape)])


def zoom(vol, zoom, output=None, order=3, mode='constant', cval=0.0, prefilter=True, grid_mode=False):
    """scipy.ndimage.zoom(vol, zoom, output, order, mode, cval, prefilter) as a device volume; grid_mode=True is not offered."""
    if grid_mode:
        raise ValueError('grid_mode=True is not offered')
    meta = _check_volume(vol)
    out_shape, step = zoom_arguments(tuple(meta.shape), zoom)
    return _resample(vol, out_shape, ZOOMSHIFT, step, np.zeros(3), output, order, mode, cval, prefilter)


def shift(vol, shift, output=None, order=3, mode='constant', cval=0.0, prefilter=True):
    """scipy.ndimage.shift(vol, shift, output, order, mode, cval, prefilter) as a device volume: output voxel o reads the input at o - shift."""
    meta = _check_volume(vol)
    s = _vector(shift, 'shift')
    return _resample(vol, tuple(meta.shape), ZOOMSHIFT, np.ones(3), -s, output, order, mode, cval, prefilter)


# ------------------------------------------------------------------------------------------------ rigid transforms
def rigid_matrix(rotation, centre_in, centre_out):
    """(matrix, offset) for affine_transform of the rigid motion that turns the volume's content by `rotation` (3 x 3, orthonormal, acting on
    voxel index vectors) about the point centre_in and puts that point at centre_out of the output: an output voxel o reads the input at
    rotation^T (o - centre_out) + centre_in, so matrix = rotation^T and offset = centre_in - rotation^T centre_out.  Host only."""
    r = np.asarray(rotation, dtype=np.float64)
    if r.shape != (3, 3) or not np.isfinite(r).all():
        raise ValueError('rotation: a finite 3 x 3 matrix expected')
    if np.abs(r @ r.T - np.eye(3)).max() > 1e-9:
        raise ValueError('rotation: an orthonormal matrix expected (|R R^T - I| <= 1e-9)')
    ci, co = _vector(centre_in, 'centre_in', False), _vector(centre_out, 'centre_out', False)
    m = r.T.copy()
    return m, ci - m @ co


def rigid_transform(vol, rotation, centre=None, output_shape=None, output=None, order=3, mode='constant', cval=0.0, prefilter=True):
    """The volume turned by `rotation` about `centre` (default: the middle of the volume, (A - 1) / 2).  With output_shape the centre lands in
    the middle of the output, otherwise where it was."""
    meta = _check_volume(vol)
    mid = (np.array(tuple(meta.shape), dtype=np.float64) - 1.0) / 2.0
    ci = mid if centre is None else _vector(centre, 'centre', False)
    co = ci if output_shape is None else (np.array(_check_shape(output_shape, 'output_shape'), dtype=np.float64) - 1.0) / 2.0
    m, off = rigid_matrix(rotation, ci, co)
    return affine_transform(vol, m, off, output_shape, output, order, mode, cval, prefilter)


# ------------------------------------------------------------------------------------------------ spacing
def spacing_plan(shape, spacing, new_spacing):
    """The plan of resample_to_spacing: both shapes, both spacings and the zoom-shift arguments in both directions.  The output extent is
    round(A * s / s_new) (at least 1) and the grid points lie at the end voxels, as in zoom().  Host only."""
    shape = _check_shape(shape, 'shape')
    s, n = _vector(spacing, 'spacing'), _vector(new_spacing, 'new_spacing')
    if (s <= 0).any() or (n <= 0).any():
        raise ValueError('spacing: positive numbers expected')
    out_shape = tuple(max(1, int(round(a * x / y))) for a, x, y in zip(shape, s, n))
    fwd = np.array([(a - 1) / (o - 1) if o != 1 else 1.0 for a, o in zip(shape, out_shape)])
    back = np.array([(o - 1) / (a - 1) if a != 1 else 1.0 for a, o in zip(shape, out_shape)])
    return {'shape': shape, 'new_shape': out_shape, 'spacing': tuple(s.tolist()), 'new_spacing': tuple(n.tolist()),
            'forward': {'zoom': fwd, 'shift': np.zeros(3)}, 'backward': {'zoom': back, 'shift': np.zeros(3)}}


def resample_to_spacing(vol, spacing, new_spacing, order=3, mode='constant', cval=0.0, output=None):
    """The volume on the grid of voxel size new_spacing -> (volume, plan); plan takes results back (resample_back) and maps points."""
    meta = _check_volume(vol)
    plan = spacing_plan(tuple(meta.shape), spacing, new_spacing)
    f = plan['forward']
    return _resample(vol, plan['new_shape'], ZOOMSHIFT, f['zoom'], f['shift'], output, order, mode, cval, True), plan


def resample_label_to_spacing(label, spacing, new_spacing, mode='constant', cval=0):
    """resample_to_spacing at order 0: every output voxel is one of the label's own values."""
    return resample_to_spacing(label, spacing, new_spacing, 0, mode, cval)


def resample_back(vol, plan, order=3, mode='constant', cval=0.0, output=None):
    """A volume on the plan's new grid resampled onto the original grid."""
    meta = _check_volume(vol)
    if tuple(meta.shape) != tuple(plan['new_shape']):
        raise ValueError('resample_back: a volume of shape %s expected, got %s' % (tuple(plan['new_shape']), tuple(meta.shape)))
    b = plan['backward']
    return _resample(vol, plan['shape'], ZOOMSHIFT, b['zoom'], b['shift'], output, order, mode, cval, True)


def points_to_resampled(points, plan):
    """Voxel coordinates [n][3] on the original grid -> on the new grid (the inverse of u = (o + shift) * zoom).  Host only."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    return p / plan['forward']['zoom'] - plan['forward']['shift']


def points_from_resampled(points, plan):
    """Voxel coordinates [n][3] on the new grid -> on the original grid.  Host only."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    return (p + plan['forward']['shift']) * plan['forward']['zoom']
