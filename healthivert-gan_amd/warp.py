"""Deformable 3-D resampling of resident volumes (csrc/warp.hip through hv_map_coordinates and hv_warp_grid).

A deformation field from a registration is applied to a resident CT and its label, and a training crop gets a smooth random (elastic)
deformation, CT and label alike, without a trip through the host and without dense float64 coordinates in memory:
  map_coordinates(vol, coordinates, output=None, order=3, mode='constant', cval=0.0, prefilter=True)       scipy.ndimage.map_coordinates
  warp(vol, displacement, spacing=None, order=1, output=None, mode='constant', cval=0.0, prefilter=True)   a dense displacement field
  ControlGrid(values, gzoom, gshift, gorder, out_shape)                                                    a coarse grid of displacements
  control_grid(values, out_shape, gorder=3)                      the grid spanning the output box end to end
  random_control_grid(out_shape, spacing, control_mm, amplitude_mm, seed, gorder=3, fix_border=True, clip=0.4)
  warp_grid(vol, grid, matrix=None, offset=0.0, output_shape=None, output=None, order=1, mode='constant', cval=0.0, prefilter=True)
  elastic_pair(ct, label, grid, ct_order=1, ct_cval=None, label_cval=0)                                    -> (ct, label), both resident
  displacement_of(grid)                                          the dense [3, *out_shape] float64 field a grid stands for (inspection)
Volumes, dtypes, `output=`, orders, modes, cval and prefilter are resample.py's: 3-D device tensors with any strides (numpy arrays are
uploaded), uint8 / int16 / float32 / float64; orders 0, 1 and 3; mode 'constant', and 'nearest' at order 0; at order 3 prefilter=True runs
hv_spline_prefilter first and prefilter=False takes the float64 coefficients.  Nothing is read back.

The control grid.  values[h] is the displacement along source axis h, in source voxels, at the control points.  Output voxel o looks the grid
up at q_a = (o_a + gshift[a]) * gzoom[a], clamped to [0, G_a - 1]; the displacement d_h there is the order-1 interpolation of values[h] or, at
gorder=3, the cubic B-spline with the control values as its coefficients (no prefilter: the approximating spline of free-form deformation,
Rueckert et al. 1999 -- smooth, local support, it does not pass through the control values); the volume is sampled at base(o) + d, base the
affine lattice of affine_transform (default: the identity).  The bytes are those of scipy.ndimage.map_coordinates at these coordinates
(tests/warp_ref.py restates them; tests/test_warp_ref_cpu.py pins the restatement to scipy)."""
import collections
import ctypes
import math

import numpy as np
import torch

from . import lib as _lib
from .components import _check_volume, _device, _ll
from .filters import _overlaps
from .resample import (_DT, _check_cval, _check_order_mode, _check_shape, _out_dtype, _upload, _vector, affine_arguments, spline_filter,
                       MATRIX, ZOOMSHIFT)

ABSOLUTE, DISPLACEMENT = 0, 1                                                    # HV_COORDS_*
_COORD_DT = {torch.float32: 4, torch.float64: 5}
GORDERS = (1, 3)

ControlGrid = collections.namedtuple('ControlGrid', 'values gzoom gshift gorder out_shape')
ControlGrid.__doc__ = """values: the resident [3, G0, G1, G2] float64 tensor; gzoom, gshift: three floats each; gorder: 1 or 3; out_shape: the
output shape the grid was made for (warp_grid's default output shape)."""


# ------------------------------------------------------------------------------------------------ host: checks
def _check_gorder(gorder):
    if isinstance(gorder, bool) or not isinstance(gorder, (int, np.integer)) or int(gorder) not in GORDERS:
        raise ValueError('gorder: 1 or 3 expected, got %r' % (gorder,))
    return int(gorder)


def _check_coordinates(coordinates, dev):
    """-> (device tensor [3, O0, O1, O2] float32 / float64 as it lies, the trailing shape the caller gave)."""
    c = torch.as_tensor(coordinates)
    if c.dim() < 2 or c.dim() > 4 or c.shape[0] != 3:
        raise ValueError('coordinates: shape [3, ...] with 1 to 3 trailing dimensions expected, got %s' % (tuple(c.shape),))
    if 0 in tuple(c.shape):
        raise ValueError('coordinates: a non-empty array expected, got shape %s' % (tuple(c.shape),))
    if c.dtype not in _COORD_DT:
        c = c.to(torch.float64)                                                  # scipy converts any other dtype to float64
    c = c.to(dev)
    _lib.require_gpu(c)
    trailing = tuple(int(n) for n in c.shape[1:])
    return c[(slice(None),) + (None,) * (4 - c.dim())], trailing


def _check_grid(grid):
    if not isinstance(grid, ControlGrid):
        raise ValueError('grid: a ControlGrid expected (control_grid() or random_control_grid()), got %r' % (type(grid).__name__,))
    v = grid.values
    if not isinstance(v, torch.Tensor) or v.dtype != torch.float64 or v.dim() != 4 or v.shape[0] != 3 or 0 in tuple(v.shape):
        raise ValueError('grid.values: a float64 tensor [3, G0, G1, G2] expected')
    _lib.require_gpu(v)
    return v, _vector(grid.gzoom, 'gzoom', False), _vector(grid.gshift, 'gshift', False), _check_gorder(grid.gorder)


def _prepare(vol, out_shape, output, order, mode, cval, prefilter, others=()):
    """resample.py's preparation of one launch: -> (the source the kernel reads, out, order, mode code, cval).  `others`: the device tensors
    the launch also reads, which `output` must not share memory with."""
    _check_volume(vol)
    order, m = _check_order_mode(order, mode)
    meta = torch.as_tensor(vol) if not isinstance(vol, torch.Tensor) else vol
    if 0 in tuple(meta.shape):
        raise ValueError('warp: a non-empty volume expected, got shape %s' % (tuple(meta.shape),))
    v = _upload(vol, _device(vol, output if isinstance(output, torch.Tensor) else None, *others))
    dtype, out = _out_dtype(output, v)
    c = _check_cval(cval, dtype)
    if max(v.numel(), out_shape[0] * out_shape[1] * out_shape[2]) > 2 ** 30:
        raise ValueError('warp: at most 2^30 voxels on either side are supported')
    if out is None:
        out = torch.empty(out_shape, dtype=dtype, device=v.device)
    else:
        if tuple(out.shape) != tuple(out_shape):
            raise ValueError('output: a tensor of shape %s expected, got %s' % (tuple(out_shape), tuple(out.shape)))
        _lib.require_gpu(out)
        if any(_overlaps(t, out) for t in (v,) + tuple(others)):
            raise ValueError('output: a tensor that shares no memory with the inputs expected')
    src = v
    if order == 3:
        if prefilter:
            src = spline_filter(v)
        elif v.dtype != torch.float64:
            raise TypeError('prefilter=False at order 3: the float64 coefficients of spline_filter() expected, got %s' % (v.dtype,))
    return src, out, order, m, c


def _box(t):
    return (_lib.ptr(t), _DT[t.dtype], *_ll(t.stride()), *(int(s) for s in t.shape))


# ------------------------------------------------------------------------------------------------ coordinates the caller supplies
def _map(vol, coordinates, kind, output, order, mode, cval, prefilter):
    dev = _device(vol, coordinates, output if isinstance(output, torch.Tensor) else None)
    c, trailing = _check_coordinates(coordinates, dev)
    out_shape = tuple(int(n) for n in c.shape[1:])
    given = output if isinstance(output, torch.Tensor) else None
    if given is not None:
        if tuple(output.shape) != trailing:
            raise ValueError('output: a tensor of shape %s expected, got %s' % (trailing, tuple(output.shape)))
        output = output[(None,) * (3 - output.dim())]
    src, out, order, m, cv = _prepare(vol, out_shape, output, order, mode, cval, prefilter, (c,))
    L = _lib.get()
    with torch.cuda.device(src.device):
        L.call('hv_map_coordinates', *_box(src), _lib.ptr(c), _COORD_DT[c.dtype], *_ll(c.stride()), kind, _lib.ptr(out), _DT[out.dtype],
               *_ll(out.stride()), *out_shape, order, m, cv, _lib.stream())
    return out.reshape(trailing) if given is None else given


def map_coordinates(vol, coordinates, output=None, order=3, mode='constant', cval=0.0, prefilter=True):
    """scipy.ndimage.map_coordinates(vol, coordinates, output, order, mode, cval, prefilter) as a device array: element p of the result is the
    volume at (coordinates[0][p], coordinates[1][p], coordinates[2][p]).  coordinates: [3, ...] with 1 to 3 trailing dimensions, float32 or
    float64 (anything else becomes float64, as in scipy), a host array or a device tensor with any strides -- a permuted view passes as it
    lies.  A NaN coordinate gives cval in mode 'constant'."""
    return _map(vol, coordinates, ABSOLUTE, output, order, mode, cval, prefilter)


def warp(vol, displacement, spacing=None, order=1, output=None, mode='constant', cval=0.0, prefilter=True):
    """The volume pulled back through a dense displacement field [3, *vol.shape]: output voxel o reads the input at o + displacement[:, o].
    The field is in voxels, or in millimetres when `spacing` (three voxel sizes) is given: it is then divided by the spacing once, on the
    device, in float64."""
    meta = _check_volume(vol)
    d = torch.as_tensor(displacement)
    if tuple(d.shape) != (3,) + tuple(meta.shape):
        raise ValueError('displacement: shape %s expected, got %s' % ((3,) + tuple(meta.shape), tuple(d.shape)))
    if spacing is not None:
        s = _vector(spacing, 'spacing')
        if (s <= 0).any():
            raise ValueError('spacing: positive numbers expected')
        d = d.to(_device(vol, d)).to(torch.float64)
        d = d / torch.tensor(s, dtype=torch.float64, device=d.device).view(3, 1, 1, 1)
    return _map(vol, d, DISPLACEMENT, output, order, mode, cval, prefilter)


# ------------------------------------------------------------------------------------------------ control grids
def control_grid(values, out_shape, gorder=3):
    """The ControlGrid of `values` [3, G0, G1, G2] (displacements in source voxels; a host array is uploaded as float64) whose control points
    span an output box of out_shape end to end: gzoom_a = (G_a - 1) / (O_a - 1), 1.0 where O_a == 1, and gshift = 0 -- zoom_arguments' rule."""
    out_shape = _check_shape(out_shape, 'out_shape')
    gorder = _check_gorder(gorder)
    v = torch.as_tensor(values)
    if v.dim() != 4 or v.shape[0] != 3 or 0 in tuple(v.shape):
        raise ValueError('values: shape [3, G0, G1, G2] expected, got %s' % (tuple(v.shape),))
    v = v.to(_device(values)).to(torch.float64)
    _lib.require_gpu(v)
    gzoom = tuple((int(g) - 1) / (o - 1) if o != 1 else 1.0 for g, o in zip(v.shape[1:], out_shape))
    return ControlGrid(v, gzoom, (0.0, 0.0, 0.0), gorder, out_shape)


def random_control_values(out_shape, spacing, control_mm, amplitude_mm, seed, fix_border=True, clip=0.4):
    """The host half of random_control_grid: -> float64 array [3, G0, G1, G2].  No device."""
    out_shape = _check_shape(out_shape, 'out_shape')
    s = _vector(spacing, 'spacing')
    for x, name in ((control_mm, 'control_mm'), (amplitude_mm, 'amplitude_mm'), (clip, 'clip')):
        if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)) or not math.isfinite(x) or x < 0:
            raise ValueError('%s: a non-negative finite number expected, got %r' % (name, x))
    if (s <= 0).any() or control_mm <= 0:
        raise ValueError('spacing, control_mm: positive numbers expected')
    G = tuple(max(2, int(math.ceil((o - 1) / (control_mm / s[a]))) + 1) if o != 1 else 1 for a, o in enumerate(out_shape))
    v = np.random.RandomState(seed).standard_normal((3,) + G)
    for h in range(3):
        delta = (out_shape[h] - 1) / (G[h] - 1) if G[h] != 1 else control_mm / s[h]      # the control spacing along axis h in voxels
        v[h] *= amplitude_mm / s[h]
        v[h] = np.clip(v[h], -clip * delta, clip * delta)
    if fix_border:
        for a in range(3):
            if G[a] != 1:
                idx = [slice(None)] * 4
                for end in (0, -1):
                    idx[a + 1] = end
                    v[tuple(idx)] = 0.0
    return v


def random_control_grid(out_shape, spacing, control_mm, amplitude_mm, seed, gorder=3, fix_border=True, clip=0.4, device=None):
    """A smooth random deformation for a box of out_shape voxels of size `spacing` (mm): control points at most control_mm apart, spanning the
    box end to end (extent ceil((O - 1) / (control_mm / spacing)) + 1, at least 2; 1 where O == 1).  The values are drawn on the host with
    numpy.random.RandomState(seed).standard_normal, so one seed gives one field on every machine; component h is scaled by amplitude_mm /
    spacing[h] (a standard deviation in voxels) and clipped to +-clip x the control spacing in voxels along axis h; fix_border zeroes the
    outermost control layer.  At gorder=3 the default clip of 0.4 lies just inside Choi and Lee's sufficient condition for an injective 3-D
    cubic B-spline deformation (displacements below about 0.403 of the control spacing), so the default cannot fold.  At gorder=1 the same
    clip is a bound on the slope of the piecewise-linear field (at most 2 x clip per component and axis), not that theorem."""
    gorder = _check_gorder(gorder)
    v = random_control_values(out_shape, spacing, control_mm, amplitude_mm, seed, fix_border, clip)
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else device
    return control_grid(torch.from_numpy(v).to(dev), out_shape, gorder)


def _warp_grid(vol, values, gzoom, gshift, gorder, form, a, b, out_shape, output, order, mode, cval, prefilter):
    src, out, order, m, c = _prepare(vol, out_shape, output, order, mode, cval, prefilter, (values,))
    L = _lib.get()
    d = L.hv_warp_desc()
    d.base.form, d.base.order, d.base.mode, d.base.cval = form, order, m, c
    mat, off = (a, b) if form == MATRIX else (np.eye(3), np.zeros(3))
    zm, sh = (a, b) if form == ZOOMSHIFT else (np.ones(3), np.zeros(3))
    for i, x in enumerate(np.asarray(mat, dtype=np.float64).reshape(9)):
        d.base.matrix[i] = float(x)
    for i in range(3):
        d.base.offset[i], d.base.zoom[i], d.base.shift[i] = float(off[i]), float(zm[i]), float(sh[i])
        d.gzoom[i], d.gshift[i] = float(gzoom[i]), float(gshift[i])
    d.gorder = gorder
    with torch.cuda.device(src.device):
        L.call('hv_warp_grid', *_box(src), _lib.ptr(values), *_ll(values.stride()), *(int(n) for n in values.shape[1:]), _lib.ptr(out),
               _DT[out.dtype], *_ll(out.stride()), *out_shape, ctypes.byref(d), _lib.stream())
    return out


def warp_grid(vol, grid, matrix=None, offset=0.0, output_shape=None, output=None, order=1, mode='constant', cval=0.0, prefilter=True):
    """The volume sampled at matrix @ o + offset + d(o), d the displacement of the ControlGrid at output voxel o.  matrix and offset are
    affine_transform's (3 x 3, homogeneous, or a diagonal); the default is the identity.  output_shape defaults to the shape the grid was
    made for; on any other shape the grid coordinate is clamped to the grid."""
    values, gzoom, gshift, gorder = _check_grid(grid)
    form, a, b = affine_arguments(np.ones(3) if matrix is None else matrix, offset)
    out_shape = _check_shape(grid.out_shape if output_shape is None else output_shape, 'output_shape')
    return _warp_grid(vol, values, gzoom, gshift, gorder, form, a, b, out_shape, output, order, mode, cval, prefilter)


def elastic_pair(ct, label, grid, ct_order=1, ct_cval=None, label_cval=0):
    """One elastic deformation applied to a CT crop (order 1 or 3) and its label (order 0) through the same grid, so the two stay registered:
    two launches, both results resident -> (ct, label).  ct_cval defaults to the CT dtype's minimum for integers and -1024.0 for floats."""
    if ct_order not in (1, 3):
        raise ValueError('ct_order: 1 or 3 expected, got %r' % (ct_order,))
    mc, ml = _check_volume(ct), _check_volume(label)
    if tuple(mc.shape) != tuple(ml.shape):
        raise ValueError('elastic_pair: a CT and a label of one shape expected, got %s and %s' % (tuple(mc.shape), tuple(ml.shape)))
    if ct_cval is None:
        ct_cval = -1024.0 if mc.dtype.is_floating_point else (0 if mc.dtype in (torch.uint8, torch.bool) else -32768)
    shape = tuple(mc.shape)
    return (warp_grid(ct, grid, output_shape=shape, order=ct_order, cval=ct_cval),
            warp_grid(label, grid, output_shape=shape, order=0, cval=label_cval))


def displacement_of(grid):
    """The dense float64 field [3, *grid.out_shape] the grid stands for, in source voxels: each component of the control values sampled by
    hv_map_coordinates at the clamped grid coordinates at order gorder, prefilter=False.  warp(vol, displacement_of(grid)) is
    warp_grid(vol, grid) on the identity lattice, byte for byte; this is for inspection, warp_grid never forms the field."""
    values, gzoom, gshift, gorder = _check_grid(grid)
    O = _check_shape(grid.out_shape, 'out_shape')
    q = torch.empty((3,) + O, dtype=torch.float64, device=values.device)
    for a in range(3):
        x = (torch.arange(O[a], dtype=torch.float64, device=values.device) + float(gshift[a])) * float(gzoom[a])
        hi = float(values.shape[a + 1] - 1)
        x = torch.where(x >= 0.0, torch.where(x <= hi, x, torch.full_like(x, hi)), torch.zeros_like(x))
        q[a] = x.view([-1 if i == a else 1 for i in range(3)])
    out = torch.empty((3,) + O, dtype=torch.float64, device=values.device)
    for h in range(3):
        _map(values[h], q, ABSOLUTE, out[h], gorder, 'constant', 0.0, False)
    return out
