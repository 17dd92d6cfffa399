"""Parallel-beam projections of resident volumes (csrc/projection.hip through hv_project): the lateral or AP
radiograph, the minimum / maximum intensity projection, the thickness map and the areal density of a vertebra.

Every other volume tool here is a 3-D measure; clinicians judge these vertebrae on projections (the Genant grade is defined on the lateral
radiograph, osteoporosis on DXA's areal density).  A projection is resample.affine_transform's lattice (p0, p1, t) -- pixel (p0, p1) of a
P0 x P1 detector, step t of T along the ray -- reduced over t inside the kernel: the lattice is never written.
  project(vol, poses, det_shape, steps, order=1, label=None, label_value=None)  -> Projection: acc float64 [K, 3, P0, P1] (sum, min, max),
                                                                                   idx int32 [K, 3, P0, P1] (count, first, last), info int64 [K, 8]
  view_pose(shape, spacing, view, det_spacing=None, step_mm=None, det_shape=None, steps=None)  -> ViewPose                     (host, float64)
  radiograph(vol, spacing, view='lateral', ...)        the line integral sum * step_mm per pixel (value * mm)
  mip(vol, spacing, view='lateral', ...)               (min, max) per pixel
  thickness_map(label, value, spacing, view=..., ...)  count * step_mm per pixel: the path length inside label == value (mm)
  areal_density(ct, label, vert_id, spacing, view='lateral', ...)       projected area, integral, their quotient, mean path length
  projection_comparison(ct_original, label_original, ct_synth, label_synth, vert_id, neighbours=(), spacing=..., view='lateral', ...)
Volumes are 3-D device tensors with any strides, uint8 / int16 / float32 / float64 (numpy arrays are uploaded first); a label volume may also
be int32 / int64.  A pose is affine_transform's (matrix [3][3], offset [3]): lattice point (p0, p1, t) reads the volume at matrix @ (p0, p1,
t) + offset.  Only the part of a ray inside the volume is measured; nothing is padded.  With a label, a sample counts only where the label
at the nearest voxel equals label_value.

Named views, consistent with infer.py (sagittal slices are `[:, :, k]`, coronal slices `[:, k, :]`): 'lateral' runs the ray along array axis 2
(the detector shows axes 0 and 1: the picture of a sagittal slice), 'ap' along array axis 1 (the detector shows axes 0 and 2: a coronal
slice), 'axial' along array axis 0 (axes 1 and 2).  Three angles (degrees) turn the lateral frame by similarity.rotation_matrix.

The sum's order of summation is part of the definition (chunks of 16 steps; include/hvgan.h), so acc is the same bytes on every run.  The
results stay on the device; each derived function reads back once.  Cone-beam (perspective) geometry, scatter, beam hardening and the
HU -> BMD calibration of a densitometer are out of scope: the areal density here is in (CT value) x mm, not g/cm^2."""
import ctypes
import math
from collections import namedtuple

import numpy as np
import torch

from . import lib as _lib
from . import resample as _rs
from .components import _device, _ll
from .label_statistics import NONFINITE, EMPTY  # noqa: F401  (the status bits of info[:, 0])
from .labelled import check_spacing
from .similarity import _check_poses, rotation_matrix
from .straighten import _DT as _LABEL_DT

CHUNK, MAX_POSES, INFO = 16, 16, 8                                    # HV_PROJ_* of include/hvgan.h
STATUS, COUNTED, OUTSIDE, REJECTED, NOT_FINITE = range(5)
SUM, MIN, MAX = range(3)                                              # the planes of acc
COUNT, FIRST, LAST = range(3)                                         # the planes of idx
VIEWS = {'lateral': (0, 1, 2), 'ap': (0, 2, 1), 'axial': (1, 2, 0)}   # detector axis 0, detector axis 1, the ray's array axis
SCALARS = ('area', 'integral', 'areal_density', 'mean_path')

Projection = namedtuple('Projection', 'acc idx info')
ViewPose = namedtuple('ViewPose', 'matrix offset det_shape steps det_spacing step_mm')


# ------------------------------------------------------------------------------------------------ host: geometry
def view_frame(view):
    """The 3 x 3 matrix whose columns are the detector's two axes and the ray's direction, unit vectors in millimetre space: a named view's
    are array axes (VIEWS), three angles give similarity.rotation_matrix(angles) -- the lateral frame turned."""
    if isinstance(view, str):
        if view not in VIEWS:
            raise ValueError('view: one of %s or three angles expected, got %r' % (', '.join(VIEWS), view))
        a0, a1, ar = VIEWS[view]
        f = np.zeros((3, 3))
        f[a0, 0], f[a1, 1], f[ar, 2] = 1.0, 1.0, 1.0
        return f
    return rotation_matrix(view)


def _positive(v, name):
    v = float(v)
    if not math.isfinite(v) or not v > 0.0:
        raise ValueError('%s: a positive finite number expected, got %r' % (name, v))
    return v


def _count(n, name):
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
        raise ValueError('%s: a positive integer expected, got %r' % (name, n))
    return int(n)


def view_pose(shape, spacing, view, det_spacing=None, step_mm=None, det_shape=None, steps=None):
    """The pose of a parallel-beam view of a volume of `shape` voxels of `spacing` millimetres (anisotropic is fine).  The detector is
    centred on the volume's centre (shape - 1) / 2 and the middle step of the ray lies on it.  det_spacing (one number or two) and step_mm are
    the pixel pitch and the step along the ray in millimetres, by default the smallest voxel spacing; det_shape and steps cover the volume's
    bounding sphere -- ceil(diameter / pitch) + 1 with diameter = |(shape - 1) * spacing| -- unless given.  In this order: F = view_frame(view),
    matrix = (F * (ds0, ds1, step)[None, :]) / spacing[:, None], offset = (shape - 1) / 2 - matrix @ ((P0 - 1) / 2, (P1 - 1) / 2, (T - 1) / 2).
    A named view with the volume's own pitches and extents samples every voxel once, at whole indices.  Host only, float64.
    -> ViewPose(matrix, offset, det_shape, steps, det_spacing, step_mm)"""
    n = np.array(_rs._check_shape(shape, 'shape'), dtype=np.float64)
    sp = np.array(check_spacing(spacing), dtype=np.float64)
    f = view_frame(view)
    if det_spacing is None:
        ds = np.array([sp.min(), sp.min()])
    else:
        ds = np.asarray(det_spacing, dtype=np.float64) * np.ones(2)
        ds = np.array([_positive(ds[0], 'det_spacing'), _positive(ds[1], 'det_spacing')])
    st = float(sp.min()) if step_mm is None else _positive(step_mm, 'step_mm')
    diameter = float(np.sqrt((((n - 1.0) * sp) ** 2).sum()))
    if det_shape is None:
        det_shape = (int(math.ceil(diameter / ds[0])) + 1, int(math.ceil(diameter / ds[1])) + 1)
    elif len(tuple(det_shape)) != 2:
        raise ValueError('det_shape: two positive integers expected, got %r' % (det_shape,))
    det_shape = (_count(det_shape[0], 'det_shape'), _count(det_shape[1], 'det_shape'))
    steps = int(math.ceil(diameter / st)) + 1 if steps is None else _count(steps, 'steps')
    pitch = np.array([ds[0], ds[1], st])
    matrix = (f * pitch[None, :]) / sp[:, None]
    centre = (n - 1.0) / 2.0
    mid = (np.array([det_shape[0], det_shape[1], steps], dtype=np.float64) - 1.0) / 2.0
    offset = centre - matrix @ mid
    return ViewPose(matrix, offset, det_shape, steps, ds, st)


# ------------------------------------------------------------------------------------------------ the launch
def _volume(x, name, dev, shape=None, dtypes=None):
    t = torch.as_tensor(x)
    if t.dim() != 3 or 0 in tuple(t.shape):
        raise ValueError('%s: a non-empty 3-D volume expected, got shape %s' % (name, tuple(t.shape)))
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError('%s: shape %s expected, got %s' % (name, tuple(shape), tuple(t.shape)))
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    if t.dtype not in (dtypes or _rs._DT):
        raise TypeError('%s: a volume of dtype %s expected, got %s' % (name, ' / '.join(str(d) for d in (dtypes or _rs._DT)), t.dtype))
    if t.numel() > 2 ** 30:
        raise ValueError('%s: at most 2^30 voxels are supported' % name)
    t = t.to(dev)
    _lib.require_gpu(t)
    return t


def _launch(v, lab, label_value, poses, det_shape, steps, order, acc, idx, info):
    """Queue one hv_project on the current stream: up to 16 poses [n][12]; acc float64 [n][3][P0][P1], idx int32 likewise, info int64 [n][INFO]."""
    L = _lib.get()
    n = len(poses)
    flat = (ctypes.c_double * (12 * n))(*[float(x) for x in poses.reshape(-1)])
    lst = lab.stride() if lab is not None else (0, 0, 0)
    with torch.cuda.device(v.device):
        L.call('hv_project', _lib.ptr(v), _rs._DT[v.dtype], *_ll(v.stride()), *(int(s) for s in v.shape), _lib.ptr(lab),
               _LABEL_DT[lab.dtype] if lab is not None else 0, *_ll(lst), ctypes.c_double(label_value), flat, n, det_shape[0], det_shape[1],
               steps, order, _lib.ptr(acc), _lib.ptr(idx), _lib.ptr(info), None, ctypes.c_size_t(0), _lib.stream())


def _prepare(vol, label, label_value, order):
    if isinstance(order, bool) or not isinstance(order, (int, np.integer)) or int(order) not in _rs.ORDERS:
        raise ValueError('order: 0, 1 or 3 expected, got %r' % (order,))
    dev = _device(vol, label)
    v = _volume(vol, 'vol', dev)
    lab, lv = None, 0.0
    if label is not None:
        lab = _volume(label, 'label', dev, v.shape, _LABEL_DT)
        if label_value is None or isinstance(label_value, bool) or not math.isfinite(float(label_value)):
            raise ValueError('label_value: a finite number expected with a label, got %r' % (label_value,))
        lv = float(label_value)
    elif label_value is not None:
        raise ValueError('label_value without a label')
    if int(order) == 3:
        v = _rs.spline_filter(v)                                      # the coefficients, once per call
    return v, lab, lv, int(order)


def _check_lattice(det_shape, steps):
    if len(tuple(det_shape)) != 2:
        raise ValueError('det_shape: two positive integers expected, got %r' % (det_shape,))
    P0, P1, T = _count(det_shape[0], 'det_shape'), _count(det_shape[1], 'det_shape'), _count(steps, 'steps')
    if P0 * P1 * T > 2 ** 30:
        raise ValueError('det_shape x steps: at most 2^30 samples per pose are supported')
    return (P0, P1), T


def _buffers(n, det_shape, dev):
    """One allocation for the three results of n poses, so that one copy reads all of them back: acc, idx, info and the raw bytes."""
    P = det_shape[0] * det_shape[1]
    na, ni = n * 3 * P * 8, n * 3 * P * 4
    ni_pad = -(-ni // 8) * 8
    raw = torch.empty((na + ni_pad + n * INFO * 8,), dtype=torch.uint8, device=dev)
    acc = raw[:na].view(torch.float64).view(n, 3, *det_shape)
    idx = raw[na:na + ni].view(torch.int32).view(n, 3, *det_shape)
    info = raw[na + ni_pad:].view(torch.int64).view(n, INFO)
    return acc, idx, info, raw


def _host(raw, n, det_shape):
    P = det_shape[0] * det_shape[1]
    na, ni = n * 3 * P * 8, n * 3 * P * 4
    ni_pad = -(-ni // 8) * 8
    h = raw.cpu().numpy()
    return Projection(h[:na].view(np.float64).reshape(n, 3, *det_shape), h[na:na + ni].view(np.int32).reshape(n, 3, *det_shape),
                      h[na + ni_pad:].view(np.int64).reshape(n, INFO))


def _run(v, lab, lv, poses, det_shape, steps, order, acc, idx, info):
    for c in range(0, len(poses), MAX_POSES):
        _launch(v, lab, lv, poses[c:c + MAX_POSES], det_shape, steps, order, acc[c:c + MAX_POSES], idx[c:c + MAX_POSES], info[c:c + MAX_POSES])


def project(vol, poses, det_shape, steps, order=1, label=None, label_value=None, readback=False):
    """The projections of `vol` under every pose (one (matrix, offset) pair or a sequence of any length, run in chunks of 16 with no
    readback in between) onto a detector of det_shape = (P0, P1) pixels with `steps` steps per ray, at spline order 0 / 1 / 3 (order 3 makes
    the coefficients once, through resample.spline_filter).  label, label_value: count a sample only where label == label_value at the voxel
    nearest to it.  -> Projection(acc float64 [K, 3, P0, P1]: the sum, minimum and maximum over the counted samples of each ray; idx int32
    [K, 3, P0, P1]: their number, the first and the last counted step; info int64 [K, 8]: status (label_statistics' bits: 2 a NaN or
    infinity was sampled, 4 nothing counted), counted, outside the volume, rejected by the label, not finite).  A ray with no counted sample
    has sum 0, min +inf, max -inf, first = steps, last = -1.  The three are resident device tensors and nothing is read back;
    readback=True returns numpy arrays instead, from one copy."""
    p = _check_poses(poses)
    det_shape, steps = _check_lattice(det_shape, steps)
    v, lab, lv, order = _prepare(vol, label, label_value, order)
    acc, idx, info, raw = _buffers(len(p), det_shape, v.device)
    _run(v, lab, lv, p, det_shape, steps, order, acc, idx, info)
    return _host(raw, len(p), det_shape) if readback else Projection(acc, idx, info)


# ------------------------------------------------------------------------------------------------ the derived pictures and numbers
def _is_one_view(view):
    """A name or three angles (True), or a list of those (False)."""
    if isinstance(view, str):
        return True
    try:
        return np.asarray(view, dtype=np.float64).shape == (3,)
    except (TypeError, ValueError):
        return False


def _one_view(vol, spacing, view, order, label, label_value, geometry):
    shape = tuple(torch.as_tensor(vol).shape) if not isinstance(vol, torch.Tensor) else tuple(vol.shape)
    vp = view_pose(shape, spacing, view, **geometry)
    return vp, project(vol, (vp.matrix, vp.offset), vp.det_shape, vp.steps, order, label, label_value, readback=True)


def radiograph(vol, spacing, view='lateral', order=1, label=None, label_value=None, **geometry):
    """The line integral of `vol` along every ray of the view: sum * step_mm, float64 [P0, P1], in (value of vol) x mm.  geometry:
    view_pose's det_spacing, step_mm, det_shape, steps.  One readback."""
    vp, res = _one_view(vol, spacing, view, order, label, label_value, geometry)
    return res.acc[0, SUM] * vp.step_mm


def mip(vol, spacing, view='lateral', order=1, label=None, label_value=None, **geometry):
    """(minimum, maximum) intensity projections of the view, float64 [P0, P1] each; +inf / -inf where a ray met nothing.  One readback."""
    _, res = _one_view(vol, spacing, view, order, label, label_value, geometry)
    return res.acc[0, MIN], res.acc[0, MAX]


def thickness_map(label, value, spacing, view='lateral', **geometry):
    """The path length of every ray inside label == value: count * step_mm, float64 [P0, P1], millimetres (order 0 on the label volume
    itself).  One readback."""
    vp, res = _one_view(label, spacing, view, 0, label, value, geometry)
    return res.idx[0, COUNT].astype(np.float64) * vp.step_mm


def _areal(acc, idx, vp):
    """One pose's planes on the host -> the areal numbers (tests/projection_ref.py's areal_density, line for line)."""
    pixel = float(vp.det_spacing[0]) * float(vp.det_spacing[1])
    hit = idx[COUNT] > 0
    area = float(hit.sum()) * pixel
    integral = float(acc[SUM][hit].sum()) * vp.step_mm * pixel
    path = float(idx[COUNT][hit].astype(np.float64).sum()) * vp.step_mm
    nan = float('nan')
    return {'area': area, 'integral': integral, 'areal_density': integral / area if area > 0 else nan,
            'mean_path': path / float(hit.sum()) if hit.any() else nan, 'pixels': int(hit.sum()), 'samples': int(idx[COUNT].sum())}


def areal_density(ct, label, vert_id, spacing, view='lateral', order=1, **geometry):
    """What a densitometer reports of one vertebra, from the CT: the rays of the view through label == vert_id.
    -> {'area': the projected area, pixels with count > 0 times the pixel area (mm^2); 'integral': sum over them of sum * step_mm * pixel
    area ((CT value) x mm^3); 'areal_density': integral / area ((CT value) x mm: DXA's quantity before any calibration); 'mean_path': the mean
    path length inside the vertebra over those pixels (mm); 'pixels', 'samples': the integer counts}.  NaN where nothing was hit.  One
    readback."""
    vp, res = _one_view(ct, spacing, view, order, label, vert_id, geometry)
    return _areal(res.acc[0], res.idx[0], vp)


def projection_comparison(ct_original, label_original, ct_synth, label_synth, vert_id, neighbours=(), spacing=(1, 1, 1), view='lateral',
                          order=1, **geometry):
    """Does the pseudo-healthy vertebra project like the patient's intact ones?  areal_density of vertebra vert_id in the original pair, in
    the synthesized pair, and of every listed neighbour in the original pair, under `view` -- one named view or angle triple, or a list of them
    that share det_shape and steps (then they run as ONE K-pose call per volume and label value and every entry below is a list over the views).
    -> {'original', 'synthesized': areal_density's dicts, 'neighbours': {id: dict}, 'original_ratio': {scalar: synthesized / original},
    'neighbour_ratio': {scalar: synthesized / the mean over the neighbours}} for the scalars of SCALARS (no neighbours: NaN).
    One launch sequence per (volume, label value) into one result buffer and one readback for all of them; at order 3 the coefficients of
    each CT are made once."""
    single = _is_one_view(view)
    views = [view] if single else list(view)
    ids = [vert_id] + list(neighbours)
    if any(isinstance(i, bool) or not isinstance(i, (int, np.integer)) for i in ids) or len(set(ids)) != len(ids):
        raise ValueError('vert_id, neighbours: distinct integers expected, got %r' % (ids,))
    o_ct, o_lab, _, order = _prepare(ct_original, label_original, vert_id, order)
    s_ct, s_lab, _, _ = _prepare(ct_synth, label_synth, vert_id, order)
    if tuple(s_ct.shape) != tuple(o_ct.shape) or s_ct.device != o_ct.device:
        raise ValueError('the original and the synthesized volumes must agree in shape and lie on one device')
    vps = [view_pose(tuple(o_ct.shape), spacing, w, **geometry) for w in views]
    if any(vp.det_shape != vps[0].det_shape or vp.steps != vps[0].steps for vp in vps):
        raise ValueError('view: the views of one call must share det_shape and steps (give them)')
    poses = _check_poses([(vp.matrix, vp.offset) for vp in vps])
    det_shape, steps = _check_lattice(vps[0].det_shape, vps[0].steps)
    K = len(poses)
    jobs = [(o_ct, o_lab, float(vert_id)), (s_ct, s_lab, float(vert_id))] + [(o_ct, o_lab, float(i)) for i in ids[1:]]
    acc, idx, info, raw = _buffers(K * len(jobs), det_shape, o_ct.device)
    for j, (v, lab, lv) in enumerate(jobs):
        _run(v, lab, lv, poses, det_shape, steps, order, acc[j * K:(j + 1) * K], idx[j * K:(j + 1) * K], info[j * K:(j + 1) * K])
    res = _host(raw, K * len(jobs), det_shape)
    table = [[_areal(res.acc[j * K + k], res.idx[j * K + k], vps[k]) for k in range(K)] for j in range(len(jobs))]
    nan = float('nan')

    def ratio(a, b):
        a, b = float(a), float(b)
        return a / b if b != 0 and b == b else nan

    def per_view(k):
        ori, syn = table[0][k], table[1][k]
        nb = {i: table[2 + s][k] for s, i in enumerate(ids[1:])}
        mean = {q: (float(np.mean([float(x[q]) for x in nb.values()])) if nb else nan) for q in SCALARS}
        return {'original': ori, 'synthesized': syn, 'neighbours': nb, 'original_ratio': {q: ratio(syn[q], ori[q]) for q in SCALARS},
                'neighbour_ratio': {q: ratio(syn[q], mean[q]) for q in SCALARS}}

    out = [per_view(k) for k in range(K)]
    if single:
        return out[0]
    return {key: [o[key] for o in out] for key in out[0]}
