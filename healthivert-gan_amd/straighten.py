"""Spine straightening and per-vertebra volume extraction on the device (stage 1 of the reference workflow).

The reference runs this stage on the CPU, one patient at a time:
  straighten/location_json_local.py:14-16,33-45          the centroid list (mean voxel index per label, two small-label drops)
  straighten/straighten_mask_3d.py:463-563 process_mask3d curve extension, bone window, straightening along the spine curve
                                                          (straighten/curve.py, Interpolator with get_local_basis), the split cleanup
                                                          and the per-vertebra crops (mask_2d and the file I/O excepted)
Here the two volumes stay on the device: one stats pass (CT min / max, per-label counts and index sums, the label check), one small read
back of that record, the curve math on the host (a few hundred points, numpy), then one sampling launch and one crop launch for every
requested vertebra (csrc/straighten.hip).

  vertebra_centroids(label) -> [{"label", "X", "Y", "Z"}, ...]             the JSON list location_json_local.py writes
  straighten_patient(ct, label, vertebrae_ids, centroids=None, out_size=(256, 256, 64), depedicle=False) -> {vert_id: (ct_vol, label_vol)}
  depedicle(label_vol, out=None) -> uint8 volume            process_3d_array (straighten_mask_3d.py:189-219) on a crop or a batch of crops
  component_counts(label_vol) -> int32 [Z, 256]             4-connected components of every label value per slice
  single_component_range(label_vol, label, offset=10)       find_single_component_layers (:249-280) -> (z0, z1)
  spline_coefficients(vol, window=None) -> float64 volume    scipy.ndimage.spline_filter(vol, 3, mode='mirror'): the prefilter of order=3
  restore_patient(plan, crops, shape=None, ct=None, label=None, where='vertebra') -> (ct_out, label_out[, covered][, local])
                                                            the way back: Interpolator.global_to_local (curve.py:104-150,223-239) for every
                                                            voxel of a vertebra's patient-space box (restore_box) and a resample of the
                                                            (synthesized) crop there (csrc/restore.hip)
  points_to_local(plan, points) / points_to_global(plan, points)   Interpolator.global_to_local / local_to_global (curve.py:104-114) for a
                                                            list of points on the device: where in the patient's scan a position of the
                                                            straightened frame lies, and back

Scans with anisotropic voxels: straighten_patient, plan, curve_frame, global_to_local, local_to_global and restore_box take
spacing=(sx, sy, sz), millimetres per voxel, the `spacing` of the reference's Interpolator (curve.py:26-52,160-195), which process_mask3d
leaves at 1.  The scan is read at its native spacing, the crops come out on the 1 mm grid the later stages assume, and restore_patient
(which reads the spacing from the plan) writes back onto the scan's own grid.

Cubic resampling: straighten_patient and restore_patient take order=1 (trilinear, the default and what process_mask3d asks for) or order=3,
the cubic B-spline of interpolate_along(array, shape, order=3) (curve.py:77-102 -> scipy.ndimage.map_coordinates): the scan (each crop's
filled part on the way back) is prefiltered once into float64 B-spline coefficients (csrc/spline.hip; spline_coefficients(vol) is that step
alone) and the CT is sampled from 4 x 4 x 4 taps of them.  Labels stay order 0.  There is no clipping: a cubic sample of windowed [0, 255] data
may leave that interval, as it does in scipy.  The coefficients cost 8 bytes per voxel of the scan (839 MB for 512 x 512 x 400).

Volumes are [X, Y, Z] device tensors as nibabel hands them over (any strides; a Fortran-ordered array passes as it lies).  The CT may be
int16, float32 or float64 and is windowed in double for every dtype.  Deviation: the reference reads CT files over 500 MB as float32
(straighten_mask_3d.py:474-477); here the CT is always widened to double, which moves the windowed values of such files by less than 1e-4.

The host functions below restate the reference's curve code (citing the lines they restate); they are numpy only and never build the
N x 128 x 128 x 3 sample grid: the kernel computes each sample's coordinate from the knot and the frame of its plane.
"""
import ctypes
import warnings

import numpy as np
import torch

from . import lib as _lib

PLANE = (128, 128)            # interpolate_along(vol, shape) (straighten_mask_3d.py:494)
WINDOW = (-300.0, 800.0)      # window(ct_data, -300, 800) (:491)
EXTENSION = 20                # extend_curve(coords, 20, (0, 0, 0), label.shape) (:487)
DROP_MAX, DROP_MIN = 8000, 6000   # location_json_local.py:40-43

_DT = {torch.uint8: 0, torch.int16: 1, torch.int32: 2, torch.int64: 3, torch.float32: 4, torch.float64: 5}
_CT_DT = (torch.int16, torch.float32, torch.float64)
_HDR, _CNT, _SUM, _PRES = 4, 4, 260, 1028   # word offsets of the stats record (include/hvgan.h)


# ------------------------------------------------------------------------------------------------ host curve math (numpy)
def interp_linear(x, y, x_new):
    """scipy.interpolate.interp1d(x, y, axis=0) (linear; extrapolating with the end segments) at x_new: x sorted stably, the segment
    found by searchsorted and clipped to [1, len - 1], y = slope * (x_new - x_lo) + y_lo with slope = (y_hi - y_lo) / (x_hi - x_lo)."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    order = np.argsort(x, kind='mergesort')
    x, y = x[order], y[order]
    x_new = np.atleast_1d(np.asarray(x_new, dtype=np.float64))
    hi = np.searchsorted(x, x_new).clip(1, len(x) - 1).astype(int)
    lo = hi - 1
    slope = (y[hi] - y[lo]) / (x[hi] - x[lo])[:, None]
    return slope * (x_new - x[lo])[:, None] + y[lo]


def extend_curve(curve, extension_length=EXTENSION, min_bounds=(0, 0, 0), max_bounds=None):
    """straighten_mask_3d.py:96-121: one point more at each end, `extension_length` along the end segment, each axis clamped to
    [min_bounds[i], max_bounds[i]] (the reference passes the volume shape, so the upper bound is shape_i, not shape_i - 1)."""
    curve = np.asarray(curve, dtype=np.float64)
    out = [None, None]
    for k, (p, q) in enumerate(((curve[0], curve[1]), (curve[-1], curve[-2]))):
        d = p - q
        pt = p + d / np.linalg.norm(d) * extension_length
        out[k] = np.array([max(min_bounds[i], min(max_bounds[i], pt[i])) for i in range(3)])
    return np.vstack([out[0], curve, out[1]])


def cumulative_length(curve):
    """curve.py:203-206: 0, then the running sum of the segment lengths."""
    return np.insert(np.cumsum(np.linalg.norm(np.diff(curve, axis=0), axis=1)), 0, 0)


def local_basis(grad):
    """get_local_basis (straighten_mask_3d.py:155-170): columns = unit tangent, a unit vector in the sagittal (axis 0, axis 2) plane
    oriented by the sign of a 2 x 2 determinant, and their cross product.  -> [N][3][3], basis[n][:, j] = vector j."""
    g = grad / np.linalg.norm(grad, axis=1, keepdims=True)
    sag = g[:, [0, 2]]
    second = sag[:, ::-1] * [1, -1]
    dets = np.linalg.det(np.stack([sag, second], -1))
    second = second * dets[:, None]
    second = second / np.linalg.norm(second, axis=1, keepdims=True)
    second = np.insert(second, 1, np.zeros_like(second[:, 0]), axis=1)
    return np.stack([g, second, np.cross(second, g)], -1)


def check_spacing(spacing):
    """The `spacing` of Interpolator (curve.py:26-44) as three positive finite floats, millimetres per voxel along axes 0, 1, 2; a scalar
    stands for all three.  The library's per-axis position tables (a sequence per axis, curve.py:172-173,191-192) are out of scope."""
    if isinstance(spacing, (int, float, np.integer, np.floating)) and not isinstance(spacing, bool):
        spacing = [spacing] * 3
    try:
        spacing = list(spacing)
    except TypeError:
        raise ValueError('spacing: three positive floats or one, got %r' % (spacing,))
    if len(spacing) != 3:
        raise ValueError('spacing: one value per axis (3), got %d' % len(spacing))
    out = []
    for s in spacing:
        if isinstance(s, bool) or not isinstance(s, (int, float, np.integer, np.floating)):
            if np.ndim(s) > 0 or isinstance(s, (list, tuple)):
                raise ValueError('spacing: per-axis position tables (a sequence per axis) are out of scope, one positive float per axis')
            raise ValueError('spacing: one positive float per axis, got %r' % (s,))
        s = float(s)
        if not (np.isfinite(s) and s > 0.0):
            raise ValueError('spacing: values must be positive and finite, got %r' % (spacing,))
        out.append(s)
    return tuple(out)


def curve_frame(curve, step=1, spacing=(1.0, 1.0, 1.0)):
    """Interpolator(curve, step, spacing, get_local_basis=get_local_basis) (curve.py:26-52 with get_derivatives :209-221): the curve (voxel
    indices) times the spacing (pixel_to_spatial, :160-176), knots at arange(0, L, step) of its cumulative length in millimetres, np.gradient
    of the points interpolated the same way, the frame of local_basis.  -> knots [N][3] (millimetres), basis [N][3][3]."""
    curve = np.asarray(curve, dtype=np.float64) * np.asarray(check_spacing(spacing))
    lengths = cumulative_length(curve)
    xs = np.arange(0, lengths[-1], step)
    knots = interp_linear(lengths, curve, xs)
    grad = interp_linear(lengths, np.gradient(curve, axis=0), xs)
    return knots, local_basis(grad)


def _centers(knots, shape):
    """Interpolator._get_centers (curve.py:116-120): per knot (cumulative length, shape / 2)."""
    centers = np.zeros_like(knots)
    centers[:, 0] = cumulative_length(knots)
    centers[:, 1:] = np.broadcast_to(shape, 2) / 2
    return centers


def _interpolate_coords(coords, to_origin, to_plane):
    """interpolate_coords (curve.py:223-239)."""
    idx = to_origin.argmin()
    cand, = np.diff(np.sign(to_plane)).nonzero()
    if len(cand) != 1:
        warnings.warn("Couldn't uniquely choose a local basis.")
    if len(cand) > 0:
        idx = cand[np.abs(cand - idx).argmin()]
    slc = slice(max(0, idx - 2), idx + 2)
    return interp_linear(to_plane[slc], coords[slc], 0.0)[0]


def global_to_local(point, knots, basis, shape=PLANE, spacing=(1.0, 1.0, 1.0)):
    """Interpolator.global_to_local (curve.py:104-150,223-239) for one point (voxel indices): times the spacing (pixel_to_spatial), its
    offsets from every knot in that knot's frame, plus the plane centres (cumulative length, shape / 2); the plane is chosen where the
    distance to the plane changes sign closest to the nearest knot, and the coordinates are interpolated linearly to distance 0 over up to
    four planes around it."""
    p = np.asarray(point, dtype=np.float64) * np.asarray(check_spacing(spacing)) - knots
    to_origin = np.linalg.norm(p, axis=-1)
    p = np.einsum('nji,nj->ni', basis, p)
    to_plane = p[:, 0]
    return _interpolate_coords(p + _centers(knots, shape), to_origin, to_plane)


def local_to_global(points, knots, basis, shape=PLANE, spacing=(1.0, 1.0, 1.0)):
    """Interpolator.local_to_global (curve.py:110-114,131-138,223-239) for one local point or an array [..., 3] of them (cumulative length,
    offset along frame vector 1, along frame vector 2): per knot the offset from the plane centre, carried into the scan by the knot's
    frame and added to the knot; the plane is chosen and the result interpolated to distance 0 as in global_to_local; the millimetres are
    divided by the spacing (spatial_to_pixel, :179-195).  -> voxel indices, the shape of `points`."""
    sp = np.asarray(check_spacing(spacing))
    pts = np.asarray(points, dtype=np.float64)
    centers = _centers(knots, shape)
    out = np.empty((pts.size // 3, 3))
    for k, point in enumerate(pts.reshape(-1, 3)):
        p = point - centers
        to_plane = p[:, 0]
        p = np.einsum('nij,nj->ni', basis, p)
        to_origin = np.linalg.norm(p, axis=-1)
        out[k] = _interpolate_coords(p + knots, to_origin, to_plane)
    return (out / sp).reshape(pts.shape)


def crop_box(center, src_shape, size):
    """extract_3d_volume (straighten_mask_3d.py:222-247) as index arithmetic: per axis the source range [lo, lo + n) (int() truncation of
    c -+ d // 2, clipped to the volume) and where it lands in the zero volume of `size` (centred; on the last axis a range longer than the
    output keeps its first size[2] elements).  -> (lo0, lo1, lo2, n0, n1, n2, start0, start1, start2)."""
    lo, n, start = [], [], []
    for i in range(3):
        c, d = center[i], size[i]
        a, b = max(0, int(c - d // 2)), min(src_shape[i], int(c + d // 2))
        m = b - a
        s = (d - m) // 2
        if m > d:
            if i < 2:
                raise ValueError('crop: source range %d longer than the output axis %d' % (m, d))
            s, m = 0, d
        lo.append(a)
        n.append(max(m, 0))
        start.append(s)
    return lo + n + start


def centroids_from_counts(counts, sums):
    """location_json_local.py:33-45 from per-label voxel counts [256] and index sums [256][3] (exact integers): labels in ascending order,
    the largest dropped below 8000 voxels, the smallest below 6000, centre = sum / count per axis."""
    labels = [l for l in range(1, 256) if counts[l] > 0]
    out = []
    for l in labels:
        if counts[l] < DROP_MAX and l == max(labels):
            continue
        if counts[l] < DROP_MIN and l == min(labels):
            continue
        c = [float(np.float64(int(sums[l][a])) / np.float64(int(counts[l]))) for a in range(3)]
        out.append({'label': int(l), 'X': c[0], 'Y': c[1], 'Z': c[2]})
    out.sort(key=lambda e: e.get('label', 0))
    return out


# ------------------------------------------------------------------------------------------------ device side
def _dtype_code(t, allowed, what):
    if t.dtype not in allowed:
        raise TypeError('%s: dtype %s not supported (%s)' % (what, t.dtype, ', '.join(str(d) for d in allowed)))
    return _DT[t.dtype]


def _check(ct, label):
    _lib.require_gpu(ct, label)
    if ct.dim() != 3 or tuple(ct.shape) != tuple(label.shape):
        raise ValueError('straighten: CT and label must be two [X, Y, Z] volumes of one shape, got %s and %s'
                         % (tuple(ct.shape), tuple(label.shape)))
    if ct.device != label.device:
        raise ValueError('straighten: CT and label on different devices')
    return _dtype_code(ct, _CT_DT, 'CT'), _dtype_code(label, tuple(_DT), 'label')


def _strides(t):
    return [ctypes.c_longlong(s) for s in t.stride()]


class _Stats:
    def __init__(self, words):
        w = words.view(np.uint64)
        kmin, kmax = ~w[0], w[1]
        self.ct_min = float(self._decode(kmin))
        self.ct_max = float(self._decode(kmax))
        self.bad_label = bool(w[2])
        self.counts = w[_CNT:_CNT + 256].astype(np.int64)
        self.sums = w[_SUM:_SUM + 768].reshape(256, 3)

    @staticmethod
    def _decode(k):
        k = np.uint64(k)
        u = k ^ np.uint64(1 << 63) if k >> np.uint64(63) else ~k
        return np.array([u], dtype=np.uint64).view(np.float64)[0]


def _stats(ct, label, ctc, lc):
    L = _lib.get()
    X, Y, Z = ct.shape
    nbytes = L.size('hv_straighten_stats_bytes', Y)
    rec = torch.empty(nbytes // 8, dtype=torch.int64, device=ct.device)
    L.call('hv_straighten_stats', _lib.ptr(ct), ctc, *_strides(ct), _lib.ptr(label), lc, *_strides(label), X, Y, Z, _lib.ptr(rec),
           ctypes.c_size_t(nbytes), _lib.stream())
    head = rec[:_PRES].cpu().numpy()          # the one read back per patient: the curve math runs on the host
    st = _Stats(head)
    if st.bad_label:
        raise ValueError('straighten: the label volume holds values that are not integers in [0, 255]')
    return st, rec


def check_order(order):
    """The spline order of the CT resampling: 1 (trilinear) or 3 (cubic B-spline); anything else is a ValueError (orders 2, 4 and 5 of
    scipy's map_coordinates are out of scope)."""
    if isinstance(order, bool) or not isinstance(order, (int, np.integer)) or int(order) not in (1, 3):
        raise ValueError('order: 1 (trilinear) or 3 (cubic B-spline), got %r' % (order,))
    return int(order)


def _prefilter(vol, dims, win, wmin, wmax):
    """hv_spline_prefilter of the [dims] box whose first element is vol's (a view: its pointer and strides) -> float64 [dims], contiguous."""
    coef = torch.empty(tuple(dims), dtype=torch.float64, device=vol.device)
    _lib.get().call('hv_spline_prefilter', _lib.ptr(vol), _DT[vol.dtype], *_strides(vol), *(int(d) for d in dims), int(win),
                    ctypes.c_double(wmin), ctypes.c_double(wmax), _lib.ptr(coef), _lib.stream())
    return coef


def spline_coefficients(vol, window=None):
    """The cubic B-spline prefilter alone: scipy.ndimage.spline_filter(vol, 3, mode='mirror') in float64 for a [X, Y, Z] device tensor
    (int16 / float32 / float64, any strides) -> contiguous float64 device tensor of the same shape (8 bytes per voxel).  window: None or
    (win_min, win_max): every voxel goes through window() (straighten_mask_3d.py:178-183) as it is read, before the filter."""
    _lib.require_gpu(vol)
    if vol.dim() != 3 or min(vol.shape) <= 0:
        raise ValueError('spline_coefficients: expected a non-empty [X, Y, Z] volume, got %s' % (tuple(vol.shape),))
    _dtype_code(vol, _CT_DT, 'volume')
    wmin, wmax = (0.0, 1.0) if window is None else (float(window[0]), float(window[1]))
    with torch.cuda.device(vol.device):
        return _prefilter(vol, vol.shape, window is not None, wmin, wmax)


def vertebra_centroids(label):
    """The centroid list of location_json_local.py for one label volume (device tensor [X, Y, Z], integer values 0..255): labels ascending,
    the two small-label drops applied, {"label", "X", "Y", "Z"} = mean voxel index along axes 0, 1, 2 (bit-identical to numpy's)."""
    _lib.require_gpu(label)
    lc = _dtype_code(label, tuple(_DT), 'label')
    L = _lib.get()
    X, Y, Z = label.shape
    nbytes = L.size('hv_straighten_stats_bytes', Y)
    rec = torch.empty(nbytes // 8, dtype=torch.int64, device=label.device)
    zero = [ctypes.c_longlong(0)] * 3
    L.call('hv_straighten_stats', None, 0, *zero, _lib.ptr(label), lc, *_strides(label), X, Y, Z, _lib.ptr(rec),   # no CT: labels only
           ctypes.c_size_t(nbytes), _lib.stream())
    st = _Stats(rec[:_PRES].cpu().numpy())
    if st.bad_label:
        raise ValueError('vertebra_centroids: the label volume holds values that are not integers in [0, 255]')
    return centroids_from_counts(st.counts, st.sums)


class Plan(tuple):
    """What plan() returns: the tuple (knots, basis, local, boxes) with the spacing it was made with as `.spacing`."""
    spacing = (1.0, 1.0, 1.0)


def plan(centroids, shape, vertebrae_ids, out_size=(256, 256, 64), plane=PLANE, spacing=(1.0, 1.0, 1.0)):
    """Host part of process_mask3d (straighten_mask_3d.py:485-541) for a centroid list and a volume shape: the extended curve, knots and
    frame (None, None with one centroid), and per requested vertebra the local centroid and its crop box.  Raises ValueError for a
    missing id or a degenerate curve (the reference would divide by zero or hit a NameError).
    spacing: millimetres per voxel of the scan, handed to the Interpolator (:505 with spacing=spacing).  Centroids, the curve extension and
    its clamp stay in voxel indices as in the reference; knots, frame and local centroids are in millimetres, so the straight volume is on
    a 1 mm grid.  The single-centroid branch crops the raw volume and ignores the spacing.  -> Plan (knots, basis, local, boxes)."""
    spacing = check_spacing(spacing)
    coords = [[e['X'], e['Y'], e['Z']] for e in centroids if isinstance(e, dict) and 'X' in e]
    if not coords:
        raise ValueError('straighten: no centroid')
    knots = basis = None
    if len(coords) > 1:
        curve = np.asarray(coords, dtype=np.float64)
        if not np.isfinite(curve).all() or (np.linalg.norm(np.diff(curve, axis=0), axis=1) == 0).any():
            raise ValueError('straighten: degenerate curve (two equal consecutive centroids)')
        curve = extend_curve(curve, EXTENSION, (0, 0, 0), tuple(shape))
        if (np.linalg.norm(np.diff(curve, axis=0), axis=1) == 0).any():
            raise ValueError('straighten: degenerate curve after the extension')
        knots, basis = curve_frame(curve, 1, spacing)
        if len(knots) == 0 or not (np.isfinite(knots).all() and np.isfinite(basis).all()):
            raise ValueError('straighten: degenerate curve (no finite frame)')
        src_shape = (len(knots), plane[1], plane[0])
    else:
        src_shape = tuple(shape)
    boxes, local = [], {}
    for vid in vertebrae_ids:
        centroid = None
        for e in centroids:            # the last entry with that label wins, as in the reference's loop (:516-523)
            if e.get('label') is None:
                continue
            if e['label'] == vid:
                centroid = (e['X'], e['Y'], e['Z'])
        if centroid is None:
            raise ValueError('straighten: vertebra %r has no centroid' % (vid,))
        if knots is not None:
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                centroid = global_to_local(centroid, knots, basis, plane, spacing)
            if not np.isfinite(centroid).all():
                raise ValueError('straighten: vertebra %r: no local position on the curve' % (vid,))
        local[vid] = np.asarray(centroid, dtype=np.float64)
        boxes.append(crop_box(centroid, src_shape, out_size))
    res = Plan((knots, basis, local, boxes))
    res.spacing = spacing
    return res


def _depedicle_launch(vol4, out4, counts):
    """One hv_depedicle launch for a [V, A0, A1, Z] batch (csrc/depedicle.hip) and the read back of its status words."""
    L = _lib.get()
    V, A0, A1, Z = vol4.shape
    status = torch.empty(V, dtype=torch.int32, device=vol4.device)
    sv, s0, s1, s2 = _strides(vol4)
    if out4 is None:
        optr, (ov, o0, o1, o2) = None, [ctypes.c_longlong(0)] * 4
    else:
        optr, (ov, o0, o1, o2) = _lib.ptr(out4), _strides(out4)
    L.call('hv_depedicle', _lib.ptr(vol4), _DT[vol4.dtype], s0, s1, s2, sv, A0, A1, Z, V, optr, o0, o1, o2, ov, _lib.ptr(counts),
           _lib.ptr(status), _lib.stream())
    st = status.cpu().numpy()
    if (st & 1).any():
        raise ValueError('depedicle: the label volume holds values that are not integers in [0, 255]')
    if (st & 2).any():
        where = '' if counts is None else ': (volume, slice) %s' % [tuple(int(i) for i in r) for r in (counts[:, :, 0] < 0).nonzero().cpu().numpy()]
        raise RuntimeError('depedicle: the labelling of a slice did not converge' + where)


def _as_batch(label_vol, what):
    _lib.require_gpu(label_vol)
    if label_vol.dim() not in (3, 4):
        raise ValueError('%s: expected a [A0, A1, Z] volume or a [V, A0, A1, Z] batch, got %s' % (what, tuple(label_vol.shape)))
    _dtype_code(label_vol, tuple(_DT), 'label')
    if label_vol.numel() == 0:
        raise ValueError('%s: empty volume %s' % (what, tuple(label_vol.shape)))
    return label_vol if label_vol.dim() == 4 else label_vol.unsqueeze(0)


def depedicle(label_vol, out=None):
    """process_3d_array (straighten_mask_3d.py:215-219) on the device: in every slice [:, :, z] and for every label value, only the 4-connected
    component that reaches the smallest index on axis 1 stays (ties: the component scipy numbers first), which cuts the vertebral arches off.
    label_vol: a [A0, A1, Z] volume or a [V, A0, A1, Z] batch (one launch), integer values 0..255 in any dtype of _DT, any strides; a slice
    holds at most 65536 pixels.  out: None or a uint8 device tensor of the same shape (any strides; may be label_vol itself).  -> out."""
    vol4 = _as_batch(label_vol, 'depedicle')
    if out is None:
        out = torch.empty(tuple(label_vol.shape), dtype=torch.uint8, device=label_vol.device)
    else:
        _lib.require_gpu(out)
        if out.dtype != torch.uint8 or tuple(out.shape) != tuple(label_vol.shape) or out.device != label_vol.device:
            raise ValueError('depedicle: out must be a uint8 tensor of shape %s on the device of the labels' % (tuple(label_vol.shape),))
    V, _, _, Z = vol4.shape
    counts = torch.empty(V, Z, 256, dtype=torch.int32, device=vol4.device)
    _depedicle_launch(vol4, out if out.dim() == 4 else out.unsqueeze(0), counts)
    return out


def component_counts(label_vol):
    """-> int32 device tensor [Z, 256] ([V, Z, 256] for a batch): the number of 4-connected components of every label value in every slice
    [:, :, z] (scipy.ndimage.label(layer == value)[1]; 0 for an absent value and for value 0)."""
    vol4 = _as_batch(label_vol, 'component_counts')
    V, _, _, Z = vol4.shape
    counts = torch.empty(V, Z, 256, dtype=torch.int32, device=vol4.device)
    _depedicle_launch(vol4, None, counts)
    return counts if label_vol.dim() == 4 else counts[0]


def single_component_walk(ncomp, offset=10):
    """The walk of find_single_component_layers (straighten_mask_3d.py:255-280) over the per-slice component counts of one label: from
    mid - offset downwards and from mid + offset upwards (both start indices clamped to the volume) to the first slice with exactly one
    component; z0 = 1 and z1 = 128 where none is found."""
    Z = len(ncomp)
    mid = Z // 2
    start_left, start_right = max(0, mid - offset), min(Z - 1, mid + offset)
    z0, z1 = 1, 128
    for i in range(start_left, -1, -1):
        if ncomp[i] == 1:
            z0 = i
            break
    for i in range(start_right, Z):
        if ncomp[i] == 1:
            z1 = i
            break
    return z0, z1


def single_component_range(label_vol, label, offset=10):
    """find_single_component_layers(data, label) (straighten_mask_3d.py:249-280) for one [A0, A1, Z] device volume: the slice range over
    which vertebra `label` is one piece, from one read back of that label's count column."""
    _lib.require_gpu(label_vol)
    if label_vol.dim() != 3:
        raise ValueError('single_component_range: expected one [A0, A1, Z] volume, got %s' % (tuple(label_vol.shape),))
    counts = component_counts(label_vol)
    if float(label) == int(label) and 1 <= int(label) <= 255:
        col = counts[:, int(label)].cpu().numpy()
    else:                                   # no voxel can hold it: no slice qualifies
        col = np.zeros(counts.shape[0], dtype=np.int32)
    return single_component_walk(col, offset)


_depedicle = depedicle


def straighten_patient(ct, label, vertebrae_ids, centroids=None, out_size=(256, 256, 64), return_plan=False, depedicle=False,
                       spacing=(1.0, 1.0, 1.0), order=1):
    """process_mask3d(ct, label, json, vertebrae_ids, out, out_size) on device tensors (straighten_mask_3d.py:463-563, mask_2d and file I/O
    excepted).  ct: [X, Y, Z] int16 / float32 / float64; label: [X, Y, Z] integer values 0..255 in any integer or float dtype.  centroids:
    the list location_json_local.py writes, or None = computed on the device from the same stats pass.
    depedicle: the label crops of all requested vertebrae go through one de-pedicling launch, in place, before they are returned (the
    process_3d_array call the reference keeps commented out in process_mask3d).
    spacing: millimetres per voxel of the scan along its three axes (a scalar: all three), the Interpolator's `spacing` (curve.py:26-52):
    the scan is read at its native spacing and the crops come out on the 1 mm grid the later stages assume; no resampled copy is made.
    order: how the CT is resampled, interpolate_along's `order` (curve.py:77-102): 1 = trilinear (what process_mask3d passes), 3 = cubic
    B-spline: the scan is prefiltered once, the window fused into that pass (8 bytes per voxel of the scan while the call runs), and sampled
    cubically.  Labels are order 0 either way and come out bit-identical.  A cubic sample is not clipped: it may leave the window's [0, 255],
    as in scipy.  With one centroid (a raw crop at integer offsets) order has no effect.  The plan records it as 'order'.
    -> {vert_id: (ct_vol float64, label_vol uint8)}, each [out_size] on the device, the orientation the reference saves."""
    spacing = check_spacing(spacing)          # before any GPU work
    order = check_order(order)
    ctc, lc = _check(ct, label)
    L = _lib.get()
    dev = ct.device
    X, Y, Z = ct.shape
    st, rec = _stats(ct, label, ctc, lc)
    if centroids is None:
        centroids = centroids_from_counts(st.counts, st.sums)
    vertebrae_ids = list(vertebrae_ids)
    knots, basis, local, boxes = plan(centroids, (X, Y, Z), vertebrae_ids, out_size, spacing=spacing)
    # window(): the whole volume inside (-300, 800) is returned unchanged (:172-176)
    win = 0 if (st.ct_max < WINDOW[1] and st.ct_min > WINDOW[0]) else 1
    wmin, wmax = ctypes.c_double(WINDOW[0]), ctypes.c_double(WINDOW[1])
    O0, O1, O2 = (int(s) for s in out_size)
    V = len(vertebrae_ids)
    ct_out = torch.empty(max(V, 1), O0, O1, O2, dtype=torch.float64, device=dev)
    lab_out = torch.empty(max(V, 1), O0, O1, O2, dtype=torch.uint8, device=dev)
    if V:
        d_boxes = torch.tensor(boxes, dtype=torch.int32).to(dev, non_blocking=False)
        if knots is not None:
            N, PA, PB = len(knots), PLANE[1], PLANE[0]
            d_knots = torch.from_numpy(np.ascontiguousarray(knots)).to(dev)
            d_basis = torch.from_numpy(np.ascontiguousarray(basis)).to(dev)
            sct = torch.empty(N, PA, PB, dtype=torch.float64, device=dev)
            slab = torch.empty(N, PA, PB, dtype=torch.uint8, device=dev)
            pbytes = L.size('hv_straighten_presence_bytes', PA)
            pres = torch.empty(pbytes // 8, dtype=torch.int64, device=dev)
            if order == 3:
                coef = _prefilter(ct, (X, Y, Z), win, *WINDOW)
                L.call('hv_straighten_sample_spline', _lib.ptr(coef), _lib.ptr(label), lc, *_strides(label), X, Y, Z, _lib.ptr(d_knots),
                       _lib.ptr(d_basis), N, PA, PB, _lib.ptr(sct), _lib.ptr(slab), _lib.ptr(pres), ctypes.c_size_t(pbytes),
                       (ctypes.c_double * 3)(*spacing), _lib.stream())
            else:
                L.call('hv_straighten_sample_sp', _lib.ptr(ct), ctc, *_strides(ct), _lib.ptr(label), lc, *_strides(label), X, Y, Z,
                       _lib.ptr(d_knots), _lib.ptr(d_basis), N, PA, PB, win, wmin, wmax, _lib.ptr(sct), _lib.ptr(slab), _lib.ptr(pres),
                       ctypes.c_size_t(pbytes), (ctypes.c_double * 3)(*spacing), _lib.stream())
            L.call('hv_straighten_crop', _lib.ptr(sct), 5, *_strides(sct), _lib.ptr(slab), 0, *_strides(slab), PA, 0, wmin, wmax,
                   _lib.ptr(pres), _lib.ptr(d_boxes), V, O0, O1, O2, _lib.ptr(ct_out), _lib.ptr(lab_out), _lib.stream())
        else:   # one centroid: the windowed raw CT and the raw label are cropped at the raw position (:499-502)
            L.call('hv_straighten_crop', _lib.ptr(ct), ctc, *_strides(ct), _lib.ptr(label), lc, *_strides(label), Y, win, wmin, wmax,
                   _lib.ptr(rec[_PRES:]), _lib.ptr(d_boxes), V, O0, O1, O2, _lib.ptr(ct_out), _lib.ptr(lab_out), _lib.stream())
        if depedicle:
            _depedicle(lab_out, out=lab_out)
    out = {vid: (ct_out[i], lab_out[i]) for i, vid in enumerate(vertebrae_ids)}
    if return_plan:
        return out, {'centroids': centroids, 'knots': knots, 'basis': basis, 'local': local, 'boxes': boxes, 'window': bool(win),
                     'spacing': spacing, 'order': order}
    return out


# ------------------------------------------------------------------------------------------------ back to patient space
RESTORE = {'crop': 0, 'vertebra': 1}          # HV_RESTORE_CROP / HV_RESTORE_VERTEBRA (include/hvgan.h)


def restore_box(knots, basis, box, shape, plane=PLANE, pad=2, spacing=(1.0, 1.0, 1.0)):
    """Patient-space integer box that holds every voxel a crop's filled part can reach: -> [x0, y0, z0, nx, ny, nz] (all zero when nothing
    is filled).  box: the crop_box row of the vertebra.  With a curve, the filled part is the knots whose cumulative length lies in the
    row's axis-0 range (one knot more at each end: global_to_local interpolates between neighbouring planes) times the in-plane rectangle
    [lo1, lo1 + n1 - 1] x [lo2, lo2 + n2 - 1]; the box is the min / max over those knots of the rectangle's four corners
    knots[n] + basis[n][:, 1] (b - plane[0] / 2) + basis[n][:, 2] (a - plane[1] / 2), in millimetres, divided by the spacing, widened by
    `pad` (voxels) and clipped to the volume.  Without one (knots None: the crop was cut from the raw volume) it is the row's source range
    itself, whatever the spacing."""
    sp = np.asarray(check_spacing(spacing))
    lo, n = [int(v) for v in box[0:3]], [int(v) for v in box[3:6]]
    shape = [int(s) for s in shape]
    if min(n) <= 0:
        return [0] * 6
    if knots is None:
        a = [max(0, lo[i]) for i in range(3)]
        b = [min(shape[i], lo[i] + n[i]) for i in range(3)]
        return [0] * 6 if min(b[i] - a[i] for i in range(3)) <= 0 else a + [b[i] - a[i] for i in range(3)]
    cum = cumulative_length(knots)
    sel, = np.nonzero((cum >= lo[0] - 1) & (cum <= lo[0] + n[0]))
    if len(sel) == 0:
        return [0] * 6
    k0, k1 = max(int(sel[0]) - 1, 0), min(int(sel[-1]) + 1, len(knots) - 1)
    K, B = np.asarray(knots)[k0:k1 + 1], np.asarray(basis)[k0:k1 + 1]
    a = np.array([lo[1], lo[1] + n[1] - 1], dtype=np.float64) - plane[1] / 2      # axis 1 of the straight volume runs along frame vector 2
    b = np.array([lo[2], lo[2] + n[2] - 1], dtype=np.float64) - plane[0] / 2
    corners = K[:, None, None, :] + B[:, None, None, :, 1] * b[None, None, :, None] + B[:, None, None, :, 2] * a[None, :, None, None]
    corners = corners.reshape(-1, 3) / sp
    mn = np.floor(corners.min(0)).astype(np.int64) - pad
    mx = np.ceil(corners.max(0)).astype(np.int64) + pad
    mn = np.maximum(mn, 0)
    mx = np.minimum(mx, np.array(shape) - 1)
    if (mx < mn).any():
        return [0] * 6
    return [int(v) for v in mn] + [int(v) for v in mx - mn + 1]


def _plan_spacing(plan, spacing=None):
    """The spacing a plan was made with (ones for a plan from before plans recorded it); a `spacing` argument has to agree with it."""
    own = check_spacing(plan.get('spacing', (1.0, 1.0, 1.0)))
    if spacing is not None and check_spacing(spacing) != own:
        raise ValueError('spacing %r is not the spacing %r the plan was made with' % (tuple(check_spacing(spacing)), own))
    return own


def restore_patient(plan, crops, shape=None, ct=None, label=None, where='vertebra', return_covered=False, return_local=False, out=None,
                    regions=None, spacing=None, order=None):
    """The way back from the straightened crops to the patient's scan: Interpolator.global_to_local (curve.py:104-150,223-239) for every
    voxel of each vertebra's patient-space box and a resample of the crop there, on the device (csrc/restore.hip), where the reference
    offers the transform one point at a time in Python.
    plan: what straighten_patient(..., return_plan=True) returned.  crops: {vert_id: (ct_vol, label_vol)} device tensors of the size the
    crops were cut at -- float64 / float32 CT in the crops' windowed 0..255 units, uint8 label, any strides; applied in the dict's order.
    ct / label: the patient volumes (the dtypes straighten_patient accepts): the CT output starts as the patient CT under the plan's window
    rule, the label output as the patient label in uint8; without them both start as zeros of `shape`.  out: (ct_out float64, label_out uint8)
    device tensors of the patient's shape (any strides) to start from and write into instead.  regions: {vert_id: [x0, y0, z0, nx, ny, nz]}
    patient-space boxes to visit instead of restore_box's (a region of interest; voxels outside are not touched).
    where = 'crop': every voxel the crop covers is written (trilinear CT sample, nearest label sample); 'vertebra' (needs `label`): only
    where the label sample or the patient's own label is vert_id.  The crop's zero padding never reaches the patient.
    spacing: None = plan['spacing'], the spacing of the scan the plan was made for ((1, 1, 1) for a plan without the entry); a value that
    disagrees with the plan is a ValueError.  The outputs are on the scan's own grid: a box voxel enters the curve math in millimetres.
    order: None = plan['order'] (1 for a plan without the entry); an explicit 1 or 3 overrides it.  3: the CT sample is the cubic B-spline of
    the crop's filled part (map_coordinates order 3 on crop[start : start + len], mirrored at its own edges): one prefilter call per vertebra
    before its restore launch, on the same stream; not clipped, so it may leave the crop's value range.  Labels, the covered mask and the
    local coordinates do not depend on it.  With a single-centroid plan (an integer un-crop) it has no effect.
    -> (ct_out float64, label_out uint8[, covered uint8: 1 where written][, {vert_id: (box, local)}: the patient-space box
    [x0, y0, z0, nx, ny, nz] and the local coordinate of each of its voxels, float64 [nx, ny, nz, 3], NaN where there is none])."""
    if where not in RESTORE:
        raise ValueError("restore: where must be 'crop' or 'vertebra', got %r" % (where,))
    if where == 'vertebra' and label is None:
        raise ValueError("restore: where='vertebra' needs the patient's label volume")
    spacing = _plan_spacing(plan, spacing)
    order = check_order(plan.get('order', 1) if order is None else order)
    crops = dict(crops)
    if not crops:
        raise ValueError('restore: no crop')
    for t in (ct, label) + tuple(out or ()):
        if t is not None:
            if t.dim() != 3:
                raise ValueError('restore: patient volumes are [X, Y, Z], got %s' % (tuple(t.shape),))
            if shape is not None and tuple(t.shape) != tuple(int(s) for s in shape):
                raise ValueError('restore: volume of shape %s where shape=%s was given' % (tuple(t.shape), tuple(shape)))
            shape = tuple(t.shape)
    if shape is None or len(shape) != 3 or min(shape) <= 0:
        raise ValueError('restore: the patient shape is needed (shape=, ct=, label= or out=)')
    shape = tuple(int(s) for s in shape)
    knots, basis = plan['knots'], plan['basis']
    src_shape = shape if knots is None else (len(knots), PLANE[1], PLANE[0])
    # plan['boxes'] has one row per requested id in request order, plan['local'] one entry per distinct id in first-request order: a
    # repeated id repeats its row, so the distinct rows in order are the vertebrae's own
    rows = []
    for b in plan['boxes']:
        b = [int(v) for v in b]
        if len(plan['boxes']) == len(plan['local']) or b not in rows:
            rows.append(b)
    if len(rows) != len(plan['local']):
        raise ValueError('restore: the plan holds %d box rows for %d vertebrae' % (len(rows), len(plan['local'])))
    own_box = dict(zip(plan['local'], rows))
    jobs = []      # every ValueError comes before the first launch (and before the device is asked for)
    for vid, pair in crops.items():
        if vid not in plan['local']:
            raise ValueError('restore: vertebra %r is not in the plan' % (vid,))
        if float(vid) != int(vid) or not 0 <= int(vid) <= 255:
            raise ValueError('restore: vertebra id %r is not an integer in [0, 255]' % (vid,))
        cvol, lvol = pair
        if cvol.dim() != 3 or tuple(cvol.shape) != tuple(lvol.shape) or min(cvol.shape) <= 0:
            raise ValueError('restore: vertebra %r: CT and label crop must be two volumes of one size, got %s and %s'
                             % (vid, tuple(cvol.shape), tuple(lvol.shape)))
        _dtype_code(cvol, (torch.float32, torch.float64), 'crop CT')
        _dtype_code(lvol, (torch.uint8,), 'crop label')
        try:
            box = crop_box(plan['local'][vid], src_shape, tuple(cvol.shape))
        except ValueError:
            box = None
        if box != own_box[vid]:        # the row the vertebra's crop was cut with: another size gives another row
            raise ValueError('restore: vertebra %r: a crop of size %s is not what the plan cut' % (vid, tuple(cvol.shape)))
        region = restore_box(knots, basis, box, shape, spacing=spacing)
        if regions is not None and vid in regions:
            region = [int(v) for v in regions[vid]]
            if len(region) != 6 or any(region[i] < 0 or region[3 + i] < 0 or region[i] + region[3 + i] > shape[i] for i in range(3)):
                raise ValueError('restore: vertebra %r: region %s leaves the volume %s' % (vid, region, shape))
        jobs.append((int(vid), cvol, lvol, box, region))
    dev = jobs[0][1].device
    for _, cvol, lvol, _, _ in jobs:
        _lib.require_gpu(cvol, lvol)
        if cvol.device != dev or lvol.device != dev:
            raise ValueError('restore: crops on different devices')
    _lib.require_gpu(ct, label, *(out or ()))
    if label is not None:
        _dtype_code(label, tuple(_DT), 'label')
        if label.device != dev:
            raise ValueError('restore: label on another device than the crops')
    if ct is not None:
        _dtype_code(ct, _CT_DT, 'CT')
        if ct.device != dev:
            raise ValueError('restore: CT on another device than the crops')
    if out is not None:
        ct_out, lab_out = out
        if ct_out.dtype != torch.float64 or lab_out.dtype != torch.uint8 or ct_out.device != dev or lab_out.device != dev:
            raise ValueError('restore: out must be (float64, uint8) tensors on the device of the crops')
    else:
        if ct is None:
            ct_out = torch.zeros(shape, dtype=torch.float64, device=dev)
        else:       # window(ct_data, -300, 800) (straighten_mask_3d.py:172-184), as the crops were: not hot, plain torch in double
            ct_out = ct.to(torch.float64).contiguous()
            if ct_out.data_ptr() == ct.data_ptr():
                ct_out = ct_out.clone()
            if plan['window']:
                ct_out = (255.0 * (ct_out - WINDOW[0]) / (WINDOW[1] - WINDOW[0])).clamp_(0.0, 255.0)
        lab_out = torch.zeros(shape, dtype=torch.uint8, device=dev) if label is None else label.to(torch.uint8).contiguous()
        if label is not None and lab_out.data_ptr() == label.data_ptr():
            lab_out = lab_out.clone()
    covered = torch.zeros(shape, dtype=torch.uint8, device=dev) if return_covered else None
    L = _lib.get()
    zero3 = [ctypes.c_longlong(0)] * 3
    N = 0
    d_knots = d_basis = d_cum = None
    if knots is not None:
        N = len(knots)
        d_knots = torch.from_numpy(np.ascontiguousarray(knots, dtype=np.float64)).to(dev)
        d_basis = torch.from_numpy(np.ascontiguousarray(basis, dtype=np.float64)).to(dev)
        d_cum = torch.from_numpy(np.ascontiguousarray(cumulative_length(knots), dtype=np.float64)).to(dev)
    local = {}
    for vid, cvol, lvol, box, region in jobs:
        loc = None
        if return_local:
            loc = torch.empty(region[3], region[4], region[5], 3, dtype=torch.float64, device=dev)
            local[vid] = (region, loc)
        if min(region[3:]) <= 0:
            continue
        if order == 3 and knots is not None and min(box[3:6]) > 0:
            sub = cvol[box[6]:box[6] + box[3], box[7]:box[7] + box[4], box[8]:box[8] + box[5]]
            coef = _prefilter(sub, box[3:6], 0, 0.0, 1.0)
            L.call('hv_restore_volume_spline', _lib.ptr(coef), _lib.ptr(lvol), *_strides(lvol), *cvol.shape, (ctypes.c_int * 9)(*box),
                   _lib.ptr(d_knots), _lib.ptr(d_basis), _lib.ptr(d_cum), N, ctypes.c_double(PLANE[0] / 2), ctypes.c_double(PLANE[1] / 2),
                   _lib.ptr(label), 0 if label is None else _DT[label.dtype], *(zero3 if label is None else _strides(label)), *shape,
                   (ctypes.c_int * 6)(*region), RESTORE[where], vid, _lib.ptr(ct_out), *_strides(ct_out), _lib.ptr(lab_out),
                   *_strides(lab_out), _lib.ptr(covered), *(zero3 if covered is None else _strides(covered)), _lib.ptr(loc),
                   (ctypes.c_double * 3)(*spacing), _lib.stream())
            continue
        L.call('hv_restore_volume_sp', _lib.ptr(cvol), _DT[cvol.dtype], *_strides(cvol), _lib.ptr(lvol), *_strides(lvol), *cvol.shape,
               (ctypes.c_int * 9)(*box), _lib.ptr(d_knots), _lib.ptr(d_basis), _lib.ptr(d_cum), N, ctypes.c_double(PLANE[0] / 2),
               ctypes.c_double(PLANE[1] / 2), _lib.ptr(label), 0 if label is None else _DT[label.dtype],
               *(zero3 if label is None else _strides(label)), *shape, (ctypes.c_int * 6)(*region), RESTORE[where], vid, _lib.ptr(ct_out),
               *_strides(ct_out), _lib.ptr(lab_out), *_strides(lab_out), _lib.ptr(covered), *(zero3 if covered is None else _strides(covered)),
               _lib.ptr(loc), (ctypes.c_double * 3)(*spacing), _lib.stream())
    res = (ct_out, lab_out)
    if return_covered:
        res += (covered,)
    if return_local:
        res += (local,)
    return res


# ------------------------------------------------------------------------------------------------ points between the two spaces
CURVE = {'local': 0, 'global': 1}             # HV_CURVE_TO_LOCAL / HV_CURVE_TO_GLOBAL (include/hvgan.h)


def _plan_curve(plan):
    """knots, basis, spacing of a plan: the dictionary straighten_patient(..., return_plan=True) returns, or what plan() returns."""
    if isinstance(plan, Plan):
        return plan[0], plan[1], check_spacing(plan.spacing)
    return plan['knots'], plan['basis'], _plan_spacing(plan)


def _points(plan, points, direction):
    knots, basis, spacing = _plan_curve(plan)
    on_device = isinstance(points, torch.Tensor)
    pts = points if on_device else np.ascontiguousarray(points, dtype=np.float64)
    if pts.ndim != 2 or pts.shape[1] != 3 or pts.shape[0] <= 0 or (on_device and pts.dtype != torch.float64):
        raise ValueError('points: expected [M, 3] float64 with M > 0, got %s %s' % (tuple(pts.shape), pts.dtype))
    if on_device:
        _lib.require_gpu(pts)
    else:
        pts = torch.from_numpy(pts).cuda()
    pts = pts.contiguous()
    if knots is None:               # one centroid: the crops were cut from the raw volume, local is global
        return pts.clone()
    dev = pts.device
    d_knots = torch.from_numpy(np.ascontiguousarray(knots, dtype=np.float64)).to(dev)
    d_basis = torch.from_numpy(np.ascontiguousarray(basis, dtype=np.float64)).to(dev)
    d_cum = torch.from_numpy(np.ascontiguousarray(cumulative_length(knots), dtype=np.float64)).to(dev)
    out = torch.empty_like(pts)
    with torch.cuda.device(dev):
        _lib.get().call('hv_curve_points', _lib.ptr(pts), ctypes.c_longlong(pts.shape[0]), _lib.ptr(d_knots), _lib.ptr(d_basis),
                        _lib.ptr(d_cum), len(knots), ctypes.c_double(PLANE[0] / 2), ctypes.c_double(PLANE[1] / 2),
                        (ctypes.c_double * 3)(*spacing), CURVE[direction], _lib.ptr(out), _lib.stream())
    return out


def points_to_local(plan, points):
    """Interpolator.global_to_local (curve.py:104-108) for a list of points on the device: points [M, 3] float64, voxel indices of the
    patient's scan (a numpy array is uploaded; a device tensor is read where it lies) -> device tensor [M, 3]: (cumulative length along
    the curve, offset along frame vector 1, offset along frame vector 2), the reference's order; the index in the straight volume is
    (row 0, row 2, row 1) and a crop adds its box: crop index = that - box[0:3] + box[6:9].  A row without a finite result is NaN.  With a
    single-centroid plan the points come back unchanged."""
    return _points(plan, points, 'local')


def points_to_global(plan, points):
    """Interpolator.local_to_global (curve.py:110-114) for a list of points on the device: where in the patient's scan (voxel indices, at
    the plan's spacing) a local position lies, for example a column of height_loss_map.  Same conventions as points_to_local, of which it
    is the inverse inside the curve's range."""
    return _points(plan, points, 'global')
