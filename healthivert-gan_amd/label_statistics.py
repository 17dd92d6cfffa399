"""Per-label intensity statistics and percentiles on the device (csrc/labelstats.hip through hv_label_stats).

What intensities does a (synthesized) vertebra have, per vertebra, and how do they compare with the original and with its neighbours?  The
definitions are scipy.ndimage.sum_labels / mean / variance / minimum / maximum / center_of_mass / find_objects and np.percentile (linear), on
volumes that stay resident; one readback of 256 bytes per (volume, label):
  label_statistics(vol, label, labels=None, percentiles=(), mask=None, spacing=(1, 1, 1))         -> dict of arrays [V][S] ([S] for one volume)
  vertebra_density(ct, label, vert_id, erode_mm=0.0, spacing=(1, 1, 1), percentiles=(5, 50, 95), median_size=None)
                                                                                                   one vertebra's cancellous core
  density_comparison(ct_original, ct_synth, label_original, label_synth, vert_id, neighbours=(), erode_mm=0.0, spacing=(1, 1, 1))
vol: a device tensor [A0][A1][A2] or a stacked [V][A0][A1][A2], any strides, uint8 / int16 / float32 / float64.  label: the same shape, its own
strides, uint8 / int16 / int32 / int64 / float32 / float64 holding integers in [0, 255].  mask: uint8 or bool of the same shape, a voxel counts
where it is non-zero.  Nothing falls back to the host: a CPU tensor is a ValueError, anything that is not a tensor a TypeError.

The device returns exact integers and the two order statistics around each percentile; this module derives, in float64 on the host, mean and
population variance (integer dtypes: from the exact integer sums in Python integers; float dtypes: from the two sums in rational arithmetic,
so nothing is lost beyond the sums' own rounding) and the percentile by numpy's linear rule, `_lerp` with its t >= 0.5 branch included."""
import ctypes
import math
from fractions import Fraction

import numpy as np
import torch

from . import lib as _lib
from . import ops

REC, MAX_LABELS, MAX_Q = 32, 64, 8                                     # HV_LS_REC, HV_LS_MAX_LABELS, HV_LS_MAX_Q of include/hvgan.h
COUNT, SUM, SUMSQ, MIN, MAX, COORD, LO, HI, STATUS, ORDER = 0, 1, 2, 3, 4, 5, 8, 11, 14, 16
BAD_LABEL, NONFINITE, EMPTY = 1, 2, 4                                  # HV_LS_* status bits
_VOL_DT = {torch.uint8: 0, torch.int16: 1, torch.float32: 4, torch.float64: 5}
_LABEL_DT = {torch.uint8: 0, torch.int16: 1, torch.int32: 2, torch.int64: 3, torch.float32: 4, torch.float64: 5}
_INTEGER = (torch.uint8, torch.int16)


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


def _check_percentiles(percentiles):
    try:
        q = [float(p) for p in percentiles]
    except (TypeError, ValueError):
        raise ValueError('percentiles: a sequence of numbers in [0, 100] expected, got %r' % (percentiles,))
    if len(q) > MAX_Q or not all(math.isfinite(p) and 0.0 <= p <= 100.0 for p in q):
        raise ValueError('percentiles: at most %d numbers in [0, 100] expected, got %r' % (MAX_Q, percentiles))
    return q


def _check_labels(labels):
    try:
        ls = [int(x) for x in labels]
        same = all(float(x) == int(x) for x in labels)
    except (TypeError, ValueError):
        ls, same = [], False
    if not same or not 1 <= len(ls) <= MAX_LABELS or len(set(ls)) != len(ls) or not all(0 <= x <= 255 for x in ls):
        raise ValueError('labels: 1 to %d distinct integers in [0, 255] expected, got %r' % (MAX_LABELS, labels))
    return ls


def _check_tensor(t, name, table, shape=None):
    if not isinstance(t, torch.Tensor):
        raise TypeError('%s: a device tensor expected, got %s (nothing is uploaded or computed on the host here)' % (name, type(t).__name__))
    if not t.is_cuda:
        raise ValueError('%s: a device tensor expected, got a %s tensor; there is no CPU path' % (name, t.device))
    if t.dtype not in table:
        raise TypeError('%s: dtype %s expected, got %s' % (name, ' / '.join(str(d).replace('torch.', '') for d in table), t.dtype))
    if shape is None:
        if t.dim() not in (3, 4) or t.numel() == 0:
            raise ValueError('%s: a non-empty [A0][A1][A2] volume or a stacked [V][A0][A1][A2] batch expected, got shape %s' % (name, tuple(t.shape)))
    elif tuple(t.shape) != tuple(shape):
        raise ValueError('%s: shape %s expected (the volume\'s), got %s' % (name, tuple(shape), tuple(t.shape)))
    return t


def _ll(strides):
    return [ctypes.c_longlong(s) for s in strides]


def _as4(t):
    return t if t.dim() == 4 else t.unsqueeze(0)


def _launch(vol, label, mask, labels, q, out):
    """Queue one hv_label_stats on the current stream: 4-D device tensors (mask may be None), out a float64 device tensor [V][S][REC]."""
    L = _lib.get()
    V, A0, A1, A2 = (int(s) for s in vol.shape)
    S, Q = len(labels), len(q)
    need = L.size('hv_label_stats_workspace_bytes', V, A0, A1, A2, S, Q)
    if need == 0:
        raise ValueError('label_statistics: at most 2^30 voxels per volume and 65535 volumes per call, got shape %s' % (tuple(vol.shape),))
    ws, wsz = ops._ws(need, vol.device, slot=3)
    mst = mask.stride() if mask is not None else (0, 0, 0, 0)
    L.call('hv_label_stats', _lib.ptr(vol), _VOL_DT[vol.dtype], *_ll(vol.stride()), _lib.ptr(label), _LABEL_DT[label.dtype], *_ll(label.stride()),
           _lib.ptr(mask), *_ll(mst), V, A0, A1, A2, (ctypes.c_int * S)(*labels), S, (ctypes.c_double * max(Q, 1))(*q), Q, _lib.ptr(out),
           _lib.ptr(ws), wsz, _lib.stream())
    return out


def _lerp(a, b, t):
    """numpy's _lerp for float64 scalars: a + (b - a) t, and b - (b - a) (1 - t) once t >= 0.5."""
    a, b, t = np.float64(a), np.float64(b), np.float64(t)
    diff = b - a
    return b - diff * (np.float64(1.0) - t) if t >= 0.5 else a + diff * t


def percentile_from_order(n, q, lo, hi):
    """np.percentile(x, q) (linear) from n = len(x) and the order statistics x[floor(vi)], x[floor(vi) + 1] (both x[n - 1] once vi >= n - 1)
    with numpy's virtual index vi = (n - 1) * (q / 100)."""
    vi = np.float64(int(n) - 1) * np.true_divide(np.float64(q), np.float64(100))
    return _lerp(lo, hi, vi - np.floor(vi))


def stats_from_records(rec, integer, labels, percentiles=(), shape=(1, 1, 1), spacing=(1, 1, 1)):
    """The host half: the dict of label_statistics from the device records rec [V][S][REC] (float64; `integer`: the sums are int64 bit patterns)."""
    rec = np.ascontiguousarray(rec, dtype=np.float64)
    V, S = rec.shape[:2]
    q = list(percentiles)
    sp = np.asarray(spacing, dtype=np.float64)
    raw = rec.view(np.int64)
    nan = float('nan')
    out = {
        'labels': np.asarray(labels, dtype=np.int64),
        'count': rec[..., COUNT].astype(np.int64),
        'status': rec[..., STATUS].astype(np.int64),
        'box': np.stack([rec[..., LO:LO + 3], rec[..., HI:HI + 3]], axis=2).astype(np.int64),
    }
    out['volume_mm3'] = out['count'].astype(np.float64) * float(np.prod(sp))
    for k in ('sum', 'mean', 'variance', 'std', 'min', 'max'):
        out[k] = np.full((V, S), nan)
    out['centroid'] = np.full((V, S, 3), nan)
    out['percentiles'] = np.full((V, S, len(q)), nan)
    out['unusable'] = [[None] * S for _ in range(V)]
    out['box_slices'] = [[None] * S for _ in range(V)]
    for v in range(V):
        for s in range(S):
            n, st = int(out['count'][v, s]), int(out['status'][v, s])
            if n == 0:
                out['unusable'][v][s] = 'no voxel of label %d is counted' % out['labels'][s]
                continue
            out['centroid'][v, s] = rec[v, s, COORD:COORD + 3] / np.float64(n)
            out['box_slices'][v][s] = tuple(slice(int(lo), int(hi) + 1) for lo, hi in zip(out['box'][v, s, 0], out['box'][v, s, 1]))
            if st & NONFINITE:
                out['unusable'][v][s] = 'a NaN or infinite value lies inside label %d' % out['labels'][s]
                continue
            if integer:
                sv, svv = int(raw[v, s, SUM]), int(raw[v, s, SUMSQ])
                out['sum'][v, s] = float(sv)
                out['mean'][v, s] = sv / n
                out['variance'][v, s] = (n * svv - sv * sv) / (n * n)
            else:
                sv, svv = rec[v, s, SUM], rec[v, s, SUMSQ]
                out['sum'][v, s] = sv
                if math.isfinite(sv) and math.isfinite(svv):
                    out['mean'][v, s] = sv / np.float64(n)
                    out['variance'][v, s] = max(float(Fraction(float(svv)) / n - (Fraction(float(sv)) / n) ** 2), 0.0)
                else:                                          # finite values whose sum or squares overflow a double
                    out['unusable'][v][s] = 'the sums of label %d overflow a double' % out['labels'][s]
            out['std'][v, s] = math.sqrt(out['variance'][v, s]) if out['variance'][v, s] == out['variance'][v, s] else nan
            out['min'][v, s], out['max'][v, s] = rec[v, s, MIN], rec[v, s, MAX]
            for t, p in enumerate(q):
                out['percentiles'][v, s, t] = percentile_from_order(n, p, rec[v, s, ORDER + 2 * t], rec[v, s, ORDER + 2 * t + 1])
    out['centroid_mm'] = out['centroid'] * sp
    return out


def _squeeze(res):
    """The [V = 1] axis dropped: what a single volume's caller gets."""
    return {k: (v[0] if k != 'labels' else v) for k, v in res.items()}


def _present(vol, label, mask):
    """The non-zero label values with a counted voxel in any volume: four count-only calls (64 values each), one readback of the counts."""
    out = torch.empty((4, vol.shape[0], MAX_LABELS, REC), dtype=torch.float64, device=vol.device)
    for g in range(4):
        _launch(vol, label, mask, list(range(64 * g, 64 * g + 64)), [], out[g])
    cnt = out[..., COUNT].sum(dim=1).reshape(-1).cpu().numpy()
    return [int(l) for l in np.nonzero(cnt)[0] if l != 0]


def _records(vol, label, labels, q, mask):
    out = torch.empty((vol.shape[0], len(labels), REC), dtype=torch.float64, device=vol.device)
    return _launch(vol, label, mask, labels, q, out)


def _check_inputs(vol, label, mask):
    _check_tensor(vol, 'vol', _VOL_DT)
    _check_tensor(label, 'label', _LABEL_DT, vol.shape)
    if mask is not None:
        _check_tensor(mask, 'mask', (torch.uint8, torch.bool), vol.shape)
        if mask.dtype == torch.bool:
            mask = mask.view(torch.uint8)
    if label.device != vol.device or (mask is not None and mask.device != vol.device):
        raise ValueError('vol, label and mask must lie on one device')
    return _as4(vol), _as4(label), None if mask is None else _as4(mask)


def label_statistics(vol, label, labels=None, percentiles=(), mask=None, spacing=(1, 1, 1)):
    """Statistics of `vol` inside every listed label value (up to 64) of `label`, restricted to mask != 0: a dict of numpy arrays [V][S] (one 3-D
    volume: [S]) -- labels, count, volume_mm3 (count * prod(spacing)), sum, mean, variance (population, np.var), std, min, max, centroid and
    centroid_mm [..][3], box [..][2][3] (lo, hi inclusive; an absent label: lo = the extents, hi = -1) and box_slices (find_objects' slices or
    None), percentiles [..][Q] (np.percentile, linear; up to 8), status (bit 0: the volume holds a label that is no integer in [0, 255], bit 1:
    a NaN or infinity inside the label, bit 2: no voxel) and unusable (None, or why the floating results of the slot are NaN).  An absent label
    gives count 0 and NaN, without a warning.  One launch sequence and one readback for the whole batch.
    labels=None: the non-zero label values present anywhere in the batch (under the mask); this costs four count-only passes over the volumes and
    one extra readback of 256 counts per volume.  ValueError if none or more than 64 are present."""
    q = _check_percentiles(percentiles)
    sp = _check_spacing(spacing)
    single = isinstance(vol, torch.Tensor) and vol.dim() == 3
    v4, l4, m4 = _check_inputs(vol, label, mask)
    if labels is None:
        ls = _present(v4, l4, m4)
        if not 1 <= len(ls) <= MAX_LABELS:
            raise ValueError('labels=None: 1 to %d non-zero label values expected in the volumes, found %d' % (MAX_LABELS, len(ls)))
    else:
        ls = _check_labels(labels)
    rec = _records(v4, l4, ls, q, m4).cpu().numpy()
    res = stats_from_records(rec, vol.dtype in _INTEGER, ls, q, tuple(v4.shape[1:]), sp)
    return _squeeze(res) if single else res


def _core_mask(label, vert_ids, erode_mm, sp, out):
    """The union over vert_ids of binary_erosion(label == id, ball(erode_mm, spacing), border_value=0) into the uint8 device volume `out`: inside
    label == id it IS that label's erosion, since an erosion never leaves its set."""
    from . import morphology
    tmp = None
    for n, vid in enumerate(vert_ids):
        if n == 0:
            morphology.binary_erosion(label, value=vid, radius=erode_mm, spacing=sp, border_value=0, out=out)
        else:
            tmp = morphology.binary_erosion(label, value=vid, radius=erode_mm, spacing=sp, border_value=0, out=tmp)
            out |= tmp
    return out


def _check_erode(erode_mm):
    if isinstance(erode_mm, bool) or not isinstance(erode_mm, (int, float, np.integer, np.floating)) or not (math.isfinite(erode_mm) and erode_mm >= 0):
        raise ValueError('erode_mm: a non-negative finite number expected, got %r' % (erode_mm,))
    return float(erode_mm)


def _check_3d(t, name, table, shape=None):
    _check_tensor(t, name, table, shape)
    if t.dim() != 3:
        raise ValueError('%s: one [A0][A1][A2] volume expected, got shape %s' % (name, tuple(t.shape)))
    return t


def _one(res, v, s):
    """The statistics of slot s of volume v as scalars / small arrays."""
    return {k: (res[k][v][s] if k != 'labels' else int(res[k][s])) for k in res}


def vertebra_density(ct, label, vert_id, erode_mm=0.0, spacing=(1, 1, 1), percentiles=(5, 50, 95), median_size=None):
    """The statistics of one vertebra's cancellous core: label_statistics of `ct` inside label == vert_id, under the mask
    morphology.binary_erosion(label == vert_id, ball(erode_mm, spacing), border_value=0) (erode_mm = 0: no morphology runs, no mask).
    median_size (an integer or one per axis): the statistics are those of rank_filters.median_filter(ct, size=median_size), the usual pre-step
    against salt-and-pepper noise (None: no filter runs).
    -> the dict of label_statistics for that one label (scalars; percentiles [Q])."""
    sp = _check_spacing(spacing)
    r = _check_erode(erode_mm)
    vid = _check_labels([vert_id])[0]
    _check_3d(ct, 'ct', _VOL_DT)
    _check_3d(label, 'label', _LABEL_DT, ct.shape)
    if median_size is not None:
        from . import rank_filters
        ct = rank_filters.median_filter(ct, size=median_size)
    mask = None
    if r > 0.0:
        mask = _core_mask(label, [vid], r, sp, torch.empty(tuple(label.shape), dtype=torch.uint8, device=label.device))
    res = label_statistics(ct, label, [vid], percentiles, mask, sp)
    return {k: (res[k][0] if k != 'labels' else int(res[k][0])) for k in res}


def density_comparison(ct_original, ct_synth, label_original, label_synth, vert_id, neighbours=(), erode_mm=0.0, spacing=(1, 1, 1)):
    """Does the pseudo-healthy vertebra have the attenuation of the patient's intact ones?  The statistics (percentiles 5, 50, 95) of vertebra
    vert_id in the original CT under the original label, in the synthesized CT under the synthesized label, and of every listed neighbour in the
    original CT under the original label, each inside its core (erode_mm as in vertebra_density).
    -> {'original', 'synthesized': dicts as vertebra_density's, 'neighbours': {id: dict}, 'mean_difference', 'median_difference' (synthesized -
    original), 'neighbour_mean_difference', 'neighbour_median_difference': {id: synthesized - neighbour}}.
    The two pairs run as ONE batch (V = 2, the second volume addressed through the batch stride, no copy) when the CTs agree in dtype and
    strides and the labels do, else as two calls into one result buffer; one readback either way."""
    sp = _check_spacing(spacing)
    r = _check_erode(erode_mm)
    ids = _check_labels([vert_id] + list(neighbours))
    _check_3d(ct_original, 'ct_original', _VOL_DT)
    _check_3d(ct_synth, 'ct_synth', _VOL_DT, ct_original.shape)
    _check_3d(label_original, 'label_original', _LABEL_DT, ct_original.shape)
    _check_3d(label_synth, 'label_synth', _LABEL_DT, ct_original.shape)
    if ct_synth.dtype != ct_original.dtype:
        raise TypeError('ct_synth: the dtype of ct_original (%s) expected, got %s' % (ct_original.dtype, ct_synth.dtype))
    dev, shape = ct_original.device, tuple(ct_original.shape)
    q = [5.0, 50.0, 95.0]
    masks = None
    if r > 0.0:
        masks = torch.empty((2,) + shape, dtype=torch.uint8, device=dev)
        _core_mask(label_original, ids, r, sp, masks[0])
        _core_mask(label_synth, ids[:1], r, sp, masks[1])
    out = torch.empty((2, len(ids), REC), dtype=torch.float64, device=dev)

    def batch_stride(a, b):
        """b's distance from a in elements if the pair can be addressed as a [2][...] batch, else None."""
        d = b.data_ptr() - a.data_ptr()
        ok = a.dtype == b.dtype and a.stride() == b.stride() and d % a.element_size() == 0
        return d // a.element_size() if ok else None

    cs, lsd = batch_stride(ct_original, ct_synth), batch_stride(label_original, label_synth)
    if cs is not None and lsd is not None:
        _launch(_Strided(ct_original, cs), _Strided(label_original, lsd), masks, ids, q, out)
    else:
        _launch(ct_original[None], label_original[None], None if masks is None else masks[0:1], ids, q, out[0:1])
        _launch(ct_synth[None], label_synth[None], None if masks is None else masks[1:2], ids, q, out[1:2])
    res = stats_from_records(out.cpu().numpy(), ct_original.dtype in _INTEGER, ids, q, shape, sp)
    ori, syn = _one(res, 0, 0), _one(res, 1, 0)
    nb = {i: _one(res, 0, s) for s, i in enumerate(ids) if s > 0}
    return {'original': ori, 'synthesized': syn, 'neighbours': nb,
            'mean_difference': syn['mean'] - ori['mean'], 'median_difference': syn['percentiles'][1] - ori['percentiles'][1],
            'neighbour_mean_difference': {i: syn['mean'] - d['mean'] for i, d in nb.items()},
            'neighbour_median_difference': {i: syn['percentiles'][1] - d['percentiles'][1] for i, d in nb.items()}}


class _Strided:
    """Two separate 3-D allocations of one dtype and stride triple addressed as a [2][...] batch: the batch stride is their distance."""

    def __init__(self, t, batch_stride):
        self.t, self.bs = t, batch_stride
        self.shape, self.dtype, self.device = (2,) + tuple(t.shape), t.dtype, t.device

    def stride(self):
        return (self.bs,) + tuple(self.t.stride())

    def data_ptr(self):
        return self.t.data_ptr()
