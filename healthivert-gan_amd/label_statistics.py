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
from . import labelled as _lb
from .labelled import MAX_LABELS  # noqa: F401  (HV_LS_MAX_LABELS; the label protocol's)

REC, MAX_Q = 32, 8                                                     # HV_LS_REC, HV_LS_MAX_Q of include/hvgan.h
COUNT, SUM, SUMSQ, MIN, MAX, COORD, LO, HI, STATUS, ORDER = 0, 1, 2, 3, 4, 5, 8, 11, 14, 16
BAD_LABEL, NONFINITE, EMPTY = 1, 2, 4                                  # HV_LS_* status bits
_INTEGER = (torch.uint8, torch.int16)


def _check_percentiles(percentiles):
    try:
        q = [float(p) for p in percentiles]
    except (TypeError, ValueError):
        raise ValueError('percentiles: a sequence of numbers in [0, 100] expected, got %r' % (percentiles,))
    if len(q) > MAX_Q or not all(math.isfinite(p) and 0.0 <= p <= 100.0 for p in q):
        raise ValueError('percentiles: at most %d numbers in [0, 100] expected, got %r' % (MAX_Q, percentiles))
    return q


def _launch(vol, label, mask, labels, q, out):
    """Queue one hv_label_stats on the current stream: 4-D device tensors (mask may be None), out a float64 device tensor [V][S][REC]."""
    Q = len(q)
    ws, wsz = _lb.workspace('label_stats', vol, len(labels), Q, who='label_statistics')
    _lib.get().call('hv_label_stats', *_lb.volume_args(vol, label, mask, labels), (ctypes.c_double * max(Q, 1))(*q), Q, _lib.ptr(out), _lib.ptr(ws),
                    wsz, _lib.stream())
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


def present(vol, label, mask):
    """The non-zero label values with a counted voxel in any volume: four count-only calls (64 values each), one readback of the counts."""
    out = torch.empty((4, vol.shape[0], MAX_LABELS, REC), dtype=torch.float64, device=vol.device)
    for g in range(4):
        _launch(vol, label, mask, list(range(64 * g, 64 * g + 64)), [], out[g])
    cnt = out[..., COUNT].sum(dim=1).reshape(-1).cpu().numpy()
    return [int(l) for l in np.nonzero(cnt)[0] if l != 0]


def _records(vol, label, labels, q, mask):
    out = torch.empty((vol.shape[0], len(labels), REC), dtype=torch.float64, device=vol.device)
    return _launch(vol, label, mask, labels, q, out)


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
    sp = _lb.check_spacing(spacing)
    single, v4, l4, m4 = _lb.check_inputs(vol, label, mask)
    ls = _lb.resolve_labels(labels, lambda: present(v4, l4, m4))
    rec = _records(v4, l4, ls, q, m4).cpu().numpy()
    res = stats_from_records(rec, vol.dtype in _INTEGER, ls, q, tuple(v4.shape[1:]), sp)
    return _lb.squeeze(res) if single else res


def _one(res, v, s):
    """The statistics of slot s of volume v as scalars / small arrays."""
    return {k: (res[k][v][s] if k != 'labels' else int(res[k][s])) for k in res}


def vertebra_density(ct, label, vert_id, erode_mm=0.0, spacing=(1, 1, 1), percentiles=(5, 50, 95), median_size=None):
    """The statistics of one vertebra's cancellous core: label_statistics of `ct` inside label == vert_id, under the mask
    morphology.binary_erosion(label == vert_id, ball(erode_mm, spacing), border_value=0) (erode_mm = 0: no morphology runs, no mask).
    median_size (an integer or one per axis): the statistics are those of rank_filters.median_filter(ct, size=median_size), the usual pre-step
    against salt-and-pepper noise (None: no filter runs).
    -> the dict of label_statistics for that one label (scalars; percentiles [Q])."""
    ct, label, mask, vid, sp = _lb.vertebra_inputs(ct, label, vert_id, erode_mm, spacing, median_size, upload=False)
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
    pair = _lb.Pair(label_original, label_synth, [vert_id] + list(neighbours), ct_original, ct_synth, erode_mm, spacing, upload=False)
    ids, sp, shape, q = pair.ids, pair.spacing, pair.shape, [5.0, 50.0, 95.0]
    out = torch.empty((2, len(ids), REC), dtype=torch.float64, device=pair.device)
    pair.launch(lambda vol, label, mask, sel: _launch(vol, label, mask, ids, q, out[sel]))
    res = stats_from_records(out.cpu().numpy(), pair.dtype in _INTEGER, ids, q, shape, sp)
    ori, syn = _one(res, 0, 0), _one(res, 1, 0)
    nb = {i: _one(res, 0, s) for s, i in enumerate(ids) if s > 0}
    return {'original': ori, 'synthesized': syn, 'neighbours': nb,
            'mean_difference': syn['mean'] - ori['mean'], 'median_difference': syn['percentiles'][1] - ori['percentiles'][1],
            'neighbour_mean_difference': {i: syn['mean'] - d['mean'] for i, d in nb.items()},
            'neighbour_median_difference': {i: syn['percentiles'][1] - d['percentiles'][1] for i, d in nb.items()}}

