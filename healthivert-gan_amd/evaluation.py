"""Device-side RHLV quantification (reference evaluation/RHLV_quantification.py and evaluation/RHLV_quantification_coronal.py),
SURVEY.md section 8f row f4.

Same entry points as the reference modules, on device tensors:
  calculate_rhlv(segmentation_fake, segmentation_label, center_z, length, vertebra, height_threshold)   (:120-147)
  rhlv_volume(vol_fake, vol_label, label_index, length_divisor, height_threshold)       per-vertebra body of :160-178
each with view='sagittal' (the default: hv_rhlv) or view='coronal' (the coronal script's slicing `[:, z, :]` AND its own arithmetic: rescale
ratios without the sagittal script's + 1e-6, ValueError where it takes max() of an empty third), and for the 2.5D grade
(evaluation/SVM_grading_2.5d.py: Pre / Mid / Post RHLV of both views):
  rhlv_volume_25d(vol_fake, vol_label, label_index, ...)   both views from one pass over the volumes, one readback
  rhlv_dataset(fakes, labels, label_indices, ...)          N pairs of equal shape: one launch sequence per chunk, one readback in all
  svm_features(records, file1='sagittal')                  the six feature columns in SVM_grading_2.5d.py's order
  rhlv_sweep(fakes, labels, label_indices, length_divisors, height_thresholds, ...)   rhlv_dataset at every point of a parameter grid
                                                           (the reference's ParameterGrid tuning) from one pass over each pair
  svm_feature_grid(sweep)                                  the six feature columns at every grid point
and what the reference's README draws from those scripts' per-column heights (the distribution of height loss over the vertebra's
cross-section and the curve of height loss along it), left on the device:
  height_loss_map(vol_fake, vol_label, label_index, ...)       per view: loss / height maps [S, C], flags, column and slice profiles
  height_loss_dataset(fakes, labels, label_indices, ...)       the same stacked over N pairs of equal shape
Volumes are [H, W, Z] tensors (any strides; float32 or uint8) already resident in HBM, e.g. the label volume infer.process_volume
just produced.  The file I/O / Excel part of the reference and the SVM stay on the host.
"""
import ctypes

import numpy as np
import torch

from . import lib as _lib
from . import ops

INT_MIN = -2147483648
SAGITTAL, CORONAL = 1, 2          # HV_RHLV_SAGITTAL, HV_RHLV_CORONAL
VIEWS = {'sagittal': SAGITTAL, 'coronal': CORONAL}
EMPTY_THIRD = ('rhlv (coronal view): a slice of the generated vertebra is too narrow for non-empty pre and mid thirds -- '
               'the reference raises here (max() of an empty array)')


def _prep(v, device):
    t = torch.as_tensor(v)
    if t.dtype not in (torch.float32, torch.uint8):
        t = t.to(torch.float32)
    return t.to(device)


def _pair(fake, label):
    dev = fake.device if isinstance(fake, torch.Tensor) and fake.is_cuda else torch.device('cuda', torch.cuda.current_device())
    f, l = _prep(fake, dev), _prep(label, dev)
    if l.dtype != f.dtype:
        f, l = f.to(torch.float32), l.to(torch.float32)
    _lib.require_gpu(f, l)
    if f.shape != l.shape or f.dim() != 3 or f.stride() != l.stride():
        raise ValueError('rhlv: two [H, W, Z] volumes of equal shape and strides expected')
    return f, l, dev


def _geometry(f):
    """dtype code, strides and shape of a volume as the C entries take them."""
    return (0 if f.dtype == torch.float32 else 1, ctypes.c_longlong(f.stride(0)), ctypes.c_longlong(f.stride(1)), ctypes.c_longlong(f.stride(2)),
            f.shape[0], f.shape[1], f.shape[2])


def _run(fake, label, label_index, length_divisor, z_lo, z_hi, height_threshold):
    L = _lib.get()
    f, l, dev = _pair(fake, label)
    H, W, Z = f.shape
    out = torch.zeros(14, dtype=torch.float64, device=dev)
    need = L.size('hv_rhlv_workspace_bytes', W, Z)
    ws, _ = ops._ws(need, dev, slot=3)
    L.call('hv_rhlv', _lib.ptr(f), _lib.ptr(l), *_geometry(f), ctypes.c_float(label_index), int(length_divisor), int(z_lo), int(z_hi),
           ctypes.c_double(height_threshold), _lib.ptr(out), _lib.ptr(ws), ctypes.c_size_t(ws.numel()), _lib.stream())
    return out


def _view_args(L, views, length_divisor, lo, hi, height_threshold):
    """-> (hv_rhlv_view or None for the sagittal view, the same for the coronal view); height_threshold: one value or a (sagittal, coronal) pair."""
    thr = tuple(height_threshold) if isinstance(height_threshold, (tuple, list)) else (height_threshold, height_threshold)
    return tuple(ctypes.byref(L.hv_rhlv_view(int(length_divisor), int(lo), int(hi), float(t))) if views & bit else None
                 for bit, t in zip((SAGITTAL, CORONAL), thr))


def _run_views(fake, label, label_index, views, length_divisor, lo, hi, height_threshold):
    """hv_rhlv_views -> [views][16] float64 on the device (sagittal first)."""
    L = _lib.get()
    f, l, dev = _pair(fake, label)
    H, W, Z = f.shape
    out = torch.zeros(bin(views).count('1'), 16, dtype=torch.float64, device=dev)
    need = L.size('hv_rhlv_views_workspace_bytes', W, Z, views, 1)
    ws, _ = ops._ws(need, dev, slot=3)
    sag, cor = _view_args(L, views, length_divisor, lo, hi, height_threshold)
    L.call('hv_rhlv_views', _lib.ptr(f), _lib.ptr(l), *_geometry(f), ctypes.c_float(label_index), views, sag, cor, _lib.ptr(out), _lib.ptr(ws),
           ctypes.c_size_t(ws.numel()), _lib.stream())
    return out


def _results(o, return_means):
    """One 14- or 16-double record on the host -> what rhlv_volume returns; ValueError where the reference would have raised."""
    if o[13] == 0:
        return None
    if len(o) > 14 and o[14] != 0:
        raise ValueError(EMPTY_THIRD)
    res = tuple(float(v) for v in o[:5])
    return (res, [float(v) for v in o[5:13]]) if return_means else res


def calculate_rhlv(segmentation_fake, segmentation_label, center_z, length, vertebra=None, height_threshold=0.64, view='sagittal'):
    """-> (all_rhlv, pre_rhlv, mid_rhlv, post_rhlv, relative_height_label): binary volumes, slices [center_z-length, center_z+length)
    along axis 2 (view='sagittal') or axis 1 (view='coronal', the coronal script)."""
    lo, hi = int(center_z) - int(length), int(center_z) + int(length)
    if VIEWS[view] == SAGITTAL:
        o = _run(segmentation_fake, segmentation_label, -1.0, 1, lo, hi, height_threshold).cpu()
    else:
        o = _run_views(segmentation_fake, segmentation_label, -1.0, CORONAL, 1, lo, hi, height_threshold)[0].cpu()
        if o[14] != 0:
            raise ValueError(EMPTY_THIRD)
    return tuple(float(v) for v in o[:5])


def rhlv_volume(vol_fake, vol_label, label_index, length_divisor=5, height_threshold=0.64, return_means=False, view='sagittal'):
    """Label volumes carrying vertebra ids -> the five values of calculate_rhlv for vertebra `label_index`, or None if the original
    volume does not contain it (the reference's `continue`)."""
    if VIEWS[view] == SAGITTAL:
        o = _run(vol_fake, vol_label, float(label_index), length_divisor, INT_MIN, 0, height_threshold).cpu()
    else:
        o = _run_views(vol_fake, vol_label, float(label_index), CORONAL, length_divisor, INT_MIN, 0, height_threshold)[0].cpu()
    return _results(o, return_means)


def rhlv_volume_25d(vol_fake, vol_label, label_index, length_divisor=5, height_threshold=0.64, return_means=False):
    """Both views of rhlv_volume from one pass over the volumes and one readback -> {'sagittal': ..., 'coronal': ...}, or None if the
    original volume does not contain the vertebra.  height_threshold: one value or a (sagittal, coronal) pair."""
    o = _run_views(vol_fake, vol_label, float(label_index), SAGITTAL | CORONAL, length_divisor, INT_MIN, 0, height_threshold).cpu()
    if o[0, 13] == 0:
        return None
    return {'sagittal': _results(o[0], return_means), 'coronal': _results(o[1], return_means)}


def rhlv_dataset(fakes, labels, label_indices, length_divisor=5, height_threshold=0.64, chunk=256):
    """rhlv_volume_25d over N resident volume pairs of equal shape, dtype and strides (lists of device tensors, one vertebra id per pair):
    one launch sequence per `chunk` pairs (hv_rhlv_views_batch), nothing read back until the end.
    -> (records, present): float64 numpy [N, 2, 16] ([:, 0] sagittal, [:, 1] coronal: hv_rhlv_views' records -- five results, eight means,
    vertebra present, "the coronal script would have raised", spare) and bool [N], False where the original lacks the vertebra (the
    reference's `continue`; that row's numbers mean nothing).  Nothing raises per vertebra: check records[:, 1, 14]."""
    L = _lib.get()
    n = len(fakes)
    if n == 0 or len(labels) != n or len(label_indices) != n:
        raise ValueError('rhlv_dataset: equally many (at least one) generated volumes, original volumes and label indices expected')
    dev = fakes[0].device
    geo = (fakes[0].shape, fakes[0].stride(), fakes[0].dtype)
    for t in list(fakes) + list(labels):
        _lib.require_gpu(t)
        if t.dim() != 3 or (t.shape, t.stride(), t.dtype) != geo or t.dtype not in (torch.float32, torch.uint8) or t.device != dev:
            raise ValueError('rhlv_dataset: [H, W, Z] float32 or uint8 device volumes of one shape, dtype and stride pattern expected')
    H, W, Z = geo[0]
    views = SAGITTAL | CORONAL
    table = torch.tensor([p for f, l in zip(fakes, labels) for p in (f.data_ptr(), l.data_ptr())], dtype=torch.int64).to(dev)
    ids = torch.tensor([float(i) for i in label_indices], dtype=torch.float32).to(dev)
    out = torch.zeros(n, 2, 16, dtype=torch.float64, device=dev)
    chunk = max(1, min(int(chunk), n))
    ws, _ = ops._ws(L.size('hv_rhlv_views_workspace_bytes', W, Z, views, chunk), dev, slot=3)
    sag, cor = _view_args(L, views, length_divisor, INT_MIN, 0, height_threshold)
    for i in range(0, n, chunk):
        m = min(chunk, n - i)
        L.call('hv_rhlv_views_batch', _lib.ptr(table[2 * i:]), _lib.ptr(ids[i:]), m, *_geometry(fakes[0]), views, sag, cor, _lib.ptr(out[i:]),
               _lib.ptr(ws), ctypes.c_size_t(ws.numel()), _lib.stream())
    rec = out.cpu().numpy()
    return rec, rec[:, 0, 13] != 0


def svm_features(records, file1='sagittal'):
    """records [N, 2, 16] of rhlv_dataset -> [N, 6]: Pre / Mid / Post RHLV of the view the caller feeds SVM_grading_2.5d.py as `file1`, then the
    other view's (its `_2` columns)."""
    first = 0 if VIEWS[file1] == SAGITTAL else 1
    return np.concatenate([records[:, first, 1:4], records[:, 1 - first, 1:4]], axis=1)


# ---------------------------------------------------------------- parameter sweep (hv_rhlv_sweep)
MAX_DIVISORS, MAX_THRESHOLDS = 16, 32       # HV_RHLV_MAX_DIVISORS, HV_RHLV_MAX_THRESHOLDS: longer grids are split over several calls
SWEEP_WORKSPACE = 1 << 30                   # pairs per launch sequence are limited to this many workspace bytes


def rhlv_sweep(fakes, labels, label_indices, length_divisors=(5,), height_thresholds=(0.64,), views=('sagittal', 'coronal'), chunk=256):
    """rhlv_dataset at every (length_divisor, height_threshold) of a grid from ONE pass over each volume pair (hv_rhlv_sweep): the tuning the
    reference imports sklearn's ParameterGrid for.  fakes / labels: N [H, W, Z] volumes of one shape, dtype and stride pattern (device tensors;
    arrays and host tensors are uploaded), one vertebra id per pair; one launch sequence and one readback per `chunk` pairs.
    -> {'records': float64 numpy [N, D, T, V, 16] (hv_rhlv_views' record per grid point and view, bit for bit rhlv_dataset's at that setting),
        'length_divisors': [D], 'height_thresholds': [T], 'views': the V view names in the records' order (sagittal first),
        'raised': bool numpy [N, D] -- the coronal script would have raised on a slice of that divisor's range (all False without the coronal view)}
    Nothing raises per vertebra or per setting: a sweep reports the settings that are unusable.  records[..., 13] == 0 where the original lacks
    the vertebra."""
    L = _lib.get()
    bits = _view_bits(views)
    names = tuple(v for v in VIEWS if bits & VIEWS[v])
    divs, thrs = [int(d) for d in length_divisors], [float(t) for t in height_thresholds]
    n = len(fakes)
    if n == 0 or len(labels) != n or len(label_indices) != n:
        raise ValueError('rhlv_sweep: equally many (at least one) generated volumes, original volumes and label indices expected')
    if not divs or not thrs or any(d <= 0 for d in divs):
        raise ValueError('rhlv_sweep: at least one length divisor (each > 0) and one height threshold expected')
    first = fakes[0]
    dev = first.device if isinstance(first, torch.Tensor) and first.is_cuda else torch.device('cuda', torch.cuda.current_device())
    fakes, labels = [_prep(t, dev) for t in fakes], [_prep(t, dev) for t in labels]
    geo = (fakes[0].shape, fakes[0].stride(), fakes[0].dtype)
    for t in fakes + labels:
        _lib.require_gpu(t)
        if t.dim() != 3 or (t.shape, t.stride(), t.dtype) != geo or t.device != dev:
            raise ValueError('rhlv_sweep: [H, W, Z] float32 or uint8 volumes of one shape, dtype and stride pattern expected')
    H, W, Z = geo[0]
    D, T, V = len(divs), len(thrs), len(names)
    table = torch.tensor([p for f, l in zip(fakes, labels) for p in (f.data_ptr(), l.data_ptr())], dtype=torch.int64).to(dev)
    ids = torch.tensor([float(i) for i in label_indices], dtype=torch.float32).to(dev)
    chunk = max(1, min(int(chunk), n))
    per_pair = L.size('hv_rhlv_sweep_workspace_bytes', W, Z, bits, 1, min(D, MAX_DIVISORS), min(T, MAX_THRESHOLDS))
    chunk = max(1, min(chunk, SWEEP_WORKSPACE // max(1, per_pair)))
    ws, _ = ops._ws(per_pair * chunk, dev, slot=3)
    records = np.empty((n, D, T, V, 16), dtype=np.float64)
    for i in range(0, n, chunk):
        m = min(chunk, n - i)
        whole = torch.empty(m, D, T, V, 16, dtype=torch.float64, device=dev)
        for d0 in range(0, D, MAX_DIVISORS):
            for t0 in range(0, T, MAX_THRESHOLDS):
                dd, tt = divs[d0:d0 + MAX_DIVISORS], thrs[t0:t0 + MAX_THRESHOLDS]
                grid = L.hv_rhlv_grid(len(dd), (ctypes.c_int * MAX_DIVISORS)(*dd), len(tt), (ctypes.c_double * MAX_THRESHOLDS)(*tt))
                part = whole if (len(dd), len(tt)) == (D, T) else torch.empty(m, len(dd), len(tt), V, 16, dtype=torch.float64, device=dev)
                L.call('hv_rhlv_sweep', _lib.ptr(table[2 * i:]), _lib.ptr(ids[i:]), m, *_geometry(fakes[0]), bits, ctypes.byref(grid),
                       _lib.ptr(part), _lib.ptr(ws), ctypes.c_size_t(ws.numel()), _lib.stream())
                if part is not whole:
                    whole[:, d0:d0 + len(dd), t0:t0 + len(tt)] = part
        records[i:i + m] = whole.cpu().numpy()
    raised = records[:, :, 0, names.index('coronal'), 14] != 0 if 'coronal' in names else np.zeros((n, D), dtype=bool)
    return {'records': records, 'length_divisors': np.array(divs), 'height_thresholds': np.array(thrs), 'views': names, 'raised': raised}


def svm_feature_grid(sweep):
    """rhlv_sweep's result (both views) -> float64 [N, D, T, 6]: svm_features' columns (Pre / Mid / Post RHLV of the sagittal view, then of the
    coronal view) at every grid point; NaN where the coronal script would have raised at that divisor or the original lacks the vertebra."""
    rec, names = np.asarray(sweep['records']), tuple(sweep['views'])
    if set(names) != set(VIEWS):
        raise ValueError('svm_feature_grid: a sweep of both views expected')
    sag, cor = names.index('sagittal'), names.index('coronal')
    feats = np.concatenate([rec[:, :, :, sag, 1:4], rec[:, :, :, cor, 1:4]], axis=-1)
    unusable = np.asarray(sweep['raised'], dtype=bool)[:, :, None] | (rec[:, :, :, sag, 13] == 0)
    feats[unusable] = np.nan
    return feats


# ---------------------------------------------------------------- per-column height-loss maps and profiles (hv_rhlv_maps)
FLAG_REGION, FLAG_SEL_FAKE, FLAG_SEL_LABEL, FLAG_VISITED = 3, 4, 8, 16      # bits of a `flags` element: region 0 pre / 1 mid / 2 post


def _view_bits(views):
    names = (views,) if isinstance(views, str) else tuple(views)
    if not names or len(set(names)) != len(names) or any(v not in VIEWS for v in names):
        raise ValueError("height_loss_map: views must name 'sagittal', 'coronal' or both")
    return sum(VIEWS[v] for v in names)


def _map_buffers(bits, n, W, Z, dev):
    """Output buffers of hv_rhlv_maps(_batch) for n pairs -> ({view: dict of device tensors with a leading [n] axis}, ranges int32 [2, n, 2])."""
    tensors = {}
    ranges = torch.empty(2, n, 2, dtype=torch.int32, device=dev)          # a requested view's rows are always written
    for j, name in enumerate(VIEWS):
        if not bits & VIEWS[name]:
            continue
        S, C = (Z, W) if name == 'sagittal' else (W, Z)
        t = {k: torch.empty(n, S, C, dtype=torch.float64, device=dev) for k in ('loss', 'height_fake', 'height_label')}
        t['flags'] = torch.empty(n, S, C, dtype=torch.uint8, device=dev)
        t['column_profile'] = torch.empty(n, 3, C, dtype=torch.float64, device=dev)
        t['slice_profile'] = torch.empty(n, 3, S, dtype=torch.float64, device=dev)
        t['range'] = ranges[j]
        tensors[name] = t
    return tensors, ranges


def _map_args(L, tensors, i=0):
    """-> the hv_rhlv_map_out of the sagittal and of the coronal view (None where not asked for), writing from pair i on."""
    order = ('loss', 'height_fake', 'height_label', 'flags', 'column_profile', 'slice_profile', 'range')
    return tuple(ctypes.byref(L.hv_rhlv_map_out(*(tensors[name][k][i:].data_ptr() for k in order))) if name in tensors else None
                 for name in VIEWS)


def _map_view(t, i=None):
    """The raw buffers of one view -> the named tensors (pair i of a batch, or the whole [N, ...] stack)."""
    pick = (lambda a: a) if i is None else (lambda a: a[i])
    cp, sp = pick(t['column_profile']), pick(t['slice_profile'])
    return {'loss': pick(t['loss']), 'height_fake': pick(t['height_fake']), 'height_label': pick(t['height_label']), 'flags': pick(t['flags']),
            'profile_fake': cp[..., 0, :], 'profile_label': cp[..., 1, :], 'curve': cp[..., 2, :],
            'slice_profile_fake': sp[..., 0, :], 'slice_profile_label': sp[..., 1, :], 'slice_curve': sp[..., 2, :]}


def _run_maps(fake, label, label_index, views, length_divisor, lo, hi, height_threshold, buffers=None):
    """hv_rhlv_maps -> ([views][16] float64 records, {view: raw output buffers}, ranges), all on the device, nothing read back.
    buffers: (records, tensors, ranges) of an earlier call on the same shapes to write into instead of allocating (tools/bench_rhlv.py)."""
    L = _lib.get()
    f, l, dev = _pair(fake, label)
    H, W, Z = f.shape
    ws, _ = ops._ws(L.size('hv_rhlv_maps_workspace_bytes', W, Z, views, 1), dev, slot=3)
    sag, cor = _view_args(L, views, length_divisor, lo, hi, height_threshold)
    if buffers is None:
        buffers = (torch.zeros(bin(views).count('1'), 16, dtype=torch.float64, device=dev),) + _map_buffers(views, 1, W, Z, dev)
    out, tensors, ranges = buffers
    so, co = _map_args(L, tensors)
    L.call('hv_rhlv_maps', _lib.ptr(f), _lib.ptr(l), *_geometry(f), ctypes.c_float(label_index), views, sag, cor, so, co, _lib.ptr(out), _lib.ptr(ws),
           ctypes.c_size_t(ws.numel()), _lib.stream())
    return out, tensors, ranges


def height_loss_map(vol_fake, vol_label, label_index, length_divisor=5, height_threshold=0.64, views=('sagittal', 'coronal')):
    """The per-column heights behind rhlv_volume / rhlv_volume_25d, from the same single pass over the volumes (hv_rhlv_maps).
    -> {view: {...}, 'records': float64 numpy [len(views), 16]}, or None if the original volume does not contain the vertebra.  Per view, with
    S slices of C columns (sagittal: S = Z, C = W; coronal: S = W, C = Z), all DEVICE tensors -- only the records and the ranges are read back:
      loss, height_fake, height_label   [S, C] float64: height_fake = column count * the slice's whole-slice rescale ratio, height_label = column
                                        count, loss = (height_fake - height_label) / (height_fake + 1e-6) where the script selects the generated
                                        column, NaN elsewhere; a slice the script does not visit is NaN / 0
      flags                             [S, C] uint8: FLAG_REGION bits (0 pre, 1 mid, 2 post), FLAG_SEL_FAKE, FLAG_SEL_LABEL, FLAG_VISITED
      profile_fake, profile_label, curve                           [C]: mean selected height per column over the slices, and its relative loss
      slice_profile_fake, slice_profile_label, slice_curve         [S]: the same per slice over its columns
      range                             (lo, hi): the slices the script walks
    The selected height_fake (height_label) of a whole map average to the view's record [5] ([6]), the means rhlv_volume reports.
    height_threshold: one value or a (sagittal, coronal) pair.  ValueError where the coronal script would have raised."""
    out, tensors, ranges = _run_maps(vol_fake, vol_label, float(label_index), _view_bits(views), length_divisor, INT_MIN, 0, height_threshold)
    rec = out.cpu().numpy()
    if rec[0, 13] == 0:
        return None
    if np.any(rec[:, 14] != 0):
        raise ValueError(EMPTY_THIRD)
    ranges = ranges.cpu()
    res = {'records': rec}
    for j, name in enumerate(VIEWS):
        if name in tensors:
            res[name] = _map_view(tensors[name], 0)
            res[name]['range'] = (int(ranges[j, 0, 0]), int(ranges[j, 0, 1]))
    return res


def height_loss_dataset(fakes, labels, label_indices, length_divisor=5, height_threshold=0.64, views=('sagittal', 'coronal'), chunk=256):
    """height_loss_map over N resident volume pairs of equal shape, dtype and strides (the batched form beside rhlv_dataset): one launch sequence
    per `chunk` pairs (hv_rhlv_maps_batch).  -> {view: height_loss_map's tensors stacked to [N, ...] on the device ('range': int32 [N, 2]),
    'records': float64 numpy [N, len(views), 16], 'present': bool numpy [N]}.  present is False where the original lacks the vertebra (that
    pair's rows are NaN / 0); nothing raises per vertebra: check records[:, -1, 14] for the coronal view.  The maps take 25 bytes per column
    of every slice, view and pair."""
    L = _lib.get()
    bits = _view_bits(views)
    n = len(fakes)
    if n == 0 or len(labels) != n or len(label_indices) != n:
        raise ValueError('height_loss_dataset: equally many (at least one) generated volumes, original volumes and label indices expected')
    dev = fakes[0].device
    geo = (fakes[0].shape, fakes[0].stride(), fakes[0].dtype)
    for t in list(fakes) + list(labels):
        _lib.require_gpu(t)
        if t.dim() != 3 or (t.shape, t.stride(), t.dtype) != geo or t.dtype not in (torch.float32, torch.uint8) or t.device != dev:
            raise ValueError('height_loss_dataset: [H, W, Z] float32 or uint8 device volumes of one shape, dtype and stride pattern expected')
    H, W, Z = geo[0]
    nv = bin(bits).count('1')
    table = torch.tensor([p for f, l in zip(fakes, labels) for p in (f.data_ptr(), l.data_ptr())], dtype=torch.int64).to(dev)
    ids = torch.tensor([float(i) for i in label_indices], dtype=torch.float32).to(dev)
    out = torch.zeros(n, nv, 16, dtype=torch.float64, device=dev)
    chunk = max(1, min(int(chunk), n))
    ws, _ = ops._ws(L.size('hv_rhlv_maps_workspace_bytes', W, Z, bits, chunk), dev, slot=3)
    sag, cor = _view_args(L, bits, length_divisor, INT_MIN, 0, height_threshold)
    tensors, _ = _map_buffers(bits, n, W, Z, dev)
    for i in range(0, n, chunk):
        m = min(chunk, n - i)
        so, co = _map_args(L, tensors, i)
        L.call('hv_rhlv_maps_batch', _lib.ptr(table[2 * i:]), _lib.ptr(ids[i:]), m, *_geometry(fakes[0]), bits, sag, cor, so, co,
               _lib.ptr(out[i:]), _lib.ptr(ws), ctypes.c_size_t(ws.numel()), _lib.stream())
    rec = out.cpu().numpy()
    res = {'records': rec, 'present': rec[:, 0, 13] != 0}
    for name in tensors:
        res[name] = _map_view(tensors[name])
        res[name]['range'] = tensors[name]['range']
    return res
