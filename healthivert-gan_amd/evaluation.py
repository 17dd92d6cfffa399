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
  svm_grade_grid(features, labels, dataset, ...)           the reference's grading (SVM_grading.py / SVM_grading_2.5d.py: scaler, 5-fold linear SVM,
                                                           val-set scores) of every grid point in one launch sequence (hv_svm_grade_grid)
  stratified_folds(y)                                      the unshuffled StratifiedKFold assignment the grading uses (host, labels only)
  best_setting(sweep, grades, score='f1')                  the (length_divisor, height_threshold) with the best mean score
  svm_fit(features, labels, train=None, ...)               the grader svm_grade_grid scores, fitted on chosen rows and KEPT (hv_svm_fit)
  svm_predict(model, features, ...)                        grades, decisions, votes and per-feature contributions of new rows (hv_svm_predict)
  fit_grader(sweep, labels, dataset, ...) -> Grader        the grader at the best (or a given) setting; Grader.grade_dataset goes from resident
                                                           volumes to grades on the device with one readback (the reference stops at the fold scores)
and what the reference's README draws from those scripts' per-column heights (the distribution of height loss over the vertebra's
cross-section and the curve of height loss along it), left on the device:
  height_loss_map(vol_fake, vol_label, label_index, ...)       per view: loss / height maps [S, C], flags, column and slice profiles
  height_loss_dataset(fakes, labels, label_indices, ...)       the same stacked over N pairs of equal shape
Volumes are [H, W, Z] tensors (any strides; float32 or uint8) already resident in HBM, e.g. the label volume infer.process_volume
just produced.  The file I/O / Excel part of the reference stays on the host.
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


# ---------------------------------------------------------------- SVM grading of every grid point (hv_svm_grade_grid)
N_SPLITS, MAX_CLASSES, MAX_PAIR_ROWS, MAX_GRID = 5, 4, 1792, 65535    # HV_SVM_FOLDS, HV_SVM_MAX_CLASSES, HV_SVM_MAX_ROWS, the launch grid's z extent
CONVERGED, HIT_MAX_ITER, PAIR_ABSENT, UNUSABLE, BAD_PLAN = 0, 1, 2, 3, 4   # HV_SVM_*: a problem's status
SCORES = ('f1', 'precision', 'recall', 'accuracy')


def stratified_folds(y, n_splits=N_SPLITS):
    """The test fold of every row under scikit-learn 1.7.2's unshuffled StratifiedKFold(n_splits): the classes are numbered in order of first
    appearance, the sorted labels dealt to the folds round robin give the number of rows of every class per fold, and a class's rows take
    their folds in contiguous blocks of those sizes.  Depends on the labels only.  -> int32 [len(y)]"""
    y = np.asarray(y)
    if y.ndim != 1 or len(y) == 0:
        raise ValueError('stratified_folds: a non-empty vector of labels expected')
    _, first, inverse = np.unique(y, return_index=True, return_inverse=True)
    encoded = np.argsort(np.argsort(first))[inverse]
    counts = np.bincount(encoded)
    if np.all(n_splits > counts):
        raise ValueError('stratified_folds: n_splits=%d cannot be greater than the number of members in each class' % n_splits)
    order = np.sort(encoded)
    allocation = np.array([np.bincount(order[i::n_splits], minlength=len(first)) for i in range(n_splits)])
    folds = np.empty(len(y), dtype=np.int32)
    for k in range(len(first)):
        folds[encoded == k] = np.arange(n_splits).repeat(allocation[:, k])
    return folds


def svm_grade_grid(features, labels, dataset, folds=None, tol=1e-3, max_iter=100000, decisions=False):
    """The reference's grading (evaluation/SVM_grading.py with three feature columns, SVM_grading_2.5d.py with six) of EVERY grid point of a
    sweep on the device: StandardScaler fitted on the train + test rows, SVC(kernel='linear', class_weight='balanced') with tolerance `tol`
    (libsvm's 1e-3), StratifiedKFold(5), each fold's model applied to the val rows, confusion matrix and macro F1 / precision / recall /
    accuracy per fold, their mean and np.var over the folds.
    features [N, G..., F] (svm_feature_grid's [N, D, T, 6]; its first three columns alone reproduce SVM_grading.py), labels [N] small
    non-negative integer grades (at most 4 different ones), dataset [N] of 'train' / 'test' / 'val', folds: the test fold (0..4) of every
    train + test row in row order (default: stratified_folds of their labels).  Rows that are NaN at every grid point (vertebra absent) are
    dropped.  One upload, one launch sequence, one readback.  ->
      {'confusion' [G..., 5, K, K] (true x predicted), 'scores' [G..., 5, 4] (SCORES order), 'mean', 'var' [G..., 4] over the folds,
       'pred' [G..., 5, Mv] (grades; -1 at an unusable grid point), 'w' [G..., 5, P, F], 'b', 'gap' [G..., 5, P] (decision = w . x_scaled - b, the pairs
       (0,1), (0,2), ... of `classes`, positive = the lower class), 'iterations', 'status', 'support' [G..., 5, P], 'unusable' [G...] (a feature
       of that grid point is not finite: nothing solved, NaN scores), 'classes' [K], 'folds' [M], 'rows_tt' / 'rows_val' (the rows of `features`
       used), and with decisions=True 'decision' [G..., 5, Mv, P]}
    Nothing raises per grid point: check 'unusable' and 'status' (CONVERGED, HIT_MAX_ITER, PAIR_ABSENT: a class of the pair does not occur
    in that fold's training rows).  ValueError before any launch: F not 3 or 6, more than 4 grades, a class pair with more than 1792 training
    rows in a fold (the solver keeps them in LDS), bad fold ids."""
    feats = np.asarray(features, dtype=np.float64)
    labels, dataset = np.asarray(labels), np.asarray(dataset)
    if feats.ndim < 2 or labels.shape != feats.shape[:1] or dataset.shape != feats.shape[:1]:
        raise ValueError('svm_grade_grid: features [N, G..., F] with one label and one dataset name per row expected')
    grid, F = feats.shape[1:-1], feats.shape[-1]
    if F not in (3, 6):
        raise ValueError('svm_grade_grid: 3 or 6 feature columns expected, got %d' % F)
    if not np.all(np.isin(dataset, ('train', 'test', 'val'))):
        raise ValueError("svm_grade_grid: dataset entries must be 'train', 'test' or 'val'")
    if not np.all(labels == np.floor(labels)) or np.any(labels < 0):
        raise ValueError('svm_grade_grid: labels must be non-negative integers')
    if not (tol > 0) or int(max_iter) < 1:
        raise ValueError('svm_grade_grid: tol > 0 and max_iter >= 1 expected')
    flat = feats.reshape(feats.shape[0], -1, F)
    G = flat.shape[1]
    if G == 0 or G > MAX_GRID:
        raise ValueError('svm_grade_grid: between 1 and %d grid points expected' % MAX_GRID)
    keep = ~np.isnan(flat).any(axis=2).all(axis=1)
    rows_tt, rows_val = np.flatnonzero(keep & (dataset != 'val')), np.flatnonzero(keep & (dataset == 'val'))
    M, Mv = len(rows_tt), len(rows_val)
    if M == 0 or Mv == 0:
        raise ValueError('svm_grade_grid: train / test rows and val rows expected')
    y_tt, y_val = labels[rows_tt].astype(np.int32), labels[rows_val].astype(np.int32)
    classes = np.unique(np.concatenate([y_tt, y_val])).astype(np.int32)
    K = len(classes)
    if K < 2 or K > MAX_CLASSES:
        raise ValueError('svm_grade_grid: between 2 and %d different grades expected, got %d' % (MAX_CLASSES, K))
    folds = stratified_folds(y_tt) if folds is None else np.ascontiguousarray(folds, dtype=np.int32)
    if folds.shape != (M,):
        raise ValueError('svm_grade_grid: one fold id per train / test row expected')
    L = _lib.get()
    y_tt, y_val, folds = np.ascontiguousarray(y_tt), np.ascontiguousarray(y_val), np.ascontiguousarray(folds, dtype=np.int32)
    plan = np.zeros(L.size('hv_svm_grade_plan_bytes', M, Mv), dtype=np.uint8)
    max_rows = ctypes.c_int(0)
    rc = L.cdll.hv_svm_grade_plan(y_tt.ctypes.data, folds.ctypes.data, M, y_val.ctypes.data, Mv, classes.ctypes.data, K, plan.ctypes.data,
                                  ctypes.c_size_t(plan.nbytes), ctypes.byref(max_rows))
    if rc != 0:
        raise ValueError('svm_grade_grid: %s' % ('a class pair has %d training rows in one fold, more than the %d the solver keeps in LDS'
                                                 % (max_rows.value, MAX_PAIR_ROWS) if max_rows.value > MAX_PAIR_ROWS else
                                                 'fold ids must be 0..%d (hv_svm_grade_plan: %s)' % (N_SPLITS - 1, _lib.ERRORS.get(rc, rc))))
    dev = torch.device('cuda', torch.cuda.current_device())
    x_tt, x_val = np.ascontiguousarray(flat[rows_tt].transpose(1, 0, 2)), np.ascontiguousarray(flat[rows_val].transpose(1, 0, 2))
    blob = torch.from_numpy(np.concatenate([x_tt.reshape(-1).view(np.uint8), x_val.reshape(-1).view(np.uint8), plan])).to(dev)
    _lib.require_gpu(blob)
    P = K * (K - 1) // 2
    # one output buffer, the float64 arrays first: name -> (dtype, shape)
    outs = [('w', np.float64, (G, N_SPLITS, P, F)), ('b', np.float64, (G, N_SPLITS, P)), ('gap', np.float64, (G, N_SPLITS, P)),
            ('scores', np.float64, (G, N_SPLITS, 4)), ('mean', np.float64, (G, 4)), ('var', np.float64, (G, 4))]
    if decisions:
        outs.append(('decision', np.float64, (G, N_SPLITS, Mv, P)))
    outs += [('info', np.int32, (G, N_SPLITS, P, 4)), ('pred', np.int32, (G, N_SPLITS, Mv)), ('confusion', np.int32, (G, N_SPLITS, K, K)),
             ('unusable', np.int32, (G,))]
    offs, total = {}, 0
    for name, dt, shape in outs:
        offs[name] = total
        total += int(np.prod(shape)) * np.dtype(dt).itemsize
    buf = torch.zeros(total + 8, dtype=torch.uint8, device=dev)
    at = lambda name: ctypes.c_void_p(buf.data_ptr() + offs[name]) if name in offs else None
    base = blob.data_ptr()
    L.call('hv_svm_grade_grid', ctypes.c_void_p(base), ctypes.c_void_p(base + x_tt.nbytes), ctypes.c_void_p(base + x_tt.nbytes + x_val.nbytes), G, M,
           Mv, F, K, max_rows.value, ctypes.c_double(tol), int(max_iter), at('w'), at('b'), at('gap'), at('info'), at('pred'), at('confusion'),
           at('scores'), at('mean'), at('var'), at('unusable'), at('decision'), _lib.stream())
    host = buf.cpu().numpy()
    res = {name: host[offs[name]:offs[name] + int(np.prod(shape)) * np.dtype(dt).itemsize].view(dt).reshape(grid + shape[1:]).copy()
           for name, dt, shape in outs}
    info = res.pop('info')
    res['iterations'], res['status'], res['support'] = info[..., 0].copy(), info[..., 1].copy(), info[..., 2].copy()
    res['unusable'] = res['unusable'] != 0
    res['pred'] = np.where(res['pred'] >= 0, classes[np.clip(res['pred'], 0, K - 1)], -1)
    res.update(classes=classes, folds=folds, rows_tt=rows_tt, rows_val=rows_val)
    return res


def best_setting(sweep, grades, score='f1'):
    """The (length_divisor, height_threshold) of rhlv_sweep's grid whose grading (svm_grade_grid of svm_feature_grid(sweep)) has the highest mean
    `score` over the folds, among the usable grid points whose every problem converged; ties go to the first in grid order."""
    k = SCORES.index(score)
    mean, status = np.asarray(grades['mean'])[..., k], np.asarray(grades['status'])
    divs, thrs = np.asarray(sweep['length_divisors']), np.asarray(sweep['height_thresholds'])
    if mean.shape != (len(divs), len(thrs)):
        raise ValueError('best_setting: grades of the sweep\'s [D, T] grid expected')
    ok = ~np.asarray(grades['unusable'], dtype=bool) & np.all((status == CONVERGED) | (status == PAIR_ABSENT), axis=(-2, -1)) & ~np.isnan(mean)
    if not ok.any():
        raise ValueError('best_setting: no usable grid point whose problems all converged')
    d, t = np.unravel_index(int(np.argmax(np.where(ok, mean, -np.inf))), mean.shape)
    return int(divs[d]), float(thrs[t])


# ---------------------------------------------------------------- fit at a chosen setting, keep the model, grade new vertebrae
MODEL_KEYS = ('mean', 'scale', 'w', 'b', 'gap', 'iterations', 'status', 'support', 'pair_rows', 'unusable', 'classes', 'present')


def _layout(outs):
    """[(name, dtype, shape)] -> (name -> byte offset, total bytes): one buffer, the 8-byte types first."""
    offs, total = {}, 0
    for name, dt, shape in outs:
        offs[name] = total
        total += int(np.prod(shape)) * np.dtype(dt).itemsize
    return offs, total


def _unpack(host, outs, offs, lead=None):
    return {name: host[offs[name]:offs[name] + int(np.prod(shape)) * np.dtype(dt).itemsize].view(dt).reshape(shape if lead is None else lead + shape[1:]).copy()
            for name, dt, shape in outs}


def svm_fit(features, labels, train=None, tol=1e-3, max_iter=100000):
    """Fit the grader svm_grade_grid scores -- StandardScaler over ALL the rows given, SVC(kernel='linear', class_weight='balanced') on the rows
    with train != 0 (default: every row) -- at every grid point, and keep the models (hv_svm_fit: the grading kernels' own scaler and solver, so
    train = (folds != f) gives bit for bit svm_grade_grid's model of fold f).
    features [N, G..., F], labels [N] small non-negative integer grades (at most 4 different ones), train [N] flags.  Rows that are NaN at every
    grid point (vertebra absent) are dropped.  One upload, one launch, one readback.  ->
      {'mean', 'scale' [G..., F], 'w' [G..., P, F], 'b', 'gap' [G..., P] (decision = w . x_scaled - b, the pairs (0,1), (0,2), ... of `classes`,
       positive = the lower class), 'iterations', 'status', 'support', 'pair_rows' [G..., P], 'unusable' [G...] (a feature of that grid point is
       not finite: NaN model), 'classes' [K], 'present' [K] (the class has train rows), 'rows' (the rows of `features` used)}
    ValueError before any launch: F not 3 or 6, fewer than 2 or more than 4 grades, a class pair with more than 1792 train rows, bad tol /
    max_iter, no rows."""
    feats = np.asarray(features, dtype=np.float64)
    labels = np.asarray(labels)
    if feats.ndim < 2 or labels.shape != feats.shape[:1]:
        raise ValueError('svm_fit: features [N, G..., F] with one label per row expected')
    grid, F = feats.shape[1:-1], feats.shape[-1]
    if F not in (3, 6):
        raise ValueError('svm_fit: 3 or 6 feature columns expected, got %d' % F)
    if not np.all(labels == np.floor(labels)) or np.any(labels < 0):
        raise ValueError('svm_fit: labels must be non-negative integers')
    if not (tol > 0) or int(max_iter) < 1:
        raise ValueError('svm_fit: tol > 0 and max_iter >= 1 expected')
    flat = feats.reshape(feats.shape[0], -1, F)
    G = flat.shape[1]
    if G == 0 or G > MAX_GRID:
        raise ValueError('svm_fit: between 1 and %d grid points expected' % MAX_GRID)
    if train is not None:
        train = np.asarray(train)
        if train.shape != labels.shape:
            raise ValueError('svm_fit: one train flag per row expected')
    rows = np.flatnonzero(~np.isnan(flat).any(axis=2).all(axis=1))
    M = len(rows)
    if M == 0:
        raise ValueError('svm_fit: no usable rows')
    y = np.ascontiguousarray(labels[rows].astype(np.int32))
    flags = None if train is None else np.ascontiguousarray(train[rows] != 0, dtype=np.int32)
    classes = np.unique(y).astype(np.int32)
    K = len(classes)
    if K < 2 or K > MAX_CLASSES:
        raise ValueError('svm_fit: between 2 and %d different grades expected, got %d' % (MAX_CLASSES, K))
    L = _lib.get()
    plan = np.zeros(L.size('hv_svm_fit_plan_bytes', M), dtype=np.uint8)
    max_rows = ctypes.c_int(0)
    rc = L.cdll.hv_svm_fit_plan(y.ctypes.data, None if flags is None else flags.ctypes.data, M, classes.ctypes.data, K, plan.ctypes.data,
                                ctypes.c_size_t(plan.nbytes), ctypes.byref(max_rows))
    if rc != 0:
        raise ValueError('svm_fit: %s' % ('a class pair has %d train rows, more than the %d the solver keeps in LDS' % (max_rows.value, MAX_PAIR_ROWS)
                                          if max_rows.value > MAX_PAIR_ROWS else 'hv_svm_fit_plan: %s' % _lib.ERRORS.get(rc, rc)))
    present = plan[8 * MAX_CLASSES + 32:8 * MAX_CLASSES + 32 + 4 * K].view(np.int32) != 0
    dev = torch.device('cuda', torch.cuda.current_device())
    x = np.ascontiguousarray(flat[rows].transpose(1, 0, 2))
    blob = torch.from_numpy(np.concatenate([x.reshape(-1).view(np.uint8), plan])).to(dev)
    _lib.require_gpu(blob)
    P = K * (K - 1) // 2
    outs = [('mean', np.float64, (G, F)), ('scale', np.float64, (G, F)), ('w', np.float64, (G, P, F)), ('b', np.float64, (G, P)),
            ('gap', np.float64, (G, P)), ('info', np.int32, (G, P, 4))]
    offs, total = _layout(outs)
    buf = torch.zeros(total + 8, dtype=torch.uint8, device=dev)
    at = lambda name: ctypes.c_void_p(buf.data_ptr() + offs[name])
    base = blob.data_ptr()
    L.call('hv_svm_fit', ctypes.c_void_p(base), ctypes.c_void_p(base + x.nbytes), G, M, F, K, max_rows.value, ctypes.c_double(tol), int(max_iter),
           at('mean'), at('scale'), at('w'), at('b'), at('gap'), at('info'), _lib.stream())
    res = _unpack(buf.cpu().numpy(), outs, offs, grid)
    info = res.pop('info')
    res['iterations'], res['status'], res['support'], res['pair_rows'] = (info[..., k].copy() for k in range(4))
    res['unusable'] = np.any(res['status'] == UNUSABLE, axis=-1)
    res.update(classes=classes, present=present.copy(), rows=rows)
    return res


def _model_arrays(model):
    """-> (grid shape, F, K, P, the float64 arrays mean, scale, w, b and info [G, P, 4], present [K] as int32, classes), checked."""
    try:
        classes = np.asarray(model['classes'], dtype=np.int32)
        present = np.ascontiguousarray(np.asarray(model['present']) != 0, dtype=np.int32)
        mean, scale, w, b = (np.ascontiguousarray(model[k], dtype=np.float64) for k in ('mean', 'scale', 'w', 'b'))
        cols = [np.asarray(model[k], dtype=np.int32) for k in ('iterations', 'status', 'support', 'pair_rows')]
    except (KeyError, TypeError) as e:
        raise ValueError('svm_predict: a model of svm_fit expected (%s)' % e)
    K = len(classes)
    P = K * (K - 1) // 2
    if K < 2 or K > MAX_CLASSES or present.shape != (K,) or mean.ndim < 1 or mean.shape[-1] not in (3, 6):
        raise ValueError('svm_predict: a model of 2 to %d classes and 3 or 6 feature columns expected' % MAX_CLASSES)
    grid, F = mean.shape[:-1], mean.shape[-1]
    if scale.shape != grid + (F,) or w.shape != grid + (P, F) or b.shape != grid + (P,) or any(c.shape != grid + (P,) for c in cols):
        raise ValueError('svm_predict: the model arrays do not belong together')
    G = int(np.prod(grid, dtype=np.int64))
    if G == 0 or G > MAX_GRID:
        raise ValueError('svm_predict: between 1 and %d grid points expected' % MAX_GRID)
    info = np.ascontiguousarray(np.stack(cols, axis=-1).reshape(G, P, 4))
    return grid, F, K, P, (mean, scale, w, b), info, present, classes


def _model_blob(arrays, info, present, extra=()):
    """The model (and `extra` float64 arrays in front) as one upload -> (byte array, offsets in upload order)."""
    parts = [np.ascontiguousarray(a).reshape(-1).view(np.uint8) for a in tuple(extra) + tuple(arrays) + (info, present)]
    offs = np.concatenate([[0], np.cumsum([p.nbytes for p in parts])]).astype(np.int64)
    return np.concatenate(parts), [int(o) for o in offs[:-1]]


def svm_predict(model, features, decisions=False, contributions=False):
    """Grade rows with a model of svm_fit (hv_svm_predict: svm_grade_grid's own scaling, decisions and libsvm vote, one lane per row).
    features [N', G..., F] with the model's grid and F.  -> grade [G..., N'] (the grades themselves; -1 where the row has a non-finite feature, the
    grid point's model is unusable or no class has train rows), or with decisions / contributions a dict {'grade', 'decision' [G..., N', P],
    'votes' [G..., N', K] (decisions=True), 'contrib' [G..., N', P, F] = w[p][c] * x_scaled[c] (contributions=True): contrib summed in column order
    minus b is the decision, bit for bit}.  One upload, one launch, one readback."""
    grid, F, K, P, arrays, info, present, classes = _model_arrays(model)
    feats = np.asarray(features, dtype=np.float64)
    if feats.ndim < 2 or feats.shape[1:] != grid + (F,) or feats.shape[0] == 0:
        raise ValueError('svm_predict: features [N, G..., F] of the model\'s grid %s and %d columns expected' % (grid, F))
    N, G = feats.shape[0], info.shape[0]
    L = _lib.get()
    dev = torch.device('cuda', torch.cuda.current_device())
    x = np.ascontiguousarray(feats.reshape(N, G, F).transpose(1, 0, 2))
    host, o = _model_blob(arrays, info, present, extra=(x,))
    blob = torch.from_numpy(host).to(dev)
    _lib.require_gpu(blob)
    outs = ([('decision', np.float64, (G, N, P))] if decisions else []) + ([('contrib', np.float64, (G, N, P, F))] if contributions else [])
    outs += [('pred', np.int32, (G, N))] + ([('votes', np.int32, (G, N, K))] if decisions else [])
    offs, total = _layout(outs)
    buf = torch.zeros(total + 8, dtype=torch.uint8, device=dev)
    at = lambda name: ctypes.c_void_p(buf.data_ptr() + offs[name]) if name in offs else None
    src = lambda k: ctypes.c_void_p(blob.data_ptr() + o[k])
    L.call('hv_svm_predict', src(0), G, N, F, K, src(6), src(1), src(2), src(3), src(4), src(5), at('pred'), at('decision'), at('votes'), at('contrib'),
           _lib.stream())
    res = _unpack(buf.cpu().numpy(), outs, offs, grid)
    pred = res.pop('pred')
    grade = np.where(pred >= 0, classes[np.clip(pred, 0, K - 1)], -1)
    if not (decisions or contributions):
        return grade
    res['grade'] = grade
    return res


class Grader:
    """The fracture grader at one setting: (length_divisor, height_threshold), the classes and the model svm_fit kept.  fit_grader builds one,
    state_dict() / from_state_dict() carry it as plain numpy arrays and python scalars (np.savez-able; reloading gives the same bytes)."""

    def __init__(self, setting, model, file1='sagittal'):
        if file1 not in VIEWS:
            raise ValueError("Grader: file1 must be 'sagittal' or 'coronal'")
        self.setting = (int(setting[0]), float(setting[1]))
        self.file1 = file1
        self.model = {k: np.array(model[k], copy=True) for k in MODEL_KEYS}
        grid = _model_arrays(self.model)[0]
        if grid != ():
            raise ValueError('Grader: the model of one setting expected, got a grid %s' % (grid,))
        self.classes = self.model['classes']

    def state_dict(self):
        d = {k: np.array(v, copy=True) for k, v in self.model.items()}
        d.update(length_divisor=self.setting[0], height_threshold=self.setting[1], file1=self.file1)
        return d

    @classmethod
    def from_state_dict(cls, state):
        """state_dict()'s result, or what np.load gives of its np.savez."""
        try:
            setting = (int(state['length_divisor']), float(state['height_threshold']))
            return cls(setting, {k: np.asarray(state[k]) for k in MODEL_KEYS}, str(state['file1']))
        except KeyError as e:
            raise ValueError('Grader.from_state_dict: %s is missing' % e)

    def predict(self, features, decisions=False, contributions=False):
        """svm_predict of the kept model: features [N, F] in svm_features' column order for this grader's file1."""
        return svm_predict(self.model, features, decisions, contributions)

    def grade_dataset(self, fakes, labels, label_indices, chunk=256, contributions=False):
        """Resident volume pairs -> grades with ONE readback: hv_rhlv_views_batch at the grader's setting exactly as rhlv_dataset launches it, then
        hv_svm_features and hv_svm_predict on the device.  fakes / labels / label_indices as for rhlv_dataset.  ->
          {'grade' [N] (-1: ungradable), 'present' bool [N] (False: the original lacks the vertebra), 'raised' bool [N] (the coronal script would
           have raised), 'records' [N, 2, 16] (rhlv_dataset's), 'features' [N, F], 'decision' [N, P], 'votes' [N, K], and with contributions=True
           'contrib' [N, P, F]}
        Nothing raises per vertebra: an absent vertebra or a raised coronal slice comes back as grade -1 with its flag."""
        L = _lib.get()
        grid, F, K, P, arrays, info, present, classes = _model_arrays(self.model)
        n = len(fakes)
        if n == 0 or len(labels) != n or len(label_indices) != n:
            raise ValueError('grade_dataset: equally many (at least one) generated volumes, original volumes and label indices expected')
        dev = fakes[0].device
        geo = (fakes[0].shape, fakes[0].stride(), fakes[0].dtype)
        for t in list(fakes) + list(labels):
            _lib.require_gpu(t)
            if t.dim() != 3 or (t.shape, t.stride(), t.dtype) != geo or t.dtype not in (torch.float32, torch.uint8) or t.device != dev:
                raise ValueError('grade_dataset: [H, W, Z] float32 or uint8 device volumes of one shape, dtype and stride pattern expected')
        H, W, Z = geo[0]
        views = SAGITTAL | CORONAL
        table = torch.tensor([p for f, l in zip(fakes, labels) for p in (f.data_ptr(), l.data_ptr())], dtype=torch.int64).to(dev)
        ids = torch.tensor([float(i) for i in label_indices], dtype=torch.float32).to(dev)
        host, o = _model_blob(arrays, info, present)
        blob = torch.from_numpy(host).to(dev)
        outs = [('records', np.float64, (n, 2, 16)), ('features', np.float64, (n, F)), ('decision', np.float64, (n, P))]
        outs += ([('contrib', np.float64, (n, P, F))] if contributions else []) + [('pred', np.int32, (n,)), ('votes', np.int32, (n, K))]
        offs, total = _layout(outs)
        buf = torch.zeros(total + 8, dtype=torch.uint8, device=dev)
        at = lambda name, skip=0: ctypes.c_void_p(buf.data_ptr() + offs[name] + skip) if name in offs else None
        src = lambda k: ctypes.c_void_p(blob.data_ptr() + o[k])
        chunk = max(1, min(int(chunk), n))
        ws, _ = ops._ws(L.size('hv_rhlv_views_workspace_bytes', W, Z, views, chunk), dev, slot=3)
        sag, cor = _view_args(L, views, self.setting[0], INT_MIN, 0, self.setting[1])
        for i in range(0, n, chunk):
            m = min(chunk, n - i)
            L.call('hv_rhlv_views_batch', _lib.ptr(table[2 * i:]), _lib.ptr(ids[i:]), m, *_geometry(fakes[0]), views, sag, cor,
                   at('records', i * 2 * 16 * 8), _lib.ptr(ws), ctypes.c_size_t(ws.numel()), _lib.stream())
        L.call('hv_svm_features', at('records'), n, 0 if VIEWS[self.file1] == SAGITTAL else 1, F, at('features'), _lib.stream())
        L.call('hv_svm_predict', at('features'), 1, n, F, K, src(5), src(0), src(1), src(2), src(3), src(4), at('pred'), at('decision'), at('votes'),
               at('contrib'), _lib.stream())
        res = _unpack(buf.cpu().numpy(), outs, offs)
        pred = res.pop('pred')
        res['grade'] = np.where(pred >= 0, classes[np.clip(pred, 0, K - 1)], -1)
        res['present'] = res['records'][:, 0, 13] != 0
        res['raised'] = res['records'][:, 1, 14] != 0
        return res


def fit_grader(sweep, labels, dataset, grades=None, score='f1', setting=None, file1='sagittal', tol=1e-3, max_iter=100000):
    """The grader of a sweep: fitted at `setting` = (length_divisor, height_threshold) of the sweep's grid, by default best_setting(sweep, grades,
    score) with grades = svm_grade_grid(svm_feature_grid(sweep), labels, dataset) where none are given, on the train + test rows -- scaler and SVC as
    the reference's grading fits them, the val rows stay untouched.  file1: the view whose three columns come first (svm_features' order).
    -> Grader"""
    feats = svm_feature_grid(sweep)
    labels, dataset = np.asarray(labels), np.asarray(dataset)
    if labels.shape != feats.shape[:1] or dataset.shape != feats.shape[:1]:
        raise ValueError('fit_grader: one label and one dataset name per row of the sweep expected')
    if not np.all(np.isin(dataset, ('train', 'test', 'val'))):
        raise ValueError("fit_grader: dataset entries must be 'train', 'test' or 'val'")
    if file1 not in VIEWS:
        raise ValueError("fit_grader: file1 must be 'sagittal' or 'coronal'")
    if setting is None:
        if grades is None:
            grades = svm_grade_grid(feats, labels, dataset, tol=tol, max_iter=max_iter)
        setting = best_setting(sweep, grades, score)
    divs, thrs = [int(d) for d in sweep['length_divisors']], [float(t) for t in sweep['height_thresholds']]
    setting = (int(setting[0]), float(setting[1]))
    if setting[0] not in divs or setting[1] not in thrs:
        raise ValueError('fit_grader: setting %s is not a point of the sweep\'s grid' % (setting,))
    at = feats[:, divs.index(setting[0]), thrs.index(setting[1])]
    if VIEWS[file1] == CORONAL:
        at = np.concatenate([at[:, 3:], at[:, :3]], axis=1)
    # as svm_grade_grid: a row that is NaN at every grid point (vertebra absent) is dropped, a row that is NaN at this one makes the model unusable
    keep = (dataset != 'val') & ~np.isnan(feats.reshape(len(feats), -1, 6)).any(axis=2).all(axis=1)
    model = svm_fit(at[keep], labels[keep], tol=tol, max_iter=max_iter)
    return Grader(setting, model, file1)


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
