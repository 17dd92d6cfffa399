"""Device-side generation-quality evaluation (reference evaluation/generation_eval_sagittal.py and generation_eval_coronal.py),
DESIGN.md section 8 row f6.

Same entry points as the reference modules, on device tensors (csrc/gen_eval.hip through hv_gen_eval):
  calculate_iou / calculate_dice / relative_volume_difference(ori_seg, fake_seg)         binary (0 / 1) volumes (:11-37)
  process_images(ori_ct, fake_ct, ori_seg, fake_seg, label, view)                        (:39-103) -> the seven values
  evaluate_generation(items, view)                                                       the skip and average rule of main() (:140-158)
  process_images_batch(originals, fakes, view) / evaluate_experiments(originals, experiments, view)    main()'s two loops (:124-162), every
      validation vertebra x every experiment against the same original, through hv_gen_eval_batch: one launch sequence and one readback,
      what depends on the original alone computed once per item, every pair's values the bits process_images gives for it
Beyond the reference (section 8 row f9, csrc/edt.hip): distance_transform(volume, value, spacing) -- the exact Euclidean distance transform --
and surface_distances / surface_distances_batch(ori_seg, fake_seg, label, spacing): Hausdorff distance, HD95 and average symmetric surface
distance of the vertebra's two outlines, in the units of `spacing`; largest_component=True first reduces both sets to their largest 3-D
component (components.py, csrc/ccl3d.hip; row f10), so that a stray island of a slice-wise synthesized label does not set the distances
Volumes are [H, W, Z] with any strides: CT float32 / float64, labels uint8 / float32 / float64 (other dtypes are converted), device tensors
or numpy arrays (uploaded), e.g. the float64 arrays infer.process_volume returns.  `label` is the vertebra id the reference parses from the
file name.  File I/O, the vertebra_data.json selection and the .txt report stay on the host.
"""
import ctypes
import math
import warnings

import numpy as np
import torch

from . import lib as _lib
from . import ops

VIEWS = {'sagittal': 2, 'coronal': 1}
KEYS = ('global_psnr', 'global_ssim', 'patch_psnr', 'patch_ssim', 'iou', 'rv_diff', 'dice')
SLICE_FIELDS = ('z', 'x1', 'x2', 'R_patch', 'R_global', 'psnr_patch', 'ssim_patch', 'psnr_global', 'ssim_global')
_DT = {torch.uint8: 0, torch.float32: 4, torch.float64: 5}   # HV_DT_* of include/hvgan.h


def _device(*vols):
    for v in vols:
        if isinstance(v, torch.Tensor) and v.is_cuda:
            return v.device
    return torch.device('cuda', torch.cuda.current_device())


def _prep(v, device, allowed, fallback):
    t = torch.as_tensor(v)
    if t.dtype not in allowed:
        t = t.to(fallback)
    return t.to(device)


def _pair(a, b, device, allowed, fallback):
    """Both volumes on `device` with one dtype and one set of strides (the kernel takes one stride triple per pair)."""
    a, b = _prep(a, device, allowed, fallback), _prep(b, device, allowed, fallback)
    if a.dtype != b.dtype:
        a, b = a.to(torch.float64), b.to(torch.float64)
    if a.dim() != 3 or a.shape != b.shape:
        raise ValueError('generation_eval: [H, W, Z] volumes of equal shape expected, got %s and %s' % (tuple(a.shape), tuple(b.shape)))
    if a.stride() != b.stride():
        a, b = a.contiguous(), b.contiguous()
    _lib.require_gpu(a, b)
    return a, b


def _launch(ori_ct, fake_ct, ori_seg, fake_seg, label, view, out, slices=None):
    """Queue one hv_gen_eval on the current stream; `out` (16 doubles) and `slices` are device views written by it."""
    if view not in VIEWS:
        raise ValueError("view must be 'sagittal' or 'coronal', got %r" % (view,))
    L = _lib.get()
    dev = out.device
    ls, lf = _pair(ori_seg, fake_seg, dev, (torch.uint8, torch.float32, torch.float64), torch.float64)
    if ori_ct is None:
        cs = cf = None
    else:
        cs, cf = _pair(ori_ct, fake_ct, dev, (torch.float32, torch.float64), torch.float64)
        if cs.shape != ls.shape:
            raise ValueError('generation_eval: CT %s and label %s volumes differ in shape' % (tuple(cs.shape), tuple(ls.shape)))
    H, W, Z = ls.shape
    need = L.size('hv_gen_eval_workspace_bytes', H, W, Z, VIEWS[view])
    ws, wsz = ops._ws(need, dev, slot=3)
    cst = cs.stride() if cs is not None else (0, 0, 0)
    L.call('hv_gen_eval', _lib.ptr(cs), _lib.ptr(cf), _DT[cs.dtype] if cs is not None else 5,
           *[ctypes.c_longlong(v) for v in cst], _lib.ptr(ls), _lib.ptr(lf), _DT[ls.dtype], *[ctypes.c_longlong(v) for v in ls.stride()],
           H, W, Z, VIEWS[view], ctypes.c_double(float(label)), _lib.ptr(out), _lib.ptr(slices), _lib.ptr(ws), wsz, _lib.stream())
    return (H, W, Z)


def _check(o, what='process_images'):
    if o[7] != 0:
        raise ValueError('%s: the original volume does not contain the vertebra (the reference: min() arg is an empty sequence)' % what)
    if o[8] != 0:
        raise ValueError('%s: an evaluated slice has a patch or side shorter than 7 pixels (structural_similarity: win_size exceeds '
                         'image extent)' % what)


def _counts(ori_seg, fake_seg):
    dev = _device(ori_seg, fake_seg)
    out = torch.zeros(16, dtype=torch.float64, device=dev)
    _launch(None, None, ori_seg, fake_seg, 1.0, 'sagittal', out)
    return out.cpu().numpy()


def calculate_iou(ori_seg, fake_seg):
    """|ori & fake| / |ori | fake| of two binary (0 / 1) volumes, 0 if the union is empty."""
    return float(_counts(ori_seg, fake_seg)[4])


def calculate_dice(ori_seg, fake_seg):
    """2 |ori & fake| / (|ori| + |fake|) of two binary (0 / 1) volumes, 0 if both are empty."""
    return float(_counts(ori_seg, fake_seg)[6])


def relative_volume_difference(ori_seg, fake_seg):
    """| |ori| - |fake| | / |ori| of two binary (0 / 1) volumes, 0 if the original is empty."""
    return float(_counts(ori_seg, fake_seg)[5])


def process_images(ori_ct, fake_ct, ori_seg, fake_seg, label, view='sagittal', return_slices=False):
    """-> (global_psnr, global_ssim, patch_psnr, patch_ssim, iou, rv_diff, dice) of vertebra `label`; with return_slices also a dict of
    per-evaluated-slice numpy arrays (SLICE_FIELDS).  Raises ValueError where the reference raises (absent vertebra, patch < 7 rows)."""
    dev = _device(ori_ct, fake_ct, ori_seg, fake_seg)
    S = torch.as_tensor(ori_seg).shape[VIEWS.get(view, 2)] if return_slices else 0
    buf = torch.zeros(16 + len(SLICE_FIELDS) * S, dtype=torch.float64, device=dev)
    _launch(ori_ct, fake_ct, ori_seg, fake_seg, label, view, buf[:16], buf[16:] if return_slices else None)
    o = buf.cpu().numpy()
    _check(o)
    res = tuple(float(v) for v in o[:7])
    if not return_slices:
        return res
    n = int(o[15])
    rec = o[16:16 + len(SLICE_FIELDS) * n].reshape(n, len(SLICE_FIELDS))
    rec = rec[rec[:, 0] >= 0]                      # the slices of the 4/5 range that were evaluated
    sl = {k: rec[:, i].astype(np.int64) if k in ('z', 'x1', 'x2') else rec[:, i].copy() for i, k in enumerate(SLICE_FIELDS)}
    return res, sl


def average_outputs(all_o, what='evaluate_generation (volume %d)'):
    """main()'s skip and average rule (:140-158) on an [n][16] array of hv_gen_eval outputs, host arithmetic only: a volume whose patch PSNR
    or SSIM is NaN or 0 is skipped; each key is np.mean over the kept volumes (NaN if none).  Raises ValueError for a volume whose error
    flags are set, named by `what % index`.  -> dict of the seven averages plus 'count' and 'per_volume'."""
    lists = {k: [] for k in KEYS}
    for i, o in enumerate(all_o):
        _check(o, what % i)
        pp, ps = float(o[2]), float(o[3])
        if math.isnan(pp) or math.isnan(ps) or pp == 0 or ps == 0:
            continue
        for q, k in enumerate(KEYS):
            lists[k].append(float(o[q]))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)     # np.mean([]) -> nan, as main() gets when every volume was skipped
        res = {k: float(np.mean(v)) for k, v in lists.items()}
    res['count'] = len(lists['iou'])
    res['per_volume'] = [tuple(float(v) for v in o[:7]) for o in all_o]
    return res


def evaluate_generation(items, view='sagittal'):
    """main()'s per-experiment body over an iterable of (ori_ct, fake_ct, ori_seg, fake_seg, label): every volume is queued on the device,
    then one readback.  A volume whose patch PSNR or SSIM is NaN or 0 is skipped; each key is np.mean over the kept volumes (NaN if none).
    -> dict of the seven averages plus 'count' (kept volumes) and 'per_volume' (the seven values of every volume, skipped ones included)."""
    outs = []
    for it in items:
        ori_ct, fake_ct, ori_seg, fake_seg, label = it
        dev = _device(ori_ct, fake_ct, ori_seg, fake_seg)
        out = torch.empty(16, dtype=torch.float64, device=dev)
        _launch(ori_ct, fake_ct, ori_seg, fake_seg, label, view, out)
        outs.append(out)
    all_o = torch.stack([o.to(outs[0].device) for o in outs]).cpu().numpy() if outs else np.zeros((0, 16))
    return average_outputs(all_o)


# ------------------------------------------------------------------------------------------------ a whole set, several experiments
WORKSPACE_BOUND = 1 << 30      # process_images_batch: the default `chunk` keeps one call's workspace below this


def _meta(v, allowed, fallback):
    """(shape, dtype, strides) a volume has once _prep has run on it, without touching a device."""
    t = v if isinstance(v, torch.Tensor) else torch.as_tensor(v)
    dt = t.dtype if t.dtype in allowed else fallback
    return tuple(t.shape), dt, tuple(t.stride())


_LABEL_DT = (torch.uint8, torch.float32, torch.float64)
_CT_DT = (torch.float32, torch.float64)


def _item_signature(original, fakes_i, counts_only=False):
    """What one hv_gen_eval_batch call must share among its volumes, for one item: (shape, CT dtype, CT strides, label dtype, label strides).
    A dtype that differs inside the item becomes float64, strides that differ become the contiguous ones: what _pair does to a pair."""
    def common(vols, allowed):
        metas = [_meta(v, allowed, torch.float64) for v in vols]
        shapes = {m[0] for m in metas}
        if len(shapes) != 1 or len(metas[0][0]) != 3:
            raise ValueError('generation_eval: [H, W, Z] volumes of equal shape expected, got %s' % sorted(shapes))
        dts = {m[1] for m in metas}
        dt = metas[0][1] if len(dts) == 1 else torch.float64
        sts = {m[2] for m in metas}
        st = metas[0][2] if len(sts) == 1 and len(dts) == 1 else None       # None: made contiguous
        return metas[0][0], dt, st
    shape, ldt, lst = common([original[1]] + [f[1] for f in fakes_i], _LABEL_DT)
    if counts_only:
        return shape, None, None, ldt, lst
    cshape, cdt, cst = common([original[0]] + [f[0] for f in fakes_i], _CT_DT)
    if cshape != shape:
        raise ValueError('generation_eval: CT %s and label %s volumes differ in shape' % (cshape, shape))
    return shape, cdt, cst, ldt, lst


def group_items(originals, fakes, counts_only=False):
    """Host-side grouping for process_images_batch: -> (E, [(signature, [item indices])]) in order of first appearance.  Raises ValueError
    on a ragged `fakes` (before any device work) and on volumes of unequal shape, naming the item."""
    if len(fakes) != len(originals):
        raise ValueError('process_images_batch: %d originals but %d rows of fakes' % (len(originals), len(fakes)))
    E = len(fakes[0]) if len(fakes) else 0
    for i, row in enumerate(fakes):
        if len(row) != E:
            raise ValueError('process_images_batch: ragged fakes, item %d has %d experiments, item 0 has %d' % (i, len(row), E))
    if len(fakes) and E == 0:
        raise ValueError('process_images_batch: no experiment')
    groups = {}
    for i, (o, row) in enumerate(zip(originals, fakes)):
        try:
            sig = _item_signature(o, row, counts_only)
        except ValueError as e:
            raise ValueError('%s (item %d)' % (e, i)) from None
        groups.setdefault(sig, []).append(i)
    return E, list(groups.items())


def _conform(v, device, dtype, strides, allowed):
    t = _prep(v, device, allowed, torch.float64)
    if t.dtype != dtype:
        t = t.to(dtype)
    if strides is None or tuple(t.stride()) != strides:
        t = t.contiguous()
    _lib.require_gpu(t)
    return t


def _launch_batch(sig, originals, fakes, idx, E, view, out, slices, device):
    """Queue one hv_gen_eval_batch for the items `idx` (all of signature `sig`); `out` [n][E][16] and `slices` are device tensors."""
    L = _lib.get()
    shape, cdt, cst, ldt, lst = sig
    n = len(idx)
    tab = np.zeros(2 * n + 2 * n * E + n, dtype=np.float64)     # pointer tables (as int64) and the labels: one upload
    ptrs = tab.view(np.int64)
    o_ct, f_ct, o_lab, f_lab, lab = 0, n, n + n * E, 2 * n + n * E, 2 * n + 2 * n * E
    labs, cts = [], []                                           # (table slot, tensor)
    for a, i in enumerate(idx):
        oc, ol, label = originals[i]
        tab[lab + a] = float(label)
        labs.append((o_lab + a, _conform(ol, device, ldt, lst, _LABEL_DT)))
        labs += [(f_lab + a * E + e, _conform(fakes[i][e][1], device, ldt, lst, _LABEL_DT)) for e in range(E)]
        if cdt is not None:
            cts.append((o_ct + a, _conform(oc, device, cdt, cst, _CT_DT)))
            cts += [(f_ct + a * E + e, _conform(fakes[i][e][0], device, cdt, cst, _CT_DT)) for e in range(E)]
    for vols in (labs, cts):                                     # one stride triple per kind, whatever the conversions left
        if len({tuple(t.stride()) for _, t in vols}) > 1:
            vols[:] = [(slot, t.contiguous()) for slot, t in vols]
        for slot, t in vols:
            ptrs[slot] = t.data_ptr()
    keep = [t for _, t in labs + cts]
    lstr = labs[0][1].stride()
    cstr = cts[0][1].stride() if cdt is not None else (0, 0, 0)
    dtab = torch.from_numpy(tab).to(device)
    base = dtab.data_ptr()
    at = lambda off: ctypes.c_void_p(base + 8 * off)
    H, W, Z = shape
    need = L.size('hv_gen_eval_batch_workspace_bytes', H, W, Z, VIEWS[view], n, E)
    ws, wsz = ops._ws(need, device, slot=3)
    L.call('hv_gen_eval_batch', at(o_ct) if cdt is not None else None, at(f_ct) if cdt is not None else None, _DT[cdt] if cdt is not None else 5,
           *[ctypes.c_longlong(v) for v in cstr], at(o_lab), at(f_lab), _DT[ldt], *[ctypes.c_longlong(v) for v in lstr],
           H, W, Z, VIEWS[view], at(lab), n, E, _lib.ptr(out), _lib.ptr(slices), _lib.ptr(ws), wsz, _lib.stream())
    return keep + [dtab]       # alive until the caller has synchronised


def _batch_outputs(originals, fakes, view, return_slices, chunk, counts_only=False):
    """-> (out [N][E][16] numpy, records [N][E][S][9] numpy or None): every call queued, then one readback per group of volumes."""
    if view not in VIEWS:
        raise ValueError("view must be 'sagittal' or 'coronal', got %r" % (view,))
    originals, fakes = list(originals), [list(row) for row in fakes]
    E, groups = group_items(originals, fakes, counts_only)
    N = len(originals)
    out = np.zeros((N, E, 16))
    rec = None
    if not N:
        return out, rec
    L = _lib.get()
    dev = _device(*[v for o in originals for v in o[:2]], *[v for row in fakes for f in row for v in f])
    pending, keep = [], []
    for sig, idx in groups:
        H, W, Z = sig[0]
        S = sig[0][VIEWS[view]]
        per_item = L.size('hv_gen_eval_batch_workspace_bytes', H, W, Z, VIEWS[view], 1, E)
        step = int(chunk) if chunk else max(1, min(WORKSPACE_BOUND // max(1, per_item), 65535 // E))
        if step < 1:
            raise ValueError('process_images_batch: chunk must be at least 1, got %r' % (chunk,))
        for a in range(0, len(idx), step):
            part = idx[a:a + step]
            d_out = torch.zeros(len(part), E, 16, dtype=torch.float64, device=dev)
            d_rec = torch.zeros(len(part), E, S, len(SLICE_FIELDS), dtype=torch.float64, device=dev) if return_slices else None
            keep.append(_launch_batch(sig, originals, fakes, part, E, view, d_out, d_rec, dev))
            pending.append((part, d_out, d_rec))
    if return_slices:
        rec = [[None] * E for _ in range(N)]
    for part, d_out, d_rec in pending:
        out[part] = d_out.cpu().numpy()
        if d_rec is not None:
            r = d_rec.cpu().numpy()
            for a, i in enumerate(part):
                for e in range(E):
                    rec[i][e] = r[a, e]
    return out, rec


def _slice_dict(o, rec):
    n = int(o[15])
    rec = rec[:n]
    rec = rec[rec[:, 0] >= 0]                      # the slices of the 4/5 range that were evaluated
    return {k: rec[:, i].astype(np.int64) if k in ('z', 'x1', 'x2') else rec[:, i].copy() for i, k in enumerate(SLICE_FIELDS)}


def process_images_batch(originals, fakes, view='sagittal', return_slices=False, chunk=None):
    """process_images for a whole set and several experiments (main() :124-162) in one launch sequence per group of equal volumes.
    originals: sequence of (ori_ct, ori_seg, label); fakes[i][e] = (fake_ct, fake_seg) of item i in experiment e (every item has the same
    number of experiments).  -> [N][E][7] numpy array, each row the bits process_images gives for that pair; with return_slices also
    [N][E] dicts of per-evaluated-slice arrays (SLICE_FIELDS).  Device tensors or numpy arrays.  Items whose shape, dtypes or strides differ
    go into further calls (within an item, differing dtypes become float64 and differing strides contiguous, as for a pair); `chunk`
    bounds the items per call (default: a workspace of at most WORKSPACE_BOUND bytes).  Raises ValueError where process_images raises,
    naming the item and experiment, and before the first launch on a ragged `fakes`."""
    out, rec = _batch_outputs(originals, fakes, view, return_slices, chunk)
    for i in range(out.shape[0]):
        for e in range(out.shape[1]):
            _check(out[i, e], 'process_images_batch (item %d, experiment %d)' % (i, e))
    res = out[:, :, :7].copy()
    if not return_slices:
        return res
    return res, [[_slice_dict(out[i, e], rec[i][e]) for e in range(out.shape[1])] for i in range(out.shape[0])]


def evaluate_experiments(originals, experiments, view='sagittal'):
    """main() over every experiment folder: originals as for process_images_batch, experiments {name: [(fake_ct, fake_seg) per item]}.
    -> {name: the dict evaluate_generation returns for that experiment}; averaging on the host (np.mean, the reference's own summation)."""
    originals = list(originals)
    names = list(experiments)
    rows = {k: list(experiments[k]) for k in names}
    for k in names:
        if len(rows[k]) != len(originals):
            raise ValueError('evaluate_experiments: experiment %r has %d volumes for %d originals' % (k, len(rows[k]), len(originals)))
    if not names:
        return {}
    fakes = [[rows[k][i] for k in names] for i in range(len(originals))]
    out, _ = _batch_outputs(originals, fakes, view, False, None)
    return {k: average_outputs(out[:, e], 'evaluate_experiments (experiment %r, volume %%d)' % (k,)) for e, k in enumerate(names)}


# ------------------------------------------------------------------------------------------------ distance transform, surface distances
# The shape part of the evaluation beyond overlap (csrc/edt.hip through hv_edt / hv_surface_distance): the exact
# Euclidean distance transform (scipy.ndimage.distance_transform_edt) and MedPy's boundary metrics -- Hausdorff distance, its 95th percentile,
# average symmetric surface distance -- in the units of `spacing` (millimetres per voxel, straighten.check_spacing: a scalar or three floats).
SURFACE_KEYS = ('hd', 'hd95', 'assd', 'asd_ab', 'asd_ba', 'n_a', 'n_b')
_SURFACE_AT = {'n_a': 0, 'n_b': 1, 'max_ab': 2, 'max_ba': 3, 'asd_ab': 4, 'asd_ba': 5, 'hd': 6, 'hd95': 7, 'assd': 8}


def _spacing3(spacing):
    from .straighten import check_spacing
    sp = check_spacing(spacing)
    return sp, (ctypes.c_double * 3)(*sp)


def _label_volume(v, device):
    t = torch.as_tensor(v)
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    t = _prep(t, device, _LABEL_DT, torch.float64)
    if t.dim() != 3:
        raise ValueError('generation_eval: a 3-D volume expected, got shape %s' % (tuple(t.shape),))
    return t


def _check_box(box, shape):
    if box is None:
        return None
    try:
        vals = [int(v) for v in box]
    except (TypeError, ValueError):
        raise ValueError('box: (lo0, lo1, lo2, n0, n1, n2) expected, got %r' % (box,))
    if len(vals) != 6 or any(vals[a] < 0 or vals[3 + a] < 1 or vals[a] + vals[3 + a] > shape[a] for a in range(3)):
        raise ValueError('box: (lo0, lo1, lo2, n0, n1, n2) inside the volume %s expected, got %r' % (tuple(shape), box))
    return (ctypes.c_int * 6)(*vals)


def distance_transform(mask_or_volume, value=0, spacing=1.0, out=None, box=None, return_status=False):
    """The exact Euclidean distance of every voxel to the nearest voxel equal to `value`, scipy.ndimage.distance_transform_edt(v != value,
    sampling=spacing): for a mask and value 0 the distance to the background.  -> device float64 tensor of the volume's shape (`out`, if
    given: contiguous float64 of that shape on the device).  box (lo0, lo1, lo2, n0, n1, n2) limits the voxels written and the voxels
    considered (a fresh output is NaN outside it).  No voxel equal to `value`: every distance is +inf; return_status also returns the device
    int32 word that says so (1), without a synchronisation."""
    sp, csp = _spacing3(spacing)
    if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise ValueError('value: a number expected, got %r' % (value,))
    meta = torch.as_tensor(mask_or_volume)
    if meta.dim() != 3:
        raise ValueError('generation_eval: a 3-D volume expected, got shape %s' % (tuple(meta.shape),))
    cbox = _check_box(box, meta.shape)
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.float64 or tuple(out.shape) != tuple(meta.shape)
                            or not out.is_contiguous()):
        raise ValueError('out: a contiguous float64 tensor of shape %s expected' % (tuple(meta.shape),))
    dev = _device(mask_or_volume, out)
    v = _label_volume(mask_or_volume, dev)
    _lib.require_gpu(v, out)
    L = _lib.get()
    A0, A1, A2 = v.shape
    if out is None:
        out = torch.empty(A0, A1, A2, dtype=torch.float64, device=dev) if box is None else \
            torch.full((A0, A1, A2), float('nan'), dtype=torch.float64, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ws, wsz = ops._ws(L.size('hv_edt_workspace_bytes', A0, A1, A2), dev, slot=3)
    L.call('hv_edt', _lib.ptr(v), _DT[v.dtype], *[ctypes.c_longlong(s) for s in v.stride()], A0, A1, A2, ctypes.c_double(float(value)), csp,
           cbox, _lib.ptr(out), _lib.ptr(status), _lib.ptr(ws), wsz, _lib.stream())
    return (out, status) if return_status else out


def _launch_surface(ori_seg, fake_seg, label, csp, restrict, out):
    """Queue one hv_surface_distance on the current stream; `out` (16 doubles) is a device view written by it."""
    L = _lib.get()
    dev = out.device
    a, b = _pair(ori_seg, fake_seg, dev, _LABEL_DT, torch.float64)
    A0, A1, A2 = a.shape
    ws, wsz = ops._ws(L.size('hv_surface_distance_workspace_bytes', A0, A1, A2), dev, slot=3)
    L.call('hv_surface_distance', _lib.ptr(a), _lib.ptr(b), _DT[a.dtype], *[ctypes.c_longlong(s) for s in a.stride()], A0, A1, A2,
           ctypes.c_double(float(label)), csp, 1 if restrict else 0, _lib.ptr(out), _lib.ptr(ws), wsz, _lib.stream())


def _surface_dict(o, what):
    if o[9] != 0 or o[10] != 0:
        raise ValueError('%s: %s has no voxel of the label, the surface distances are undefined'
                         % (what, ' and '.join(n for n, f in (('the original', o[9]), ('the synthesized volume', o[10])) if f != 0)))
    res = {k: float(o[_SURFACE_AT[k]]) for k in SURFACE_KEYS}
    res['n_a'], res['n_b'] = int(o[0]), int(o[1])
    return res


def _bool_mask(v):
    t = torch.as_tensor(v)
    return t.to(torch.uint8) if t.dtype == torch.bool else v


def _largest_components(ori_seg, fake_seg, label, connectivity, dev):
    """Both volumes with every 3-D component of `label` but the largest one erased (components.clean_label; csrc/ccl3d.hip), queued on the
    current stream: contiguous device volumes of one dtype, nothing read back."""
    from . import components
    a, b = _pair(ori_seg, fake_seg, dev, _LABEL_DT, torch.float64)
    fill = 0 if float(label) != 0.0 else 1
    tables = torch.empty(2, 8, dtype=torch.int32, device=dev)
    return tuple(components._clean(v, label, connectivity, 0, True, False, None, fill, tables[i]) for i, v in enumerate((a, b)))


def _check_largest(largest_component, connectivity):
    if largest_component:
        from . import components
        components._check_connectivity(connectivity)


def surface_distances(ori_seg, fake_seg, label=1, spacing=1.0, restrict=True, return_raw=False, largest_component=False, connectivity=1):
    """Boundary metrics of vertebra `label` between two label volumes (A = ori_seg == label, B = fake_seg == label; surface = the voxels of a
    set with a face neighbour outside it): -> {'hd': Hausdorff distance, 'hd95': 95th percentile of both directed distance lists joined
    (numpy's linear rule), 'assd': average symmetric surface distance, 'asd_ab' / 'asd_ba': the directed means, 'n_a' / 'n_b': the surface
    counts}, distances in the units of `spacing`.  One readback (16 doubles; return_raw returns them too).  restrict=False runs the two
    distance transforms over the whole volume instead of the sets' bounding box: the same bits, more work.  largest_component: both sets are
    first reduced to their largest 3-D component (connectivity 1 / 2 / 3: 6, 18 or 26 neighbours; equal sizes: the first in raster order) on
    the device, so that a stray island of a slice-wise synthesized label does not set the Hausdorff distance; no extra readback.  Raises
    ValueError if either set is empty."""
    _, csp = _spacing3(spacing)
    _check_largest(largest_component, connectivity)
    ori_seg, fake_seg = _bool_mask(ori_seg), _bool_mask(fake_seg)
    dev = _device(ori_seg, fake_seg)
    out = torch.empty(16, dtype=torch.float64, device=dev)
    if largest_component:
        ori_seg, fake_seg = _largest_components(ori_seg, fake_seg, label, connectivity, dev)
    _launch_surface(ori_seg, fake_seg, label, csp, restrict, out)
    o = out.cpu().numpy()
    if return_raw:
        return (_surface_dict(o, 'surface_distances') if o[9] == 0 and o[10] == 0 else None), o
    return _surface_dict(o, 'surface_distances')


def surface_distances_batch(pairs, spacing=1.0, restrict=True, largest_component=False, connectivity=1):
    """surface_distances for an iterable of (ori_seg, fake_seg, label): every pair is queued on the device, then one readback.  `spacing`,
    largest_component and connectivity hold for all pairs.  -> list of the dicts surface_distances returns, each the bits of the single
    call.  Raises ValueError, naming the pair, if a set is empty."""
    pairs = [tuple(p) for p in pairs]
    for i, p in enumerate(pairs):
        if len(p) != 3:
            raise ValueError('surface_distances_batch: (ori_seg, fake_seg, label) expected, pair %d has %d entries' % (i, len(p)))
    _, csp = _spacing3(spacing)
    _check_largest(largest_component, connectivity)
    if not pairs:
        return []
    dev = _device(*[v for p in pairs for v in p[:2]])
    outs = torch.empty(len(pairs), 16, dtype=torch.float64, device=dev)
    for i, (a, b, label) in enumerate(pairs):
        a, b = _bool_mask(a), _bool_mask(b)
        if largest_component:
            a, b = _largest_components(a, b, label, connectivity, dev)
        _launch_surface(a, b, label, csp, restrict, outs[i])
    o = outs.cpu().numpy()
    return [_surface_dict(o[i], 'surface_distances_batch (pair %d)' % i) for i in range(len(pairs))]
