"""Device-side generation-quality evaluation (reference evaluation/generation_eval_sagittal.py and generation_eval_coronal.py),
DESIGN.md section 8 row f6.

Same entry points as the reference modules, on device tensors (csrc/gen_eval.hip through hv_gen_eval):
  calculate_iou / calculate_dice / relative_volume_difference(ori_seg, fake_seg)         binary (0 / 1) volumes (:11-37)
  process_images(ori_ct, fake_ct, ori_seg, fake_seg, label, view)                        (:39-103) -> the seven values
  evaluate_generation(items, view)                                                       the skip and average rule of main() (:140-158)
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
    lists = {k: [] for k in KEYS}
    for i, o in enumerate(all_o):
        _check(o, 'evaluate_generation (volume %d)' % i)
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
