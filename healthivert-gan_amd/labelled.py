"""The input protocol of the per-label analyses (label_statistics, texture, texture_runs, shape): what a volume, a label
volume, a mask and a label list must be, how they reach the C ABI, and the two recurring call shapes -- one vertebra's cancellous core, and the
original / synthesized pair addressed as one [2][...] batch.  Everything here checks or addresses; nothing computes a feature.  The device
side of the same contract is csrc/volume_access.h."""
import ctypes
import math

import numpy as np
import torch

from . import lib as _lib
from . import ops

MAX_LABELS = 64                                                        # HV_LS_MAX_LABELS of include/hvgan.h
VOL_DT = {torch.uint8: 0, torch.int16: 1, torch.float32: 4, torch.float64: 5}
LABEL_DT = {torch.uint8: 0, torch.int16: 1, torch.int32: 2, torch.int64: 3, torch.float32: 4, torch.float64: 5}
LIMIT = 'at most 2^30 voxels per volume and 65535 volumes per call'


# ------------------------------------------------------------------------------------------------ checks
def check_spacing(spacing):
    if isinstance(spacing, (int, float, np.integer, np.floating)) and not isinstance(spacing, bool):
        spacing = (spacing,) * 3
    try:
        sp = tuple(float(s) for s in spacing)
    except (TypeError, ValueError):
        sp = ()
    if len(sp) != 3 or not all(math.isfinite(s) and s > 0.0 for s in sp):
        raise ValueError('spacing: three positive finite numbers expected, got %r' % (spacing,))
    return sp


def check_labels(labels):
    try:
        ls = [int(x) for x in labels]
        same = all(float(x) == int(x) for x in labels)
    except (TypeError, ValueError):
        ls, same = [], False
    if not same or not 1 <= len(ls) <= MAX_LABELS or len(set(ls)) != len(ls) or not all(0 <= x <= 255 for x in ls):
        raise ValueError('labels: 1 to %d distinct integers in [0, 255] expected, got %r' % (MAX_LABELS, labels))
    return ls


def check_erode(erode_mm):
    if isinstance(erode_mm, bool) or not isinstance(erode_mm, (int, float, np.integer, np.floating)) or not (math.isfinite(erode_mm) and erode_mm >= 0):
        raise ValueError('erode_mm: a non-negative finite number expected, got %r' % (erode_mm,))
    return float(erode_mm)


def check_tensor(t, name, table, shape=None):
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


def check_3d(t, name, table, shape=None):
    check_tensor(t, name, table, shape)
    if t.dim() != 3:
        raise ValueError('%s: one [A0][A1][A2] volume expected, got shape %s' % (name, tuple(t.shape)))
    return t


def resident(x):
    """A numpy array uploaded to the current device; anything else as it is (check_tensor refuses what is no device tensor)."""
    if isinstance(x, np.ndarray):
        return torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return x


def as4(t):
    return t if t.dim() == 4 else t.unsqueeze(0)


def squeeze(res, per_call=('labels',)):
    """The [V = 1] axis dropped: what a single volume's caller gets (the entries named in per_call have none)."""
    return {k: (v if k in per_call else v[0]) for k, v in res.items()}


def check_inputs(vol, label, mask, upload=False):
    """vol (None: the analysis reads the label alone), label and mask checked against each other -> (whether the caller gave one 3-D volume,
    vol, label, mask as 4-D tensors, mask as uint8).  upload: numpy arrays are uploaded first."""
    if upload:
        vol, label, mask = resident(vol), resident(label), resident(mask)
    if vol is not None:
        check_tensor(vol, 'vol', VOL_DT)
    check_tensor(label, 'label', LABEL_DT, None if vol is None else vol.shape)
    first = label if vol is None else vol
    if mask is not None:
        check_tensor(mask, 'mask', (torch.uint8, torch.bool), first.shape)
        if mask.dtype == torch.bool:
            mask = mask.view(torch.uint8)
    if label.device != first.device or (mask is not None and mask.device != first.device):
        raise ValueError('%slabel and mask must lie on one device' % ('' if vol is None else 'vol, '))
    return (first.dim() == 3,) + tuple(None if t is None else as4(t) for t in (vol, label, mask))


def resolve_labels(labels, present):
    """The checked label list; labels=None: what present() finds, which must be 1 to 64 values."""
    if labels is not None:
        return check_labels(labels)
    ids = present()
    if not 1 <= len(ids) <= MAX_LABELS:
        raise ValueError('labels=None: 1 to %d non-zero label values expected in the volumes, found %d' % (MAX_LABELS, len(ids)))
    return ids


# ------------------------------------------------------------------------------------------------ the C ABI
def ll(strides):
    return [ctypes.c_longlong(s) for s in strides]


def volume_args(vol, label, mask, labels):
    """The arguments every per-label entry point starts with: (vol, dtype, strides, label, dtype, strides, mask, strides, V, A0, A1, A2, labels,
    S).  vol None: without the first three (hv_shape).  4-D device tensors or Strided pairs; mask may be None."""
    V, A0, A1, A2 = (int(s) for s in label.shape)
    S = len(labels)
    mst = mask.stride() if mask is not None else (0, 0, 0, 0)
    head = [] if vol is None else [_lib.ptr(vol), VOL_DT[vol.dtype], *ll(vol.stride())]
    return head + [_lib.ptr(label), LABEL_DT[label.dtype], *ll(label.stride()), _lib.ptr(mask), *ll(mst), V, A0, A1, A2, (ctypes.c_int * S)(*labels), S]


def workspace(entry, t, *sizes, who=None, limit=LIMIT):
    """(workspace, its bytes) for hv_<entry> on the volumes t [V][A0][A1][A2]; ValueError where the device refuses the shape."""
    need = _lib.get().size('hv_%s_workspace_bytes' % entry, *(int(s) for s in t.shape), *sizes)
    if need == 0:
        raise ValueError('%s: %s, got shape %s' % (who or entry, limit, tuple(t.shape)))
    return ops._ws(need, t.device, slot=3)


# ------------------------------------------------------------------------------------------------ one vertebra, and the pair
def core_mask(label, vert_ids, erode_mm, sp, out):
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


def vertebra_inputs(ct, label, vert_id, erode_mm, spacing, median_size, upload=True):
    """What the single-vertebra functions start with: every check, then (device work) the optional median pre-step of ct and the optional core
    mask.  -> (ct, label, mask [A0][A1][A2] uint8 or None, the label id, the spacing triple)."""
    sp = check_spacing(spacing)
    r = check_erode(erode_mm)
    vid = check_labels([vert_id])[0]
    if upload:
        ct, label = resident(ct), resident(label)
    check_3d(ct, 'ct', VOL_DT)
    check_3d(label, 'label', LABEL_DT, ct.shape)
    if median_size is not None:
        from . import rank_filters
        ct = rank_filters.median_filter(ct, size=median_size)
    mask = None
    if r > 0.0:
        mask = core_mask(label, [vid], r, sp, torch.empty(tuple(label.shape), dtype=torch.uint8, device=label.device))
    return ct, label, mask, vid, sp


class Strided:
    """Two separate 3-D allocations of one dtype and stride triple addressed as a [2][...] batch: the batch stride is their distance."""

    def __init__(self, t, batch_stride):
        self.t, self.bs = t, batch_stride
        self.shape, self.dtype, self.device = (2,) + tuple(t.shape), t.dtype, t.device

    def stride(self):
        return (self.bs,) + tuple(self.t.stride())

    def data_ptr(self):
        return self.t.data_ptr()


def batch_stride(a, b):
    """b's distance from a in elements if the pair can be addressed as a [2][...] batch, else None."""
    d = b.data_ptr() - a.data_ptr()
    ok = a.dtype == b.dtype and a.stride() == b.stride() and d % a.element_size() == 0
    return d // a.element_size() if ok else None


def pair_plan(cts, labels):
    """How the pair (original, synthesized) of cts (None: labels alone) and of labels is addressed -> [(vol4, label4, sel)]: one [2] batch (sel =
    slice(None)) when each synthesized member lies a whole number of elements from its original with the same dtype and strides, else the two
    members on their own with sel = slice(0, 1) and slice(1, 2)."""
    members = [p for p in (cts, labels) if p is not None]
    strides = [batch_stride(a, b) for a, b in members]
    if None not in strides:
        batch = [Strided(p[0], s) for p, s in zip(members, strides)]
        return [(batch[0] if cts else None, batch[-1], slice(None))]
    return [(cts[v][None] if cts else None, labels[v][None], slice(v, v + 1)) for v in (0, 1)]


class Pair:
    """The original and the synthesized (ct, label) -- or the two labels alone -- of a comparison.  The constructor is the checks and then the
    device work they guard: the four volumes against each other, the ids (the vertebra first, then its neighbours: the synthesized member's core
    is the vertebra's alone), erode radius and spacing, the two core masks.  launch() then addresses the pair."""

    def __init__(self, label_original, label_synth, ids, ct_original=None, ct_synth=None, erode_mm=0.0, spacing=(1, 1, 1), upload=True):
        self.spacing = check_spacing(spacing)
        r = check_erode(erode_mm)
        self.ids = check_labels(ids)
        if upload:
            ct_original, ct_synth, label_original, label_synth = (resident(t) for t in (ct_original, ct_synth, label_original, label_synth))
        if ct_original is None:
            check_3d(label_original, 'label_original', LABEL_DT)
            check_3d(label_synth, 'label_synth', LABEL_DT, label_original.shape)
            if label_synth.device != label_original.device:
                raise ValueError('label_original and label_synth must lie on one device')
        else:
            check_3d(ct_original, 'ct_original', VOL_DT)
            check_3d(ct_synth, 'ct_synth', VOL_DT, ct_original.shape)
            check_3d(label_original, 'label_original', LABEL_DT, ct_original.shape)
            check_3d(label_synth, 'label_synth', LABEL_DT, ct_original.shape)
            if ct_synth.dtype != ct_original.dtype:
                raise TypeError('ct_synth: the dtype of ct_original (%s) expected, got %s' % (ct_original.dtype, ct_synth.dtype))
        self.cts = None if ct_original is None else (ct_original, ct_synth)
        self.labels = (label_original, label_synth)
        first = label_original if ct_original is None else ct_original
        self.device, self.shape, self.dtype = first.device, tuple(first.shape), first.dtype
        self.masks = None
        if r > 0.0:
            self.masks = torch.empty((2,) + self.shape, dtype=torch.uint8, device=self.device)
            core_mask(label_original, self.ids, r, self.spacing, self.masks[0])
            core_mask(label_synth, self.ids[:1], r, self.spacing, self.masks[1])

    def launch(self, launch):
        """launch(vol4, label4, mask4, sel) once for the [2] batch or once per member; sel picks the members' rows of a [2][...] result."""
        for vol, label, sel in pair_plan(self.cts, self.labels):
            launch(vol, label, None if self.masks is None else self.masks[sel], sel)
