"""Per-label 3-D grey-level co-occurrence texture on the device (csrc/texture.hip through hv_glcm).

label_statistics answers whether a (synthesized) vertebra has the attenuation of the patient's intact ones; first-order statistics cannot see
structure.  The grey-level co-occurrence matrix (Haralick 1973; skimage.feature.graycomatrix carried to three dimensions and restricted to a
label) can: contrast, homogeneity, entropy and correlation of the cancellous core come from it.
  directions(distance=1)                                                                     -> the 13 unique 3-D offsets (times distance)
  glcm(vol, label, labels=None, offsets=None, levels=32, lo=-200.0, width=25.0, symmetric=True, mask=None)
                                                                                             -> dict, matrices int64 [V?][S][D][G][G]
  haralick_features(matrices)                                                                -> dict of float64 arrays [...][D] and 'mean'
  vertebra_texture(ct, label, vert_id, erode_mm=0.0, spacing=(1, 1, 1), levels=32, lo=-200.0, width=25.0, distance=1, median_size=None)
  texture_comparison(ct_original, ct_synth, label_original, label_synth, vert_id, neighbours=(), ...)
vol, label and mask are what label_statistics takes (device tensors [A0][A1][A2] or stacked [V][A0][A1][A2], any strides); a numpy array is
uploaded first.  Nothing is counted on the host: a CPU tensor is a ValueError.  The level of a voxel is floor((v - lo) / width) in float64,
clamped to [0, levels - 1]; the defaults cover -200 .. 600 HU in 32 bins of 25 HU, and the result reports how many voxels were clamped.
The matrices are exact integers (integer atomics only: the same bytes on every run); the features are numpy float64 on the host, on purpose:
the matrices are a few hundred KB at most."""
import ctypes
import math

import numpy as np
import torch

from . import lib as _lib
from . import labelled as _lb
from .label_statistics import BAD_LABEL, NONFINITE, EMPTY, MAX_LABELS, present  # noqa: F401  (the status bits of 'status')

MAX_LEVELS, MAX_OFFSETS, MAX_REACH, INFO = 64, 26, 4, 4                # HV_GLCM_* of include/hvgan.h
SYMMETRIC = 1
FEATURES = ('contrast', 'dissimilarity', 'homogeneity', 'asm', 'energy', 'entropy', 'correlation', 'max_probability')


def directions(distance=1):
    """The 13 unique 3-D offsets (one of every pair d, -d: the first non-zero component is positive), in lexicographic order, times `distance`;
    a list of distances gives them for each distance in turn (two distances: 26 offsets).  -> int64 array [D][3]."""
    ds = list(distance) if isinstance(distance, (list, tuple, np.ndarray)) else [distance]
    ok = all(isinstance(d, (int, np.integer)) and not isinstance(d, bool) and 1 <= d <= MAX_REACH for d in ds)
    if not ok or not 1 <= len(ds) <= 2 or len(set(int(d) for d in ds)) != len(ds):
        raise ValueError('distance: an integer in [1, %d] or one or two distinct ones expected, got %r' % (MAX_REACH, distance))
    unit = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) > (0, 0, 0)]
    return np.asarray([[int(d) * x for x in u] for d in ds for u in unit], dtype=np.int64)


def check_offsets(offsets):
    try:
        off = np.asarray(offsets)
        same = off.ndim == 2 and off.shape[1] == 3 and bool((off == np.floor(off)).all())
        off = off.astype(np.int64)
    except (TypeError, ValueError):
        same = False
    if not same or not 1 <= len(off) <= MAX_OFFSETS or int(np.abs(off).max()) > MAX_REACH or len(set(map(tuple, off.tolist()))) != len(off):
        raise ValueError('offsets: 1 to %d distinct integer triples with components in [-%d, %d] expected, got %r'
                         % (MAX_OFFSETS, MAX_REACH, MAX_REACH, offsets))
    return off


def check_levels(levels, lo, width):
    if isinstance(levels, bool) or not isinstance(levels, (int, np.integer)) or not 2 <= levels <= MAX_LEVELS:
        raise ValueError('levels: an integer in [2, %d] expected, got %r' % (MAX_LEVELS, levels))
    try:
        lo, width = float(lo), float(width)
    except (TypeError, ValueError):
        raise ValueError('lo, width: two numbers expected, got %r, %r' % (lo, width))
    if not math.isfinite(lo) or not math.isfinite(width) or not width > 0.0:
        raise ValueError('lo: a finite number, width: a positive finite number expected, got %r, %r' % (lo, width))
    return int(levels), lo, width


def _buffers(V, S, D, G, device):
    """One int64 allocation for out [V][S][D][G][G] and info [V][S][INFO]: one readback brings both."""
    nout = V * S * D * G * G
    buf = torch.empty((nout + V * S * INFO,), dtype=torch.int64, device=device)
    return buf, buf[:nout].view(V, S, D, G, G), buf[nout:].view(V, S, INFO)


def _launch(vol, label, mask, labels, offsets, levels, lo, width, symmetric, out, info):
    """Queue one hv_glcm on the current stream: 4-D device tensors (mask may be None), out int64 [V][S][D][G][G], info int64 [V][S][INFO]."""
    D = len(offsets)
    ws, wsz = _lb.workspace('glcm', vol, len(labels), D, levels)
    flat = [int(x) for x in np.asarray(offsets).reshape(-1)]
    _lib.get().call('hv_glcm', *_lb.volume_args(vol, label, mask, labels), (ctypes.c_int * (3 * D))(*flat), D, ctypes.c_double(lo),
                    ctypes.c_double(width), levels, SYMMETRIC if symmetric else 0, _lib.ptr(out), _lib.ptr(info), _lib.ptr(ws), wsz, _lib.stream())


def _result(buf, V, S, D, G, labels, offsets):
    """The one readback and the dict of glcm."""
    host = buf.cpu().numpy()
    nout = V * S * D * G * G
    info = host[nout:].reshape(V, S, INFO)
    return {'labels': np.asarray(labels, dtype=np.int64), 'offsets': np.asarray(offsets, dtype=np.int64),
            'matrices': host[:nout].reshape(V, S, D, G, G), 'count': info[..., 1].copy(), 'clamped_low': info[..., 2].copy(),
            'clamped_high': info[..., 3].copy(), 'status': info[..., 0].copy()}


_PER_CALL = ('labels', 'offsets')


def glcm(vol, label, labels=None, offsets=None, levels=32, lo=-200.0, width=25.0, symmetric=True, mask=None):
    """The co-occurrence matrices of `vol` inside every listed label value (up to 64) of `label`, restricted to mask != 0: for every offset d
    (default: directions(1)) and every pair of voxels p, p + d inside the volume that carry the same listed label, matrices[.., s, d, level(p),
    level(p + d)] += 1; symmetric=True adds the transpose (graycomatrix(symmetric=True): the diagonal doubled).  level = (v - lo) / width in
    float64, truncated, clamped to [0, levels - 1].  No boundary modes: a pair that leaves the volume is not counted; offset (0, 0, 0) gives the
    level histogram on the diagonal.
    -> {'labels' [S], 'offsets' [D][3], 'matrices' int64 [V][S][D][G][G] ([S][D][G][G] for one volume), 'count' (the finite voxels of the label),
    'clamped_low', 'clamped_high' (how many of them lay below lo / at or above lo + levels * width), 'status' (label_statistics' bits: 1 the
    volume holds a label that is no integer in [0, 255], 2 a NaN or infinity inside the label -- it is in no pair --, 4 no voxel)}, the last four
    [V][S] ([S]).  One launch sequence and one readback.  labels=None: the non-zero label values present, as label_statistics finds them."""
    G, lo, width = check_levels(levels, lo, width)
    off = directions(1) if offsets is None else check_offsets(offsets)
    single, v4, l4, m4 = _lb.check_inputs(vol, label, mask, upload=True)
    ids = _lb.resolve_labels(labels, lambda: present(v4, l4, m4))
    V, S, D = int(v4.shape[0]), len(ids), len(off)
    buf, out, info = _buffers(V, S, D, G, v4.device)
    _launch(v4, l4, m4, ids, off, G, lo, width, bool(symmetric), out, info)
    res = _result(buf, V, S, D, G, ids, off)
    return _lb.squeeze(res, _PER_CALL) if single else res


def haralick_features(matrices):
    """Haralick's texture features of co-occurrence matrices [...][D][G][G] (any leading axes), in numpy float64 on the host.  Per matrix
    p = P / P.sum(): contrast sum p (i - j)^2, dissimilarity sum p |i - j|, homogeneity sum p / (1 + (i - j)^2), asm sum p^2, energy sqrt(asm),
    entropy -sum p log2 p (bits), correlation sum p (i - mu_i)(j - mu_j) / (sigma_i sigma_j) (1 where a marginal's variance is 0, as
    skimage.feature.graycoprops) and max_probability.
    -> {feature: [...][D], 'mean': {feature: [...]}}, the mean over the offsets; an empty matrix gives NaN (and so does a mean over one)."""
    P = np.asarray(matrices)
    if P.ndim < 3 or P.shape[-1] != P.shape[-2] or P.shape[-1] < 1 or P.dtype.kind not in 'iuf':
        raise ValueError('matrices: an array [...][D][G][G] of counts expected, got %s' % (getattr(P, 'shape', None),))
    P = P.astype(np.float64)
    G = P.shape[-1]
    total = P.sum(axis=(-2, -1))
    empty = total == 0
    p = P / np.where(empty, 1.0, total)[..., None, None]
    i, j = np.meshgrid(np.arange(G, dtype=np.float64), np.arange(G, dtype=np.float64), indexing='ij')
    d = i - j
    s2 = lambda w: (p * w).sum(axis=(-2, -1))
    out = {'contrast': s2(d * d), 'dissimilarity': s2(np.abs(d)), 'homogeneity': s2(1.0 / (1.0 + d * d)), 'asm': s2(p)}
    out['energy'] = np.sqrt(out['asm'])
    out['entropy'] = -(p * np.log2(np.where(p > 0, p, 1.0))).sum(axis=(-2, -1))
    mi, mj = s2(i), s2(j)
    ci, cj = i - mi[..., None, None], j - mj[..., None, None]
    vi, vj = s2(ci * ci), s2(cj * cj)
    flat = (vi == 0) | (vj == 0)
    out['correlation'] = np.where(flat, 1.0, s2(ci * cj) / np.where(flat, 1.0, np.sqrt(vi) * np.sqrt(vj)))
    out['max_probability'] = p.max(axis=(-2, -1))
    for k in FEATURES:
        out[k] = np.where(empty, np.nan, out[k])
    out['mean'] = {k: out[k].mean(axis=-1) for k in FEATURES}
    return out


def _offsets_of(offsets, distance):
    return directions(distance) if offsets is None else check_offsets(offsets)


def _one(res, feats, v, s):
    """Slot s of volume v of a [V][S] result with its features."""
    out = {'label': int(res['labels'][s]), 'offsets': res['offsets'], 'matrices': res['matrices'][v, s]}
    for k in ('count', 'clamped_low', 'clamped_high', 'status'):
        out[k] = int(res[k][v, s])
    out['features'] = {k: feats[k][v, s] for k in FEATURES}
    out['features']['mean'] = {k: float(feats['mean'][k][v, s]) for k in FEATURES}
    return out


def vertebra_texture(ct, label, vert_id, erode_mm=0.0, spacing=(1, 1, 1), levels=32, lo=-200.0, width=25.0, distance=1, median_size=None,
                     offsets=None, symmetric=True):
    """The texture of one vertebra's cancellous core: glcm of `ct` inside label == vert_id under the mask and after the median pre-step of
    label_statistics.vertebra_density (erode_mm = 0: no morphology runs, no mask; median_size None: no filter runs).  The offsets are
    directions(distance) unless `offsets` lists them.
    -> {'label', 'offsets', 'matrices' [D][G][G], 'count', 'clamped_low', 'clamped_high', 'status', 'features': haralick_features of the
    matrices ([D] each, and 'mean')}."""
    off = _offsets_of(offsets, distance)
    check_levels(levels, lo, width)
    ct, label, mask, vid, _ = _lb.vertebra_inputs(ct, label, vert_id, erode_mm, spacing, median_size)
    res = glcm(ct[None], label[None], [vid], off, levels, lo, width, symmetric, None if mask is None else mask[None])
    return _one(res, haralick_features(res['matrices']), 0, 0)


def texture_comparison(ct_original, ct_synth, label_original, label_synth, vert_id, neighbours=(), erode_mm=0.0, spacing=(1, 1, 1), levels=32,
                       lo=-200.0, width=25.0, distance=1, offsets=None, symmetric=True):
    """Does the pseudo-healthy vertebra have the structure of the patient's intact ones?  The texture of vertebra vert_id in the original CT
    under the original label, in the synthesized CT under the synthesized label, and of every listed neighbour in the original CT under the
    original label, each inside its core (erode_mm as in vertebra_texture).
    -> {'original', 'synthesized': dicts as vertebra_texture's, 'neighbours': {id: dict}, 'difference': {feature: synthesized - original},
    'neighbour_difference': {id: {feature: synthesized - neighbour}}}, the differences those of the features' means over the offsets.
    The two pairs run as ONE batch (V = 2, the second volume addressed through the batch stride, no copy) when the CTs agree in dtype and
    strides and the labels do, else as two calls into one result buffer; one readback either way."""
    off = _offsets_of(offsets, distance)
    G, lo, width = check_levels(levels, lo, width)
    pair = _lb.Pair(label_original, label_synth, [vert_id] + list(neighbours), ct_original, ct_synth, erode_mm, spacing)
    ids, sym = pair.ids, bool(symmetric)
    S, D = len(ids), len(off)
    buf, out, info = _buffers(2, S, D, G, pair.device)
    pair.launch(lambda vol, label, mask, sel: _launch(vol, label, mask, ids, off, G, lo, width, sym, out[sel], info[sel]))
    res = _result(buf, 2, S, D, G, ids, off)
    feats = haralick_features(res['matrices'])
    ori, syn = _one(res, feats, 0, 0), _one(res, feats, 1, 0)
    nb = {i: _one(res, feats, 0, s) for s, i in enumerate(ids) if s > 0}
    diff = lambda a, b: {k: a['features']['mean'][k] - b['features']['mean'][k] for k in FEATURES}
    return {'original': ori, 'synthesized': syn, 'neighbours': nb, 'difference': diff(syn, ori),
            'neighbour_difference': {i: diff(syn, d) for i, d in nb.items()}}
