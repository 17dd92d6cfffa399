"""Per-label 3-D run-length, dependence and neighbourhood grey-tone texture on the device (csrc/texture_runs.hip through hv_glrlm and hv_gldm;
DESIGN.md section 8 row f21).

texture.glcm sees pairs of voxels at one offset and nothing longer.  The grey-level run-length matrix (Galloway 1975) counts, per direction, the
maximal runs of one level: a volume synthesized slice by slice keeps its levels in plane and breaks them from one slice to the next, which is a
statement about run lengths per direction.  The dependence matrix (Sun and Wee 1983) counts how many of a voxel's 26 neighbours share its
level, the neighbouring grey-tone difference matrix (Amadasun and King 1989) how far a voxel lies from the mean of its neighbours.
  glrlm(vol, label, labels=None, offsets=None, levels=32, lo=-200.0, width=25.0, max_run=None, mask=None)  -> dict, matrices int64 [V?][S][D][G][R]
  gldm(vol, label, labels=None, alpha=0, levels=32, lo=-200.0, width=25.0, mask=None)  -> dict, dependence [V?][S][G][27], ngtdm [V?][S][G][27][2]
  glrlm_features(matrices), gldm_features(dependence), ngtdm_features(ngtdm)           -> dicts of float64 arrays
  vertebra_run_texture(ct, label, vert_id, erode_mm=0.0, spacing=(1, 1, 1), levels=32, lo=-200.0, width=25.0, alpha=0, median_size=None,
                       slice_axis=2)
  run_texture_comparison(ct_original, ct_synth, label_original, label_synth, vert_id, neighbours=(), ...)
vol, label, mask, labels, levels, lo and width are texture.glcm's, and so are the slot and the level of a voxel.  Nothing is counted on the host:
a CPU tensor is a ValueError.  The matrices are exact integers (integer atomics only: the same bytes on every run); the features are numpy
float64 on the host, on purpose, as texture.haralick_features.  Their formulas are restated from the pyradiomics documentation (levels and
lengths 1-based: i = level + 1, j = run length, j = k + 1 for dependence); the package is not a dependency and the formulas are not pinned
against it -- the matrices are pinned (tests/texture_runs_ref.py)."""
import ctypes

import numpy as np
import torch

from . import lib as _lib
from . import labelled as _lb
from .label_statistics import BAD_LABEL, NONFINITE, EMPTY, MAX_LABELS, present  # noqa: F401  (the status bits of 'status')
from .texture import INFO, directions, check_levels

MAX_OFFSETS, RLM_INFO, NEIGHBOURS = 13, 17, 27                           # HV_GLRLM_MAX_OFFSETS, HV_GLRLM_INFO, HV_GLDM_NEIGHBOURS of include/hvgan.h
GLRLM_FEATURES = ('SRE', 'LRE', 'GLN', 'GLNN', 'RLN', 'RLNN', 'RP', 'GLV', 'RV', 'RE', 'LGLRE', 'HGLRE', 'SRLGLE', 'SRHGLE', 'LRLGLE', 'LRHGLE')
GLDM_FEATURES = ('SDE', 'LDE', 'GLN', 'DN', 'DNN', 'GLV', 'DV', 'DE', 'LGLE', 'HGLE', 'SDLGLE', 'SDHGLE', 'LDLGLE', 'LDHGLE')
NGTDM_FEATURES = ('coarseness', 'contrast', 'busyness', 'complexity', 'strength')
_INFO_KEYS = (('status', 0), ('count', 1), ('clamped_low', 2), ('clamped_high', 3))
_PER_CALL = ('labels', 'offsets')


def _check_run_offsets(offsets):
    try:
        off = np.asarray(offsets)
        same = off.ndim == 2 and off.shape[1] == 3 and bool((off == np.floor(off)).all())
        off = off.astype(np.int64)
    except (TypeError, ValueError):
        same = False
    rows = set(map(tuple, off.tolist())) if same else set()
    if (not same or not 1 <= len(off) <= MAX_OFFSETS or int(np.abs(off).max()) > 1 or (0, 0, 0) in rows or len(rows) != len(off)
            or any(tuple(-c for c in r) in rows for r in rows)):
        raise ValueError('offsets: 1 to %d distinct non-zero triples with components in {-1, 0, 1}, none beside its negative, expected, got %r'
                         % (MAX_OFFSETS, offsets))
    return off


def _check_int(x, name, lo, hi):
    if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or not lo <= x <= hi:
        raise ValueError('%s: an integer in [%d, %d] expected, got %r' % (name, lo, hi, x))
    return int(x)


def _inputs(vol, label, mask, labels):
    """The resident 4-D tensors and the label ids of glrlm and gldm -> (single, vol, label, mask, ids)."""
    single, v4, l4, m4 = _lb.check_inputs(vol, label, mask, upload=True)
    return single, v4, l4, m4, _lb.resolve_labels(labels, lambda: present(v4, l4, m4))


def _launch_glrlm(vol, label, mask, labels, offsets, levels, lo, width, R, out, info):
    """Queue one hv_glrlm on the current stream: 4-D device tensors (mask may be None), out int64 [V][S][D][G][R], info int64 [V][S][RLM_INFO]."""
    D = len(offsets)
    ws, wsz = _lb.workspace('glrlm', vol, len(labels), D, levels, R)
    flat = [int(x) for x in np.asarray(offsets).reshape(-1)]
    _lib.get().call('hv_glrlm', *_lb.volume_args(vol, label, mask, labels), (ctypes.c_int * (3 * D))(*flat), D, ctypes.c_double(lo),
                    ctypes.c_double(width), levels, R, _lib.ptr(out), _lib.ptr(info), _lib.ptr(ws), wsz, _lib.stream())


def _launch_gldm(vol, label, mask, labels, levels, lo, width, alpha, dep, ngt, info):
    """Queue one hv_gldm on the current stream: dep int64 [V][S][G][27], ngt int64 [V][S][G][27][2], info int64 [V][S][INFO]."""
    ws, wsz = _lb.workspace('gldm', vol, len(labels), levels)
    _lib.get().call('hv_gldm', *_lb.volume_args(vol, label, mask, labels), ctypes.c_double(lo), ctypes.c_double(width), levels, alpha, _lib.ptr(dep),
                    _lib.ptr(ngt), _lib.ptr(info), _lib.ptr(ws), wsz, _lib.stream())


class _Buffers:
    """One int64 allocation for every output of a call (one readback brings them all): any of out [V][S][D][G][R] with info_r [V][S][RLM_INFO],
    and dep [V][S][G][27] with ngt [V][S][G][27][2] and info_d [V][S][INFO]."""

    def __init__(self, V, S, G, device, D=0, R=0, runs=True, neighbours=True):
        shapes = {}
        if runs:
            shapes.update(out=(V, S, D, G, R), info_r=(V, S, RLM_INFO))
        if neighbours:
            shapes.update(dep=(V, S, G, NEIGHBOURS), ngt=(V, S, G, NEIGHBOURS, 2), info_d=(V, S, INFO))
        self.shapes, self.at, n = shapes, {}, 0
        for k, sh in shapes.items():
            self.at[k] = n
            n += int(np.prod(sh))
        self.buf = torch.empty((n,), dtype=torch.int64, device=device)

    def dev(self, k):
        return self.buf[self.at[k]:self.at[k] + int(np.prod(self.shapes[k]))].view(self.shapes[k])

    def read(self):
        """The one readback -> {name: numpy array}."""
        host = self.buf.cpu().numpy()
        return {k: host[self.at[k]:self.at[k] + int(np.prod(sh))].reshape(sh) for k, sh in self.shapes.items()}


def _info_dict(info):
    return {k: info[..., c].copy() for k, c in _INFO_KEYS}


def _glrlm_result(host, labels, offsets):
    res = {'labels': np.asarray(labels, dtype=np.int64), 'offsets': np.asarray(offsets, dtype=np.int64), 'matrices': host['out']}
    res.update(_info_dict(host['info_r']))
    res['capped'] = host['info_r'][..., INFO:INFO + len(offsets)].copy()
    return res


def _gldm_result(host, labels):
    res = {'labels': np.asarray(labels, dtype=np.int64), 'dependence': host['dep'], 'ngtdm': host['ngt']}
    res.update(_info_dict(host['info_d']))
    return res


def glrlm(vol, label, labels=None, offsets=None, levels=32, lo=-200.0, width=25.0, max_run=None, mask=None):
    """The run-length matrices of `vol` inside every listed label value (up to 64) of `label`, restricted to mask != 0.  A run along offset d
    (default: directions(1), the 13 unique 3-D directions; components in {-1, 0, 1}, d and -d give the same runs and may not both be listed) is a
    maximal sequence p, p + d, ..., p + (L - 1) d of voxels of one label and one level; matrices[.., s, d, level, min(L, max_run) - 1] += 1.
    max_run (default: the longest axis, so nothing is capped) is the number of length bins; 'capped' counts the runs longer than that.
    -> {'labels' [S], 'offsets' [D][3], 'matrices' int64 [V][S][D][G][R] ([S][D][G][R] for one volume), 'count', 'clamped_low', 'clamped_high',
    'status' as texture.glcm's [V][S] ([S]), 'capped' [V][S][D] ([S][D])}.  One launch sequence and one readback."""
    G, lo, width = check_levels(levels, lo, width)
    off = directions(1) if offsets is None else _check_run_offsets(offsets)
    R = None if max_run is None else _check_int(max_run, 'max_run', 1, 1 << 30)
    single, v4, l4, m4, ids = _inputs(vol, label, mask, labels)
    R = R or max(int(s) for s in v4.shape[1:])
    b = _Buffers(int(v4.shape[0]), len(ids), G, v4.device, D=len(off), R=R, neighbours=False)
    _launch_glrlm(v4, l4, m4, ids, off, G, lo, width, R, b.dev('out'), b.dev('info_r'))
    res = _glrlm_result(b.read(), ids, off)
    return _lb.squeeze(res, _PER_CALL) if single else res


def gldm(vol, label, labels=None, alpha=0, levels=32, lo=-200.0, width=25.0, mask=None):
    """The dependence matrix and the neighbourhood grey-tone sums of `vol` inside every listed label value of `label`, restricted to mask != 0.
    For a voxel of level i: of its 26 neighbours inside the volume with the same label (a NaN has none), n is their number, A the sum of their
    levels and k how many lie within `alpha` levels of i.  dependence[.., s, i, k] += 1 (column k + 1 of the pyradiomics matrix);
    ngtdm[.., s, i, n, 0] += 1 and ngtdm[.., s, i, n, 1] += |i n - A| (ngtdm_features divides by n on the host: exact in any order).
    -> {'labels' [S], 'dependence' int64 [V][S][G][27], 'ngtdm' int64 [V][S][G][27][2], 'count', 'clamped_low', 'clamped_high', 'status'}, without
    the leading axis for one volume.  One launch sequence and one readback."""
    G, lo, width = check_levels(levels, lo, width)
    alpha = _check_int(alpha, 'alpha', 0, G - 1)
    single, v4, l4, m4, ids = _inputs(vol, label, mask, labels)
    b = _Buffers(int(v4.shape[0]), len(ids), G, v4.device, runs=False)
    _launch_gldm(v4, l4, m4, ids, G, lo, width, alpha, b.dev('dep'), b.dev('ngt'), b.dev('info_d'))
    res = _gldm_result(b.read(), ids)
    return _lb.squeeze(res, _PER_CALL) if single else res


# ------------------------------------------------------------------------------------------------ host features
def _counts(matrices, name, ndim):
    P = np.asarray(matrices)
    if P.ndim < ndim or P.shape[-1] < 1 or P.shape[-2] < 1 or P.dtype.kind not in 'iuf':
        raise ValueError('%s: an array of counts with at least %d axes expected, got %s' % (name, ndim, getattr(P, 'shape', None)))
    return P.astype(np.float64)


def _matrix_features(P, names):
    """What the run-length and the dependence features share, for P [...][G][J] (rows: level i = 1 .. G, columns: j = 1 .. J).
    -> ({name: [...]}, N [...], empty [...], the level margin [...][G], N with 1 for 0), names: (short, long, level non-uniformity, length non-uniformity and its normalised form, level
    variance, length variance, entropy, low, high level emphasis, short low, short high, long low, long high)."""
    G, J = P.shape[-2:]
    N = P.sum(axis=(-2, -1))
    empty = N == 0
    Ns = np.where(empty, 1.0, N)
    i = np.arange(1, G + 1, dtype=np.float64)[:, None]
    j = np.arange(1, J + 1, dtype=np.float64)[None, :]
    s2 = lambda w: (P * w).sum(axis=(-2, -1)) / Ns
    p = P / Ns[..., None, None]
    pg, pj = P.sum(axis=-1), P.sum(axis=-2)
    mu_i, mu_j = s2(i), s2(j)
    short, long_, gln, ln, lnn, glv, lv, ent, low, high, sl, sh, ll, lh = names
    f = {short: s2(1.0 / (j * j)), long_: s2(j * j), gln: (pg * pg).sum(axis=-1) / Ns, ln: (pj * pj).sum(axis=-1) / Ns,
         lnn: (pj * pj).sum(axis=-1) / (Ns * Ns), glv: (p * (i - mu_i[..., None, None]) ** 2).sum(axis=(-2, -1)),
         lv: (p * (j - mu_j[..., None, None]) ** 2).sum(axis=(-2, -1)), ent: -(p * np.log2(np.where(p > 0, p, 1.0))).sum(axis=(-2, -1)),
         low: s2(1.0 / (i * i)), high: s2(i * i), sl: s2(1.0 / (i * i * j * j)), sh: s2(i * i / (j * j)), ll: s2(j * j / (i * i)),
         lh: s2(i * i * j * j)}
    return f, N, empty, pg, Ns


def glrlm_features(matrices):
    """The sixteen pyradiomics GLRLM features of run-length matrices [...][D][G][R] (any leading axes), numpy float64 on the host.  With P(i, j)
    the runs of level i and length j, Nr = sum P, Np = sum j P(i, j) (the voxels in runs), p = P / Nr: SRE sum P / j^2 / Nr, LRE sum P j^2 / Nr,
    GLN sum_i (sum_j P)^2 / Nr, GLNN GLN / Nr, RLN sum_j (sum_i P)^2 / Nr, RLNN RLN / Nr, RP Nr / Np, GLV and RV the variances of i and j under p,
    RE -sum p log2 p (0 log 0 = 0), LGLRE sum P / i^2 / Nr, HGLRE sum P i^2 / Nr, SRLGLE sum P / (i^2 j^2) / Nr, SRHGLE sum P i^2 / j^2 / Nr,
    LRLGLE sum P j^2 / i^2 / Nr, LRHGLE sum P i^2 j^2 / Nr.
    -> {feature: [...][D], 'mean_run': [...][D] (Np / Nr), 'mean': {feature: [...]}}, the mean over the directions; an empty matrix gives NaN."""
    P = _counts(matrices, 'matrices', 3)
    f, N, empty, pg, Ns = _matrix_features(P, ('SRE', 'LRE', 'GLN', 'RLN', 'RLNN', 'GLV', 'RV', 'RE', 'LGLRE', 'HGLRE', 'SRLGLE', 'SRHGLE',
                                                'LRLGLE', 'LRHGLE'))
    f['GLNN'] = (pg * pg).sum(axis=-1) / (Ns * Ns)
    Np = (P * np.arange(1, P.shape[-1] + 1, dtype=np.float64)).sum(axis=(-2, -1))
    f['RP'] = N / np.where(empty, 1.0, Np)
    out = {k: np.where(empty, np.nan, f[k]) for k in GLRLM_FEATURES}
    out['mean_run'] = np.where(empty, np.nan, Np / Ns)
    out['mean'] = {k: out[k].mean(axis=-1) for k in GLRLM_FEATURES}
    return out


def gldm_features(dependence):
    """The fourteen pyradiomics GLDM features of dependence matrices [...][G][27], numpy float64 on the host.  With P(i, j) the voxels of level i
    with j - 1 dependent neighbours (j = k + 1), Nz = sum P, p = P / Nz: SDE sum P / j^2 / Nz, LDE sum P j^2 / Nz, GLN sum_i (sum_j P)^2 / Nz,
    DN sum_j (sum_i P)^2 / Nz, DNN DN / Nz, GLV and DV the variances of i and j under p, DE -sum p log2 p, LGLE sum P / i^2 / Nz, HGLE
    sum P i^2 / Nz, SDLGLE sum P / (i^2 j^2) / Nz, SDHGLE sum P i^2 / j^2 / Nz, LDLGLE sum P j^2 / i^2 / Nz, LDHGLE sum P i^2 j^2 / Nz.
    -> {feature: [...]}; an empty matrix gives NaN."""
    P = _counts(dependence, 'dependence', 2)
    f, _, empty, _, _ = _matrix_features(P, GLDM_FEATURES)
    return {k: np.where(empty, np.nan, f[k]) for k in GLDM_FEATURES}


def ngtdm_table(ngtdm):
    """ngtdm [...][G][27][2] -> (n_i [...][G], s_i [...][G]): the voxels of level i with at least one neighbour, and the sum of their distances
    |i - mean of the neighbours' levels|, each numerator over its own denominator n."""
    T = np.asarray(ngtdm)
    if T.ndim < 3 or T.shape[-1] != 2 or T.shape[-2] < 2 or T.dtype.kind not in 'iuf':
        raise ValueError('ngtdm: an array [...][G][27][2] of sums expected, got %s' % (getattr(T, 'shape', None),))
    T = T.astype(np.float64)
    n = np.arange(1, T.shape[-2], dtype=np.float64)
    return T[..., 1:, 0].sum(axis=-1), (T[..., 1:, 1] / n).sum(axis=-1)


def ngtdm_features(ngtdm):
    """Amadasun and King's five features of the neighbourhood sums [...][G][27][2], numpy float64 on the host.  With n_i, s_i of ngtdm_table,
    Nvp = sum n_i, p_i = n_i / Nvp, Ngp the levels with p_i > 0, and every double sum over the pairs with p_i > 0 and p_j > 0: coarseness
    1 / sum p_i s_i (1e6 where the sum is 0), contrast (sum_ij p_i p_j (i - j)^2 / (Ngp (Ngp - 1))) (sum s_i / Nvp) (0 for Ngp = 1), busyness
    sum p_i s_i / sum_ij |i p_i - j p_j| (0 where the denominator is 0), complexity sum_ij |i - j| (p_i s_i + p_j s_j) / (p_i + p_j) / Nvp,
    strength sum_ij (p_i + p_j) (i - j)^2 / sum s_i (0 where sum s_i = 0).
    -> {feature: [...]}; no voxel with a neighbour gives NaN."""
    n, s = ngtdm_table(ngtdm)
    G = n.shape[-1]
    Nvp = n.sum(axis=-1)
    empty = Nvp == 0
    Ns = np.where(empty, 1.0, Nvp)
    p = n / Ns[..., None]
    lev = np.arange(1, G + 1, dtype=np.float64)
    on = p > 0
    both = on[..., :, None] & on[..., None, :]
    pi, pj, si, sj = p[..., :, None], p[..., None, :], s[..., :, None], s[..., None, :]
    di = lev[:, None] - lev[None, :]
    ps, ssum, Ngp = (p * s).sum(axis=-1), s.sum(axis=-1), on.sum(axis=-1).astype(np.float64)
    f = {'coarseness': np.where(ps == 0, 1e6, 1.0 / np.where(ps == 0, 1.0, ps))}
    f['contrast'] = np.where(Ngp > 1, (pi * pj * di * di).sum(axis=(-2, -1)) / np.where(Ngp > 1, Ngp * (Ngp - 1), 1.0) * ssum / Ns, 0.0)
    den = np.where(both, np.abs(lev[:, None] * pi - lev[None, :] * pj), 0.0).sum(axis=(-2, -1))
    f['busyness'] = np.where(den == 0, 0.0, ps / np.where(den == 0, 1.0, den))
    f['complexity'] = np.where(both, np.abs(di) * (pi * si + pj * sj) / np.where(both, pi + pj, 1.0), 0.0).sum(axis=(-2, -1)) / Ns
    num = np.where(both, (pi + pj) * di * di, 0.0).sum(axis=(-2, -1))
    f['strength'] = np.where(ssum == 0, 0.0, num / np.where(ssum == 0, 1.0, ssum))
    return {k: np.where(empty, np.nan, f[k]) for k in NGTDM_FEATURES}


# ------------------------------------------------------------------------------------------------ one vertebra
def _axis_offsets(slice_axis):
    """The three axis-aligned unit offsets, `slice_axis`' first, and where each lies in directions(1)."""
    axis = _check_int(slice_axis, 'slice_axis', 0, 2)
    rows = [tuple(r) for r in directions(1).tolist()]
    order = [axis] + [a for a in range(3) if a != axis]
    return [rows.index(tuple(1 if c == a else 0 for c in range(3))) for a in order]


def run_anisotropy(mean_run, slice_axis=2):
    """mean_run [...][13] over directions(1) -> the mean run length along `slice_axis` over the mean of the other two axes' (below 1: runs break
    from slice to slice more often than inside a slice)."""
    along, a, b = _axis_offsets(slice_axis)
    m = np.asarray(mean_run, dtype=np.float64)
    return m[..., along] / ((m[..., a] + m[..., b]) / 2.0)


def _one(host, feats, labels, offsets, v, s, slice_axis):
    """Slot s of volume v of a batch's readback with its features."""
    info = host['info_d']
    out = {'label': int(labels[s]), 'offsets': np.asarray(offsets, dtype=np.int64), 'glrlm': host['out'][v, s], 'dependence': host['dep'][v, s],
           'ngtdm': host['ngt'][v, s], 'capped': host['info_r'][v, s, INFO:INFO + len(offsets)].copy()}
    for k, c in _INFO_KEYS:
        out[k] = int(info[v, s, c])
    r, d, n = feats
    f = {'glrlm': {k: r[k][v, s] for k in GLRLM_FEATURES + ('mean_run',)}, 'gldm': {k: float(d[k][v, s]) for k in GLDM_FEATURES},
         'ngtdm': {k: float(n[k][v, s]) for k in NGTDM_FEATURES}}
    f['glrlm']['mean'] = {k: float(r['mean'][k][v, s]) for k in GLRLM_FEATURES}
    out['features'] = f
    out['run_anisotropy'] = float(run_anisotropy(r['mean_run'][v, s], slice_axis))
    return out


def _features(host):
    return glrlm_features(host['out']), gldm_features(host['dep']), ngtdm_features(host['ngt'])


def _launch_both(vol, label, mask, ids, off, G, lo, width, alpha, R, b, sel=slice(None)):
    _launch_glrlm(vol, label, mask, ids, off, G, lo, width, R, b.dev('out')[sel], b.dev('info_r')[sel])
    _launch_gldm(vol, label, mask, ids, G, lo, width, alpha, b.dev('dep')[sel], b.dev('ngt')[sel], b.dev('info_d')[sel])


def vertebra_run_texture(ct, label, vert_id, erode_mm=0.0, spacing=(1, 1, 1), levels=32, lo=-200.0, width=25.0, alpha=0, median_size=None,
                         slice_axis=2):
    """The run-length, dependence and neighbourhood texture of one vertebra's cancellous core: glrlm (the 13 directions, nothing capped) and gldm
    of `ct` inside label == vert_id under the mask and after the median pre-step of texture.vertebra_texture.
    -> {'label', 'offsets', 'glrlm' [13][G][R], 'dependence' [G][27], 'ngtdm' [G][27][2], 'capped', 'count', 'clamped_low', 'clamped_high',
    'status', 'features': {'glrlm': glrlm_features ([13] each, 'mean_run' and 'mean'), 'gldm': gldm_features, 'ngtdm': ngtdm_features},
    'run_anisotropy': the mean run length along the unit offset of `slice_axis` over the mean of the other two axis-aligned ones}."""
    G, lo, width = check_levels(levels, lo, width)
    alpha = _check_int(alpha, 'alpha', 0, G - 1)
    _axis_offsets(slice_axis)
    ct, label, mask, vid, _ = _lb.vertebra_inputs(ct, label, vert_id, erode_mm, spacing, median_size)
    off, R = directions(1), max(int(s) for s in ct.shape)
    b = _Buffers(1, 1, G, ct.device, D=len(off), R=R)
    _launch_both(ct[None], label[None], None if mask is None else mask[None], [vid], off, G, lo, width, alpha, R, b)
    host = b.read()
    return _one(host, _features(host), [vid], off, 0, 0, slice_axis)


def run_texture_comparison(ct_original, ct_synth, label_original, label_synth, vert_id, neighbours=(), erode_mm=0.0, spacing=(1, 1, 1),
                           levels=32, lo=-200.0, width=25.0, alpha=0, slice_axis=2):
    """texture.texture_comparison for the run-length and neighbourhood classes: vertebra vert_id in the original CT under the original label, in the
    synthesized CT under the synthesized label, and every listed neighbour in the original CT under the original label, each inside its core.
    -> {'original', 'synthesized': dicts as vertebra_run_texture's, 'neighbours': {id: dict}, 'difference': synthesized - original as
    {'glrlm': {feature: mean over the directions}, 'gldm': {feature}, 'ngtdm': {feature}, 'run_anisotropy'}, 'neighbour_difference': {id: the same,
    synthesized - neighbour}}.  The two pairs run as ONE batch (V = 2, the second volume addressed through the batch stride, no copy) when the
    CTs agree in dtype and strides and the labels do, else as two calls into one result buffer; one readback either way."""
    G, lo, width = check_levels(levels, lo, width)
    alpha = _check_int(alpha, 'alpha', 0, G - 1)
    _axis_offsets(slice_axis)
    pair = _lb.Pair(label_original, label_synth, [vert_id] + list(neighbours), ct_original, ct_synth, erode_mm, spacing)
    ids, off, R = pair.ids, directions(1), max(pair.shape)
    b = _Buffers(2, len(ids), G, pair.device, D=len(off), R=R)
    pair.launch(lambda vol, label, mask, sel: _launch_both(vol, label, mask, ids, off, G, lo, width, alpha, R, b, sel))
    host = b.read()
    feats = _features(host)
    ori, syn = _one(host, feats, ids, off, 0, 0, slice_axis), _one(host, feats, ids, off, 1, 0, slice_axis)
    nb = {i: _one(host, feats, ids, off, 0, s, slice_axis) for s, i in enumerate(ids) if s > 0}

    def diff(x, y):
        fx, fy = x['features'], y['features']
        return {'glrlm': {k: fx['glrlm']['mean'][k] - fy['glrlm']['mean'][k] for k in GLRLM_FEATURES},
                'gldm': {k: fx['gldm'][k] - fy['gldm'][k] for k in GLDM_FEATURES},
                'ngtdm': {k: fx['ngtdm'][k] - fy['ngtdm'][k] for k in NGTDM_FEATURES},
                'run_anisotropy': x['run_anisotropy'] - y['run_anisotropy']}

    return {'original': ori, 'synthesized': syn, 'neighbours': nb, 'difference': diff(syn, ori),
            'neighbour_difference': {i: diff(syn, d) for i, d in nb.items()}}
