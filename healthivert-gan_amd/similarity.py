"""Joint-histogram similarity of two resident volumes and rigid registration on it (csrc/similarity.hip through hv_joint_hist; DESIGN.md
section 8 row f18).

resample, warp and straighten apply a transform; this module finds one.  A follow-up scan is never on the baseline's lattice, and
density_comparison / texture_comparison / feather_blend mean something only when the two volumes are in one frame.  The measure is the joint
histogram of the fixed volume and the moving volume sampled under a pose, and what is derived from it: mutual information (Collignon 1995;
Viola and Wells 1997), the normalised form (Studholme 1999) and the entropy correlation coefficient.
  joint_histogram(fixed, moving, poses=None, *, bins=32, fixed_range=(-200., 600.), moving_range=None, mask=None, order=1, prefilter=True)
                                                                                  -> JointHistogram: hist int64 [K, Gf, Gm], info int64 [K, 8]
  entropies(h) / mutual_information(h) / normalized_mutual_information(h) / entropy_correlation(h)   one value per pose   (host, float64)
  rigid_pose(params, shape_fixed, shape_moving, spacing_fixed=(1, 1, 1), spacing_moving=(1, 1, 1))  -> (matrix, offset)  (host, float64)
  similarity_sweep(fixed, moving, poses, metric='nmi', **kw)                      -> the score of every pose, one readback
  register_rigid(fixed, moving, *, spacing_fixed, spacing_moving, start=None, steps_deg=(4., 2., 1., .5), steps_mm=(4., 2., 1., .5),
                 metric='nmi', max_moves=64, **kw)                                -> Registration
  align(fixed, moving, reg, output=None, order=3, ...)                            the moving volume on the fixed lattice (affine_transform)
Volumes are 3-D device tensors with any strides, uint8 / int16 / float32 / float64 (bool becomes uint8); numpy arrays are uploaded first.  A
pose is affine_transform's (matrix [3][3], offset [3]): fixed voxel o reads the moving volume at matrix @ o + offset.  Only the overlap is
measured: a fixed voxel whose image leaves the moving volume is in no pair and is counted in info[:, 4].  The level of a value is
floor((v - lo) / width) clamped to [0, G - 1], as in texture.glcm; a range (lo, hi) gives width = (hi - lo) / G.

The histograms are exact integers (integer atomics only: the same bytes on every run) and every score is numpy float64 on the host, on
purpose, as texture.haralick_features: the search's trajectory is a pure function of its inputs.  Each public function does one readback per
call of the device (register_rigid: one per 13-pose step)."""
import ctypes
import math
from collections import namedtuple

import numpy as np
import torch

from . import lib as _lib
from . import resample as _rs
from .components import _device, _ll
from .label_statistics import NONFINITE, EMPTY  # noqa: F401  (the status bits of info[:, 0])

MAX_LEVELS, MAX_POSES, INFO = 64, 16, 8                              # HV_JH_* of include/hvgan.h
STATUS, COUNT, MASKED, NOT_FINITE, OUTSIDE, FIXED_LOW, FIXED_HIGH, MOVING_CLAMPED = range(INFO)
METRICS = ('mi', 'nmi', 'ecc')
SEARCH_POSES = 13                                                    # the current pose and each of six parameters plus and minus a step

JointHistogram = namedtuple('JointHistogram', 'hist info')
Registration = namedtuple('Registration', 'params matrix offset score history calls')


# ------------------------------------------------------------------------------------------------ host: checks
def _check_bins(bins):
    b = (bins, bins) if isinstance(bins, (int, np.integer)) and not isinstance(bins, bool) else tuple(bins)
    if len(b) != 2 or any(isinstance(g, bool) or not isinstance(g, (int, np.integer)) or not 2 <= g <= MAX_LEVELS for g in b):
        raise ValueError('bins: an integer in [2, %d] or a pair of them expected, got %r' % (MAX_LEVELS, bins))
    return int(b[0]), int(b[1])


def _check_range(rng, G, name):
    try:
        lo, hi = (float(x) for x in rng)
    except (TypeError, ValueError):
        raise ValueError('%s: a pair (lo, hi) of numbers expected, got %r' % (name, rng))
    width = (hi - lo) / G
    if not math.isfinite(lo) or not math.isfinite(width) or not width > 0.0:
        raise ValueError('%s: finite lo < hi expected, got %r' % (name, rng))
    return lo, width


def _check_poses(poses):
    """-> float64 [n][12]: matrix[9] then offset[3] of every pose.  None: the identity; one (matrix, offset) pair; a sequence of pairs."""
    def is_pair(p):
        try:
            return len(p) == 2 and np.shape(p[0]) == (3, 3) and np.shape(p[1]) == (3,)
        except (TypeError, ValueError):                              # a ragged sequence: a list of pairs, not a pair
            return False

    if poses is None:
        poses = [(np.eye(3), np.zeros(3))]
    elif is_pair(poses):
        poses = [poses]
    rows = []
    for p in poses:
        if not is_pair(p):
            raise ValueError('poses: (matrix [3][3], offset [3]) pairs expected')
        rows.append(np.concatenate([np.asarray(p[0], dtype=np.float64).reshape(9), np.asarray(p[1], dtype=np.float64)]))
    out = np.asarray(rows, dtype=np.float64).reshape(-1, 12)
    if len(out) < 1 or not np.isfinite(out).all():
        raise ValueError('poses: at least one pose of finite numbers expected')
    return out


def _volume(x, name, dev, shape=None, dtypes=None):
    t = torch.as_tensor(x)
    if t.dim() != 3 or 0 in tuple(t.shape):
        raise ValueError('%s: a non-empty 3-D volume expected, got shape %s' % (name, tuple(t.shape)))
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError('%s: shape %s expected, got %s' % (name, tuple(shape), tuple(t.shape)))
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    if t.dtype not in (dtypes or _rs._DT):
        raise TypeError('%s: a uint8 / int16 / float32 / float64 (or bool) volume expected, got %s' % (name, t.dtype))
    if t.numel() > 2 ** 30:
        raise ValueError('%s: at most 2^30 voxels are supported' % name)
    t = t.to(dev)
    _lib.require_gpu(t)
    return t


def _prepare(fixed, moving, mask, order, prefilter):
    """The three device tensors the entry reads; at order 3 the moving one is the float64 coefficient volume (made here if prefilter)."""
    if isinstance(order, bool) or not isinstance(order, (int, np.integer)) or int(order) not in _rs.ORDERS:
        raise ValueError('order: 0, 1 or 3 expected, got %r' % (order,))
    dev = _device(fixed, moving)
    f, m = _volume(fixed, 'fixed', dev), _volume(moving, 'moving', dev)
    k = None if mask is None else _volume(mask, 'mask', dev, f.shape, (torch.uint8,))
    if int(order) == 3:
        if prefilter:
            m = _rs.spline_filter(m)
        elif m.dtype != torch.float64:
            raise TypeError('prefilter=False at order 3: the float64 coefficients of resample.spline_filter() expected, got %s' % (m.dtype,))
    return f, m, k, int(order)


# ------------------------------------------------------------------------------------------------ the launch
def _launch(f, m, k, poses, order, flo, fwidth, Gf, mlo, mwidth, Gm, out, info):
    """Queue one hv_joint_hist on the current stream: up to 16 poses [n][12], out int64 [n][Gf][Gm], info int64 [n][INFO]."""
    L = _lib.get()
    n = len(poses)
    flat = (ctypes.c_double * (12 * n))(*[float(x) for x in poses.reshape(-1)])
    kst = k.stride() if k is not None else (0, 0, 0)
    with torch.cuda.device(f.device):
        L.call('hv_joint_hist', _lib.ptr(f), _rs._DT[f.dtype], *_ll(f.stride()), *(int(s) for s in f.shape), _lib.ptr(m), _rs._DT[m.dtype],
               *_ll(m.stride()), *(int(s) for s in m.shape), _lib.ptr(k), *_ll(kst), flat, n, order, ctypes.c_double(flo), ctypes.c_double(fwidth),
               Gf, ctypes.c_double(mlo), ctypes.c_double(mwidth), Gm, _lib.ptr(out), _lib.ptr(info), None, ctypes.c_size_t(0), _lib.stream())


def _histograms(f, m, k, poses, order, bins, fixed_range, moving_range):
    """Every pose in chunks of 16 into one buffer, then the one readback."""
    Gf, Gm = _check_bins(bins)
    flo, fwidth = _check_range(fixed_range, Gf, 'fixed_range')
    mlo, mwidth = _check_range(fixed_range if moving_range is None else moving_range, Gm, 'moving_range')
    n, G2 = len(poses), Gf * Gm
    buf = torch.empty((n * (G2 + INFO),), dtype=torch.int64, device=f.device)
    out, info = buf[:n * G2].view(n, Gf, Gm), buf[n * G2:].view(n, INFO)
    for c in range(0, n, MAX_POSES):
        _launch(f, m, k, poses[c:c + MAX_POSES], order, flo, fwidth, Gf, mlo, mwidth, Gm, out[c:c + MAX_POSES], info[c:c + MAX_POSES])
    host = buf.cpu().numpy()
    return JointHistogram(host[:n * G2].reshape(n, Gf, Gm), host[n * G2:].reshape(n, INFO))


def joint_histogram(fixed, moving, poses=None, *, bins=32, fixed_range=(-200.0, 600.0), moving_range=None, mask=None, order=1, prefilter=True):
    """The joint histogram of `fixed` and of `moving` sampled at matrix @ o + offset, for every pose: hist[k, level(fixed(o)), level(sample)] +=
    1 over the fixed voxels o with mask(o) != 0 whose image lies inside the moving volume (no cval is invented) and whose two values are finite.
    poses: None (the identity), one (matrix, offset) pair or a sequence of them of any length (run in chunks of 16, no readback in between).
    bins: G or (Gf, Gm), each in [2, 64]; a range (lo, hi) gives width = (hi - lo) / G, moving_range=None takes fixed_range.  order 0 / 1 / 3;
    at order 3 the coefficients are made once per call (prefilter=False: `moving` holds them already).
    -> JointHistogram(hist int64 [K, Gf, Gm], info int64 [K, 8]): info[:, 0] the status (label_statistics' bits: 2 a NaN or infinity was met,
    4 no pair), [1] counted pairs, [2] masked out, [3] not finite, [4] outside, [5] / [6] counted pairs whose fixed level was clamped from below /
    above, [7] whose moving level was clamped.  [1] + [2] + [3] + [4] is the number of fixed voxels.  One readback."""
    p = _check_poses(poses)
    f, m, k, order = _prepare(fixed, moving, mask, order, prefilter)
    return _histograms(f, m, k, p, order, bins, fixed_range, moving_range)


# ------------------------------------------------------------------------------------------------ host: the measures
def _hist_of(h):
    P = np.asarray(h.hist if isinstance(h, JointHistogram) else h)
    if P.ndim == 2:
        P = P[None]
    if P.ndim != 3 or P.dtype.kind not in 'iuf':
        raise ValueError('h: a JointHistogram or an array [K][Gf][Gm] of counts expected, got shape %s' % (P.shape,))
    return P.astype(np.float64)


def _plogp(p):
    return p * np.log(np.where(p > 0, p, 1.0))                       # 0 log 0 = 0


def entropies(h):
    """(H_f, H_m, H_fm), each [K]: the entropies of the two marginals and of the joint distribution p = hist / hist.sum(), natural logarithms,
    0 log 0 = 0.  An empty histogram gives NaN."""
    P = _hist_of(h)
    total = P.sum(axis=(1, 2))
    empty = total == 0
    p = P / np.where(empty, 1.0, total)[:, None, None]
    hf = -_plogp(p.sum(axis=2)).sum(axis=1)
    hm = -_plogp(p.sum(axis=1)).sum(axis=1)
    hfm = -_plogp(p).sum(axis=(1, 2))
    nan = np.where(empty, np.nan, 0.0)
    return hf + nan, hm + nan, hfm + nan


def mutual_information(h):
    """H_f + H_m - H_fm per pose (nats)."""
    hf, hm, hfm = entropies(h)
    return (hf + hm) - hfm


def normalized_mutual_information(h):
    """(H_f + H_m) / H_fm per pose (Studholme 1999): 1 for independent volumes, 2 for one a function of the other.  NaN where H_fm == 0 (every
    pair in one bin) and for an empty histogram."""
    hf, hm, hfm = entropies(h)
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(hfm > 0, (hf + hm) / np.where(hfm > 0, hfm, 1.0), np.nan)


def entropy_correlation(h):
    """2 (H_f + H_m - H_fm) / (H_f + H_m) per pose, in [0, 1].  NaN where H_f + H_m == 0 and for an empty histogram."""
    hf, hm, hfm = entropies(h)
    s = hf + hm
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(s > 0, 2.0 * (s - hfm) / np.where(s > 0, s, 1.0), np.nan)


_METRIC = {'mi': mutual_information, 'nmi': normalized_mutual_information, 'ecc': entropy_correlation}


def _check_metric(metric):
    if metric not in _METRIC:
        raise ValueError('metric: one of %s expected, got %r' % (', '.join(METRICS), metric))
    return _METRIC[metric]


# ------------------------------------------------------------------------------------------------ host: rigid poses
def _vec(v, name, n=3, positive=False):
    a = np.asarray(v, dtype=np.float64)
    if a.shape != (n,) or not np.isfinite(a).all() or (positive and not (a > 0).all()):
        raise ValueError('%s: %d finite%s numbers expected, got %r' % (name, n, ' positive' if positive else '', v))
    return a


def rotation_matrix(angles_deg):
    """R = R2 @ R1 @ R0: the rotation by angles_deg[0] about array axis 0 is applied first, then about axis 1, then about axis 2; each turns
    the other two axes (b, c) in cyclic order by [[cos, -sin], [sin, cos]]."""
    a = _vec(angles_deg, 'angles_deg')
    r = np.eye(3)
    for axis in range(3):
        t = math.radians(float(a[axis]))
        c, s = math.cos(t), math.sin(t)
        b, d = (axis + 1) % 3, (axis + 2) % 3
        q = np.eye(3)
        q[b, b], q[b, d], q[d, b], q[d, d] = c, -s, s, c
        r = q @ r
    return r


def rigid_pose(params, shape_fixed, shape_moving, spacing_fixed=(1, 1, 1), spacing_moving=(1, 1, 1)):
    """(matrix, offset) in voxel indices of the rigid motion params = (r0, r1, r2, t0, t1, t2): the moving volume's content is turned by
    rotation_matrix((r0, r1, r2)) (degrees) about its centre (A - 1) / 2 and that centre is put t (millimetres) from the fixed volume's centre
    (O - 1) / 2.  In millimetres a fixed point x_f (from the fixed centre) reads the moving point R^T (x_f - t) (from the moving centre).  In this
    order: R = rotation_matrix(params[:3]); with equal isotropic spacing s, resample.rigid_matrix(R, c_m, c_f + t / s); otherwise (mr, offr) =
    resample.rigid_matrix(R, 0, s_f * c_f + t), matrix = (mr * s_f[None, :]) / s_m[:, None] and offset = offr / s_m + c_m.  Host only."""
    p = _vec(params, 'params', 6)
    of, om = _rs._check_shape(shape_fixed, 'shape_fixed'), _rs._check_shape(shape_moving, 'shape_moving')
    sf, sm = _vec(spacing_fixed, 'spacing_fixed', positive=True), _vec(spacing_moving, 'spacing_moving', positive=True)
    cf = (np.array(of, dtype=np.float64) - 1.0) / 2.0
    cm = (np.array(om, dtype=np.float64) - 1.0) / 2.0
    r = rotation_matrix(p[:3])
    t = p[3:]
    if (sf == sf[0]).all() and (sm == sf[0]).all():
        return _rs.rigid_matrix(r, cm, cf + t / sf[0])
    mr, offr = _rs.rigid_matrix(r, np.zeros(3), sf * cf + t)
    return (mr * sf[None, :]) / sm[:, None], offr / sm + cm


# ------------------------------------------------------------------------------------------------ scores and the search
def similarity_sweep(fixed, moving, poses, metric='nmi', **kw):
    """The score ('mi', 'nmi' or 'ecc') of every pose -> float64 [K]; kw as joint_histogram's.  One readback."""
    fn = _check_metric(metric)
    return fn(joint_histogram(fixed, moving, poses, **kw))


def _neighbours(p, step):
    """The 13 parameter vectors of one step: p, then parameter i plus and minus step[i] for i = 0 .. 5."""
    out = [p.copy()]
    for i in range(6):
        for sign in (1.0, -1.0):
            q = p.copy()
            q[i] = q[i] + sign * step[i]
            out.append(q)
    return out


def _best(scores):
    """The lowest index of the largest score, a NaN counting as -inf."""
    s = np.where(np.isnan(scores), -np.inf, scores)
    return int(np.argmax(s)), s


def register_rigid(fixed, moving, *, spacing_fixed, spacing_moving, start=None, steps_deg=(4.0, 2.0, 1.0, 0.5), steps_mm=(4.0, 2.0, 1.0, 0.5),
                   metric='nmi', max_moves=64, bins=32, fixed_range=(-200.0, 600.0), moving_range=None, mask=None, order=1, prefilter=True):
    """A deterministic pattern search for the rigid_pose parameters that maximise `metric`.  At level l the current parameters and their 12
    neighbours (each parameter plus, then minus, steps_deg[l] or steps_mm[l]) are scored in one 13-pose call; the search moves to the best
    neighbour if it is strictly better than the current pose (ties: the lowest index; a NaN score counts as -inf), goes to the next level when
    none is, and ends after the last level or after max_moves moves.  At order 3 the coefficients are made once.
    -> Registration(params [6], matrix, offset, score, history: one (level, params, score) per call, calls)."""
    fn = _check_metric(metric)
    sd, sm_ = np.asarray(steps_deg, dtype=np.float64), np.asarray(steps_mm, dtype=np.float64)
    if sd.ndim != 1 or sd.shape != sm_.shape or len(sd) < 1 or not (np.isfinite(sd).all() and np.isfinite(sm_).all() and (sd > 0).all() and (sm_ > 0).all()):
        raise ValueError('steps_deg, steps_mm: two equally long lists of positive numbers expected')
    if isinstance(max_moves, bool) or not isinstance(max_moves, (int, np.integer)) or max_moves < 0:
        raise ValueError('max_moves: a non-negative integer expected, got %r' % (max_moves,))
    p = np.zeros(6) if start is None else _vec(start, 'start', 6).copy()
    f, m, k, order = _prepare(fixed, moving, mask, order, prefilter)
    of, om = tuple(f.shape), tuple(m.shape)
    history, calls, moves, score = [], 0, 0, float('nan')
    for level in range(len(sd)):
        step = np.array([sd[level]] * 3 + [sm_[level]] * 3)
        while True:
            cands = _neighbours(p, step)
            poses = _check_poses([rigid_pose(q, of, om, spacing_fixed, spacing_moving) for q in cands])
            scores = fn(_histograms(f, m, k, poses, order, bins, fixed_range, moving_range))
            calls += 1
            score = float(scores[0])
            history.append((level, tuple(float(x) for x in p), score))
            b, s = _best(scores)
            if b == 0 or not s[b] > s[0] or moves >= max_moves:
                break
            p, score, moves = cands[b], float(scores[b]), moves + 1
        if moves >= max_moves:
            break
    matrix, offset = rigid_pose(p, of, om, spacing_fixed, spacing_moving)
    return Registration(p, matrix, offset, score, history, calls)


def align(fixed, moving, reg, output=None, order=3, mode='constant', cval=0.0, prefilter=True):
    """The moving volume on the fixed volume's lattice under `reg` (a Registration, or a (matrix, offset) pair): resample.affine_transform(moving,
    matrix, offset, output_shape=fixed.shape, ...).  Nothing is read back."""
    matrix, offset = (reg.matrix, reg.offset) if isinstance(reg, Registration) else reg
    shape = tuple(torch.as_tensor(fixed).shape) if not isinstance(fixed, torch.Tensor) else tuple(fixed.shape)
    return _rs.affine_transform(moving, np.asarray(matrix, dtype=np.float64), np.asarray(offset, dtype=np.float64), shape, output, order, mode,
                                cval, prefilter)
