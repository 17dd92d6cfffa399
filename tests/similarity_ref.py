"""Numpy restatement of hv_joint_hist (csrc/similarity.hip) and of the host side of healthivert-gan_amd/similarity.py (DESIGN.md section 8 row
f18).  No device.  The coordinates and the sampler are tests/resample_ref.py's coords_matrix() and sample() (pinned to scipy there), the levels
tests/texture_ref.py's levels_of(); this file adds the order of the tests per fixed voxel o and pose k --
  1 mask(o) == 0 -> info[k][2];  2 fixed(o) not finite -> info[k][3];  3 u = matrix @ o + offset;  4 u outside [0, A - 1] on any axis ->
  info[k][4];  5 y = sample(moving, u) not finite -> info[k][3];  6 out[k][level(x)][level(y)] += 1, info[k][1]
-- the entropies, the rigid pose and the pattern search, each restated line for line so that the device search must take the same path."""
import math

import numpy as np

import resample_ref as R
import texture_ref as T

INFO = 8
NONFINITE, EMPTY = 2, 4
MAX_POSES = 16


def _source(moving, order, coef):
    if order == 3:
        return R.spline_filter_scipy(moving) if coef is None else np.asarray(coef, dtype=np.float64)
    return np.asarray(moving)


def sampled(moving, out_shape, matrix, offset, order, coef=None):
    """-> (y [M] float64, inside [M]): the sampler's sums over the fixed lattice and which voxels' images lie inside the moving volume."""
    src = _source(moving, order, coef)
    u = R.coords_matrix(out_shape, matrix, offset)
    inside = np.ones(u.shape[1], dtype=bool)
    for h in range(3):
        inside &= (u[h] >= 0.0) & (u[h] <= src.shape[h] - 1)
    return R.sample(src, u, order, 'constant', 0.0), inside


def joint_hist_ref(fixed, moving, poses, order, flo, fwidth, Gf, mlo, mwidth, Gm, mask=None, coef=None):
    """-> (out [K][Gf][Gm] int64, info [K][INFO] int64) as the device writes them.  poses: (matrix, offset) pairs."""
    fixed = np.asarray(fixed)
    lf, ffin, flow, fhigh = T.levels_of(fixed.ravel(), flo, fwidth, Gf)
    keep = np.ones(fixed.size, dtype=bool) if mask is None else np.asarray(mask).ravel() != 0
    valid = keep & ffin
    out = np.zeros((len(poses), Gf, Gm), dtype=np.int64)
    info = np.zeros((len(poses), INFO), dtype=np.int64)
    for k, (m, off) in enumerate(poses):
        y, inside = sampled(moving, fixed.shape, m, off, order, coef)
        lm, yfin, mlow, mhigh = T.levels_of(y, mlo, mwidth, Gm)
        cnt = valid & inside & yfin
        np.add.at(out[k], (lf[cnt], lm[cnt]), 1)
        info[k, 1] = cnt.sum()
        info[k, 2] = (~keep).sum()
        info[k, 3] = (keep & ~ffin).sum() + (valid & inside & ~yfin).sum()
        info[k, 4] = (valid & ~inside).sum()
        info[k, 5], info[k, 6] = (cnt & flow).sum(), (cnt & fhigh).sum()
        info[k, 7] = (cnt & (mlow | mhigh)).sum()
        info[k, 0] = (NONFINITE if info[k, 3] else 0) | (0 if info[k, 1] else EMPTY)
    return out, info


def joint_hist_brute(fixed, moving, poses, order, flo, fwidth, Gf, mlo, mwidth, Gm, mask=None, coef=None):
    """The definition as three loops over the fixed voxels, one sample at a time (tiny cases only) -> out."""
    fixed = np.asarray(fixed)
    src = _source(moving, order, coef)
    out = np.zeros((len(poses), Gf, Gm), dtype=np.int64)

    def level(v, lo, width, G):
        t = (np.float64(v) - np.float64(lo)) / np.float64(width)
        return 0 if t < 0 else (G - 1 if t >= G else int(t))

    for k, (m, off) in enumerate(poses):
        m, off = np.asarray(m, dtype=np.float64), np.asarray(off, dtype=np.float64)
        for i in range(fixed.shape[0]):
            for j in range(fixed.shape[1]):
                for l in range(fixed.shape[2]):
                    if mask is not None and not mask[i, j, l]:
                        continue
                    x = np.float64(fixed[i, j, l])
                    if not np.isfinite(x):
                        continue
                    u = np.array([((0.0 + i * m[h, 0]) + j * m[h, 1]) + l * m[h, 2] + off[h] for h in range(3)])
                    if not all(0.0 <= u[h] <= src.shape[h] - 1 for h in range(3)):
                        continue
                    y = R.sample(src, u[:, None], order)[0]
                    if not np.isfinite(y):
                        continue
                    out[k, level(x, flo, fwidth, Gf), level(y, mlo, mwidth, Gm)] += 1
    return out


# ------------------------------------------------------------------------------------------------ the measures (similarity.py's, line for line)
def _plogp(p):
    return p * np.log(np.where(p > 0, p, 1.0))


def entropies(hist):
    P = np.asarray(hist)
    if P.ndim == 2:
        P = P[None]
    P = P.astype(np.float64)
    total = P.sum(axis=(1, 2))
    empty = total == 0
    p = P / np.where(empty, 1.0, total)[:, None, None]
    hf = -_plogp(p.sum(axis=2)).sum(axis=1)
    hm = -_plogp(p.sum(axis=1)).sum(axis=1)
    hfm = -_plogp(p).sum(axis=(1, 2))
    nan = np.where(empty, np.nan, 0.0)
    return hf + nan, hm + nan, hfm + nan


def mutual_information(hist):
    hf, hm, hfm = entropies(hist)
    return (hf + hm) - hfm


def normalized_mutual_information(hist):
    hf, hm, hfm = entropies(hist)
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(hfm > 0, (hf + hm) / np.where(hfm > 0, hfm, 1.0), np.nan)


def entropy_correlation(hist):
    hf, hm, hfm = entropies(hist)
    s = hf + hm
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(s > 0, 2.0 * (s - hfm) / np.where(s > 0, s, 1.0), np.nan)


METRIC = {'mi': mutual_information, 'nmi': normalized_mutual_information, 'ecc': entropy_correlation}


# ------------------------------------------------------------------------------------------------ rigid poses (similarity.py's, line for line)
def rigid_matrix(rotation, centre_in, centre_out):
    m = np.asarray(rotation, dtype=np.float64).T.copy()
    return m, np.asarray(centre_in, dtype=np.float64) - m @ np.asarray(centre_out, dtype=np.float64)


def rotation_matrix(angles_deg):
    a = np.asarray(angles_deg, dtype=np.float64)
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
    p = np.asarray(params, dtype=np.float64)
    sf, sm = np.asarray(spacing_fixed, dtype=np.float64), np.asarray(spacing_moving, dtype=np.float64)
    cf = (np.array(shape_fixed, dtype=np.float64) - 1.0) / 2.0
    cm = (np.array(shape_moving, dtype=np.float64) - 1.0) / 2.0
    r = rotation_matrix(p[:3])
    t = p[3:]
    if (sf == sf[0]).all() and (sm == sf[0]).all():
        return rigid_matrix(r, cm, cf + t / sf[0])
    mr, offr = rigid_matrix(r, np.zeros(3), sf * cf + t)
    return (mr * sf[None, :]) / sm[:, None], offr / sm + cm


# ------------------------------------------------------------------------------------------------ the search (similarity.py's, line for line)
def _neighbours(p, step):
    out = [p.copy()]
    for i in range(6):
        for sign in (1.0, -1.0):
            q = p.copy()
            q[i] = q[i] + sign * step[i]
            out.append(q)
    return out


def _best(scores):
    s = np.where(np.isnan(scores), -np.inf, scores)
    return int(np.argmax(s)), s


def register_rigid(fixed, moving, spacing_fixed, spacing_moving, start=None, steps_deg=(4.0, 2.0, 1.0, 0.5), steps_mm=(4.0, 2.0, 1.0, 0.5),
                   metric='nmi', max_moves=64, bins=32, fixed_range=(-200.0, 600.0), moving_range=None, mask=None, order=1, coef=None):
    """-> (params, matrix, offset, score, history, calls)"""
    fn = METRIC[metric]
    Gf, Gm = (bins, bins) if isinstance(bins, int) else bins
    flo, fwidth = float(fixed_range[0]), (float(fixed_range[1]) - float(fixed_range[0])) / Gf
    mr = fixed_range if moving_range is None else moving_range
    mlo, mwidth = float(mr[0]), (float(mr[1]) - float(mr[0])) / Gm
    sd, sm_ = np.asarray(steps_deg, dtype=np.float64), np.asarray(steps_mm, dtype=np.float64)
    p = np.zeros(6) if start is None else np.asarray(start, dtype=np.float64).copy()
    fixed, moving = np.asarray(fixed), np.asarray(moving)
    if order == 3 and coef is None:
        coef = R.spline_filter_scipy(moving)
    of, om = fixed.shape, moving.shape
    history, calls, moves, score = [], 0, 0, float('nan')
    for level in range(len(sd)):
        step = np.array([sd[level]] * 3 + [sm_[level]] * 3)
        while True:
            cands = _neighbours(p, step)
            poses = [rigid_pose(q, of, om, spacing_fixed, spacing_moving) for q in cands]
            scores = fn(joint_hist_ref(fixed, moving, poses, order, flo, fwidth, Gf, mlo, mwidth, Gm, mask, coef)[0])
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
    return p, matrix, offset, score, history, calls


# ------------------------------------------------------------------------------------------------ shared cases
REG_SHAPE = (24, 28, 20)
REG_SPACING = (1.0, 1.0, 1.5)
REG_TRUE = (3.0, -2.0, 1.5, 1.5, -1.0, 2.0)                           # degrees, millimetres
REG_KW = dict(bins=16, order=1, steps_deg=(2.0, 1.0, 0.5), steps_mm=(2.0, 1.0, 0.5))
_REG_CACHE = {}


def registration_case():
    """-> (fixed, moving) float32: a smooth blob with a ramp plus seeded noise, and the same content under the rigid motion REG_TRUE, so that
    fixed(o) is about moving(matrix @ o + offset) for rigid_pose(REG_TRUE, ...): moving(x) = fixed(matrix^-1 (x - offset)), order 1."""
    if 'pair' not in _REG_CACHE:
        g = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in REG_SHAPE], indexing='ij')
        c = [(n - 1) / 2.0 for n in REG_SHAPE]
        r2 = ((g[0] - c[0] - 2.0) / 7.0) ** 2 + ((g[1] - c[1] + 1.0) / 9.0) ** 2 + ((g[2] - c[2]) / 5.0) ** 2
        base = 500.0 * np.exp(-r2) + 6.0 * g[1] - 4.0 * g[2] + 150.0 * np.exp(-(((g[0] - 5.0) / 3.0) ** 2 + ((g[1] - 20.0) / 4.0) ** 2 + ((g[2] - 6.0) / 3.0) ** 2))
        fixed = (base + np.random.RandomState(7).standard_normal(REG_SHAPE) * 12.0).astype(np.float32)
        m, off = rigid_pose(REG_TRUE, REG_SHAPE, REG_SHAPE, REG_SPACING, REG_SPACING)
        inv = np.linalg.inv(m)
        moving = R.affine_transform(fixed, inv, -inv @ off, order=1, output=np.float32)
        moving = (moving + np.random.RandomState(8).standard_normal(REG_SHAPE).astype(np.float32) * np.float32(6.0)).astype(np.float32)
        _REG_CACHE['pair'] = (fixed, moving)
    return _REG_CACHE['pair']


def registration_ref():
    """The restatement's search on registration_case(), computed once."""
    if 'reg' not in _REG_CACHE:
        fixed, moving = registration_case()
        _REG_CACHE['reg'] = register_rigid(fixed, moving, REG_SPACING, REG_SPACING, **REG_KW)
    return _REG_CACHE['reg']


def corner_error(shape, pose, true_pose):
    """The mean distance, over the fixed volume's eight corners, between where two poses send them (moving voxels)."""
    cs = np.array([[a, b, c] for a in (0, shape[0] - 1) for b in (0, shape[1] - 1) for c in (0, shape[2] - 1)], dtype=np.float64)
    pa = cs @ np.asarray(pose[0]).T + pose[1]
    pb = cs @ np.asarray(true_pose[0]).T + true_pose[1]
    return float(np.sqrt(((pa - pb) ** 2).sum(axis=1)).mean())
