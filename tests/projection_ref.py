"""Numpy float64 restatement of hv_project (csrc/projection.hip) and of the host side of healthivert-gan_amd/projection.py (DESIGN.md section 8
row f20).  No device.  The coordinates and the sampler are tests/resample_ref.py's coords_matrix() and sample() (pinned to scipy there) on the
lattice (p0, p1, t); this file adds the order of the tests per sample --
  1 u = matrix @ (p0, p1, t) + offset;  2 u outside [0, A - 1] on any axis -> info[k][2];  3 label(floor(u + 0.5)) != label_value -> info[k][3];
  4 y = sample(vol, u) not finite -> info[k][4];  5 counted, info[k][1]
-- and the reduction along t over the counted samples: the sum in chunks of CHUNK consecutive t, each chunk summed sequentially from +0.0 in
increasing t, the chunk sums added sequentially from +0.0 in increasing chunk order (every chunk, the empty ones too); min and max by value,
stored as m + 0.0; count, first, last.  A sample that is not counted adds nothing; adding +0.0 in its place gives the same bits, because a
sum that starts at +0.0 is never -0.0, and that is how the vectorised form below skips it (project_brute skips it literally)."""
import math

import numpy as np

import resample_ref as R
import similarity_ref as SIM

CHUNK = 16
INFO = 8
MAX_POSES = 16
NONFINITE, EMPTY = 2, 4
STATUS, COUNTED, OUTSIDE, REJECTED, NOT_FINITE = range(5)
VIEWS = {'lateral': (0, 1, 2), 'ap': (0, 2, 1), 'axial': (1, 2, 0)}   # detector axis 0, detector axis 1, the ray's array axis


def _source(vol, order, coef):
    if order == 3:
        return R.spline_filter_scipy(vol) if coef is None else np.asarray(coef, dtype=np.float64)
    return np.asarray(vol)


def samples(vol, pose, det_shape, steps, order, label=None, label_value=None, coef=None):
    """-> (y [P0][P1][T] float64, state [P0][P1][T] int: 1 counted, 2 outside, 3 rejected by the label, 4 not finite)."""
    src = _source(vol, order, coef)
    P0, P1 = det_shape
    u = R.coords_matrix((P0, P1, steps), pose[0], pose[1])
    inside = np.ones(u.shape[1], dtype=bool)
    for h in range(3):
        inside &= (u[h] >= 0.0) & (u[h] <= src.shape[h] - 1)
    state = np.where(inside, 1, 2)
    if label is not None:
        lab = np.asarray(label)
        q = [np.floor(u[h][inside] + 0.5).astype(np.int64) for h in range(3)]
        rej = lab[q[0], q[1], q[2]].astype(np.float64) != np.float64(label_value)
        state[np.flatnonzero(inside)[rej]] = 3
    y = R.sample(src, u, order, 'constant', 0.0)
    state[(state == 1) & ~np.isfinite(y)] = 4
    return y.reshape(P0, P1, steps), state.reshape(P0, P1, steps)


def reduce_rays(y, state):
    """-> (acc [3][P0][P1] float64, idx [3][P0][P1] int32, info [INFO] int64) of one pose."""
    P0, P1, T = y.shape
    cnt = state == 1
    nch = -(-T // CHUNK)
    yz = np.zeros((P0, P1, nch * CHUNK))
    yz[:, :, :T] = np.where(cnt, y, 0.0)
    yz = yz.reshape(P0, P1, nch, CHUNK)
    with np.errstate(invalid='ignore', over='ignore'):
        cs = np.zeros((P0, P1, nch))
        for i in range(CHUNK):
            cs = cs + yz[..., i]
        run = np.zeros((P0, P1))
        for c in range(nch):
            run = run + cs[..., c]
    mn = np.where(cnt, y, np.inf).min(axis=2) + 0.0
    mx = np.where(cnt, y, -np.inf).max(axis=2) + 0.0
    t = np.arange(T)
    count = cnt.sum(axis=2)
    first = np.where(cnt, t, T).min(axis=2)
    last = np.where(cnt, t, -1).max(axis=2)
    info = np.zeros(INFO, dtype=np.int64)
    for w in (1, 2, 3, 4):
        info[w] = (state == w).sum()
    info[0] = (NONFINITE if info[4] else 0) | (0 if info[1] else EMPTY)
    return np.stack([run, mn, mx]), np.stack([count, first, last]).astype(np.int32), info


def project_ref(vol, poses, det_shape, steps, order, label=None, label_value=None, coef=None):
    """-> (acc [K][3][P0][P1] float64, idx [K][3][P0][P1] int32, info [K][INFO] int64) as the device writes them.  poses: (matrix, offset)."""
    src = _source(vol, order, coef)
    out = [reduce_rays(*samples(vol, p, det_shape, steps, order, label, label_value, src if order == 3 else None)) for p in poses]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.stack([o[2] for o in out])


def project_brute(vol, poses, det_shape, steps, order, label=None, label_value=None, coef=None):
    """The definition as plain loops, one sample at a time (tiny cases only)."""
    src = _source(vol, order, coef)
    P0, P1 = det_shape
    K = len(poses)
    acc = np.zeros((K, 3, P0, P1))
    idx = np.zeros((K, 3, P0, P1), dtype=np.int32)
    info = np.zeros((K, INFO), dtype=np.int64)
    for k, (m, off) in enumerate(poses):
        m, off = np.asarray(m, dtype=np.float64).reshape(3, 3), np.asarray(off, dtype=np.float64)
        for p0 in range(P0):
            for p1 in range(P1):
                run, mn, mx, count, first, last = np.float64(0.0), np.inf, -np.inf, 0, steps, -1
                for c0 in range(0, steps, CHUNK):
                    cs = np.float64(0.0)
                    for t in range(c0, min(c0 + CHUNK, steps)):
                        u = np.array([(((0.0 + p0 * m[h, 0]) + p1 * m[h, 1]) + t * m[h, 2]) + off[h] for h in range(3)])
                        if not all(0.0 <= u[h] <= src.shape[h] - 1 for h in range(3)):
                            info[k, 2] += 1
                            continue
                        if label is not None:
                            q = [int(math.floor(u[h] + 0.5)) for h in range(3)]
                            if np.float64(label[q[0], q[1], q[2]]) != np.float64(label_value):
                                info[k, 3] += 1
                                continue
                        y = R.sample(src, u[:, None], order)[0]
                        if not np.isfinite(y):
                            info[k, 4] += 1
                            continue
                        info[k, 1] += 1
                        cs = cs + y
                        mn, mx = (y if y < mn else mn), (y if y > mx else mx)
                        count, first, last = count + 1, min(first, t), t
                    run = run + cs
                acc[k, :, p0, p1] = run, mn + 0.0, mx + 0.0
                idx[k, :, p0, p1] = count, first, last
        info[k, 0] = (NONFINITE if info[k, 4] else 0) | (0 if info[k, 1] else EMPTY)
    return acc, idx, info


# ------------------------------------------------------------------------------------------------ the host formulas (projection.py's, line for line)
def view_frame(view):
    """-> the 3 x 3 matrix whose columns are the detector's two axes and the ray's direction, unit vectors in millimetre space."""
    if isinstance(view, str):
        a0, a1, ar = VIEWS[view]
        f = np.zeros((3, 3))
        f[a0, 0], f[a1, 1], f[ar, 2] = 1.0, 1.0, 1.0
        return f
    return SIM.rotation_matrix(view)


def view_pose(shape, spacing, view, det_spacing=None, step_mm=None, det_shape=None, steps=None):
    """-> (matrix, offset, det_shape, steps, det_spacing, step_mm)"""
    n = np.array(shape, dtype=np.float64)
    sp = np.asarray(spacing, dtype=np.float64)
    f = view_frame(view)
    ds = np.array([sp.min(), sp.min()]) if det_spacing is None else np.asarray(det_spacing, dtype=np.float64) * np.ones(2)
    st = float(sp.min()) if step_mm is None else float(step_mm)
    diameter = float(np.sqrt((((n - 1.0) * sp) ** 2).sum()))
    if det_shape is None:
        det_shape = (int(math.ceil(diameter / ds[0])) + 1, int(math.ceil(diameter / ds[1])) + 1)
    if steps is None:
        steps = int(math.ceil(diameter / st)) + 1
    pitch = np.array([ds[0], ds[1], st])
    matrix = (f * pitch[None, :]) / sp[:, None]
    centre = (n - 1.0) / 2.0
    mid = (np.array([det_shape[0], det_shape[1], steps], dtype=np.float64) - 1.0) / 2.0
    offset = centre - matrix @ mid
    return matrix, offset, (int(det_shape[0]), int(det_shape[1])), int(steps), ds, st


def radiograph(acc, step_mm):
    return acc[..., 0, :, :] * step_mm


def thickness_map(idx, step_mm):
    return idx[..., 0, :, :].astype(np.float64) * step_mm


def areal_density(acc, idx, det_spacing, step_mm):
    """One pose's acc [3][P0][P1] and idx -> (area, integral, areal density, mean path), float64."""
    pixel = float(det_spacing[0]) * float(det_spacing[1])
    hit = idx[0] > 0
    area = float(hit.sum()) * pixel
    integral = float(acc[0][hit].sum()) * step_mm * pixel
    path = float(idx[0][hit].astype(np.float64).sum()) * step_mm
    nan = float('nan')
    return {'area': area, 'integral': integral, 'areal_density': integral / area if area > 0 else nan,
            'mean_path': path / float(hit.sum()) if hit.any() else nan, 'pixels': int(hit.sum()), 'samples': int(idx[0].sum())}


def ball(shape, spacing, radius_mm, value, dtype=np.float64):
    """A ball of `value` about the volume's centre (voxel centres within radius_mm), 0 elsewhere."""
    g = np.meshgrid(*[(np.arange(n) - (n - 1) / 2.0) * s for n, s in zip(shape, spacing)], indexing='ij')
    return np.where(g[0] ** 2 + g[1] ** 2 + g[2] ** 2 <= radius_mm ** 2, value, 0).astype(dtype)


def phantom():
    """tests/test_shape_gpu.py's two vertebra-like bodies in (24, 28, 20) -- 21 a box with a wedge cut away and a stray fragment, 22 an
    ellipsoid -- with a CT over them and the synthesized pair (the wedge filled) -> (ct, label, ct_synth, label_synth)."""
    shape = (24, 28, 20)
    g = np.indices(shape)
    lab = np.zeros(shape, dtype=np.uint8)
    lab[3:11, 4:24, 3:17] = 21
    lab[(g[0] < 3 + (g[1] - 4) * 0.2) & (lab == 21)] = 0
    lab[1, 1, 1:3] = 21
    lab[((g[0] - 17.0) / 4.5) ** 2 + ((g[1] - 14.0) / 10.0) ** 2 + ((g[2] - 10.0) / 7.0) ** 2 <= 1.0] = 22
    synth = lab.copy()
    synth[3:11, 4:24, 3:17] = 21
    synth[1, 1, 1:3] = 0
    rng = np.random.RandomState(5)
    noise = rng.randint(-40, 41, shape)
    ct = (np.where(lab > 0, 300, -50) + 8 * g[1] + noise).astype(np.int16)
    ct_s = (np.where(synth > 0, 320, -50) + 8 * g[1] + noise).astype(np.int16)
    return ct, lab, ct_s, synth
