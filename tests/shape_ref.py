"""numpy restatement of hv_shape (csrc/shape.hip) and of the host half of healthivert-gan_amd/shape.py, written
without looking at either: the record by padding, eight shifted slices and np.bincount, moments and extents by plain numpy on the voxel
coordinates, the Minkowski measures from tables built here corner by corner.  tests/test_shape_ref_cpu.py pins it (a triple loop, shapes of
known topology, Ohser and Muecklich's weights, spheres, np.cov); the GPU tests compare the device's records with it byte for byte."""
import math

import numpy as np

from labelstats_ref import BAD_LABEL, EMPTY
from texture_ref import directions13, slots_of

REC, COUNT, SUM, SUM2, EXTENT, STATUS = 320, 256, 257, 260, 266, 292
I64_MAX, I64_MIN = np.iinfo(np.int64).max, np.iinfo(np.int64).min
DIRS = directions13()
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
CORNERS = [(d0, d1, d2) for d0 in (0, 1) for d1 in (0, 1) for d2 in (0, 1)]        # corner q = 4 d0 + 2 d1 + d2


def histogram_ref(x):
    """The configuration histogram [256] of one boolean volume: the cells -1 .. A - 1 per axis of the volume padded by one background layer."""
    x = np.asarray(x, dtype=bool)
    p = np.pad(x, 1, constant_values=False)
    n = tuple(a + 1 for a in x.shape)
    code = np.zeros(n, dtype=np.int64)
    for q, (d0, d1, d2) in enumerate(CORNERS):
        code += p[d0:d0 + n[0], d1:d1 + n[1], d2:d2 + n[2]].astype(np.int64) << q
    return np.bincount(code.ravel(), minlength=256).astype(np.int64)


def histogram_brute(x):
    """The definition as three loops over the cells (tiny cases only)."""
    x = np.asarray(x, dtype=bool)
    A = x.shape
    h = np.zeros(256, dtype=np.int64)
    for i in range(-1, A[0]):
        for j in range(-1, A[1]):
            for k in range(-1, A[2]):
                code = 0
                for q, d in enumerate(CORNERS):
                    c = (i + d[0], j + d[1], k + d[2])
                    if all(0 <= u < a for u, a in zip(c, A)) and x[c]:
                        code |= 1 << q
                h[code] += 1
    return h


def record_ref(label, labels, mask=None):
    """One 3-D label volume -> int64 [S][REC] as the device writes it."""
    slot, bad = slots_of(label, labels, mask)
    out = np.zeros((len(labels), REC), dtype=np.int64)
    for s in range(len(labels)):
        mine = slot == s
        out[s, :256] = histogram_ref(mine)
        p = np.argwhere(mine).astype(np.int64)
        out[s, COUNT] = len(p)
        out[s, EXTENT:STATUS:2], out[s, EXTENT + 1:STATUS:2] = I64_MAX, I64_MIN
        if len(p):
            out[s, SUM:SUM + 3] = p.sum(axis=0)
            for n, (a, b) in enumerate(PAIRS):
                out[s, SUM2 + n] = (p[:, a] * p[:, b]).sum()
            for t, d in enumerate(DIRS):
                dot = p @ np.asarray(d, dtype=np.int64)
                out[s, EXTENT + 2 * t], out[s, EXTENT + 2 * t + 1] = dot.min(), dot.max()
        out[s, STATUS] = (BAD_LABEL if bad else 0) | (0 if len(p) else EMPTY)
    return out


# ------------------------------------------------------------------------------------------------ the host formulas
def _tables():
    edges = [(p, q) for p in range(8) for q in range(p + 1, 8) if bin(p ^ q).count('1') == 1]
    faces = [[q for q in range(8) if (q >> ax) & 1 == side] for ax in range(3) for side in (0, 1)]
    assert len(edges) == 12 and len(faces) == 6
    e6, e26, v = (np.zeros(256, dtype=np.int64) for _ in range(3))
    t = np.zeros((13, 256), dtype=np.int64)
    for c in range(256):
        on = [(c >> q) & 1 for q in range(8)]
        v[c] = sum(on)
        e_all, e_any = sum(on[p] & on[q] for p, q in edges), sum(on[p] | on[q] for p, q in edges)
        f_all, f_any = sum(all(on[q] for q in f) for f in faces), sum(any(on[q] for q in f) for f in faces)
        e6[c] = v[c] - 2 * e_all + 4 * f_all - 8 * (c == 255)                       # eight times the cell's share
        e26[c] = 8 * (c != 0) - 4 * f_any + 2 * e_any - v[c]
        for n, d in enumerate(DIRS):
            for q, p in enumerate(CORNERS):
                r = tuple(a + b for a, b in zip(p, d))
                if all(u in (0, 1) for u in r):
                    t[n, c] += (1 - on[q]) & on[4 * r[0] + 2 * r[1] + r[2]]
    return v, e6, e26, t


_V, _E6, _E26, _T = _tables()
_Z = np.asarray([sum(1 for c in d if c == 0) for d in DIRS])


def fibonacci_points(N=200000):
    i = np.arange(N, dtype=np.float64) + 0.5
    z = 1.0 - 2.0 * i / N
    phi = i * (math.pi * (3.0 - math.sqrt(5.0)))
    r = np.sqrt(1.0 - z * z)
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)


def direction_weights_ref(spacing=(1, 1, 1), N=200000):
    """The share of the sphere nearest to +-(d o s) / |d o s| for each of the 13 directions, by the fixed Fibonacci quadrature."""
    u = np.asarray(DIRS, dtype=np.float64) * np.asarray(spacing, dtype=np.float64)
    u /= np.sqrt((u * u).sum(axis=1))[:, None]
    near = np.abs(fibonacci_points(N) @ u.T).argmax(axis=1)
    return np.bincount(near, minlength=13) / float(N)


def minkowski_ref(hist, spacing=(1, 1, 1)):
    h = np.asarray(hist, dtype=np.int64)
    s = np.asarray(spacing, dtype=np.float64)
    out = {'count': (h * _V).sum(axis=-1) // 8, 'euler_6': (h * _E6).sum(axis=-1) // 8, 'euler_26': (h * _E26).sum(axis=-1) // 8}
    assert ((h * _V).sum(axis=-1) % 8 == 0).all() and ((h * _E6).sum(axis=-1) % 8 == 0).all() and ((h * _E26).sum(axis=-1) % 8 == 0).all()
    N = np.stack([(h * _T[n]).sum(axis=-1) // (1 << _Z[n]) for n in range(13)], axis=-1)
    out['intercepts'] = N.astype(np.float64)
    ax = [DIRS.index((1, 0, 0)), DIRS.index((0, 1, 0)), DIRS.index((0, 0, 1))]
    out['face_area'] = 2.0 * (N[..., ax[0]] * (s[1] * s[2]) + N[..., ax[1]] * (s[0] * s[2]) + N[..., ax[2]] * (s[0] * s[1]))
    w = direction_weights_ref(spacing)
    length = np.sqrt(((np.asarray(DIRS, dtype=np.float64) * s) ** 2).sum(axis=1))
    out['surface_area'] = 4.0 * (out['intercepts'] * (w * float(np.prod(s)) / length)).sum(axis=-1)
    return out


def descriptors_ref(rec, spacing=(1, 1, 1)):
    """One record [REC] -> the dict of shape.shape_descriptors for that label."""
    rec = np.asarray(rec, dtype=np.int64)
    s = np.asarray(spacing, dtype=np.float64)
    mk = minkowski_ref(rec[:256], spacing)
    n = int(rec[COUNT])
    nan = float('nan')
    out = {'count': n, 'status': int(rec[STATUS]), 'euler_6': int(mk['euler_6']), 'euler_26': int(mk['euler_26']),
           'surface_area': float(mk['surface_area']), 'face_area': float(mk['face_area']), 'intercepts': mk['intercepts']}
    assert int(mk['count']) == n
    if n == 0:
        for k in ('voxel_volume', 'surface_area', 'face_area', 'sphericity', 'surface_volume_ratio', 'major_axis_length', 'minor_axis_length',
                  'least_axis_length', 'elongation', 'flatness', 'max_caliper_width', 'min_caliper_width'):
            out[k] = nan
        out.update(centroid=np.full(3, nan), covariance=np.full((3, 3), nan), principal_moments=np.full(3, nan),
                   principal_axes=np.full((3, 3), nan), caliper_widths=np.full(13, nan))
        return out
    vol = n * float(np.prod(s))
    area = out['surface_area']
    out['voxel_volume'] = vol
    out['sphericity'] = (36.0 * math.pi * vol * vol) ** (1.0 / 3.0) / area if area > 0 else nan
    out['surface_volume_ratio'] = area / vol if area > 0 else nan
    sums = [int(x) for x in rec[SUM:SUM + 3]]
    out['centroid'] = np.asarray([sums[a] / n for a in range(3)]) * s
    cov = np.zeros((3, 3))
    for m, (a, b) in enumerate(PAIRS):
        cov[a, b] = cov[b, a] = (n * int(rec[SUM2 + m]) - sums[a] * sums[b]) / (n * n) * (s[a] * s[b])
    out['covariance'] = cov
    lam, vec = np.linalg.eigh(cov)
    lam, vec = np.maximum(lam[::-1], 0.0), vec[:, ::-1]
    out['principal_moments'], out['principal_axes'] = lam, vec.T
    out['major_axis_length'], out['minor_axis_length'], out['least_axis_length'] = (4.0 * math.sqrt(x) for x in lam)
    out['elongation'] = math.sqrt(lam[1] / lam[0]) if lam[0] > 0 else nan
    out['flatness'] = math.sqrt(lam[2] / lam[0]) if lam[0] > 0 else nan
    ext = rec[EXTENT:STATUS].reshape(13, 2)
    norm = np.sqrt(((np.asarray(DIRS, dtype=np.float64) / s) ** 2).sum(axis=1))
    out['caliper_widths'] = (ext[:, 1] - ext[:, 0]).astype(np.float64) / norm
    out['max_caliper_width'], out['min_caliper_width'] = float(out['caliper_widths'].max()), float(out['caliper_widths'].min())
    return out


# ------------------------------------------------------------------------------------------------ shapes of known topology
def ball(r, size=None):
    n = size or 2 * int(math.ceil(r)) + 3
    g = np.indices((n,) * 3) - (n - 1) / 2.0
    return (g ** 2).sum(axis=0) <= r * r


def hollow_ball(r_out, r_in):
    n = 2 * int(math.ceil(r_out)) + 3
    return ball(r_out, n) & ~ball(r_in, n)


def torus(R, r):
    n = 2 * int(math.ceil(R + r)) + 3
    g = np.indices((n,) * 3) - (n - 1) / 2.0
    return (np.sqrt(g[0] ** 2 + g[1] ** 2) - R) ** 2 + g[2] ** 2 <= r * r


def ellipsoid_mm(radius_mm, spacing):
    """A physical sphere of radius_mm sampled at `spacing`."""
    n = [2 * int(math.ceil(radius_mm / s)) + 3 for s in spacing]
    g = np.meshgrid(*[(np.arange(m) - (m - 1) / 2.0) * s for m, s in zip(n, spacing)], indexing='ij')
    return g[0] ** 2 + g[1] ** 2 + g[2] ** 2 <= radius_mm * radius_mm
