"""Numpy float64 restatement of the exact Euclidean distance transform and of the surface-distance metrics (csrc/edt.hip, hv_edt and
hv_surface_distance), with the cases the CPU and GPU tests share.

The transform is scipy.ndimage.distance_transform_edt; the metrics are MedPy's metric.binary hd / hd95 / asd / assd restated (MedPy is not
installed: the restatement is unpinned against it).  tests/test_surface_ref_cpu.py pins what can be pinned: the transform against scipy, the
surface rule against scipy's erosion, the percentile against numpy, the metrics against numbers worked out by hand.

edt(): brute force per axis, in the order 0, 1, 2 -- every voxel of a line against every other, no envelope, no early exit -- on squared
distances: int64 at unit spacing, else float64 with the sum formed as ((s0 d0)^2 + (s1 d1)^2) + (s2 d2)^2.  Rounding is monotonic, so the
minimum over a line of fl(g + c) is fl(min g + c) and the result is, bit for bit, the minimum over ALL target voxels of that sum
(edt_allpairs(), which the CPU test holds against it).
"""
import math

import numpy as np

# The largest relative difference |edt - scipy| / scipy over the anisotropic cases below, as tests/test_surface_ref_cpu.py measures it (scipy sums the
# three squares in its own order, so equal-length ties and the last bit may differ -- on these cases they do not: the measured value is 0);
# EDT_TOL is 10 x that, with a floor of 1e-12: the floor.
MEASURED_REL = 0.0
EDT_TOL = max(10.0 * MEASURED_REL, 1e-12)

SPACINGS = ((1.0, 1.0, 1.0), (0.7, 0.7, 1.5), (2.5, 0.9, 0.9))
# the widths of csrc/edt.hip: columns per tile of the axis-1 pass, lines per workgroup of the axis-2 pass, lanes per workgroup (lines of the axis-0 pass)
ED_KT, ED_LINES, ED_THREADS = 32, 32, 256
_BIG = np.int64(1) << 62


def is_unit(spacing):
    return tuple(float(s) for s in spacing) == (1.0, 1.0, 1.0)


def _axis_min(g, axis, s, unit):
    """out(i) = min_j g(j) + (s (i - j))^2 along `axis`, every pair."""
    n = g.shape[axis]
    g = np.moveaxis(g, axis, -1)
    d = np.arange(n)[:, None] - np.arange(n)[None, :]
    if unit:
        q = (d * d).astype(np.int64)
    else:
        t = np.float64(s) * d.astype(np.float64)
        q = t * t
    out = (g[..., None, :] + q).min(-1)
    return np.moveaxis(out, -1, axis)


def edt(target, spacing=(1.0, 1.0, 1.0)):
    """Distance of every voxel to the nearest True voxel of `target` (3-D bool), axes scaled by `spacing`; +inf everywhere if there is none."""
    target = np.asarray(target, dtype=bool)
    unit = is_unit(spacing)
    if unit:
        g = np.where(target, np.int64(0), _BIG)
    else:
        g = np.where(target, 0.0, np.inf)
    for axis in range(3):
        g = _axis_min(g, axis, spacing[axis], unit)
    if unit:
        out = np.sqrt(np.where(g >= _BIG, 0, g).astype(np.float64))
        out[g >= _BIG] = np.inf
        return out
    return np.sqrt(g)


def edt_allpairs(target, spacing=(1.0, 1.0, 1.0)):
    """The same by the definition: every voxel against every target voxel."""
    target = np.asarray(target, dtype=bool)
    idx = np.argwhere(target)
    out = np.full(target.shape, np.inf)
    if not len(idx):
        return out
    p = np.argwhere(np.ones(target.shape, dtype=bool))
    unit = is_unit(spacing)
    best = None
    for lo in range(0, len(idx), 256):
        d = p[:, None, :] - idx[None, lo:lo + 256, :]
        if unit:
            q = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        else:
            t = d.astype(np.float64) * np.asarray(spacing, dtype=np.float64)
            q = (t[..., 0] * t[..., 0] + t[..., 1] * t[..., 1]) + t[..., 2] * t[..., 2]
        q = q.min(1)
        best = q if best is None else np.minimum(best, q)
    return np.sqrt(best.astype(np.float64)).reshape(target.shape)


def surface(X):
    """The voxels of X with a face neighbour outside X; outside the volume counts as outside X."""
    X = np.asarray(X, dtype=bool)
    P = np.pad(X, 1, constant_values=False)
    inner = (P[:-2, 1:-1, 1:-1] & P[2:, 1:-1, 1:-1] & P[1:-1, :-2, 1:-1] & P[1:-1, 2:, 1:-1] & P[1:-1, 1:-1, :-2] & P[1:-1, 1:-1, 2:])
    return X & ~inner


def percentile95(x):
    """np.percentile(x, 95) (method 'linear') restated: v = (n - 1) 0.95, lo / hi the order statistics floor(v) and floor(v) + 1, t the fraction."""
    x = np.sort(np.asarray(x, dtype=np.float64))
    n = len(x)
    v = np.float64(n - 1) * np.float64(0.95)
    k = int(np.floor(v))
    t = v - np.float64(k)
    lo, hi = x[k], x[min(k + 1, n - 1)]
    d = hi - lo
    return lo + d * t if t < 0.5 else hi - d * (np.float64(1.0) - t)


def metrics(a, b, value=1, spacing=(1.0, 1.0, 1.0)):
    """-> dict(n_a, n_b, max_ab, max_ba, asd_ab, asd_ba, hd, hd95, assd) of A = (a == value), B = (b == value), or None if a surface is empty."""
    SA, SB = surface(np.asarray(a) == value), surface(np.asarray(b) == value)
    if not SA.any() or not SB.any():
        return None
    ab, ba = edt(SB, spacing)[SA], edt(SA, spacing)[SB]
    res = {'n_a': int(SA.sum()), 'n_b': int(SB.sum()), 'max_ab': float(ab.max()), 'max_ba': float(ba.max()),
           'asd_ab': float(ab.mean()), 'asd_ba': float(ba.mean())}
    res['hd'] = max(res['max_ab'], res['max_ba'])
    res['hd95'] = float(percentile95(np.concatenate([ab, ba])))
    res['assd'] = (res['asd_ab'] + res['asd_ba']) / 2.0
    return res


# ------------------------------------------------------------------------------------------------ shared cases
def edt_shapes():
    """Each axis in turn at 1, 2 and around ED_KT / ED_LINES (31, 32, 33), the other axes small and odd; line counts of the axis-2 pass around
    ED_LINES; line counts of the axis-0 pass around ED_THREADS (255, 256, 257), among them one line of 257 along the unit-stride axis."""
    shapes = []
    for size in (1, 2, ED_KT - 1, ED_KT, ED_KT + 1):
        shapes += [(size, 5, 7), (5, size, 7), (7, 5, size)]
    shapes += [(ED_LINES - 1, 1, 3), (ED_LINES, 1, 3), (ED_LINES + 1, 1, 3), (4, 8, 5)]
    shapes += [(3, 1, ED_THREADS - 1), (3, 1, ED_THREADS), (2, 1, ED_THREADS + 1), (2, 8, 32), (6, 8, 33), (1, 1, 1)]
    return shapes


TARGET_SETS = ('corners', 'all', 'none', 'checker', 'planes', 'random')


def target_set(shape, kind, seed=0):
    """A bool volume: the voxels the distances are taken to."""
    T = np.zeros(shape, dtype=bool)
    if kind == 'corners':
        T[::max(1, shape[0] - 1), ::max(1, shape[1] - 1), ::max(1, shape[2] - 1)] = True
    elif kind == 'all':
        T[:] = True
    elif kind == 'checker':
        i, j, k = np.meshgrid(*(np.arange(s) for s in shape), indexing='ij')
        T = (i + j + k) % 2 == 0
    elif kind == 'planes':                         # two parallel planes across the longest axis: the voxels half way between them tie
        ax = int(np.argmax(shape))
        sl = [slice(None)] * 3
        for pos in (shape[ax] // 4, (3 * shape[ax]) // 4):
            sl[ax] = pos
            T[tuple(sl)] = True
    elif kind == 'random':
        T = np.random.RandomState(1000 + seed).rand(*shape) < 0.02
    elif kind != 'none':
        raise ValueError(kind)
    return T


def blob(shape, centre, radii):
    """An ellipsoid mask."""
    g = np.meshgrid(*(np.arange(s, dtype=np.float64) for s in shape), indexing='ij')
    return sum(((x - c) / r) ** 2 for x, c, r in zip(g, centre, radii)) <= 1.0


def analytic_cases():
    """(name, a, b, expected) with the expected numbers worked out by hand (unit spacing, label 1)."""
    cases = []
    m = np.zeros((7, 6, 5), dtype=np.uint8)
    m[2:5, 1:4, 1:4] = 1
    # identical masks: every distance is 0
    cases.append(('identical', m, m.copy(), dict(hd=0.0, hd95=0.0, assd=0.0)))
    # two single voxels 3, 4 and 12 apart along the axes: both are their own surface, both lists hold 13 = sqrt(9 + 16 + 144)
    a, b = np.zeros((6, 7, 15), dtype=np.uint8), np.zeros((6, 7, 15), dtype=np.uint8)
    a[1, 1, 1] = 1
    b[4, 5, 13] = 1
    cases.append(('two_voxels', a, b, dict(n_a=1, n_b=1, hd=13.0, hd95=13.0, assd=13.0, asd_ab=13.0, asd_ba=13.0)))
    # a 6^3 cube centred in a 12^3 cube (a volume of 14^3, so the big cube keeps clear of the faces).  Surfaces: 12^3 - 10^3 = 728 and
    # 6^3 - 4^3 = 152 voxels.  Big cube [1, 12], small cube [4, 9]: from a corner of the big cube the nearest small-cube voxel is its corner,
    # 3 away along every axis: max_ab = sqrt(27); every small-cube surface voxel has a big-cube face 3 voxels away and none nearer: the list
    # b -> a holds 152 times 3.
    a, b = np.zeros((14, 14, 14), dtype=np.uint8), np.zeros((14, 14, 14), dtype=np.uint8)
    a[1:13, 1:13, 1:13] = 1
    b[4:10, 4:10, 4:10] = 1
    cases.append(('cube_in_cube', a, b, dict(n_a=728, n_b=152, max_ab=math.sqrt(27.0), max_ba=3.0, asd_ba=3.0, hd=math.sqrt(27.0))))
    return cases
