"""The reference of the 3-D morphology tests (csrc/morph.hip: hv_morph_ball, hv_morph_struct, hv_morph_merge):
scipy.ndimage.binary_dilation / binary_erosion / binary_opening / binary_closing with the ball this file builds or with
generate_binary_structure(3, c), the merge rules in numpy, and the cases the CPU and GPU tests share.  Everything is Boolean: every comparison
is exact.

ball(): the integer offsets o with ((s0 o0)^2 + (s1 o1)^2) + (s2 o2)^2 <= radius * radius, float64 in this order -- the ordered sum of
tests/surface_ref.py's transform.  d2(): that transform's squared distances (before the square root) plus the border term, the nearest voxel
outside the volume; tests/test_morph_ref_cpu.py holds {d2 <= r r} against scipy's dilation by ball(), which is what the kernels rest on."""
import numpy as np
from scipy import ndimage

import surface_ref as SR

SPACINGS = SR.SPACINGS
RADII = (0.0, 1.0, np.sqrt(2.0), np.sqrt(3.0), 2.0, 2.5, 3.2)
OPS = ('dilation', 'erosion', 'opening', 'closing')
_SCIPY = {'dilation': ndimage.binary_dilation, 'erosion': ndimage.binary_erosion, 'opening': ndimage.binary_opening,
          'closing': ndimage.binary_closing}


def _steps(r2, s):
    """The largest d with (s d)^2 <= r2."""
    d = 0
    while (np.float64(s) * np.float64(d + 1)) * (np.float64(s) * np.float64(d + 1)) <= r2:
        d += 1
    return d


def ball(radius, spacing=(1.0, 1.0, 1.0)):
    r2 = np.float64(radius) * np.float64(radius)
    sq = []
    for s in spacing:
        n = _steps(r2, s)
        t = np.float64(s) * np.arange(-n, n + 1, dtype=np.float64)
        sq.append(t * t)
    return ((sq[0][:, None, None] + sq[1][None, :, None]) + sq[2][None, None, :]) <= r2


def ball_brute(radius, spacing=(1.0, 1.0, 1.0)):
    """The same set, one offset at a time over a box that certainly holds it -> the set of offsets."""
    r2 = float(radius) * float(radius)
    n = [int(np.floor(float(radius) / float(s))) + 2 for s in spacing]
    s0, s1, s2 = (float(s) for s in spacing)
    members = set()
    for a in range(-n[0], n[0] + 1):
        for b in range(-n[1], n[1] + 1):
            for c in range(-n[2], n[2] + 1):
                if ((s0 * a) * (s0 * a) + (s1 * b) * (s1 * b)) + (s2 * c) * (s2 * c) <= r2:
                    members.add((a, b, c))
    return members


def d2(X, spacing=(1.0, 1.0, 1.0), border=0):
    """float64 [shape]: the ordered squared distance of every voxel to the nearest member of X (surface_ref's three brute-force passes, the
    sum formed as ((s0 d0)^2 + (s1 d1)^2) + (s2 d2)^2; int64 at unit spacing, exact in float64 here), +inf if there is none; with border = 1
    the voxels outside the volume are members: the nearest lies min(i + 1, n - i) steps away along one axis."""
    X = np.asarray(X, dtype=bool)
    unit = SR.is_unit(spacing)
    g = np.where(X, np.int64(0), SR._BIG) if unit else np.where(X, 0.0, np.inf)
    for axis in range(3):
        g = SR._axis_min(g, axis, spacing[axis], unit)
    if unit:
        none = g >= SR._BIG
        g = np.where(none, 0, g).astype(np.float64)
        g[none] = np.inf
    if border:
        for axis, n in enumerate(X.shape):
            i = np.arange(n)
            t = np.float64(spacing[axis]) * np.minimum(i + 1, n - i).astype(np.float64)
            sh = [1, 1, 1]
            sh[axis] = n
            g = np.minimum(g, (t * t).reshape(sh))
    return g


def by_ball(op, X, radius, spacing=(1.0, 1.0, 1.0), border_value=0):
    """scipy's result with structure = ball(radius, spacing) -> bool."""
    return _SCIPY[op](np.asarray(X, dtype=bool), structure=ball(radius, spacing), border_value=border_value)


def by_struct(op, X, connectivity, iterations=1, border_value=0):
    return _SCIPY[op](np.asarray(X, dtype=bool), structure=ndimage.generate_binary_structure(3, connectivity), iterations=iterations,
                      border_value=border_value)


def merge(vol, mask, rule, value, background=0, fill=0):
    """hv_morph_merge: 'grow' -- mask set and vol == background -> value; 'shrink' -- vol == value and mask clear -> fill; else copied."""
    vol, mask = np.asarray(vol), np.asarray(mask).astype(bool)
    out = vol.copy()
    if rule == 'grow':
        out[mask & (vol == background)] = value
    else:
        out[(vol == value) & ~mask] = fill
    return out


def close_label(vol, value, radius, spacing=(1.0, 1.0, 1.0), background=0):
    return merge(vol, by_ball('closing', np.asarray(vol) == value, radius, spacing, 0), 'grow', value, background)


def open_label(vol, value, radius, spacing=(1.0, 1.0, 1.0), fill=0):
    return merge(vol, by_ball('opening', np.asarray(vol) == value, radius, spacing, 0), 'shrink', value, fill=fill)


# ------------------------------------------------------------------------------------------------ shared cases
def random_mask(shape, density, seed):
    return np.random.RandomState(seed).rand(*shape) < density


def contents(shape, seed=0):
    """name -> bool volume: random fill at three densities, the empty and the full set, a single voxel in a corner."""
    out = {'d%.2f' % d: random_mask(shape, d, seed + int(100 * d)) for d in (0.02, 0.5, 0.98)}
    out['empty'] = np.zeros(shape, dtype=bool)
    out['full'] = np.ones(shape, dtype=bool)
    corner = np.zeros(shape, dtype=bool)
    corner[0, shape[1] - 1, 0] = True
    out['corner'] = corner
    return out


def slabs(gap, shape=(9, 8, 16)):
    """Two slabs across axis 2 separated by `gap` empty planes, clear of every face."""
    v = np.zeros(shape, dtype=bool)
    v[2:-2, 2:-2, 3:6] = True
    v[2:-2, 2:-2, 6 + gap:9 + gap] = True
    return v


def bridged(shape=(12, 11, 20)):
    """Two bodies joined by a bridge one voxel thick -> (the volume, the bridge's voxels)."""
    v = np.zeros(shape, dtype=bool)
    v[2:9, 2:9, 2:8] = True
    v[2:9, 2:9, 12:18] = True
    bridge = np.zeros(shape, dtype=bool)
    bridge[5, 5, 8:12] = True
    return v | bridge, bridge


def two_fragment_body(label=20, other=19, shape=(24, 22, 30)):
    """A body of `label` with a cavity, a fragment of the same label behind a one-voxel gap (smaller than the body), a far speckle, and
    another label beside them, all clear of the faces -> uint8 volume."""
    v = np.zeros(shape, dtype=np.uint8)
    v[4:18, 4:18, 4:14] = label
    v[9:12, 9:12, 7:10] = 0                          # a cavity
    v[6:16, 6:16, 15:19] = label                     # the fragment: plane 14 is the gap
    v[20, 19, 26] = label                            # a speckle
    v[4:18, 4:18, 21:25] = other
    return v
