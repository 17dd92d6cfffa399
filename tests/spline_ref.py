"""Numpy float64 restatement of scipy.ndimage.map_coordinates(v, coords, order=3, mode='constant', cval=0), the two steps the device
implements (csrc/spline.hip, csrc/spline_tap.h), and the loader of fixture G23 (tools/make_golden_spline.py).  No device.

Step 1, the prefilter, is spline_filter(v, 3, mode='mirror') in float64: along each axis in turn, with z = sqrt(3) - 2, each line c[0..n-1]
  is scaled by (1 - z)(1 - 1/z);  c[0] = (c[0] + z^(n-1) c[n-1] + sum_{i=1..n-2} (z^i + z^(2n-2-i)) c[i]) / (1 - z^(2n-2));
  c[i] += z c[i-1];  c[n-1] = z / (z^2 - 1) (c[n-1] + z c[n-2]);  c[i] = z (c[i+1] - c[i]);  a line of length 1 is left as it is.
Step 2, the sample: a coordinate outside [0, n - 1] on any axis gives 0; otherwise i = floor(u), t = u - i, the taps i - 1 .. i + 2 carry the
  cubic B-spline weights and tap indices outside the line are mirrored (-1 -> 1, n -> n - 2).  Nothing is clipped.
"""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANE = (128, 128)
WINDOW = (-300.0, 800.0)
Z = np.sqrt(3.0) - 2.0

# Measured on the host by tests/test_spline_cpu.py (which asserts them again), rounded up to two digits: the largest |restatement - scipy| over
# its prefilter cases (2.73e-12: random whole numbers, whose coefficients are some 30 times the data; divided by max|data| / 255 where the data
# is larger than 255) and its sample cases (3.13e-13), and the largest |restatement - G23| over the fixture's crops (2.84e-13 in all three cases;
# windowed CT, magnitude <= 255 plus the overshoot).
MEASURED_SCIPY = 2.8e-12
MEASURED_G23 = 2.9e-13
# The device tolerance: 10 x the larger of the two, floor 1e-9 (the project's crop tolerance) -- for data of
# magnitude up to 255; a test with larger data scales it by max|data| / 255.
SPLINE_TOL = max(10 * max(MEASURED_SCIPY, MEASURED_G23), 1e-9)


def window(v, wmin=WINDOW[0], wmax=WINDOW[1]):
    """window(img, win_min, win_max) (straighten_mask_3d.py:178-183) without its whole-volume shortcut."""
    return np.clip(255.0 * (np.asarray(v, dtype=np.float64) - wmin) / (wmax - wmin), 0.0, 255.0)


def filter_lines(c):
    """The recursive filter along axis 0 of c (float64, modified in place): every column is one line."""
    n = c.shape[0]
    if n == 1:
        return c
    c *= (1.0 - Z) * (1.0 - 1.0 / Z)
    i = np.arange(1, n - 1).reshape((-1,) + (1,) * (c.ndim - 1))
    c[0] = (c[0] + Z ** (n - 1) * c[n - 1] + ((Z ** i + Z ** (2 * n - 2 - i)) * c[1:n - 1]).sum(0)) / (1.0 - Z ** (2 * n - 2))
    for k in range(1, n):
        c[k] += Z * c[k - 1]
    c[n - 1] = Z / (Z * Z - 1.0) * (c[n - 1] + Z * c[n - 2])
    for k in range(n - 2, -1, -1):
        c[k] = Z * (c[k + 1] - c[k])
    return c


def spline_filter3(v):
    """scipy.ndimage.spline_filter(v, 3, mode='mirror') in float64."""
    c = np.array(v, dtype=np.float64)
    for axis in range(c.ndim):
        m = np.moveaxis(c, axis, 0)
        filter_lines(m)
    return c


def _taps(u, n):
    f = np.floor(u)
    y = u - f
    z = 1.0 - y
    w1 = (y * y * (y - 2.0) * 3.0 + 4.0) / 6.0
    w2 = (z * z * (z - 2.0) * 3.0 + 4.0) / 6.0
    w0 = z * z * z / 6.0
    w = np.stack([w0, w1, w2, 1.0 - w0 - w1 - w2])
    idx = f.astype(np.int64)[None] + np.arange(-1, 3)[:, None]
    if n == 1:
        idx = np.zeros_like(idx)
    else:
        p = 2 * (n - 1)
        idx = np.abs(idx) % p
        idx = np.where(idx >= n, p - idx, idx)
    return idx, w


def sample3(coef, coords):
    """Step 2 on the coefficients `coef` ([n0, n1, n2] float64) at coords [3, M] -> [M]."""
    coords = np.asarray(coords, dtype=np.float64)
    shape = coef.shape
    inside = np.ones(coords.shape[1], dtype=bool)
    for a in range(3):
        inside &= (coords[a] >= 0.0) & (coords[a] <= shape[a] - 1)
    out = np.zeros(coords.shape[1])
    u = coords[:, inside]
    (i0, w0), (i1, w1), (i2, w2) = (_taps(u[a], shape[a]) for a in range(3))
    acc = np.zeros(u.shape[1])
    for a in range(4):
        for b in range(4):
            for c in range(4):
                acc += ((coef[i0[a], i1[b], i2[c]] * w0[a]) * w1[b]) * w2[c]
    out[inside] = acc
    return out


def map_coordinates3(v, coords):
    """scipy.ndimage.map_coordinates(v, coords, order=3, mode='constant', cval=0) for a 3-D v and coords [3, ...]."""
    coords = np.asarray(coords, dtype=np.float64)
    return sample3(spline_filter3(v), coords.reshape(3, -1)).reshape(coords.shape[1:])


def straight_grid(knots, basis, spacing, plane=PLANE):
    """Sample coordinates of the straight volume [N][PA][PB] in voxel indices of the scan (csrc/straighten.hip's, Interpolator.get_grid's):
    (knots[n] + basis[n][:, 1] (b - PB / 2) + basis[n][:, 2] (a - PA / 2)) / spacing -> [3, N, PA, PB]."""
    PB, PA = plane
    gb = (np.arange(PB, dtype=np.float64) - PB / 2.0)[None, None, :, None]
    ga = (np.arange(PA, dtype=np.float64) - PA / 2.0)[None, :, None, None]
    g = ((basis[:, None, None, :, 0] * 0.0 + basis[:, None, None, :, 1] * gb) + basis[:, None, None, :, 2] * ga) + knots[:, None, None, :]
    return np.moveaxis(g / np.asarray(spacing, dtype=np.float64), -1, 0)


def crop(src, box, out_size):
    """extract_3d_volume as straighten.crop_box lays it out."""
    out = np.zeros(out_size, dtype=src.dtype)
    lo, n, st = box[0:3], box[3:6], box[6:9]
    out[st[0]:st[0] + n[0], st[1]:st[1] + n[1], st[2]:st[2] + n[2]] = src[lo[0]:lo[0] + n[0], lo[1]:lo[1] + n[1], lo[2]:lo[2] + n[2]]
    return out


def straighten_crops(ct, plan, out_size, win, spacing, mapper=None):
    """The CT crops of straighten_patient(order=3) from the host plan (knots, basis, local, boxes): window, cubic resample, crop -> [V, *out_size].
    mapper: map_coordinates3 (default) or scipy's with order=3."""
    knots, basis, _, boxes = plan
    v = window(ct) if win else np.asarray(ct, dtype=np.float64)
    grid = straight_grid(knots, basis, spacing)
    straight = (mapper or map_coordinates3)(v, grid)
    return np.stack([crop(straight, [int(x) for x in b], tuple(out_size)) for b in boxes])


LENGTHS = (1, 2, 3, 4, 63, 64, 65, 257)     # line lengths of the prefilter edge cases: below, at and past the tile (32) and the horizon


def prefilter_shapes():
    """Every length of LENGTHS on each of the three axes in turn beside extents 5 and 7 (multiples of no tile), and one 1 x 1 x 1030 line."""
    shapes = []
    for axis in range(3):
        for n in LENGTHS:
            s = [5, 7]
            s.insert(axis, n)
            shapes.append(tuple(s))
    return shapes + [(1, 1, 1030)]


def case_volume(shape, seed=0):
    """A float64 volume of whole numbers in [-1000, 2000] (exact in int16 and float32 too): both ends leave the bone window."""
    return np.random.RandomState(seed).randint(-1000, 2001, size=shape).astype(np.float64)


def scale_of(v):
    """The factor on SPLINE_TOL for data `v`: the tolerance is stated for magnitudes up to 255."""
    return max(1.0, float(np.abs(v).max()) / 255.0)


def make_patient(kw, swap):
    from hvgan import synth
    ct, label = synth.make_spine_patient(**kw)
    if swap:
        ct, label = np.ascontiguousarray(ct.transpose(2, 1, 0)), np.ascontiguousarray(label.transpose(2, 1, 0))
    return ct, label


def load_g23():
    """-> {case: {'spacing', 'ids', 'out_size', 'centroid_list', 'window', 'boxes', 'crop_ct' [V, *out_size], 'crop_label', 'ct', 'label' (the
    synthetic patient, rebuilt from the recorded arguments)}}."""
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'g23_spline.npz'))
    cases = {}
    for k in z.files:
        name, key = k.split('/')
        cases.setdefault(name, {})[key] = z[k]
    for c in cases.values():
        kw = json.loads(str(c.pop('kwargs')))
        kw = {k: tuple(v) if isinstance(v, list) else v for k, v in kw.items()}
        c['ct'], c['label'] = make_patient(kw, bool(c.pop('swap02')))
        c['spacing'] = tuple(float(v) for v in c['spacing'])
        c['ids'] = [int(v) for v in c['ids']]
        c['out_size'] = tuple(int(v) for v in c['out_size'])
        c['window'] = bool(c['window'])
        c['centroid_list'] = [{'label': int(r[0]), 'X': float(r[1]), 'Y': float(r[2]), 'Z': float(r[3])} for r in c['centroids']]
    return cases


def plan_of(c):
    """The host plan tuple (knots, basis, local, boxes) of a G23 case."""
    from hvgan import straighten as S
    return S.plan(c['centroid_list'], c['ct'].shape, c['ids'], c['out_size'], spacing=c['spacing'])
