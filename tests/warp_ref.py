"""Numpy float64 restatement of the deformable resampling as the device implements it (csrc/warp.hip through hv_map_coordinates and
hv_warp_grid).  No device.  From the coordinate u on everything is tests/resample_ref.py's sample() and
convert(); this file adds the three rules that make u, float64, no fused multiply-add:
  absolute       u_h = c_h(o)                      a float32 coordinate is widened exactly              scipy.ndimage.map_coordinates
  displacement   u_h = (double)o_h + c_h(o)        a dense displacement field in source voxels
  control grid   q_a = (o_a + gshift[a]) * gzoom[a], clamped to [0, G_a - 1] as q >= 0 ? (q <= hi ? q : hi) : 0
                 d_h = sample(grid[h], q, gorder)  order 1, or order 3 on the control values themselves (no prefilter)
                 u_h = base_h(o) + d_h             base: coords_matrix / coords_zoomshift of resample_ref
and random_control_values' arithmetic.

Found against scipy 1.15.3 (tests/test_warp_ref_cpu.py): convert(sample(...)) equals map_coordinates(..., prefilter=False) bit for bit for
all four output dtypes, orders 0 / 1 / 3 in mode 'constant' and order 0 in mode 'nearest', float64 and float32 coordinates, on 0, on A - 1,
one ulp beyond each, on -0.0 and on NaN.  A NaN coordinate gives cval in mode 'constant' for the integer outputs as for the float ones; in
mode 'nearest' scipy's clamp leaves a NaN at index 0, and so does the restatement's (and the device's) clamp form."""
import math

import numpy as np

import resample_ref as R

ABSOLUTE, DISPLACEMENT = 0, 1


# ------------------------------------------------------------------------------------------------ the three coordinate rules
def coords_absolute(coordinates):
    c = np.asarray(coordinates)
    return c.astype(np.float64).reshape(3, -1)


def coords_displacement(displacement, spacing=None):
    d = np.asarray(displacement)
    if spacing is not None:
        d = d.astype(np.float64) / np.asarray(spacing, dtype=np.float64).reshape(3, 1, 1, 1)
    o = R._grid(d.shape[1:])
    return np.stack([o[h] + d[h].astype(np.float64).ravel() for h in range(3)])


def grid_coordinate(out_shape, G, gzoom, gshift):
    """q [3, M]: the clamped grid coordinate of every output voxel."""
    o = R._grid(out_shape)
    q = []
    for a in range(3):
        x = (o[a] + float(gshift[a])) * float(gzoom[a])
        hi = float(G[a] - 1)
        q.append(np.where(x >= 0.0, np.where(x <= hi, x, hi), 0.0))
    return np.stack(q)


def displacement_of(values, out_shape, gzoom, gshift, gorder):
    """[3, *out_shape] float64: each component of the control values sampled at q at order gorder, as they are (no prefilter)."""
    values = np.asarray(values, dtype=np.float64)
    q = grid_coordinate(out_shape, values.shape[1:], gzoom, gshift)
    return np.stack([R.sample(values[h], q, gorder) for h in range(3)]).reshape((3,) + tuple(out_shape))


def coords_grid(out_shape, values, gzoom, gshift, gorder, form='zoomshift', a=(1.0, 1.0, 1.0), b=(0.0, 0.0, 0.0)):
    base = R.coords_matrix(out_shape, a, b) if form == 'matrix' else R.coords_zoomshift(out_shape, a, b)
    d = displacement_of(values, out_shape, gzoom, gshift, gorder).reshape(3, -1)
    return np.stack([base[h] + d[h] for h in range(3)])


# ------------------------------------------------------------------------------------------------ the entries
def _source(vol, order, coef):
    vol = np.asarray(vol)
    if order == 3:
        return R.spline_filter_scipy(vol) if coef is None else np.asarray(coef, dtype=np.float64)
    return vol


def _finish(vol, u, shape, order, mode, cval, output, coef):
    vol = np.asarray(vol)
    t = R.sample(_source(vol, order, coef), u, order, mode, cval)
    return R.convert(t, vol.dtype if output is None else output).reshape(shape)


def map_coordinates(vol, coordinates, order=3, mode='constant', cval=0.0, output=None, coef=None):
    return _finish(vol, coords_absolute(coordinates), np.asarray(coordinates).shape[1:], order, mode, cval, output, coef)


def warp(vol, displacement, spacing=None, order=1, mode='constant', cval=0.0, output=None, coef=None):
    return _finish(vol, coords_displacement(displacement, spacing), np.asarray(displacement).shape[1:], order, mode, cval, output, coef)


def control_gzoom(G, out_shape):
    return tuple((g - 1) / (o - 1) if o != 1 else 1.0 for g, o in zip(G, out_shape))


def warp_grid(vol, values, out_shape, gorder=3, gzoom=None, gshift=(0.0, 0.0, 0.0), form='zoomshift', a=(1.0, 1.0, 1.0), b=(0.0, 0.0, 0.0),
              order=1, mode='constant', cval=0.0, output=None, coef=None):
    values = np.asarray(values, dtype=np.float64)
    gzoom = control_gzoom(values.shape[1:], out_shape) if gzoom is None else gzoom
    return _finish(vol, coords_grid(out_shape, values, gzoom, gshift, gorder, form, a, b), tuple(out_shape), order, mode, cval, output, coef)


def random_control_values(out_shape, spacing, control_mm, amplitude_mm, seed, fix_border=True, clip=0.4):
    G = tuple(max(2, int(math.ceil((o - 1) / (control_mm / spacing[a]))) + 1) if o != 1 else 1 for a, o in enumerate(out_shape))
    v = np.random.RandomState(seed).standard_normal((3,) + G)
    for h in range(3):
        delta = (out_shape[h] - 1) / (G[h] - 1) if G[h] != 1 else control_mm / spacing[h]
        v[h] *= amplitude_mm / spacing[h]
        v[h] = np.clip(v[h], -clip * delta, clip * delta)
    if fix_border:
        for a in range(3):
            if G[a] != 1:
                v.swapaxes(1, a + 1)[:, 0] = 0.0
                v.swapaxes(1, a + 1)[:, -1] = 0.0
    return v


def control_spacing(out_shape, G, spacing, control_mm):
    return tuple((o - 1) / (g - 1) if g != 1 else control_mm / s for o, g, s in zip(out_shape, G, spacing))


# ------------------------------------------------------------------------------------------------ shared cases
SRC_SHAPE = (7, 9, 6)
CVAL = 3.0
ORDER_MODES = ((0, 'constant'), (1, 'constant'), (3, 'constant'), (0, 'nearest'))
OUT_SHAPES = tuple(tuple(n if i == axis else m for i, m in enumerate((5, 6, 4))) for axis in range(3) for n in (7, 8, 9)) + ((17, 9, 10), (1, 6, 5))
GRIDS = ((4, 5, 3), (2, 2, 2), (3, 1, 4))


def case_coordinates(out_shape, dtype=np.float64, seed=11, src_shape=SRC_SHAPE):
    """Random coordinates over the source box and a little beyond it, so that some fall outside on every side."""
    r = np.random.RandomState(seed)
    c = np.stack([r.uniform(-0.7, n - 1 + 0.7, size=out_shape) for n in src_shape])
    return c.astype(dtype)


def edge_coordinates(dtype=np.float64, src_shape=SRC_SHAPE):
    """[3, M]: per axis, coordinates on 0, on A - 1, one ulp beyond each (in `dtype`), on -0.0 and on NaN; the other two axes inside."""
    dtype = np.dtype(dtype)
    cols = []
    mid = [1.25, 2.5, 3.75]
    for h, n in enumerate(src_shape):
        lo, hi = dtype.type(0.0), dtype.type(n - 1)
        for x in (lo, hi, np.nextafter(lo, dtype.type(-1)), np.nextafter(hi, dtype.type(1e9)), np.nextafter(hi, dtype.type(0)),
                  dtype.type(-0.0), dtype.type(np.nan)):
            col = list(mid)
            col[h] = x
            cols.append(col)
    cols.append([0.0, 0.0, 0.0])
    cols.append([n - 1 for n in src_shape])
    return np.array(cols, dtype=dtype).T.copy()


def case_displacement(shape, seed=12, scale=1.5):
    return np.random.RandomState(seed).uniform(-scale, scale, size=(3,) + tuple(shape))


def case_grid(G, seed=13, scale=1.2):
    return np.random.RandomState(seed).uniform(-scale, scale, size=(3,) + tuple(G))
