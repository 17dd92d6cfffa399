"""Numpy float64 restatement of scipy.ndimage's geometric transforms as the device implements them (csrc/resample.hip through hv_resample;
DESIGN.md section 8 row f15): affine_transform, zoom and shift of a 3-D volume at orders 0 / 1 / 3.  No device.

Coordinates, float64, no fused multiply-add.  For output index o and input axis h
  matrix form      u_h = ((o0 m[h][0] + o1 m[h][1]) + o2 m[h][2]) + offset[h]     (the products summed from 0.0, the offset added last)
  zoom-shift form  u_h = (o_h + shift[h]) * zoom[h]                               (scipy's zoom_shift: zoom, shift, a 1-D matrix)
Sampling (NI_GeometricTransform / NI_ZoomShift).  mode 'constant': u_h < 0 or u_h > A_h - 1 on any axis gives cval; mode 'nearest' (order 0
only): u_h is clamped to [0, A_h - 1].  Order 0 reads the voxel at floor(u + 0.5); order 1 the taps floor(u), floor(u) + 1 with the weights
w0 = 1 - y and 1 - w0 (scipy forms the last weight as one minus the others; it is not always y, and the difference shows in float64 results);
order 3 the four taps floor(u) - 1 .. floor(u) + 2 of the B-spline coefficients with the weights of tests/spline_ref.py.  Tap indices beyond
the ends are mirrored about the end points.  The sum runs over the taps with the last axis fastest, each term ((c w0) w1) w2, added from 0.0.
Output: float64 as it is; float32 rounded once; int16 t > 0 ? t + 0.5 : t - 0.5, clamped, truncated; uint8 t > 0 ? t + 0.5 : 0, clamped,
truncated.

Found against scipy 1.15.3 (tests/test_resample_ref_cpu.py): everything above is bit for bit in mode 'constant' at all three orders and in
mode 'nearest' at order 0.  At order 1 a clamped coordinate does NOT reproduce scipy's 'nearest' in the last bit of float64 results, so that
pair is refused (sample() raises).  The order-3 coefficients: spline_filter_scipy() restates ni_splines.c and is within rounding of
scipy.ndimage.spline_filter(v, 3, mode='mirror') but not bit for bit (neither is tests/spline_ref.py's, nor the device's prefilter with its
Horner form and 32-term horizon; each is within SPLINE_TOL).  The sampler is pinned bit for bit on coefficients handed over with coef=: scipy's
own on the host, the device's own in the device tests.  On whole-number data the rounding of a uint8 / int16 / float32 output absorbs the
prefilter's last bits."""
import numpy as np

Z = np.sqrt(3.0) - 2.0
DTYPES = (np.uint8, np.int16, np.float32, np.float64)
TILE = 8                                  # hv_resample_tile: outputs per workgroup along each axis


# ------------------------------------------------------------------------------------------------ the prefilter, scipy's order
def _filter_lines_scipy(c):
    """ni_splines.c apply_filter with the one pole of order 3 and the mirror boundary, along axis 0 of c (float64, in place)."""
    n = c.shape[0]
    if n == 1:
        return c
    c *= (1.0 - Z) * (1.0 - 1.0 / Z)
    zn1 = Z ** (n - 1)
    zi = Z
    c[0] = c[0] + zn1 * c[n - 1]
    for i in range(1, n - 1):
        c[0] += zi * (c[i] + zn1 * c[n - 1 - i])
        zi *= Z
    c[0] /= 1.0 - zn1 * zn1
    for i in range(1, n):
        c[i] += Z * c[i - 1]
    c[n - 1] = (Z * c[n - 2] + c[n - 1]) * Z / (Z * Z - 1.0)
    for i in range(n - 2, -1, -1):
        c[i] = Z * (c[i + 1] - c[i])
    return c


def spline_filter_scipy(v):
    c = np.array(v, dtype=np.float64)
    for axis in range(c.ndim):
        _filter_lines_scipy(np.moveaxis(c, axis, 0))
    return c


# ------------------------------------------------------------------------------------------------ coordinates
def _grid(shape):
    return [g.astype(np.float64).ravel() for g in np.meshgrid(*[np.arange(n) for n in shape], indexing='ij')]


def coords_matrix(out_shape, matrix, offset):
    m = np.asarray(matrix, dtype=np.float64).reshape(3, 3)
    off = np.asarray(offset, dtype=np.float64).reshape(3)
    o = _grid(out_shape)
    u = []
    for h in range(3):
        s = 0.0 + o[0] * m[h, 0]
        s = s + o[1] * m[h, 1]
        s = s + o[2] * m[h, 2]
        u.append(s + off[h])
    return np.stack(u)


def coords_zoomshift(out_shape, zoom, shift):
    z = np.asarray(zoom, dtype=np.float64).reshape(3)
    s = np.asarray(shift, dtype=np.float64).reshape(3)
    o = _grid(out_shape)
    return np.stack([(o[h] + s[h]) * z[h] for h in range(3)])


# ------------------------------------------------------------------------------------------------ sampling
def _mirror(idx, n):
    if n == 1:
        return np.zeros_like(idx)
    p = 2 * (n - 1)
    idx = np.abs(idx) % p
    return np.where(idx >= n, p - idx, idx)


def _taps(u, n, order):
    if order == 0:
        return np.floor(u + 0.5).astype(np.int64)[None], np.ones((1,) + u.shape)
    f = np.floor(u)
    y = u - f
    i = f.astype(np.int64)
    if order == 1:
        w0 = 1.0 - y
        return _mirror(np.stack([i, i + 1]), n), np.stack([w0, 1.0 - w0])         # scipy: the last weight is 1 - the others, not y
    z = 1.0 - y
    w1 = (y * y * (y - 2.0) * 3.0 + 4.0) / 6.0
    w2 = (z * z * (z - 2.0) * 3.0 + 4.0) / 6.0
    w0 = z * z * z / 6.0
    return _mirror(i[None] + np.arange(-1, 3)[:, None], n), np.stack([w0, w1, w2, 1.0 - w0 - w1 - w2])


def sample(src, u, order, mode='constant', cval=0.0):
    """The float64 sums t at the coordinates u [3, M] of src (order 3: the coefficients)."""
    A = src.shape
    u = np.array(u, dtype=np.float64)
    if mode == 'constant':
        inside = np.ones(u.shape[1], dtype=bool)
        for h in range(3):
            inside &= (u[h] >= 0.0) & (u[h] <= A[h] - 1)
    elif mode == 'nearest' and order == 0:
        for h in range(3):
            u[h] = np.where(u[h] >= 0.0, np.where(u[h] <= A[h] - 1, u[h], float(A[h] - 1)), 0.0)
        inside = np.ones(u.shape[1], dtype=bool)
    else:
        raise ValueError('mode %r is not offered' % (mode,))
    ui = u[:, inside]
    (i0, w0), (i1, w1), (i2, w2) = (_taps(ui[h], A[h], order) for h in range(3))
    acc = np.zeros(ui.shape[1])
    with np.errstate(invalid='ignore'):
        for a in range(len(i0)):
            for b in range(len(i1)):
                for c in range(len(i2)):
                    v = src[i0[a], i1[b], i2[c]].astype(np.float64)
                    acc += v if order == 0 else ((v * w0[a]) * w1[b]) * w2[c]
    t = np.full(u.shape[1], float(cval))
    t[inside] = acc
    return t


def convert(t, dtype):
    dtype = np.dtype(dtype)
    if dtype == np.float64:
        return t.copy()
    if dtype == np.float32:
        with np.errstate(over='ignore'):
            return t.astype(np.float32)
    if dtype == np.int16:
        r = np.where(t > 0, t + 0.5, t - 0.5)
        return np.trunc(np.clip(r, -32768.0, 32767.0)).astype(np.int16)
    if dtype == np.uint8:
        r = np.where(t > 0, t + 0.5, 0.0)
        return np.trunc(np.clip(r, 0.0, 255.0)).astype(np.uint8)
    raise TypeError(dtype)


def resample(vol, out_shape, order, form, a, b, mode='constant', cval=0.0, output=None, coef=None):
    """form 'matrix': a, b = matrix [3][3], offset [3]; form 'zoomshift': a, b = zoom [3], shift [3] -> array of out_shape, vol's dtype unless
    `output`.  coef: the order-3 coefficients to sample (default spline_filter_scipy(vol))."""
    vol = np.asarray(vol)
    src = vol
    if order == 3:
        src = spline_filter_scipy(vol) if coef is None else np.asarray(coef, dtype=np.float64)
    u = coords_matrix(out_shape, a, b) if form == 'matrix' else coords_zoomshift(out_shape, a, b)
    t = sample(src, u, order, mode, cval)
    return convert(t, vol.dtype if output is None else output).reshape(out_shape)


# ------------------------------------------------------------------------------------------------ scipy's front ends
def affine_transform(vol, matrix, offset=0.0, output_shape=None, order=3, mode='constant', cval=0.0, output=None, coef=None):
    vol = np.asarray(vol)
    m = np.asarray(matrix, dtype=np.float64)
    shape = tuple(vol.shape if output_shape is None else output_shape)
    if m.ndim == 2 and m.shape in ((3, 4), (4, 4)):
        offset, m = m[:3, 3], m[:3, :3]
    off = np.full(3, offset, dtype=np.float64) if np.ndim(offset) == 0 else np.asarray(offset, dtype=np.float64)
    if m.ndim == 1:
        return resample(vol, shape, order, 'zoomshift', m, off / m, mode, cval, output, coef)
    return resample(vol, shape, order, 'matrix', m, off, mode, cval, output, coef)


def zoom_arguments(in_shape, zoom):
    z = (float(zoom),) * 3 if np.ndim(zoom) == 0 else tuple(float(x) for x in zoom)
    out_shape = tuple(int(round(n * f)) for n, f in zip(in_shape, z))
    step = tuple((n - 1) / (o - 1) if o != 1 else 1.0 for n, o in zip(in_shape, out_shape))
    return out_shape, step


def zoom(vol, zoom, order=3, mode='constant', cval=0.0, output=None, coef=None):
    vol = np.asarray(vol)
    out_shape, step = zoom_arguments(vol.shape, zoom)
    return resample(vol, out_shape, order, 'zoomshift', step, (0.0, 0.0, 0.0), mode, cval, output, coef)


def shift(vol, shift, order=3, mode='constant', cval=0.0, output=None, coef=None):
    vol = np.asarray(vol)
    s = (float(shift),) * 3 if np.ndim(shift) == 0 else tuple(float(x) for x in shift)
    return resample(vol, vol.shape, order, 'zoomshift', (1.0, 1.0, 1.0), tuple(-x for x in s), mode, cval, output, coef)


# ------------------------------------------------------------------------------------------------ shared cases
def case_volume(dtype, shape=(7, 9, 6), seed=0):
    """A random volume: floats in [-1, 1) scaled by 300; int16 whole numbers reaching both ends of the type, so that order 3 overshoots the
    clamps and the negative rounding branch is hit; uint8 reaching 0 and 255, so that order 3 overshoots below 0 and above 255."""
    r = np.random.RandomState(seed)
    dtype = np.dtype(dtype)
    if dtype == np.int16:
        v = r.randint(-32768, 32768, size=shape).astype(np.int16)
        v.flat[:4] = (-32768, 32767, -32768, 32767)
        return v
    if dtype == np.uint8:
        v = r.randint(0, 256, size=shape).astype(np.uint8)
        v.flat[:4] = (0, 255, 0, 255)
        return v
    return ((r.random_sample(shape) * 2.0 - 1.0) * 300.0).astype(dtype)


MATRIX = np.array([[0.9, 0.12, -0.07], [-0.15, 1.1, 0.2], [0.05, -0.3, 0.6]])
OFFSET = np.array([0.4, 1.3, 0.8])
DIAGONAL = np.array([0.8, 1.25, 0.6])
DIAG_OFFSET = np.array([0.3, -0.4, 0.2])
OUT_SHAPE = (8, 7, 9)
ZOOMS = ((2.0, 1.5, 1.7), (0.5, 0.7, 0.6), (1.0, 1.0, 1.0), (0.1, 1.3, 0.1))       # larger, smaller, equal, extents of 1
SHIFTS = ((0.3, -1.7, 2.25), (-0.3, 0.5, -0.01))
