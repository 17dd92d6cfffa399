"""A numpy restatement of scipy.ndimage.correlate1d / gaussian_filter1d / gaussian_filter for odd-length weights and origin 0, and of
filters.smooth_label / feather_blend built from it: what csrc/filter3d.hip computes, operation for operation.  tests/test_filters_ref_cpu.py
pins it against scipy bit for bit; tests/test_filters_gpu.py compares the device against it bit for bit.

Everything is float64.  The loop over the taps is written out in scipy's order (NI_Correlate1D); each step is one elementwise numpy operation
over all outputs at once, which rounds every output exactly as a scalar loop would."""
import numpy as np

MODES = ('reflect', 'constant', 'nearest', 'mirror', 'wrap')
EPS = np.finfo(np.float64).eps


# ------------------------------------------------------------------------------------------------ the boundary index maps
def index_map(p, n, mode):
    """The index in [0, n) that position p (any integer) of the extended line reads, -1 where mode 'constant' reads cval.
    reflect: d c b a | a b c d | d c b a; mirror: d c b | a b c d | c b a; wrap: a b c d | a b c d; the patterns repeat."""
    p = np.asarray(p, dtype=np.int64)
    if mode == 'constant':
        return np.where((p >= 0) & (p < n), p, -1)
    if mode == 'nearest':
        return np.clip(p, 0, n - 1)
    if mode == 'wrap':
        return np.mod(p, n)
    if mode == 'reflect':
        m = np.mod(p, 2 * n)
        return np.where(m < n, m, 2 * n - 1 - m)
    if mode == 'mirror':
        if n == 1:
            return np.zeros_like(p)
        m = np.mod(p, 2 * n - 2)
        return np.where(m < n, m, 2 * n - 2 - m)
    raise ValueError(mode)


def extend(a, r, mode, cval):
    """a [..., n] float64 -> [..., n + 2 r]: the lines extended by r on both sides."""
    n = a.shape[-1]
    idx = index_map(np.arange(-r, n + r), n, mode)
    x = a[..., np.maximum(idx, 0)]
    if mode == 'constant':
        x = np.where(idx >= 0, x, np.float64(cval))
    return x


# ------------------------------------------------------------------------------------------------ the three summation forms
def detect_form(w):
    """+1 symmetric, -1 antisymmetric, 0 general: scipy's test with DBL_EPSILON."""
    w = np.asarray(w, dtype=np.float64)
    r = len(w) // 2
    if all(abs(w[r + ii] - w[r - ii]) <= EPS for ii in range(1, r + 1)):
        return 1
    if all(abs(w[r + ii] + w[r - ii]) <= EPS for ii in range(1, r + 1)):
        return -1
    return 0


def correlate_lines(x, w, form, n):
    """x [..., n + 2 r] extended lines -> [..., n]; output l sits at c = l + r of its extended line."""
    r = len(w) // 2
    at = lambda o: x[..., r + o:r + o + n]          # x[c + o] for every output
    if form > 0:
        t = at(0) * w[r]
        for ii in range(-r, 0):
            t = t + (at(ii) + at(-ii)) * w[ii + r]
    elif form < 0:
        t = at(0) * w[r]
        for ii in range(-r, 0):
            t = t + (at(ii) - at(-ii)) * w[ii + r]
    else:
        t = at(r) * w[2 * r]                        # scipy starts the general sum with the LAST tap, then adds the others from the first
        for ii in range(0, 2 * r):
            t = t + at(ii - r) * w[ii]
    return t


def correlate1d(a, weights, axis=-1, mode='reflect', cval=0.0):
    w = np.asarray(weights, dtype=np.float64)
    if w.ndim != 1 or len(w) % 2 != 1:
        raise ValueError('odd-length weights expected')
    a = np.moveaxis(np.asarray(a).astype(np.float64), axis, -1)
    out = correlate_lines(extend(a, len(w) // 2, mode, cval), w, detect_form(w), a.shape[-1])
    return np.ascontiguousarray(np.moveaxis(out, -1, axis))


# ------------------------------------------------------------------------------------------------ Gaussian weights and filters
def gaussian_kernel1d(sigma, order, radius):
    """scipy.ndimage._filters._gaussian_kernel1d."""
    if order < 0:
        raise ValueError('order must be non-negative')
    exponent_range = np.arange(order + 1)
    sigma2 = sigma * sigma
    x = np.arange(-radius, radius + 1)
    phi_x = np.exp(-0.5 / sigma2 * x ** 2)
    phi_x = phi_x / phi_x.sum()
    if order == 0:
        return phi_x
    q = np.zeros(order + 1)
    q[0] = 1
    D = np.diag(exponent_range[1:], 1)
    P = np.diag(np.ones(order) / -sigma2, -1)
    Q_deriv = D + P
    for _ in range(order):
        q = Q_deriv.dot(q)
    q = (x[:, None] ** exponent_range).dot(q)
    return q * phi_x


def gaussian_filter1d(a, sigma, axis=-1, order=0, mode='reflect', cval=0.0, truncate=4.0, radius=None):
    sd = float(sigma)
    lw = int(truncate * sd + 0.5) if radius is None else int(radius)
    return correlate1d(a, gaussian_kernel1d(sigma, order, lw)[::-1], axis, mode, cval)


def _per_axis(v, name):
    v = tuple(v) if np.ndim(v) else (v,) * 3
    if len(v) != 3:
        raise ValueError('%s: a scalar or three values expected' % name)
    return v


def gaussian_filter(a, sigma, order=0, mode='reflect', cval=0.0, truncate=4.0, radius=None, spacing=None):
    """scipy.ndimage.gaussian_filter of the float64 copy of a 3-D array; spacing: sigma is in its units, sigma_vox = sigma / spacing[a]."""
    sig, orders, radii = _per_axis(sigma, 'sigma'), _per_axis(order, 'order'), _per_axis(radius, 'radius')
    if spacing is not None:
        sig = tuple(float(s) / float(sp) for s, sp in zip(sig, _per_axis(spacing, 'spacing')))
    out = np.asarray(a).astype(np.float64)
    for ax in range(3):
        if sig[ax] > 1e-15:
            out = gaussian_filter1d(out, sig[ax], ax, orders[ax], mode, cval, truncate, radii[ax])
    return out


# ------------------------------------------------------------------------------------------------ what filters.py builds from them
def merge(vol, mask, value, background=0, fill=0):
    """The mask of a label written back: gained voxels only where the volume holds `background`, lost voxels become `fill`."""
    vol = np.asarray(vol)
    out = vol.copy()
    out[mask & (vol == background)] = value
    out[~mask & (vol == value)] = fill
    return out


def smooth_mask(vol, value, sigma, spacing=None, threshold=0.5, mode='reflect'):
    return gaussian_filter((np.asarray(vol) == value).astype(np.float64), sigma, spacing=spacing, mode=mode) >= threshold


def smooth_label(vol, value, sigma, spacing=None, threshold=0.5, background=0, fill=0):
    return merge(vol, smooth_mask(vol, value, sigma, spacing, threshold), value, background, fill)


def blend_lerp(a, b, w):
    a, b, w = (np.asarray(t).astype(np.float64) for t in (a, b, w))
    return ((1.0 - w) * a) + (w * b)


def feather_blend(a, b, mask, sigma, spacing=None):
    return blend_lerp(a, b, gaussian_filter((np.asarray(mask) != 0).astype(np.float64), sigma, spacing=spacing))


# ------------------------------------------------------------------------------------------------ shared cases
SHAPES = ((5, 7, 9), (1, 6, 3), (9, 4, 11))
DTYPES = (np.float64, np.float32, np.int16, np.uint8)
SIGMA_ORDER = (((1.0, 0.7, 1.5), (0, 0, 0)), ((0.5, 2.0, 0.0), (0, 1, 0)), ((1.2, 1.2, 0.8), (2, 0, 1)))
CVAL = -7.0
GENERAL_W = np.array([0.3, -1.25, 0.5, 2.0, 0.125, 0.7, -0.4])


def volume(shape, dtype, seed=0):
    r = np.random.RandomState(seed + sum(shape))
    if np.dtype(dtype).kind == 'f':
        return (r.randn(*shape) * 100).astype(dtype)
    if np.dtype(dtype) == np.uint8:
        return r.randint(0, 256, shape).astype(np.uint8)
    return r.randint(-2000, 3000, shape).astype(np.int16)


def same(got, want):
    """Bit for bit on finite values and infinities, NaN exactly where the other has NaN."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan], want[~nan]))


def staircase(label=20, other=19, shape=(20, 18, 14)):
    """A body of `label` whose outline jumps from slice to slice along axis 2 (the slice-wise generator's staircase), with another label
    touching it -> uint8 volume."""
    v = np.zeros(shape, dtype=np.uint8)
    for k in range(2, shape[2] - 2):
        o = (0, 2, -1, 1)[k % 4]
        v[5 + o:14 + o, 4:13, k] = label
    v[2:5, 4:13, 2:shape[2] - 2] = other
    return v
