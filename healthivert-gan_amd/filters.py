"""Separable linear filtering of resident volumes (csrc/filter3d.hip through hv_separable_filter / hv_blend_lerp).

The slice-wise generator leaves a label as a staircase along the slice axis, which closing, opening and the component rules cannot round; the
remedy is a Gaussian of the label's indicator thresholded at one half.  The same kernel smooths the synthesized CT (along the slice axis only:
sigma = (0, 0, s)) and gives the blurred mask a seamless composite of a restored vertebra needs.  The definitions are scipy.ndimage's, for
odd-length weights and origin 0, on volumes that stay resident:
  gaussian_kernel1d(sigma, order, radius)                         scipy's Gaussian (derivative) weights, float64 on the host
  correlate1d(vol, weights, axis=-1, mode='reflect', cval=0.0)    -> float64 device volume
  gaussian_filter1d(vol, sigma, axis=-1, order=0, ...)            -> float64 device volume
  gaussian_filter(vol, sigma, order=0, mode='reflect', cval=0.0, truncate=4.0, radius=None, spacing=None)
  smooth_label(vol, value, sigma, spacing=None, threshold=0.5, background=0, fill=0)
                                                                  gaussian_filter(vol == value) >= threshold written back into the label volume
  feather_blend(a, b, mask, sigma, spacing=None)                  ((1 - w) * a) + (w * b) with w = gaussian_filter(mask != 0)
Volumes are 3-D device tensors with any strides (a permuted view or a sub-box passes as it lies: nothing is copied), uint8 / int16 / float32 /
float64; bool becomes uint8, other dtypes float64, numpy arrays are uploaded.  mode is one of reflect / constant / nearest / mirror / wrap,
the same for every axis.  Nothing is read back.

The float32 rule: every result is scipy's on the FLOAT64 COPY of the input, bit for bit on finite values (NaN where scipy has NaN), and is
returned as float64.  scipy itself answers a float32 input with float32 and rounds to float32 between the axes; compare with
scipy.ndimage.gaussian_filter(vol.astype(np.float64), ...).  The arithmetic is float64 in scipy's order of summation (symmetric, antisymmetric
or general, chosen by scipy's test on the weights), without fma."""
import ctypes
import math

import numpy as np
import torch

from . import lib as _lib
from . import ops
from .components import _check_value, _check_volume, _device, _ll, _out_for
from .components import _DT as _LABEL_DT
from .components import _upload as _upload_label

_DT = {torch.uint8: 0, torch.int16: 1, torch.float32: 4, torch.float64: 5}      # HV_DT_* of include/hvgan.h
_BLEND_DT = {torch.int16: 1, torch.float32: 4, torch.float64: 5}
IN_VALUE, IN_EQ = 0, 1                                                           # HV_FILT_IN_*
MODES = {'reflect': 0, 'constant': 1, 'nearest': 2, 'mirror': 3, 'wrap': 4}      # HV_FILT_*
MAX_RADIUS = 64                                                                  # HV_FILT_MAX_RADIUS
_EPS = float(np.finfo(np.float64).eps)


def gaussian_kernel1d(sigma, order, radius):
    """scipy.ndimage's _gaussian_kernel1d: the weights of a Gaussian (order 0) or of its order-th derivative on -radius .. radius, float64."""
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
    D = np.diag(exponent_range[1:], 1)               # D @ q(x) = q'(x)
    P = np.diag(np.ones(order) / -sigma2, -1)        # P @ q(x) = q(x) * p'(x)
    Q_deriv = D + P
    for _ in range(order):
        q = Q_deriv.dot(q)
    q = (x[:, None] ** exponent_range).dot(q)
    return q * phi_x


def weights_form(weights):
    """How scipy sums these weights: +1 symmetric, -1 antisymmetric, 0 general (its test against DBL_EPSILON)."""
    w = np.asarray(weights, dtype=np.float64)
    r = len(w) // 2
    if all(abs(w[r + i] - w[r - i]) <= _EPS for i in range(1, r + 1)):
        return 1
    if all(abs(w[r + i] + w[r - i]) <= _EPS for i in range(1, r + 1)):
        return -1
    return 0


def _check_weights(weights):
    w = np.array(weights, dtype=np.float64)
    if w.ndim != 1 or len(w) < 1 or len(w) % 2 != 1:
        raise ValueError('weights: a 1-D sequence of odd length expected (even lengths and origin are not offered), got shape %s' % (w.shape,))
    if len(w) // 2 > MAX_RADIUS:
        raise ValueError('weights: at most %d taps (radius %d) are supported, got %d' % (2 * MAX_RADIUS + 1, MAX_RADIUS, len(w)))
    if not np.isfinite(w).all():
        raise ValueError('weights: finite numbers expected')
    return w


def _check_mode(mode, cval):
    if mode not in MODES:
        raise ValueError('mode: one of %s expected, got %r' % (', '.join(MODES), mode))
    c = _check_value(cval, 'cval')
    if not math.isfinite(c):
        raise ValueError('cval: a finite number expected, got %r' % (cval,))
    return MODES[mode], c


def _check_axis(axis):
    if isinstance(axis, bool) or not isinstance(axis, (int, np.integer)) or not -3 <= int(axis) < 3:
        raise ValueError('axis: an integer in [-3, 3) expected, got %r' % (axis,))
    return int(axis) % 3


def _per_axis(v, name):
    v = tuple(v) if np.ndim(v) else (v,) * 3
    if len(v) != 3:
        raise ValueError('%s: a scalar or one value per axis expected, got %r' % (name, v))
    return v


def _check_spacing(spacing):
    from .morphology import _check_spacing as check
    return None if spacing is None else check(spacing)


def _gaussian_axes(sigma, order, truncate, radius, spacing):
    """The per-axis weights (None: the axis is skipped, as scipy skips sigma <= 1e-15) of gaussian_filter, reversed as gaussian_filter1d
    hands them to correlate1d."""
    sig, orders, radii = _per_axis(sigma, 'sigma'), _per_axis(order, 'order'), _per_axis(radius, 'radius')
    sp = _check_spacing(spacing)
    out = []
    for a in range(3):
        s = float(sig[a]) if sp is None else float(sig[a]) / sp[a]
        if not math.isfinite(s) or s < 0.0:
            raise ValueError('sigma: non-negative finite numbers expected, got %r' % (sigma,))
        o = orders[a]
        if isinstance(o, bool) or not isinstance(o, (int, np.integer)) or o < 0:
            raise ValueError('order: non-negative integers expected, got %r' % (order,))
        if not s > 1e-15:
            out.append(None)
            continue
        lw = int(float(truncate) * s + 0.5)
        if radii[a] is not None:
            lw = radii[a]
            if isinstance(lw, bool) or not isinstance(lw, (int, np.integer)) or lw < 0:
                raise ValueError('radius: non-negative integers expected, got %r' % (radius,))
        if lw > MAX_RADIUS:
            raise ValueError('sigma %g voxels at truncate %g needs a radius of %d, above the %d the kernels take'
                             % (s, float(truncate), lw, MAX_RADIUS))
        out.append(_check_weights(gaussian_kernel1d(s, int(o), int(lw))[::-1]))
    return out


def _stored(meta):
    if meta.dtype == torch.bool:
        return torch.uint8
    return meta.dtype if meta.dtype in _DT else torch.float64


def _upload(vol, dev):
    t = torch.as_tensor(vol)
    t = t.to(_stored(t)).to(dev)
    _lib.require_gpu(t)
    return t


def _overlaps(x, y):
    def span(t):
        lo = hi = 0
        for n, s in zip(t.shape, t.stride()):
            lo, hi = lo + min(0, (n - 1) * s), hi + max(0, (n - 1) * s)
        e = t.element_size()
        return t.data_ptr() + lo * e, t.data_ptr() + (hi + 1) * e
    (a0, a1), (b0, b1) = span(x), span(y)
    return a0 < b1 and b0 < a1


def _launch(v, axes, mode, cval, out, in_eq=None, threshold=0.0):
    """Queue one hv_separable_filter on the current stream: v filtered by `axes` (three weight arrays or None) into `out`, float64 for the
    doubles or uint8 for the mask >= threshold; in_eq: filter the indicator v == in_eq."""
    L = _lib.get()
    A = tuple(int(s) for s in v.shape)
    desc = (L.hv_filter_axis * 3)()
    for a, w in enumerate(axes):
        if w is None:
            desc[a].radius = -1
            continue
        desc[a].radius, desc[a].form = len(w) // 2, weights_form(w)
        for i, x in enumerate(w):
            desc[a].w[i] = float(x)
    if _overlaps(v, out):
        raise ValueError('out: a tensor that does not share the input\'s memory expected')
    ws, wsz = ops._ws(L.size('hv_filter_workspace_bytes', *A, desc), v.device, slot=3)
    L.call('hv_separable_filter', _lib.ptr(v), _DT[v.dtype], *_ll(v.stride()), *A, IN_VALUE if in_eq is None else IN_EQ,
           ctypes.c_double(0.0 if in_eq is None else in_eq), desc, mode, ctypes.c_double(cval), _lib.ptr(out),
           _DT[out.dtype], ctypes.c_double(threshold), *_ll(out.stride()), _lib.ptr(ws), wsz, _lib.stream())
    return out


def _f64_out(out, v):
    if out is None:
        return torch.empty(tuple(v.shape), dtype=torch.float64, device=v.device)
    if not isinstance(out, torch.Tensor) or out.dtype != torch.float64 or tuple(out.shape) != tuple(v.shape):
        raise ValueError('out: a float64 tensor of shape %s expected' % (tuple(v.shape),))
    _lib.require_gpu(out)
    return out


def correlate1d(vol, weights, axis=-1, mode='reflect', cval=0.0, out=None, origin=0):
    """scipy.ndimage.correlate1d(vol.astype(float64), weights, axis, mode=mode, cval=cval) as a float64 device volume (`out`, if given).
    weights: odd length, at most 129; origin is not offered (anything but 0 raises ValueError)."""
    _check_volume(vol)
    if origin != 0:
        raise ValueError('origin is not offered: the weights are centred (origin=0)')
    w = _check_weights(weights)
    ax = _check_axis(axis)
    m, c = _check_mode(mode, cval)
    v = _upload(vol, _device(vol, out))
    return _launch(v, [w if a == ax else None for a in range(3)], m, c, _f64_out(out, v))


def gaussian_filter1d(vol, sigma, axis=-1, order=0, mode='reflect', cval=0.0, truncate=4.0, radius=None, out=None):
    """scipy.ndimage.gaussian_filter1d of the float64 copy: radius int(truncate * sigma + 0.5) unless given, order-th derivative."""
    _check_volume(vol)
    ax = _check_axis(axis)
    m, c = _check_mode(mode, cval)
    if not float(sigma) > 0.0:
        raise ValueError('sigma: a positive number expected, got %r' % (sigma,))
    axes = _gaussian_axes([sigma if a == ax else 0.0 for a in range(3)], order, truncate, radius, None)
    if axes[ax] is None:                          # scipy skips nothing here: a tiny sigma is a one-tap filter
        lw = int(float(truncate) * float(sigma) + 0.5) if radius is None else int(radius)
        axes[ax] = _check_weights(gaussian_kernel1d(float(sigma), int(order), lw)[::-1])
    v = _upload(vol, _device(vol, out))
    return _launch(v, axes, m, c, _f64_out(out, v))


def gaussian_filter(vol, sigma, order=0, mode='reflect', cval=0.0, truncate=4.0, radius=None, spacing=None, out=None):
    """scipy.ndimage.gaussian_filter(vol.astype(float64), sigma, order, mode=mode, cval=cval, truncate=truncate, radius=radius) as a float64
    device volume.  sigma, order and radius are scalars or one per axis; an axis whose sigma is <= 1e-15 is skipped, with all three skipped the
    result is the float64 copy.  spacing (the voxel size along the three axes): sigma is in its units, sigma_vox = sigma / spacing[a].  order 1 /
    2 / ... per axis gives the derivative-of-Gaussian filters."""
    _check_volume(vol)
    m, c = _check_mode(mode, cval)
    axes = _gaussian_axes(sigma, order, truncate, radius, spacing)
    v = _upload(vol, _device(vol, out))
    return _launch(v, axes, m, c, _f64_out(out, v))


def _check_threshold(threshold):
    t = _check_value(threshold, 'threshold')
    if math.isnan(t):
        raise ValueError('threshold: a number expected, got %r' % (threshold,))
    return t


def smooth_mask(vol, value, sigma, spacing=None, threshold=0.5, mode='reflect', out=None):
    """gaussian_filter(vol == value, sigma, spacing=spacing, mode=mode) >= threshold as a uint8 device mask (0 / 1).  Neither the indicator nor
    the doubles of the last axis are stored."""
    _check_volume(vol)
    val = _check_value(value)
    thr = _check_threshold(threshold)
    m, c = _check_mode(mode, 0.0)
    axes = _gaussian_axes(sigma, 0, 4.0, None, spacing)
    v = _upload(vol, _device(vol, out))
    if out is None:
        out = torch.empty(tuple(v.shape), dtype=torch.uint8, device=v.device)
    elif not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != tuple(v.shape):
        raise ValueError('out: a uint8 tensor of shape %s expected' % (tuple(v.shape),))
    return _launch(v, axes, m, c, out, in_eq=val, threshold=thr)


def _smooth_op(v, val, axes, threshold, background, fill, out):
    """The smoothed mask of v == val merged into `out` (v itself: in place): first the voxels it gains (only where v holds `background`),
    then the voxels it loses (`fill`).  v and out are device tensors of a label dtype; everything is queued on the current stream."""
    from .morphology import GROW, SHRINK
    mask = torch.empty(tuple(v.shape), dtype=torch.uint8, device=v.device)
    _launch(v, axes, MODES['reflect'], 0.0, mask, in_eq=val, threshold=threshold)
    A = tuple(int(s) for s in v.shape)
    L = _lib.get()
    for src, rule in ((v, GROW), (out, SHRINK)):
        L.call('hv_morph_merge', _lib.ptr(src), _LABEL_DT[src.dtype], *_ll(src.stride()), *A, _lib.ptr(mask), *_ll(mask.stride()), rule,
               ctypes.c_double(val), ctypes.c_double(background), ctypes.c_double(fill), _lib.ptr(out), *_ll(out.stride()), _lib.stream())
    return out


def smooth_label(vol, value, sigma, spacing=None, threshold=0.5, background=0, fill=0, out=None):
    """Label `value` of a label volume smoothed: the mask gaussian_filter(vol == value, sigma, spacing=spacing) >= threshold (mode reflect)
    is written back with hv_morph_merge's rules, so other labels are never overwritten -- a voxel the mask gains becomes `value` only where the
    volume holds `background`, a voxel of `value` the mask loses becomes `fill`, every other voxel is copied.  The volume is a label volume
    as components.py takes it (uint8 / float32 / float64; other dtypes are uploaded as float64).  -> the device volume in the volume's dtype
    (`out`: a device tensor of that dtype and shape, `vol` itself for in place)."""
    meta = _check_volume(vol)
    val, bg, fl = _check_value(value), _check_value(background, 'background'), _check_value(fill, 'fill')
    thr = _check_threshold(threshold)
    axes = _gaussian_axes(sigma, 0, 4.0, None, spacing)
    v = _upload_label(vol, _device(vol, out))
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != v.dtype or tuple(out.shape) != tuple(meta.shape)):
        raise ValueError('out: a %s tensor of shape %s expected' % (str(v.dtype).replace('torch.', ''), tuple(meta.shape)))
    return _smooth_op(v, val, axes, thr, bg, fl, _out_for(v, out))


def blend_lerp(a, b, w, out=None):
    """((1 - w) * a) + (w * b) in float64, in this order, as a float64 device volume.  a, b: int16 / float32 / float64, w: float64, or uint8 /
    bool as a mask (non-zero = 1); all of one shape, each with its own strides.  `out` may be `a` (float64)."""
    shape = tuple(_check_volume(a).shape)
    dev = _device(a, b, w, out)

    def up(t, name, table):
        t = torch.as_tensor(t)
        if tuple(t.shape) != shape:
            raise ValueError('%s: shape %s expected, got %s' % (name, shape, tuple(t.shape)))
        if t.dtype == torch.bool:
            t = t.to(torch.uint8)
        t = t.to(t.dtype if t.dtype in table else torch.float64).to(dev)
        _lib.require_gpu(t)
        return t
    a, b = up(a, 'a', _BLEND_DT), up(b, 'b', _BLEND_DT)
    w = up(w, 'w', {torch.uint8: 0, torch.float64: 5})
    out = _f64_out(out, a)
    _lib.get().call('hv_blend_lerp', _lib.ptr(a), _BLEND_DT[a.dtype], *_ll(a.stride()), _lib.ptr(b), _BLEND_DT[b.dtype], *_ll(b.stride()),
                    _lib.ptr(w), _DT[w.dtype], *_ll(w.stride()), *shape, _lib.ptr(out), *_ll(out.stride()), _lib.stream())
    return out


def feather_blend(a, b, mask, sigma, spacing=None, value=None, out=None):
    """The composite of b into a with a feathered seam: w = gaussian_filter(mask != 0, sigma, spacing=spacing) (mode reflect) -- with `value`,
    of the indicator mask == value, which is then never materialised -- and ((1 - w) * a) + (w * b) in float64.  With a the patient CT, b the
    HV_RESTORE_CROP result of straighten.restore_patient and mask, value the restored label and vert_id, this is restore_patient's write
    without its hard edge.  -> float64 device volume (`out` may be `a`)."""
    meta = _check_volume(mask)
    val = None if value is None else _check_value(value)
    axes = _gaussian_axes(sigma, 0, 4.0, None, spacing)
    if tuple(torch.as_tensor(a).shape) != tuple(meta.shape):
        raise ValueError('mask: shape %s expected, got %s' % (tuple(torch.as_tensor(a).shape), tuple(meta.shape)))
    dev = _device(a, b, mask, out)
    m = _upload(mask, dev)
    if val is None and meta.dtype != torch.bool:
        m = (m != 0).view(torch.uint8)               # (a bool mask is its own indicator; any other is compared once)
    w = torch.empty(tuple(m.shape), dtype=torch.float64, device=dev)
    _launch(m, axes, MODES['reflect'], 0.0, w, in_eq=val)
    return blend_lerp(a, b, w, out)
