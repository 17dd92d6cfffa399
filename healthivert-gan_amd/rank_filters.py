"""3-D rank filters of resident volumes (csrc/rankfilt.hip through hv_rank_filter).

The slice-wise generator makes a synthesized vertebra flicker from slice to slice; a median along the slice axis or over a small ball removes
single-slice outliers without blurring cortical edges the way a Gaussian does.  The same kernel gives the local minimum / maximum and the flat
grey-scale morphology of a CT.  The definitions are scipy.ndimage's, on volumes that stay resident:
  footprint_offsets(size=None, footprint=None, origin=0)        the footprint as integer offsets from the centre          (host, no device)
  percentile_rank(n, percentile)                                scipy's rank of a percentile in a window of n             (host, no device)
  ball(radius_mm, spacing=(1, 1, 1))                            the offsets of morphology.ball                            (host, no device)
  dilation_arguments(size=None, footprint=None, origin=0)       the maximum filter scipy's grey_dilation runs             (host, no device)
  rank_filter(vol, rank, size=None, footprint=None, mode='reflect', cval=0.0, origin=0)
  median_filter / percentile_filter / minimum_filter / maximum_filter           the same arguments as scipy's
  grey_erosion / grey_dilation / grey_opening / grey_closing                    flat footprints only
  median_ct(vol, radius_mm=None, size=None, spacing=None, mode='nearest')       the median over a ball given in mm, or over a box
  deflicker(vol, size=3, axis=2, mode='nearest')                                the median along the slice axis only
Volumes are 3-D device tensors with any strides (a permuted view or a sub-box passes as it lies: nothing is copied), uint8 / int16 / float32 /
float64; bool becomes uint8, numpy arrays are uploaded, any other dtype is refused.  Results have the input's dtype, as scipy's do, and are
scipy's values exactly: selection needs no arithmetic.  Nothing is read back.

A footprint reaches at most 4 voxels from its centre along each axis (9 x 9 x 9 cells with origin 0).  cval must be a value of the volume's
dtype (scipy compares another cval as a double and truncates it on output; that form is not offered).  A window that holds a NaN gets the
answer of the key order -- NaNs sort at the two ends by their sign bit -- which need not be scipy's; other windows are not affected."""
import ctypes
import math
import warnings

import numpy as np
import torch

from . import lib as _lib
from .components import _check_value, _check_volume, _device, _ll
from .filters import _overlaps

_DT = {torch.uint8: 0, torch.int16: 1, torch.float32: 4, torch.float64: 5}      # HV_DT_* of include/hvgan.h
MODES = {'reflect': 0, 'constant': 1, 'nearest': 2, 'mirror': 3, 'wrap': 4}      # HV_FILT_*
REACH = 4                                                                        # HV_RANK_REACH


# ------------------------------------------------------------------------------------------------ host: footprints and ranks
def _per_axis(v, name):
    v = tuple(v) if np.ndim(v) else (v,) * 3
    if len(v) != 3 or any(isinstance(x, bool) or not isinstance(x, (int, np.integer)) for x in v):
        raise ValueError('%s: an integer or one integer per axis expected, got %r' % (name, v))
    return tuple(int(x) for x in v)


def _footprint_array(size, footprint):
    if footprint is None:
        if size is None:
            raise RuntimeError('no footprint or filter size provided')
        sizes = _per_axis(size, 'size')
        if min(sizes) < 1:
            raise ValueError('size: positive integers expected, got %r' % (size,))
        return np.ones(sizes, dtype=bool)
    if size is not None:
        warnings.warn('ignoring size because footprint is set', UserWarning, stacklevel=3)
    fp = np.asarray(footprint, dtype=bool)
    if fp.ndim != 3 or 0 in fp.shape:
        raise RuntimeError('footprint: a non-empty 3-D array expected, got shape %s' % (fp.shape,))
    if not fp.any():
        raise ValueError('All-zero footprint is not supported.')
    return fp


def _offsets_of(fp, origin):
    """The cells of the bool array fp as offsets from the centre shape // 2 + origin, in the C order of the cells -> int array [n][3]."""
    org = _per_axis(origin, 'origin')
    centre = [s // 2 + o for s, o in zip(fp.shape, org)]
    if any(c < 0 or c >= s for c, s in zip(centre, fp.shape)):
        raise ValueError('invalid origin')
    off = np.argwhere(fp) - np.array(centre)
    if np.abs(off).max() > REACH:
        raise ValueError('footprint: offsets of at most %d voxels from the centre are supported, got %d (shape %s, origin %s)'
                         % (REACH, int(np.abs(off).max()), fp.shape, org))
    return off.astype(np.int64)


def footprint_offsets(size=None, footprint=None, origin=0):
    """The footprint of scipy.ndimage's rank filters as offsets from the window's centre, int array [n][3]: cell j of the footprint reads the
    input at p + j - (shape // 2 + origin) per axis.  Even extents are legal; a footprint wins over size (scipy warns and ignores size).
    ValueError for an origin that puts the centre outside the footprint (scipy refuses it as well) and for an offset beyond +-4."""
    return _offsets_of(_footprint_array(size, footprint), origin)


def percentile_rank(n, percentile):
    """scipy.ndimage.percentile_filter's rank in a window of n: a negative percentile counts from 100, 100 is the maximum."""
    p = percentile
    if p < 0.0:
        p += 100.0
    if p < 0 or p > 100:
        raise RuntimeError('invalid percentile')
    return n - 1 if p == 100.0 else int(float(n) * p / 100.0)


def ball(radius_mm, spacing=(1, 1, 1)):
    """The offsets of hv_morph_ball's structuring element (morphology.ball: ((s0 o0)^2 + (s1 o1)^2) + (s2 o2)^2 <= radius * radius, float64
    in this order), int array [n][3]."""
    from .morphology import ball as _ball
    b = _ball(radius_mm, spacing)
    return _offsets_of(b, 0)


def dilation_arguments(size=None, footprint=None, origin=0):
    """(footprint, origin) of the maximum filter that scipy.ndimage.grey_dilation(size=, footprint=, origin=) runs: the footprint reversed
    along every axis (None with size= alone), the origin negated and, along an axis of even extent, shifted by -1."""
    if size is None and footprint is None:
        raise ValueError('size or footprint must be given (structure= is not offered)')
    org = list(_per_axis(origin, 'origin'))
    if footprint is not None:
        footprint = np.asarray(footprint, dtype=bool)
        if footprint.ndim != 3:
            raise RuntimeError('footprint: a 3-D array expected, got shape %s' % (footprint.shape,))
        shape = footprint.shape
        footprint = footprint[::-1, ::-1, ::-1]
    else:
        shape = _per_axis(size, 'size')
    for a in range(3):
        org[a] = -org[a]
        if not shape[a] & 1:
            org[a] -= 1
    return footprint, tuple(org)


def _rank_of(rank, n):
    if isinstance(rank, bool) or not isinstance(rank, (int, np.integer)):
        raise ValueError('rank: an integer expected, got %r' % (rank,))
    r = int(rank) + n if rank < 0 else int(rank)
    if r < 0 or r >= n:
        raise RuntimeError('rank not within filter footprint size')
    return r


# ------------------------------------------------------------------------------------------------ the launch
def _check_mode(mode, cval, dtype):
    if mode not in MODES:
        raise ValueError('mode: one of %s expected, got %r' % (', '.join(MODES), mode))
    c = _check_value(cval, 'cval')
    ok = math.isfinite(c)
    if ok and dtype in (torch.uint8, torch.int16):
        lo, hi = (0, 255) if dtype == torch.uint8 else (-32768, 32767)
        ok = c == math.floor(c) and lo <= c <= hi
    elif ok and dtype == torch.float32:
        ok = abs(c) <= float(np.finfo(np.float32).max) and float(np.float32(c)) == c
    if not ok:
        raise ValueError('cval: a finite value of the volume\'s dtype (%s) expected, got %r' % (str(dtype).replace('torch.', ''), cval))
    return MODES[mode], c


def _upload(vol, dev):
    t = torch.as_tensor(vol)
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    if t.dtype not in _DT:
        raise TypeError('rank_filters: a uint8 / int16 / float32 / float64 (or bool) volume expected, got %s' % (t.dtype,))
    t = t.to(dev)
    _lib.require_gpu(t)
    return t


def _check_out(out, v):
    if out is None:
        return torch.empty(tuple(v.shape), dtype=v.dtype, device=v.device)
    if not isinstance(out, torch.Tensor) or out.dtype != v.dtype or tuple(out.shape) != tuple(v.shape):
        raise ValueError('out: a %s tensor of shape %s expected' % (str(v.dtype).replace('torch.', ''), tuple(v.shape)))
    _lib.require_gpu(out)
    return out


def _launch(v, offsets, rank, mode, cval, out=None):
    """Queue one hv_rank_filter on the current stream: the rank-th smallest over `offsets` ([n][3]) of the device tensor v -> out."""
    L = _lib.get()
    out = _check_out(out, v)
    fp = L.hv_rank_footprint()
    words = [0] * len(fp.bits)
    for o0, o1, o2 in np.asarray(offsets).tolist():
        b = ((o0 + REACH) * 9 + (o1 + REACH)) * 9 + (o2 + REACH)
        words[b // 64] |= 1 << (b % 64)
    for i, w in enumerate(words):
        fp.bits[i] = w
    fp.n = sum(bin(w).count('1') for w in words)
    if fp.n != len(offsets):
        raise ValueError('footprint: distinct offsets expected')
    if _overlaps(v, out):
        raise ValueError('out: a tensor that does not share the input\'s memory expected')
    L.call('hv_rank_filter', _lib.ptr(v), _DT[v.dtype], *_ll(v.stride()), *(int(s) for s in v.shape), ctypes.byref(fp), int(rank), mode,
           ctypes.c_double(cval), _lib.ptr(out), *_ll(out.stride()), _lib.stream())
    return out


def _prepare(vol, mode, cval, out=None):
    _check_volume(vol)
    v = _upload(vol, _device(vol, out))
    m, c = _check_mode(mode, cval, v.dtype)
    return v, m, c


# ------------------------------------------------------------------------------------------------ scipy's rank filters
def rank_filter(vol, rank, size=None, footprint=None, mode='reflect', cval=0.0, origin=0, out=None):
    """scipy.ndimage.rank_filter(vol, rank, size, footprint, mode=mode, cval=cval, origin=origin) as a device volume of the input's dtype.
    A negative rank counts from the end (-1: the maximum)."""
    off = footprint_offsets(size, footprint, origin)
    v, m, c = _prepare(vol, mode, cval, out)
    return _launch(v, off, _rank_of(rank, len(off)), m, c, out)


def median_filter(vol, size=None, footprint=None, mode='reflect', cval=0.0, origin=0, out=None):
    """scipy.ndimage.median_filter: rank n // 2 of the n cells of the footprint."""
    off = footprint_offsets(size, footprint, origin)
    v, m, c = _prepare(vol, mode, cval, out)
    return _launch(v, off, len(off) // 2, m, c, out)


def percentile_filter(vol, percentile, size=None, footprint=None, mode='reflect', cval=0.0, origin=0, out=None):
    """scipy.ndimage.percentile_filter: rank percentile_rank(n, percentile); a negative percentile counts from 100."""
    off = footprint_offsets(size, footprint, origin)
    v, m, c = _prepare(vol, mode, cval, out)
    return _launch(v, off, percentile_rank(len(off), percentile), m, c, out)


def _min_or_max(vol, size, footprint, mode, cval, origin, maximum, out=None):
    """scipy's _min_or_max_filter without `structure`.  A box given by size= runs as one launch per axis of extent above 1 with a line
    footprint, as scipy decomposes it (the values are those of the 3-D footprint); intermediates are tensors of the input's dtype."""
    v, m, c = _prepare(vol, mode, cval, out)
    if footprint is not None:
        off = footprint_offsets(size, footprint, origin)
        return _launch(v, off, len(off) - 1 if maximum else 0, m, c, out)
    off = footprint_offsets(size, None, origin)                  # the checks of the whole box
    lo, hi = off.min(axis=0), off.max(axis=0)
    axes = [a for a in range(3) if hi[a] > lo[a]] or [2]         # (a 1 x 1 x 1 box: one launch with one tap, the copy)
    cur = v
    for i, a in enumerate(axes):
        line = np.zeros((hi[a] - lo[a] + 1, 3), dtype=np.int64)
        line[:, a] = np.arange(lo[a], hi[a] + 1)
        cur = _launch(cur, line, len(line) - 1 if maximum else 0, m, c, out if i == len(axes) - 1 else None)
    return cur


def minimum_filter(vol, size=None, footprint=None, mode='reflect', cval=0.0, origin=0, out=None):
    """scipy.ndimage.minimum_filter; with size= and no footprint it runs separably, one launch per axis."""
    return _min_or_max(vol, size, footprint, mode, cval, origin, False, out)


def maximum_filter(vol, size=None, footprint=None, mode='reflect', cval=0.0, origin=0, out=None):
    """scipy.ndimage.maximum_filter; with size= and no footprint it runs separably, one launch per axis."""
    return _min_or_max(vol, size, footprint, mode, cval, origin, True, out)


# ------------------------------------------------------------------------------------------------ flat grey-scale morphology
def grey_erosion(vol, size=None, footprint=None, mode='reflect', cval=0.0, origin=0, out=None):
    """scipy.ndimage.grey_erosion with a flat footprint: the minimum filter.  `structure=` (a non-flat structuring element) is not offered."""
    if size is None and footprint is None:
        raise ValueError('size or footprint must be given (structure= is not offered)')
    return _min_or_max(vol, size, footprint, mode, cval, origin, False, out)


def grey_dilation(vol, size=None, footprint=None, mode='reflect', cval=0.0, origin=0, out=None):
    """scipy.ndimage.grey_dilation with a flat footprint: the maximum filter over the REVERSED footprint with the origin negated and, along an
    axis of even extent, shifted by -1, as scipy does.  `structure=` is not offered."""
    footprint, origin = dilation_arguments(size, footprint, origin)
    return _min_or_max(vol, size, footprint, mode, cval, origin, True, out)


def grey_opening(vol, size=None, footprint=None, mode='reflect', cval=0.0, origin=0, out=None):
    """scipy.ndimage.grey_opening with a flat footprint: grey_dilation(grey_erosion(vol)).  `structure=` is not offered."""
    return grey_dilation(grey_erosion(vol, size, footprint, mode, cval, origin), size, footprint, mode, cval, origin, out)


def grey_closing(vol, size=None, footprint=None, mode='reflect', cval=0.0, origin=0, out=None):
    """scipy.ndimage.grey_closing with a flat footprint: grey_erosion(grey_dilation(vol)).  `structure=` is not offered."""
    return grey_erosion(grey_dilation(vol, size, footprint, mode, cval, origin), size, footprint, mode, cval, origin, out)


# ------------------------------------------------------------------------------------------------ what the pipeline gets
def median_ct(vol, radius_mm=None, size=None, spacing=None, mode='nearest', out=None):
    """The median of a CT over ball(radius_mm, spacing) -- a ball in mm on the scan's voxel grid (spacing None: unit voxels) -- or, with
    size=, over a box of voxels.  Exactly one of radius_mm and size is given."""
    if (radius_mm is None) == (size is None):
        raise ValueError('median_ct: exactly one of radius_mm and size expected')
    off = ball(radius_mm, (1, 1, 1) if spacing is None else spacing) if size is None else footprint_offsets(size)
    v, m, c = _prepare(vol, mode, 0.0, out)
    return _launch(v, off, len(off) // 2, m, c, out)


def deflicker(vol, size=3, axis=2, mode='nearest', out=None):
    """The median over `size` voxels along the slice axis only: a single-slice outlier of the slice-wise generator goes, in-plane edges stay."""
    if isinstance(axis, bool) or not isinstance(axis, (int, np.integer)) or not -3 <= int(axis) < 3:
        raise ValueError('axis: an integer in [-3, 3) expected, got %r' % (axis,))
    if isinstance(size, bool) or not isinstance(size, (int, np.integer)) or size < 1:
        raise ValueError('size: a positive integer expected, got %r' % (size,))
    sizes = [1, 1, 1]
    sizes[int(axis) % 3] = int(size)
    return median_filter(vol, size=tuple(sizes), mode=mode, out=out)
