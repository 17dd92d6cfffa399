"""3-D connected components on the device and the clean-up of synthesized label volumes (csrc/ccl3d.hip through hv_label3d /
hv_clean_components / hv_fill_holes).

The generator synthesizes a vertebra slice by slice, so the stacked label has no 3-D consistency: stray islands move the surface distances
(generation_eval.surface_distances), RHLV and the grader.  The reference filters components per 2-D slice only; these are the 3-D forms,
scipy.ndimage.label / binary_fill_holes bit for bit, on volumes that stay resident:
  label(vol, value=None, connectivity=1)                  -> (labels int32, table) device tensors, no synchronisation
  component_sizes(vol, value=None, connectivity=1)        -> numpy int64 sizes of the n components (one readback)
  keep_largest_component / remove_small_components / fill_holes(vol, value, ...)        -> the cleaned device volume
  clean_label(vol, value, ...)                            the filter, then optionally the hole fill, queued back to back; closing_mm /
                                                          opening_mm / spacing: morphology.open_label / close_label run first; smooth_mm:
                                                          then filters.smooth_label
  clean_labels(volumes, values, ...)                      the same for a list (the 13 crops of a patient), one readback of the tables
Volumes are 3-D with any strides, uint8 / float32 / float64 (bool masks become uint8, other dtypes float64), device tensors or numpy arrays
(uploaded).  connectivity 1 / 2 / 3 is generate_binary_structure(3, c): 6, 18 or 26 neighbours.  table: int32, [0] the number of components
n, [1] the label of the largest (equal sizes: the lowest), [2] its size, [3] status (bit 0: no foreground voxel), then the sizes."""
import ctypes

import numpy as np
import torch

from . import lib as _lib
from . import ops

_DT = {torch.uint8: 0, torch.float32: 4, torch.float64: 5}   # HV_DT_* of include/hvgan.h
_EQ, _NE = 0, 1                                              # HV_CCL_*


def _device(*vols):
    for v in vols:
        if isinstance(v, torch.Tensor) and v.is_cuda:
            return v.device
    return torch.device('cuda', torch.cuda.current_device())


def _check_volume(vol):
    """The 3-D check on the argument as given, before anything is uploaded."""
    meta = torch.as_tensor(vol)
    if meta.dim() != 3:
        raise ValueError('components: a 3-D volume expected, got shape %s' % (tuple(meta.shape),))
    return meta


def _check_connectivity(connectivity):
    if isinstance(connectivity, bool) or not isinstance(connectivity, (int, np.integer)) or not 1 <= int(connectivity) <= 3:
        raise ValueError('connectivity: 1, 2 or 3 expected (6, 18 or 26 neighbours), got %r' % (connectivity,))
    return int(connectivity)


def _check_value(value, name='value'):
    if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise ValueError('%s: a number expected, got %r' % (name, value))
    return float(value)


def _check_min_size(min_size):
    if isinstance(min_size, bool) or not isinstance(min_size, (int, np.integer)) or int(min_size) < 0 or int(min_size) > 2 ** 31 - 1:
        raise ValueError('min_size: a non-negative integer expected, got %r' % (min_size,))
    return int(min_size)


def _stored_dtype(meta):
    """The dtype the volume has on the device: bool -> uint8, anything the kernels do not read -> float64."""
    if meta.dtype == torch.bool:
        return torch.uint8
    return meta.dtype if meta.dtype in _DT else torch.float64


def _check_out(out, meta, dtype, what):
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != dtype or tuple(out.shape) != tuple(meta.shape)):
        raise ValueError('out: a %s tensor of shape %s expected' % (what, tuple(meta.shape)))


def _upload(vol, dev):
    t = torch.as_tensor(vol)
    t = t.to(_stored_dtype(t)).to(dev)
    _lib.require_gpu(t)
    return t


def _ll(strides):
    return [ctypes.c_longlong(s) for s in strides]


def _ws(L, shape, dev):
    return ops._ws(L.size('hv_label3d_workspace_bytes', *shape), dev, slot=3)


def label(vol, value=None, connectivity=1, out=None, max_components=4096):
    """Connected components of the foreground vol == value (value=None: vol != 0, scipy.ndimage.label(vol, generate_binary_structure(3,
    connectivity))).  -> (labels, table): labels a contiguous int32 device tensor of the volume's shape (`out`, if given), 0 = background,
    1..n in scipy's order; table int32 [4 + max_components] on the device, the sizes of the first max_components components from [4] on.
    Nothing is read back."""
    meta = _check_volume(vol)
    conn = _check_connectivity(connectivity)
    val = 0.0 if value is None else _check_value(value)
    if isinstance(max_components, bool) or not isinstance(max_components, (int, np.integer)) or max_components < 0:
        raise ValueError('max_components: a non-negative integer expected, got %r' % (max_components,))
    _check_out(out, meta, torch.int32, 'contiguous int32')
    if out is not None and not out.is_contiguous():
        raise ValueError('out: a contiguous int32 tensor of shape %s expected' % (tuple(meta.shape),))
    dev = _device(vol, out)
    v = _upload(vol, dev)
    _lib.require_gpu(out)
    L = _lib.get()
    A = tuple(int(s) for s in v.shape)
    if out is None:
        out = torch.empty(A, dtype=torch.int32, device=dev)
    table = torch.empty(4 + int(max_components), dtype=torch.int32, device=dev)
    ws, wsz = _ws(L, A, dev)
    L.call('hv_label3d', _lib.ptr(v), _DT[v.dtype], *_ll(v.stride()), *A, ctypes.c_double(val), _NE if value is None else _EQ, conn,
           _lib.ptr(out), _lib.ptr(table), int(max_components), _lib.ptr(ws), wsz, _lib.stream())
    return out, table


def component_sizes(vol, value=None, connectivity=1, max_components=4096):
    """The voxel counts of the components in label order, np.bincount(labels.ravel())[1:]: a numpy int64 array of length n.  One readback;
    raises ValueError if there are more than max_components components."""
    _, table = label(vol, value, connectivity, max_components=max_components)
    t = table.cpu().numpy()
    n = int(t[0])
    if n > max_components:
        raise ValueError('component_sizes: the volume has %d components, more than max_components = %d' % (n, max_components))
    return t[4:4 + n].astype(np.int64)


def _launch_clean(v, value, conn, min_size, keep_largest, fill, out, table):
    """Queue one hv_clean_components on the current stream; `table` (4 int32) is a device view written by it."""
    L = _lib.get()
    A = tuple(int(s) for s in v.shape)
    ws, wsz = _ws(L, A, v.device)
    L.call('hv_clean_components', _lib.ptr(v), _DT[v.dtype], *_ll(v.stride()), *A, ctypes.c_double(value), _EQ, conn, min_size,
           1 if keep_largest else 0, ctypes.c_double(fill), _lib.ptr(out), *_ll(out.stride()), _lib.ptr(table), _lib.ptr(ws), wsz, _lib.stream())


def _launch_fill(v, value, fill, out, table):
    """Queue one hv_fill_holes on the current stream."""
    L = _lib.get()
    A = tuple(int(s) for s in v.shape)
    ws, wsz = _ws(L, A, v.device)
    L.call('hv_fill_holes', _lib.ptr(v), _DT[v.dtype], *_ll(v.stride()), *A, ctypes.c_double(value), _EQ, ctypes.c_double(fill), _lib.ptr(out),
           *_ll(out.stride()), _lib.ptr(table), _lib.ptr(ws), wsz, _lib.stream())


def _out_for(v, out):
    """`out` as the kernels take it: the input itself (in place), a tensor that does not share its memory, or a fresh contiguous one."""
    if out is None:
        return torch.empty(tuple(v.shape), dtype=v.dtype, device=v.device)
    _lib.require_gpu(out)
    if out.data_ptr() == v.data_ptr() and out.stride() != v.stride():
        raise ValueError('out: the input itself or a tensor that does not share its memory expected')
    return out


def _prepare(vol, value, connectivity, out):
    meta = _check_volume(vol)
    conn = _check_connectivity(connectivity)
    val = _check_value(value)
    dtype = _stored_dtype(meta)
    _check_out(out, meta, dtype, str(dtype).replace('torch.', ''))
    return conn, val, dtype


def _check_morph(closing_mm, opening_mm, spacing, smooth_mm=None):
    """-> None when none of the three is given (no morphology or filter code runs), else (opening radius or None, closing radius or None,
    spacing, the Gaussian weights per axis of smooth_mm or None), checked."""
    if closing_mm is None and opening_mm is None and smooth_mm is None:
        return None
    from . import morphology as M
    smooth = None
    if smooth_mm is not None:
        from . import filters as F
        if isinstance(smooth_mm, bool) or not isinstance(smooth_mm, (int, float, np.integer, np.floating)) or not float(smooth_mm) >= 0.0:
            raise ValueError('smooth_mm: a non-negative number expected, got %r' % (smooth_mm,))
        smooth = F._gaussian_axes(float(smooth_mm), 0, 4.0, None, M._check_spacing(spacing))
    return (None if opening_mm is None else M._check_radius(opening_mm), None if closing_mm is None else M._check_radius(closing_mm),
            M._check_spacing(spacing), smooth)


def _clean(vol, value, connectivity, min_size, keep_largest, fill_holes, out, fill, table, morph=None):
    """clean_label's checks and launches; `table`: a device int32 [8] view (the filter's four words, then the hole fill's); `morph`: what
    _check_morph returned."""
    conn, val, _ = _prepare(vol, value, connectivity, out)
    ms = _check_min_size(min_size)
    fl = _check_value(fill, 'fill')
    v = _upload(vol, table.device)
    out = _out_for(v, out)
    if morph is not None:                        # the opening first (bridges), then the closing (gaps), then in place on `out`
        from . import morphology as M
        for op, radius in ((M.OPEN, morph[0]), (M.CLOSE, morph[1])):
            if radius is not None:
                v = M._label_op(op, v, val, radius, morph[2], fl, fl, out)
        if morph[3] is not None:                 # then the staircase along the slice axis is rounded
            from . import filters as F
            v = F._smooth_op(v, val, morph[3], 0.5, fl, fl, out)
    _launch_clean(v, val, conn, ms, bool(keep_largest), fl, out, table[:4])
    if fill_holes:
        _launch_fill(out, val, val, out, table[4:])
    return out


def clean_label(vol, value, connectivity=1, min_size=0, keep_largest=True, fill_holes=False, out=None, fill=0, return_table=False,
                closing_mm=None, opening_mm=None, spacing=(1, 1, 1), smooth_mm=None):
    """The 3-D clean-up of label `value` in a (synthesized) label volume: components of vol == value with fewer than min_size voxels are
    dropped (a component of exactly min_size voxels stays: the reference's rule for its 2-D filter), with keep_largest all but the largest
    one; their voxels become `fill`.  With fill_holes the cavities of what is left -- voxels from which no face of the volume is reached
    through face neighbours outside the label -- are then set to `value` (binary_fill_holes).  Every other voxel, other labels included, is
    copied.  -> the device volume (`out`: a device tensor of the volume's dtype and shape, `vol` itself for in place); return_table adds the
    device int32 [4] table of the labelling before the filter.  Nothing is read back.
    opening_mm / closing_mm (radii in the units of `spacing`, the voxel size along the three axes): before all of this, vol == value is opened
    and / or closed by that ball (morphology.open_label, then morphology.close_label, border_value 0, with `fill` as both the opening's fill
    and the background the closing may grow into): the opening cuts thin bridges to a neighbour, the closing joins fragments that a gap
    narrower than two radii separates from the body, so that keep_largest keeps them.  The table is then the labelling after them.
    smooth_mm (the sigma of a Gaussian in the units of `spacing`): after the opening / closing and before the component rules the label is
    smoothed (filters.smooth_label(..., sigma=smooth_mm, spacing=spacing, threshold=0.5, background=fill, fill=fill)), which rounds the
    staircase the slice-wise generator leaves along the slice axis.  Without it no filter code runs."""
    _prepare(vol, value, connectivity, out)
    _check_min_size(min_size)
    _check_value(fill, 'fill')
    morph = _check_morph(closing_mm, opening_mm, spacing, smooth_mm)
    table = torch.empty(8, dtype=torch.int32, device=_device(vol, out))
    out = _clean(vol, value, connectivity, min_size, keep_largest, fill_holes, out, fill, table, morph)
    return (out, table[:4]) if return_table else out


def keep_largest_component(vol, value, connectivity=1, out=None, fill=0):
    """vol with every component of vol == value but the largest set to `fill` (equal sizes: the first in raster order stays)."""
    return clean_label(vol, value, connectivity, 0, True, False, out, fill)


def remove_small_components(vol, value, min_size, connectivity=1, out=None, fill=0):
    """vol with the components of vol == value that have fewer than min_size voxels set to `fill`."""
    return clean_label(vol, value, connectivity, min_size, False, False, out, fill)


def fill_holes(vol, value, out=None, return_table=False):
    """vol with the holes of vol == value set to `value` (scipy.ndimage.binary_fill_holes: the background is 6-connected).  return_table
    adds the device int32 [4] table: [0] the number of holes, [2] the voxels filled."""
    _, val, _ = _prepare(vol, value, 1, out)
    dev = _device(vol, out)
    v = _upload(vol, dev)
    out = _out_for(v, out)
    table = torch.empty(4, dtype=torch.int32, device=dev)
    _launch_fill(v, val, val, out, table)
    return (out, table) if return_table else out


def clean_labels(volumes, values, connectivity=1, min_size=0, keep_largest=True, fill_holes=False, fill=0, closing_mm=None, opening_mm=None,
                 spacing=(1, 1, 1), smooth_mm=None):
    """clean_label for a list of volumes and their labels (one value for all, or one per volume): every call is queued on the stream, then
    the tables are read back once.  -> (the device volumes, each the bytes of the single call; numpy int32 [V][4] tables).  closing_mm /
    opening_mm / spacing / smooth_mm as for clean_label, the same for every volume."""
    volumes = list(volumes)
    if isinstance(values, (int, float, np.integer, np.floating)) and not isinstance(values, bool):
        values = [values] * len(volumes)
    values = list(values)
    if len(values) != len(volumes):
        raise ValueError('clean_labels: %d volumes but %d values' % (len(volumes), len(values)))
    for v, val in zip(volumes, values):          # every argument is checked before the first launch
        _prepare(v, val, connectivity, None)
    _check_min_size(min_size)
    _check_value(fill, 'fill')
    morph = _check_morph(closing_mm, opening_mm, spacing, smooth_mm)
    if not volumes:
        return [], np.zeros((0, 4), dtype=np.int32)
    tables = torch.empty(len(volumes), 8, dtype=torch.int32, device=_device(*volumes))
    outs = [_clean(v, val, connectivity, min_size, keep_largest, fill_holes, None, fill, tables[i], morph)
            for i, (v, val) in enumerate(zip(volumes, values))]
    return outs, tables.cpu().numpy()[:, :4]
