"""Per-label 3-D shape descriptors on the device (csrc/shape.hip through hv_shape).

label_statistics compares a (synthesized) vertebra's attenuation with the patient's intact ones and texture its structure; this module compares
the shape of the label itself -- what the network changes when a wedge-shaped fractured body becomes a healthy one.  It rests on the histogram
of the 256 configurations of the 2 x 2 x 2 cells of the binary lattice image (Ohser and Muecklich 2000): volume, the Crofton surface area and
both Euler numbers are linear functions of these 256 integers.  The device returns them, the coordinate moments and the extents along the 13
directions as exact integers; everything floating is numpy float64 on the host, a pure function of them.
  configurations(label, labels=None, mask=None)                             -> dict of the raw integers, [V?][S][...]
  minkowski(histogram, spacing=(1, 1, 1))                                    -> count, euler_6, euler_26, intercepts, face_area, surface_area
  direction_weights(spacing=(1, 1, 1))                                       -> the 13 Crofton weights
  shape_descriptors(label, labels=None, spacing=(1, 1, 1), mask=None)        -> dict of arrays [V?][S][...]
  vertebra_shape(label, vert_id, spacing=(1, 1, 1), largest_component=False) -> one vertebra's descriptors
  shape_comparison(label_original, label_synth, vert_id, neighbours=(), spacing=(1, 1, 1))
label and mask are what label_statistics takes (device tensors [A0][A1][A2] or stacked [V][A0][A1][A2], any strides); a numpy array is uploaded
first.  Nothing is counted on the host: a CPU tensor is a ValueError."""
import functools
import math

import numpy as np
import torch

from . import lib as _lib
from . import labelled as _lb
from .label_statistics import BAD_LABEL, EMPTY, MAX_LABELS, present  # noqa: F401  (the status bits of 'status')
from .texture import directions

REC, COUNT, SUM, SUM2, EXTENT, STATUS = 320, 256, 257, 260, 266, 292      # HV_SHAPE_* of include/hvgan.h
QUADRATURE_POINTS = 200000
SCALARS = ('voxel_volume', 'surface_area', 'face_area', 'sphericity', 'surface_volume_ratio', 'euler_6', 'euler_26', 'major_axis_length',
           'minor_axis_length', 'least_axis_length', 'elongation', 'flatness', 'max_caliper_width', 'min_caliper_width')
_PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


# ------------------------------------------------------------------------------------------------ the device half
def _launch(label, mask, labels, out):
    """Queue one hv_shape on the current stream: 4-D device tensors (mask may be None), out int64 [V][S][REC]."""
    ws, wsz = _lb.workspace('shape', label, len(labels), limit='at most 2^30 voxels per volume, 65535 volumes per call and voxels * (largest extent '
                            '- 1)^2 < 2^62')
    _lib.get().call('hv_shape', *_lb.volume_args(None, label, mask, labels), _lib.ptr(out), _lib.ptr(ws), wsz, _lib.stream())


def _present(l4, m4):
    """The non-zero label values with a counted voxel in any volume: label_statistics' count-only passes with the label as its own volume."""
    if l4.dtype in _lb.VOL_DT:
        return present(l4, l4, m4)
    vol = torch.empty((1,) + tuple(l4.shape[1:]), dtype=torch.uint8, device=l4.device).expand(l4.shape)   # never summed: the counts only
    return present(vol, l4, m4)


def _split(rec, labels):
    """The dict of configurations from the records [V][S][REC]."""
    return {'labels': np.asarray(labels, dtype=np.int64), 'histogram': rec[..., :256].copy(), 'count': rec[..., COUNT].copy(),
            'sum': rec[..., SUM:SUM + 3].copy(), 'sum2': rec[..., SUM2:SUM2 + 6].copy(),
            'extent': rec[..., EXTENT:STATUS].reshape(rec.shape[:-1] + (13, 2)).copy(), 'status': rec[..., STATUS].copy()}


def _records(label, labels, mask):
    """-> (records int64 [V][S][REC] on the host, the label list, whether the caller gave one volume): one launch sequence, one readback."""
    single, _, l4, m4 = _lb.check_inputs(None, label, mask, upload=True)
    ids = _lb.resolve_labels(labels, lambda: _present(l4, m4))
    out = torch.empty((int(l4.shape[0]), len(ids), REC), dtype=torch.int64, device=l4.device)
    _launch(l4, m4, ids, out)
    return out.cpu().numpy(), ids, single


def configurations(label, labels=None, mask=None):
    """The raw integers of every listed label value (up to 64) of `label`, restricted to mask != 0.
    -> {'labels' [S], 'histogram' int64 [V][S][256] -- the number of cells (i, j, k), i in [-1, A0 - 1] and so on (the lattice padded by one
    background layer), whose corners c + d, d in {0, 1}^3, belong to the label exactly where bit 4 d0 + 2 d1 + d2 of the code is set; every
    histogram sums to (A0 + 1)(A1 + 1)(A2 + 1) --, 'count' [V][S], 'sum' [..][3] (of p_a), 'sum2' [..][6] (of p_a p_b: 00, 01, 02, 11, 12, 22),
    'extent' [..][13][2] (min and max of d . p for the 13 texture.directions(1); no voxel: INT64_MAX, INT64_MIN), 'status' (bit 0: the volume
    holds a label that is no integer in [0, 255], bit 2: no voxel)}; one 3-D volume drops the [V].  One launch sequence and one readback.
    labels=None: the non-zero label values present, as label_statistics finds them."""
    rec, ids, single = _records(label, labels, mask)
    res = _split(rec, ids)
    return _lb.squeeze(res) if single else res


# ------------------------------------------------------------------------------------------------ the host half
@functools.lru_cache(maxsize=None)
def _config_tables():
    """Per configuration: popcount, eight times its share of either Euler number, and per direction the corner pairs (p unset, p + d set)."""
    corner = [(q >> 2 & 1, q >> 1 & 1, q & 1) for q in range(8)]
    index = {c: q for q, c in enumerate(corner)}
    edges = [(index[c], index[tuple(c[x] + (x == ax) for x in range(3))]) for c in corner for ax in range(3) if c[ax] == 0]
    faces = [[q for q, c in enumerate(corner) if c[ax] == side] for ax in range(3) for side in (0, 1)]
    dirs = [tuple(d) for d in directions(1).tolist()]
    pairs = [[(index[c], index[tuple(a + b for a, b in zip(c, d))]) for c in corner if tuple(a + b for a, b in zip(c, d)) in index] for d in dirs]
    pop, chi6, chi26 = (np.zeros(256, dtype=np.int64) for _ in range(3))
    hits = np.zeros((13, 256), dtype=np.int64)
    for code in range(256):
        bit = [code >> q & 1 for q in range(8)]
        v = sum(bit)
        e_all, e_any = sum(bit[p] and bit[q] for p, q in edges), sum(bit[p] or bit[q] for p, q in edges)
        f_all, f_any = sum(all(bit[q] for q in f) for f in faces), sum(any(bit[q] for q in f) for f in faces)
        pop[code], chi6[code], chi26[code] = v, v - 2 * e_all + 4 * f_all - (8 if code == 255 else 0), (8 if code else 0) - 4 * f_any + 2 * e_any - v
        for t in range(13):
            hits[t, code] = sum(1 for p, q in pairs[t] if not bit[p] and bit[q])
    shared = np.asarray([1 << sum(1 for c in d if c == 0) for d in dirs], dtype=np.int64)      # the cells one pair (p, p + d) lies in
    return pop, chi6, chi26, hits, shared


@functools.lru_cache(maxsize=64)
def _weights(sp):
    i = np.arange(QUADRATURE_POINTS, dtype=np.float64) + 0.5
    z = 1.0 - 2.0 * i / QUADRATURE_POINTS
    phi = i * (math.pi * (3.0 - math.sqrt(5.0)))
    r = np.sqrt(1.0 - z * z)
    P = np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)
    u = directions(1).astype(np.float64) * np.asarray(sp, dtype=np.float64)
    u /= np.sqrt((u * u).sum(axis=1))[:, None]
    w = np.bincount(np.abs(P @ u.T).argmax(axis=1), minlength=13) / float(QUADRATURE_POINTS)
    w.setflags(write=False)
    return w


def direction_weights(spacing=(1, 1, 1)):
    """The Crofton weight w_d of each of the 13 directions: the share of the sphere that lies nearest to +-(d o s) / |d o s| (the areas of the
    Voronoi cells of the 26 directions, two cells per d).  A fixed quadrature, so a pure function of the spacing: the 200 000 Fibonacci points
    z_i = 1 - 2 (i + 1/2) / N, phi_i = (i + 1/2) pi (3 - sqrt 5), P_i = (sqrt(1 - z^2) cos phi, sqrt(1 - z^2) sin phi, z), each assigned to
    the direction with the largest |P . u| (the first on a tie).  Isotropic: 0.0916, 0.0740, 0.0704 for axes, face and space diagonals (Ohser
    and Muecklich: 0.091556, 0.073961, 0.070391).  -> float64 [13], summing to 1."""
    return _weights(_lb.check_spacing(spacing)).copy()


def minkowski(histogram, spacing=(1, 1, 1)):
    """The Minkowski measures of configuration histograms [...][256] (any leading axes), numpy on the host.  With v the popcount of code c,
    e_all / e_any the cell's 12 edges with both / either end set and f_all / f_any its 6 faces with all / any corner set:
      count = sum h[c] v / 8;  euler_6 = sum h[c] (v / 8 - e_all / 4 + f_all / 2 - [c = 255]) (the foreground 6-connected);
      euler_26 = sum h[c] ([c != 0] - f_any / 2 + e_any / 4 - v / 8) (26-connected), both in integer arithmetic on eight times the number;
      intercepts[t] = sum h[c] t_d(c) / 2^z(d): the voxel pairs (p, p + d) with p outside the label and p + d inside (t_d: such corner pairs
      of the cell, z: the zero components of d -- the cells a pair lies in);
      face_area = 2 sum_axes N_axis s_b s_c, the area of the exposed voxel faces;
      surface_area = 4 sum_d w_d N_d (s0 s1 s2) / |d o s|, the Crofton estimate with direction_weights(spacing).
    -> {'count', 'euler_6', 'euler_26' int64 [...], 'intercepts' float64 [...][13], 'face_area', 'surface_area' float64 [...]}."""
    h = np.asarray(histogram)
    if h.ndim < 1 or h.shape[-1] != 256 or h.dtype.kind not in 'iu':
        raise ValueError('histogram: an integer array [...][256] expected, got %s' % (getattr(h, 'shape', None),))
    sp = np.asarray(_lb.check_spacing(spacing), dtype=np.float64)
    h = h.astype(np.int64)
    pop, chi6, chi26, hits, shared = _config_tables()
    out = {'count': (h @ pop) // 8, 'euler_6': (h @ chi6) // 8, 'euler_26': (h @ chi26) // 8}
    crossings = (h @ hits.T) // shared
    out['intercepts'] = crossings.astype(np.float64)
    d = directions(1)
    axis = [int(np.nonzero((d == e).all(axis=1))[0][0]) for e in np.eye(3, dtype=np.int64)]
    out['face_area'] = 2.0 * (crossings[..., axis[0]] * (sp[1] * sp[2]) + crossings[..., axis[1]] * (sp[0] * sp[2])
                              + crossings[..., axis[2]] * (sp[0] * sp[1]))
    length = np.sqrt(((d.astype(np.float64) * sp) ** 2).sum(axis=1))
    out['surface_area'] = 4.0 * (out['intercepts'] * (_weights(tuple(sp.tolist())) * float(np.prod(sp)) / length)).sum(axis=-1)
    return out


def descriptors_from_records(rec, labels, spacing=(1, 1, 1)):
    """The host half of shape_descriptors: records int64 [V][S][REC] -> the dict of arrays [V][S][...]."""
    rec = np.ascontiguousarray(rec, dtype=np.int64)
    sp = np.asarray(_lb.check_spacing(spacing), dtype=np.float64)
    V, S = rec.shape[:2]
    mk = minkowski(rec[..., :256], spacing)
    nan = float('nan')
    out = {'labels': np.asarray(labels, dtype=np.int64), 'count': rec[..., COUNT].copy(), 'status': rec[..., STATUS].copy(),
           'euler_6': mk['euler_6'], 'euler_26': mk['euler_26'], 'intercepts': mk['intercepts']}
    for k in SCALARS:
        if k not in out:
            out[k] = np.full((V, S), nan)
    out['centroid'], out['principal_moments'], out['caliper_widths'] = np.full((V, S, 3), nan), np.full((V, S, 3), nan), np.full((V, S, 13), nan)
    out['covariance'], out['principal_axes'] = np.full((V, S, 3, 3), nan), np.full((V, S, 3, 3), nan)
    norm = np.sqrt(((directions(1).astype(np.float64) / sp) ** 2).sum(axis=1))                # |d / s|
    cell = float(np.prod(sp))
    for v in range(V):
        for s in range(S):
            n = int(rec[v, s, COUNT])
            if n == 0:
                continue
            vol, area = n * cell, float(mk['surface_area'][v, s])
            out['voxel_volume'][v, s], out['surface_area'][v, s], out['face_area'][v, s] = vol, area, mk['face_area'][v, s]
            if area > 0:
                out['sphericity'][v, s] = (36.0 * math.pi * vol * vol) ** (1.0 / 3.0) / area
                out['surface_volume_ratio'][v, s] = area / vol
            first = [int(x) for x in rec[v, s, SUM:SUM + 3]]
            out['centroid'][v, s] = np.asarray([first[a] / n for a in range(3)]) * sp
            cov = np.zeros((3, 3))
            for m, (a, b) in enumerate(_PAIRS):                # Python integers: n * sum p_a p_b leaves int64
                cov[a, b] = cov[b, a] = (n * int(rec[v, s, SUM2 + m]) - first[a] * first[b]) / (n * n) * (sp[a] * sp[b])
            lam, vec = np.linalg.eigh(cov)
            lam, vec = np.maximum(lam[::-1], 0.0), vec[:, ::-1]
            out['covariance'][v, s], out['principal_moments'][v, s], out['principal_axes'][v, s] = cov, lam, vec.T
            out['major_axis_length'][v, s], out['minor_axis_length'][v, s], out['least_axis_length'][v, s] = (4.0 * math.sqrt(x) for x in lam)
            if lam[0] > 0:
                out['elongation'][v, s], out['flatness'][v, s] = math.sqrt(lam[1] / lam[0]), math.sqrt(lam[2] / lam[0])
            ext = rec[v, s, EXTENT:STATUS].reshape(13, 2)
            out['caliper_widths'][v, s] = (ext[:, 1] - ext[:, 0]).astype(np.float64) / norm
            out['max_caliper_width'][v, s], out['min_caliper_width'][v, s] = out['caliper_widths'][v, s].max(), out['caliper_widths'][v, s].min()
    return out


def shape_descriptors(label, labels=None, spacing=(1, 1, 1), mask=None):
    """The shape of every listed label value (up to 64) of `label`, restricted to mask != 0: a dict of numpy arrays [V][S] (one 3-D volume:
    [S]) -- labels, count, status (configurations'), voxel_volume (count * prod(spacing), mm^3), surface_area (the Crofton estimate of
    minkowski) and face_area (mm^2), sphericity (36 pi V^2)^(1/3) / S, surface_volume_ratio S / V, euler_6 and euler_26 (components - tunnels
    + cavities with the label 6- / 26-connected), intercepts [..][13], centroid [..][3] (mm), covariance [..][3][3] (mm^2, of the voxel centres,
    divided by n), principal_moments [..][3] (its eigenvalues l1 >= l2 >= l3) and principal_axes [..][3][3] (the eigenvectors as rows, sign
    free), major_ / minor_ / least_axis_length 4 sqrt(l) (pyradiomics' definition), elongation sqrt(l2 / l1), flatness sqrt(l3 / l1),
    caliper_widths [..][13] ((max - min of d . p) / |d / s|: the centre-to-centre width along the physical direction d / s, mm) and their
    max_caliper_width, min_caliper_width.  A label without a voxel, or without a surface, gives NaN where nothing is defined; nothing raises.
    One launch sequence and one readback."""
    sp = _lb.check_spacing(spacing)
    rec, ids, single = _records(label, labels, mask)
    res = descriptors_from_records(rec, ids, sp)
    return _lb.squeeze(res) if single else res


def _one(res, v, s):
    return {k: (int(res[k][s]) if k == 'labels' else res[k][v][s]) for k in res}


def vertebra_shape(label, vert_id, spacing=(1, 1, 1), largest_component=False):
    """The shape of one vertebra: shape_descriptors of label == vert_id as scalars / small arrays.  largest_component=True: of its largest
    6-connected component (components.keep_largest_component runs first; the caller's volume is not changed)."""
    sp = _lb.check_spacing(spacing)
    vid = _lb.check_labels([vert_id])[0]
    label = _lb.check_3d(_lb.resident(label), 'label', _lb.LABEL_DT)
    if largest_component:
        from . import components
        label = components.keep_largest_component(label, vid, fill=0 if vid != 0 else 255)
    rec, ids, _ = _records(label[None], [vid], None)
    return _one(descriptors_from_records(rec, ids, sp), 0, 0)


def shape_comparison(label_original, label_synth, vert_id, neighbours=(), spacing=(1, 1, 1)):
    """Does the pseudo-healthy vertebra have the shape of the patient's intact ones?  The shape of vertebra vert_id under the original label,
    under the synthesized label, and of every listed neighbour under the original label.
    -> {'original', 'synthesized': dicts as vertebra_shape's, 'neighbours': {id: dict}, 'original_ratio': {scalar: synthesized / original},
    'neighbour_ratio': {scalar: synthesized / the mean over the neighbours}} for the scalars of SCALARS (no neighbours: NaN).
    The two labels run as ONE batch (V = 2, the second volume addressed through the batch stride, no copy) when they agree in dtype and
    strides, else as two calls into one result buffer; one readback either way."""
    pair = _lb.Pair(label_original, label_synth, [vert_id] + list(neighbours), spacing=spacing)
    ids, sp = pair.ids, pair.spacing
    out = torch.empty((2, len(ids), REC), dtype=torch.int64, device=pair.device)
    pair.launch(lambda _, label, mask, sel: _launch(label, mask, ids, out[sel]))
    res = descriptors_from_records(out.cpu().numpy(), ids, sp)
    ori, syn = _one(res, 0, 0), _one(res, 1, 0)
    nb = {i: _one(res, 0, s) for s, i in enumerate(ids) if s > 0}
    nan = float('nan')

    def ratio(a, b):
        a, b = float(a), float(b)
        return a / b if b != 0 and b == b else nan

    mean = {k: (float(np.mean([float(x[k]) for x in nb.values()])) if nb else nan) for k in SCALARS}
    return {'original': ori, 'synthesized': syn, 'neighbours': nb, 'original_ratio': {k: ratio(syn[k], ori[k]) for k in SCALARS},
            'neighbour_ratio': {k: ratio(syn[k], mean[k]) for k in SCALARS}}
