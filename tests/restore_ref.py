"""Numpy float64 restatement of hvgan.straighten.restore_patient (csrc/restore.hip): straighten.global_to_local point by point (the
restatement of the reference's Interpolator.global_to_local, curve.py:104-150,223-239, pinned to it by tests/test_straighten_cpu.py and
by fixture G20), the coverage test, scipy.ndimage.map_coordinates orders 1 / 0 on the crop, and both write rules.  No device."""
import json
import os
import warnings

import numpy as np
from scipy.ndimage import map_coordinates

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Largest |restore_ref local - the reference's recorded local| over every box voxel of G20, measured on the host: 0 (both are numpy float64
# and run the same einsum, norm and interpolation arithmetic).  The device gets ten times that with the project's figure for the host curve
# math (1e-12, tests/test_straighten_cpu.py) as the floor; the floor it is.  It sums the frame products in its own loop, not einsum's.
LOCAL_MEASURED = 0.0
LOCAL_TOL = max(10 * LOCAL_MEASURED, 1e-12)
MARGIN_DELTA = 100 * LOCAL_TOL        # voxels whose decision margin (tools/make_golden_restore.py) is below this are left out ...
MARGIN_CAP = 0.01                     # ... and at most this share of a box may be


def box_points(region):
    """[nx, ny, nz, 3] float64: the voxel indices of the patient-space box region = [x0, y0, z0, nx, ny, nz]."""
    x0, y0, z0, nx, ny, nz = region
    g = np.meshgrid(np.arange(x0, x0 + nx), np.arange(y0, y0 + ny), np.arange(z0, z0 + nz), indexing='ij')
    return np.stack(g, -1).astype(np.float64)


def local_coords(knots, basis, region, plane=(128, 128)):
    """straighten.global_to_local for every voxel of the box -> [nx, ny, nz, 3] (non-finite where the window holds a duplicate to_plane)."""
    from hvgan import straighten as S
    pts = box_points(region)
    out = np.empty_like(pts)
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        for i in np.ndindex(*pts.shape[:3]):
            out[i] = S.global_to_local(pts[i], knots, basis, plane)
    return out


def crop_coords(local, box):
    """Local coordinates -> crop coordinates and the coverage mask.  The straight volume [N][PA][PB] is indexed (n, a, b) with a along frame
    vector 2 and b along frame vector 1 (Interpolator.get_grid's meshgrid), local coordinates are (length, along vector 1, along vector 2):
    the in-plane pair swaps.  c = straight - lo + start; covered iff start <= c <= start + n - 1 on all axes and local is finite."""
    lo, n, st = (np.array(box[i:i + 3], dtype=np.float64) for i in (0, 3, 6))
    c = (local[..., [0, 2, 1]] - lo) + st
    with np.errstate(invalid='ignore'):
        covered = np.isfinite(local).all(-1) & (c >= st).all(-1) & (c <= st + n - 1).all(-1)
    return c, covered


def base_volumes(plan, shape, ct=None, label=None):
    if ct is None:
        ct_out = np.zeros(shape, dtype=np.float64)
    else:
        ct_out = np.asarray(ct, dtype=np.float64).copy()
        if plan['window']:
            ct_out = np.clip(255.0 * (ct_out - (-300.0)) / (800.0 - (-300.0)), 0.0, 255.0)
    lab_out = np.zeros(shape, dtype=np.uint8) if label is None else np.asarray(label).astype(np.uint8)
    return ct_out, lab_out


def restore(plan, crops, shape, ct=None, label=None, where='vertebra', local=None):
    """-> (ct_out float64, label_out uint8, covered uint8) as restore_patient(..., return_covered=True) defines them.  crops: {vert_id:
    (ct_vol, label_vol)} numpy arrays, applied in the dict's order.  local: {vert_id: [nx, ny, nz, 3]} to reuse coordinates already
    computed for the vertebra's restore_box (the fixture's, or an earlier call's)."""
    from hvgan import straighten as S
    knots, basis = plan['knots'], plan['basis']
    ct_out, lab_out = base_volumes(plan, shape, ct, label)
    covered_out = np.zeros(shape, dtype=np.uint8)
    src_shape = tuple(shape) if knots is None else (len(knots), 128, 128)
    for vid, (cvol, lvol) in crops.items():
        box = S.crop_box(plan['local'][vid], src_shape, cvol.shape)
        region = S.restore_box(knots, basis, box, shape)
        if min(region[3:]) <= 0:
            continue
        sl = tuple(slice(region[i], region[i] + region[3 + i]) for i in range(3))
        if knots is None:
            loc = box_points(region)
            c = (loc - np.array(box[0:3], dtype=np.float64)) + np.array(box[6:9], dtype=np.float64)
            cov = np.ones(loc.shape[:3], dtype=bool)
        else:
            loc = local[vid] if local is not None and vid in local else local_coords(knots, basis, region)
            c, cov = crop_coords(loc, box)
        s_ct = np.zeros(cov.shape)
        s_lab = np.zeros(cov.shape, dtype=np.uint8)
        s_ct[cov] = map_coordinates(np.asarray(cvol, dtype=np.float64), c[cov].T, order=1)
        s_lab[cov] = map_coordinates(np.asarray(lvol), c[cov].T, order=0)
        write = cov
        if where == 'vertebra':
            write = cov & ((s_lab == vid) | (np.asarray(label)[sl] == vid))
        ct_out[sl][write] = s_ct[write]
        lab_out[sl][write] = s_lab[write]
        covered_out[sl][write] = 1
    return ct_out, lab_out, covered_out


def load_g20():
    """-> {case: {'ids', 'out_size', 'centroids', 'window', 'crop_ct', 'crop_label', 'knots', 'basis', 'boxes', 'ct', 'label' (the synthetic
    patient, rebuilt from the recorded arguments), vert_id: {'region', 'local', 'covered', 'covered_volume' (whole patient volume), 'sample_ct', 'sample_label', 'margin',
    'margin_label'}, 'probe' (some cases): {'region', 'local', 'margin'}}}."""
    from hvgan import synth
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'g20_restore.npz'))
    cases = {}
    for k in z.files:
        parts = k.split('/')
        d = cases.setdefault(parts[0], {})
        if len(parts) == 3:
            d.setdefault(parts[1] if parts[1] == 'probe' else int(parts[1]), {})[parts[2]] = z[k]
        else:
            d[parts[1]] = z[k]
    for c in cases.values():
        kw = json.loads(str(c.pop('kwargs')))
        kw = {k: tuple(v) if isinstance(v, list) else v for k, v in kw.items()}
        c['ct'], c['label'] = synth.make_spine_patient(**kw)
        c['ids'] = [int(v) for v in c['ids']]
        c['out_size'] = tuple(int(v) for v in c['out_size'])
        c['centroid_list'] = [{'label': int(r[0]), 'X': float(r[1]), 'Y': float(r[2]), 'Z': float(r[3])} for r in c['centroids']]
    return cases


def plan_of(c):
    """The host plan of a G20 case as straighten_patient(..., return_plan=True) returns it."""
    from hvgan import straighten as S
    knots, basis, local, boxes = S.plan(c['centroid_list'], c['ct'].shape, c['ids'], c['out_size'])
    return {'centroids': c['centroid_list'], 'knots': knots, 'basis': basis, 'local': local, 'boxes': boxes, 'window': bool(c['window'])}
