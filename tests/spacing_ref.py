"""Reference helpers for scans with anisotropic voxel spacing (fixture G21, tools/make_golden_spacing.py): the loader, the host plan of a
case, and restore_ref's point-by-point local coordinates with a spacing.  No device."""
import json
import os
import warnings

import numpy as np

import restore_ref as R

ROOT = R.ROOT
PLANE = (128, 128)

# Largest |hvgan.straighten host restatement - reference| over G21, as tools/make_golden_spacing.py prints them (tests/test_spacing_cpu.py
# measures them again): knots, basis, local centroids, the local coordinate of every box voxel, local_to_global on the lattice.  All 0: both
# sides are numpy float64 and multiply / divide by the spacing at the same places in the same order (curve * spacing before the knots,
# point * spacing before the knot offsets, the interpolated millimetres / spacing last), so no operation's order differs.
MEASURED = {'knots': 0.0, 'basis': 0.0, 'local centroid': 0.0, 'box local': 0.0, 'lattice global': 0.0}
# The device tolerance follows tests/test_restore_gpu.py's rule: ten times the measured figure, floor 1e-12 (the device sums the frame
# products in its own loop, not einsum's).  Local coordinates are millimetres (up to a few hundred); local_to_global results are voxel
# indices, the millimetres divided by a spacing >= 0.5, so the same absolute figure holds a rounding error of the quotient (<= 2^-53 * 200).
LOCAL_TOL = max(10 * max(MEASURED['box local'], MEASURED['local centroid']), 1e-12)
GLOBAL_TOL = max(10 * MEASURED['lattice global'], 1e-12)
MARGIN_DELTA = R.MARGIN_DELTA
MARGIN_CAP = R.MARGIN_CAP
# Counts below MARGIN_DELTA over the fixture, as the tool prints them: label samples of the crops within it of a half-integer, box voxels
# with a decision margin under it, lattice points with |to_plane| under it.
RISKY = {'label samples': 0, 'box voxels': 0, 'lattice points': 0}


def make_patient(kw, swap):
    from hvgan import synth
    ct, label = synth.make_spine_patient(**kw)
    if swap:
        ct, label = np.ascontiguousarray(ct.transpose(2, 1, 0)), np.ascontiguousarray(label.transpose(2, 1, 0))
    return ct, label


def load_g21():
    """-> {case: {'spacing' (3 floats), 'ids', 'out_size', 'centroid_list', 'window', 'crop_ct', 'crop_label', 'boxes', 'ct', 'label' (the
    synthetic patient, rebuilt from the recorded arguments) and, with a curve: 'curve', 'knots', 'basis', 'local', 'crop_risky' {vid: mask},
    'covered_volume' {vid: mask}, 'region' {vid: box}, 'box' {'vid', 'region', 'local', 'covered', 'sample_ct', 'sample_label', 'margin',
    'margin_label'}, 'lattice' {'local', 'global', 'round', 'margin', 'round_margin'}}}."""
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'g21_spacing.npz'))
    cases = {}
    for k in z.files:
        parts = k.split('/')
        d = cases.setdefault(parts[0], {})
        if len(parts) == 3:
            d.setdefault(parts[1], {})[int(parts[2]) if parts[2].isdigit() else parts[2]] = z[k]
        else:
            d[parts[1]] = z[k]
    for c in cases.values():
        kw = json.loads(str(c.pop('kwargs')))
        kw = {k: tuple(v) if isinstance(v, list) else v for k, v in kw.items()}
        c['ct'], c['label'] = make_patient(kw, bool(c.pop('swap02')))
        c['spacing'] = tuple(float(v) for v in c['spacing'])
        c['ids'] = [int(v) for v in c['ids']]
        c['out_size'] = tuple(int(v) for v in c['out_size'])
        c['centroid_list'] = [{'label': int(r[0]), 'X': float(r[1]), 'Y': float(r[2]), 'Z': float(r[3])} for r in c['centroids']]
        if 'box' in c:
            c['box']['vid'] = int(c['box']['vid'])
    return cases


def plan_of(c, spacing=None):
    """The host plan of a G21 case as straighten_patient(..., return_plan=True, spacing=...) returns it."""
    from hvgan import straighten as S
    sp = c['spacing'] if spacing is None else spacing
    p = S.plan(c['centroid_list'], c['ct'].shape, c['ids'], c['out_size'], spacing=sp)
    knots, basis, local, boxes = p
    return {'centroids': c['centroid_list'], 'knots': knots, 'basis': basis, 'local': local, 'boxes': boxes, 'window': bool(c['window']),
            'spacing': p.spacing}


def local_coords(knots, basis, region, spacing, plane=PLANE):
    """straighten.global_to_local at `spacing` for every voxel of the box -> [nx, ny, nz, 3] (restore_ref.local_coords with a spacing)."""
    from hvgan import straighten as S
    pts = R.box_points(region)
    out = np.empty_like(pts)
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        for i in np.ndindex(*pts.shape[:3]):
            out[i] = S.global_to_local(pts[i], knots, basis, plane, spacing)
    return out
