"""Golden vectors G21 for straightening and restoring scans with anisotropic voxel spacing, generated
by running the reference's own code on synthetic patients with ONE change: the Interpolator that process_mask3d builds
(straighten_mask_3d.py:505) gets spacing=<the case's spacing> (a subclass injects the keyword; the bundled library models it,
straighten/straighten/curve.py:26-52,160-195).  location_json_local.process_directory writes the centroid JSON and process_mask3d cuts the
crops exactly as in tools/make_golden_straighten.py (import and def statements only, stand-in modules for what is never called); that
Interpolator then answers global_to_local for EVERY voxel of the patient volume (as tools/make_golden_restore.py does for G20) and
local_to_global on a lattice of local points that spans the crops and passes both curve ends.

Per case: centroids, curve, knots, basis, local centroids, crops; per crop voxel whether its label sample coordinate lies within
restore_ref.MARGIN_DELTA of a half-integer (`crop_risky`); for the first requested vertebra the patient-space box (straighten.restore_box),
the reference's local coordinate of each of its voxels, the coverage of the box and of the whole volume, scipy's samples of the crop there
and the decision margins of tools/make_golden_restore.py; the lattice, the reference's local_to_global on it, its margin, and the
reference's global_to_local of those results (its own round trip).  The patients are rebuilt from the recorded synth arguments.

While generating it prints the largest |host restatement (hvgan.straighten) - reference| per quantity and the counts of samples / voxels
below the margin; tests/spacing_ref.py records them as constants.

    python tools/make_golden_spacing.py [--ref PATH_TO_REFERENCE]
writes tests/golden/g21_spacing.npz.
"""
import argparse
import io
import json
import os
import sys
import tempfile
import warnings
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANE = (128, 128)

CASES = [  # name, kwargs of synth.make_spine_patient, axes 0 and 2 swapped, spacing (mm per voxel), requested ids, out_size
    ('aniso', dict(seed=1), False, (0.7, 0.7, 1.5), [17, 18], (20, 10, 6)),        # coarse along the spine (axis 2): more knots than slices
    # the spine along axis 0 (the patient transposed), which is the coarse one: 96 rows become some 190 knots, pure upsampling
    ('thick', dict(seed=2), True, (2.5, 0.9, 0.9), [17, 18], (20, 10, 6)),
    # 24 x 32 x 48 mm of scan under a 128 mm plane: most of it samples outside; the crop's axis-0 range is clipped at the curve's start
    ('fine', dict(seed=5), False, (0.5, 0.5, 0.5), [17], (24, 4, 4)),
    ('edge', dict(seed=4, shape=(44, 56, 72), n_vert=6, margin=2, curve=(4.0, 8.0)), False, (0.8, 1.25, 1.0), [17, 20], (16, 8, 6)),
    ('single', dict(seed=3, shape=(40, 48, 56), n_vert=3, radius=(10, 9, 6)), False, (0.7, 0.7, 1.5), [17], (16, 20, 12)),
]


def make_patient(kw, swap):
    from hvgan import synth
    ct, label = synth.make_spine_patient(**kw)
    if swap:
        ct, label = np.ascontiguousarray(ct.transpose(2, 1, 0)), np.ascontiguousarray(label.transpose(2, 1, 0))
    return ct, label


def lattice_points(length):
    """Local points (cumulative length, along frame vector 1, along frame vector 2): 12 stations from 6 mm before the curve's start to 6 mm
    past its end, 4 x 4 offsets around the plane centre."""
    l0 = np.linspace(-6.37, length + 6.37, 12)
    l1 = PLANE[0] / 2 + np.array([-8.0, -2.5, 3.25, 9.0])
    l2 = PLANE[1] / 2 + np.array([-9.0, -3.25, 2.5, 8.0])
    return np.stack(np.meshgrid(l0, l1, l2, indexing='ij'), -1).reshape(-1, 3)


def global_margin(points, cum):
    """Decision margin of local_to_global: to_plane[n] = point[0] - cumlen[n], so the plane choice turns on min |to_plane|."""
    return np.abs(points[:, 0][:, None] - cum[None, :]).min(1)


def save_npz(path, arrs):
    """np.savez_compressed with a fixed member date, so that a second run writes the same bytes (numpy stamps the members with the time)."""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for k, v in arrs.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', default='/root/reference')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden'))
    args = ap.parse_args()
    sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')]
    import hvgan  # noqa: F401
    from hvgan import straighten as S
    from scipy.ndimage import map_coordinates
    import make_golden_straighten as g13
    import make_golden_restore as g20
    import restore_ref as R
    store = {}
    g13._stub_modules(store)
    sys.path.insert(0, os.path.join(args.ref, 'straighten'))
    loc = g13._load_defs(os.path.join(args.ref, 'straighten', 'location_json_local.py'), 'ref_location_json_local')
    smk = g13._load_defs(os.path.join(args.ref, 'straighten', 'straighten_mask_3d.py'), 'ref_straighten_mask_3d')
    smk.extract_mask_volume = lambda vol, label: np.zeros((1, 1, 1), np.uint8)
    record, current = {}, {}

    class SpacingInterpolator(smk.Interpolator):           # the one change: spacing= handed to the library
        def __init__(self, curve, *a, **kw):
            kw['spacing'] = current['spacing']
            super().__init__(curve, *a, **kw)
            record['curve'], record['inter'] = np.array(curve), self

        def global_to_local(self, points, shape):
            r = super().global_to_local(points, shape)
            if np.ndim(points) == 1:
                record.setdefault('local', []).append(np.asarray(r, dtype=np.float64))
            return r
    smk.Interpolator = SpacingInterpolator

    def run_reference(tmp, name, ct, label, ids, out_size, spacing):
        record.clear()
        current['spacing'] = spacing
        pdir = os.path.join(tmp, name, 'data', name)
        os.makedirs(pdir, exist_ok=True)
        ct_path, seg_path = os.path.join(pdir, name + '.nii.gz'), os.path.join(pdir, name + '_seg.nii.gz')
        for p in (ct_path, seg_path):
            open(p, 'wb').close()
        store[ct_path], store[seg_path] = ct, label
        loc.process_directory(os.path.dirname(pdir))
        json_path = os.path.join(pdir, name + '.json')
        cents = json.load(open(json_path))
        out_dir = os.path.join(tmp, 'out', name)
        smk.process_mask3d(ct_path, seg_path, json_path, ids, out_dir, out_size)
        crops_ct = np.stack([store[os.path.join(out_dir, 'CT', '%s_%d.nii.gz' % (name, v))] for v in ids])
        crops_lab = np.stack([store[os.path.join(out_dir, 'label', '%s_%d.nii.gz' % (name, v))] for v in ids])
        assert crops_ct.dtype == np.float64 and np.all(crops_lab == np.round(crops_lab)) and crops_lab.max() <= 255
        return cents, crops_ct, crops_lab.astype(np.uint8)

    arrs = {}
    worst = {'knots': 0.0, 'basis': 0.0, 'local centroid': 0.0, 'box local': 0.0, 'lattice global': 0.0}
    risky = {'label samples': 0, 'label samples total': 0, 'box voxels': 0, 'box voxels total': 0, 'lattice points': 0}
    with tempfile.TemporaryDirectory() as tmp:
        for name, kw, swap, spacing, ids, out_size in CASES:
            ct, label = make_patient(kw, swap)
            assert ct.size <= 48 * 64 * 96
            cents, crops_ct, crops_lab = run_reference(tmp, name, ct, label, ids, out_size, spacing)
            arrs[name + '/kwargs'] = np.array(json.dumps(kw))
            arrs[name + '/swap02'] = np.array(swap)
            arrs[name + '/spacing'] = np.array(spacing, dtype=np.float64)
            arrs[name + '/ids'] = np.array(ids, dtype=np.int64)
            arrs[name + '/out_size'] = np.array(out_size, dtype=np.int64)
            arrs[name + '/centroids'] = np.array([[e['label'], e['X'], e['Y'], e['Z']] for e in cents], dtype=np.float64)
            arrs[name + '/window'] = np.array(not (ct.max() < 800 and ct.min() > -300))
            arrs[name + '/crop_ct'] = crops_ct
            arrs[name + '/crop_label'] = crops_lab
            plan = S.plan(cents, ct.shape, ids, out_size, spacing=spacing)
            knots, basis, local_c, boxes = plan
            arrs[name + '/boxes'] = np.array(boxes, dtype=np.int64)
            if 'inter' not in record:           # one centroid: the raw volume is cropped and the spacing ignored
                assert knots is None
                unit = run_reference(tmp, name + '_unit', ct, label, ids, out_size, (1.0, 1.0, 1.0))
                assert np.array_equal(unit[1], crops_ct) and np.array_equal(unit[2], crops_lab)
                print(name, 'single centroid: the crops equal the unit-spacing crops')
                store.clear()
                continue
            inter = record['inter']
            ref_local_c = np.stack(record['local'])
            arrs[name + '/curve'] = record['curve']
            arrs[name + '/knots'] = inter.knots
            arrs[name + '/basis'] = inter.basis
            arrs[name + '/local'] = ref_local_c
            worst['knots'] = max(worst['knots'], float(np.abs(knots - inter.knots).max()))
            worst['basis'] = max(worst['basis'], float(np.abs(basis - inter.basis).max()))
            worst['local centroid'] = max(worst['local centroid'], float(np.abs(np.stack([local_c[v] for v in ids]) - ref_local_c).max()))
            # label samples of the straightening near a half-integer, carried into each crop's layout
            grid = np.moveaxis(inter.get_grid(PLANE), 0, -1)                       # [N][PA][PB][3] voxel coordinates
            inside = ((grid >= 0) & (grid <= np.array(ct.shape) - 1)).all(-1)
            near = inside & (np.abs(grid - np.floor(grid) - 0.5).min(-1) < R.MARGIN_DELTA)
            for k, box in enumerate(boxes):
                lo, n, st = box[0:3], box[3:6], box[6:9]
                cr = np.zeros(out_size, dtype=bool)
                cr[st[0]:st[0] + n[0], st[1]:st[1] + n[1], st[2]:st[2] + n[2]] = near[lo[0]:lo[0] + n[0], lo[1]:lo[1] + n[1], lo[2]:lo[2] + n[2]]
                arrs['%s/crop_risky/%d' % (name, ids[k])] = cr
                risky['label samples'] += int(cr.sum())
                risky['label samples total'] += cr.size
                assert cr.mean() <= R.MARGIN_CAP, (name, ids[k])
            # the way back: the reference, point by point, for EVERY voxel of the patient volume
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                whole = np.asarray(inter.global_to_local(R.box_points([0, 0, 0] + list(ct.shape)), PLANE), dtype=np.float64)
            vid, box = ids[0], boxes[0]
            for k, (v, bx) in enumerate(zip(ids, boxes)):            # what restore_box has to contain, for every vertebra
                region = S.restore_box(knots, basis, bx, ct.shape, spacing=spacing)
                covered_volume = R.crop_coords(whole, bx)[1]
                arrs['%s/covered_volume/%d' % (name, v)] = covered_volume
                arrs['%s/region/%d' % (name, v)] = np.array(region, dtype=np.int64)
                sl = tuple(slice(region[i], region[i] + region[3 + i]) for i in range(3))
                outside = covered_volume.copy()
                outside[sl] = False
                print(name, v, 'box', bx, 'region', region, 'covered in the volume', int(covered_volume.sum()), 'outside restore_box', int(outside.sum()))
            region = S.restore_box(knots, basis, box, ct.shape, spacing=spacing)
            sl = tuple(slice(region[i], region[i] + region[3 + i]) for i in range(3))
            pts = R.box_points(region)
            local = whole[sl]
            c, covered = R.crop_coords(local, box)
            margin = np.empty(pts.shape[:3])
            host = np.empty_like(local)
            seen = {'none': 0, 'several': 0, 'clipped': 0}
            with warnings.catch_warnings(), np.errstate(all='ignore'):
                warnings.simplefilter('ignore')
                for i in np.ndindex(*pts.shape[:3]):
                    idx, ncand, margin[i] = g20.decision_terms(pts[i] * np.array(spacing), inter.knots, inter.basis)
                    seen['none'] += ncand == 0
                    seen['several'] += ncand > 1
                    seen['clipped'] += idx < 2
                    host[i] = S.global_to_local(pts[i], knots, basis, PLANE, spacing)
            fin = np.isfinite(local).all(-1)
            assert np.array_equal(fin, np.isfinite(host).all(-1))
            worst['box local'] = max(worst['box local'], float(np.abs(host - local)[fin].max()))
            lo_b = np.array(box[6:9], dtype=np.float64)
            hi_b = lo_b + np.array(box[3:6]) - 1
            with np.errstate(invalid='ignore'):
                bound = np.minimum(np.abs(c - lo_b), np.abs(c - hi_b)).min(-1)
                half = np.abs(c - np.floor(c) - 0.5).min(-1)
            margin = np.where(fin, np.minimum(margin, np.where(fin, bound, 0.0)), 0.0)
            margin_label = np.where(fin, np.minimum(margin, np.where(fin, half, 0.0)), 0.0)
            s_ct = np.zeros(pts.shape[:3])
            s_lab = np.zeros(pts.shape[:3], dtype=np.uint8)
            s_ct[covered] = map_coordinates(crops_ct[0], c[covered].T, order=1)
            s_lab[covered] = map_coordinates(crops_lab[0], c[covered].T, order=0)
            low = margin_label < R.MARGIN_DELTA
            risky['box voxels'] += int(low.sum())
            risky['box voxels total'] += low.size
            assert low.mean() <= R.MARGIN_CAP and covered.any(), (name, vid, float(low.mean()))
            tag = '%s/box/' % name
            arrs[tag + 'vid'] = np.array(vid)
            arrs[tag + 'region'] = np.array(region, dtype=np.int64)
            arrs[tag + 'local'] = local
            arrs[tag + 'covered'] = covered
            arrs[tag + 'sample_ct'] = s_ct
            arrs[tag + 'sample_label'] = s_lab
            arrs[tag + 'margin'] = margin.astype(np.float32)
            arrs[tag + 'margin_label'] = margin_label.astype(np.float32)
            # local -> global on the lattice, and the reference's own way back from there
            cum = S.cumulative_length(inter.knots)
            lat = lattice_points(cum[-1])
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                lat_global = np.asarray(inter.local_to_global(lat, PLANE), dtype=np.float64)
                lat_round = np.asarray(inter.global_to_local(lat_global, PLANE), dtype=np.float64)
                host_g = S.local_to_global(lat, knots, basis, PLANE, spacing)
            assert np.isfinite(lat_global).all()
            worst['lattice global'] = max(worst['lattice global'], float(np.abs(host_g - lat_global).max()))
            lat_margin = global_margin(lat, cum)
            lat_round_margin = np.array([g20.decision_terms(p * np.array(spacing), inter.knots, inter.basis)[2] for p in lat_global])
            risky['lattice points'] += int((lat_margin < R.MARGIN_DELTA).sum())
            arrs[name + '/lattice/local'] = lat
            arrs[name + '/lattice/global'] = lat_global
            arrs[name + '/lattice/round'] = lat_round
            arrs[name + '/lattice/margin'] = lat_margin.astype(np.float32)
            arrs[name + '/lattice/round_margin'] = lat_round_margin.astype(np.float32)
            print(name, 'shape', ct.shape, 'spacing', spacing, 'knots', len(knots), 'box voxels', low.size, 'covered', int(covered.sum()), seen,
                  'lattice', len(lat), 'past the ends', int(((lat[:, 0] < 0) | (lat[:, 0] > cum[-1])).sum()))
            store.clear()
    for k, v in worst.items():
        print('largest |host restatement - reference| %s: %.3g' % (k, v))
    print('below MARGIN_DELTA:', risky)
    path = os.path.join(args.out, 'g21_spacing.npz')
    save_npz(path, arrs)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
