"""Host side of straightening and restoring scans with anisotropic voxel spacing (hvgan.straighten: curve_frame, global_to_local,
local_to_global, plan, restore_box with spacing=, the argument checks) against fixture G21 (tools/make_golden_spacing.py: the reference's
own process_mask3d with spacing= handed to its Interpolator, its global_to_local for every voxel of the patient and its local_to_global on
a lattice), and against G13 / G20 at unit spacing.  No device: these run everywhere."""
import os
import warnings

import numpy as np
import pytest
import torch

import restore_ref as R
import spacing_ref as SR

_CACHE = {}
CURVED = ('aniso', 'thick', 'fine', 'edge')


def _g():
    if 'g' not in _CACHE:
        import hvgan  # noqa: F401
        _CACHE['g'] = SR.load_g21()
    return _CACHE['g']


def _plan(name):
    if ('plan', name) not in _CACHE:
        _CACHE['plan', name] = SR.plan_of(_g()[name])
    return _CACHE['plan', name]


def test_fixture_holds_the_cases_and_the_margin_cap():
    g = _g()
    assert set(g) == set(CURVED) | {'single'}
    assert g['aniso']['spacing'] == (0.7, 0.7, 1.5) and g['thick']['spacing'] == (2.5, 0.9, 0.9) and g['fine']['spacing'] == (0.5, 0.5, 0.5)
    assert g['edge']['spacing'] == (0.8, 1.25, 1.0) and g['single']['spacing'] != (1.0, 1.0, 1.0)
    assert len(g['aniso']['ids']) == 2 and len(g['single']['centroids']) == 1 and 'knots' not in g['single']
    for name in CURVED:
        c = g[name]
        assert c['ct'].size <= 48 * 64 * 96
        b = c['box']
        assert b['local'].shape == tuple(b['region'][3:]) + (3,) and b['covered'].any()
        assert (b['margin_label'] < SR.MARGIN_DELTA).mean() <= SR.MARGIN_CAP and (b['margin'] < SR.MARGIN_DELTA).mean() <= SR.MARGIN_CAP
        for vid in c['ids']:
            assert c['crop_risky'][vid].mean() <= SR.MARGIN_CAP
        lat = c['lattice']
        L = np.linalg.norm(np.diff(c['knots'], axis=0), axis=1).sum()
        assert 100 <= len(lat['local']) <= 1000 and (lat['local'][:, 0] < 0).any() and (lat['local'][:, 0] > L).any()
    # thick: more knots than rows along the curve's axis (pure upsampling); aniso the same along axis 2
    assert len(g['thick']['knots']) > g['thick']['ct'].shape[0] and len(g['aniso']['knots']) > g['aniso']['ct'].shape[2]
    # fine: the crop's axis-0 range is clipped at the curve's start, and the plane is wider than the scan
    assert g['fine']['boxes'][0][0] == 0 and g['fine']['boxes'][0][6] > 0
    assert max(s * d for s, d in zip(g['fine']['spacing'], g['fine']['ct'].shape[:2])) < 128
    # edge: the extension clamped at a volume end
    curve, shape = g['edge']['curve'], g['edge']['ct'].shape
    assert curve[0][2] == 0.0 or curve[-1][2] == shape[2]
    assert SR.LOCAL_TOL == max(10 * max(SR.MEASURED['box local'], SR.MEASURED['local centroid']), 1e-12)
    assert SR.GLOBAL_TOL == max(10 * SR.MEASURED['lattice global'], 1e-12)


def test_host_restatement_against_the_reference_and_the_recorded_figures():
    """knots, basis, local centroids, boxes, the box's local coordinates and local_to_global on the lattice: the largest differences are the
    constants the device tolerances are derived from."""
    from hvgan import straighten as S
    worst = dict.fromkeys(SR.MEASURED, 0.0)
    risky = dict.fromkeys(SR.RISKY, 0)
    for name in CURVED:
        c, plan = _g()[name], _plan(name)
        coords = np.array([[e['X'], e['Y'], e['Z']] for e in c['centroid_list']])
        curve = S.extend_curve(coords, 20, (0, 0, 0), c['ct'].shape)              # voxel indices, before the Interpolator converts
        assert np.array_equal(curve, c['curve']), name
        knots, basis = S.curve_frame(curve, 1, c['spacing'])
        assert np.array_equal(knots, plan['knots']) and np.array_equal(basis, plan['basis'])
        worst['knots'] = max(worst['knots'], np.abs(knots - c['knots']).max())
        worst['basis'] = max(worst['basis'], np.abs(basis - c['basis']).max())
        worst['local centroid'] = max(worst['local centroid'], np.abs(np.stack([plan['local'][v] for v in c['ids']]) - c['local']).max())
        assert np.array_equal(np.array(plan['boxes']), c['boxes']), name
        b = c['box']
        region = S.restore_box(plan['knots'], plan['basis'], plan['boxes'][0], c['ct'].shape, spacing=c['spacing'])
        assert region == [int(v) for v in b['region']], name
        got = SR.local_coords(plan['knots'], plan['basis'], region, c['spacing'])
        fin = np.isfinite(b['local']).all(-1)
        assert np.array_equal(fin, np.isfinite(got).all(-1)), name
        worst['box local'] = max(worst['box local'], np.abs(got - b['local'])[fin].max())
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            glob = S.local_to_global(c['lattice']['local'], plan['knots'], plan['basis'], SR.PLANE, c['spacing'])
            one = S.local_to_global(c['lattice']['local'][7], plan['knots'], plan['basis'], SR.PLANE, c['spacing'])
        assert glob.shape == c['lattice']['global'].shape and np.array_equal(one, glob[7])
        worst['lattice global'] = max(worst['lattice global'], np.abs(glob - c['lattice']['global']).max())
        risky['label samples'] += sum(int(c['crop_risky'][v].sum()) for v in c['ids'])
        risky['box voxels'] += int((b['margin_label'] < SR.MARGIN_DELTA).sum())
        risky['lattice points'] += int((c['lattice']['margin'] < SR.MARGIN_DELTA).sum())
    for k, v in worst.items():
        print('largest |host restatement - reference| %s over G21: %.3g' % (k, v))
        assert v <= SR.MEASURED[k], (k, v)
    print('below MARGIN_DELTA over G21:', risky)
    assert risky == SR.RISKY


def test_single_centroid_ignores_the_spacing():
    from hvgan import straighten as S
    c = _g()['single']
    a = S.plan(c['centroid_list'], c['ct'].shape, c['ids'], c['out_size'], spacing=c['spacing'])
    b = S.plan(c['centroid_list'], c['ct'].shape, c['ids'], c['out_size'])
    assert a[0] is None and a[1] is None and a[3] == b[3] == [[int(v) for v in r] for r in c['boxes']]
    assert a.spacing == c['spacing'] and b.spacing == (1.0, 1.0, 1.0)
    box = a[3][0]
    assert S.restore_box(None, None, box, c['ct'].shape, spacing=c['spacing']) == S.restore_box(None, None, box, c['ct'].shape)
    # the reference's crops at this spacing are its unit-spacing crops: the filled part is the raw (windowed) volume's box
    lo, n, st = box[0:3], box[3:6], box[6:9]
    lab = c['crop_label'][0][st[0]:st[0] + n[0], st[1]:st[1] + n[1], st[2]:st[2] + n[2]]
    raw = c['label'][lo[0]:lo[0] + n[0], lo[1]:lo[1] + n[1], lo[2]:lo[2] + n[2]]
    assert (lab == raw)[lab != 0].all() and (lab != 0).any()


def test_unit_spacing_reproduces_g13_and_g20_exactly():
    from hvgan import straighten as S
    g13 = np.load(os.path.join(SR.ROOT, 'tests', 'golden', 'g13_straighten.npz'))
    for n in ('curved', 'bypass', 'edge'):
        cents = [{'label': int(r[0]), 'X': float(r[1]), 'Y': float(r[2]), 'Z': float(r[3])} for r in g13[n + '/centroids']]
        ids, out_size = [int(v) for v in g13[n + '/ids']], tuple(int(v) for v in g13[n + '/out_size'])
        a = S.plan(cents, g13[n + '/ct'].shape, ids, out_size)
        for sp in ((1.0, 1.0, 1.0), 1, 1.0, np.float64(1.0), [1, 1, 1]):
            b = S.plan(cents, g13[n + '/ct'].shape, ids, out_size, spacing=sp)
            assert b.spacing == (1.0, 1.0, 1.0)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[3] == b[3]
            assert all(np.array_equal(a[2][v], b[2][v]) for v in ids)
        k, bs = S.curve_frame(g13[n + '/curve'], 1)
        assert np.array_equal(k, a[0]) and np.array_equal(bs, a[1])
        assert np.abs(a[0] - g13[n + '/knots']).max() <= 1e-12 and np.abs(a[1] - g13[n + '/basis']).max() <= 1e-12
    g20 = R.load_g20()
    for name, c in g20.items():
        plan = R.plan_of(c)
        for vid, box in zip(c['ids'], plan['boxes']):
            v = c[vid]
            assert S.restore_box(plan['knots'], plan['basis'], box, c['ct'].shape, spacing=(1.0, 1.0, 1.0)) == [int(x) for x in v['region']]
            pts = R.box_points([int(x) for x in v['region']])[::3, ::3, ::3].reshape(-1, 3)
            ref = v['local'][::3, ::3, ::3].reshape(-1, 3)
            with warnings.catch_warnings(), np.errstate(all='ignore'):
                warnings.simplefilter('ignore')
                got = np.array([S.global_to_local(p, plan['knots'], plan['basis'], SR.PLANE, (1.0, 1.0, 1.0)) for p in pts])
                same = np.array([S.global_to_local(p, plan['knots'], plan['basis']) for p in pts])
            assert np.array_equal(got, same, equal_nan=True)
            fin = np.isfinite(ref).all(-1)
            assert np.abs(got - ref)[fin].max() <= R.LOCAL_MEASURED


def test_restore_box_contains_every_covered_voxel():
    """For every vertebra of every case: the fixture records, from the reference's own global_to_local of EVERY patient voxel, which voxels
    the crop covers; none of them may lie outside restore_box at that spacing (pad stays 2 voxels)."""
    from hvgan import straighten as S
    for name in CURVED:
        c, plan = _g()[name], _plan(name)
        shape = c['ct'].shape
        for vid, box in zip(c['ids'], plan['boxes']):
            region = S.restore_box(plan['knots'], plan['basis'], box, shape, spacing=c['spacing'])
            assert region == [int(v) for v in c['region'][vid]]
            mask = c['covered_volume'][vid]
            assert mask.shape == shape and mask.any()
            sl = tuple(slice(region[i], region[i] + region[3 + i]) for i in range(3))
            outside = mask.copy()
            outside[sl] = False
            assert not outside.any(), (name, vid, int(outside.sum()))
        b = c['box']
        sl = tuple(slice(int(b['region'][i]), int(b['region'][i] + b['region'][3 + i])) for i in range(3))
        assert np.array_equal(c['covered_volume'][b['vid']][sl], b['covered'])


def test_bad_spacing_is_refused_before_any_launch():
    """Host tensors reach every spacing check: a valid call then stops at the device check (RuntimeError), an invalid one never gets there."""
    from hvgan import straighten as S
    c = _g()['aniso']
    plan = _plan('aniso')
    ct, label = torch.from_numpy(c['ct']), torch.from_numpy(c['label'])
    crops = {v: (torch.from_numpy(c['crop_ct'][k]), torch.from_numpy(c['crop_label'][k])) for k, v in enumerate(c['ids'])}
    bad = [(0.7, 0.0, 1.5), (0.7, -1.0, 1.5), (0.7, float('nan'), 1.5), (0.7, float('inf'), 1.5), (0.7, 1.5), (1, 2, 3, 4), 0, -2.0, 'abc',
           None, (True, 1.0, 1.0)]
    tables = [([0.0, 0.7, 1.4], 0.7, 1.5), (0.7, np.arange(64) * 0.7, 1.5)]
    for sp in bad + tables:
        with pytest.raises(ValueError):
            S.check_spacing(sp)
        with pytest.raises(ValueError):
            S.straighten_patient(ct, label, c['ids'], spacing=sp)
        with pytest.raises(ValueError):
            S.plan(c['centroid_list'], c['ct'].shape, c['ids'], c['out_size'], spacing=sp)
        with pytest.raises(ValueError):
            S.curve_frame(c['curve'], 1, sp)
        with pytest.raises(ValueError):
            S.restore_box(plan['knots'], plan['basis'], plan['boxes'][0], c['ct'].shape, spacing=sp)
        if sp is not None:          # None: the plan's own
            with pytest.raises(ValueError):
                S.restore_patient(plan, crops, shape=c['ct'].shape, where='crop', spacing=sp)
    for sp in tables:
        with pytest.raises(ValueError, match='per-axis position tables'):
            S.check_spacing(sp)
    with pytest.raises(ValueError, match='plan'):
        S.restore_patient(plan, crops, shape=c['ct'].shape, where='crop', spacing=(1.0, 1.0, 1.0))      # disagrees with the plan
    old = {k: v for k, v in plan.items() if k != 'spacing'}                                            # a plan from before: ones
    with pytest.raises(ValueError, match='plan'):
        S.restore_patient(old, crops, shape=c['ct'].shape, where='crop', spacing=c['spacing'])
    with pytest.raises(ValueError):
        S.points_to_local(plan, np.zeros((4, 2)))
    with pytest.raises(ValueError):
        S.points_to_global(dict(plan, spacing=(0.0, 1.0, 1.0)), np.zeros((4, 3)))
    for good in (None, c['spacing'], list(c['spacing'])):
        with pytest.raises(RuntimeError):                        # valid, but host tensors: no CPU path
            S.restore_patient(plan, crops, shape=c['ct'].shape, where='crop', spacing=good)
    with pytest.raises(RuntimeError):
        S.straighten_patient(ct, label, c['ids'], spacing=c['spacing'])
    assert S.check_spacing(2) == (2.0, 2.0, 2.0) and S.check_spacing(np.float32(0.5)) == (0.5, 0.5, 0.5)


def test_header_declares_and_library_exports_the_entries():
    from hvgan import lib
    _, protos = lib.parse_header()
    import ctypes
    for name, nargs in (('hv_straighten_sample_sp', 27), ('hv_restore_volume_sp', 45), ('hv_curve_points', 12)):
        assert name in protos and len(protos[name][1]) == nargs, name
        assert protos[name][0] is ctypes.c_int
    # the entries from before keep their signatures: the new ones are those plus the spacing pointer before the stream
    for old, new in (('hv_straighten_sample', 'hv_straighten_sample_sp'), ('hv_restore_volume', 'hv_restore_volume_sp')):
        assert protos[new][1][:-2] == protos[old][1][:-1] and protos[new][1][-2:] == [ctypes.c_void_p, ctypes.c_void_p]
    L = lib.get()
    for name in ('hv_straighten_sample', 'hv_straighten_sample_sp', 'hv_restore_volume', 'hv_restore_volume_sp', 'hv_curve_points'):
        assert hasattr(L.cdll, name), name
    src = open(lib.HEADER).read()
    assert 'HV_CURVE_TO_LOCAL = 0' in src and 'HV_CURVE_TO_GLOBAL = 1' in src
