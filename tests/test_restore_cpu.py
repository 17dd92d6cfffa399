"""Host side of the restore to patient space (hvgan.straighten.restore_box / restore_patient's argument checks) and its numpy restatement
tests/restore_ref.py against fixture G20 (tools/make_golden_restore.py: the reference's own Interpolator.global_to_local for every voxel
of each restore box, scipy's samples of the crops there, per-voxel decision margins).  No device: these run everywhere."""
import numpy as np
import pytest
import torch

import restore_ref as R

_CACHE = {}


def _g():
    if 'g' not in _CACHE:
        import hvgan  # noqa: F401
        _CACHE['g'] = R.load_g20()
    return _CACHE['g']


def _ref_local(name, vid):
    """restore_ref's own coordinates for one fixture box (computed once per session)."""
    key = ('local', name, vid)
    if key not in _CACHE:
        c = _g()[name]
        _CACHE[key] = R.local_coords(c['knots'], c['basis'], [int(v) for v in c[vid]['region']])
    return _CACHE[key]


def _boxes(c):
    return [(vid, [int(v) for v in box]) for vid, box in zip(c['ids'], c['boxes'])]


def test_fixture_holds_the_branches_and_the_margin_cap():
    g = _g()
    assert set(g) == {'curved', 'edge'} and g['curved']['ids'] == [17, 18] and 'probe' in g['edge']
    for name, c in g.items():
        assert c['ct'].shape == (48, 64, 96)
        for vid, _ in _boxes(c):
            v = c[vid]
            assert v['local'].shape == tuple(v['region'][3:]) + (3,) and v['covered'].any()
            assert (v['margin_label'] < R.MARGIN_DELTA).mean() <= R.MARGIN_CAP, (name, vid)       # a condition, not a measurement
            assert (v['margin'] < R.MARGIN_DELTA).mean() <= R.MARGIN_CAP, (name, vid)
        if 'probe' in c:
            assert (c['probe']['margin'] < R.MARGIN_DELTA).mean() <= R.MARGIN_CAP, name
    # the two boxes of the adjacent vertebrae overlap
    a, b = (g['curved'][v]['region'] for v in (17, 18))
    assert all(max(a[i], b[i]) < min(a[i] + a[3 + i], b[i] + b[3 + i]) for i in range(3))
    assert R.LOCAL_TOL == max(10 * R.LOCAL_MEASURED, 1e-12) and R.MARGIN_DELTA == 100 * R.LOCAL_TOL


def test_restore_ref_reproduces_the_reference_coordinates():
    worst = 0.0
    for name, c in _g().items():
        for vid, _ in _boxes(c):
            ref, got = c[vid]['local'], _ref_local(name, vid)
            fin = np.isfinite(ref).all(-1)
            assert np.array_equal(fin, np.isfinite(got).all(-1)), (name, vid)
            worst = max(worst, float(np.abs(got - ref)[fin].max()))
    print('largest |restore_ref - reference| local coordinate over G20: %.3g' % worst)
    assert worst <= R.LOCAL_MEASURED          # the figure the device tolerance is derived from


def test_restore_ref_reproduces_the_recorded_samples():
    from hvgan import straighten as S
    for name, c in _g().items():
        plan = R.plan_of(c)
        assert np.array_equal(np.array(plan['boxes']), c['boxes'])
        for k, (vid, box) in enumerate(_boxes(c)):
            v = c[vid]
            assert S.restore_box(plan['knots'], plan['basis'], box, c['ct'].shape) == [int(x) for x in v['region']]
            got = R.restore(plan, {vid: (c['crop_ct'][k], c['crop_label'][k])}, c['ct'].shape, where='crop', local={vid: _ref_local(name, vid)})
            sl = tuple(slice(int(v['region'][i]), int(v['region'][i] + v['region'][3 + i])) for i in range(3))
            keep = v['margin'] >= R.MARGIN_DELTA
            assert np.array_equal(got[2][sl].astype(bool)[keep], v['covered'][keep]), (name, vid)
            cov = v['covered'] & keep
            assert np.abs(got[0][sl] - v['sample_ct'])[cov].max() <= 1e-9, (name, vid)
            cov = v['covered'] & (v['margin_label'] >= R.MARGIN_DELTA)
            assert np.array_equal(got[1][sl][cov], v['sample_label'][cov]), (name, vid)
            outside = np.ones(c['ct'].shape, dtype=bool)
            outside[sl] = False
            assert not got[2][outside].any()


def test_restore_box_contains_every_covered_voxel():
    """Brute force over the whole 48 x 64 x 96 volume, for every vertebra of both cases: the fixture records, from the reference's own
    global_to_local of EVERY patient voxel, which voxels each crop covers (`covered_volume`); none of them may lie outside restore_box.
    The mask is pinned to this code by a point-by-point recomputation on a lattice over the whole volume (every fifth voxel per axis,
    offset per vertebra) and by the box's own recorded coverage."""
    import warnings
    from hvgan import straighten as S
    for name, c in _g().items():
        plan = R.plan_of(c)
        shape = c['ct'].shape
        for k, (vid, box) in enumerate(_boxes(c)):
            region = S.restore_box(plan['knots'], plan['basis'], box, shape)
            assert region == [int(x) for x in c[vid]['region']]
            mask = c[vid]['covered_volume']
            assert mask.shape == shape and mask.dtype == bool and mask.any()
            sl = tuple(slice(region[i], region[i] + region[3 + i]) for i in range(3))
            outside = mask.copy()
            outside[sl] = False
            assert not outside.any(), (name, vid, int(outside.sum()))
            assert np.array_equal(mask[sl], c[vid]['covered']), (name, vid)
            lattice = R.box_points([0, 0, 0] + list(shape))[k % 5::5, (k + 2) % 5::5, (k + 4) % 5::5]
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                loc = np.array([S.global_to_local(p, plan['knots'], plan['basis']) for p in lattice.reshape(-1, 3)])
            cov = R.crop_coords(loc, box)[1].reshape(lattice.shape[:3])
            assert np.array_equal(cov, mask[k % 5::5, (k + 2) % 5::5, (k + 4) % 5::5]), (name, vid)
    # the single-centroid branch: the box is the crop's source range
    assert S.restore_box(None, None, [3, 4, 5, 6, 7, 8, 1, 0, 2], (20, 20, 20)) == [3, 4, 5, 6, 7, 8]
    assert S.restore_box(None, None, [3, 4, 5, 0, 7, 8, 1, 0, 2], (20, 20, 20)) == [0] * 6


def test_restore_patient_refuses_bad_arguments_before_any_launch():
    """Every ValueError is raised from host arithmetic alone: host tensors get that far (a valid call then stops at the device check)."""
    from hvgan import straighten as S
    c = _g()['curved']
    plan = R.plan_of(c)
    shape = c['ct'].shape
    crops = {v: (torch.from_numpy(c['crop_ct'][k]), torch.from_numpy(c['crop_label'][k])) for k, v in enumerate(c['ids'])}
    label = torch.from_numpy(c['label'])
    with pytest.raises(ValueError):
        S.restore_patient(plan, {42: crops[17]}, shape=shape, where='crop')                  # not in the plan
    with pytest.raises(ValueError):
        S.restore_patient(plan, {17: (crops[17][0][:-2], crops[17][1][:-2])}, shape=shape, where='crop')   # not the size the plan cut
    other = S.plan(c['centroid_list'], shape, [18, 17], c['out_size'])       # the rows in another order: 17's row is not at 17's index
    swapped = dict(plan, boxes=other[3])
    with pytest.raises(ValueError):
        S.restore_patient(swapped, {17: crops[17]}, shape=shape, where='crop')               # matched against its own row only
    with pytest.raises(ValueError):
        S.restore_patient(plan, crops, shape=shape)                                          # where='vertebra' without the label
    with pytest.raises(ValueError):
        S.restore_patient(plan, crops, shape=(48, 64, 95), label=label)                      # shape against the label's
    with pytest.raises(ValueError):
        S.restore_patient(plan, crops, where='crop')                                         # no shape at all
    with pytest.raises(ValueError):
        S.restore_patient(plan, crops, shape=shape, where='everything')
    with pytest.raises(RuntimeError):
        S.restore_patient(plan, crops, shape=shape, where='crop')                            # valid, but host tensors: no CPU path
