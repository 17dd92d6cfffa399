"""Restore of straightened crops to patient space on the device (hvgan.straighten.restore_patient: csrc/restore.hip) against the
reference's own Interpolator.global_to_local and scipy's samples (fixture G20, tools/make_golden_restore.py), against the numpy
restatement tests/restore_ref.py for the write rules, and on an affine round trip that needs no fixture."""
import numpy as np
import pytest
import torch

import restore_ref as R

pytestmark = pytest.mark.gpu

# Largest |restore_ref - reference| local coordinate over G20, measured on the host: 0 (tests/test_restore_cpu.py prints it).  The device
# tolerance is ten times that with the floor 1e-12 (the project's figure for the host curve math), the decision margin 100 times the tolerance.
LOCAL_TOL = 1e-12
MARGIN_DELTA = 1e-10
CT_TOL = 1e-9             # the crops against the reference

_CACHE = {}


def _g():
    if 'g' not in _CACHE:
        import hvgan  # noqa: F401
        _CACHE['g'] = R.load_g20()
    return _CACHE['g']


def _case(name):
    """Plan, device crops and the reference results of restore_ref (from the fixture's coordinates) of one G20 case, built once."""
    if name not in _CACHE:
        c = _g()[name]
        plan = R.plan_of(c)
        crops = {v: (c['crop_ct'][k], c['crop_label'][k]) for k, v in enumerate(c['ids'])}
        local = {v: c[v]['local'] for v in c['ids']}
        _CACHE[name] = (c, plan, crops, local)
    return _CACHE[name]


def _dev(crops, order=None):
    return {v: (torch.from_numpy(np.ascontiguousarray(crops[v][0])).cuda(), torch.from_numpy(np.ascontiguousarray(crops[v][1])).cuda())
            for v in (order or list(crops))}


def _sl(region):
    return tuple(slice(int(region[i]), int(region[i] + region[3 + i])) for i in range(3))


@pytest.mark.parametrize('case', ['lds', 'global'])
def test_affine_round_trip(case):
    """Collinear centroids on an oblique line: constant frames, local <-> global affine, a linear ramp CT inside the window comes back as it
    was.  'global': more knots than the LDS stage holds (630), so the kernel reads them from global memory."""
    import hvgan  # noqa: F401
    from hvgan import straighten as S
    if case == 'lds':
        shape, p0, p1, out_size = (56, 56, 96), np.array([22.0, 24.0, 26.0]), np.array([34.0, 32.0, 70.0]), (40, 32, 16)
    else:
        shape, p0, p1, out_size = (24, 24, 720), np.array([10.0, 11.0, 30.0]), np.array([14.0, 13.0, 690.0]), (40, 16, 12)
    ids = [1, 2, 3, 4]
    cents = [{'label': i, 'X': float(p[0]), 'Y': float(p[1]), 'Z': float(p[2])} for i, p in zip(ids, (p0 + (p1 - p0) * t for t in (0, 1 / 3, 2 / 3, 1)))]
    x, y, z = np.meshgrid(*(np.arange(s, dtype=np.float64) for s in shape), indexing='ij')
    ramp = 1.75 * x - 2.5 * y + 0.625 * z + 40.0
    assert ramp.min() > -300 and ramp.max() < 800
    label = np.zeros(shape, dtype=np.uint8)
    for e in cents:
        label[int(e['X']) - 1:int(e['X']) + 2, int(e['Y']) - 1:int(e['Y']) + 2, int(e['Z']) - 1:int(e['Z']) + 2] = e['label']
    tct, tlab = torch.from_numpy(ramp).cuda(), torch.from_numpy(label).cuda()
    want = [2, 3]
    crops, plan = S.straighten_patient(tct, tlab, want, centroids=cents, out_size=out_size, return_plan=True)
    assert not plan['window']
    N = len(plan['knots'])
    assert (N > 630) == (case == 'global')
    assert np.abs(plan['basis'] - plan['basis'][0]).max() <= 1e-12            # constant frames: the extension was not clamped
    ct_out, lab_out, covered = S.restore_patient(plan, crops, shape=shape, where='crop', return_covered=True)
    torch.cuda.synchronize()
    ct_out, covered = ct_out.cpu().numpy(), covered.cpu().numpy().astype(bool)
    assert covered.any()
    inside_boxes = np.zeros(shape, dtype=bool)
    checked = 0
    for vid, box in zip(want, plan['boxes']):
        region = S.restore_box(plan['knots'], plan['basis'], box, shape)
        inside_boxes[_sl(region)] = True
        keep = np.zeros(shape, dtype=bool)            # 2 away from the box border and from the volume border
        keep[tuple(slice(max(region[i], 0) + 2, min(region[i] + region[3 + i], shape[i]) - 2) for i in range(3))] = True
        keep[:2], keep[-2:], keep[:, :2], keep[:, -2:], keep[:, :, :2], keep[:, :, -2:] = (False,) * 6
        m = keep & covered
        checked += int(m.sum())
        # the other vertebra's crop may have written a kept voxel last: both hold the ramp
        err = np.abs(ct_out - ramp)[m].max()
        print(case, vid, 'N', N, 'region', region, 'checked', int(m.sum()), 'max |ct - ramp| %.3g' % err)
        assert err <= CT_TOL, (case, vid, err)
    assert checked > 1000
    assert not (covered & ~inside_boxes).any()
    assert (ct_out[~covered] == 0).all() and (lab_out.cpu().numpy()[~covered] == 0).all()


def _run_single(name, vid, regions=None):
    from hvgan import straighten as S
    c, plan, crops, _ = _case(name)
    out = S.restore_patient(plan, _dev(crops, [vid]), shape=c['ct'].shape, where='crop', return_covered=True, return_local=True, regions=regions)
    torch.cuda.synchronize()
    ct_out, lab_out, covered, local = out
    region, loc = local[vid]
    return ct_out.cpu().numpy(), lab_out.cpu().numpy(), covered.cpu().numpy().astype(bool), region, loc.cpu().numpy()


def _check_local(tag, got, ref, margin):
    keep = margin >= MARGIN_DELTA
    assert (~keep).mean() <= R.MARGIN_CAP, tag
    fin = np.isfinite(ref).all(-1)
    assert np.isnan(got[keep & ~fin]).all(), tag                 # no coordinate in the reference: NaN here
    err = np.abs(got - ref)[keep & fin]
    print(tag, 'voxels', keep.size, 'kept', int(keep.sum()), 'max |local - reference| %.3g' % err.max())
    assert np.isfinite(got[keep & fin]).all() and err.max() <= LOCAL_TOL, (tag, err.max())


def test_g20_local_coordinates_match_the_reference():
    for name, c in _g().items():
        for vid in c['ids']:
            v = c[vid]
            _, _, _, region, loc = _run_single(name, vid)
            assert list(region) == [int(x) for x in v['region']]
            _check_local('%s/%d' % (name, vid), loc, v['local'], v['margin'])
        if 'probe' in c:        # a slab far from the vertebra: several sign changes, none, the clipped window
            pr = c['probe']
            reg = [int(x) for x in pr['region']]
            _, _, _, region, loc = _run_single(name, c['ids'][0], regions={c['ids'][0]: reg})
            assert list(region) == reg
            _check_local(name + '/probe', loc, pr['local'], pr['margin'])


def test_g20_samples_labels_and_coverage_match_scipy():
    for name, c in _g().items():
        for vid in c['ids']:
            v = c[vid]
            ct_out, lab_out, covered, region, _ = _run_single(name, vid)
            sl = _sl(region)
            keep = v['margin'] >= MARGIN_DELTA
            assert np.array_equal(covered[sl][keep], v['covered'][keep]), (name, vid)
            m = keep & v['covered']
            err = np.abs(ct_out[sl] - v['sample_ct'])[m].max()
            print(name, vid, 'covered', int(m.sum()), 'max |ct - scipy| %.3g' % err)
            assert err <= CT_TOL, (name, vid, err)
            m = v['covered'] & (v['margin_label'] >= MARGIN_DELTA)
            assert np.array_equal(lab_out[sl][m], v['sample_label'][m]), (name, vid)
            outside = np.ones(covered.shape, dtype=bool)
            outside[sl] = False
            assert not covered[outside].any() and (ct_out[outside] == 0).all() and (lab_out[outside] == 0).all()


def _agree(tag, got, ref, low):
    """Device outputs against restore_ref's, the voxels with a small decision margin left out."""
    ct_out, lab_out, covered = (t.cpu().numpy() for t in got)
    ok = ~low
    assert np.array_equal(covered[ok], ref[2][ok]), tag
    assert np.abs(ct_out - ref[0])[ok].max() <= CT_TOL, tag
    assert np.array_equal(lab_out[ok], ref[1][ok]), tag


@pytest.mark.parametrize('where', ['crop', 'vertebra'])
def test_write_rules_and_overlapping_boxes_in_both_orders(where):
    from hvgan import straighten as S
    c, plan, crops, local = _case('curved')
    shape = c['ct'].shape
    tct, tlab = torch.from_numpy(c['ct']).cuda(), torch.from_numpy(c['label']).cuda()
    low = np.zeros(shape, dtype=bool)
    boxes = np.zeros(shape, dtype=np.int32)
    for vid in c['ids']:
        low[_sl(c[vid]['region'])] |= c[vid]['margin_label'] < MARGIN_DELTA
        boxes[_sl(c[vid]['region'])] += 1
    assert (boxes == 2).any()                                    # the two boxes overlap
    base = R.base_volumes(plan, shape, c['ct'], c['label'])
    for order in (c['ids'], c['ids'][::-1]):
        key = ('ref', where, tuple(order))
        if key not in _CACHE:
            _CACHE[key] = R.restore(plan, {v: crops[v] for v in order}, shape, c['ct'], c['label'], where=where, local=local)
        ref = _CACHE[key]
        got = S.restore_patient(plan, _dev(crops, order), ct=tct, label=tlab, where=where, return_covered=True)
        _agree((where, order), got, ref, low)
        assert ref[2].any() and (where == 'crop' or (ref[2] == 0)[boxes > 0].any())      # the vertebra rule writes less than the box covers
        # == one vertebra after the other, in that order, bit for bit
        seq = None
        cov = np.zeros(shape, dtype=np.uint8)
        for v in order:
            r = S.restore_patient(plan, _dev(crops, [v]), ct=tct, label=tlab, where=where, return_covered=True, out=seq)
            seq = (r[0], r[1])
            cov |= r[2].cpu().numpy()
        assert torch.equal(seq[0], got[0]) and torch.equal(seq[1], got[1]) and np.array_equal(cov, got[2].cpu().numpy())
        # outside every box: the base, byte for byte
        assert np.array_equal(got[0].cpu().numpy()[boxes == 0], base[0][boxes == 0])
        assert np.array_equal(got[1].cpu().numpy()[boxes == 0], base[1][boxes == 0])
        assert not got[2].cpu().numpy()[boxes == 0].any()


def test_layouts_and_dtypes_give_the_same_bytes():
    from hvgan import straighten as S
    c, plan, crops, _ = _case('curved')
    shape = c['ct'].shape
    # float32-representable crop values, so that a float32 crop holds the same numbers
    crops = {v: (crops[v][0].astype(np.float32).astype(np.float64), crops[v][1]) for v in crops}
    tct, tlab = torch.from_numpy(c['ct']).cuda(), torch.from_numpy(c['label']).cuda()
    want = S.restore_patient(plan, _dev(crops), ct=tct, label=tlab, where='vertebra', return_covered=True)

    def same(got):
        assert all(torch.equal(a, b) for a, b in zip(got, want))

    fort = {v: tuple(torch.from_numpy(np.asfortranarray(a)).cuda() for a in crops[v]) for v in crops}
    assert all(t.stride()[0] == 1 for pair in fort.values() for t in pair)
    same(S.restore_patient(plan, fort, ct=tct, label=tlab, where='vertebra', return_covered=True))
    f32 = {v: (torch.from_numpy(crops[v][0].astype(np.float32)).cuda(), torch.from_numpy(crops[v][1]).cuda()) for v in crops}
    same(S.restore_patient(plan, f32, ct=tct, label=tlab, where='vertebra', return_covered=True))
    fct = torch.from_numpy(np.asfortranarray(c['ct'])).cuda()            # int16, Fortran order
    flab = torch.from_numpy(np.asfortranarray(c['label']).astype(np.float64)).cuda()
    assert fct.stride()[0] == 1 and fct.dtype == torch.int16
    same(S.restore_patient(plan, _dev(crops), ct=fct, label=flab, where='vertebra', return_covered=True))
    # non-contiguous outputs: every second element of wider tensors, started from the same bases
    wide_ct = torch.zeros(shape[0], shape[1], 2 * shape[2], dtype=torch.float64, device='cuda')
    wide_lab = torch.zeros(2 * shape[0], shape[1], shape[2], dtype=torch.uint8, device='cuda')
    base = R.base_volumes(plan, shape, c['ct'], c['label'])
    out = (wide_ct[:, :, ::2], wide_lab[::2])
    out[0].copy_(torch.from_numpy(base[0]))
    out[1].copy_(torch.from_numpy(base[1]))
    got = S.restore_patient(plan, _dev(crops), label=tlab, where='vertebra', return_covered=True, out=out)
    assert got[0].data_ptr() == wide_ct.data_ptr() and not got[0].is_contiguous()
    same(got)
    assert (wide_ct[:, :, 1::2] == 0).all() and (wide_lab[1::2] == 0).all()


def test_single_centroid_is_the_plain_uncrop():
    import hvgan  # noqa: F401
    from hvgan import straighten as S, synth
    ct, label = synth.make_spine_patient(seed=3, shape=(40, 48, 56), n_vert=3, radius=(10, 9, 6))
    tct, tlab = torch.from_numpy(ct).cuda(), torch.from_numpy(label).cuda()
    crops, plan = S.straighten_patient(tct, tlab, [17], out_size=(32, 40, 24), return_plan=True)
    assert plan['knots'] is None
    for where in ('crop', 'vertebra'):
        ct_out, lab_out, covered = S.restore_patient(plan, crops, shape=ct.shape, label=tlab, where=where, return_covered=True,
                                                     out=(torch.zeros(ct.shape, dtype=torch.float64, device='cuda'),
                                                          torch.zeros(ct.shape, dtype=torch.uint8, device='cuda')))
        lo, n, st = (plan['boxes'][0][i:i + 3] for i in (0, 3, 6))
        src = tuple(slice(st[i], st[i] + n[i]) for i in range(3))
        dst = tuple(slice(lo[i], lo[i] + n[i]) for i in range(3))
        cc, cl = crops[17][0].cpu().numpy()[src], crops[17][1].cpu().numpy()[src]
        write = np.ones(cc.shape, dtype=bool) if where == 'crop' else (cl == 17) | (label[dst] == 17)
        exp_ct, exp_lab, exp_cov = np.zeros(ct.shape), np.zeros(ct.shape, np.uint8), np.zeros(ct.shape, np.uint8)
        exp_ct[dst][write], exp_lab[dst][write], exp_cov[dst][write] = cc[write], cl[write], 1
        assert write.any() and (where == 'crop' or not write.all())
        assert np.array_equal(ct_out.cpu().numpy(), exp_ct) and np.array_equal(lab_out.cpu().numpy(), exp_lab)
        assert np.array_equal(covered.cpu().numpy(), exp_cov)


def test_bad_inputs_raise_and_a_following_call_succeeds():
    from hvgan import straighten as S
    c, plan, crops, _ = _case('curved')
    shape = c['ct'].shape
    d = _dev(crops)
    tlab = torch.from_numpy(c['label']).cuda()
    with pytest.raises(ValueError):
        S.restore_patient(plan, {42: d[17]}, shape=shape, where='crop')
    with pytest.raises(ValueError):
        S.restore_patient(plan, {17: (d[17][0][:, :-1], d[17][1][:, :-1])}, shape=shape, where='crop')
    with pytest.raises(ValueError):
        S.restore_patient(plan, d, shape=shape)
    with pytest.raises(ValueError):
        S.restore_patient(plan, d, shape=(48, 64, 90), label=tlab)
    with pytest.raises(ValueError):
        S.restore_patient(plan, d, shape=shape, where='crop', regions={17: [40, 0, 0, 20, 64, 96]})
    with pytest.raises(TypeError):
        S.restore_patient(plan, {17: (d[17][0], d[17][1].to(torch.int16))}, shape=shape, where='crop')
    with pytest.raises(RuntimeError):
        S.restore_patient(plan, {17: (d[17][0].cpu(), d[17][1].cpu())}, shape=shape, where='crop')
    got = S.restore_patient(plan, {17: d[17]}, shape=shape, where='crop', return_covered=True)
    v = c[17]
    keep = v['margin'] >= MARGIN_DELTA
    assert np.array_equal(got[2].cpu().numpy().astype(bool)[_sl(v['region'])][keep], v['covered'][keep])


def test_full_size_patient_restores_its_vertebra():
    import hvgan  # noqa: F401
    from hvgan import straighten as S, synth
    shape = (512, 512, 400)
    ct, label = synth.make_spine_patient(seed=11, shape=shape, n_vert=10, radius=(40, 30, 11), end_radius=(14, 12, 6), margin=20, curve=(20.0, 40.0))
    tct, tlab = torch.from_numpy(ct).cuda(), torch.from_numpy(label).cuda()
    vid = 20
    crops, plan = S.straighten_patient(tct, tlab, [vid], out_size=(256, 256, 64), return_plan=True)
    zeros = (torch.zeros(shape, dtype=torch.float64, device='cuda'), torch.zeros(shape, dtype=torch.uint8, device='cuda'))
    ct_out, lab_out, covered = S.restore_patient(plan, crops, label=tlab, where='vertebra', return_covered=True, out=zeros)
    torch.cuda.synchronize()
    assert int(covered.sum()) > 0
    n_crop, n_back = int((crops[vid][1] == vid).sum()), int((lab_out == vid).sum())
    print('knots', len(plan['knots']), 'crop voxels', n_crop, 'restored', n_back)
    # loose on purpose: a check of orientation and axis order, not parity
    assert n_crop > 0 and abs(n_back - n_crop) <= 0.05 * n_crop
    # the restored vertebra lies on the patient's own (the crop holds all of it but what the 64-wide axis cuts off)
    both = int(((lab_out == vid) & (tlab == vid)).sum())
    assert both >= 0.9 * n_back
