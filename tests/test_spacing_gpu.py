"""Straightening and restoring scans with anisotropic voxel spacing on the device (hvgan.straighten with spacing=, points_to_local /
points_to_global: csrc/straighten.hip, csrc/restore.hip) against the reference's own results at that spacing (fixture G21,
tools/make_golden_spacing.py), bit for bit against the entries without a spacing at (1, 1, 1), and on an affine round trip."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import restore_ref as R
import spacing_ref as SR

pytestmark = pytest.mark.gpu

# Largest |host restatement - reference| over G21, measured on the host (tests/test_spacing_cpu.py prints and asserts them): 0 for the
# local coordinates and 0 for local_to_global.  Device tolerance: ten times that, floor 1e-12; the decision margin 100 times the tolerance.
LOCAL_MEASURED, GLOBAL_MEASURED = 0.0, 0.0
LOCAL_TOL = 1e-12
GLOBAL_TOL = 1e-12
MARGIN_DELTA = 1e-10
CT_TOL = 1e-9             # the crops against the reference
CURVED = ('aniso', 'thick', 'fine', 'edge')

_CACHE = {}


def _g():
    if 'g' not in _CACHE:
        import hvgan  # noqa: F401
        _CACHE['g'] = SR.load_g21()
        assert SR.LOCAL_TOL == LOCAL_TOL and SR.GLOBAL_TOL == GLOBAL_TOL and SR.MARGIN_DELTA == MARGIN_DELTA
    return _CACHE['g']


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _straighten(name, **kw):
    """straighten_patient of one G21 case at its spacing, once per session: -> (case, crops, plan)."""
    from hvgan import straighten as S
    key = ('straight', name)
    if key not in _CACHE:
        c = _g()[name]
        crops, plan = S.straighten_patient(_dev(c['ct']), _dev(c['label']), c['ids'], out_size=c['out_size'], return_plan=True,
                                           spacing=c['spacing'])
        torch.cuda.synchronize()
        _CACHE[key] = (c, crops, plan)
    return _CACHE[key]


def _sl(region):
    return tuple(slice(int(region[i]), int(region[i] + region[3 + i])) for i in range(3))


@pytest.mark.parametrize('name', CURVED + ('single',))
def test_crops_and_plan_match_the_reference(name):
    c, crops, plan = _straighten(name)
    assert plan['spacing'] == c['spacing'] and plan['window'] == bool(c['window'])
    assert np.array_equal(np.array(plan['boxes']), c['boxes'])
    if name == 'single':
        assert plan['knots'] is None
    else:
        for key in ('knots', 'basis'):
            err = np.abs(plan[key] - c[key]).max()
            print(name, key, 'max |plan - reference| %.3g' % err)
            assert plan[key].shape == c[key].shape and err <= LOCAL_TOL, (name, key, err)
        err = np.abs(np.stack([plan['local'][v] for v in c['ids']]) - c['local']).max()
        print(name, 'local centroids max |plan - reference| %.3g' % err)
        assert err <= LOCAL_TOL, (name, err)
    for k, v in enumerate(c['ids']):
        ct, lab = crops[v]
        assert ct.dtype == torch.float64 and lab.dtype == torch.uint8 and tuple(ct.shape) == c['out_size']
        ct, lab = ct.cpu().numpy(), lab.cpu().numpy()
        err = np.abs(ct - c['crop_ct'][k]).max()
        risky = c['crop_risky'][v] if name != 'single' else np.zeros(c['out_size'], dtype=bool)
        bad = lab != c['crop_label'][k]
        print(name, v, 'max |ct - reference| %.3g' % err, 'label mismatches', int(bad.sum()), 'near a half-integer', int(risky.sum()))
        assert err <= CT_TOL, (name, v, err)
        assert risky.mean() <= SR.MARGIN_CAP and not (bad & ~risky).any(), (name, v, int((bad & ~risky).sum()))
        assert (lab != 0).any() and (ct != 0).any()
    if name == 'fine':          # the 128 mm plane is wider than the scan: most of the crop's plane is outside and zero
        assert (crops[c['ids'][0]][0] == 0).any()


def test_unit_spacing_gives_the_bytes_of_the_call_without_it():
    import hvgan  # noqa: F401
    from hvgan import straighten as S
    c = R.load_g20()['curved']
    tct, tlab = _dev(c['ct']), _dev(c['label'])
    a, pa = S.straighten_patient(tct, tlab, c['ids'], out_size=c['out_size'], return_plan=True)
    for sp in ((1.0, 1.0, 1.0), 1):
        b, pb = S.straighten_patient(tct, tlab, c['ids'], out_size=c['out_size'], return_plan=True, spacing=sp)
        assert pa['spacing'] == pb['spacing'] == (1.0, 1.0, 1.0)
        assert np.array_equal(pa['knots'], pb['knots']) and np.array_equal(pa['basis'], pb['basis']) and pa['boxes'] == pb['boxes']
        for v in c['ids']:
            assert torch.equal(a[v][0], b[v][0]) and torch.equal(a[v][1], b[v][1])
    old = {k: v for k, v in pa.items() if k != 'spacing'}            # a plan made before plans recorded the spacing
    ra = S.restore_patient(old, a, ct=tct, label=tlab, where='vertebra', return_covered=True, return_local=True)
    rb = S.restore_patient(pa, a, ct=tct, label=tlab, where='vertebra', return_covered=True, return_local=True, spacing=(1.0, 1.0, 1.0))
    assert all(torch.equal(x, y) for x, y in zip(ra[:3], rb[:3])) and ra[2].any()
    for v in c['ids']:
        assert ra[3][v][0] == rb[3][v][0] and torch.equal(ra[3][v][1].view(torch.int64), rb[3][v][1].view(torch.int64))


def test_sp_entries_with_ones_give_the_bytes_of_the_old_entries():
    import hvgan  # noqa: F401
    from hvgan import lib as _lib, straighten as S
    c = R.load_g20()['curved']
    plan = R.plan_of(c)
    L = _lib.get()
    tct, tlab = _dev(c['ct']), _dev(c['label'])
    st = lambda t: [ctypes.c_longlong(s) for s in t.stride()]      # noqa: E731
    X, Y, Z = c['ct'].shape
    N = len(plan['knots'])
    d_knots, d_basis, d_cum = _dev(plan['knots']), _dev(plan['basis']), _dev(S.cumulative_length(plan['knots']))
    ones = (ctypes.c_double * 3)(1.0, 1.0, 1.0)
    pbytes = L.size('hv_straighten_presence_bytes', 128)
    wmin, wmax = ctypes.c_double(-300.0), ctypes.c_double(800.0)
    outs = []
    for entry, extra in (('hv_straighten_sample', ()), ('hv_straighten_sample_sp', (ones,))):
        sct = torch.full((N, 128, 128), -1.0, dtype=torch.float64, device='cuda')
        slab = torch.full((N, 128, 128), 255, dtype=torch.uint8, device='cuda')
        pres = torch.full((pbytes // 8,), -1, dtype=torch.int64, device='cuda')
        L.call(entry, _lib.ptr(tct), 1, *st(tct), _lib.ptr(tlab), 0, *st(tlab), X, Y, Z, _lib.ptr(d_knots), _lib.ptr(d_basis), N, 128, 128, 1,
               wmin, wmax, _lib.ptr(sct), _lib.ptr(slab), _lib.ptr(pres), ctypes.c_size_t(pbytes), *extra, _lib.stream())
        outs.append((sct, slab, pres))
    assert all(torch.equal(a, b) for a, b in zip(*outs)) and (outs[0][1] != 0).any()
    vid, box = c['ids'][0], plan['boxes'][0]
    region = [int(v) for v in c[vid]['region']]
    cvol, lvol = _dev(c['crop_ct'][0]), _dev(c['crop_label'][0])
    outs = []
    for entry, extra in (('hv_restore_volume', ()), ('hv_restore_volume_sp', (ones,))):
        ct_out = torch.zeros(X, Y, Z, dtype=torch.float64, device='cuda')
        lab_out = torch.zeros(X, Y, Z, dtype=torch.uint8, device='cuda')
        cov = torch.zeros(X, Y, Z, dtype=torch.uint8, device='cuda')
        loc = torch.zeros(*region[3:], 3, dtype=torch.float64, device='cuda')
        L.call(entry, _lib.ptr(cvol), S._DT[cvol.dtype], *st(cvol), _lib.ptr(lvol), *st(lvol), *cvol.shape, (ctypes.c_int * 9)(*box),
               _lib.ptr(d_knots), _lib.ptr(d_basis), _lib.ptr(d_cum), N, ctypes.c_double(64.0), ctypes.c_double(64.0), _lib.ptr(tlab), 0,
               *st(tlab), X, Y, Z, (ctypes.c_int * 6)(*region), S.RESTORE['vertebra'], vid, _lib.ptr(ct_out), *st(ct_out), _lib.ptr(lab_out),
               *st(lab_out), _lib.ptr(cov), *st(cov), _lib.ptr(loc), *extra, _lib.stream())
        outs.append((ct_out, lab_out, cov, loc.view(torch.int64)))
    assert all(torch.equal(a, b) for a, b in zip(*outs)) and outs[0][2].any()
    # HV_ERR_ARG: nothing launched, nothing written
    pts, out = _dev(np.ones((5, 3))), torch.full((5, 3), 7.0, dtype=torch.float64, device='cuda')
    args = lambda sp, direction, n=N: (_lib.ptr(pts), ctypes.c_longlong(5), _lib.ptr(d_knots), _lib.ptr(d_basis), _lib.ptr(d_cum), n,  # noqa: E731
                                       ctypes.c_double(64.0), ctypes.c_double(64.0), sp, direction, _lib.ptr(out), _lib.stream())
    for sp, direction, n in ((None, 0, N), ((ctypes.c_double * 3)(1.0, 0.0, 1.0), 0, N), ((ctypes.c_double * 3)(1.0, float('inf'), 1.0), 1, N),
                             ((ctypes.c_double * 3)(1.0, float('nan'), 1.0), 1, N), (ones, 2, N), (ones, -1, N), (ones, 0, 1)):
        assert L.cdll.hv_curve_points(*args(sp, direction, n)) == -1
    torch.cuda.synchronize()
    assert (out == 7.0).all()


@pytest.mark.parametrize('name', CURVED)
def test_restore_with_spacing_matches_the_reference(name):
    from scipy.ndimage import map_coordinates
    from hvgan import straighten as S
    c = _g()[name]
    plan = SR.plan_of(c)
    b = c['box']
    vid = b['vid']
    crops = {vid: (_dev(c['crop_ct'][0]), _dev(c['crop_label'][0]))}
    ct_out, lab_out, covered, local = S.restore_patient(plan, crops, shape=c['ct'].shape, where='crop', return_covered=True, return_local=True)
    torch.cuda.synchronize()
    region, loc = local[vid]
    assert list(region) == [int(v) for v in b['region']]
    got, ref, margin = loc.cpu().numpy(), b['local'], b['margin']
    # the margin logic of tests/test_restore_gpu.py::_check_local
    keep = margin >= MARGIN_DELTA
    assert (~keep).mean() <= SR.MARGIN_CAP, name
    fin = np.isfinite(ref).all(-1)
    assert np.isnan(got[keep & ~fin]).all(), name
    err = np.abs(got - ref)[keep & fin]
    print(name, 'voxels', keep.size, 'kept', int(keep.sum()), 'max |local - reference| %.3g' % err.max())
    assert np.isfinite(got[keep & fin]).all() and err.max() <= LOCAL_TOL, (name, err.max())
    sl = _sl(region)
    ct_out, lab_out, covered = ct_out.cpu().numpy(), lab_out.cpu().numpy(), covered.cpu().numpy().astype(bool)
    assert np.array_equal(covered[sl][keep], b['covered'][keep]), name
    m = keep & b['covered']
    c_ref, _ = R.crop_coords(ref, plan['boxes'][0])
    scipy_ct = map_coordinates(c['crop_ct'][0], c_ref[m].T, order=1)
    assert np.array_equal(scipy_ct, b['sample_ct'][m])
    err = np.abs(ct_out[sl][m] - scipy_ct).max()
    print(name, 'covered', int(m.sum()), 'max |ct - scipy| %.3g' % err)
    assert m.any() and err <= CT_TOL, (name, err)
    m = b['covered'] & (b['margin_label'] >= MARGIN_DELTA)
    assert np.array_equal(lab_out[sl][m], b['sample_label'][m]), name
    outside = np.ones(covered.shape, dtype=bool)
    outside[sl] = False
    assert not covered[outside].any() and (ct_out[outside] == 0).all() and (lab_out[outside] == 0).all()


def test_affine_round_trip_at_aniso():
    """A CT that is affine in millimetres, straightened at (0.7, 0.7, 1.5) along collinear centroids and restored: the ramp on the covered
    voxels, to the bound of tests/test_restore_gpu.py::test_affine_round_trip (1e-9)."""
    import hvgan  # noqa: F401
    from hvgan import straighten as S
    sp = np.array([0.7, 0.7, 1.5])
    shape, p0, p1, out_size = (64, 64, 96), np.array([27.0, 30.0, 27.0]), np.array([36.0, 34.0, 63.0]), (40, 24, 12)
    ids = [1, 2, 3, 4]
    cents = [{'label': i, 'X': float(p[0]), 'Y': float(p[1]), 'Z': float(p[2])} for i, p in zip(ids, (p0 + (p1 - p0) * t for t in (0, 1 / 3, 2 / 3, 1)))]
    x, y, z = np.meshgrid(*(np.arange(s, dtype=np.float64) * f for s, f in zip(shape, sp)), indexing='ij')
    ramp = 1.75 * x - 2.5 * y + 0.625 * z + 40.0
    assert ramp.min() > -300 and ramp.max() < 800
    label = np.zeros(shape, dtype=np.uint8)
    for e in cents:
        label[int(e['X']) - 1:int(e['X']) + 2, int(e['Y']) - 1:int(e['Y']) + 2, int(e['Z']) - 1:int(e['Z']) + 2] = e['label']
    want = [2, 3]
    crops, plan = S.straighten_patient(_dev(ramp), _dev(label), want, centroids=cents, out_size=out_size, return_plan=True, spacing=tuple(sp))
    assert not plan['window'] and plan['spacing'] == tuple(sp)
    assert np.abs(plan['basis'] - plan['basis'][0]).max() <= 1e-12            # constant frames: the extension was not clamped
    ct_out, lab_out, covered = S.restore_patient(plan, crops, shape=shape, where='crop', return_covered=True)
    torch.cuda.synchronize()
    ct_out, covered = ct_out.cpu().numpy(), covered.cpu().numpy().astype(bool)
    checked = 0
    for vid, box in zip(want, plan['boxes']):
        region = S.restore_box(plan['knots'], plan['basis'], box, shape, spacing=tuple(sp))
        keep = np.zeros(shape, dtype=bool)            # 2 away from the box border and from the volume border
        keep[tuple(slice(max(region[i], 0) + 2, min(region[i] + region[3 + i], shape[i]) - 2) for i in range(3))] = True
        keep[:2], keep[-2:], keep[:, :2], keep[:, -2:], keep[:, :, :2], keep[:, :, -2:] = (False,) * 6
        m = keep & covered
        checked += int(m.sum())
        err = np.abs(ct_out - ramp)[m].max()
        print(vid, 'N', len(plan['knots']), 'region', region, 'checked', int(m.sum()), 'max |ct - ramp| %.3g' % err)
        assert err <= CT_TOL, (vid, err)
    assert checked > 1000
    assert (ct_out[~covered] == 0).all() and (lab_out.cpu().numpy()[~covered] == 0).all()


@pytest.mark.parametrize('name', CURVED)
def test_points_between_the_two_spaces_match_the_reference(name):
    from hvgan import straighten as S
    c = _g()[name]
    plan = SR.plan_of(c)
    lat = c['lattice']
    x = np.ascontiguousarray(lat['local'])
    glob = S.points_to_global(plan, x)
    assert glob.is_cuda and glob.dtype == torch.float64 and tuple(glob.shape) == x.shape
    keep = lat['margin'] >= MARGIN_DELTA
    err = np.abs(glob.cpu().numpy() - lat['global'])[keep].max()
    print(name, 'points', len(x), 'max |points_to_global - reference| %.3g' % err)
    assert (~keep).mean() <= SR.MARGIN_CAP and err <= GLOBAL_TOL, (name, err)
    # numpy and device-tensor input: the same bytes
    assert torch.equal(S.points_to_global(plan, _dev(x)), glob)
    # global -> local at the reference's global points, against the reference's own way back
    back = S.points_to_local(plan, lat['global'])
    assert torch.equal(S.points_to_local(plan, _dev(lat['global'])).view(torch.int64), back.view(torch.int64))
    keep_r = lat['round_margin'] >= MARGIN_DELTA
    fin = np.isfinite(lat['round']).all(-1)
    assert (~keep_r).mean() <= SR.MARGIN_CAP
    assert np.isnan(back.cpu().numpy()[keep_r & ~fin]).all()
    err = np.abs(back.cpu().numpy() - lat['round'])[keep_r & fin].max()
    print(name, 'max |points_to_local - reference| %.3g' % err)
    assert err <= LOCAL_TOL, (name, err)
    # the round trip on the device returns x inside the curve's range wherever the reference's own round trip does (on a bent curve the
    # two maps interpolate between different pairs of planes and are inverse only to first order: the reference's own error is the bound)
    cum = S.cumulative_length(plan['knots'])
    inside = (x[:, 0] > cum[1]) & (x[:, 0] < cum[-2]) & keep & keep_r & fin
    rt = S.points_to_local(plan, glob).cpu().numpy()
    ref_err = np.abs(lat['round'] - x)[inside].max(-1)
    dev_err = np.abs(rt - x)[inside].max(-1)
    print(name, 'inside', int(inside.sum()), 'round trip: reference %.3g device %.3g' % (ref_err.max(), dev_err.max()))
    assert inside.sum() > 50 and (dev_err <= ref_err + LOCAL_TOL + GLOBAL_TOL * 4).all()
    # M = 1 and an M that is no multiple of the block (512)
    one = S.points_to_global(plan, x[5:6])
    assert torch.equal(one, glob[5:6])
    many = np.tile(x, (3, 1))[:len(x) * 3 - 7]
    assert len(many) > 512 and len(many) % 512 != 0
    assert torch.equal(S.points_to_global(plan, many), glob.repeat(3, 1)[:len(many)])


def test_points_on_a_straight_curve_global_memory_path_and_single():
    """More than 630 knots (the knots are read from global memory): a long straight centroid list at a large axis-0 spacing, built by plan();
    no volume is needed.  On a straight curve the frames are constant and the two maps are affine inverses of each other: the round trip
    returns x up to rounding.  Bound: coordinates up to 2^10 mm, some 30 operations each way with unit-length frame vectors, 2^-53
    relative each: 60 * 2^10 * 1.1e-16 < 1e-11; 1e-10 leaves a decade."""
    import hvgan  # noqa: F401
    from hvgan import straighten as S
    sp = (8.0, 1.0, 1.0)
    cents = [{'label': i + 1, 'X': 30.0 + 25.0 * i, 'Y': 30.0 + 2.0 * i, 'Z': 40.0 + 1.0 * i} for i in range(4)]     # the 20-voxel extension is not clamped
    p = S.plan(cents, (140, 80, 80), [2], (16, 16, 8), spacing=sp)
    N = len(p[0])
    assert N > 630 and p.spacing == sp and np.abs(p[1] - p[1][0]).max() <= 1e-12
    cum = S.cumulative_length(p[0])
    rng = np.random.RandomState(0)
    x = np.stack([rng.uniform(cum[2], cum[-3], 700), 64 + rng.uniform(-20, 20, 700), 64 + rng.uniform(-20, 20, 700)], -1)
    glob = S.points_to_global(p, x)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        host = S.local_to_global(x[:40], p[0], p[1], SR.PLANE, sp)
        host_back = np.array([S.global_to_local(q, p[0], p[1], SR.PLANE, sp) for q in host])
    assert np.abs(glob.cpu().numpy()[:40] - host).max() <= GLOBAL_TOL
    back = S.points_to_local(p, glob)
    assert np.abs(back.cpu().numpy()[:40] - host_back).max() <= LOCAL_TOL * 8         # the host's input differs from glob by GLOBAL_TOL * 8 mm
    err = np.abs(back.cpu().numpy() - x).max()
    print('knots', N, 'round trip max |x - local(global(x))| %.3g' % err)
    assert err <= 1e-10
    # a single-centroid plan: both are the identity
    one = S.plan(cents[:1], (140, 80, 80), [1], (16, 16, 8), spacing=sp)
    assert one[0] is None
    pts = rng.uniform(0, 50, (9, 3))
    for f in (S.points_to_local, S.points_to_global):
        r = f(one, pts)
        assert r.is_cuda and np.array_equal(r.cpu().numpy(), pts)
        t = _dev(pts)
        r = f({'knots': None, 'basis': None, 'spacing': sp}, t)
        assert torch.equal(r, t) and r.data_ptr() != t.data_ptr()


def test_layouts_and_dtypes_give_the_same_bytes_at_aniso():
    from hvgan import straighten as S
    c, want, _ = _straighten('aniso')
    assert c['ct'].dtype == np.int16

    def same(ct, label):
        got = S.straighten_patient(ct, label, c['ids'], out_size=c['out_size'], spacing=c['spacing'])
        for v in c['ids']:
            assert torch.equal(got[v][0], want[v][0]) and torch.equal(got[v][1], want[v][1])

    f64 = _dev(c['ct'].astype(np.float64))
    same(f64, _dev(c['label']))                                                   # the contiguous float64 patient
    fct = torch.from_numpy(np.asfortranarray(c['ct'])).cuda()                     # int16, Fortran order
    flab = torch.from_numpy(np.asfortranarray(c['label'])).cuda()
    assert fct.stride()[0] == 1 and fct.dtype == torch.int16 and flab.stride()[0] == 1
    same(fct, flab)
    same(torch.from_numpy(np.asfortranarray(c['ct'].astype(np.float64))).cuda(), _dev(c['label'].astype(np.float64)))


def test_bad_spacing_raises_and_a_following_call_gives_the_right_bytes():
    from hvgan import straighten as S
    c, want, plan = _straighten('aniso')
    tct, tlab = _dev(c['ct']), _dev(c['label'])
    for sp in ((0.7, 0.0, 1.5), (0.7, float('nan'), 1.5), (0.7, 1.5), ([0.0, 0.7], 0.7, 1.5), -1.0):
        with pytest.raises(ValueError):
            S.straighten_patient(tct, tlab, c['ids'], out_size=c['out_size'], spacing=sp)
        with pytest.raises(ValueError):
            S.restore_patient(plan, want, shape=c['ct'].shape, where='crop', spacing=sp)
        with pytest.raises(ValueError):
            S.points_to_local(dict(plan, spacing=sp), _dev(np.zeros((3, 3))))
    with pytest.raises(ValueError):
        S.restore_patient(plan, want, shape=c['ct'].shape, where='crop', spacing=(1.0, 1.0, 1.0))
    got = S.straighten_patient(tct, tlab, c['ids'], out_size=c['out_size'], spacing=list(c['spacing']))
    for v in c['ids']:
        assert torch.equal(got[v][0], want[v][0]) and torch.equal(got[v][1], want[v][1])
    a = S.restore_patient(plan, want, shape=c['ct'].shape, where='crop', return_covered=True)
    b = S.restore_patient(plan, want, shape=c['ct'].shape, where='crop', return_covered=True, spacing=c['spacing'])
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and a[2].any()
