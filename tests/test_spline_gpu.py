"""Cubic B-spline (order=3) resampling on the device -- hv_spline_prefilter (csrc/spline.hip), the cubic forms of the straightening sampler and
the restore (csrc/spline_tap.h in csrc/straighten.hip, csrc/restore.hip) and order= of hvgan.straighten -- against the numpy restatement
(tests/spline_ref.py), scipy.ndimage and the reference's own order=3 crops (fixture G23).

SPLINE_TOL = 1e-9 for data of magnitude up to 255 (tests/test_spline_cpu.py: 10 x the measured 2.8e-12 / 2.9e-13 is below the 1e-9 floor), scaled
by max|data| / 255 for larger data."""
import ctypes

import numpy as np
import pytest
import torch

import restore_ref as R
import spacing_ref as SR
import spline_ref as P

pytestmark = pytest.mark.gpu

SPLINE_TOL = 1e-9
GUARD = 64
_CACHE = {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _st(t):
    return [ctypes.c_longlong(s) for s in t.stride()]


def _lib():
    import hvgan  # noqa: F401
    from hvgan import lib
    assert P.SPLINE_TOL == SPLINE_TOL
    return lib, lib.get()


def _prefilter_guarded(src, dims, win):
    """hv_spline_prefilter of the [dims] box at src's first element into the middle of a NaN buffer -> (coef numpy, the buffer's int64 bits)."""
    lib, L = _lib()
    from hvgan import straighten as S
    total = int(np.prod(dims))
    buf = torch.full((total + 2 * GUARD,), float('nan'), dtype=torch.float64, device='cuda')
    coef = buf[GUARD:GUARD + total]
    L.call('hv_spline_prefilter', lib.ptr(src), S._DT[src.dtype], *_st(src), *(int(d) for d in dims), int(win), ctypes.c_double(P.WINDOW[0]),
           ctypes.c_double(P.WINDOW[1]), lib.ptr(coef), lib.stream())
    torch.cuda.synchronize()
    assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[GUARD + total:]).all(), 'the NaN border did not survive'
    return coef.cpu().numpy().reshape(dims), buf.view(torch.int64).clone()


# ------------------------------------------------------------------------------------------------ prefilter
@pytest.mark.parametrize('case', list(enumerate(P.prefilter_shapes())), ids=lambda c: 'x'.join(str(d) for d in c[1]))
def test_prefilter_edges(case):
    k, shape = case
    v = P.case_volume(shape, k)
    refs = {0: P.spline_filter3(v), 1: P.spline_filter3(P.window(v))}
    for dt in (np.int16, np.float32, np.float64):
        src = _dev(v.astype(dt))
        for win in (0, 1):
            got, bits = _prefilter_guarded(src, shape, win)
            tol = SPLINE_TOL * P.scale_of(P.window(v) if win else v)
            err = np.abs(got - refs[win]).max()
            print(shape, np.dtype(dt).name, 'window', win, 'max |coef - restatement| %.3g (tol %.3g)' % (err, tol))
            assert err <= tol, (shape, dt, win, err)
            _, again = _prefilter_guarded(src, shape, win)
            assert torch.equal(bits, again), 'two runs differ'


def test_prefilter_of_a_permuted_view_and_of_a_sub_box():
    from hvgan import straighten as S
    _lib()
    v = P.case_volume((12, 70, 9), 40)
    ref = P.spline_filter3(v)
    # the same values laid out [Z][X][Y] in memory, handed over as the [X][Y][Z] view
    for dt in (np.int16, np.float64):
        perm = _dev(v.astype(dt).transpose(2, 0, 1)).permute(1, 2, 0)
        assert tuple(perm.shape) == v.shape and not perm.is_contiguous()
        got, _ = _prefilter_guarded(perm, v.shape, 0)
        assert np.abs(got - ref).max() <= SPLINE_TOL * P.scale_of(v)
        api = S.spline_coefficients(perm)
        assert api.dtype == torch.float64 and api.is_contiguous() and np.array_equal(api.cpu().numpy(), got)
    api = S.spline_coefficients(_dev(v.astype(np.float32)), window=P.WINDOW)
    assert np.abs(api.cpu().numpy() - P.spline_filter3(P.window(v))).max() <= SPLINE_TOL
    # a sub-box: the pointer of its first element and the strides of the array it lies in; mirrored at its own edges
    big = _dev(v)
    sub = big[2:7, 3:68, 1:8]
    assert sub.data_ptr() != big.data_ptr()
    got, _ = _prefilter_guarded(sub, (5, 65, 7), 0)
    assert np.abs(got - P.spline_filter3(v[2:7, 3:68, 1:8])).max() <= SPLINE_TOL * P.scale_of(v)


# ------------------------------------------------------------------------------------------------ the cubic straightening sampler
def _sample(v, label, knots, basis, PA, PB, spacing=(1.0, 1.0, 1.0), order=3, win=0):
    """The straight volumes [N][PA][PB] of one sampling call (order 3: prefilter + hv_straighten_sample_spline; order 1:
    hv_straighten_sample_sp) -> (ct numpy, label tensor, presence tensor)."""
    lib, L = _lib()
    from hvgan import straighten as S
    tv, tl = _dev(v), _dev(label)
    N = len(knots)
    dk, db = _dev(np.asarray(knots, dtype=np.float64)), _dev(np.asarray(basis, dtype=np.float64))
    sct = torch.full((N, PA, PB), -7.0, dtype=torch.float64, device='cuda')
    slab = torch.full((N, PA, PB), 255, dtype=torch.uint8, device='cuda')
    pbytes = L.size('hv_straighten_presence_bytes', PA)
    pres = torch.full((pbytes // 8,), -1, dtype=torch.int64, device='cuda')
    sp = (ctypes.c_double * 3)(*spacing)
    wmin, wmax = ctypes.c_double(P.WINDOW[0]), ctypes.c_double(P.WINDOW[1])
    if order == 3:
        coef = S.spline_coefficients(tv, window=P.WINDOW if win else None)
        L.call('hv_straighten_sample_spline', lib.ptr(coef), lib.ptr(tl), S._DT[tl.dtype], *_st(tl), *v.shape, lib.ptr(dk), lib.ptr(db), N, PA,
               PB, lib.ptr(sct), lib.ptr(slab), lib.ptr(pres), ctypes.c_size_t(pbytes), sp, lib.stream())
    else:
        L.call('hv_straighten_sample_sp', lib.ptr(tv), S._DT[tv.dtype], *_st(tv), lib.ptr(tl), S._DT[tl.dtype], *_st(tl), *v.shape, lib.ptr(dk),
               lib.ptr(db), N, PA, PB, win, wmin, wmax, lib.ptr(sct), lib.ptr(slab), lib.ptr(pres), ctypes.c_size_t(pbytes), sp, lib.stream())
    torch.cuda.synchronize()
    return sct.cpu().numpy(), slab, pres


def _identity_frame(n):
    return np.tile(np.eye(3), (n, 1, 1))


def _labels(shape, seed=0):
    return np.random.RandomState(seed).randint(0, 4, size=shape).astype(np.uint8)


def test_lattice_points_give_the_voxels_and_half_offsets_match_scipy():
    from scipy.ndimage import map_coordinates
    shape = (14, 12, 16)
    v = P.window(P.case_volume(shape, 50))
    lab = _labels(shape)
    PA, PB = 8, 6
    knots = np.array([[n + 2.0, 5.0, 6.0] for n in range(9)])
    got, slab, pres = _sample(v, lab, knots, _identity_frame(9), PA, PB)
    # sample (n, a, b) lies at (n + 2, 5 + b - PB / 2, 6 + a - PA / 2): lattice points, where the cubic spline is the voxel itself
    want = v[2:11, 2:8, 2:10].transpose(0, 2, 1)
    err = np.abs(got - want).max()
    print('lattice: max |straight - voxel| %.3g' % err)
    assert got.shape == want.shape and err <= SPLINE_TOL
    assert np.array_equal(slab.cpu().numpy(), lab[2:11, 2:8, 2:10].transpose(0, 2, 1))
    # labels and presence bits: those of the order-1 call, bit for bit
    _, slab1, pres1 = _sample(v, lab, knots, _identity_frame(9), PA, PB, order=1)
    assert torch.equal(slab, slab1) and torch.equal(pres, pres1)
    half = knots + 0.5
    got, _, _ = _sample(v, lab, half, _identity_frame(9), PA, PB)
    grid = P.straight_grid(half, _identity_frame(9), (1.0, 1.0, 1.0), plane=(PB, PA))
    ref = map_coordinates(v, grid, order=3, mode='constant', cval=0.0)
    err = np.abs(got - ref).max()
    print('half-voxel offset: max |straight - scipy| %.3g' % err)
    assert err <= SPLINE_TOL and np.abs(got - P.map_coordinates3(v, grid)).max() <= SPLINE_TOL


def test_boundary_rule_matches_scipy():
    """Identity frame: axis 0 of the sample is the knot's, axis 1 runs over ky + (b - PB / 2), axis 2 over kz + (a - PA / 2).  With PB = 11,
    ky = 5.5 the axis-1 coordinates are 0 .. 10 = D1 - 1 exactly; with PA = 14, kz = 7 the axis-2 coordinates are 0 .. 13, the last one past
    D2 - 1 = 12; the knots put axis 0 exactly at 0, at D0 - 1, just past it, and inside the last cell (the tap at D0 mirrors to D0 - 2)."""
    from scipy.ndimage import map_coordinates
    shape = (9, 11, 13)
    v = P.window(P.case_volume(shape, 51))
    xs = [0.0, 8.0, 8.0 + 1e-7, 7.5, 7.999999, 4.0]
    knots = np.array([[x, 5.5, 7.0] for x in xs])
    PA, PB = 14, 11
    got, slab, _ = _sample(v, _labels(shape, 1), knots, _identity_frame(len(xs)), PA, PB)
    grid = P.straight_grid(knots, _identity_frame(len(xs)), (1.0, 1.0, 1.0), plane=(PB, PA))
    assert grid[1].min() == 0.0 and grid[1].max() == 10.0 and grid[2].min() == 0.0 and grid[2].max() == 13.0 and grid[0, 1].max() == 8.0
    ref = map_coordinates(v, grid, order=3, mode='constant', cval=0.0)
    err = np.abs(got - ref).max()
    print('borders: max |straight - scipy| %.3g' % err)
    assert err <= SPLINE_TOL
    assert (got[2] == 0.0).all() and (slab[2] == 0).all()             # just past D0 - 1: outside
    assert (got[:, 13, :] == 0.0).all()                               # axis 2 at 13 > D2 - 1
    assert np.abs(got[1, :13, :] - v[8, :, :].T).max() <= SPLINE_TOL  # exactly at D0 - 1 (and at 0 and D1 - 1 on axis 1): the voxels
    assert np.abs(got[0, :13, :] - v[0, :, :].T).max() <= SPLINE_TOL
    assert (got[3, :13] != 0.0).any() and (got[4, :13] != 0.0).any()


def test_a_quadratic_comes_back_under_order_3_and_not_under_order_1():
    """What the feature is for.  A quadratic CT on 40^3 sampled along a bent curve through the middle, 8 x 8 planes: every sample lies at least
    K voxels from every face.  The spline of mirrored data departs from the polynomial near a face and the departure decays as |z|^k with
    the distance k (|z| = 0.268): the bound asserted is max|data| * |z|^K, for scipy on the host first (the margin is a condition) and for the
    device with SPLINE_TOL on top.  Trilinear sampling of the same points misses the polynomial by about q'' / 8 per axis."""
    from scipy.ndimage import map_coordinates
    from hvgan import straighten as S
    D = 40
    x, y, z = np.meshgrid(*(np.arange(D, dtype=np.float64),) * 3, indexing='ij')

    def poly(x, y, z):
        return 20.0 + 0.11 * x * x - 0.07 * y * y + 0.09 * z * z + 0.05 * x * y - 0.06 * y * z + 0.3 * x - 0.2 * z

    v = poly(x, y, z)
    curve = np.array([[17.0, 18.0, 14.0], [19.0, 19.5, 18.0], [22.0, 20.0, 22.0], [23.0, 21.0, 26.0]])
    knots, basis = S.curve_frame(curve)
    assert np.abs(basis - basis[0]).max() > 0.05                      # a curved frame
    PA = PB = 8
    grid = P.straight_grid(knots, basis, (1.0, 1.0, 1.0), plane=(PB, PA))
    K = int(np.floor(min(grid.min(), (D - 1) - grid.max())))
    bound = np.abs(v).max() * abs(P.Z) ** K
    want = poly(*grid)
    sci = np.abs(map_coordinates(v, grid, order=3, mode='constant', cval=0.0) - want).max()
    print('margin', K, 'bound %.3g' % bound, 'scipy order 3 max |sample - polynomial| %.3g' % sci)
    assert K >= 8 and sci <= bound
    lab = np.zeros(v.shape, dtype=np.uint8)
    got3, _, _ = _sample(v, lab, knots, basis, PA, PB)
    got1, _, _ = _sample(v, lab, knots, basis, PA, PB, order=1)
    e3, e1 = np.abs(got3 - want).max(), np.abs(got1 - want).max()
    print('device max |sample - polynomial|: order 3 %.3g, order 1 %.3g' % (e3, e1))
    assert e3 <= bound + SPLINE_TOL * P.scale_of(v)
    assert e1 > 1e-2 and e1 > 100 * (bound + SPLINE_TOL * P.scale_of(v))


# ------------------------------------------------------------------------------------------------ straighten_patient / restore_patient
def _g23():
    if 'g23' not in _CACHE:
        _lib()
        _CACHE['g23'] = P.load_g23()
    return _CACHE['g23']


@pytest.mark.parametrize('name', ['iso', 'thick', 'aniso'])
def test_straighten_patient_order_3_matches_the_reference(name):
    from hvgan import straighten as S
    c = _g23()[name]
    tct, tlab = _dev(c['ct']), _dev(c['label'])
    crops, plan = S.straighten_patient(tct, tlab, c['ids'], out_size=c['out_size'], return_plan=True, spacing=c['spacing'], order=3)
    lin, plan1 = S.straighten_patient(tct, tlab, c['ids'], out_size=c['out_size'], return_plan=True, spacing=c['spacing'])
    torch.cuda.synchronize()
    assert plan['order'] == 3 and plan1['order'] == 1 and plan['window'] == c['window'] and plan['spacing'] == c['spacing']
    assert np.array_equal(np.array(plan['boxes']), c['boxes'])
    for k, vid in enumerate(c['ids']):
        ct, lab = crops[vid]
        assert ct.dtype == torch.float64 and lab.dtype == torch.uint8 and tuple(ct.shape) == c['out_size']
        err = np.abs(ct.cpu().numpy() - c['crop_ct'][k]).max()
        print(name, vid, 'max |ct - G23| %.3g' % err, 'labels differing from G23', int((lab.cpu().numpy() != c['crop_label'][k]).sum()))
        assert err <= SPLINE_TOL, (name, vid, err)
        assert torch.equal(lab, lin[vid][1]) and (lab != 0).any()            # labels: the order-1 call's, bit for bit
        assert not torch.equal(ct, lin[vid][0])


def _restore_case(name):
    """A G21 case, its host plan with order 3, the first vertebra's crops on the device."""
    if ('g21', name) not in _CACHE:
        _lib()
        c = SR.load_g21()[name]
        plan = SR.plan_of(c)
        vid = c['box']['vid']
        _CACHE[('g21', name)] = (c, plan, vid, {vid: (_dev(c['crop_ct'][0]), _dev(c['crop_label'][0]))})
    return _CACHE[('g21', name)]


@pytest.mark.parametrize('name', ['aniso', 'thick'])
def test_restore_reads_order_3_from_the_plan_and_matches_scipy(name):
    from scipy.ndimage import map_coordinates
    from hvgan import straighten as S
    c, plan, vid, crops = _restore_case(name)
    b = c['box']
    kw = dict(shape=c['ct'].shape, where='crop', return_covered=True, return_local=True)
    ct3, lab3, cov3, loc3 = S.restore_patient(dict(plan, order=3), crops, **kw)
    ct1, lab1, cov1, loc1 = S.restore_patient(plan, crops, **kw)
    ctx, _, _, _ = S.restore_patient(dict(plan, order=1), crops, order=3, **kw)            # an explicit order overrides the plan's
    torch.cuda.synchronize()
    assert torch.equal(ctx, ct3) and not torch.equal(ct3, ct1)
    # labels, the covered mask and the local coordinates: the order-1 restore's, bit for bit
    assert torch.equal(lab3, lab1) and torch.equal(cov3, cov1) and cov3.any()
    assert loc3[vid][0] == loc1[vid][0] == [int(x) for x in b['region']]
    assert torch.equal(loc3[vid][1].view(torch.int64), loc1[vid][1].view(torch.int64))
    # the CT against scipy order 3 on the filled sub-box at the reference's coordinates (the margin logic of tests/test_spacing_gpu.py)
    box = [int(x) for x in plan['boxes'][0]]
    sub = c['crop_ct'][0][box[6]:box[6] + box[3], box[7]:box[7] + box[4], box[8]:box[8] + box[5]]
    c_ref, _ = R.crop_coords(b['local'], box)
    m = (b['margin'] >= SR.MARGIN_DELTA) & b['covered']
    ref = map_coordinates(sub, (c_ref[m] - np.array(box[6:9], dtype=np.float64)).T, order=3, mode='constant', cval=0.0)
    sl = tuple(slice(int(b['region'][i]), int(b['region'][i] + b['region'][3 + i])) for i in range(3))
    err = np.abs(ct3.cpu().numpy()[sl][m] - ref).max()
    print(name, 'covered', int(m.sum()), 'max |ct - scipy order 3| %.3g' % err)
    assert m.sum() > 100 and err <= SPLINE_TOL * P.scale_of(sub), (name, err)
    keep = b['margin'] >= SR.MARGIN_DELTA
    assert np.array_equal(cov3.cpu().numpy().astype(bool)[sl][keep], b['covered'][keep])


def test_round_trip_of_a_smooth_patient_is_closer_under_order_3():
    """scan -> crops -> scan at spacing (0.7, 0.7, 1.5) along collinear centroids (the layout of tests/test_spacing_gpu.py's affine round trip)
    for a smooth CT inside the window: compared on the covered voxels whose crop coordinate lies at least 5 voxels inside the filled part
    (the mirror at the sub-box's edges decays as 0.268^k), the largest error is smaller with order 3 than with order 1."""
    _lib()
    from hvgan import straighten as S
    sp = np.array([0.7, 0.7, 1.5])
    shape, p0, p1, out_size = (64, 64, 96), np.array([27.0, 30.0, 27.0]), np.array([36.0, 34.0, 63.0]), (40, 24, 12)
    ids = [1, 2, 3, 4]
    cents = [{'label': i, 'X': float(p[0]), 'Y': float(p[1]), 'Z': float(p[2])} for i, p in zip(ids, (p0 + (p1 - p0) * t for t in (0, 1 / 3, 2 / 3, 1)))]
    x, y, z = np.meshgrid(*(np.arange(s, dtype=np.float64) * f for s, f in zip(shape, sp)), indexing='ij')
    smooth = 200.0 + 80.0 * np.sin(x / 4.0) * np.cos(y / 5.0) + 60.0 * np.sin(z / 3.0)
    assert smooth.min() > -300 and smooth.max() < 800
    label = np.zeros(shape, dtype=np.uint8)
    for e in cents:
        label[int(e['X']) - 1:int(e['X']) + 2, int(e['Y']) - 1:int(e['Y']) + 2, int(e['Z']) - 1:int(e['Z']) + 2] = e['label']
    tct, tlab = _dev(smooth), _dev(label)
    errs = {}
    for order in (1, 3):
        crops, plan = S.straighten_patient(tct, tlab, [2], centroids=cents, out_size=out_size, return_plan=True, spacing=tuple(sp), order=order)
        assert not plan['window'] and plan['order'] == order
        ct_out, _, covered, local = S.restore_patient(plan, crops, shape=shape, where='crop', return_covered=True, return_local=True)
        torch.cuda.synchronize()
        region, loc = local[2]
        box = [int(v) for v in plan['boxes'][0]]
        cc, cov = R.crop_coords(loc.cpu().numpy(), box)
        lo = np.array(box[6:9], dtype=np.float64)
        hi = lo + np.array(box[3:6]) - 1
        with np.errstate(invalid='ignore'):
            inner = cov & (np.minimum(cc - lo, hi - cc).min(-1) >= 5.0)
        sl = tuple(slice(region[i], region[i] + region[3 + i]) for i in range(3))
        assert covered.cpu().numpy().astype(bool)[sl][inner].all() and inner.sum() > 500
        errs[order] = float(np.abs(ct_out.cpu().numpy()[sl] - smooth[sl])[inner].max())
        errs[order, 'n'] = int(inner.sum())
    print('round trip max error: order 1 %.4g, order 3 %.4g over %d voxels' % (errs[1], errs[3], errs[3, 'n']))
    assert errs[1, 'n'] == errs[3, 'n'] and errs[3] < errs[1]


def test_order_1_explicit_and_defaulted_gives_the_bytes_of_the_plain_entries():
    lib, L = _lib()
    from hvgan import straighten as S
    c = R.load_g20()['curved']
    tct, tlab = _dev(c['ct']), _dev(c['label'])
    a, pa = S.straighten_patient(tct, tlab, c['ids'], out_size=c['out_size'], return_plan=True)
    b, pb = S.straighten_patient(tct, tlab, c['ids'], out_size=c['out_size'], return_plan=True, order=1)
    assert pa['order'] == pb['order'] == 1
    # hv_straighten_sample_sp called directly, cropped on the host
    sct, slab, _ = _sample(c['ct'], c['label'], pa['knots'], pa['basis'], 128, 128, order=1, win=int(pa['window']))
    for k, v in enumerate(c['ids']):
        assert torch.equal(a[v][0], b[v][0]) and torch.equal(a[v][1], b[v][1])
        assert np.array_equal(a[v][0].cpu().numpy(), P.crop(sct, pa['boxes'][k], c['out_size']))
    # restore: defaulted (a plan without the entry too), explicit, and hv_restore_volume_sp called directly
    old = {k: v for k, v in pa.items() if k != 'order'}
    kw = dict(ct=tct, label=tlab, where='vertebra', return_covered=True)
    ra, rb, rc = S.restore_patient(pa, a, **kw), S.restore_patient(old, a, **kw), S.restore_patient(pa, a, order=1, **kw)
    assert all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(ra, rb, rc)) and ra[2].any()
    X, Y, Z = c['ct'].shape
    vid, box = c['ids'][0], pa['boxes'][0]
    region = S.restore_box(pa['knots'], pa['basis'], box, (X, Y, Z))
    N = len(pa['knots'])
    dk, db, dc = _dev(pa['knots']), _dev(pa['basis']), _dev(S.cumulative_length(pa['knots']))
    cvol, lvol = a[vid]
    only = S.restore_patient(pa, {vid: a[vid]}, shape=(X, Y, Z), where='crop', return_covered=True)
    ct_out = torch.zeros(X, Y, Z, dtype=torch.float64, device='cuda')
    lab_out = torch.zeros(X, Y, Z, dtype=torch.uint8, device='cuda')
    cov = torch.zeros(X, Y, Z, dtype=torch.uint8, device='cuda')
    L.call('hv_restore_volume_sp', lib.ptr(cvol), S._DT[cvol.dtype], *_st(cvol), lib.ptr(lvol), *_st(lvol), *cvol.shape, (ctypes.c_int * 9)(*box),
           lib.ptr(dk), lib.ptr(db), lib.ptr(dc), N, ctypes.c_double(64.0), ctypes.c_double(64.0), None, 0, *([ctypes.c_longlong(0)] * 3), X, Y, Z,
           (ctypes.c_int * 6)(*region), S.RESTORE['crop'], vid, lib.ptr(ct_out), *_st(ct_out), lib.ptr(lab_out), *_st(lab_out), lib.ptr(cov),
           *_st(cov), None, (ctypes.c_double * 3)(1.0, 1.0, 1.0), lib.stream())
    torch.cuda.synchronize()
    assert torch.equal(only[0], ct_out) and torch.equal(only[1], lab_out) and torch.equal(only[2], cov) and cov.any()


# ------------------------------------------------------------------------------------------------ refusals
def test_another_order_is_a_value_error_before_any_gpu_work():
    _lib()
    from hvgan import straighten as S
    c, plan, vid, crops = _restore_case('aniso')
    # host tensors: a call that got as far as the device checks would raise RuntimeError (there is no CPU path), not ValueError
    hct, hlab = torch.from_numpy(c['ct']), torch.from_numpy(c['label'])
    hcrops = {vid: (torch.from_numpy(c['crop_ct'][0]), torch.from_numpy(c['crop_label'][0]))}
    for order in (2, 0, 4, 5, 3.0, '3', True):
        with pytest.raises(ValueError):
            S.straighten_patient(hct, hlab, c['ids'], out_size=c['out_size'], spacing=c['spacing'], order=order)
        with pytest.raises(ValueError):
            S.restore_patient(plan, hcrops, shape=c['ct'].shape, where='crop', order=order)
    with pytest.raises(ValueError):
        S.restore_patient(dict(plan, order=2), hcrops, shape=c['ct'].shape, where='crop')
    tct, tlab = _dev(c['ct']), _dev(c['label'])
    before = torch.cuda.memory_allocated()
    with pytest.raises(ValueError):
        S.straighten_patient(tct, tlab, c['ids'], out_size=c['out_size'], order=2)
    assert torch.cuda.memory_allocated() == before                     # not even the stats record was allocated


def test_c_entries_refuse_bad_arguments_and_leave_guarded_outputs_untouched():
    lib, L = _lib()
    from hvgan import straighten as S
    shape = (6, 5, 7)
    src = _dev(P.case_volume(shape, 60))
    buf = torch.full((int(np.prod(shape)) + 2 * GUARD,), 7.0, dtype=torch.float64, device='cuda')
    coef = buf[GUARD:-GUARD]
    wmin, wmax = ctypes.c_double(-300.0), ctypes.c_double(800.0)

    def pre(p=lib.ptr(src), dt=5, dims=shape, out=lib.ptr(coef)):
        return L.cdll.hv_spline_prefilter(p, dt, *_st(src), *dims, 0, wmin, wmax, out, lib.stream())

    byte_off = ctypes.c_void_p(coef.data_ptr() + 4)
    for kw in (dict(p=None), dict(out=None), dict(dt=0), dict(dt=2), dict(dt=3), dict(dt=6), dict(dt=-1), dict(dims=(0, 5, 7)), dict(dims=(6, -1, 7)),
               dict(dims=(6, 5, 0)), dict(out=byte_off)):
        assert pre(**kw) == -1, kw
    # the cubic sampler: hv_straighten_sample_sp's refusals
    lab = _dev(_labels(shape))
    dk, db = _dev(np.array([[2.0, 2.0, 3.0], [3.0, 2.0, 3.0]])), _dev(_identity_frame(2))
    sct = torch.full((2, 4, 4), 7.0, dtype=torch.float64, device='cuda')
    slab = torch.full((2, 4, 4), 7, dtype=torch.uint8, device='cuda')
    pbytes = L.size('hv_straighten_presence_bytes', 4)
    pres = torch.full((pbytes // 8,), 7, dtype=torch.int64, device='cuda')
    ones = (ctypes.c_double * 3)(1.0, 1.0, 1.0)

    def smp(cf=lib.ptr(src), lb=lib.ptr(lab), ldt=0, dims=shape, k=lib.ptr(dk), bs=lib.ptr(db), n=2, pa=4, out=lib.ptr(sct), pb=pbytes, sp=ones):
        return L.cdll.hv_straighten_sample_spline(cf, lb, ldt, *_st(lab), *dims, k, bs, n, pa, 4, out, lib.ptr(slab), lib.ptr(pres),
                                                  ctypes.c_size_t(pb), sp, lib.stream())

    for kw in (dict(cf=None), dict(lb=None), dict(ldt=9), dict(dims=(6, 0, 7)), dict(k=None), dict(bs=None), dict(n=0), dict(pa=0), dict(out=None),
               dict(sp=None), dict(sp=(ctypes.c_double * 3)(1.0, 0.0, 1.0)), dict(sp=(ctypes.c_double * 3)(1.0, float('nan'), 1.0))):
        assert smp(**kw) == -1, kw
    assert smp(pb=pbytes - 8) == -3
    # the cubic restore: hv_restore_volume_sp's refusals, and no un-crop form
    c, plan, vid, crops = _restore_case('aniso')
    X, Y, Z = c['ct'].shape
    box = [int(x) for x in plan['boxes'][0]]
    region = [int(x) for x in c['box']['region']]
    lvol = crops[vid][1]
    ccoef = torch.zeros(box[3], box[4], box[5], dtype=torch.float64, device='cuda')
    N = len(plan['knots'])
    rk, rb, rc = _dev(plan['knots']), _dev(plan['basis']), _dev(S.cumulative_length(plan['knots']))
    ct_out = torch.full((X, Y, Z), 7.0, dtype=torch.float64, device='cuda')
    lab_out = torch.full((X, Y, Z), 7, dtype=torch.uint8, device='cuda')
    sp = (ctypes.c_double * 3)(*c['spacing'])

    def rst(cf=lib.ptr(ccoef), k=lib.ptr(rk), n=N, bx=box, rg=region, where=0, v=vid, out=lib.ptr(ct_out), s=sp):
        return L.cdll.hv_restore_volume_spline(cf, lib.ptr(lvol), *_st(lvol), *lvol.shape, (ctypes.c_int * 9)(*bx), k, lib.ptr(rb), lib.ptr(rc), n,
                                               ctypes.c_double(64.0), ctypes.c_double(64.0), None, 0, *([ctypes.c_longlong(0)] * 3), X, Y, Z,
                                               (ctypes.c_int * 6)(*rg), where, v, out, *_st(ct_out), lib.ptr(lab_out), *_st(lab_out), None,
                                               *([ctypes.c_longlong(0)] * 3), None, s, lib.stream())

    bad_box = box[:6] + [lvol.shape[0], box[7], box[8]]
    bad_region = region[:3] + [X + 1, region[4], region[5]]
    for kw in (dict(cf=None), dict(k=None), dict(n=1), dict(bx=bad_box), dict(rg=bad_region), dict(where=2), dict(where=1), dict(v=256), dict(out=None),
               dict(s=None), dict(s=(ctypes.c_double * 3)(1.0, -1.0, 1.0))):
        assert rst(**kw) == -1, kw
    torch.cuda.synchronize()
    assert (buf == 7.0).all() and (sct == 7.0).all() and (slab == 7).all() and (pres == 7).all()
    assert (ct_out == 7.0).all() and (lab_out == 7).all()
