"""hv_project (csrc/projection.hip) and healthivert-gan_amd/projection.py against tests/projection_ref.py (pinned on the host by
tests/test_projection_ref_cpu.py).  acc, idx and info are compared byte for byte with the restatement -- the sum's order of summation is part
of the definition -- in guarded buffers pre-filled with 0xA5 bytes.  The kernel gives a ray R lanes, R the power of two that covers its
ceil(T / 16) chunks, at most 16 when the ray runs along the volume's contiguous axis (a pass is 256 steps) and 4 when a detector axis does (a
pass is 64 steps); a workgroup takes 256 / R pixels along one detector axis."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import projection_ref as PR
import resample_ref as R
from hvtest import Guarded

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED = -1, -2
_DT = {torch.uint8: 0, torch.int16: 1, torch.int32: 2, torch.int64: 3, torch.float32: 4, torch.float64: 5}
VOL_DTYPES = (np.uint8, np.int16, np.float32, np.float64)
LABEL_DTYPES = (np.uint8, np.int16, np.int32, np.int64, np.float32, np.float64)
EDGE = (17, 18, 33)
IDENT = (np.eye(3), np.zeros(3))
OBLIQUE = (np.array([[0.9, 0.1, 0.3], [-0.1, 0.95, 0.2], [0.05, -0.2, 0.8]]), np.array([0.3, 0.5, -1.0]))


def _lib():
    import hvgan  # noqa: F401
    from hvgan import lib
    return lib, lib.get()


def _P():
    import hvgan  # noqa: F401
    from hvgan import projection
    return projection


def _dev(a):
    return torch.from_numpy(np.array(a, order='C')).cuda()


def _ll(st):
    return [ctypes.c_longlong(s) for s in st]


def _call(vol, poses, det, T, order, label=None, label_value=0.0, prefill=0xA5, **over):
    """One hv_project on device tensors -> (return code, acc, idx, info as numpy).  `over` replaces single arguments (refusal tests)."""
    lib, L = _lib()
    K = len(poses)
    flat = np.concatenate([np.concatenate([np.asarray(m, dtype=np.float64).reshape(9), np.asarray(o, dtype=np.float64)]) for m, o in poses])
    a = dict(A0=int(vol.shape[0]), A1=int(vol.shape[1]), A2=int(vol.shape[2]), K=K, P0=det[0], P1=det[1], T=T, order=order, dtype=_DT[vol.dtype],
             label_dtype=_DT[label.dtype] if label is not None else 0, label_value=label_value)
    a.update({k: v for k, v in over.items() if k in a})
    shape = (K, 3, det[0], det[1])
    g_acc, g_idx, g_info = Guarded(shape, torch.float64), Guarded(shape, torch.int32), Guarded((K, PR.INFO), torch.int64)
    for g in (g_acc, g_idx, g_info):
        g.t.view(-1).view(torch.uint8).fill_(prefill)
    nul = ctypes.c_void_p(None)

    def out(g, name):
        return nul if over.get(name + '_null') else ctypes.c_void_p(g.t.data_ptr() + over.get(name + '_off', 0))

    rc = L.cdll.hv_project(
        nul if over.get('vol_null') else ctypes.c_void_p(vol.data_ptr() + over.get('vol_off', 0)), a['dtype'], *_ll(vol.stride()), a['A0'], a['A1'],
        a['A2'], over.get('label_ptr', lib.ptr(label)), a['label_dtype'], *_ll(label.stride() if label is not None else (0, 0, 0)),
        ctypes.c_double(a['label_value']), None if over.get('poses_null') else (ctypes.c_double * len(flat))(*over.get('poses_flat', flat)), a['K'],
        a['P0'], a['P1'], a['T'], a['order'], over.get('acc_ptr', out(g_acc, 'acc')), out(g_idx, 'idx'), out(g_info, 'info'),
        ctypes.c_void_p(over.get('ws_ptr', 0)), ctypes.c_size_t(0), lib.stream())
    torch.cuda.synchronize()
    assert g_acc.intact() and g_idx.intact() and g_info.intact(), 'wrote outside a buffer'
    return rc, g_acc.t.cpu().numpy().copy(), g_idx.t.cpu().numpy().copy(), g_info.t.cpu().numpy().copy()


def _same(got, ref, what=None):
    for name, x, y in zip(('acc', 'idx', 'info'), got, ref):
        assert x.shape == y.shape and x.dtype == y.dtype, (what, name, x.shape, y.shape, x.dtype, y.dtype)
        if x.tobytes() != y.tobytes():
            bad = np.argwhere(x.view(np.int64 if x.itemsize == 8 else np.int32) != y.view(np.int64 if y.itemsize == 8 else np.int32))
            raise AssertionError((what, name, len(bad), bad[:6].tolist(), [x[tuple(b)] for b in bad[:6]], [y[tuple(b)] for b in bad[:6]]))


def _check(vol, poses, det, T, order, label=None, label_value=None, what=None, dvol=None, dlabel=None):
    """Run the entry on `vol` (numpy; order 3: the coefficients are made on the host and handed to both sides) and compare."""
    src = R.spline_filter_scipy(vol) if order == 3 else vol
    ref = PR.project_ref(vol, poses, det, T, order, label, label_value, coef=src if order == 3 else None)
    dv = _dev(src) if dvol is None else dvol
    dl = None if label is None else (_dev(label) if dlabel is None else dlabel)
    rc, acc, idx, info = _call(dv, poses, det, T, order, dl, 0.0 if label_value is None else float(label_value))
    assert rc == 0, (what, rc)
    _same((acc, idx, info), ref, what)
    for k in range(len(poses)):
        assert info[k, 1:5].sum() == det[0] * det[1] * T and idx[k, 0].sum() == info[k, 1], what
    return acc, idx, info


@functools.lru_cache(maxsize=None)
def _volume(dtype, shape=EDGE, seed=0):
    v = R.case_volume(dtype, shape, seed)
    v.setflags(write=False)
    return v


def _axis_pose(shape, view, step=1.0):
    """The volume's own lattice seen along one array axis (whole indices), the ray's step scaled by `step` -> (pose, det_shape, extent)."""
    a0, a1, ar = PR.VIEWS[view]
    m = np.zeros((3, 3))
    m[a0, 0], m[a1, 1], m[ar, 2] = 1.0, 1.0, step
    return (m, np.zeros(3)), (shape[a0], shape[a1]), shape[ar]


# ------------------------------------------------------------------------------------------------ the entry
@pytest.mark.parametrize('order', (0, 1, 3))
@pytest.mark.parametrize('dtype', VOL_DTYPES, ids=lambda d: np.dtype(d).name)
def test_dtypes_and_orders_on_an_oblique_and_an_identity_pose(dtype, order):
    vol = _volume(dtype).astype(np.float64) if order == 3 else _volume(dtype)
    _check(vol, [OBLIQUE, IDENT], (9, 11), 33, order, what=(dtype, order))


@pytest.mark.parametrize('shape', ((1, 1, 1), (5, 6, 7), EDGE), ids=str)
def test_volumes_and_detectors(shape):
    vol = _volume(np.int16, shape)
    for det in ((1, 1), (9, 11), (16, 1), (1, 64), (256, 1), (2, 65)):
        for order in (0, 1):
            _check(vol, [IDENT, OBLIQUE], det, 17, order, what=(shape, det, order))


@pytest.mark.parametrize('T', (1, 15, 16, 17, 33, 70, 260, 530))
def test_steps_along_and_across_the_contiguous_axis(T):
    """Steps of a third of a voxel (a seventeenth for the long rays) so that the rays stay inside for long: along axis 2 the ray runs along
    the lanes (a pass is 256 steps: 260 takes two, 530 three), along axes 1 and 0 a detector axis does (a pass is 64 steps: 70 takes two)."""
    vol = _volume(np.float32)
    for view in ('lateral', 'ap', 'axial'):
        pose, det, _ = _axis_pose(EDGE, view, step=1.0 / 3.0 if T <= 70 else 1.0 / 17.0)
        _check(vol, [pose], det, T, 1, what=(T, view))


@pytest.mark.parametrize('view', ('lateral', 'ap', 'axial'))
def test_identity_views_are_the_plain_sums(view):
    vol = _volume(np.int16)
    pose, det, T = _axis_pose(EDGE, view)
    ar = PR.VIEWS[view][2]
    for order in (0, 1):
        acc, idx, info = _check(vol, [pose], det, T, order, what=(view, order))
        assert (acc[0, 0] == vol.sum(axis=ar, dtype=np.int64)).all() and (idx[0, 0] == T).all() and info[0, 1] == vol.size
        assert (acc[0, 1] == vol.min(axis=ar)).all() and (acc[0, 2] == vol.max(axis=ar)).all()


@pytest.mark.parametrize('K', (1, 2, 16))
def test_pose_counts(K):
    g = np.random.default_rng(K)
    poses = [(OBLIQUE[0] + 0.05 * g.standard_normal((3, 3)), OBLIQUE[1] + g.standard_normal(3)) for _ in range(K)]
    _check(_volume(np.int16), poses, (9, 11), 33, 1, what=K)
    _check(_volume(np.uint8), poses[::-1], (9, 11), 20, 0, what=K)


def test_samples_on_the_faces_one_ulp_beyond_and_wholly_outside():
    vol = _volume(np.float64)
    hi = np.array(EDGE, dtype=np.float64) - 1.0
    zero = np.zeros((3, 3))
    on_lo, on_hi = (zero, np.zeros(3)), (zero, hi)
    below, above = (zero, np.full(3, -np.finfo(np.float64).tiny)), (zero, np.nextafter(hi, np.inf))
    one_axis = (zero, np.array([0.0, np.nextafter(17.0, np.inf), 3.0]))
    ramp = (np.array([[0, 0, 0.5], [0, 0, 0.0], [0, 0, 0.0]]), np.array([-1.0, 2.0, 3.0]))     # enters at t = 2, leaves after t = 34
    far = (np.eye(3), np.array([100.0, 0.0, 0.0]))
    for order in (0, 1, 3):
        v = vol
        acc, idx, info = _check(v, [on_lo, on_hi, below, above, one_axis, ramp, far], (2, 3), 40, order, what=order)
        assert info[:, 1].tolist() == [240, 240, 0, 0, 0, 6 * 33, 0] and info[:, 0].tolist() == [0, 0, 4, 4, 4, 0, 4]
        assert idx[5, :, 0, 0].tolist() == [33, 2, 34] and (idx[6, 1] == 40).all() and (idx[6, 2] == -1).all()
        assert np.isposinf(acc[6, 1]).all() and np.isneginf(acc[6, 2]).all() and not acc[6, 0].any()


def test_nan_and_infinite_voxels_and_a_volume_of_minus_zero():
    vol = _volume(np.float32).copy()
    g = np.random.default_rng(9)
    for bad in (np.nan, np.inf, -np.inf):
        vol[g.random(EDGE) < 0.02] = bad
    for order in (0, 1):
        acc, idx, info = _check(vol, [IDENT, OBLIQUE], (9, 11), 33, order, what=order)
        assert (info[:, 4] > 0).all() and (info[:, 0] == PR.NONFINITE).all() and np.isfinite(acc[:, 0]).all()
    mz = np.full((5, 6, 7), -0.0)
    for order in (0, 1, 3):
        src = mz                                                         # the coefficients of -0.0 are handed over as they are
        ref = PR.project_ref(mz, [IDENT], (5, 6), 7, order, coef=src)
        rc, acc, idx, info = _call(_dev(src), [IDENT], (5, 6), 7, order)
        assert rc == 0
        _same((acc, idx, info), ref, ('-0.0', order))
        assert not np.signbit(acc).any() and not acc.any() and (idx[0, 0] == 7).all()


@pytest.mark.parametrize('ldtype', LABEL_DTYPES, ids=lambda d: np.dtype(d).name)
def test_label_dtypes(ldtype):
    lab = (np.random.default_rng(2).integers(0, 3, EDGE) * 7).astype(ldtype)
    _check(_volume(np.int16), [IDENT, OBLIQUE], (9, 11), 33, 1, lab, 7, what=ldtype)
    if np.dtype(ldtype).kind == 'f':
        lab = lab.copy()
        lab[lab == 7] = 7.5
        lab[0, 0, :5] = np.nan                                           # a NaN label equals nothing
        _check(_volume(np.int16), [IDENT], (9, 11), 33, 0, lab, 7.5, what=(ldtype, 7.5))


def test_a_label_that_rejects_whole_rays_and_one_that_cuts_mid_chunk():
    vol = _volume(np.int16)
    lab = np.ones(EDGE, dtype=np.uint8)
    lab[:, 5:9, :] = 0                                                   # whole rays of the lateral view
    lab[3, :, 7:29] = 0                                                  # counted t = 0 .. 6 and 29 .. 32: chunk 1 empty, chunks 0 and 2 cut
    lab[4, 2, :] = 0
    lab[4, 2, 20] = 1                                                    # one sample
    for view in ('lateral', 'ap'):
        pose, det, T = _axis_pose(EDGE, view)
        acc, idx, info = _check(vol, [pose], det, T, 1, lab, 1, what=view)
        assert info[0, 3] == (lab == 0).sum() and info[0, 1] == (lab == 1).sum()
    pose, det, T = _axis_pose(EDGE, 'lateral')
    acc, idx, info = _check(vol, [pose], det, T, 0, lab, 1)
    assert idx[0, :, 3, 0].tolist() == [11, 0, 32] and idx[0, :, 0, 6].tolist() == [0, 33, -1] and idx[0, :, 4, 2].tolist() == [1, 20, 20]
    assert acc[0, :, 4, 2].tolist() == [vol[4, 2, 20]] * 3
    _check(vol, [pose], det, T, 1, lab, 9)                               # a value no voxel has: nothing counted


def _layouts(a):
    """The same logical array under several storages -> (name, device tensor) pairs."""
    big = torch.full(tuple(n + 5 for n in a.shape), 0, dtype=torch.from_numpy(np.zeros(1, a.dtype)).dtype, device='cuda')
    big.view(-1).view(torch.uint8).fill_(0x5A)
    sub = big[2:2 + a.shape[0], 3:3 + a.shape[1], 1:1 + a.shape[2]]
    sub.copy_(_dev(a))
    return [('C', _dev(a)), ('F', _dev(a.transpose(2, 1, 0)).permute(2, 1, 0)), ('permuted', _dev(a.transpose(1, 2, 0)).permute(2, 0, 1)), ('sub-box', sub)]


def test_layouts_of_volume_and_label_give_the_contiguous_bytes():
    vol = _volume(np.int16)
    lab = (np.random.default_rng(4).random(EDGE) < 0.8).astype(np.int32) * 3
    poses = [OBLIQUE, _axis_pose(EDGE, 'lateral')[0]]
    ref = PR.project_ref(vol, poses, (17, 18), 33, 1, lab, 3)
    for vn, dv in _layouts(vol):
        for ln, dl in _layouts(lab):
            assert tuple(dv.shape) == EDGE and tuple(dl.shape) == EDGE
            rc, acc, idx, info = _call(dv, poses, (17, 18), 33, 1, dl, 3.0)
            assert rc == 0
            _same((acc, idx, info), ref, (vn, ln))


def test_same_bytes_twice_and_on_poisoned_buffers():
    vol = _volume(np.float32)
    dv = _dev(vol)
    runs = [_call(dv, [IDENT, OBLIQUE], (9, 11), 33, 1, prefill=p) for p in (0xA5, 0xA5, 0x00, 0xFF)]
    ref = PR.project_ref(vol, [IDENT, OBLIQUE], (9, 11), 33, 1)
    for rc, acc, idx, info in runs:
        assert rc == 0
        _same((acc, idx, info), ref)


def test_refusals_write_nothing():
    lib, L = _lib()
    dv = _dev(_volume(np.float32))
    dl = _dev(np.ones(EDGE, dtype=np.int16))
    bad_pose = np.concatenate([np.eye(3).reshape(9), [0.0, np.nan, 0.0]])
    inf_pose = np.concatenate([np.full(9, np.inf), np.zeros(3)])
    cases = [
        (dict(vol_null=1), ERR_ARG), (dict(poses_null=1), ERR_ARG), (dict(acc_null=1), ERR_ARG), (dict(idx_null=1), ERR_ARG),
        (dict(info_null=1), ERR_ARG), (dict(A0=0), ERR_ARG), (dict(A1=-1), ERR_ARG), (dict(A2=0), ERR_ARG), (dict(P0=0), ERR_ARG),
        (dict(P1=-3), ERR_ARG), (dict(T=0), ERR_ARG), (dict(K=0), ERR_ARG), (dict(K=17), ERR_ARG), (dict(dtype=2), ERR_ARG), (dict(dtype=6), ERR_ARG),
        (dict(dtype=-1), ERR_ARG), (dict(order=2), ERR_ARG), (dict(order=-1), ERR_ARG), (dict(order=3), ERR_ARG),    # order 3 on float32
        (dict(poses_flat=bad_pose), ERR_ARG), (dict(poses_flat=inf_pose), ERR_ARG), (dict(label_value=float('nan')), ERR_ARG),
        (dict(label_value=float('inf'), with_label=1), ERR_ARG), (dict(label_dtype=6, with_label=1), ERR_ARG), (dict(label_dtype=-1, with_label=1), ERR_ARG),
        (dict(vol_off=2), ERR_ARG), (dict(acc_off=4), ERR_ARG), (dict(idx_off=2), ERR_ARG), (dict(info_off=4), ERR_ARG), (dict(ws_ptr=8), ERR_ARG),
        (dict(label_ptr=ctypes.c_void_p(dl.data_ptr() + 1), with_label=1), ERR_ARG),
        (dict(acc_ptr=ctypes.c_void_p(dv.data_ptr())), ERR_ARG),                                   # an output inside the volume
        (dict(A0=1 << 11, A1=1 << 10, A2=(1 << 9) + 1), ERR_UNSUPPORTED), (dict(P0=1 << 10, P1=1 << 10, T=1025), ERR_UNSUPPORTED),
        (dict(P0=1 << 16, P1=1 << 15, T=1), ERR_UNSUPPORTED),
    ]
    before = dv.clone()
    for over, code in cases:
        over = dict(over)
        label = dl if over.pop('with_label', 0) else None
        det = (over.get('P0', 2), over.get('P1', 3))
        args = (over.pop('T', 5), over.pop('order', 1), label, over.pop('label_value', 1.0))
        rc, acc, idx, info = _call(dv, [IDENT], (max(1, min(det[0], 4)), max(1, min(det[1], 4))), *args, **over)
        assert rc == code, (over, rc)
        for w in (acc, idx, info):
            assert (w.view(np.uint8) == 0xA5).all(), over
    assert torch.equal(before.view(torch.int32), dv.view(torch.int32))
    assert L.size('hv_project_workspace_bytes', 17, 18, 33, 1, 9, 11, 33) == 0


# ------------------------------------------------------------------------------------------------ the module
def _close(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert (np.isnan(a) == np.isnan(b)).all() and (np.isinf(a) == np.isinf(b)).all(), (what, a, b)
    ok = np.isfinite(a)
    assert (np.abs(a[ok] - b[ok]) <= 1e-12 * np.abs(b[ok])).all(), (what, a, b)


def _areal_ref(ct, lab, value, sp, view, order=1, **geometry):
    m, off, det, T, ds, st = PR.view_pose(ct.shape, sp, view, **geometry)
    acc, idx, info = PR.project_ref(ct, [(m, off)], det, T, order, lab, value)
    return PR.areal_density(acc[0], idx[0], ds, st), (acc, idx, info), (m, off, det, T, ds, st)


def _same_areal(got, want, what):
    assert got['pixels'] == want['pixels'] and got['samples'] == want['samples'], (what, got, want)
    for q in ('area', 'integral', 'areal_density', 'mean_path'):
        _close(got[q], want[q], (what, q))


def test_project_and_the_pictures_on_the_phantom():
    P = _P()
    ct, lab, ct_s, lab_s = PR.phantom()
    sp = (1.0, 0.8, 1.25)
    for view in ('lateral', 'ap', 'axial', (10.0, -20.0, 5.0)):
        vp = P.view_pose(ct.shape, sp, view)
        m, off, det, T, ds, st = PR.view_pose(ct.shape, sp, view)
        _close(vp.matrix, m, 'matrix')
        _close(vp.offset, off, 'offset')
        assert vp.det_shape == det and vp.steps == T and tuple(vp.det_spacing) == tuple(ds) and vp.step_mm == st
        res = P.project(_dev(ct), (vp.matrix, vp.offset), vp.det_shape, vp.steps, order=1, label=_dev(lab), label_value=21)
        assert res.acc.is_cuda and res.idx.dtype == torch.int32 and res.info.dtype == torch.int64
        ref = PR.project_ref(ct, [(vp.matrix, vp.offset)], det, T, 1, lab, 21)
        _same((res.acc.cpu().numpy(), res.idx.cpu().numpy(), res.info.cpu().numpy()), ref, view)
        host = P.project(ct, (vp.matrix, vp.offset), vp.det_shape, vp.steps, label=lab, label_value=21, readback=True)   # numpy in, numpy out
        _same(tuple(host), ref, view)
        full = PR.project_ref(ct, [(m, off)], det, T, 1)
        _close(P.radiograph(_dev(ct), sp, view), PR.radiograph(full[0][0], st), 'radiograph')
        mn, mx = P.mip(_dev(ct), sp, view)
        assert mn.tobytes() == full[0][0, 1].tobytes() and mx.tobytes() == full[0][0, 2].tobytes()
        thick = PR.project_ref(lab, [(m, off)], det, T, 0, lab, 22)
        _close(P.thickness_map(_dev(lab), 22, sp, view), PR.thickness_map(thick[1][0], st), 'thickness')
        _same_areal(P.areal_density(_dev(ct), _dev(lab), 21, sp, view), _areal_ref(ct, lab, 21, sp, view)[0], view)
    o3 = P.project(_dev(ct), IDENT, (24, 28), 20, order=3, readback=True)                  # the coefficients are made on the device
    want = PR.project_ref(ct, [IDENT], (24, 28), 20, 3)
    assert (o3.idx == want[1]).all() and (o3.info == want[2]).all()
    # the device's prefilter is within spline_ref.SPLINE_TOL = 1e-9 of the data's magnitude per coefficient, the weights of a sample are
    # non-negative at whole indices and sum to 1, and a ray adds 20 samples
    assert np.abs(o3.acc[0, 0] - want[0][0, 0]).max() <= 20 * 1e-9 * np.abs(ct).max()
    many = P.project(_dev(ct), [OBLIQUE] * 17 + [IDENT], (5, 4), 9, order=0, readback=True)  # more than 16 poses: two launches, one buffer
    _same(tuple(many), PR.project_ref(ct, [OBLIQUE] * 17 + [IDENT], (5, 4), 9, 0), 'many')


def test_projection_comparison_on_the_phantom(monkeypatch):
    P = _P()
    ct, lab, ct_s, lab_s = PR.phantom()
    sp = (1.0, 0.8, 1.25)
    geometry = dict(det_spacing=0.8, step_mm=0.5, det_shape=(41, 39), steps=80)
    calls = []
    real = P._launch
    monkeypatch.setattr(P, '_launch', lambda *a: (calls.append(len(a[3])), real(*a))[1])
    one = P.projection_comparison(_dev(ct), _dev(lab), _dev(ct_s), _dev(lab_s), 21, neighbours=(22,), spacing=sp, view='lateral', **geometry)
    both = P.projection_comparison(_dev(ct), _dev(lab), _dev(ct_s), _dev(lab_s), 21, neighbours=(22,), spacing=sp, view=['lateral', 'ap'], **geometry)
    monkeypatch.setattr(P, '_launch', real)
    assert calls == [1, 1, 1, 2, 2, 2]                                  # one launch per (volume, label value), the views as poses of it
    for k, view in enumerate(('lateral', 'ap')):
        want_o = _areal_ref(ct, lab, 21, sp, view, **geometry)[0]
        want_s = _areal_ref(ct_s, lab_s, 21, sp, view, **geometry)[0]
        want_n = _areal_ref(ct, lab, 22, sp, view, **geometry)[0]
        for res in ([one] if k == 0 else []) + [{key: both[key][k] for key in both}]:
            _same_areal(res['original'], want_o, 'original')
            _same_areal(res['synthesized'], want_s, 'synthesized')
            _same_areal(res['neighbours'][22], want_n, 'neighbour')
            for q in P.SCALARS:
                _close(res['original_ratio'][q], want_s[q] / want_o[q], q)
                _close(res['neighbour_ratio'][q], want_s[q] / want_n[q], q)
    assert one['synthesized']['integral'] > one['original']['integral'] and one['original_ratio']['integral'] > 1.0


def test_misuse_raises():
    P = _P()
    ct, lab, _, _ = PR.phantom()
    d = _dev(ct)
    with pytest.raises(ValueError):
        P.project(d, IDENT, (4, 4), 5, order=2)
    with pytest.raises(ValueError):
        P.project(d, IDENT, (4, 4), 0)
    with pytest.raises(ValueError):
        P.project(d, IDENT, (4, 4), 5, label=_dev(lab))                 # a label without its value
    with pytest.raises(ValueError):
        P.project(d, IDENT, (4, 4), 5, label=_dev(lab)[1:], label_value=21)
    with pytest.raises(TypeError):
        P.project(d.to(torch.int32), IDENT, (4, 4), 5)
    with pytest.raises(ValueError):
        P.project(d, (np.eye(3) * np.nan, np.zeros(3)), (4, 4), 5)
    with pytest.raises(ValueError):
        P.view_pose(ct.shape, (1, 1, 1), 'oblique')
    with pytest.raises(ValueError):
        P.view_pose(ct.shape, (1, 1, 0), 'lateral')
    with pytest.raises(ValueError):
        P.projection_comparison(d, _dev(lab), d, _dev(lab), 21, neighbours=(21,))         # the vertebra as its own neighbour
    with pytest.raises(ValueError):
        P.projection_comparison(d, _dev(lab), d[1:], _dev(lab)[1:], 21)
