"""hv_resample (csrc/resample.hip) and healthivert-gan_amd/resample.py against tests/resample_ref.py (pinned against scipy by
tests/test_resample_ref_cpu.py): by dtype, shape and bytes.  Order 3 is compared on the DEVICE's coefficients: the test reads spline_filter()'s
volume back and has the restatement sample it (coef=), so hv_resample is pinned byte for byte while the prefilter keeps the tolerance of
tests/test_spline_gpu.py.  Extents are built from the tile the library reports (hv_resample_tile) and stay within a few tiles."""
import ctypes

import numpy as np
import pytest
import torch

import resample_ref as R

pytestmark = pytest.mark.gpu

_DT = {torch.uint8: 0, torch.int16: 1, torch.float32: 4, torch.float64: 5}
ERR_ARG, ERR_UNSUPPORTED = -1, -2
CONSTANT, NEAREST = 1, 2
CVAL = 3.0
DT = pytest.mark.parametrize('dtype', R.DTYPES, ids=lambda d: np.dtype(d).name)
ORD = pytest.mark.parametrize('order', (0, 1, 3))


def _lib():
    import hvgan  # noqa: F401
    from hvgan import lib
    return lib, lib.get()


def _RS():
    import hvgan  # noqa: F401
    from hvgan import resample
    return resample


def _tile():
    _, L = _lib()
    dims = (ctypes.c_int * 3)()
    assert L.cdll.hv_resample_tile(dims) == 0
    assert tuple(dims) == (R.TILE,) * 3
    return dims[0]


def _same(got, want, what=None):
    """Device tensor against the restatement's array: dtype, shape and bytes."""
    g = got.cpu().numpy()
    assert g.dtype == want.dtype and g.shape == want.shape, (what, g.dtype, want.dtype, g.shape, want.shape)
    assert np.ascontiguousarray(g).tobytes() == np.ascontiguousarray(want).tobytes(), (what, int((g != want).sum()))


def _coef(t, order):
    """The device's own order-3 coefficients of the device tensor t as a numpy array (None below order 3)."""
    return _RS().spline_filter(t).cpu().numpy() if order == 3 else None


def _layout(a, how):
    """The numpy array on the device with the same logical content: C order, Fortran order, stored as [A1][A2][A0], or a sub-box of a parent
    filled with NaN (integers: a sentinel)."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if how == 'c':
        return t.cuda()
    if how == 'f':
        return t.permute(2, 1, 0).contiguous().cuda().permute(2, 1, 0)
    if how == 'perm':
        return t.permute(1, 2, 0).contiguous().cuda().permute(2, 0, 1)
    pad = (2, 3, 1)
    shape = tuple(n + 2 * p for n, p in zip(t.shape, pad))
    big = torch.full(shape, float('nan') if t.dtype.is_floating_point else (0xA5 if t.dtype == torch.uint8 else -23131), dtype=t.dtype)
    big[pad[0]:pad[0] + t.shape[0], pad[1]:pad[1] + t.shape[1], pad[2]:pad[2] + t.shape[2]] = t
    return big.cuda()[pad[0]:pad[0] + t.shape[0], pad[1]:pad[1] + t.shape[1], pad[2]:pad[2] + t.shape[2]]


# ------------------------------------------------------------------------------------------------ the host cases on the device
@DT
@ORD
def test_affine_zoom_shift_equal_the_restatement(order, dtype):
    RS = _RS()
    v = R.case_volume(dtype)
    t = torch.from_numpy(v).cuda()
    c = _coef(t, order)
    _same(RS.affine_transform(t, R.MATRIX, R.OFFSET, R.OUT_SHAPE, order=order, cval=CVAL),
          R.affine_transform(v, R.MATRIX, R.OFFSET, R.OUT_SHAPE, order=order, cval=CVAL, coef=c), 'matrix')
    h = np.eye(4)
    h[:3, :3], h[:3, 3] = R.MATRIX, R.OFFSET
    _same(RS.affine_transform(t, h, 99.0, R.OUT_SHAPE, order=order, cval=CVAL),
          R.affine_transform(v, h, 99.0, R.OUT_SHAPE, order=order, cval=CVAL, coef=c), 'homogeneous')
    _same(RS.affine_transform(t, R.DIAGONAL, R.DIAG_OFFSET, R.OUT_SHAPE, order=order, cval=CVAL),
          R.affine_transform(v, R.DIAGONAL, R.DIAG_OFFSET, R.OUT_SHAPE, order=order, cval=CVAL, coef=c), 'diagonal')
    _same(RS.affine_transform(t, R.MATRIX, R.OFFSET, R.OUT_SHAPE, output=torch.float64, order=order, cval=CVAL),
          R.affine_transform(v, R.MATRIX, R.OFFSET, R.OUT_SHAPE, order=order, cval=CVAL, output=np.float64, coef=c), 'float64 output')
    for z in R.ZOOMS:
        _same(RS.zoom(t, z, order=order, cval=CVAL), R.zoom(v, z, order=order, cval=CVAL, coef=c), ('zoom', z))
    for s in R.SHIFTS:
        _same(RS.shift(t, s, order=order, cval=CVAL), R.shift(v, s, order=order, cval=CVAL, coef=c), ('shift', s))
    if order == 3 and np.dtype(dtype) == np.float64:
        _same(RS.affine_transform(torch.from_numpy(c).cuda(), R.MATRIX, R.OFFSET, R.OUT_SHAPE, order=3, cval=CVAL, prefilter=False),
              R.affine_transform(v, R.MATRIX, R.OFFSET, R.OUT_SHAPE, order=3, cval=CVAL, coef=c), 'prefilter=False')


@DT
def test_nearest_at_order_0(dtype):
    RS = _RS()
    v = R.case_volume(dtype)
    t = torch.from_numpy(v).cuda()
    _same(RS.affine_transform(t, R.MATRIX, R.OFFSET, R.OUT_SHAPE, order=0, mode='nearest'),
          R.affine_transform(v, R.MATRIX, R.OFFSET, R.OUT_SHAPE, order=0, mode='nearest'))
    for z in R.ZOOMS:
        _same(RS.zoom(t, z, order=0, mode='nearest'), R.zoom(v, z, order=0, mode='nearest'), z)
    for s in R.SHIFTS:
        _same(RS.shift(t, s, order=0, mode='nearest'), R.shift(v, s, order=0, mode='nearest'), s)
    for order in (1, 3):
        with pytest.raises(ValueError, match='nearest'):
            RS.shift(t, 0.5, order=order, mode='nearest')


# ------------------------------------------------------------------------------------------------ tiles and layouts
@pytest.mark.parametrize('axis', (0, 1, 2))
def test_output_extents_around_the_tile(axis):
    """1, tile - 1, tile, tile + 1 outputs along each axis beside extents that are multiples of no tile, in both forms at order 1."""
    RS = _RS()
    T = _tile()
    v = R.case_volume(np.float32, (5, 6, 7), seed=2)
    t = torch.from_numpy(v).cuda()
    for n in (1, T - 1, T, T + 1):
        shape = [3, 11]
        shape.insert(axis, n)
        shape = tuple(shape)
        m = R.MATRIX * 0.6
        _same(RS.affine_transform(t, m, R.OFFSET, shape, order=1, cval=CVAL), R.affine_transform(v, m, R.OFFSET, shape, order=1, cval=CVAL),
              ('matrix', shape))
        d = np.array([0.45, 0.5, 0.55])
        _same(RS.affine_transform(t, d, 0.1, shape, order=1, cval=CVAL), R.affine_transform(v, d, 0.1, shape, order=1, cval=CVAL),
              ('diagonal', shape))


@ORD
def test_awkward_shape_over_several_tiles(order):
    RS = _RS()
    v = R.case_volume(np.int16, (33, 17, 65), seed=4)
    t = torch.from_numpy(v).cuda()
    c = _coef(t, order)
    out_shape = (17, 40, 31)
    zoomv = tuple(o / a for o, a in zip(out_shape, v.shape))
    assert R.zoom_arguments(v.shape, zoomv)[0] == out_shape
    _same(RS.zoom(t, zoomv, order=order, cval=-1000), R.zoom(v, zoomv, order=order, cval=-1000, coef=c), 'zoom')
    m = np.array([[1.9, 0.1, -0.05], [-0.1, 0.4, 0.02], [0.3, -0.2, 2.0]])
    _same(RS.affine_transform(t, m, (1.0, 2.0, 3.5), out_shape, order=order, cval=-1000),
          R.affine_transform(v, m, (1.0, 2.0, 3.5), out_shape, order=order, cval=-1000, coef=c), 'matrix')


@pytest.mark.parametrize('how', ('f', 'perm', 'box'))
@ORD
def test_source_views_and_a_strided_destination(order, how):
    """Permuted and sliced sources pass as they lie; the destination is a sub-box with a step of a sentinel-filled parent whose other
    elements must keep their bytes."""
    RS = _RS()
    for dtype in (np.float32, np.int16):
        v = R.case_volume(dtype, (9, 7, 10), seed=5)
        t = _layout(v, how)
        assert not t.is_contiguous() and t.shape == v.shape
        c = _coef(t, order)
        want = R.affine_transform(v, R.MATRIX, R.OFFSET, R.OUT_SHAPE, order=order, cval=CVAL, coef=c)
        tt = torch.from_numpy(want).dtype
        sentinel = float('nan') if tt.is_floating_point else -23131
        big = torch.full((12, 2 * 7 + 3, 9 + 4), sentinel, dtype=tt, device='cuda')
        before = big.clone()
        out = big[2:10, 1:15:2, 3:12].permute(0, 1, 2)
        assert tuple(out.shape) == R.OUT_SHAPE
        got = RS.affine_transform(t, R.MATRIX, R.OFFSET, R.OUT_SHAPE, output=out, order=order, cval=CVAL)
        assert got.data_ptr() == out.data_ptr()
        _same(out, want, (how, dtype))
        mask = torch.ones_like(big, dtype=torch.bool)
        mask[2:10, 1:15:2, 3:12] = False
        assert torch.equal(big.view(torch.int32 if tt == torch.float32 else tt)[mask], before.view(torch.int32 if tt == torch.float32 else tt)[mask])
        out_t = torch.empty(R.OUT_SHAPE[::-1], dtype=tt, device='cuda').permute(2, 1, 0)              # a transposed destination
        _same(RS.affine_transform(t, R.MATRIX, R.OFFSET, R.OUT_SHAPE, output=out_t, order=order, cval=CVAL), want, (how, dtype, 'transposed out'))


# ------------------------------------------------------------------------------------------------ properties
@DT
@ORD
def test_identity_returns_the_input(order, dtype):
    """Every form of the identity returns the input's bytes; a float64 order-3 sample at a lattice point is (c[-1] + 4 c[0] + c[1]) / 6 of
    the coefficients, the voxel only to rounding (as in scipy), so that one is compared with the restatement."""
    RS = _RS()
    v = R.case_volume(dtype)
    t = torch.from_numpy(v).cuda()
    c = _coef(t, order)
    exact = not (order == 3 and np.dtype(dtype) == np.float64)
    for got, want in ((RS.affine_transform(t, np.eye(3), order=order), R.affine_transform(v, np.eye(3), order=order, coef=c)),
                      (RS.affine_transform(t, np.ones(3), order=order), R.affine_transform(v, np.ones(3), order=order, coef=c)),
                      (RS.zoom(t, 1.0, order=order), R.zoom(v, 1.0, order=order, coef=c)),
                      (RS.shift(t, 0.0, order=order), R.shift(v, 0.0, order=order, coef=c))):
        _same(got, want)
        if exact:
            _same(got, v)
        else:
            assert np.allclose(got.cpu().numpy(), v, rtol=0, atol=1e-9)


@DT
def test_everything_outside_gives_cval(dtype):
    RS = _RS()
    v = R.case_volume(dtype)
    t = torch.from_numpy(v).cuda()
    for order in (0, 1, 3):
        for got in (RS.shift(t, (20.0, 0.0, 0.0), order=order, cval=7), RS.affine_transform(t, np.eye(3), (0.0, -0.001 - 8, 0.0), order=order, cval=7),
                    RS.affine_transform(t, np.eye(3) * 1e300, 1e300, order=order, cval=7)[1:]):
            assert got.dtype == t.dtype and bool((got == 7).all())


@DT
def test_coordinates_exactly_on_the_last_voxel(dtype):
    """u = o / 2 ends exactly on A - 1: the last output voxel is the last input voxel, not cval; one step further is cval."""
    RS = _RS()
    v = R.case_volume(dtype)
    t = torch.from_numpy(v).cuda()
    shape = tuple(2 * n for n in v.shape)                         # 2 A - 1 lattice points inside, one beyond
    for order in (0, 1):
        got = RS.affine_transform(t, np.full(3, 0.5), 0.0, shape, order=order, cval=7)
        _same(got, R.affine_transform(v, np.full(3, 0.5), 0.0, shape, order=order, cval=7))
        g = got.cpu().numpy()
        assert g[-2, -2, -2] == v[-1, -1, -1] and g[-1, -2, -2] == 7 and np.array_equal(g[:-1:2, :-1:2, :-1:2], v)
    c = _coef(t, 3)
    _same(RS.affine_transform(t, np.full(3, 0.5), 0.0, shape, order=3, cval=7), R.affine_transform(v, np.full(3, 0.5), 0.0, shape, order=3, cval=7, coef=c))


def test_spacing_round_trip_of_a_label_is_exact():
    RS = _RS()
    lab = (np.random.RandomState(8).random_sample((9, 7, 5)) * 4).astype(np.uint8)
    t = torch.from_numpy(lab).cuda()
    up, plan = RS.resample_label_to_spacing(t, (2.0, 3.0, 1.0), (1.0, 1.0, 1.0))
    assert plan['new_shape'] == (18, 21, 5) and tuple(up.shape) == plan['new_shape'] and up.dtype == torch.uint8
    _same(up, R.resample(lab, plan['new_shape'], 0, 'zoomshift', plan['forward']['zoom'], plan['forward']['shift']))
    back = RS.resample_back(up, plan, order=0)
    _same(back, lab)
    ct = R.case_volume(np.int16, (9, 7, 5), seed=9)
    vol, plan2 = RS.resample_to_spacing(torch.from_numpy(ct).cuda(), (2.0, 3.0, 1.0), (1.0, 1.0, 1.0), order=1, cval=-1024)
    _same(vol, R.resample(ct, plan2['new_shape'], 1, 'zoomshift', plan2['forward']['zoom'], plan2['forward']['shift'], cval=-1024))


def test_host_array_and_resident_tensor_agree():
    RS = _RS()
    v = R.case_volume(np.int16)
    for order in (0, 1, 3):
        a = RS.zoom(v, (1.5, 0.7, 2.0), order=order)
        b = RS.zoom(torch.from_numpy(v).cuda(), (1.5, 0.7, 2.0), order=order)
        assert a.is_cuda and a.dtype == torch.int16 and torch.equal(a, b)
    m = (np.random.RandomState(1).random_sample((4, 5, 6)) < 0.5)
    got = RS.shift(m, (1, 0, 0), order=0)
    assert got.dtype == torch.uint8
    _same(got, R.shift(m.astype(np.uint8), (1, 0, 0), order=0))
    rot = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    sq = R.case_volume(np.float32, (5, 5, 3), seed=6)
    _same(RS.rigid_transform(sq, rot, order=1), np.ascontiguousarray(np.rot90(sq, 1, axes=(0, 1))))       # a quarter turn about the middle
    with pytest.raises(TypeError):
        RS.zoom(v.astype(np.int32), 1.0)


# ------------------------------------------------------------------------------------------------ refusals through the C ABI
def _desc(L, form=0, order=1, mode=CONSTANT, cval=0.0, matrix=None, offset=(0, 0, 0), zoom=(1, 1, 1), shift=(0, 0, 0)):
    d = L.hv_resample_desc()
    d.form, d.order, d.mode, d.cval = form, order, mode, cval
    for i, x in enumerate(np.eye(3).reshape(9) if matrix is None else matrix):
        d.matrix[i] = float(x)
    for i in range(3):
        d.offset[i], d.zoom[i], d.shift[i] = float(offset[i]), float(zoom[i]), float(shift[i])
    return d


def _call(L, src, out, d, A=None, O=None, dtype=None, out_dtype=None, sptr='t', optr='t', dptr=True):
    ll = lambda st: [ctypes.c_longlong(s) for s in st]
    return L.cdll.hv_resample(ctypes.c_void_p(src.data_ptr()) if sptr == 't' else sptr, _DT[src.dtype] if dtype is None else dtype, *ll(src.stride()),
                              *(tuple(src.shape) if A is None else A), ctypes.c_void_p(out.data_ptr()) if optr == 't' else optr,
                              _DT[out.dtype] if out_dtype is None else out_dtype, *ll(out.stride()), *(tuple(out.shape) if O is None else O),
                              ctypes.byref(d) if dptr else None, None)


def test_every_refusal_leaves_out_unchanged():
    _, L = _lib()
    src = torch.from_numpy(R.case_volume(np.float64)).cuda()
    src16 = torch.from_numpy(R.case_volume(np.int16)).cuda()
    nan, inf = float('nan'), float('inf')
    for odt in (torch.float64, torch.int16, torch.uint8):
        out = torch.full(R.OUT_SHAPE, 0x5A if odt != torch.float64 else -1.25, dtype=odt, device='cuda')
        before = out.clone()
        ok = _desc(L)
        cases = [
            (ERR_ARG, dict(sptr=None)), (ERR_ARG, dict(optr=None)), (ERR_ARG, dict(dptr=False)),
            (ERR_ARG, dict(A=(0, 9, 6))), (ERR_ARG, dict(A=(7, -1, 6))), (ERR_ARG, dict(O=(8, 7, 0))), (ERR_ARG, dict(O=(-8, 7, 9))),
            (ERR_ARG, dict(dtype=2)), (ERR_ARG, dict(dtype=7)), (ERR_ARG, dict(out_dtype=3)), (ERR_ARG, dict(out_dtype=-1)),
            (ERR_UNSUPPORTED, dict(A=(1 << 11, 1 << 10, (1 << 9) + 1))), (ERR_UNSUPPORTED, dict(O=((1 << 10) + 1, 1 << 10, 1 << 10))),
        ]
        for rc, kw in cases:
            assert _call(L, src, out, ok, **kw) == rc, kw
        descs = [
            (ERR_ARG, dict(form=2)), (ERR_ARG, dict(form=-1)), (ERR_ARG, dict(order=2)), (ERR_ARG, dict(order=4)), (ERR_ARG, dict(order=5)),
            (ERR_ARG, dict(order=-1)), (ERR_ARG, dict(mode=5)), (ERR_ARG, dict(mode=-1)),
            (ERR_UNSUPPORTED, dict(mode=0)), (ERR_UNSUPPORTED, dict(mode=3)), (ERR_UNSUPPORTED, dict(mode=4)),
            (ERR_UNSUPPORTED, dict(mode=NEAREST, order=1)), (ERR_UNSUPPORTED, dict(mode=NEAREST, order=3)),
            (ERR_ARG, dict(cval=nan)), (ERR_ARG, dict(cval=inf)), (ERR_ARG, dict(matrix=[1, 0, 0, 0, nan, 0, 0, 0, 1])),
            (ERR_ARG, dict(offset=(0, inf, 0))), (ERR_ARG, dict(form=1, zoom=(1, 1, nan))), (ERR_ARG, dict(form=1, shift=(-inf, 0, 0))),
            (ERR_ARG, dict(form=0, zoom=(1, nan, 1))),                                    # every field is checked, whatever the form
        ]
        if odt != torch.float64:
            descs += [(ERR_ARG, dict(cval=0.5)), (ERR_ARG, dict(cval=-1.0 if odt == torch.uint8 else -32769.0)),
                      (ERR_ARG, dict(cval=256.0 if odt == torch.uint8 else 32768.0))]
        for rc, kw in descs:
            assert _call(L, src, out, _desc(L, **kw)) == rc, kw
        assert _call(L, src16, out, _desc(L, order=3)) == ERR_ARG                         # order 3 samples float64 coefficients only
        torch.cuda.synchronize()
        assert torch.equal(out, before)
    # out inside the bytes the source spans: refused, the source (= out's memory) unchanged
    big = torch.from_numpy(R.case_volume(np.float64, (8, 7, 18), seed=3)).cuda()
    before = big.clone()
    a, b = big[:, :, :9], big[:, :, 9:]
    assert _call(L, a, b, _desc(L)) == ERR_ARG and _call(L, big, big, _desc(L)) == ERR_ARG
    torch.cuda.synchronize()
    assert torch.equal(big, before)
    RS = _RS()
    with pytest.raises(ValueError, match='output'):
        RS.shift(a, 1.0, output=b, order=1)
    with pytest.raises(ValueError, match='output'):
        RS.shift(src, 1.0, output=torch.empty((2, 2, 2), dtype=torch.float64, device='cuda'), order=1)
    with pytest.raises(TypeError):
        RS.affine_transform(src16, np.eye(3), order=3, prefilter=False)
    # the accepted call writes, so the refusals above were refusals
    out = torch.full(R.OUT_SHAPE, -1.25, dtype=torch.float64, device='cuda')
    assert _call(L, src, out, _desc(L, matrix=R.MATRIX.reshape(9), offset=R.OFFSET, cval=CVAL)) == 0
    _same(out, R.affine_transform(src.cpu().numpy(), R.MATRIX, R.OFFSET, R.OUT_SHAPE, order=1, cval=CVAL))
