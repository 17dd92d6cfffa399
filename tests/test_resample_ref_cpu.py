"""tests/resample_ref.py -- the numpy restatement the device resampling is compared with -- and the host functions of resample.py against
scipy.ndimage: np.array_equal and equal dtype on a 7 x 9 x 6 random volume.  No GPU.

Order 3: the sampler is pinned bit for bit on scipy's own coefficients (coef=), for every dtype.  The whole path -- the restatement's own
prefilter, which is within rounding of scipy's but not bit for bit -- is pinned on the uint8 / int16 / float32 outputs, whose rounding absorbs
the prefilter's last bits on these volumes, and bounded for float64 by spline_ref.SPLINE_TOL scaled to the data."""
import warnings

import numpy as np
import pytest
from scipy import ndimage

import resample_ref as R
import spline_ref

CVAL = 3.0
ORDERS = (0, 1, 3)
DT = pytest.mark.parametrize('dtype', R.DTYPES, ids=lambda d: np.dtype(d).name)
ORD = pytest.mark.parametrize('order', ORDERS)


def _RS():
    import hvgan  # noqa: F401
    from hvgan import resample
    return resample


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), what


def _coef(v):
    return ndimage.spline_filter(v, 3, output=np.float64, mode='mirror')


@DT
@ORD
def test_affine_full_matrix_equals_scipy(order, dtype):
    v = R.case_volume(dtype)
    want = ndimage.affine_transform(v, R.MATRIX, R.OFFSET, R.OUT_SHAPE, order=order, mode='constant', cval=CVAL)
    _same(R.affine_transform(v, R.MATRIX, R.OFFSET, R.OUT_SHAPE, order=order, cval=CVAL, coef=_coef(v)), want, (order, dtype))
    if np.dtype(dtype) != np.float64:
        _same(R.affine_transform(v, R.MATRIX, R.OFFSET, R.OUT_SHAPE, order=order, cval=CVAL), want, (order, dtype, 'own prefilter'))
    h = np.eye(4)
    h[:3, :3], h[:3, 3] = R.MATRIX, R.OFFSET
    for m in (h, h[:3]):
        _same(R.affine_transform(v, m, 99.0, R.OUT_SHAPE, order=order, cval=CVAL, coef=_coef(v)),
              ndimage.affine_transform(v, m, 99.0, R.OUT_SHAPE, order=order, mode='constant', cval=CVAL), (order, dtype, m.shape))


def test_order3_clamps_and_rounding_branches_are_hit():
    """int16 scaled to the ends of the type: the cubic overshoots both clamps and negative values take the t - 0.5 branch; uint8 overshoots
    below 0 and above 255.  float64 output of the same volumes shows the overshoot the integer outputs clamp."""
    for dtype, lo, hi in ((np.int16, -32768, 32767), (np.uint8, 0, 255)):
        v = R.case_volume(dtype)
        t = R.affine_transform(v, R.MATRIX, R.OFFSET, R.OUT_SHAPE, order=3, cval=CVAL, output=np.float64)
        assert t.min() < lo - 1 and t.max() > hi + 1, (dtype, t.min(), t.max())
        got = R.affine_transform(v, R.MATRIX, R.OFFSET, R.OUT_SHAPE, order=3, cval=CVAL)
        assert got.min() == lo and got.max() == hi
        _same(got, ndimage.affine_transform(v, R.MATRIX, R.OFFSET, R.OUT_SHAPE, order=3, mode='constant', cval=CVAL), dtype)
    v = R.case_volume(np.int16)
    t = R.zoom(v, 1.7, order=1, output=np.float64)
    assert ((t < 0) & (t != np.trunc(t))).any()                    # negative non-integers: the t - 0.5 branch decides


@DT
@ORD
def test_output_float64_equals_scipy(order, dtype):
    v = R.case_volume(dtype)
    want = ndimage.affine_transform(v, R.MATRIX, R.OFFSET, R.OUT_SHAPE, output=np.float64, order=order, mode='constant', cval=CVAL)
    _same(R.affine_transform(v, R.MATRIX, R.OFFSET, R.OUT_SHAPE, order=order, cval=CVAL, output=np.float64, coef=_coef(v)), want, (order, dtype))


@DT
@ORD
def test_affine_diagonal_equals_scipy(order, dtype):
    v = R.case_volume(dtype)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        want = ndimage.affine_transform(v, R.DIAGONAL, R.DIAG_OFFSET, R.OUT_SHAPE, order=order, mode='constant', cval=CVAL)
    _same(R.affine_transform(v, R.DIAGONAL, R.DIAG_OFFSET, R.OUT_SHAPE, order=order, cval=CVAL, coef=_coef(v)), want, (order, dtype))


@DT
@ORD
def test_zoom_equals_scipy(order, dtype):
    v = R.case_volume(dtype)
    shapes = []
    for z in R.ZOOMS:
        want = ndimage.zoom(v, z, order=order, mode='constant', cval=CVAL)
        shapes.append(want.shape)
        _same(R.zoom(v, z, order=order, cval=CVAL, coef=_coef(v)), want, (order, dtype, z))
        if np.dtype(dtype) != np.float64:
            _same(R.zoom(v, z, order=order, cval=CVAL), want, (order, dtype, z, 'own prefilter'))
    assert shapes == [(14, 14, 10), (4, 6, 4), (7, 9, 6), (1, 12, 1)]         # larger, smaller, equal, extents of 1


@DT
@ORD
def test_shift_equals_scipy(order, dtype):
    v = R.case_volume(dtype)
    for s in R.SHIFTS:
        want = ndimage.shift(v, s, order=order, mode='constant', cval=CVAL)
        _same(R.shift(v, s, order=order, cval=CVAL, coef=_coef(v)), want, (order, dtype, s))


@DT
def test_nearest_order0_equals_scipy(dtype):
    v = R.case_volume(dtype)
    _same(R.affine_transform(v, R.MATRIX, R.OFFSET, R.OUT_SHAPE, order=0, mode='nearest'),
          ndimage.affine_transform(v, R.MATRIX, R.OFFSET, R.OUT_SHAPE, order=0, mode='nearest'), dtype)
    for z in R.ZOOMS:
        _same(R.zoom(v, z, order=0, mode='nearest'), ndimage.zoom(v, z, order=0, mode='nearest'), (dtype, z))
    for s in R.SHIFTS:
        _same(R.shift(v, s, order=0, mode='nearest'), ndimage.shift(v, s, order=0, mode='nearest'), (dtype, s))


def test_nearest_order1_is_not_a_clamp_and_is_refused():
    """What was found: clamping the coordinate to [0, A - 1] differs from scipy's order-1 'nearest' in the last bit of float64 edge voxels,
    so neither the restatement nor resample.py offers the pair."""
    v = R.case_volume(np.float64)
    want = ndimage.shift(v, R.SHIFTS[1], order=1, mode='nearest')
    u = R.coords_zoomshift(v.shape, (1.0, 1.0, 1.0), tuple(-x for x in R.SHIFTS[1]))
    for h in range(3):
        u[h] = np.clip(u[h], 0.0, v.shape[h] - 1)
    clamp = R.sample(v, u, 1).reshape(v.shape)
    assert np.allclose(clamp, want, rtol=1e-13, atol=0) and not np.array_equal(clamp, want)
    with pytest.raises(ValueError):
        R.shift(v, R.SHIFTS[1], order=1, mode='nearest')
    RS = _RS()
    for order in (1, 3):
        with pytest.raises(ValueError, match='nearest'):
            RS._check_order_mode(order, 'nearest')
    assert RS._check_order_mode(0, 'nearest') == (0, 2)


def test_own_prefilter_is_within_the_spline_tolerance_of_scipys():
    v = R.case_volume(np.float64)
    d = np.abs(R.spline_filter_scipy(v) - _coef(v)).max()
    assert d <= spline_ref.SPLINE_TOL * spline_ref.scale_of(v), d
    got = R.affine_transform(v, R.MATRIX, R.OFFSET, R.OUT_SHAPE, order=3, cval=CVAL)
    want = ndimage.affine_transform(v, R.MATRIX, R.OFFSET, R.OUT_SHAPE, order=3, mode='constant', cval=CVAL)
    assert np.abs(got - want).max() <= spline_ref.SPLINE_TOL * spline_ref.scale_of(v)


# ------------------------------------------------------------------------------------------------ the host rules of resample.py
def test_front_end_arguments_are_the_restatements():
    RS = _RS()
    form, a, b = RS.affine_arguments(R.DIAGONAL, R.DIAG_OFFSET)
    assert form == RS.ZOOMSHIFT and np.array_equal(a, R.DIAGONAL) and np.array_equal(b, R.DIAG_OFFSET / R.DIAGONAL)
    h = np.eye(4)
    h[:3, :3], h[:3, 3] = R.MATRIX, R.OFFSET
    for m in (h, h[:3]):
        form, a, b = RS.affine_arguments(m, 99.0)
        assert form == RS.MATRIX and np.array_equal(a, R.MATRIX) and np.array_equal(b, R.OFFSET)
    form, a, b = RS.affine_arguments(R.MATRIX, 0.25)
    assert form == RS.MATRIX and np.array_equal(b, (0.25, 0.25, 0.25))
    for z in R.ZOOMS + (1.3,):
        shape, step = RS.zoom_arguments((7, 9, 6), z)
        rshape, rstep = R.zoom_arguments((7, 9, 6), z)
        assert shape == rshape and np.array_equal(step, rstep)
        assert shape == ndimage.zoom(np.zeros((7, 9, 6), np.uint8), z, order=0).shape


def test_rigid_matrix_against_a_hand_composed_matrix():
    RS = _RS()
    a, b = 0.3, -0.2
    rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    rot = rz @ rx
    ci, co = np.array([3.0, 4.0, 2.5]), np.array([3.5, 3.0, 4.0])

    def hom(r=np.eye(3), t=np.zeros(3)):
        m = np.eye(4)
        m[:3, :3], m[:3, 3] = r, t
        return m
    want = hom(t=ci) @ hom(r=rot.T) @ hom(t=-co)                     # output index -> input index: back to the centre, turn back, out again
    m, off = RS.rigid_matrix(rot, ci, co)
    assert np.allclose(m, want[:3, :3], rtol=0, atol=1e-15) and np.allclose(off, want[:3, 3], rtol=0, atol=1e-14)
    assert np.allclose(m @ co + off, ci, rtol=0, atol=1e-14)         # the centre goes to the centre
    p = np.array([1.0, 2.0, 3.0])
    assert np.allclose(m @ (rot @ (p - ci) + co) + off, p, rtol=0, atol=1e-13)
    with pytest.raises(ValueError):
        RS.rigid_matrix(rot * 1.01, ci, co)
    with pytest.raises(ValueError):
        RS.rigid_matrix(np.eye(2), ci, co)


def test_spacing_plan_and_point_round_trips():
    RS = _RS()
    plan = RS.spacing_plan((256, 256, 64), (0.7, 0.7, 1.5), (1.0, 1.0, 1.0))
    assert plan['shape'] == (256, 256, 64) and plan['new_shape'] == (179, 179, 96)
    assert plan['spacing'] == (0.7, 0.7, 1.5) and plan['new_spacing'] == (1.0, 1.0, 1.0)
    assert np.array_equal(plan['forward']['zoom'], [255 / 178, 255 / 178, 63 / 95])
    assert np.array_equal(plan['backward']['zoom'], [178 / 255, 178 / 255, 95 / 63])
    pts = np.random.RandomState(3).random_sample((20, 3)) * [255, 255, 63]
    there = RS.points_to_resampled(pts, plan)
    assert np.allclose(RS.points_from_resampled(there, plan), pts, rtol=1e-14, atol=1e-12)
    ends = RS.points_to_resampled([[0, 0, 0], [255, 255, 63]], plan)
    assert np.allclose(ends, [[0, 0, 0], [178, 178, 95]], rtol=0, atol=1e-12)      # the end voxels lie on the end voxels
    one = RS.spacing_plan((5, 1, 4), (1, 1, 1), (5, 1, 1))
    assert one['new_shape'] == (1, 1, 4) and np.array_equal(one['forward']['zoom'], [1.0, 1.0, 1.0])
    with pytest.raises(ValueError):
        RS.spacing_plan((5, 5, 5), (1, 1, 0), (1, 1, 1))


def test_python_refusals():
    RS = _RS()
    for order in (2, 4, 5, -1, 1.0, True):
        with pytest.raises(ValueError, match='order'):
            RS._check_order_mode(order, 'constant')
    for mode in ('reflect', 'mirror', 'wrap', 'grid-constant', 'grid-wrap', 'bogus'):
        with pytest.raises(ValueError, match='mode'):
            RS._check_order_mode(1, mode)
    import torch
    for cval, dt in ((float('nan'), torch.float64), (float('inf'), torch.float32), (0.5, torch.int16), (256, torch.uint8), (-1, torch.uint8),
                     (40000, torch.int16), ('0', torch.float64)):
        with pytest.raises(ValueError, match='cval'):
            RS._check_cval(cval, dt)
    assert RS._check_cval(-1024, torch.int16) == -1024.0 and RS._check_cval(0.5, torch.float32) == 0.5
    for bad in (np.eye(2), np.ones((3, 5)), [1.0, 0.0, 2.0], [[np.nan] * 3] * 3, np.ones(4)):
        with pytest.raises(ValueError, match='matrix'):
            RS.affine_arguments(bad)
    h = np.eye(4)
    h[3, 0] = 1.0
    with pytest.raises(ValueError, match='matrix'):
        RS.affine_arguments(h)
    with pytest.raises(ValueError, match='offset'):
        RS.affine_arguments(np.eye(3), [1.0, 2.0])
    with pytest.raises(ValueError, match='zoom'):
        RS.zoom_arguments((7, 9, 6), (0.01, 1, 1))
    with pytest.raises(ValueError):
        RS.zoom(np.zeros((2, 2, 2), np.uint8), 1.0, grid_mode=True)
    with pytest.raises(ValueError):
        RS.shift(np.zeros((2, 2), np.uint8), 1.0)
    assert not hasattr(RS, 'rotate')


def test_hv_resample_is_exported_and_parsed():
    import ctypes
    import __graft_entry__ as g
    g.build()
    import hvgan  # noqa: F401
    from hvgan import lib
    L = lib.get()
    structs, protos = lib.parse_header()
    assert hasattr(L.cdll, 'hv_resample') and hasattr(L.cdll, 'hv_resample_tile')
    res, args = protos['hv_resample']
    assert res is ctypes.c_int and len(args) == 18
    assert args[0] is ctypes.c_void_p and args[2] is ctypes.c_longlong and args[16] is ctypes.POINTER(structs['hv_resample_desc'])
    d = structs['hv_resample_desc']
    assert [n for n, _ in d._fields_] == ['form', 'matrix', 'offset', 'zoom', 'shift', 'order', 'mode', 'cval']
    assert d.matrix.size == 72 and d.offset.size == 24 and ctypes.sizeof(d) == 168
    dims = (ctypes.c_int * 3)()
    assert L.cdll.hv_resample_tile(dims) == 0 and tuple(dims) == (R.TILE,) * 3
