"""tests/warp_ref.py -- the numpy restatement the device's deformable resampling is compared with -- against scipy.ndimage.map_coordinates:
np.array_equal and equal dtype.  No GPU.  Order 3 is pinned on scipy's own coefficients (prefilter=False), as in test_resample_ref_cpu.py."""
import numpy as np
import pytest
from scipy import ndimage

import resample_ref as R
import warp_ref as W

DT = pytest.mark.parametrize('dtype', R.DTYPES, ids=lambda d: np.dtype(d).name)
CDT = pytest.mark.parametrize('cdtype', (np.float64, np.float32), ids=lambda d: np.dtype(d).name)
OM = pytest.mark.parametrize('order,mode', W.ORDER_MODES)
GORD = pytest.mark.parametrize('gorder', (1, 3))


def _WP():
    import hvgan  # noqa: F401
    from hvgan import warp
    return warp


def _same(got, want, what=None):
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), what


def _coef(v):
    return ndimage.spline_filter(v, 3, output=np.float64, mode='mirror')


def _scipy(src, u, dtype, order, mode, cval=W.CVAL):
    return ndimage.map_coordinates(src, u, output=dtype, order=order, mode=mode, cval=cval, prefilter=False)


# ------------------------------------------------------------------------------------------------ 1. map_coordinates
@DT
@CDT
@OM
def test_map_coordinates_equals_scipy(order, mode, cdtype, dtype):
    """Every source dtype with every output dtype, random coordinates and the edge list (0, A - 1, one ulp beyond and inside, -0.0, NaN).
    Found: scipy gives cval at a NaN coordinate for the integer outputs too (mode constant), and index 0 in mode nearest; so does sample()."""
    v = R.case_volume(dtype)
    src = _coef(v) if order == 3 else v
    for u in (W.case_coordinates((4, 5, 6), cdtype), W.edge_coordinates(cdtype)):
        for out_dtype in R.DTYPES:
            want = _scipy(src, u, out_dtype, order, mode)
            got = W.map_coordinates(v, u, order=order, mode=mode, cval=W.CVAL, output=out_dtype, coef=src if order == 3 else None)
            _same(got, want, (order, mode, cdtype, dtype, out_dtype))
    e = W.edge_coordinates(cdtype)
    if mode == 'constant':
        t = W.map_coordinates(v, e, order=order, cval=W.CVAL, output=np.float64, coef=src if order == 3 else None)
        nan = np.isnan(e).any(axis=0)
        assert nan.sum() == 3 and (t[nan] == W.CVAL).all()
        beyond = ((e < 0) | (e > np.array(v.shape)[:, None] - 1)).any(axis=0)
        assert beyond.sum() == 6 and (t[beyond] == W.CVAL).all()


@DT
def test_displacement_rule_equals_scipy_at_the_summed_coordinates(dtype):
    v = R.case_volume(dtype)
    d = W.case_displacement(v.shape)
    u = W.coords_displacement(d)
    o = np.stack(np.meshgrid(*[np.arange(n) for n in v.shape], indexing='ij')).astype(np.float64)
    assert np.array_equal(u.reshape(d.shape), o + d)
    for order in (0, 1, 3):
        src = _coef(v) if order == 3 else v
        _same(W.warp(v, d, order=order, cval=W.CVAL, coef=src), _scipy(src, u, v.dtype, order, 'constant').reshape(v.shape), order)
    mm = (0.7, 0.7, 1.5)
    _same(W.warp(v, d, spacing=mm, order=1, cval=W.CVAL), _scipy(v, (o + d / np.array(mm).reshape(3, 1, 1, 1)).reshape(3, -1), v.dtype, 1,
                                                                  'constant').reshape(v.shape), 'spacing')
    _same(W.warp(v, d.astype(np.float32), order=1, cval=W.CVAL),
          _scipy(v, (o + d.astype(np.float32).astype(np.float64)).reshape(3, -1), v.dtype, 1, 'constant').reshape(v.shape), 'float32 field')


# ------------------------------------------------------------------------------------------------ 2. the control grid
@GORD
@pytest.mark.parametrize('G', W.GRIDS)
def test_control_grid_displacement_and_warp_equal_scipy(G, gorder):
    """d_h against scipy's own sampling of grid[h] at the explicitly clamped q, bit for bit; the warped volume against scipy at u."""
    out_shape = (8, 7, 9)
    values = W.case_grid(G)
    for gzoom, gshift in ((W.control_gzoom(G, out_shape), (0.0, 0.0, 0.0)), ((0.9, 1.1, 0.8), (-2.5, -1.0, -3.0))):     # the second leaves the grid on both sides
        q = W.grid_coordinate(out_shape, G, gzoom, gshift)
        if gshift[0] != 0.0:
            for n, s, z, g in zip(out_shape, gshift, gzoom, G):
                x = (np.arange(n, dtype=np.float64) + s) * z
                assert x.min() < 0 and x.max() > g - 1
        assert (q >= 0).all() and (q <= np.array(G)[:, None] - 1).all()
        d = W.displacement_of(values, out_shape, gzoom, gshift, gorder)
        for h in range(3):
            want = ndimage.map_coordinates(values[h], q, output=np.float64, order=gorder, mode='constant', cval=0.0, prefilter=False)
            _same(d[h].ravel(), want, (G, gorder, h))
        for form, a, b in (('zoomshift', (0.8, 1.25, 0.6), (0.3, -0.4, 0.2)), ('matrix', R.MATRIX, R.OFFSET)):
            u = W.coords_grid(out_shape, values, gzoom, gshift, gorder, form, a, b)
            base = R.coords_matrix(out_shape, a, b) if form == 'matrix' else R.coords_zoomshift(out_shape, a, b)
            assert np.array_equal(u, base + d.reshape(3, -1))
            for dtype in (np.int16, np.float64):
                v = R.case_volume(dtype)
                for order in (0, 1, 3):
                    src = _coef(v) if order == 3 else v
                    got = W.warp_grid(v, values, out_shape, gorder, gzoom, gshift, form, a, b, order=order, cval=W.CVAL, coef=src)
                    _same(got, _scipy(src, u, v.dtype, order, 'constant').reshape(out_shape), (G, gorder, form, dtype, order))


# ------------------------------------------------------------------------------------------------ 3. random_control_grid
def test_random_control_values_seed_border_clip_and_the_products_equal():
    WP = _WP()
    out_shape, spacing = (32, 24, 10), (0.7, 0.7, 1.5)
    for fix_border in (True, False):
        a = W.random_control_values(out_shape, spacing, 5.0, 6.0, 7, fix_border)
        b = W.random_control_values(out_shape, spacing, 5.0, 6.0, 7, fix_border)
        assert a.tobytes() == b.tobytes() and a.dtype == np.float64
        assert a.shape == (3, 6, 5, 4)                            # ceil(31 / 7.142..) + 1, ceil(23 / 7.142..) + 1, ceil(9 / 3.33..) + 1
        assert a.tobytes() != W.random_control_values(out_shape, spacing, 5.0, 6.0, 8, fix_border).tobytes()
        delta = W.control_spacing(out_shape, a.shape[1:], spacing, 5.0)
        for h in range(3):
            assert np.abs(a[h]).max() <= 0.4 * delta[h]
        assert any(np.abs(a[h]).max() == 0.4 * delta[h] for h in range(3))            # the amplitude is large enough for the clip to act
        border = np.ones(a.shape[1:], dtype=bool)
        border[1:-1, 1:-1, 1:-1] = False
        assert (a[:, border] == 0).all() == fix_border and (a[:, ~border] != 0).all()
        assert WP.random_control_values(out_shape, spacing, 5.0, 6.0, 7, fix_border).tobytes() == a.tobytes()
    one = W.random_control_values((1, 9, 9), (1.0, 1.0, 1.0), 4.0, 1.0, 0)
    assert one.shape == (3, 1, 3, 3) and WP.random_control_values((1, 9, 9), (1.0, 1.0, 1.0), 4.0, 1.0, 0).tobytes() == one.tobytes()
    for bad in (dict(control_mm=0.0), dict(amplitude_mm=-1.0), dict(clip=float('nan')), dict(spacing=(1.0, 0.0, 1.0))):
        kw = dict(out_shape=(8, 8, 8), spacing=(1.0, 1.0, 1.0), control_mm=4.0, amplitude_mm=1.0, seed=0)
        kw.update(bad)
        with pytest.raises(ValueError):
            WP.random_control_values(**kw)


# ------------------------------------------------------------------------------------------------ 4. and 5. properties
@GORD
def test_zero_grid_gives_the_base_lattice(gorder):
    for dtype in R.DTYPES:
        v = R.case_volume(dtype)
        z = np.zeros((3, 4, 5, 3))
        for order in (0, 1, 3):
            _same(W.warp_grid(v, z, R.OUT_SHAPE, gorder, form='matrix', a=R.MATRIX, b=R.OFFSET, order=order, cval=W.CVAL),
                  R.affine_transform(v, R.MATRIX, R.OFFSET, R.OUT_SHAPE, order=order, cval=W.CVAL), (dtype, order, 'matrix'))
            _same(W.warp_grid(v, z, R.OUT_SHAPE, gorder, form='zoomshift', a=R.DIAGONAL, b=R.DIAG_OFFSET / R.DIAGONAL, order=order, cval=W.CVAL),
                  R.affine_transform(v, R.DIAGONAL, R.DIAG_OFFSET, R.OUT_SHAPE, order=order, cval=W.CVAL), (dtype, order, 'diagonal'))


def test_label_and_ct_through_one_grid_stay_registered():
    """The order-0 warp of a label picks, for every output voxel, the voxel the CT's order-1 warp is centred on: the warped label's
    indicator is the order-0 warp of the indicator, for every label value."""
    shape = (16, 16, 8)
    r = np.random.RandomState(5)
    label = (r.random_sample(shape) * 4).astype(np.uint8)
    values = W.random_control_values(shape, (0.7, 0.7, 1.5), 4.0, 3.0, 3)
    assert np.abs(values).max() > 1.0
    wl = W.warp_grid(label, values, shape, 3, order=0, cval=0)
    assert (wl != label).any()
    for k in (1, 2, 3):
        _same((wl == k).astype(np.uint8), W.warp_grid((label == k).astype(np.uint8), values, shape, 3, order=0, cval=0), k)
    ct = R.case_volume(np.int16, shape, seed=6)
    u = W.coords_grid(shape, values, W.control_gzoom(values.shape[1:], shape), (0.0, 0.0, 0.0), 3)
    _same(W.warp_grid(ct, values, shape, 3, order=1, cval=-32768), _scipy(ct, u, np.int16, 1, 'constant', -32768).reshape(shape), 'ct')
    _same(wl, _scipy(label, u, np.uint8, 0, 'constant', 0).reshape(shape), 'label')


# ------------------------------------------------------------------------------------------------ the host rules of warp.py
def test_python_refusals_and_the_header():
    import ctypes
    import torch
    import __graft_entry__ as g
    g.build()
    WP = _WP()
    from hvgan import lib
    for gorder in (0, 2, 4, True, 3.0):
        with pytest.raises(ValueError, match='gorder'):
            WP._check_gorder(gorder)
    with pytest.raises(ValueError, match='grid'):
        WP._check_grid((1, 2, 3))
    with pytest.raises(ValueError, match='ct_order'):
        WP.elastic_pair(np.zeros((2, 2, 2), np.int16), np.zeros((2, 2, 2), np.uint8), None, ct_order=0)
    with pytest.raises(ValueError, match='displacement'):
        WP.warp(np.zeros((2, 2, 2), np.int16), np.zeros((3, 2, 2, 3)))
    with pytest.raises(ValueError, match='values'):
        WP.control_grid(np.zeros((2, 2, 2, 2)), (4, 4, 4))
    assert WP.ABSOLUTE == W.ABSOLUTE == 0 and WP.DISPLACEMENT == W.DISPLACEMENT == 1
    structs, protos = lib.parse_header()
    L = lib.get()
    for name in ('hv_map_coordinates', 'hv_warp_grid', 'hv_map_coordinates_tile', 'hv_warp_grid_tile'):
        assert hasattr(L.cdll, name)
    assert len(protos['hv_map_coordinates'][1]) == 27 and len(protos['hv_warp_grid'][1]) == 26
    d = structs['hv_warp_desc']
    assert [n for n, _ in d._fields_] == ['base', 'gzoom', 'gshift', 'gorder']
    assert d.base.size == ctypes.sizeof(structs['hv_resample_desc']) == 168 and ctypes.sizeof(d) == 224
    assert protos['hv_warp_grid'][1][24] is ctypes.POINTER(d)
    for fn in (L.cdll.hv_map_coordinates_tile, L.cdll.hv_warp_grid_tile):
        dims = (ctypes.c_int * 3)()
        assert fn(dims) == 0 and tuple(dims) == (R.TILE,) * 3
    assert torch.float64 in WP._COORD_DT and torch.float32 in WP._COORD_DT and len(WP._COORD_DT) == 2
