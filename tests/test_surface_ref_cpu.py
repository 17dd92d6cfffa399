"""Pins tests/surface_ref.py -- the numpy restatement the GPU tests of hv_edt and hv_surface_distance compare with -- against scipy, numpy and
numbers worked out by hand, and checks what needs no GPU of the new entries: header declarations, library exports, wrapper refusals."""
import ctypes
import math
import os

import numpy as np
import pytest

import surface_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cases():
    for si, shape in enumerate(SR.edt_shapes()):
        for kind in SR.TARGET_SETS:
            T = SR.target_set(shape, kind, si)
            if T.any():                          # scipy's answer for an empty set is not a distance
                yield shape, kind, T


def test_edt_equals_scipy_bit_for_bit_at_unit_spacing():
    from scipy.ndimage import distance_transform_edt
    n = 0
    for shape, kind, T in _cases():
        got, ref = SR.edt(T), distance_transform_edt(~T)
        assert got.dtype == np.float64 and np.array_equal(got, ref), (shape, kind)
        n += 1
    assert n >= 5 * len(SR.edt_shapes()) - 8     # only tiny shapes lose their random set


def test_edt_anisotropic_is_within_the_recorded_difference_of_scipy():
    from scipy.ndimage import distance_transform_edt
    worst = 0.0
    for shape, kind, T in _cases():
        for sp in SR.SPACINGS[1:]:
            got, ref = SR.edt(T, sp), distance_transform_edt(~T, sampling=sp)
            assert np.array_equal(got == 0, ref == 0)
            nz = ref > 0
            if nz.any():
                worst = max(worst, float((np.abs(got - ref)[nz] / ref[nz]).max()))
    print('largest relative |restatement - scipy| over the anisotropic cases: %.3g (recorded %.3g, EDT_TOL %.3g)'
          % (worst, SR.MEASURED_REL, SR.EDT_TOL))
    assert worst <= SR.MEASURED_REL
    assert SR.EDT_TOL == max(10.0 * SR.MEASURED_REL, 1e-12)


def test_edt_per_axis_equals_all_pairs_bit_for_bit():
    for si, shape in enumerate([(5, 7, 33), (2, 8, 32), (7, 5, 1), (31, 1, 3)]):
        for kind in SR.TARGET_SETS:
            T = SR.target_set(shape, kind, si)
            for sp in SR.SPACINGS:
                assert np.array_equal(SR.edt(T, sp), SR.edt_allpairs(T, sp)), (shape, kind, sp)
    assert np.isposinf(SR.edt(np.zeros((3, 4, 5), dtype=bool))).all()


def test_surface_equals_the_scipy_erosion_expression():
    from scipy.ndimage import binary_erosion, generate_binary_structure
    st = generate_binary_structure(3, 1)
    rs = np.random.RandomState(3)
    masks = [SR.blob((20, 18, 12), (9.5, 8.0, 6.0), (7.0, 6.0, 4.0)), np.ones((4, 5, 6), dtype=bool), np.zeros((3, 3, 3), dtype=bool),
             rs.rand(9, 8, 7) < 0.7, rs.rand(1, 6, 5) < 0.5, np.ones((1, 1, 1), dtype=bool)]
    for X in masks:
        assert np.array_equal(SR.surface(X), X & ~binary_erosion(X, st, border_value=0)), X.shape
    assert SR.surface(np.ones((4, 5, 6), dtype=bool)).sum() == 4 * 5 * 6 - 2 * 3 * 4      # the set touches every face: its shell


def test_percentile_equals_numpy_bit_for_bit():
    rs = np.random.RandomState(5)
    for n in (1, 2, 20, 21, 400):
        for rep in range(5):
            x = rs.rand(n) * 50.0 if rep else np.sqrt(rs.randint(0, 40, size=n).astype(np.float64))      # rep 0: many ties
            assert SR.percentile95(x) == np.percentile(x, 95), (n, rep)


def test_analytic_cases():
    seen = set()
    for name, a, b, want in SR.analytic_cases():
        got = SR.metrics(a, b)
        for k, v in want.items():
            assert got[k] == v, (name, k, got[k], v)
        seen.add(name)
    assert seen == {'identical', 'two_voxels', 'cube_in_cube'}
    # the cube in the cube, by hand: the 152 distances b -> a are all 3; the 728 distances a -> b mean what the restatement says, and hd95 lies inside
    got = SR.metrics(*SR.analytic_cases()[2][1:3])
    assert got['assd'] == (got['asd_ab'] + 3.0) / 2.0 and 3.0 <= got['hd95'] <= math.sqrt(27.0)
    # millimetres: two voxels 2 apart along axis 2 at spacing 1.5 are 3 mm apart
    a, b = np.zeros((3, 3, 5), dtype=np.uint8), np.zeros((3, 3, 5), dtype=np.uint8)
    a[1, 1, 1] = b[1, 1, 3] = 1
    assert SR.metrics(a, b, spacing=(0.7, 0.7, 1.5))['hd'] == 3.0
    assert SR.metrics(a, np.zeros_like(a)) is None and SR.metrics(np.zeros_like(a), b) is None


# ------------------------------------------------------------------------------------------------ what needs no GPU of the new entries
NEW = ('hv_edt_workspace_bytes', 'hv_edt', 'hv_surface_distance_workspace_bytes', 'hv_surface_distance')


def test_header_declares_the_four_entries():
    import hvgan  # noqa: F401
    from hvgan import lib
    _, protos = lib.parse_header()
    for name in NEW:
        assert name in protos, name
    assert protos['hv_edt_workspace_bytes'] == (ctypes.c_size_t, [ctypes.c_int] * 3)
    assert protos['hv_surface_distance_workspace_bytes'] == (ctypes.c_size_t, [ctypes.c_int] * 3)
    res, args = protos['hv_edt']
    assert res is ctypes.c_int and len(args) == 16 and args[8] is ctypes.c_double and args[14] is ctypes.c_size_t
    res, args = protos['hv_surface_distance']
    assert res is ctypes.c_int and len(args) == 16 and args[9] is ctypes.c_double and args[11] is ctypes.c_int


def test_library_exports_them_and_sizes_are_host_arithmetic():
    import hvgan  # noqa: F401
    from hvgan import lib
    if not lib.available():
        pytest.skip('libhvgan.so not built')
    L = lib.get()
    for name in NEW:
        assert hasattr(L.cdll, name)
    up = lambda b: (b + 15) // 16 * 16
    assert L.size('hv_edt_workspace_bytes', 5, 7, 9) == up(5 * 7 * 9 * 4)
    assert L.size('hv_edt_workspace_bytes', 0, 7, 9) == 0 and L.size('hv_edt_workspace_bytes', 5, -1, 9) == 0
    n = 5 * 7 * 9
    want = 3 * up(8 * n) + up(4 * n) + up(n) + up(5 * 8 * 4) + up(5 * 2 * 4) + 2 * up(5 * 2 * 8) + 64
    assert L.size('hv_surface_distance_workspace_bytes', 5, 7, 9) == want
    assert L.size('hv_surface_distance_workspace_bytes', 5, 7, 0) == 0
    # refusals come before any device work: callable here.  NULL pointers, sizes, dtype, spacing, box
    ones, bad = (ctypes.c_double * 3)(1.0, 1.0, 1.0), (ctypes.c_double * 3)(1.0, 0.0, 1.0)
    p = ctypes.c_void_p(4096)
    ll = [ctypes.c_longlong(s) for s in (63, 9, 1)]
    ws = ctypes.c_size_t(1 << 20)

    def edt(vol=p, dt=0, dims=(5, 7, 9), sp=ones, box=None, out=p, status=p, w=p, wb=ws):
        return L.cdll.hv_edt(vol, dt, *ll, *dims, ctypes.c_double(1.0), sp, box, out, status, w, wb, None)

    for kw in (dict(vol=None), dict(out=None), dict(status=None), dict(w=None), dict(dt=1), dict(dt=6), dict(dims=(0, 7, 9)), dict(sp=None),
               dict(sp=bad), dict(sp=(ctypes.c_double * 3)(1.0, float('inf'), 1.0)), dict(wb=ctypes.c_size_t(5 * 7 * 9 * 4 - 1)),
               dict(box=(ctypes.c_int * 6)(0, 0, 0, 5, 7, 10)), dict(box=(ctypes.c_int * 6)(-1, 0, 0, 5, 7, 9)),
               dict(box=(ctypes.c_int * 6)(1, 0, 0, 5, 7, 9)), dict(box=(ctypes.c_int * 6)(0, 0, 0, 0, 7, 9)), dict(out=ctypes.c_void_p(4100)),
               dict(w=ctypes.c_void_p(4104))):
        assert edt(**kw) == -1, kw

    def sd(a=p, b=p, dt=0, dims=(5, 7, 9), sp=ones, r=1, out=p, w=p, wb=ws):
        return L.cdll.hv_surface_distance(a, b, dt, *ll, *dims, ctypes.c_double(1.0), sp, r, out, w, wb, None)

    for kw in (dict(a=None), dict(b=None), dict(out=None), dict(w=None), dict(dt=2), dict(dims=(5, 7, -9)), dict(sp=bad), dict(r=2),
               dict(wb=ctypes.c_size_t(want - 1))):
        assert sd(**kw) == -1, kw
    assert edt(dims=(2, 20000, 2), wb=ctypes.c_size_t(1 << 30)) == -2          # a line that does not fit the staging


def test_wrapper_refusals_come_before_any_device_work():
    import hvgan  # noqa: F401
    from hvgan import generation_eval as GE
    v = np.zeros((4, 5, 6), dtype=np.uint8)
    for sp in (0.0, -1.0, (1.0, 2.0), (1.0, float('nan'), 1.0), 'x', ((1, 2), 1, 1)):
        with pytest.raises(ValueError):
            GE.distance_transform(v, spacing=sp)
        with pytest.raises(ValueError):
            GE.surface_distances(v, v, spacing=sp)
        with pytest.raises(ValueError):
            GE.surface_distances_batch([(v, v, 1)], spacing=sp)
    with pytest.raises(ValueError):
        GE.distance_transform(v, value='0')
    with pytest.raises(ValueError):
        GE.distance_transform(v[0])
    for box in ((0, 0, 0, 4, 5, 7), (0, 0, 0, 0, 5, 6), (-1, 0, 0, 4, 5, 6), (0, 0, 0, 4, 5), 'box'):
        with pytest.raises(ValueError):
            GE.distance_transform(v, box=box)
    with pytest.raises(ValueError):
        GE.distance_transform(v, out=np.zeros((4, 5, 6)))
    with pytest.raises(ValueError):
        GE.surface_distances_batch([(v, v)])
    assert GE.surface_distances_batch([]) == []
    assert GE.SURFACE_KEYS == ('hd', 'hd95', 'assd', 'asd_ab', 'asd_ba', 'n_a', 'n_b')
