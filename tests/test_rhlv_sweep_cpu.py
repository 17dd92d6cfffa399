"""The RHLV parameter sweep on the CPU: the float64 restatement tests/height_map_ref.py against the reference's two scripts run at every point
of a (length_divisor, height_threshold) grid (fixture G18, tools/make_golden_rhlv_sweep.py), the host-side svm_feature_grid, the C ABI's
declaration and export, and that the random cases of tests/test_rhlv_sweep_gpu.py hold what that file relies on.  The restatement differs from
the scripts only in one float64 product per generated height and numpy's mean: 1e-12 relative with a floor of 1, as everywhere for RHLV."""
import ctypes

import numpy as np

import rhlv_sweep_cases as S

TOL = 1e-12


def _close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.all(np.abs(a - b) <= TOL * np.maximum(1.0, np.abs(b)))


def test_restatement_reproduces_every_grid_point_of_g18():
    g, names = S.g18()
    assert len(names) >= 5 and len(g['divisors']) >= 5 and len(g['thresholds']) >= 5
    compared = raised = absent = 0
    for n in names:
        idx = int(g[n + '/index'])
        if g[n + '/absent']:
            absent += 1
            for view in S.VIEWS:
                rec, r = S.reference_record(g[n + '/fake'], g[n + '/label'], idx, 5, 0.64, view)
                assert rec[13] == 0 and not r
            continue
        for view in S.VIEWS:
            out, marks = g['%s/%s/out' % (n, view)], g['%s/%s/raised' % (n, view)]
            for d, div in enumerate(g['divisors']):
                for t, thr in enumerate(g['thresholds']):
                    rec, r = S.reference_record(g[n + '/fake'], g[n + '/label'], idx, int(div), float(thr), view)
                    assert r == bool(marks[d, t]), (n, view, div, thr)
                    assert rec[13] == 1
                    if r:
                        raised += 1
                        assert np.all(np.isnan(out[d, t]))
                        continue
                    assert _close(rec[:5], out[d, t]), (n, view, div, thr, rec[:5], out[d, t])
                    compared += 1
    assert compared >= 300 and raised >= 10 and absent >= 1, (compared, raised, absent)


def test_svm_feature_grid_orders_the_columns_and_marks_unusable_settings():
    import hvgan  # noqa: F401
    from hvgan import evaluation
    N, D, T = 3, 2, 4
    rec = np.zeros((N, D, T, 2, 16))
    # value = 1000 n + 100 d + 10 t + field, negative in the coronal view
    n, d, t, f = np.meshgrid(np.arange(N), np.arange(D), np.arange(T), np.arange(16), indexing='ij')
    rec[:, :, :, 0] = 1000 * n + 100 * d + 10 * t + f
    rec[:, :, :, 1] = -rec[:, :, :, 0]
    rec[:, :, :, :, 13] = 1.0
    rec[2, :, :, :, 13] = 0.0                              # pair 2: the original lacks the vertebra
    raised = np.zeros((N, D), dtype=bool)
    raised[1, 1] = True                                    # pair 1, divisor 1: the coronal script raises
    sweep = {'records': rec, 'views': ('sagittal', 'coronal'), 'raised': raised, 'length_divisors': np.arange(D) + 1,
             'height_thresholds': np.linspace(0.3, 0.9, T)}
    feats = evaluation.svm_feature_grid(sweep)
    assert feats.shape == (N, D, T, 6) and feats.dtype == np.float64
    assert np.array_equal(feats[0, 1, 2], [121.0, 122.0, 123.0, -121.0, -122.0, -123.0])
    # one grid point of one pair is svm_features of that setting's records
    assert np.array_equal(feats[:2, 0, 3], evaluation.svm_features(rec[:2, 0, 3]))
    nan = np.isnan(feats)
    assert nan[2].all() and nan[1, 1].all() and not nan[0].any() and not nan[1, 0].any()
    assert np.array_equal(nan.all(axis=-1), nan.any(axis=-1))
    assert not np.isnan(rec).any()                         # the input is left alone
    # the views in the other order carry their names along
    swapped = dict(sweep, records=rec[:, :, :, ::-1], views=('coronal', 'sagittal'))
    assert np.array_equal(evaluation.svm_feature_grid(swapped), feats, equal_nan=True)


def test_header_declares_the_sweep_and_the_library_exports_it():
    import __graft_entry__ as g
    g.build()
    import hvgan  # noqa: F401
    from hvgan import lib
    structs, protos = lib.parse_header()
    assert 'hv_rhlv_sweep' in protos and 'hv_rhlv_sweep_workspace_bytes' in protos
    grid = structs['hv_rhlv_grid']
    assert [n for n, _ in grid._fields_] == ['n_divisors', 'divisor', 'n_thresholds', 'threshold']
    assert ctypes.sizeof(grid) == 4 + 16 * 4 + 4 + 32 * 8 and grid.threshold.offset % 8 == 0
    assert protos['hv_rhlv_sweep'][0] is ctypes.c_int and protos['hv_rhlv_sweep'][1][11] == ctypes.POINTER(grid)
    L = lib.get()
    assert hasattr(L.cdll, 'hv_rhlv_sweep') and hasattr(L.cdll, 'hv_rhlv_sweep_workspace_bytes')
    # host-only: the size of the workspace, 0 for what the entry refuses; one pair's slab holds the one-setting entries' slab
    one = L.size('hv_rhlv_sweep_workspace_bytes', 40, 28, 3, 1, 5, 5)
    assert one > L.size('hv_rhlv_views_workspace_bytes', 40, 28, 3, 1) and one % 8 == 0
    assert L.size('hv_rhlv_sweep_workspace_bytes', 40, 28, 3, 7, 5, 5) == 7 * one
    assert L.size('hv_rhlv_sweep_workspace_bytes', 40, 28, 3, 1, 16, 32) > one
    for bad in ((40, 28, 3, 1, 17, 5), (40, 28, 3, 1, 5, 33), (40, 28, 3, 1, 0, 5), (40, 28, 3, 1, 5, 0), (40, 28, 4, 1, 5, 5), (40, 28, 3, 0, 5, 5)):
        assert L.size('hv_rhlv_sweep_workspace_bytes', *bad) == 0, bad


def test_random_cases_sweep_for_the_reference_itself():
    """What tests/test_rhlv_sweep_gpu.py asserts of the device records holds for the restatement: the 25 grid points give at least 10 distinct
    records per view, divisor 1 wraps for some pair, divisor 1000 is an empty range."""
    for shape_no in range(len(S.SHAPES)):
        fakes, labels, rec, raised, wraps = S.random_case(shape_no)
        assert wraps.any(), shape_no
        assert np.all(rec[:, -1, :, :, :13] == 0) and np.all(rec[..., 13] == 1)
        for v in range(2):
            assert S.distinct(rec[0, :, :, v]) >= 10, (shape_no, v, S.distinct(rec[0, :, :, v]))
