"""The RHLV parameter sweep on the device (hv_rhlv_sweep through hvgan.evaluation.rhlv_sweep) against the reference's two scripts run at every
grid point (fixture G18) to the project's RHLV gate of 1e-12 relative with a floor of 1, and bit for bit against the one-setting path
(hv_rhlv_views_batch through rhlv_dataset) at every grid point: the sweep computes the same integers and folds the same doubles in the same
order, so nothing but equality is accepted there.  Inputs and CPU references: tests/rhlv_sweep_cases.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import rhlv_sweep_cases as S

pytestmark = pytest.mark.gpu
TOL = 1e-12
DTYPES = (torch.float32, torch.uint8)          # every dtype the RHLV entries accept


def _close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.all(np.abs(a - b) <= TOL * np.maximum(1.0, np.abs(b)))


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _device(vol, dtype, zfast):
    """uint8 id volume [H, W, Z] -> device tensor, z fastest in memory or z slowest (stored [Z, H, W])."""
    t = torch.from_numpy(np.ascontiguousarray(vol)).to(dtype).cuda()
    return t if zfast else t.permute(2, 0, 1).contiguous().permute(1, 2, 0)


@functools.lru_cache(maxsize=None)
def _swept(shape_no, dtype):
    """-> (device fakes, labels, the 5 x 5 sweep of the shape's random pairs)."""
    from hvgan import evaluation
    zfast = S.SHAPES[shape_no][1]
    fakes, labels = S.random_case(shape_no)[:2]
    f, l = [_device(v, dtype, zfast) for v in fakes], [_device(v, dtype, zfast) for v in labels]
    assert (f[0].stride(2) == 1 and f[0].stride(1) != 1) == zfast
    return f, l, evaluation.rhlv_sweep(f, l, [S.IDX] * len(f), S.DIVISORS, S.THRESHOLDS)


def test_sweep_matches_the_reference_scripts_at_every_grid_point():
    import hvgan  # noqa: F401
    from hvgan import evaluation
    g, names = S.g18()
    divs, thrs = [int(d) for d in g['divisors']], [float(t) for t in g['thresholds']]
    compared = raised = 0
    for n in names:
        idx = int(g[n + '/index'])
        fake, label = torch.from_numpy(g[n + '/fake']).cuda(), torch.from_numpy(g[n + '/label']).cuda()
        sweep = evaluation.rhlv_sweep([fake], [label], [idx], divs, thrs)
        rec = sweep['records']
        assert rec.shape == (1, len(divs), len(thrs), 2, 16) and sweep['views'] == S.VIEWS and sweep['raised'].shape == (1, len(divs))
        assert np.array_equal(sweep['length_divisors'], divs) and np.array_equal(sweep['height_thresholds'], thrs)
        assert np.all(rec[..., 15] == 0) and np.all(rec[..., 0, 14] == 0)
        # the one-setting path at the reference's defaults: the same bits, flags included
        one, present = evaluation.rhlv_dataset([fake], [label], [idx], 5, 0.64)
        assert _same_bits(rec[:, divs.index(5), thrs.index(0.64)], one), n
        if g[n + '/absent']:
            assert np.all(rec == 0) and not sweep['raised'].any() and not present[0]
            assert np.isnan(evaluation.svm_feature_grid(sweep)).all()
            continue
        assert np.all(rec[..., 13] == 1)
        feats = evaluation.svm_feature_grid(sweep)
        for v, view in enumerate(S.VIEWS):
            out, marks = g['%s/%s/out' % (n, view)], g['%s/%s/raised' % (n, view)] != 0
            assert np.all(marks == marks[:, :1])                     # the scripts raise per divisor, whatever the threshold
            if view == 'coronal':
                assert np.array_equal(sweep['raised'][0], marks[:, 0]), (n, sweep['raised'], marks[:, 0])
                assert np.array_equal(rec[0, :, :, v, 14] != 0, marks)
                assert np.array_equal(np.isnan(feats[0]).all(axis=-1), marks) and np.array_equal(np.isnan(feats[0]).any(axis=-1), marks)
            else:
                assert not marks.any()
            ok = ~marks
            assert _close(rec[0, :, :, v, :5][ok], out[ok]), (n, view, np.abs(rec[0, :, :, v, :5][ok] - out[ok]).max())
            usable = ok & (g[n + '/coronal/raised'] == 0)             # a feature row is NaN in both views where the coronal script raises
            assert _close(feats[0, :, :, 3 * v:3 * v + 3][usable], out[usable][:, 1:4])
            compared += int(ok.sum())
            raised += int(marks.sum())
    assert compared >= 300 and raised >= 10, (compared, raised)


@pytest.mark.parametrize('dtype', DTYPES, ids=('float32', 'uint8'))
@pytest.mark.parametrize('shape_no', range(len(S.SHAPES)), ids=['x'.join(map(str, s)) + ('_zfast' if z else '') for s, z in S.SHAPES])
def test_every_grid_point_has_the_bits_of_the_one_setting_path(shape_no, dtype):
    import hvgan  # noqa: F401
    from hvgan import evaluation
    f, l, sweep = _swept(shape_no, dtype)
    rec = sweep['records']
    ref = S.random_case(shape_no)[2]
    assert rec.shape == (S.PAIRS, len(S.DIVISORS), len(S.THRESHOLDS), 2, 16)
    for d, div in enumerate(S.DIVISORS):
        for t, thr in enumerate(S.THRESHOLDS):
            one, present = evaluation.rhlv_dataset(f, l, [S.IDX] * len(f), div, thr)
            assert present.all()
            assert _same_bits(rec[:, d, t], one), (div, thr, np.abs(rec[:, d, t] - one).max())
    # and the numbers are the restatement's
    assert _close(rec[..., :14], ref), np.abs(rec[..., :14] - ref).max()
    assert np.array_equal(sweep['raised'], S.random_case(shape_no)[3])


def test_refused_grids_launch_nothing():
    import hvgan  # noqa: F401
    from hvgan import lib
    L = lib.get()
    fakes, labels = S.random_case(0)[:2]
    f, l = _device(fakes[0], torch.uint8, True), _device(labels[0], torch.uint8, True)
    H, W, Z = f.shape
    table = torch.tensor([f.data_ptr(), l.data_ptr()], dtype=torch.int64).cuda()
    ids = torch.tensor([float(S.IDX)], dtype=torch.float32).cuda()
    ws = torch.zeros(L.size('hv_rhlv_sweep_workspace_bytes', W, Z, 3, 1, 16, 32) + 64, dtype=torch.uint8).cuda()
    poison = -12345.5
    out = torch.full((16 * 32 * 2 * 16,), poison, dtype=torch.float64).cuda()

    def call(divisors, thresholds, n_div=None, n_thr=None):
        grid = L.hv_rhlv_grid()
        grid.n_divisors, grid.n_thresholds = len(divisors) if n_div is None else n_div, len(thresholds) if n_thr is None else n_thr
        for i, d in enumerate(divisors):
            grid.divisor[i] = d
        for i, t in enumerate(thresholds):
            grid.threshold[i] = t
        rc = L.cdll.hv_rhlv_sweep(lib.ptr(table), lib.ptr(ids), 1, 1, ctypes.c_longlong(f.stride(0)), ctypes.c_longlong(f.stride(1)),
                                  ctypes.c_longlong(f.stride(2)), H, W, Z, 3, ctypes.byref(grid), lib.ptr(out), lib.ptr(ws),
                                  ctypes.c_size_t(ws.numel()), lib.stream())
        torch.cuda.synchronize()
        return rc

    UNSUPPORTED = -2
    assert call([5], [0.64] * 32, n_thr=33) == UNSUPPORTED          # 33 thresholds
    assert call([5, 0], [0.64]) == UNSUPPORTED                       # divisor 0
    assert call([5] * 16, [0.64], n_div=17) == UNSUPPORTED and call([5], [0.64], n_div=0) == UNSUPPORTED
    assert call([5], [0.64], n_thr=0) == UNSUPPORTED and call([-3], [0.64]) == UNSUPPORTED
    assert torch.all(out == poison) and not ws.any()
    # the same call with the grid at its caps runs, and fills exactly its records
    assert call(list(range(1, 17)), [0.03 * (i + 1) for i in range(32)]) == 0
    assert not torch.any(out == poison)
    assert call([5], [0.64]) == 0 and L.cdll.hv_rhlv_sweep(lib.ptr(table), lib.ptr(ids), 1, 1, ctypes.c_longlong(f.stride(0)),
                                                            ctypes.c_longlong(f.stride(1)), ctypes.c_longlong(f.stride(2)), H, W, Z, 3,
                                                            ctypes.byref(L.hv_rhlv_grid(1, (ctypes.c_int * 16)(5), 1, (ctypes.c_double * 32)(0.64))),
                                                            lib.ptr(out), lib.ptr(ws), ctypes.c_size_t(8), lib.stream()) == -3


def test_the_grid_really_sweeps():
    import hvgan  # noqa: F401
    wrapped = 0
    for shape_no in range(len(S.SHAPES)):
        rec = _swept(shape_no, torch.uint8)[2]['records']
        for k in range(S.PAIRS):
            for v in range(2):
                assert S.distinct(rec[k, :, :, v]) >= 10, (shape_no, k, v, S.distinct(rec[k, :, :, v]))
        # divisor 1000: length 0, an empty range -- zeros, and the original exists
        assert S.DIVISORS[-1] == 1000 and np.all(rec[:, -1, :, :, :13] == 0) and np.all(rec[:, -1, :, :, 13] == 1)
        assert np.all(rec[:, -1, :, :, 14:] == 0)
        # divisor 1 drives centre - length negative (numpy's wrap-around branch) -- and the device follows the restatement there
        wraps = S.random_case(shape_no)[4]
        wrapped += int(wraps.sum())
        ref = S.random_case(shape_no)[2]
        assert S.DIVISORS[0] == 1
        for k, v in zip(*np.nonzero(wraps)):
            assert _close(rec[k, 0, :, v, :14], ref[k, 0, :, v]) and np.any(rec[k, 0, :, v, :13] != 0)
    assert wrapped >= 1


def test_batch_chunk_and_sub_grid_invariance():
    import hvgan  # noqa: F401
    from hvgan import evaluation
    f, l, sweep = _swept(0, torch.uint8)
    full = sweep['records']
    # five pairs: the three of the shape, and two of them again with the roles swapped
    f5, l5 = f + [l[0], l[1]], l + [f[0], f[1]]
    batch = evaluation.rhlv_sweep(f5, l5, [S.IDX] * 5, S.DIVISORS, S.THRESHOLDS)['records']
    assert _same_bits(batch[:3], full)
    chunked = evaluation.rhlv_sweep(f5, l5, [S.IDX] * 5, S.DIVISORS, S.THRESHOLDS, chunk=2)['records']
    assert _same_bits(chunked, batch)
    for k in (0, 3, 4):
        alone = evaluation.rhlv_sweep([f5[k]], [l5[k]], [S.IDX], S.DIVISORS, S.THRESHOLDS)['records']
        assert _same_bits(alone[0], batch[k]), k
    # one divisor, two thresholds: the corresponding entries of the full grid
    sub = evaluation.rhlv_sweep(f5, l5, [S.IDX] * 5, S.DIVISORS[1:2], S.THRESHOLDS[1:4:2])['records']
    assert sub.shape == (5, 1, 2, 2, 16) and _same_bits(sub, batch[:, 1:2, 1:4:2])
    # one view: that view's records
    for view in S.VIEWS:
        single = evaluation.rhlv_sweep(f5, l5, [S.IDX] * 5, S.DIVISORS, S.THRESHOLDS, views=(view,))
        assert single['views'] == (view,) and _same_bits(single['records'][:, :, :, 0], batch[:, :, :, S.VIEWS.index(view)])
    # grids beyond the entry's caps are split over several calls: 18 divisors x 34 thresholds, the 5 x 5 grid inside it
    divs = list(range(3000, 3013)) + list(S.DIVISORS)
    thrs = [0.01 * i for i in range(1, 30)] + list(S.THRESHOLDS)
    big = evaluation.rhlv_sweep(f5, l5, [S.IDX] * 5, divs, thrs, chunk=3)
    assert big['records'].shape == (5, 18, 34, 2, 16) and big['raised'].shape == (5, 18)
    assert _same_bits(big['records'][:, 13:, 29:], batch)


def test_absent_vertebra_and_empty_generated_volume():
    import hvgan  # noqa: F401
    from hvgan import evaluation
    f, l, _ = _swept(0, torch.uint8)
    fakes, labels, ids = [f[0], torch.zeros_like(f[1]), f[2]], [l[0], l[1], l[2]], [S.IDX + 30, S.IDX, S.IDX]
    sweep = evaluation.rhlv_sweep(fakes, labels, ids, S.DIVISORS, S.THRESHOLDS)
    rec = sweep['records']
    # pair 0: the original lacks the id -- zeros, the existence flag 0; pair 1: nothing generated -- zeros, the original exists
    assert np.all(rec[0] == 0) and np.all(rec[1, ..., :13] == 0) and np.all(rec[1, ..., 13] == 1) and np.all(rec[1, ..., 14:] == 0)
    assert not sweep['raised'][:2].any()
    for d, div in enumerate(S.DIVISORS[:2]):
        one, present = evaluation.rhlv_dataset(fakes, labels, ids, div, S.THRESHOLDS[1])
        assert list(present) == [False, True, True] and _same_bits(rec[:, d, 1], one)
    assert _same_bits(rec[2], _swept(0, torch.uint8)[2]['records'][2])
    feats = evaluation.svm_feature_grid(sweep)
    assert np.isnan(feats[0]).all() and np.all(feats[1] == 0) and not np.isnan(feats[2]).any()
