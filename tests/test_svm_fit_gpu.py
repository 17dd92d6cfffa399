"""Fitting the grader on the device, keeping it and grading new rows (hv_svm_fit / hv_svm_predict / hv_svm_features through hvgan.evaluation's
svm_fit, svm_predict and Grader) against the numpy restatement tests/svm_fit_ref.py, against scikit-learn's recorded answers (fixture G22,
tools/make_golden_svm_fit.py) and, bit for bit, against the grading kernels of svm_grade_grid on fixture G19 -- the test that keeps ONE solver and
ONE vote in csrc/svm_grade.hip.  Solver tolerance: svm_fit_ref.SOLVER_TOL (ten times the measured difference between the restatement and
scikit-learn's SVC at tol=1e-10; G22's measurement is below G19's, so it is G19's constant)."""
import ctypes
import functools
import os

import numpy as np
import pytest

import svm_fit_ref as FR
import svm_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
CAP = 0.01
FIT_KEYS = ('mean', 'scale', 'w', 'b', 'gap', 'iterations', 'status', 'support', 'pair_rows', 'unusable')


@functools.lru_cache(maxsize=None)
def g22():
    return FR.g22(GOLDEN)


@functools.lru_cache(maxsize=None)
def g19():
    return dict(np.load(os.path.join(GOLDEN, 'g19_svm_grading.npz')))


@functools.lru_cache(maxsize=None)
def ref(case):
    g = g22()
    return FR.fit(g[case + '/X'], g[case + '/y'])


@functools.lru_cache(maxsize=None)
def device(case, tol):
    from hvgan import evaluation
    g = g22()
    return evaluation.svm_fit(g[case + '/X'], g[case + '/y'], tol=tol)


def close(a, b, tol):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.all(np.abs(a - b)[~np.isnan(a)] <= tol)


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------- 1. against the restatement and scikit-learn
@pytest.mark.parametrize('case', FR.CASES)
def test_tight_fit_matches_the_restatement(case):
    import hvgan  # noqa: F401
    from hvgan import evaluation
    g, d, r = g22(), device(case, 1e-10), ref(case)
    assert np.array_equal(d['classes'], r['classes']) and np.array_equal(d['present'], r['present']) and not d['unusable']
    assert np.all(d['status'] == evaluation.CONVERGED) and np.all(d['gap'] <= 1e-10) and np.array_equal(d['pair_rows'], r['pair_rows'])
    assert close(d['mean'], r['mean'], 1e-12) and close(d['scale'], r['scale'], 1e-12)
    out = evaluation.svm_predict(d, g[case + '/X_held'], decisions=True)
    pred, dec = FR.predict(r, g[case + '/X_held'])
    for k, a, b in (('w', d['w'], r['w']), ('b', d['b'], r['b']), ('decision', out['decision'], dec)):
        print(case, k, 'largest |device - svm_fit_ref|', np.max(np.abs(a - b)))
    assert close(d['w'], r['w'], FR.SOLVER_TOL) and close(d['b'], r['b'], FR.SOLVER_TOL) and close(out['decision'], dec, FR.SOLVER_TOL)
    assert np.all(d['support'] > 0) and np.all(d['iterations'] > 0) and np.array_equal(d['rows'], np.arange(len(g[case + '/y'])))


@pytest.mark.parametrize('case', FR.CASES)
def test_default_tolerance_grades_held_out_rows_as_scikit_learn_does(case):
    import hvgan  # noqa: F401
    from hvgan import evaluation
    g, d = g22(), device(case, 1e-3)
    assert np.all(d['status'] == evaluation.CONVERGED) and np.all(d['gap'] <= 1e-3)
    grade = evaluation.svm_predict(d, g[case + '/X_held'])
    far = ~g[case + '/near']
    assert (~far).mean() <= CAP
    assert grade.shape == far.shape and np.array_equal(grade[far], g[case + '/pred'][far])


# ---------------------------------------------------------------- 2. bit identity with the grading kernels
@pytest.mark.parametrize('case', R.CASES)
def test_fit_and_predict_are_bit_for_bit_the_grading_kernels(case):
    import hvgan  # noqa: F401
    from hvgan import evaluation
    g = g19()
    X, y, Xv, yv = (g[case + '/' + k] for k in ('X_tt', 'y_tt', 'X_val', 'y_val'))
    dataset = np.array(['train'] * len(y) + ['val'] * len(yv))
    graded = evaluation.svm_grade_grid(np.concatenate([X, Xv]), np.concatenate([y, yv]), dataset, decisions=True)
    folds = graded['folds']
    assert X.shape[1] == (6 if case in ('b', 'c') else 3)
    for f in range(R.N_SPLITS):
        m = evaluation.svm_fit(X, y, train=folds != f)
        assert np.array_equal(m['classes'], graded['classes'])
        for k in ('w', 'b', 'gap', 'iterations', 'status', 'support'):
            assert same_bytes(m[k], graded[k][f]), (f, k)
        out = evaluation.svm_predict(m, Xv, decisions=True)
        assert np.array_equal(out['grade'], graded['pred'][f]) and same_bytes(out['decision'], graded['decision'][f]), f
    if case == 'e':
        assert (graded['status'] == evaluation.PAIR_ABSENT).any()


# ---------------------------------------------------------------- 3. independence of the grid and of the batch
def grid_tables():
    """G19's case f: train + test rows [37, 3, 3] and val rows [20, 3, 3] of its first grid row, labels."""
    g = g19()
    M = len(g['a/y_tt'])
    feats = g['f/features'][:, 0]
    return feats[:M], g['f/labels'][:M], feats[M:]


def test_a_grid_point_has_the_same_bytes_alone_in_the_grid_and_in_the_reversed_grid():
    import hvgan  # noqa: F401
    from hvgan import evaluation
    X, y, Xv = grid_tables()
    whole = evaluation.svm_fit(X, y)
    rev = evaluation.svm_fit(X[:, ::-1], y)
    pw = evaluation.svm_predict(whole, Xv, decisions=True, contributions=True)
    pr = evaluation.svm_predict(rev, Xv[:, ::-1], decisions=True, contributions=True)
    assert whole['w'].shape == (3, 3, 3) and pw['grade'].shape == (3, 20) and pw['contrib'].shape == (3, 20, 3, 3)
    assert len({whole['w'][j].tobytes() for j in range(3)}) == 3
    for j in range(3):
        alone = evaluation.svm_fit(X[:, j], y)
        pa = evaluation.svm_predict(alone, Xv[:, j], decisions=True, contributions=True)
        for k in FIT_KEYS:
            assert same_bytes(alone[k], whole[k][j]) and same_bytes(rev[k][2 - j], whole[k][j]), (j, k)
        for k in ('grade', 'decision', 'votes', 'contrib'):
            assert same_bytes(pa[k], pw[k][j]) and same_bytes(pr[k][2 - j], pw[k][j]), (j, k)


def test_predicting_rows_together_equals_predicting_each_alone():
    import hvgan  # noqa: F401
    from hvgan import evaluation
    X, y, Xv = grid_tables()
    model = evaluation.svm_fit(X[:, 1], y)
    rng = np.random.default_rng(3)
    rows = np.resize(Xv[:, 1], (257, 3)) + rng.normal(0, 0.2, (257, 3))
    rows[100, 1] = np.nan
    singles = [evaluation.svm_predict(model, rows[k:k + 1], decisions=True, contributions=True) for k in range(257)]
    assert len({int(s['grade'][0]) for s in singles}) >= 3
    for n in (1, 63, 64, 65, 256, 257):
        out = evaluation.svm_predict(model, rows[:n], decisions=True, contributions=True)
        for k in ('grade', 'decision', 'votes', 'contrib'):
            assert same_bytes(out[k], np.concatenate([s[k] for s in singles[:n]])), (n, k)


# ---------------------------------------------------------------- 4. CAP dispatch edges
@functools.lru_cache(maxsize=None)
def two_class_table(rows):
    rng = np.random.default_rng(rows)
    y = (np.arange(rows + 40) % 2).astype(np.int64)
    X = rng.normal(0, 1.0, (rows + 40, 3)) + 1.2 * y[:, None]
    train = np.arange(rows + 40) < rows            # the last 40 rows only take part in the scaler
    return X, y, train


@pytest.mark.parametrize('rows', (256, 257, 512, 513, 1024, 1025))
def test_the_largest_pair_at_the_edges_of_the_lds_capacities(rows):
    import hvgan  # noqa: F401
    from hvgan import evaluation
    X, y, train = two_class_table(rows)
    d = evaluation.svm_fit(X, y, train=train, tol=1e-10)
    r = FR.fit(X, y, train)
    assert d['pair_rows'][0] == rows and d['status'][0] == evaluation.CONVERGED and d['gap'][0] <= 1e-10
    print(rows, 'largest |device - svm_fit_ref|', np.max(np.abs(d['w'] - r['w'])), np.max(np.abs(d['b'] - r['b'])), 'iterations', d['iterations'][0])
    assert close(d['mean'], r['mean'], 1e-12) and close(d['scale'], r['scale'], 1e-12)
    assert close(d['w'], r['w'], FR.SOLVER_TOL) and close(d['b'], r['b'], FR.SOLVER_TOL)
    out = evaluation.svm_predict(d, X[~train], decisions=True)
    assert close(out['decision'], FR.predict(r, X[~train])[1], FR.SOLVER_TOL)


def test_a_pair_beyond_the_lds_capacity_is_refused_before_any_launch():
    import hvgan  # noqa: F401
    from hvgan import evaluation
    with pytest.raises(ValueError, match='LDS'):
        evaluation.svm_fit(np.zeros((1793, 3)), np.arange(1793) % 2)


# ---------------------------------------------------------------- 5. status paths
def test_status_paths():
    import hvgan  # noqa: F401
    from hvgan import evaluation
    g = g22()
    X, y, Xh = g['c/X'], g['c/y'], g['c/X_held']
    one = evaluation.svm_fit(X, y, max_iter=1)
    assert np.all(one['status'] == evaluation.HIT_MAX_ITER) and np.all(one['iterations'] == 1) and np.all(one['gap'] > 1e-3) and not one['unusable']
    grade = evaluation.svm_predict(one, Xh)
    assert np.all(grade >= 0)
    # a class without train rows
    no3 = evaluation.svm_fit(X, y, train=y != 3)
    r = FR.fit(X, y, y != 3, tol=1e-3)
    assert list(no3['present']) == [True, True, True, False] and np.array_equal(no3['status'], r['status']) and (no3['status'] == evaluation.PAIR_ABSENT).sum() == 3
    assert np.isnan(no3['w'][[2, 4, 5]]).all() and np.isnan(no3['b'][[2, 4, 5]]).all() and np.all(no3['pair_rows'][[2, 4, 5]] == 0)
    out = evaluation.svm_predict(no3, Xh, decisions=True)
    assert out['grade'].max() == 2 and out['grade'].min() >= 0 and np.isnan(out['decision'][:, [2, 4, 5]]).all() and np.all(out['votes'][:, 3] == 0)
    assert np.all(out['votes'].sum(axis=1) == 3)
    # a NaN among one grid point's fit rows: that grid point alone is unusable, also for a row that does not train
    grid = np.stack([X, X * 1.5 + 0.1, X[:, ::-1]], axis=1)
    clean = evaluation.svm_fit(grid, y, train=np.arange(len(y)) > 0)
    dirty_feats = grid.copy()
    dirty_feats[0, 1, 2] = np.nan
    dirty = evaluation.svm_fit(dirty_feats, y, train=np.arange(len(y)) > 0)
    assert list(dirty['unusable']) == [False, True, False] and not clean['unusable'].any() and np.all(dirty['status'][1] == evaluation.UNUSABLE)
    for k in ('mean', 'scale', 'w', 'b'):
        assert np.isnan(dirty[k][1]).all(), k
    for k in FIT_KEYS:
        assert same_bytes(dirty[k][[0, 2]], clean[k][[0, 2]]), k
    held = np.stack([Xh, Xh * 1.5 + 0.1, Xh[:, ::-1]], axis=1)
    pc = evaluation.svm_predict(clean, held, decisions=True, contributions=True)
    pd = evaluation.svm_predict(dirty, held, decisions=True, contributions=True)
    assert np.all(pd['grade'][1] == -1) and np.isnan(pd['decision'][1]).all() and np.isnan(pd['contrib'][1]).all() and np.all(pd['votes'][1] == 0)
    for k in ('grade', 'decision', 'votes', 'contrib'):
        assert same_bytes(pd[k][[0, 2]], pc[k][[0, 2]]), k
    # a NaN or an inf in one predict row: that row of that grid point alone
    bad = held.copy()
    bad[5, 0, 1], bad[64, 2, 5] = np.nan, -np.inf
    pb = evaluation.svm_predict(clean, bad, decisions=True, contributions=True)
    hit = np.zeros((3, len(Xh)), dtype=bool)
    hit[0, 5] = hit[2, 64] = True
    assert np.all(pb['grade'][hit] == -1) and np.isnan(pb['decision'][hit]).all() and np.isnan(pb['contrib'][hit]).all() and np.all(pb['votes'][hit] == 0)
    for k in ('grade', 'decision', 'votes', 'contrib'):
        assert same_bytes(pb[k][~hit], pc[k][~hit]), k
    assert np.all(pc['grade'] >= 0)


# ---------------------------------------------------------------- 6. contributions
@pytest.mark.parametrize('case', ('a', 'c'))
def test_contributions_sum_to_the_decision_bit_for_bit(case):
    import hvgan  # noqa: F401
    from hvgan import evaluation
    g, d = g22(), device(case, 1e-3)
    out = evaluation.svm_predict(d, g[case + '/X_held'], decisions=True, contributions=True)
    c = out['contrib']
    total = np.zeros(c.shape[:-1])
    for col in range(c.shape[-1]):
        total = total + c[..., col]
    assert same_bytes(total - d['b'][None, :], out['decision'])
    xs = (g[case + '/X_held'] - d['mean']) / d['scale']
    assert same_bytes(c, d['w'][None] * xs[:, None, :])
    plain = evaluation.svm_predict(d, g[case + '/X_held'])
    assert same_bytes(plain, out['grade']) and same_bytes(evaluation.svm_predict(d, g[case + '/X_held'], contributions=True)['contrib'], c)
    # the votes are libsvm's vote of the decisions
    assert np.array_equal(R.vote(out['decision'], d['present']), np.searchsorted(d['classes'], out['grade']))
    assert np.all(out['votes'].sum(axis=1) == len(d['b']))


# ---------------------------------------------------------------- 7. guarded outputs, nullable outputs, refusals of the C entries
def _upload(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize('F,K,G,N', ((3, 3, 2, 257), (6, 4, 3, 65), (3, 2, 1, 1)))
def test_every_output_stays_inside_its_buffer(F, K, G, N):
    import hvgan  # noqa: F401
    import torch
    import hvtest as T
    from hvgan import lib
    L = lib.get()
    rng = np.random.default_rng(F * 100 + K)
    M, P = 45, K * (K - 1) // 2
    y = (np.arange(M) % K).astype(np.int32)
    X = rng.normal(0, 1, (G, M, F)) + 0.8 * y[None, :, None]
    Xn = rng.normal(0, 1, (G, N, F)) + 0.8
    cl = np.arange(K, dtype=np.int32)
    plan = np.zeros(L.size('hv_svm_fit_plan_bytes', M), np.uint8)
    rows = ctypes.c_int(0)
    assert L.cdll.hv_svm_fit_plan(y.ctypes.data, None, M, cl.ctypes.data, K, plan.ctypes.data, ctypes.c_size_t(plan.nbytes), ctypes.byref(rows)) == 0
    dx, dplan, dxn = _upload(X), _upload(plan), _upload(Xn)
    present = _upload(plan[64:64 + 16].view(np.int32)[:K].copy())
    f64, i32 = torch.float64, torch.int32
    fit = {'mean': T.Guarded((G, F), f64), 'scale': T.Guarded((G, F), f64), 'w': T.Guarded((G, P, F), f64, offset=1), 'b': T.Guarded((G, P), f64),
           'gap': T.Guarded((G, P), f64), 'info': T.Guarded((G, P, 4), i32, offset=2)}
    L.call('hv_svm_fit', lib.ptr(dx), lib.ptr(dplan), G, M, F, K, rows.value, ctypes.c_double(1e-3), 100000, *(lib.ptr(fit[k].t) for k in fit), lib.stream())
    torch.cuda.synchronize()
    assert all(v.intact() for v in fit.values())
    assert not torch.isnan(fit['w'].t).any() and bool((fit['info'].t[..., 1] == 0).all())

    def predict(decision, votes, contrib):
        out = {'pred': T.Guarded((G, N), i32, offset=1), 'decision': T.Guarded((G, N, P), f64) if decision else None,
               'votes': T.Guarded((G, N, K), i32, offset=3) if votes else None, 'contrib': T.Guarded((G, N, P, F), f64, offset=1) if contrib else None}
        L.call('hv_svm_predict', lib.ptr(dxn), G, N, F, K, lib.ptr(present), *(lib.ptr(fit[k].t) for k in ('mean', 'scale', 'w', 'b', 'info')),
               *(lib.ptr(out[k].t) if out[k] is not None else None for k in ('pred', 'decision', 'votes', 'contrib')), lib.stream())
        torch.cuda.synchronize()
        assert all(v.intact() for v in out.values() if v is not None)
        return out
    full = predict(True, True, True)
    assert bool((full['pred'].t >= 0).all()) and not torch.isnan(full['decision'].t).any() and not torch.isnan(full['contrib'].t).any()
    for flags in ((False, False, False), (True, False, False), (False, True, False), (False, False, True)):
        part = predict(*flags)
        assert torch.equal(part['pred'].t, full['pred'].t)
        for k in ('decision', 'votes', 'contrib'):
            assert part[k] is None or torch.equal(part[k].t, full[k].t)
    # the features kernel
    rec = _upload(rng.normal(0, 1, (N, 2, 16)))
    for FF in (3, 6):
        feats = T.Guarded((N, FF), f64, offset=1)
        L.call('hv_svm_features', lib.ptr(rec), N, 1, FF, lib.ptr(feats.t), lib.stream())
        torch.cuda.synchronize()
        assert feats.intact()


def test_the_c_entries_refuse_before_any_launch():
    import hvgan  # noqa: F401
    import torch
    from hvgan import lib
    L = lib.get()
    poison = torch.full((4096,), -7.5, dtype=torch.float64).cuda()
    x = torch.zeros(4096, dtype=torch.float64).cuda()
    p, q = lib.ptr(poison), lib.ptr(x)

    def fit(F=3, K=3, rows=30, G=1, M=37, max_iter=10, tol=1e-3, X=q, plan=q, outs=(p,) * 6):
        return L.cdll.hv_svm_fit(X, plan, G, M, F, K, rows, ctypes.c_double(tol), max_iter, *outs, lib.stream())

    def predict(F=3, K=3, G=1, N=20, X=q, present=q, model=(q,) * 5, pred=p):
        return L.cdll.hv_svm_predict(X, G, N, F, K, present, *model, pred, p, p, p, lib.stream())

    def features(N=20, first=0, F=6, rec=q, out=p):
        return L.cdll.hv_svm_features(rec, N, first, F, out, lib.stream())
    assert fit(F=4) == -2 and fit(F=0) == -2 and fit(K=5) == -2 and fit(K=1) == -2 and fit(rows=1793) == -2 and fit(G=65536) == -2
    assert fit(max_iter=0) == -1 and fit(tol=0.0) == -1 and fit(tol=float('nan')) == -1 and fit(G=0) == -1 and fit(M=0) == -1
    assert fit(X=None) == -1 and fit(plan=None) == -1
    for k in range(6):
        assert fit(outs=(p,) * k + (None,) + (p,) * (5 - k)) == -1
    assert predict(F=5) == -2 and predict(K=5) == -2 and predict(K=1) == -2 and predict(G=65536) == -2
    assert predict(N=0) == -1 and predict(N=-3) == -1 and predict(G=0) == -1 and predict(X=None) == -1 and predict(present=None) == -1 and predict(pred=None) == -1
    for k in range(5):
        assert predict(model=(q,) * k + (None,) + (q,) * (4 - k)) == -1
    assert features(F=4) == -2 and features(N=0) == -1 and features(first=2) == -1 and features(first=-1) == -1 and features(rec=None) == -1
    assert features(out=None) == -1
    torch.cuda.synchronize()
    assert torch.all(poison == -7.5)
    # a plan that does not belong to the sizes (zeros here) is reported per problem, nothing is solved
    out = torch.zeros(64, dtype=torch.int32).cuda()
    assert fit(outs=(p, p, p, p, p, lib.ptr(out))) == 0
    torch.cuda.synchronize()
    assert np.all(out[:12].cpu().numpy().reshape(3, 4)[:, 1] == 4)


# ---------------------------------------------------------------- 8. the features kernel
def host_features(rec, file1, F):
    """evaluation.svm_features (its first three columns for F = 3) with svm_feature_grid's NaN rules."""
    from hvgan import evaluation
    feats = evaluation.svm_features(rec, file1)[:, :F].copy()
    feats[(rec[:, 0, 13] == 0) | (rec[:, 1, 14] != 0)] = np.nan
    return feats


def test_features_kernel_is_svm_features_with_the_nan_rules():
    import hvgan  # noqa: F401
    import torch
    from hvgan import lib
    L = lib.get()
    rng = np.random.default_rng(8)
    for n in (1, 255, 256, 257):
        rec = rng.normal(0, 1, (n, 2, 16))
        rec[:, :, 13:] = 0.0
        rec[:, 0, 13] = rng.random(n) > 0.2           # the original has the vertebra
        rec[:, 1, 13] = rec[:, 0, 13]
        rec[:, 1, 14] = rng.random(n) > 0.8           # the coronal script would have raised
        rec[:, 0, 14] = 0.0
        if n > 1:
            rec[0, :, 13], rec[0, 1, 14] = 0.0, 0.0
            rec[1, :, 13], rec[1, 1, 14] = 1.0, 1.0
            rec[2, :, 13], rec[2, 1, 14] = 1.0, 0.0
        d = _upload(rec)
        for file1, first in (('sagittal', 0), ('coronal', 1)):
            for F in (3, 6):
                out = torch.full((n, F), 7.0, dtype=torch.float64).cuda()
                L.call('hv_svm_features', lib.ptr(d), n, first, F, lib.ptr(out), lib.stream())
                want = host_features(rec, file1, F)
                assert same_bytes(out.cpu().numpy(), want), (n, file1, F)
                if n > 1:
                    assert np.isnan(want[:2]).all() and not np.isnan(want[2]).any()


# ---------------------------------------------------------------- 9. from resident volumes to grades with one readback
class _CountedCpu:
    """Counts Tensor.cpu() calls: every readback of these entry points is one."""
    def __enter__(self):
        import torch
        self.n, self.orig = 0, torch.Tensor.cpu

        def cpu(t, *a, **kw):
            self.n += 1
            return self.orig(t, *a, **kw)
        torch.Tensor.cpu = cpu
        return self

    def __exit__(self, *exc):
        import torch
        torch.Tensor.cpu = self.orig


@pytest.mark.parametrize('file1', ('sagittal', 'coronal'))
def test_grade_dataset_is_the_host_chain_bit_for_bit(file1):
    import hvgan  # noqa: F401
    import torch
    from hvgan import evaluation
    import rhlv_sweep_cases as S
    (H, W, Z), _ = S.SHAPES[0]
    pairs = [S.random_pair(60 + k, H, W, Z) for k in range(6)]
    narrow = np.zeros((H, W, Z), dtype=np.uint8)       # two columns along z: the coronal view's thirds are empty
    narrow[:5, 5:30, 10:12] = S.IDX
    pairs[4] = (narrow, narrow.copy())
    fakes = [torch.from_numpy(f).cuda() for f, _ in pairs]
    labels = [torch.from_numpy(l).cuda() for _, l in pairs]
    ids = [S.IDX, S.IDX, S.IDX + 9, S.IDX, S.IDX, S.IDX]           # pair 2: the original lacks that vertebra
    setting = (2, 0.64)
    rec, present = evaluation.rhlv_dataset(fakes, labels, ids, *setting)
    feats = host_features(rec, file1, 6)
    print('present', present, 'raised', rec[:, 1, 14], 'features', feats)
    # a grader fitted on rows around the features these pairs have (made-up grades: the chain is what is tested)
    usable = feats[~np.isnan(feats).any(axis=1)]
    assert len(usable) >= 3
    rng = np.random.default_rng(9)
    table = np.concatenate([usable + rng.normal(0, 0.05, usable.shape) for _ in range(8)])
    grades = (table[:, 0] + table[:, 4] > np.median(table[:, 0] + table[:, 4])).astype(np.int64) + (table[:, 1] > np.median(table[:, 1]))
    grader = evaluation.Grader(setting, evaluation.svm_fit(table, grades), file1)
    want = evaluation.svm_predict(grader.model, feats, decisions=True, contributions=True)
    for chunk in (256, 1, 4):
        with _CountedCpu() as c:
            got = grader.grade_dataset(fakes, labels, ids, chunk=chunk, contributions=True)
        assert c.n == 1
        assert same_bytes(got['records'], rec) and np.array_equal(got['present'], present) and np.array_equal(got['raised'], rec[:, 1, 14] != 0)
        assert same_bytes(got['features'], feats)
        for k in ('grade', 'decision', 'votes', 'contrib'):
            assert same_bytes(got[k], want[k]), (chunk, k)
        assert 'contrib' not in grader.grade_dataset(fakes, labels, ids, chunk=chunk)
    assert present[4] and got['raised'][4] and got['grade'][4] == -1 and got['raised'].sum() == 1          # the narrow pair: flagged, not raised
    assert not present[2] and got['grade'][2] == -1 and np.all(got['grade'][~np.isnan(feats).any(axis=1)] >= 0)
    assert np.array_equal(got['grade'] == -1, np.isnan(feats).any(axis=1))
    assert same_bytes(grader.predict(feats), want['grade'])
    again = evaluation.Grader.from_state_dict(grader.state_dict())
    assert same_bytes(again.grade_dataset(fakes, labels, ids)['grade'], got['grade'])


def test_fit_grader_fits_the_best_setting_on_the_train_and_test_rows():
    import hvgan  # noqa: F401
    from hvgan import evaluation
    g = g19()
    # a made-up sweep whose records carry G19's case f features (sagittal columns; the coronal columns a scaled copy)
    feats = g['f/features'].copy()
    feats[~np.isfinite(feats)] = 0.25
    N, D, T = feats.shape[:3]
    rec = np.zeros((N, D, T, 2, 16))
    rec[..., 0, 1:4], rec[..., 1, 1:4], rec[..., 13] = feats, feats * 0.5 + 0.1, 1.0
    sweep = {'records': rec, 'length_divisors': np.array([4, 5]), 'height_thresholds': np.array([0.6, 0.64, 0.7]), 'views': ('sagittal', 'coronal'),
             'raised': np.zeros((N, D), bool)}
    labels, dataset = g['f/labels'], g['f/dataset']
    six = evaluation.svm_feature_grid(sweep)
    grades = evaluation.svm_grade_grid(six, labels, dataset)
    best = evaluation.best_setting(sweep, grades)
    gr = evaluation.fit_grader(sweep, labels, dataset)
    assert gr.setting == best and gr.file1 == 'sagittal' and np.array_equal(gr.classes, np.unique(labels))
    d, t = list(sweep['length_divisors']).index(best[0]), list(sweep['height_thresholds']).index(best[1])
    tt = dataset != 'val'
    direct = evaluation.svm_fit(six[tt, d, t], labels[tt])
    for k in FIT_KEYS:
        assert same_bytes(gr.model[k], direct[k]), k
    given = evaluation.fit_grader(sweep, labels, dataset, grades=grades, score='accuracy', setting=(5, 0.7), file1='coronal')
    swapped = evaluation.svm_fit(six[tt, 1, 2][:, [3, 4, 5, 0, 1, 2]], labels[tt])
    assert given.setting == (5, 0.7) and same_bytes(given.model['w'], swapped['w'])
    # the val rows were not touched: changing them changes nothing
    rec2 = rec.copy()
    rec2[~tt, ..., 1:4] += 3.0
    other = evaluation.fit_grader(dict(sweep, records=rec2), labels, dataset, setting=best)
    assert same_bytes(other.model['w'], gr.model['w']) and same_bytes(other.model['mean'], gr.model['mean'])
    assert same_bytes(gr.predict(six[~tt, d, t]), evaluation.svm_predict(direct, six[~tt, d, t]))
