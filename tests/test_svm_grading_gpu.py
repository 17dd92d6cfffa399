"""SVM grading of every grid point on the device (hv_svm_grade_grid through hvgan.evaluation.svm_grade_grid) against the numpy restatement
(tests/svm_ref.py, run to a 1e-12 KKT gap) and against what the reference's own evaluate_svm produced (fixture G19,
tools/make_golden_svm_grading.py).  Solver tolerance: svm_ref.SOLVER_TOL, ten times the measured difference between the restatement and
scikit-learn's SVC at tol=1e-10."""
import functools
import os

import numpy as np
import pytest

import svm_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DATASET = {True: 'val', False: ('train', 'test')}


@functools.lru_cache(maxsize=None)
def g19():
    return dict(np.load(os.path.join(GOLDEN, 'g19_svm_grading.npz')))


@functools.lru_cache(maxsize=None)
def ref(case):
    g = g19()
    return R.grade(g[case + '/X_tt'], g[case + '/y_tt'], g[case + '/X_val'], g[case + '/y_val'])


def table(case):
    """-> (features [N, 1, F], labels, dataset) with the train + test rows first."""
    g = g19()
    X, Xv = g[case + '/X_tt'], g[case + '/X_val']
    feats = np.concatenate([X, Xv])[:, None, :]
    labels = np.concatenate([g[case + '/y_tt'], g[case + '/y_val']])
    dataset = np.array([('train', 'test')[i % 2] for i in range(len(X))] + ['val'] * len(Xv))
    return feats, labels, dataset


@functools.lru_cache(maxsize=None)
def device(case, tol):
    from hvgan import evaluation
    return evaluation.svm_grade_grid(*table(case), tol=tol, decisions=True)


def close(a, b, tol):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.all(np.abs(a - b)[~np.isnan(a)] <= tol)


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize('case', R.CASES)
def test_tight_solve_matches_the_restatement(case):
    import hvgan  # noqa: F401
    d, r = device(case, 1e-10), ref(case)
    assert np.array_equal(d['classes'], r['classes']) and np.array_equal(d['folds'], r['folds']) and not d['unusable'].any()
    assert np.array_equal(d['status'][0], r['status'])
    solved = r['status'] != R.ABSENT
    assert np.all(d['status'][0][solved] == R.CONVERGED) and np.all(d['gap'][0][solved] <= 1e-10)
    for k in ('w', 'b', 'decision'):
        print(case, k, 'largest |device - svm_ref|', np.nanmax(np.abs(d[k][0] - r[k])))
    assert close(d['w'][0], r['w'], R.SOLVER_TOL) and close(d['b'][0], r['b'], R.SOLVER_TOL)
    assert close(d['decision'][0], r['decision'], R.SOLVER_TOL)
    assert np.all(d['support'][0][solved] > 0) and np.all(d['iterations'][0][solved] > 0)


@pytest.mark.parametrize('case', R.CASES)
def test_default_tolerance_gives_the_reference_scripts_answer(case):
    import hvgan  # noqa: F401
    g, d = g19(), device(case, 1e-3)
    solved = d['status'][0] != R.ABSENT
    assert np.all(d['status'][0][solved] == R.CONVERGED) and np.all(d['gap'][0][solved] <= 1e-3)
    far = ~g[case + '/near']
    assert (~far).mean() <= 0.05
    assert np.array_equal(d['pred'][0][far], g[case + '/pred'][far])
    if case != 'c':                     # seeds picked so that no val row lies within delta of a boundary: everything is the reference's
        assert far.all()
        assert np.array_equal(d['confusion'][0], g[case + '/confusion'])
        assert close(d['scores'][0], g[case + '/scores'], 1e-12)
        assert close(d['mean'][0], g[case + '/mean_scores'], 1e-12) and close(d['var'][0], g[case + '/var_scores'], 1e-12)


@pytest.mark.parametrize('case', R.CASES)
@pytest.mark.parametrize('tol', (1e-3, 1e-10))
def test_metrics_of_the_devices_own_predictions(case, tol):
    import hvgan  # noqa: F401
    g, d = g19(), device(case, tol)
    K = len(d['classes'])
    true_idx = np.searchsorted(d['classes'], g[case + '/y_val'])
    sc = np.zeros((5, 4))
    for f in range(5):
        cm = R.confusion(true_idx, np.searchsorted(d['classes'], d['pred'][0, f]), K)
        assert np.array_equal(d['confusion'][0, f], cm)
        sc[f] = R.scores(cm)
        # the device's vote on its own decisions
        assert np.array_equal(R.vote(d['decision'][0, f], ref(case)['present'][f]), np.searchsorted(d['classes'], d['pred'][0, f]))
    assert close(d['scores'][0], sc, 1e-12)
    m, v = R.mean_var(sc)
    assert close(d['mean'][0], m, 1e-12) and close(d['var'][0], v, 1e-12)
    if case == 'e':                     # the single-member class is never predicted in the fold that tests it: its precision term is 0
        assert (d['status'][0] == R.ABSENT).any() and (d['confusion'][0].sum(axis=1)[:, 2] == 0).any()


KEYS = ('confusion', 'scores', 'mean', 'var', 'pred', 'w', 'b', 'gap', 'iterations', 'status', 'support', 'unusable', 'decision')


@functools.lru_cache(maxsize=None)
def grid_f():
    from hvgan import evaluation
    g = g19()
    return evaluation.svm_grade_grid(g['f/features'], g['f/labels'], g['f/dataset'], decisions=True)


def test_a_grid_point_has_the_same_bytes_alone_in_the_grid_and_in_the_reversed_grid():
    import hvgan  # noqa: F401
    from hvgan import evaluation
    g, whole = g19(), grid_f()
    feats = g['f/features']
    assert whole['mean'].shape == (2, 3, 4) and whole['pred'].shape == (2, 3, 5, 20) and whole['w'].shape == (2, 3, 5, 3, 3)
    rev = evaluation.svm_grade_grid(feats[:, ::-1, ::-1], g['f/labels'], g['f/dataset'], decisions=True)
    for i in range(2):
        for j in range(3):
            alone = evaluation.svm_grade_grid(feats[:, i, j], g['f/labels'], g['f/dataset'], decisions=True)
            for k in KEYS:
                assert same_bytes(alone[k], whole[k][i, j]), (i, j, k)
                assert same_bytes(rev[k][1 - i, 2 - j], whole[k][i, j]), (i, j, k)


def test_a_grid_point_with_an_inf_is_unusable_and_leaves_its_neighbours_alone():
    import hvgan  # noqa: F401
    from hvgan import evaluation
    g, whole = g19(), grid_f()
    assert np.array_equal(whole['unusable'], g['f/unusable']) and whole['unusable'][1, 0]
    assert np.isnan(whole['scores'][1, 0]).all() and np.isnan(whole['mean'][1, 0]).all() and np.isnan(whole['var'][1, 0]).all()
    assert np.all(whole['pred'][1, 0] == -1) and np.all(whole['confusion'][1, 0] == 0) and np.all(whole['status'][1, 0] == evaluation.UNUSABLE)
    ok = ~whole['unusable']
    assert not np.isnan(whole['scores'][ok]).any() and np.all(whole['status'][ok] == evaluation.CONVERGED)
    # the same grid with the inf replaced: every other grid point keeps its bytes
    feats = g['f/features'].copy()
    feats[~np.isfinite(feats)] = 0.25
    clean = evaluation.svm_grade_grid(feats, g['f/labels'], g['f/dataset'], decisions=True)
    assert not clean['unusable'].any()
    for k in KEYS:
        assert same_bytes(clean[k][ok], whole[k][ok]), k
    # rows that are NaN at every grid point (vertebra absent) are dropped on the host
    more = np.concatenate([feats, np.full((2,) + feats.shape[1:], np.nan)])
    padded = evaluation.svm_grade_grid(more, np.concatenate([g['f/labels'], [1, 2]]), np.concatenate([g['f/dataset'], ['train', 'val']]), decisions=True)
    for k in KEYS:
        assert same_bytes(padded[k], clean[k]), k


def test_max_iter_is_reported_and_best_setting_skips_such_points():
    import hvgan  # noqa: F401
    from hvgan import evaluation
    g = g19()
    d = evaluation.svm_grade_grid(g['f/features'], g['f/labels'], g['f/dataset'], max_iter=1)
    ok = ~d['unusable']
    assert np.all(d['status'][ok] == evaluation.HIT_MAX_ITER) and np.all(d['iterations'][ok] == 1) and np.all(d['gap'][ok] > 1e-3)
    sweep = {'length_divisors': np.array([4, 5]), 'height_thresholds': np.array([0.6, 0.64, 0.7])}
    with pytest.raises(ValueError):
        evaluation.best_setting(sweep, d)
    # one point of the grid converged: it is the only candidate, whatever its score
    full = grid_f()
    mixed = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in d.items()}
    mixed['status'][0, 2] = full['status'][0, 2]
    mixed['mean'][0, 2] = 0.0
    assert evaluation.best_setting(sweep, mixed) == (4, 0.7)
    best = evaluation.best_setting(sweep, full, 'accuracy')
    m = np.where(full['unusable'], -np.inf, full['mean'][..., 3])
    i, j = np.unravel_index(np.argmax(m), m.shape)
    assert best == (int(sweep['length_divisors'][i]), float(sweep['height_thresholds'][j]))


def test_refusals_come_before_any_launch():
    import hvgan  # noqa: F401
    import torch
    from hvgan import evaluation, lib
    feats, labels, dataset = table('a')
    with pytest.raises(ValueError):
        evaluation.svm_grade_grid(np.concatenate([feats, feats[..., :1]], axis=-1), labels, dataset)          # F = 4
    with pytest.raises(ValueError):
        evaluation.svm_grade_grid(feats, np.arange(len(labels)) % 5, dataset)                                  # K = 5
    with pytest.raises(ValueError):
        evaluation.svm_grade_grid(feats, labels, dataset, folds=np.full(37, 5))                                # fold id 5
    n = 4000                                                                                                   # 3200 training rows of one pair
    with pytest.raises(ValueError, match='LDS'):
        evaluation.svm_grade_grid(np.zeros((n + 10, 1, 3)), np.arange(n + 10) % 2, np.array(['train'] * n + ['val'] * 10),
                                  folds=(np.arange(n) // 2) % 5)
    # the C entry itself: nothing is written where it refuses
    L = lib.get()
    poison = torch.full((4096,), -7.5, dtype=torch.float64).cuda()
    x = torch.zeros(4096, dtype=torch.float64).cuda()
    p = lib.ptr(poison)

    def call(F=3, K=3, rows=30, G=1, max_iter=10):
        import ctypes
        rc = L.cdll.hv_svm_grade_grid(lib.ptr(x), lib.ptr(x), lib.ptr(x), G, 37, 20, F, K, rows, ctypes.c_double(1e-3), max_iter, p, p, p, p, p, p, p, p, p, p,
                                      None, lib.stream())
        torch.cuda.synchronize()
        return rc
    assert call(F=4) == -2 and call(K=5) == -2 and call(K=1) == -2 and call(rows=1793) == -2 and call(G=65536) == -2 and call(max_iter=0) == -1
    assert torch.all(poison == -7.5)
    # a plan that does not belong to the sizes (zeros here) is reported per problem, nothing is solved
    out = torch.zeros(4096, dtype=torch.int32).cuda()
    import ctypes
    assert L.cdll.hv_svm_grade_grid(lib.ptr(x), lib.ptr(x), lib.ptr(x), 1, 37, 20, 3, 3, 30, ctypes.c_double(1e-3), 10, p, p, p, lib.ptr(out), lib.ptr(out[1024:]),
                                    lib.ptr(out[2048:]), p, p, p, lib.ptr(out[3072:]), None, lib.stream()) == 0
    torch.cuda.synchronize()
    assert np.all(out[:60].cpu().numpy().reshape(15, 4)[:, 1] == evaluation.BAD_PLAN)


def test_sweep_to_best_setting_end_to_end():
    import hvgan  # noqa: F401
    import torch
    from hvgan import evaluation
    import rhlv_sweep_cases as S
    g, names = S.g18()
    names = [n for n in names if not g[n + '/absent']]
    shapes = {}
    for n in names:
        shapes.setdefault(g[n + '/fake'].shape, []).append(n)
    divs, thrs = [int(d) for d in g['divisors']], [float(t) for t in g['thresholds']]
    feats = []
    for group in shapes.values():
        sweep = evaluation.rhlv_sweep([torch.from_numpy(g[n + '/fake']).cuda() for n in group], [torch.from_numpy(g[n + '/label']).cuda() for n in group],
                                      [int(g[n + '/index']) for n in group], divs, thrs)
        feats.append(evaluation.svm_feature_grid(sweep))
    feats = np.concatenate(feats)
    n = len(feats)                                 # five made-up rows per pair: enough members of both grades for five folds and a val set
    feats = np.concatenate([feats * (1 + 0.01 * k) + 0.003 * k for k in range(5)])
    labels = np.concatenate([np.arange(n) % 2] * 5)
    dataset = np.array((['train'] * n + ['test'] * n) * 2 + ['val'] * n)
    grades = evaluation.svm_grade_grid(feats, labels, dataset)
    assert grades['mean'].shape == (len(divs), len(thrs), 4) and grades['unusable'].shape == (len(divs), len(thrs))
    if (~grades['unusable']).any():
        best = evaluation.best_setting(sweep, grades)
        assert best[0] in divs and best[1] in thrs
