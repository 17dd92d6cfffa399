"""The grading chain's numpy restatement (tests/svm_ref.py) against fixture G19 -- the reference's own evaluate_svm of evaluation/SVM_grading.py
and SVM_grading_2.5d.py, and scikit-learn's SVC at tol=1e-10 on the same folds, recorded by tools/make_golden_svm_grading.py -- and the
package's host-side pieces (stratified_folds, the plan hv_svm_grade_plan computes).  No GPU and no scikit-learn here."""
import ctypes
import functools
import os

import numpy as np
import pytest

import svm_ref as R
from conftest import GOLDEN


@functools.lru_cache(maxsize=None)
def g19():
    return dict(np.load(os.path.join(GOLDEN, 'g19_svm_grading.npz')))


@functools.lru_cache(maxsize=None)
def graded(case):
    g = g19()
    return R.grade(g[case + '/X_tt'], g[case + '/y_tt'], g[case + '/X_val'], g[case + '/y_val'])


def close(a, b, tol):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.all(np.abs(a - b)[~np.isnan(a)] <= tol)


@pytest.mark.parametrize('case', R.CASES)
def test_folds_scaler_and_bounds_are_the_references(case):
    import hvgan  # noqa: F401
    from hvgan import evaluation
    g, r = g19(), graded(case)
    assert np.array_equal(r['folds'], g[case + '/folds'])
    assert np.array_equal(evaluation.stratified_folds(g[case + '/y_tt']), g[case + '/folds'])
    assert close(r['mean'], g[case + '/mean'], 1e-12) and close(r['scale'], g[case + '/scale'], 1e-12)
    assert close(r['bounds'], g[case + '/bounds'], 1e-12)
    if case == 'b':
        assert r['scale'][4] == 1.0 and g['b/scale'][4] == 1.0           # the constant column


@pytest.mark.parametrize('case', R.CASES)
def test_restatement_solves_what_svc_solves(case):
    g, r = g19(), graded(case)
    assert np.all((r['status'] == R.CONVERGED) | (r['status'] == R.ABSENT)) and np.nanmax(r['gap']) <= 1e-12
    worst = max(np.nanmax(np.abs(r['w'] - g[case + '/tight_coef'])), np.nanmax(np.abs(r['b'] - g[case + '/tight_b'])),
                np.nanmax(np.abs(r['decision'] - g[case + '/tight_dec'])))
    print(case, 'largest |svm_ref - SVC(tol=1e-10)|', worst)
    assert close(r['w'], g[case + '/tight_coef'], R.SOLVER_TOL) and close(r['b'], g[case + '/tight_b'], R.SOLVER_TOL)
    assert close(r['decision'], g[case + '/tight_dec'], R.SOLVER_TOL)
    if case == 'e':
        assert (r['status'] == R.ABSENT).any() and not r['present'].all()


@pytest.mark.parametrize('case', R.CASES)
def test_restatement_grades_as_the_reference_scripts_do(case):
    g, r = g19(), graded(case)
    pred = r['classes'][r['pred']]
    far = ~g[case + '/near']
    if case != 'c':
        assert far.all()
    assert (~far).mean() <= 0.05
    assert np.array_equal(pred[far], g[case + '/pred'][far])
    # the metrics, applied to the reference's own predictions, are the reference's numbers
    true_idx = np.searchsorted(r['classes'], g[case + '/y_val'])
    for f in range(5):
        cm = R.confusion(true_idx, np.searchsorted(r['classes'], g[case + '/pred'][f]), len(r['classes']))
        assert np.array_equal(cm, g[case + '/confusion'][f])
        assert close(R.scores(cm), g[case + '/scores'][f], 1e-12)
    m, v = R.mean_var(g[case + '/scores'])
    assert close(m, g[case + '/mean_scores'], 1e-12) and close(v, g[case + '/var_scores'], 1e-12)
    if far.all():
        assert np.array_equal(r['confusion'], g[case + '/confusion']) and close(r['scores'], g[case + '/scores'], 1e-12)


def test_plan_refuses_bad_arguments_on_the_host():
    import hvgan  # noqa: F401
    from hvgan import evaluation, lib
    L = lib.get()
    g = g19()
    y, yv, fo = g['e/y_tt'].astype(np.int32), g['e/y_val'].astype(np.int32), g['e/folds'].astype(np.int32)
    cl = np.unique(np.concatenate([y, yv])).astype(np.int32)

    def plan(y=y, fo=fo, yv=yv, cl=cl, short=0):
        buf = np.zeros(L.size('hv_svm_grade_plan_bytes', len(y), len(yv)) - short, np.uint8)
        rows = ctypes.c_int(-1)
        rc = L.cdll.hv_svm_grade_plan(y.ctypes.data, fo.ctypes.data, len(y), yv.ctypes.data, len(yv), cl.ctypes.data, len(cl), buf.ctypes.data,
                                      ctypes.c_size_t(buf.nbytes), ctypes.byref(rows))
        return rc, rows.value, buf
    rc, rows, buf = plan()
    assert rc == 0 and rows == max(np.isin(y[fo != f], pair).sum() for f in range(5) for pair in ((0, 1), (0, 2), (1, 2))
                                   if all((y[fo != f] == c).any() for c in pair))
    bounds = buf[:160].view(np.float64).reshape(5, 4)[:, :3]
    assert close(np.where(bounds == 0, np.nan, bounds), g['e/bounds'], 1e-12)       # 0 = the class is absent from that fold's training rows
    bad = fo.copy()
    bad[3] = 5
    assert plan(fo=bad)[0] == -1 and plan(cl=cl[::-1].copy())[0] == -1 and plan(cl=cl[:2].copy())[0] == -1       # a grade not in classes
    assert plan(cl=np.arange(5, dtype=np.int32))[0] == -2 and plan(short=8)[0] == -3
    big = np.arange(4000, dtype=np.int32) % 2
    rc, rows, _ = plan(y=big, fo=(np.arange(4000, dtype=np.int32) // 2) % 5, cl=np.arange(2, dtype=np.int32), yv=big[:10].copy())
    assert rc == -2 and rows == 3200 and rows > evaluation.MAX_PAIR_ROWS
