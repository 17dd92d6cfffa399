"""The fit / predict restatement (tests/svm_fit_ref.py) against fixture G22 -- scikit-learn's StandardScaler + SVC(kernel='linear',
class_weight='balanced') fitted on all train + test rows at tol=1e-3 and tol=1e-10 with predictions and decisions of held-out rows, recorded by
tools/make_golden_svm_fit.py -- and the package's host-side pieces: the plan hv_svm_fit_plan computes, the Grader's state and the refusals of the
Python entries.  No GPU and no scikit-learn here."""
import ctypes
import functools
import io

import numpy as np
import pytest

import svm_fit_ref as FR
import svm_ref as R
from conftest import GOLDEN

CAP = 0.01            # at most 1 % of a case's held-out rows may lie within delta of a boundary


@functools.lru_cache(maxsize=None)
def g22():
    return FR.g22(GOLDEN)


@functools.lru_cache(maxsize=None)
def fitted(case):
    g = g22()
    return FR.fit(g[case + '/X'], g[case + '/y'])


def close(a, b, tol):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.all(np.abs(a - b)[~np.isnan(a)] <= tol)


def test_the_solver_tolerance_is_the_measured_one():
    # ten times the larger of the two measured differences between the restatement and scikit-learn's SVC at tol=1e-10 (G19: 2.07e-6)
    assert float(g22()['solver_gap']) <= R.SOLVER_TOL / 10 and FR.SOLVER_TOL == R.SOLVER_TOL


@pytest.mark.parametrize('case', FR.CASES)
def test_restatement_fits_what_scikit_learn_fits(case):
    g, r = g22(), fitted(case)
    assert close(r['mean'], g[case + '/mean'], 1e-12) and close(r['scale'], g[case + '/scale'], 1e-12)
    assert close(r['bounds'], g[case + '/bounds'], 1e-12)
    assert np.all(r['status'] == R.CONVERGED) and np.max(r['gap']) <= 1e-12 and r['present'].all()
    pred, dec = FR.predict(r, g[case + '/X_held'])
    worst = max(np.max(np.abs(r['w'] - g[case + '/tight_coef'])), np.max(np.abs(r['b'] - g[case + '/tight_b'])), np.max(np.abs(dec - g[case + '/tight_dec'])))
    print(case, 'largest |svm_fit_ref - SVC(tol=1e-10)|', worst)
    assert close(r['w'], g[case + '/tight_coef'], FR.SOLVER_TOL) and close(r['b'], g[case + '/tight_b'], FR.SOLVER_TOL)
    assert close(dec, g[case + '/tight_dec'], FR.SOLVER_TOL)
    assert np.array_equal(FR.contrib(r, g[case + '/X_held']).shape, (len(pred),) + r['w'].shape)
    if case == 'e':
        assert r['scale'][4] == 1.0 and g['e/scale'][4] == 1.0          # the constant column


@pytest.mark.parametrize('case', FR.CASES)
def test_restatement_grades_held_out_rows_as_scikit_learn_does(case):
    g = g22()
    r = FR.fit(g[case + '/X'], g[case + '/y'], tol=1e-3)
    pred, dec = FR.predict(r, g[case + '/X_held'])
    far = ~g[case + '/near']
    assert (~far).mean() <= CAP
    # the fixture's own delta: a decision at least delta from 0 keeps its sign between the two tolerances
    assert np.array_equal(far, ~(np.abs(g[case + '/tight_dec']).min(axis=1) < g[case + '/delta']))
    assert np.array_equal(r['classes'][pred][far], g[case + '/pred'][far])
    assert np.array_equal(r['classes'][R.vote(dec, r['present'])], r['classes'][pred])


def test_fit_on_a_subset_scales_with_every_row_and_solves_the_subset():
    g = g22()
    X, y = g['c/X'], g['c/y']
    train = np.arange(len(y)) % 3 != 0
    r = FR.fit(X, y, train)
    whole = FR.fit(X, y)
    assert np.array_equal(r['mean'], whole['mean']) and np.array_equal(r['scale'], whole['scale'])
    cls, bnd = R.balanced_bounds(y[train])
    assert np.array_equal(r['bounds'], bnd) and np.array_equal(r['pair_rows'], [np.isin(y[train], (cls[a], cls[b])).sum() for a, b in R.pairs(4)])
    # a class without train rows: its pairs are absent and it is never predicted
    no3 = FR.fit(X, y, y != 3)
    assert list(no3['present']) == [True, True, True, False] and list(no3['status']) == [0, 0, R.ABSENT, 0, R.ABSENT, R.ABSENT]
    pred, dec = FR.predict(no3, g['c/X_held'])
    assert pred.max() == 2 and np.isnan(dec[:, [2, 4, 5]]).all()
    bad = g['c/X_held'][:4].copy()
    bad[1, 2], bad[3, 0] = np.nan, np.inf
    pred, dec = FR.predict(whole, bad)
    assert list(pred >= 0) == [True, False, True, False] and np.isnan(dec[[1, 3]]).all() and not np.isnan(dec[[0, 2]]).any()


def _plan(L, y, train, classes, short=0, fill=0x5a):
    buf = np.full(L.size('hv_svm_fit_plan_bytes', len(y)) - short, fill, np.uint8)
    rows = ctypes.c_int(-1)
    rc = L.cdll.hv_svm_fit_plan(y.ctypes.data, None if train is None else train.ctypes.data, len(y), classes.ctypes.data, len(classes), buf.ctypes.data,
                                ctypes.c_size_t(buf.nbytes), ctypes.byref(rows))
    return rc, rows.value, buf


def test_fit_plan_on_the_host():
    import hvgan  # noqa: F401
    from hvgan import evaluation, lib
    L = lib.get()
    g = g22()
    y = g['c/y'].astype(np.int32)
    cl = np.unique(y).astype(np.int32)
    M = len(y)
    assert L.size('hv_svm_fit_plan_bytes', 0) == 0 and L.size('hv_svm_fit_plan_bytes', M) == 32 + 4 * (8 + 4 + 2 * M)
    for train in (None, np.ones(M, np.int32), (np.arange(M) % 3 != 0).astype(np.int32), (y != 3).astype(np.int32), 7 * (y != 0).astype(np.int32)):
        rc, rows, buf = _plan(L, y, train, cl)
        tr = np.ones(M, bool) if train is None else train != 0
        cls, bnd = R.balanced_bounds(y[tr])
        want = np.zeros(4)
        want[np.searchsorted(cl, cls)] = bnd
        assert rc == 0 and np.array_equal(buf[:32].view(np.float64), want)          # the same two divisions: bit for bit
        ints = buf[32:].view(np.int32)
        assert list(ints[:4]) == [0x53564d32, M, 4, rows] and np.array_equal(ints[8:12] != 0, np.isin(cl, cls))
        assert rows == max(np.isin(y[tr], (a, b)).sum() for a in cls for b in cls if a < b)
        assert np.array_equal(ints[12:12 + M], np.searchsorted(cl, y)) and np.array_equal(ints[12 + M:12 + 2 * M], tr.astype(np.int32))
        if train is None:
            ones = _plan(L, y, np.ones(M, np.int32), cl)
            assert ones[0] == 0 and ones[1] == rows and ones[2].tobytes() == buf.tobytes()
    # every refusal leaves the plan buffer untouched
    untouched = lambda buf: np.all(buf == 0x5a)
    for kw, want in ((dict(classes=cl[::-1].copy()), -1), (dict(classes=cl[:3].copy()), -1), (dict(classes=np.array([-1, 0, 1, 2, 3], np.int32)[:4].copy()), -1),
                     (dict(classes=np.arange(5, dtype=np.int32)), -2), (dict(classes=cl[:1].copy()), -2), (dict(short=8), -3)):
        rc, rows, buf = _plan(L, y, None, kw.get('classes', cl), kw.get('short', 0))
        assert rc == want and untouched(buf), kw
    rows = ctypes.c_int(-1)
    buf = np.full(4096, 0x5a, np.uint8)
    for args in ((None, None, M, cl.ctypes.data, 4, buf.ctypes.data), (y.ctypes.data, None, 0, cl.ctypes.data, 4, buf.ctypes.data),
                 (y.ctypes.data, None, M, None, 4, buf.ctypes.data), (y.ctypes.data, None, M, cl.ctypes.data, 4, None)):
        assert L.cdll.hv_svm_fit_plan(*args, ctypes.c_size_t(buf.nbytes), ctypes.byref(rows)) == -1 and untouched(buf)
    assert L.cdll.hv_svm_fit_plan(y.ctypes.data, None, M, cl.ctypes.data, 4, buf.ctypes.data, ctypes.c_size_t(buf.nbytes), None) == -1 and untouched(buf)
    big = (np.arange(1793, dtype=np.int32) % 2).copy()
    rc, rows, buf = _plan(L, big, None, np.arange(2, dtype=np.int32))
    assert rc == -2 and rows == 1793 and rows > evaluation.MAX_PAIR_ROWS and untouched(buf)
    rc, rows, buf = _plan(L, big[:1792].copy(), None, np.arange(2, dtype=np.int32))
    assert rc == 0 and rows == 1792


def _model(case='a'):
    """A model dict as svm_fit returns it, from the restatement (no GPU)."""
    r = fitted(case)
    m = {k: np.ascontiguousarray(r[k]) for k in ('mean', 'scale', 'w', 'b', 'gap')}
    m.update({k: r[k].astype(np.int32) for k in ('iterations', 'status', 'support', 'pair_rows')})
    m.update(unusable=np.array(False), classes=r['classes'].astype(np.int32), present=r['present'].copy())
    return m


def test_grader_state_round_trip_is_byte_for_byte():
    import hvgan  # noqa: F401
    from hvgan import evaluation
    gr = evaluation.Grader((5, 0.64), _model(), 'coronal')
    sd = gr.state_dict()
    assert all(isinstance(v, (np.ndarray, int, float, str)) for v in sd.values()) and sd['file1'] == 'coronal'
    assert (sd['length_divisor'], sd['height_threshold']) == (5, 0.64) and set(evaluation.MODEL_KEYS) <= set(sd)
    again = evaluation.Grader.from_state_dict(sd)
    f = io.BytesIO()
    np.savez(f, **sd)
    f.seek(0)
    loaded = evaluation.Grader.from_state_dict(np.load(f))
    for other in (again, loaded):
        od = other.state_dict()
        assert other.setting == gr.setting and other.file1 == gr.file1 and set(od) == set(sd)
        for k in evaluation.MODEL_KEYS:
            assert od[k].dtype == sd[k].dtype and od[k].shape == sd[k].shape and od[k].tobytes() == sd[k].tobytes(), k
    sd['w'][0, 0] = 7.0                                   # the state is a copy: the grader keeps its own arrays
    assert gr.model['w'][0, 0] != 7.0
    with pytest.raises(ValueError):
        evaluation.Grader.from_state_dict({k: v for k, v in sd.items() if k != 'b'})
    with pytest.raises(ValueError):
        evaluation.Grader((5, 0.64), _model(), 'axial')
    grid = {k: (np.stack([v, v]) if k not in ('classes', 'present') else v) for k, v in _model().items()}
    with pytest.raises(ValueError):
        evaluation.Grader((5, 0.64), grid)


def test_python_entries_refuse_before_any_launch(monkeypatch):
    import hvgan  # noqa: F401
    from hvgan import evaluation, lib

    class NoLaunch:
        """The library with every device entry barred: a refusal must come before any of them is reached."""
        def __init__(self, real):
            self.cdll, self.real = real.cdll, real
        def size(self, *a):
            return self.real.size(*a)
        def call(self, name, *a):
            raise AssertionError('launched ' + name)
    real = lib.get()
    monkeypatch.setattr(evaluation._lib, 'get', lambda: NoLaunch(real))
    g = g22()
    X, y = g['a/X'], g['a/y']
    for bad in (dict(features=np.concatenate([X, X[:, :1]], axis=1)), dict(labels=np.arange(len(y)) % 5), dict(labels=np.zeros(len(y), int)),
                dict(labels=y - 5), dict(labels=y + 0.5), dict(labels=y[:-1]), dict(tol=0.0), dict(max_iter=0), dict(train=np.ones(3)),
                dict(features=np.full_like(X, np.nan)), dict(features=X[:, None, :][:, :0])):
        kw = dict(features=X, labels=y)
        kw.update(bad)
        with pytest.raises(ValueError):
            evaluation.svm_fit(**kw)
    with pytest.raises(ValueError, match='LDS'):
        evaluation.svm_fit(np.zeros((1793, 3)), np.arange(1793) % 2)
    m = _model()
    for feats in (X[:, :2], X[:, None, :], X[:0], np.concatenate([X, X], axis=1)):
        with pytest.raises(ValueError):
            evaluation.svm_predict(m, feats)
    for key, val in (('w', m['w'][:2]), ('present', m['present'][:2]), ('classes', np.arange(5)), ('status', m['status'][:1])):
        with pytest.raises(ValueError):
            evaluation.svm_predict(dict(m, **{key: val}), X)
    with pytest.raises(ValueError):
        evaluation.svm_predict({k: v for k, v in m.items() if k != 'scale'}, X)
    gr = evaluation.Grader((5, 0.64), m)
    with pytest.raises(ValueError):
        gr.predict(X[:, :2])
    with pytest.raises(ValueError):
        gr.grade_dataset([], [], [])
    sweep = {'records': np.zeros((len(y), 2, 2, 2, 16)), 'length_divisors': np.array([4, 5]), 'height_thresholds': np.array([0.6, 0.7]),
             'views': ('sagittal', 'coronal'), 'raised': np.zeros((len(y), 2), bool)}
    ds = np.array(['train'] * len(y))
    for kw in (dict(setting=(3, 0.6)), dict(setting=(4, 0.65)), dict(setting=(4, 0.6), file1='axial'), dict(setting=(4, 0.6), labels=y[:-1]),
               dict(setting=(4, 0.6), dataset=np.array(['fit'] * len(y)))):
        args = dict(sweep=sweep, labels=y, dataset=ds)
        args.update(kw)
        with pytest.raises(ValueError):
            evaluation.fit_grader(**args)
