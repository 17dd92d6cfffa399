"""Plain numpy float64 restatement of "fit the grader on chosen rows, keep it, grade other rows" (hv_svm_fit / hv_svm_predict), built from the
functions tests/svm_ref.py already has (scaler, balanced_bounds, smo through fit_fold, decisions, vote):
  fit       StandardScaler over ALL the rows given (the reference scales before it splits), one-vs-one C-SVC with class_weight='balanced' on the
            rows with train != 0, the pairs of the sorted classes in the order (0,1), (0,2), ...
  predict   scaled rows -> decisions w.x - b, libsvm's vote among the classes that had train rows; a row with a non-finite feature gets -1
  contrib   w[p][c] * x_scaled[c]: summed in column order minus b it is the decision
It is a helper module of the tests and of tools/make_golden_svm_fit.py, not a test file."""
import os

import numpy as np

import svm_ref as R

CASES = ('a', 'b', 'c', 'd', 'e')
# Solver tolerance of the fit tests (absolute, on w, b and decision values of the scaled features): ten times the largest difference between
# this module run to a 1e-12 gap and scikit-learn's SVC at tol=1e-10.  Over fixture G22 tools/make_golden_svm_fit.py measured 1.85e-6 (stored as G22's 'solver_gap'), below
# G19's 2.07e-6, so the constant the project derived for G19 stands.
SOLVER_TOL = R.SOLVER_TOL


def g22(golden_dir):
    return dict(np.load(os.path.join(golden_dir, 'g22_svm_fit.npz')))


def fit(X, y, train=None, tol=1e-12, max_iter=10 ** 7, classes=None):
    """-> dict(classes, present [K], mean, scale, bounds [K] (NaN: no train row), problems, w [P, F], b, gap [P], status, iterations, support [P])."""
    X, y = np.asarray(X, np.float64), np.asarray(y)
    tr = np.ones(len(y), dtype=bool) if train is None else np.asarray(train) != 0
    classes = np.unique(y) if classes is None else np.asarray(classes)
    K, F = len(classes), X.shape[1]
    P = K * (K - 1) // 2
    mean, scale = R.scaler(X)
    Xs = (X - mean) / scale
    problems, present = R.fit_fold(Xs[tr], y[tr], classes, tol, max_iter)
    out = {'classes': classes, 'present': present, 'mean': mean, 'scale': scale, 'bounds': np.full(K, np.nan), 'problems': problems,
           'w': np.full((P, F), np.nan), 'b': np.full(P, np.nan), 'gap': np.full(P, np.nan), 'status': np.zeros(P, dtype=np.int64),
           'iterations': np.zeros(P, dtype=np.int64), 'support': np.zeros(P, dtype=np.int64), 'pair_rows': np.zeros(P, dtype=np.int64)}
    cls, bnd = R.balanced_bounds(y[tr])
    out['bounds'][np.searchsorted(classes, cls)] = bnd
    for k, r in enumerate(problems):
        out['status'][k] = r['status']
        if r['status'] != R.ABSENT:
            out['w'][k], out['b'][k], out['gap'][k], out['iterations'][k] = r['w'], r['b'], r['gap'], r['iterations']
            out['support'][k], out['pair_rows'][k] = r['nsv'], len(r['rows'])
    return out


def contrib(model, X):
    """-> [rows, P, F]: w[p][c] * x_scaled[c]."""
    Xs = (np.asarray(X, np.float64) - model['mean']) / model['scale']
    return model['w'][None, :, :] * Xs[:, None, :]


def decision(model, X):
    """-> [rows, P]: the contributions summed in column order, minus b (NaN for an absent pair)."""
    c = contrib(model, X)
    d = np.zeros(c.shape[:2])
    for col in range(c.shape[2]):
        d = d + c[:, :, col]
    return d - model['b'][None, :]


def predict(model, X):
    """-> (class index per row, -1 for a row with a non-finite feature or where no class is present; decisions [rows, P])."""
    X = np.asarray(X, np.float64)
    ok = np.isfinite(X).all(axis=1)
    dec = np.full((len(X), len(model['b'])), np.nan)
    pred = np.full(len(X), -1, dtype=np.int64)
    if ok.any() and model['present'].any():
        dec[ok] = decision(model, X[ok])
        pred[ok] = R.vote(dec[ok], model['present'])
    return pred, dec
