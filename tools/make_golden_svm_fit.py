"""Golden vectors G22 for fitting the fracture grader once and grading held-out rows: scikit-learn 1.7.2's
StandardScaler + SVC(kernel='linear', class_weight='balanced') -- the classifier of the reference's evaluation/SVM_grading.py and
SVM_grading_2.5d.py -- fitted on ALL the train + test rows of small synthetic tables, at the default tol=1e-3 and at tol=1e-10, with predict and
decision_function(ovo) on held-out rows (libsvm's sign convention: positive = the pair's lower class, decision = coef . x - b).

Per case delta = 2 x the largest movement of a held-out decision value between the two tolerances (as in G19); `near` marks the held-out rows
with a tight pairwise |decision| below delta.  A case's seed is redrawn until at most 1 % of its held-out rows are near, so the fixture alone
stays inside the cap the tests assert.  The tool also prints the largest difference between tests/svm_fit_ref.py (1e-12 gap) and the tight SVC:
ten times that is the solver tolerance of the tests, unless G19's measurement (svm_ref.SOLVER_TOL) is larger.

Needs scikit-learn (1.7.2 here); runs on a development machine, never on the GPU machine.

    python tools/make_golden_svm_fit.py
writes tests/golden/g22_svm_fit.npz.
"""
import argparse
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
#        name: (fit rows, held-out rows, F, class labels, constant column or None, rare class (about 5 % of the rows) or None, noise sigma)
CASES = {'a': (90, 100, 3, (1, 2, 3), None, None, 0.3),
         'b': (120, 100, 6, (0, 1, 2), None, None, 0.3),
         'c': (150, 100, 6, (0, 1, 2, 3), None, 3, 0.25),
         'd': (60, 100, 3, (0, 1), None, None, 0.45),
         'e': (80, 100, 6, (0, 1, 2), 4, None, 0.3)}
CAP = 0.01


def draw(name, seed):
    M, Mh, F, labels, const, rare, sigma = CASES[name]
    rng = np.random.default_rng([22, ord(name), seed])
    labels = np.array(labels)
    K = len(labels)
    prob = np.full(K, 1.0 / K)
    if rare is not None:
        k = list(labels).index(rare)
        prob[:] = 0.95 / (K - 1)
        prob[k] = 0.05
    y, yh = rng.choice(K, M, p=prob), rng.choice(K, Mh, p=prob)
    if rare is not None:
        y[:3] = list(labels).index(rare)             # the rare class always has a few members to fit on
    cen = rng.normal(0, 0.25, (K, F)) + np.linspace(0, 0.6, K)[:, None]
    X = cen[y] + rng.normal(0, sigma, (M, F))
    Xh = cen[yh] + rng.normal(0, sigma, (Mh, F))
    if const is not None:
        X[:, const] = 0.37
        Xh[:, const] = 0.37
    return X, labels[y], Xh, labels[yh]


def svc(X, y, Xh, tol):
    """-> (decision [Mh, P], coef [P, F], b [P], pred [Mh], class_weight [K], mean, scale) in libsvm's sign convention."""
    from sklearn.preprocessing import StandardScaler
    from sklearn.svm import SVC
    sc = StandardScaler()
    Xs, Xhs = sc.fit_transform(X), sc.transform(Xh)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        m = SVC(kernel='linear', class_weight='balanced', tol=tol, decision_function_shape='ovo').fit(Xs, y)
    d = m.decision_function(Xhs).reshape(len(Xh), -1)
    c, i0 = m.coef_, m.intercept_
    if len(m.classes_) == 2:                          # scikit-learn flips the sign of the binary problem
        d, c, i0 = -d, -c, -i0
    return d, c, -i0, m.predict(Xhs), m.class_weight_, sc.mean_, sc.scale_


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden'))
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import svm_ref as R
    import svm_fit_ref as FR
    arrs, worst = {}, 0.0
    for name in CASES:
        for seed in range(200):
            X, y, Xh, yh = draw(name, seed)
            if len(np.unique(y)) != len(CASES[name][3]):
                continue
            tight, loose = svc(X, y, Xh, 1e-10), svc(X, y, Xh, 1e-3)
            delta = 2.0 * np.max(np.abs(tight[0] - loose[0]))
            near = np.abs(tight[0]).min(axis=1) < delta          # [Mh]
            if near.mean() <= CAP:
                break
        else:
            raise SystemExit('no seed for case ' + name)
        assert (tight[3] != loose[3])[~near].sum() == 0          # scikit-learn agrees with itself away from the boundaries
        ref = FR.fit(X, y)
        assert np.all(ref['status'] == R.CONVERGED) and ref['present'].all()
        pred, dec = FR.predict(ref, Xh)
        assert np.array_equal(R.vote(tight[0], ref['present']), np.searchsorted(ref['classes'], tight[3]))   # libsvm's vote of the recorded decisions
        gap = max(np.max(np.abs(ref['w'] - tight[1])), np.max(np.abs(ref['b'] - tight[2])), np.max(np.abs(dec - tight[0])))
        worst = max(worst, gap)
        assert np.array_equal(ref['classes'][pred][~near], loose[3][~near])
        print('case %s seed %d delta %.3g near %d/%d |svm_fit_ref - SVC(1e-10)| %.3g rows per class %s' % (
            name, seed, delta, near.sum(), near.size, gap, np.unique(y, return_counts=True)[1]))
        for k, v in (('X', X), ('y', y.astype(np.int64)), ('X_held', Xh), ('y_held', yh.astype(np.int64)), ('mean', tight[5]), ('scale', tight[6]),
                     ('bounds', tight[4]), ('pred', loose[3].astype(np.int64)), ('loose_dec', loose[0]), ('tight_pred', tight[3].astype(np.int64)),
                     ('tight_dec', tight[0]), ('tight_coef', tight[1]), ('tight_b', tight[2]), ('delta', np.array(delta)), ('near', near),
                     ('seed', np.array(seed))):
            arrs['%s/%s' % (name, k)] = v
    arrs['solver_gap'] = np.array(worst)
    path = os.path.join(args.out, 'g22_svm_fit.npz')
    np.savez_compressed(path, **arrs)
    print(path, os.path.getsize(path), 'bytes; largest |svm_fit_ref(1e-12) - SVC(1e-10)| over G22: %.3g (G19: %.3g)' % (worst, R.SOLVER_TOL / 10))


if __name__ == '__main__':
    main()
