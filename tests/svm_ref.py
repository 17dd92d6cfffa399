"""Plain numpy float64 restatement of the reference's grading chain (evaluation/SVM_grading.py:21-52,63-71, SVM_grading_2.5d.py:33-59), written from
the published algorithms and independently of csrc/svm_grade.hip:
  scaler            StandardScaler: column mean and population standard deviation, a column indistinguishable from a constant gets scale 1
                    (scikit-learn's _is_constant_feature / _handle_zeros_in_scale)
  stratified_folds  the unshuffled StratifiedKFold assignment
  balanced_bounds   class_weight='balanced' with C = 1: n_train / (n_classes_in_train * count(class))
  smo               libsvm's C-SVC dual for one class pair (Fan, Chen, Lin 2005: maximal violating pair with the second-order choice of the
                    second variable, two-variable update with clipping), run to a KKT gap of 1e-12 by default; calculate_rho
  fit_fold / vote   one-vs-one over the sorted classes of a fold's training rows, the +1 side the lower class, libsvm's voting
  metrics           confusion matrix, macro F1 / precision / recall over the classes that occur in y_true or y_pred, accuracy
  grade             the whole chain for one feature set -> what evaluate_svm computes per fold, and the mean / np.var over the folds
It is a helper module of the tests and of tools/make_golden_svm_grading.py, not a test file."""
import numpy as np

N_SPLITS = 5
TAU = 1e-12
CONVERGED, MAX_ITER, ABSENT = 0, 1, 2            # a problem's status, as hv_svm_grade_grid reports it
# Solver tolerance of the tests (absolute, on w, b and decision values of the scaled features, all O(1)): ten times the largest difference
# between the two independent reference solutions over fixture G19 -- this module run to a 1e-12 gap against scikit-learn's SVC at
# tol=1e-10, 2.07e-6 as tools/make_golden_svm_grading.py measured it (libsvm keeps its kernel rows in float32, which is what limits SVC).
SOLVER_TOL = 10 * 2.07e-6
CASES = ('a', 'b', 'c', 'd', 'e')


def scaler(X):
    """-> (mean [F], scale [F]) of the rows of X."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    mean = X.sum(axis=0) / n
    d = X - mean
    var = ((d * d).sum(axis=0) - d.sum(axis=0) ** 2 / n) / n
    eps = np.finfo(np.float64).eps
    constant = var <= n * eps * var + (n * mean * eps) ** 2
    scale = np.sqrt(var)
    scale[constant | (scale == 0.0)] = 1.0
    return mean, scale


def stratified_folds(y, n_splits=N_SPLITS):
    """One test-fold id per row: classes in order of first appearance, each class's rows dealt to the folds in contiguous blocks whose sizes
    come from dealing the sorted labels round robin."""
    y = np.asarray(y)
    _, first, inv = np.unique(y, return_index=True, return_inverse=True)
    enc = np.argsort(np.argsort(first))[inv]
    k = len(first)
    order = np.sort(enc)
    alloc = np.array([np.bincount(order[i::n_splits], minlength=k) for i in range(n_splits)])
    folds = np.empty(len(y), dtype=np.int32)
    for c in range(k):
        folds[enc == c] = np.arange(n_splits).repeat(alloc[:, c])
    return folds


def balanced_bounds(y_train):
    """-> (classes present, sorted; the bound on alpha of a row of each of them)."""
    cls, cnt = np.unique(y_train, return_counts=True)
    return cls, len(y_train) / (len(cls) * cnt.astype(np.float64))


def smo(X, y, C, tol=1e-12, max_iter=10 ** 7):
    """min 1/2 a'Qa - e'a, 0 <= a_i <= C_i, y'a = 0 with Q_ij = y_i y_j x_i.x_j.  X [n, F], y [n] of +-1, C [n].
    -> dict(w, b (libsvm's rho), alpha, grad, iterations, gap, status, nsv).  Ties go to the lowest row."""
    X, y, C = np.asarray(X, np.float64), np.asarray(y, np.float64), np.asarray(C, np.float64)
    n = len(y)
    a = np.zeros(n)
    G = -np.ones(n)
    qd = (X * X).sum(axis=1)
    it, status = 0, MAX_ITER
    while True:
        up = ((y > 0) & (a < C)) | ((y < 0) & (a > 0))
        low = ((y > 0) & (a > 0)) | ((y < 0) & (a < C))
        mg = np.where(up, -y * G, -np.inf)
        i = int(np.argmax(mg))
        gmax = mg[i]
        gmax2 = np.max(np.where(low, y * G, -np.inf))
        gap = gmax + gmax2
        if gap <= tol:
            status = CONVERGED
            break
        if it >= max_iter:
            break
        ki = X @ X[i]
        diff = gmax + y * G
        quad = qd[i] + qd - 2.0 * ki
        quad = np.where(quad > 0, quad, TAU)
        obj = np.where(low & (diff > 0), -(diff * diff) / quad, np.inf)
        j = int(np.argmin(obj))
        kj = X @ X[j]
        ai, aj = a[i], a[j]
        if y[i] != y[j]:
            q = qd[i] + qd[j] - 2.0 * ki[j]
            q = q if q > 0 else TAU
            delta = (-G[i] - G[j]) / q
            d = a[i] - a[j]
            a[i] += delta
            a[j] += delta
            if d > 0:
                if a[j] < 0:
                    a[j], a[i] = 0.0, d
            elif a[i] < 0:
                a[i], a[j] = 0.0, -d
            if d > C[i] - C[j]:
                if a[i] > C[i]:
                    a[i], a[j] = C[i], C[i] - d
            elif a[j] > C[j]:
                a[j], a[i] = C[j], C[j] + d
        else:
            q = qd[i] + qd[j] - 2.0 * ki[j]
            q = q if q > 0 else TAU
            delta = (G[i] - G[j]) / q
            s = a[i] + a[j]
            a[i] -= delta
            a[j] += delta
            if s > C[i]:
                if a[i] > C[i]:
                    a[i], a[j] = C[i], s - C[i]
            elif a[j] < 0:
                a[j], a[i] = 0.0, s
            if s > C[j]:
                if a[j] > C[j]:
                    a[j], a[i] = C[j], s - C[j]
            elif a[i] < 0:
                a[i], a[j] = 0.0, s
        G += y * (y[i] * ki * (a[i] - ai) + y[j] * kj * (a[j] - aj))
        it += 1
    # calculate_rho
    yg = y * G
    free = (a > 0) & (a < C)
    if free.any():
        b = yg[free].sum() / free.sum()
    else:
        upper = (((a >= C) & (y < 0)) | ((a <= 0) & (y > 0)))
        lower = (((a >= C) & (y > 0)) | ((a <= 0) & (y < 0)))
        b = (np.min(np.where(upper, yg, np.inf)) + np.max(np.where(lower, yg, -np.inf))) / 2
    return {'w': (a * y) @ X, 'b': b, 'alpha': a, 'grad': G, 'iterations': it, 'gap': gap, 'status': status, 'nsv': int((a > 0).sum()),
            'n_free': int(free.sum()), 'n_bounded': int((a >= C).sum())}


def pairs(k):
    return [(a, b) for a in range(k) for b in range(a + 1, k)]


def fit_fold(Xs, y, classes, tol=1e-12, max_iter=10 ** 7):
    """Scaled training rows of one fold, their labels, the global sorted class list -> one problem per global class pair
    (dict(status=ABSENT) where a class of the pair is missing from the rows), and the classes present (bool [K])."""
    present_cls, bounds = balanced_bounds(y)
    cb = dict(zip(present_cls.tolist(), bounds.tolist()))
    present = np.array([c in cb for c in classes.tolist()])
    out = []
    for p, q in pairs(len(classes)):
        if not (present[p] and present[q]):
            out.append({'status': ABSENT})
            continue
        lo, hi = classes[p], classes[q]
        rows = np.concatenate([np.flatnonzero(y == lo), np.flatnonzero(y == hi)])
        sign = np.where(y[rows] == lo, 1.0, -1.0)
        C = np.where(y[rows] == lo, cb[lo], cb[hi])
        r = smo(Xs[rows], sign, C, tol, max_iter)
        r['rows'] = rows
        out.append(r)
    return out, present


def decisions(problems, Xs):
    """-> [rows, pairs] w.x - b, NaN for an absent pair."""
    d = np.full((Xs.shape[0], len(problems)), np.nan)
    for k, r in enumerate(problems):
        if r['status'] != ABSENT:
            d[:, k] = Xs @ r['w'] - r['b']
    return d


def vote(dec, present):
    """Pairwise decisions [rows, pairs] -> the class index per row: a decision > 0 votes for the pair's lower class, the most votes win, ties go
    to the lowest class; only classes present in the training rows are candidates."""
    k = len(present)
    votes = np.zeros((dec.shape[0], k), dtype=np.int64)
    for col, (p, q) in enumerate(pairs(k)):
        if present[p] and present[q]:
            votes[:, p] += dec[:, col] > 0
            votes[:, q] += ~(dec[:, col] > 0)
    votes[:, ~present] = -1
    return np.argmax(votes, axis=1)


def confusion(true_idx, pred_idx, k):
    cm = np.zeros((k, k), dtype=np.int64)
    np.add.at(cm, (true_idx, pred_idx), 1)
    return cm


def scores(cm):
    """K x K confusion matrix -> [macro F1, macro precision, macro recall, accuracy] by scikit-learn's rule: the average runs over the classes
    that occur in the true or the predicted labels, a class with an empty denominator contributes 0."""
    cm = np.asarray(cm, dtype=np.float64)
    tp, true, pred = np.diag(cm), cm.sum(axis=1), cm.sum(axis=0)
    used = (true + pred) > 0
    def div(a, b):
        return np.where(b > 0, a / np.where(b > 0, b, 1.0), 0.0)
    f1, prec, rec = div(2 * tp, true + pred), div(tp, pred), div(tp, true)
    n = used.sum()
    return np.array([f1[used].sum() / n, prec[used].sum() / n, rec[used].sum() / n, tp.sum() / cm.sum()])


def mean_var(s):
    """[5, 4] scores -> (mean, np.var) over the folds."""
    s = np.asarray(s, dtype=np.float64)
    m = s.sum(axis=0) / s.shape[0]
    return m, ((s - m) ** 2).sum(axis=0) / s.shape[0]


def grade(X_tt, y_tt, X_val, y_val, tol=1e-12, max_iter=10 ** 7, folds=None):
    """The whole chain for one feature set.  -> dict: classes, folds, mean, scale, bounds [5, K] (NaN for an absent class), present [5, K],
    problems (5 lists), w [5, P, F], b [5, P], decision [5, Mv, P], pred [5, Mv] (class indices), confusion [5, K, K], scores [5, 4], mean_scores,
    var_scores."""
    X_tt, X_val = np.asarray(X_tt, np.float64), np.asarray(X_val, np.float64)
    y_tt, y_val = np.asarray(y_tt), np.asarray(y_val)
    classes = np.unique(np.concatenate([y_tt, y_val]))
    K, F = len(classes), X_tt.shape[1]
    P = K * (K - 1) // 2
    mean, scale = scaler(X_tt)
    Xs, Xv = (X_tt - mean) / scale, (X_val - mean) / scale
    folds = stratified_folds(y_tt) if folds is None else np.asarray(folds)
    true_idx = np.searchsorted(classes, y_val)
    out = {'classes': classes, 'folds': folds, 'mean': mean, 'scale': scale, 'bounds': np.full((N_SPLITS, K), np.nan),
           'present': np.zeros((N_SPLITS, K), dtype=bool), 'problems': [], 'w': np.full((N_SPLITS, P, F), np.nan), 'b': np.full((N_SPLITS, P), np.nan),
           'decision': np.full((N_SPLITS, len(y_val), P), np.nan), 'pred': np.zeros((N_SPLITS, len(y_val)), dtype=np.int64),
           'confusion': np.zeros((N_SPLITS, K, K), dtype=np.int64), 'scores': np.zeros((N_SPLITS, 4)),
           'iterations': np.zeros((N_SPLITS, P), dtype=np.int64), 'status': np.zeros((N_SPLITS, P), dtype=np.int64), 'gap': np.full((N_SPLITS, P), np.nan)}
    for f in range(N_SPLITS):
        tr = folds != f
        problems, present = fit_fold(Xs[tr], y_tt[tr], classes, tol, max_iter)
        cls, bnd = balanced_bounds(y_tt[tr])
        out['bounds'][f, np.searchsorted(classes, cls)] = bnd
        out['present'][f] = present
        out['problems'].append(problems)
        for k, r in enumerate(problems):
            out['status'][f, k] = r['status']
            if r['status'] != ABSENT:
                out['w'][f, k], out['b'][f, k], out['iterations'][f, k], out['gap'][f, k] = r['w'], r['b'], r['iterations'], r['gap']
        out['decision'][f] = decisions(problems, Xv)
        out['pred'][f] = vote(out['decision'][f], present)
        out['confusion'][f] = confusion(true_idx, out['pred'][f], K)
        out['scores'][f] = scores(out['confusion'][f])
    out['mean_scores'], out['var_scores'] = mean_var(out['scores'])
    return out
