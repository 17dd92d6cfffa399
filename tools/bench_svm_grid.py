"""Time evaluation.svm_grade_grid (hv_svm_grade_grid) on the sweep's workload: G = 40 and G = 512 grid points, M ~ 400 train + test rows,
100 val rows, F = 6, K = 3 -- device time of the launch sequence (events around repeated calls of the C entry on resident inputs), wall time
of the whole Python call (upload, launches, readback), iterations per problem, and the host side of the comparison: tests/svm_ref.py at the
same tolerance on a few grid points, EXTRAPOLATED to the grid, and scikit-learn's SVC loop where scikit-learn happens to be importable.

    python tools/bench_svm_grid.py [--grid 40 512] [--rows 400] [--val 100] [--host-points 2]
prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def workload(G, M, Mv, F=6, K=3, seed=0):
    """Overlapping shifted Gaussians; every grid point its own mild distortion of the same rows, as a sweep's neighbouring settings are."""
    rng = np.random.default_rng(seed)
    y = rng.integers(0, K, M + Mv)
    cen = rng.normal(0, 0.25, (K, F)) + np.linspace(0, 0.6, K)[:, None]
    base = cen[y] + rng.normal(0, 0.3, (M + Mv, F))
    feats = np.stack([base * rng.uniform(0.8, 1.25, F) + rng.normal(0, 0.03, base.shape) for _ in range(G)], axis=1)
    return feats, y, np.array(['train'] * M + ['val'] * Mv)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--grid', type=int, nargs='+', default=[40, 512])
    ap.add_argument('--rows', type=int, default=400)
    ap.add_argument('--val', type=int, default=100)
    ap.add_argument('--host-points', type=int, default=2)
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    import torch
    import hvgan  # noqa: F401
    from hvgan import evaluation
    import svm_ref as R
    out = {'rows': args.rows, 'val': args.val, 'F': 6, 'K': 3, 'tol': 1e-3, 'grids': {}}
    for G in args.grid:
        feats, y, ds = workload(G, args.rows, args.val)
        res = evaluation.svm_grade_grid(feats, y, ds)              # warm-up: library load, allocator
        torch.cuda.synchronize()
        wall = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            res = evaluation.svm_grade_grid(feats, y, ds)
            wall.append(time.perf_counter() - t0)
        # device time: the launch sequence alone, between two events, on the same stream
        dev = []
        orig = evaluation._lib.get().call
        for _ in range(args.reps):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

            def timed(name, *a, _ev=ev):
                _ev[0].record()
                orig(name, *a)
                _ev[1].record()
            evaluation._lib.get().call = timed
            try:
                evaluation.svm_grade_grid(feats, y, ds)
            finally:
                evaluation._lib.get().call = orig
            torch.cuda.synchronize()
            dev.append(ev[0].elapsed_time(ev[1]))
        it = res['iterations'][res['status'] == evaluation.CONVERGED]
        out['grids'][str(G)] = {'device_ms': float(np.median(dev)), 'wall_ms': 1e3 * float(np.median(wall)), 'problems': int(res['status'].size),
                                'not_converged': int((res['status'] == evaluation.HIT_MAX_ITER).sum()),
                                'iterations_median': float(np.median(it)), 'iterations_max': int(it.max()),
                                'best_mean_f1': float(np.nanmax(res['mean'][..., 0]))}
    # the host loop, on a few grid points of the last workload
    tt = ds != 'val'
    n = min(args.host_points, feats.shape[1])
    t0 = time.perf_counter()
    for gp in range(n):
        r = R.grade(feats[tt, gp], y[tt], feats[~tt, gp], y[~tt], tol=1e-3)
    per = (time.perf_counter() - t0) / n
    out['host_restatement_s_per_grid_point'] = per
    out['host_restatement_s_extrapolated'] = {str(G): per * G for G in args.grid}
    out['host_matches_device_scores'] = bool(np.allclose(r['scores'], res['scores'][n - 1], atol=0.05))
    try:
        import warnings
        from sklearn.model_selection import StratifiedKFold
        from sklearn.preprocessing import StandardScaler
        from sklearn.svm import SVC
        t0 = time.perf_counter()
        for gp in range(n):
            sc = StandardScaler()
            Xs, Xv = sc.fit_transform(feats[tt, gp]), sc.transform(feats[~tt, gp])
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                for tr, _ in StratifiedKFold(5).split(Xs, y[tt]):
                    SVC(kernel='linear', class_weight='balanced').fit(Xs[tr], y[tt][tr]).predict(Xv)
        per = (time.perf_counter() - t0) / n
        out['sklearn_s_per_grid_point'] = per
        out['sklearn_s_extrapolated'] = {str(G): per * G for G in args.grid}
    except ImportError:
        out['sklearn_s_per_grid_point'] = None
    print(json.dumps(out))


if __name__ == '__main__':
    main()
