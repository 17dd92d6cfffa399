"""The coronal RHLV restatement (tests/rhlv_coronal_ref.py) against the reference's own outputs (fixture G15, written by
tools/make_golden_rhlv_coronal.py from evaluation/RHLV_quantification_coronal.py), on the CPU.  The restatement's float64 steps are the
reference's, so outputs and means agree to the last few ulps of numpy's summation: 1e-12 relative, as everywhere for RHLV."""
import numpy as np
import pytest

from conftest import load_golden
import rhlv_coronal_ref as C

TOL = 1e-12


def _close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.all(np.abs(a - b) <= TOL * np.maximum(1.0, np.abs(b)))


def _cases():
    g = {k: np.asarray(v) for k, v in load_golden('g15_rhlv_coronal').items()}
    return g, sorted({k.split('/')[0] for k in g} - {'narrow'})


def test_restatement_matches_reference_golden():
    g, names = _cases()
    assert len(names) >= 4
    raised = 0
    for n in names:
        idx, div, thr, center, length = (float(v) for v in g[n + '/params'])
        fake, label = g[n + '/fake'], g[n + '/label']
        assert C.center_length(label == idx, int(div)) == (int(center), int(length)), n
        if g[n + '/raises']:
            raised += 1
            with pytest.raises(ValueError):
                C.rhlv_volume(fake, label, idx, int(div), thr)
            continue
        res, means = C.rhlv_volume(fake, label, idx, int(div), thr)
        assert _close(res, g[n + '/out']), (n, res, g[n + '/out'])
        assert _close(means, g[n + '/means']), (n, means, g[n + '/means'])
        # binary volumes and the explicit range
        res2, _ = C.rhlv((fake == idx).astype(np.float64), (label == idx).astype(np.float64), int(center), int(length), thr)
        assert _close(res2, g[n + '/out']), n
    assert raised >= 1


def test_restatement_raises_where_the_reference_does_on_narrow_extents():
    """Generated vertebra spanning columns [y_min, y_min + y_range], y_range 0..3, y_min 0 and > 0: the rows of the reference's own table."""
    g, _ = _cases()
    table = g['narrow/table']
    assert sorted(set(table[:, 1])) == [0, 1, 2, 3] and set(table[:, 0] > 0) == {False, True} and set(table[:, 2]) == {0, 1}
    for (y_min, y_range, raised), fake, label in zip(table, g['narrow/fake'], g['narrow/label']):
        if raised:
            with pytest.raises(ValueError):
                C.heights(fake, label, 0.64)
        else:
            C.heights(fake, label, 0.64)


def test_coronal_is_not_the_sagittal_script_on_a_permuted_volume():
    """oracle.restate.rhlv_volume on the [H, Z, W] view slices and walks what the coronal script does, with the sagittal script's ratio
    label.max() / (fake.max() + 1e-6): wherever a rescale ratio applies the means move by ~1e-6 / max_height relative, far outside 1e-12,
    so G15 tells the two apart; and where the coronal script raises, the sagittal arithmetic returns numbers."""
    from oracle import restate as R
    g, names = _cases()
    worst = 0.0
    for n in names:
        idx, div, thr = (float(v) for v in g[n + '/params'][:3])
        got, means = R.rhlv_volume(g[n + '/fake'].transpose(0, 2, 1), g[n + '/label'].transpose(0, 2, 1), idx, int(div), thr)
        if g[n + '/raises']:
            assert np.all(np.isfinite(got))
            continue
        ref = np.concatenate([g[n + '/out'], g[n + '/means']])
        worst = max(worst, float(np.max(np.abs(np.concatenate([got, means]) - ref) / np.maximum(1.0, np.abs(ref)))))
    assert worst > 1e-10, worst
