"""tests/labelstats_ref.py pinned on the host against scipy.ndimage (sum_labels / mean / variance / minimum / maximum / center_of_mass /
find_objects) and np.percentile, and the host half of healthivert-gan_amd/label_statistics.py (numpy's lerp, the variance from the integer sums,
empty slots) fed with the restatement's records, without a device.

Counts, integer sums, minima, maxima, boxes, coordinate sums and percentiles are compared bit for bit.  Mean and variance: the largest relative
difference |restatement - scipy| over the cases MEASURED 2.78e-16 for the mean and 3.15e-16 for the variance (the variance in units of
E[v^2] = variance + mean^2, see _rel_var; scipy sums sequentially in float64, the restatement is exactly rounded), so STATS_TOL =
max(10 x 3.15e-16, 1e-12) = 1e-12.  test_stats_tol_basis prints the figures and holds ten times the larger below STATS_TOL."""
import warnings

import numpy as np
import pytest

import labelstats_ref as LR

STATS_TOL = 1e-12
DTYPES = (np.uint8, np.int16, np.float32, np.float64)


def _case(dtype, masked=False):
    vol, lab = LR.intensities(dtype), LR.base_label()
    mask = None
    if masked:
        mask = np.ones(LR.SHAPE, dtype=np.uint8)
        mask[:, :, ::3] = 0
        mask[31, 0, 0] = 0                      # empties label 2
    return vol, lab, mask


def _rel(a, b):
    return abs(a - b) / max(abs(b), np.finfo(np.float64).tiny)


def _rel_var(var, ref_var, ref_mean):
    """A variance derived from sum v and sum v^2 carries THEIR rounding, which is relative to the mean square, not to the variance (label 3 holds
    two values one ulp apart: a variance of 6e-27 beside a mean square of 2.7e5): the difference in units of variance + mean^2 = E[v^2]."""
    return abs(var - ref_var) / max(ref_var + ref_mean * ref_mean, np.finfo(np.float64).tiny)


@pytest.mark.parametrize('masked', (False, True))
@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
def test_restatement_against_scipy(dtype, masked):
    vol, lab, mask = _case(dtype, masked)
    labels = (0,) + LR.LABELS
    rec = LR.label_stats_ref(vol, lab, labels, LR.QS, mask)
    raw = rec.view(np.int64)
    ref = LR.scipy_chain(vol, lab, labels, LR.QS, mask)
    integer = np.dtype(dtype).kind in 'iu'
    mv = LR.mean_variance(rec, integer)
    for s, l in enumerate(labels):
        n = ref['count'][s]
        assert rec[s, LR.COUNT] == n, l
        if n == 0:
            assert l in (9, 2) and int(rec[s, LR.STATUS]) == LR.EMPTY and ref['box'][s] is None
            assert tuple(rec[s, LR.LO:LR.LO + 3]) == LR.SHAPE and tuple(rec[s, LR.HI:LR.HI + 3]) == (-1, -1, -1)
            assert np.isnan(rec[s, LR.ORDER:LR.ORDER + 2 * len(LR.QS)]).all() and np.isnan(mv[s]).all()
            continue
        assert int(rec[s, LR.STATUS]) == 0
        if integer:
            assert int(raw[s, LR.SUM]) == int(ref['sum'][s]) and abs(int(raw[s, LR.SUM])) < 2 ** 53
        else:
            assert _rel(rec[s, LR.SUM], float(ref['sum'][s])) <= STATS_TOL
        assert rec[s, LR.MIN] == np.float64(ref['min'][s]) and rec[s, LR.MAX] == np.float64(ref['max'][s])
        assert tuple(rec[s, LR.COORD:LR.COORD + 3] / n) == tuple(np.float64(c) for c in ref['centroid'][s])
        box = ref['box'][s]
        assert tuple(slice(int(a), int(b) + 1) for a, b in zip(rec[s, LR.LO:LR.LO + 3], rec[s, LR.HI:LR.HI + 3])) == box
        for t, p in enumerate(LR.QS):
            lo, hi, vi = LR.order_ranks(n, p)
            a, b, tt = rec[s, LR.ORDER + 2 * t], rec[s, LR.ORDER + 2 * t + 1], vi - np.floor(vi)
            got = b - (b - a) * (1 - tt) if tt >= 0.5 else a + (b - a) * tt
            assert LR.same_value(got, ref['percentiles'][s][t]), (l, p)
        assert _rel(mv[s, 0], ref['mean'][s]) <= STATS_TOL and _rel_var(mv[s, 1], ref['variance'][s], ref['mean'][s]) <= STATS_TOL
        if dtype == np.int16:
            assert np.float64(mv[s, 0]).tobytes() == np.float64(ref['mean'][s]).tobytes(), 'int16 mean below 2^53: bit for bit'


def test_stats_tol_basis(capsys):
    worst = {'mean': 0.0, 'variance': 0.0}
    for dtype in DTYPES:
        for masked in (False, True):
            vol, lab, mask = _case(dtype, masked)
            rec = LR.label_stats_ref(vol, lab, LR.LABELS, (), mask)
            mv = LR.mean_variance(rec, np.dtype(dtype).kind in 'iu')
            ref = LR.scipy_chain(vol, lab, LR.LABELS, (), mask)
            for s in range(len(LR.LABELS)):
                if ref['count'][s]:
                    worst['mean'] = max(worst['mean'], _rel(mv[s, 0], ref['mean'][s]))
                    worst['variance'] = max(worst['variance'], _rel_var(mv[s, 1], ref['variance'][s], ref['mean'][s]))
    with capsys.disabled():
        print('\nlargest relative |restatement - scipy|: mean %.3g, variance %.3g; STATS_TOL %.1g' % (worst['mean'], worst['variance'], STATS_TOL))
    assert 10 * max(worst.values()) <= STATS_TOL


def test_sort_key_orders_like_the_values():
    for dtype in (np.float32, np.float64):
        x = np.array([-np.inf, -3.5, -np.finfo(dtype).smallest_subnormal, -0.0, 0.0, np.finfo(dtype).smallest_subnormal, 1.0,
                      np.nextafter(dtype(1.0), dtype(2.0)), np.inf], dtype=dtype)
        k = LR.sort_key(x)
        assert (np.diff(k.astype(object)) > 0).all()
    k = LR.sort_key(np.array([-32768, -1, 0, 32767], dtype=np.int16))
    assert list(k) == [0, 32767, 32768, 65535]


def test_invalid_labels_are_flagged_and_counted_nowhere():
    lab = LR.base_label().astype(np.float64)
    lab[0, 0, 0], lab[0, 0, 1], lab[0, 0, 2] = 2.5, 300.0, np.nan
    rec = LR.label_stats_ref(LR.intensities(np.float32), lab, (0, 1), ())
    assert (rec[:, LR.STATUS] == LR.BAD_LABEL).all()
    assert rec[0, LR.COUNT] == (LR.base_label() == 0).sum() - 3


# ------------------------------------------------------------------------------------------------ the wrapper's host half
def _S():
    import hvgan  # noqa: F401
    from hvgan import label_statistics
    return label_statistics


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
def test_host_half_from_records(dtype):
    S = _S()
    assert (S.REC, S.COUNT, S.SUM, S.SUMSQ, S.MIN, S.MAX, S.COORD, S.LO, S.HI, S.STATUS, S.ORDER) == (
        LR.REC, LR.COUNT, LR.SUM, LR.SUMSQ, LR.MIN, LR.MAX, LR.COORD, LR.LO, LR.HI, LR.STATUS, LR.ORDER)
    vol, lab, mask = _case(dtype, True)
    sp = (0.7, 0.7, 1.5)
    rec = LR.label_stats_ref(vol, lab, LR.LABELS, LR.QS, mask)
    integer = np.dtype(dtype).kind in 'iu'
    with warnings.catch_warnings():
        warnings.simplefilter('error')          # an empty slot gives NaN without a warning
        res = S.stats_from_records(rec[None], integer, LR.LABELS, LR.QS, LR.SHAPE, sp)
    ref = LR.scipy_chain(vol, lab, LR.LABELS, LR.QS, mask)
    for s, l in enumerate(LR.LABELS):
        n = ref['count'][s]
        assert res['count'][0, s] == n
        assert res['volume_mm3'][0, s] == n * float(np.prod(np.asarray(sp)))
        if n == 0:
            for k in ('sum', 'mean', 'variance', 'std', 'min', 'max'):
                assert np.isnan(res[k][0, s]), k
            assert np.isnan(res['centroid'][0, s]).all() and np.isnan(res['percentiles'][0, s]).all()
            assert res['box_slices'][0][s] is None and res['unusable'][0][s] and res['status'][0, s] == LR.EMPTY
            assert tuple(res['box'][0, s, 0]) == LR.SHAPE and tuple(res['box'][0, s, 1]) == (-1, -1, -1)
            continue
        assert res['unusable'][0][s] is None
        assert res['box_slices'][0][s] == ref['box'][s]
        assert tuple(res['centroid'][0, s]) == tuple(np.float64(c) for c in ref['centroid'][s])
        assert np.array_equal(res['centroid_mm'][0, s], res['centroid'][0, s] * np.asarray(sp))
        assert res['min'][0, s] == ref['min'][s] and res['max'][0, s] == ref['max'][s]
        for t in range(len(LR.QS)):
            assert LR.same_value(res['percentiles'][0, s, t], ref['percentiles'][s][t]), (l, LR.QS[t])
        assert _rel(res['mean'][0, s], ref['mean'][s]) <= STATS_TOL and _rel_var(res['variance'][0, s], ref['variance'][s], ref['mean'][s]) <= STATS_TOL
        assert res['std'][0, s] == np.sqrt(res['variance'][0, s])
        if integer:
            assert res['sum'][0, s] == float(ref['sum'][s])
            assert np.float64(res['mean'][0, s]).tobytes() == np.float64(ref['mean'][s]).tobytes()


def test_host_half_reports_a_non_finite_slot_as_nan():
    S = _S()
    vol, lab, _ = _case(np.float64)
    vol[31, 4, 7] = np.nan
    rec = LR.label_stats_ref(vol, lab, (4, 5), (50.0,))
    res = S.stats_from_records(rec[None], False, (4, 5), (50.0,), LR.SHAPE)
    assert res['status'][0, 0] == LR.NONFINITE and 'NaN' in res['unusable'][0][0] and res['count'][0, 0] == 63
    for k in ('sum', 'mean', 'variance', 'std', 'min', 'max'):
        assert np.isnan(res[k][0, 0])
    assert np.isnan(res['percentiles'][0, 0]).all() and not np.isnan(res['centroid'][0, 0]).any()
    assert res['unusable'][0][1] is None and np.isfinite(res['mean'][0, 1])


def test_lerp_takes_numpys_upper_branch():
    S = _S()
    g = np.random.default_rng(3)
    for n in (2, 3, 7, 65, 1000):
        x = np.sort(g.standard_normal(n) * 1e3)
        for q in (0, 100, 50, 5, 95, 33.3, 66.7, 99.9):
            lo, hi, _ = LR.order_ranks(n, q)
            assert np.float64(S.percentile_from_order(n, q, x[lo], x[hi])).tobytes() == np.float64(np.percentile(x, q)).tobytes(), (n, q)
