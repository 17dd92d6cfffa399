"""tests/texture_runs_ref.py pinned on the host against loop-form brute forces and the worked examples of the pyradiomics documentation, and the host
half of healthivert-gan_amd/texture_runs.py: the feature functions against loop forms written independently, closed forms, and the argument checks
that need no device."""
import numpy as np
import pytest

import texture_runs_ref as RR

D13 = RR.directions13()


def _R():
    import hvgan  # noqa: F401
    from hvgan import texture_runs
    return texture_runs


def _random_case(seed, shape):
    """Two labels and background, a mask, a NaN inside label 1; few levels, so runs longer than one and dependent neighbours exist."""
    g = np.random.default_rng(seed)
    vol = g.integers(-10, 50, shape).astype(np.float32)            # below lo and above lo + G * width: both clamps
    lab = g.integers(0, 3, shape).astype(np.uint8)
    mask = (g.random(shape) > 0.15).astype(np.uint8)
    p = tuple(n // 2 for n in shape)
    vol[p], lab[p], mask[p] = np.nan, 1, 1
    return vol, lab, mask


@pytest.mark.parametrize('seed,shape', ((0, (6, 7, 8)), (1, (3, 1, 5)), (2, (1, 4, 1))))
def test_references_equal_the_brute_forces(seed, shape):
    vol, lab, mask = _random_case(seed, shape)
    for m in (None, mask):
        for R in (2, 8):
            out, info = RR.glrlm_ref(vol, lab, (1, 2), D13, 0.0, 10.0, 4, R, m)
            want, capped = RR.glrlm_brute(vol, lab, (1, 2), D13, 0.0, 10.0, 4, R, m)
            assert out.tobytes() == want.tobytes() and (info[:, RR.INFO:] == capped).all() and out.sum() > 0, (m is not None, R)
            assert (info[:, 0] & RR.NONFINITE)[0] and not (info[:, 0] & RR.NONFINITE)[1]
            if shape == (6, 7, 8):
                assert capped.sum() > 0 if R == 2 else capped.sum() == 0
        for alpha in (0, 1, 3):
            dep, ngt, info = RR.gldm_ref(vol, lab, (1, 2), 0.0, 10.0, 4, alpha, m)
            b_dep, b_ngt = RR.gldm_brute(vol, lab, (1, 2), 0.0, 10.0, 4, alpha, m)
            assert dep.tobytes() == b_dep.tobytes() and ngt.tobytes() == b_ngt.tobytes(), (m is not None, alpha)
            assert (dep.sum(axis=(1, 2)) == info[:, 1]).all() and (ngt[..., 0].sum(axis=-1) == dep.sum(axis=-1)).all()


def test_the_documented_examples():
    vol = RR.RUN_IMAGE[None]                                        # 1 x 5 x 5: the row's direction is axis 2
    lab = np.ones(vol.shape, np.uint8)
    out, info = RR.glrlm_ref(vol, lab, (1,), [(0, 0, 1)], 1.0, 1.0, 5, 5)
    assert (out[0, 0] == RR.RUN_GLRLM).all() and tuple(info[0]) == (0, 25, 0, 0) + (0,) * 13
    assert (RR.glrlm_brute(vol, lab, (1,), [(0, 0, 1)], 1.0, 1.0, 5, 5)[0][0, 0] == RR.RUN_GLRLM).all()
    dep, _, _ = RR.gldm_ref(vol, lab, (1,), 1.0, 1.0, 5, 0)
    assert (dep[0, :, :4] == RR.RUN_GLDM).all() and not dep[0, :, 4:].any()
    vol = RR.NGTDM_IMAGE[None]
    lab = np.ones(vol.shape, np.uint8)
    _, ngt, _ = RR.gldm_ref(vol, lab, (1,), 1.0, 1.0, 5, 0)
    n, s = RR.ngtdm_table_loop(ngt[0])
    assert n == RR.NGTDM_N.tolist() and np.abs(np.array(s) - RR.NGTDM_S).max() <= 1e-12
    tn, ts = _R().ngtdm_table(ngt)
    assert (tn[0] == RR.NGTDM_N).all() and np.abs(ts[0] - RR.NGTDM_S).max() <= 1e-12


def _close(got, want, what):
    assert np.isfinite(want) and abs(got - want) <= 1e-12 * abs(want), (what, got, want)


def test_feature_functions_equal_the_loop_forms():
    R = _R()
    vol, lab, _ = _random_case(5, (6, 7, 8))
    rlm, _ = RR.glrlm_ref(vol, lab, (1, 2), D13, 0.0, 10.0, 4, 8)
    cases = [rlm, np.stack([RR.RUN_GLRLM])[None]]
    for P in cases:
        f = R.glrlm_features(P)
        for s in range(P.shape[0]):
            loops = [RR.glrlm_features_loop(P[s, d]) for d in range(P.shape[1])]
            for k in R.GLRLM_FEATURES + ('mean_run',):
                assert f[k].shape == P.shape[:2]
                for d, want in enumerate(loops):
                    _close(f[k][s, d], want[k], (k, s, d))
            for k in R.GLRLM_FEATURES:
                _close(f['mean'][k][s], sum(w[k] for w in loops) / len(loops), ('mean', k, s))
    dep, ngt, _ = RR.gldm_ref(vol, lab, (1, 2), 0.0, 10.0, 4, 1)
    ex_dep = np.zeros((1, 5, RR.NB), np.int64)
    ex_dep[0, :, :4] = RR.RUN_GLDM
    for P in (dep, ex_dep):
        f = R.gldm_features(P)
        assert sorted(f) == sorted(R.GLDM_FEATURES) and len(f) == 14
        for s in range(P.shape[0]):
            want = RR.gldm_features_loop(P[s])
            for k in R.GLDM_FEATURES:
                _close(f[k][s], want[k], (k, s))
    ex_ngt = RR.gldm_ref(RR.NGTDM_IMAGE[None], np.ones((1, 4, 4), np.uint8), (1,), 1.0, 1.0, 5, 0)[1]
    for T in (ngt, ex_ngt):
        f = R.ngtdm_features(T)
        for s in range(T.shape[0]):
            want = RR.ngtdm_features_loop(T[s])
            for k in R.NGTDM_FEATURES:
                _close(f[k][s], want[k], (k, s))
    # the documented NGTDM example by hand: Nvp = 16, sum p_i s_i = (6 * 13.35 + 2 * 2 + 4 * 91 / 30 + 4 * 10.075) / 16
    _close(R.ngtdm_features(ex_ngt)['coarseness'][0], 16.0 / (6 * 13.35 + 4.0 + 4 * 91.0 / 30.0 + 4 * 10.075), 'coarseness')


def test_closed_forms_and_empty_matrices():
    R = _R()
    one = np.zeros((1, 4, 6), np.int64)
    one[0, 1, 2] = 7                                                # seven runs of level 2 (i = 2) and length 3
    f = R.glrlm_features(one)
    want = dict(SRE=1 / 9, LRE=9, GLN=7, GLNN=1, RLN=7, RLNN=1, RP=1 / 3, mean_run=3, GLV=0, RV=0, RE=0, LGLRE=0.25, HGLRE=4, SRLGLE=1 / 36,
                SRHGLE=4 / 9, LRLGLE=2.25, LRHGLE=36)
    assert sorted(want) == sorted(R.GLRLM_FEATURES + ('mean_run',)) and len(R.GLRLM_FEATURES) == 16
    for k, x in want.items():                                      # 7 * w / 7: a product and a quotient, two roundings at most
        assert abs(f[k][0] - x) <= 4 * np.finfo(np.float64).eps * abs(x), (k, f[k][0], x)
    empty = R.glrlm_features(np.zeros((2, 3, 4, 5), np.int64))
    assert all(np.isnan(empty[k]).all() and empty[k].shape == (2, 3) for k in R.GLRLM_FEATURES + ('mean_run',))
    assert all(np.isnan(empty['mean'][k]).all() and empty['mean'][k].shape == (2,) for k in R.GLRLM_FEATURES)
    assert all(np.isnan(v).all() for v in R.gldm_features(np.zeros((2, 4, 27), np.int64)).values())
    lonely = np.zeros((3, 27, 2), np.int64)
    lonely[1, 0, 0] = 5                                             # voxels without a neighbour are left out of NGTDM
    assert all(np.isnan(v) for v in R.ngtdm_features(lonely).values())
    flat = np.zeros((3, 27, 2), np.int64)
    flat[1, 26, 0] = 9                                              # one level, every voxel equal to its neighbours' mean
    f = R.ngtdm_features(flat)
    assert f['coarseness'] == 1e6 and f['contrast'] == 0 and f['busyness'] == 0 and f['complexity'] == 0 and f['strength'] == 0
    m = np.arange(1.0, 14.0)
    rows = D13
    assert R.run_anisotropy(m, 2) == m[rows.index((0, 0, 1))] / ((m[rows.index((1, 0, 0))] + m[rows.index((0, 1, 0))]) / 2)
    assert R.run_anisotropy(m, 0) == m[rows.index((1, 0, 0))] / ((m[rows.index((0, 1, 0))] + m[rows.index((0, 0, 1))]) / 2)


def test_misuse_raises_before_any_device_work():
    R = _R()
    vol, lab = np.zeros((4, 4, 4), np.int16), np.ones((4, 4, 4), np.uint8)
    for kw in (dict(levels=1), dict(levels=65), dict(width=0.0), dict(lo=float('nan')), dict(offsets=[(0, 0, 2)]), dict(offsets=[(0, 0, 0)]),
               dict(offsets=[(0, 0, 1), (0, 0, 1)]), dict(offsets=[(0, 1, 1), (0, -1, -1)]), dict(offsets=[(0, 1)]), dict(offsets=[]),
               dict(offsets=D13 + [(0, 0, -1)]), dict(max_run=0), dict(max_run=2.0), dict(max_run=True)):
        with pytest.raises(ValueError):
            R.glrlm(vol, lab, (1,), **kw)
    for kw in (dict(alpha=-1), dict(alpha=32), dict(alpha=8, levels=8), dict(alpha=1.0), dict(levels=1)):
        with pytest.raises(ValueError):
            R.gldm(vol, lab, (1,), **kw)
    with pytest.raises(ValueError):
        R.vertebra_run_texture(vol, lab, 1, slice_axis=3)
    with pytest.raises(ValueError):
        R.vertebra_run_texture(vol, lab, 300)
    with pytest.raises(ValueError):
        R.run_texture_comparison(vol, vol, lab, lab, 1, neighbours=(1,))
    for fn, bad in ((R.glrlm_features, np.zeros((4, 4))), (R.gldm_features, np.zeros(4)), (R.ngtdm_features, np.zeros((4, 27, 3))),
                    (R.glrlm_features, np.zeros((2, 4, 4), dtype='U1'))):
        with pytest.raises(ValueError):
            fn(bad)
