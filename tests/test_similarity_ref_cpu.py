"""tests/similarity_ref.py pinned on the host: the joint histogram against a triple loop and np.histogram2d, the sampled values against scipy,
the count invariants, the entropies' identities, and the restated pattern search on the synthetic case the device test repeats.  No device."""
import numpy as np
import pytest
from scipy import ndimage

import resample_ref as R
import similarity_ref as S

IDENTITY = (np.eye(3), np.zeros(3))
POSE = (R.MATRIX, R.OFFSET)
FAR = (np.eye(3), np.array([100.0, 0.0, 0.0]))
LEVELS = dict(flo=-300.0, fwidth=75.0, Gf=8, mlo=-250.0, mwidth=100.0, Gm=5)


def _pair(fdt=np.float32, mdt=np.float32):
    fixed = R.case_volume(fdt, (5, 4, 6), seed=3)
    moving = R.case_volume(mdt, (4, 6, 5), seed=4)
    if np.dtype(fdt) == np.int16:
        fixed = (fixed // 100).astype(np.int16)
    if np.dtype(mdt) == np.int16:
        moving = (moving // 100).astype(np.int16)
    return fixed, moving


@pytest.mark.parametrize('order', (0, 1, 3))
def test_restatement_equals_the_triple_loop(order):
    for fdt, mdt in ((np.float32, np.float64), (np.int16, np.uint8)):
        fixed, moving = _pair(fdt, mdt)
        mask = (np.random.RandomState(1).random_sample(fixed.shape) > 0.2).astype(np.uint8)
        if fdt == np.float32:
            fixed = fixed.copy()
            fixed[1, 2, 3], fixed[0, 0, 0] = np.nan, np.inf
        if mdt == np.float64 and order < 3:
            moving = moving.copy()
            moving[2, 3, 2] = np.nan
        kw = dict(LEVELS, mlo=0.0, mwidth=40.0) if mdt == np.uint8 else LEVELS
        poses = [IDENTITY, POSE, FAR]
        for mk in (None, mask):
            out, info = S.joint_hist_ref(fixed, moving, poses, order, mask=mk, **kw)
            assert np.array_equal(out, S.joint_hist_brute(fixed, moving, poses, order, mask=mk, **kw))
            assert (info[:, 1:5].sum(axis=1) == fixed.size).all() and (out.sum(axis=(1, 2)) == info[:, 1]).all()
            assert info[2, 1] == 0 and info[2, 0] & S.EMPTY and not out[2].any()
            assert (info[:, 2] == (0 if mk is None else int((mk == 0).sum()))).all()
            assert (info[:, 5] + info[:, 6] <= info[:, 1]).all() and (info[:, 7] <= info[:, 1]).all()
            if fdt == np.float32:
                assert (info[:, 0] & S.NONFINITE).all() and (info[:, 3] >= 1).all()


def test_identity_order_0_is_histogram2d():
    r = np.random.RandomState(2)
    fixed = r.randint(-40, 120, size=(6, 5, 7)).astype(np.int16)
    moving = r.randint(-40, 120, size=(6, 5, 7)).astype(np.int16)
    out, info = S.joint_hist_ref(fixed, moving, [IDENTITY], 0, flo=-40.0, fwidth=20.0, Gf=8, mlo=-40.0, mwidth=10.0, Gm=16)
    want, _, _ = np.histogram2d(fixed.ravel(), moving.ravel(), bins=(np.arange(-40.0, 121.0, 20.0), np.arange(-40.0, 121.0, 10.0)))
    assert np.array_equal(out[0], want.astype(np.int64)) and info[0, 1] == fixed.size and not info[0, 5:].any()


@pytest.mark.parametrize('order', (0, 1, 3))
@pytest.mark.parametrize('dtype', R.DTYPES, ids=lambda d: np.dtype(d).name)
def test_sampled_values_are_scipys(order, dtype):
    """The y that is binned: scipy's affine_transform into float64, bit for bit -- at order 3 on scipy's own coefficients."""
    moving = R.case_volume(dtype)
    shape = (9, 7, 11)
    coef = ndimage.spline_filter(moving, 3, output=np.float64, mode='mirror') if order == 3 else None
    y, inside = S.sampled(moving, shape, R.MATRIX, R.OFFSET, order, coef)
    src = coef if order == 3 else moving
    want = ndimage.affine_transform(src, R.MATRIX, R.OFFSET, output_shape=shape, output=np.float64, order=order, mode='constant', cval=0.0,
                                    prefilter=False)
    assert 0 < inside.sum() < inside.size
    assert y.tobytes() == want.ravel().tobytes()


def test_entropy_identities():
    fixed, _ = _pair()
    out, _ = S.joint_hist_ref(fixed, fixed, [IDENTITY], 0, **dict(LEVELS, mlo=LEVELS['flo'], mwidth=LEVELS['fwidth'], Gm=LEVELS['Gf']))
    hf, hm, hfm = S.entropies(out)
    assert not (out[0] - np.diag(np.diag(out[0]))).any()              # a volume with itself: the diagonal
    assert hf[0] == hm[0] == hfm[0] and hf[0] > 0
    assert S.mutual_information(out)[0] == hf[0]                      # MI of a volume with itself is its entropy
    assert S.normalized_mutual_information(out)[0] == 2.0 and S.entropy_correlation(out)[0] == 1.0
    _, moving = _pair()
    h, _ = S.joint_hist_ref(fixed, moving, [IDENTITY, POSE], 1, **LEVELS)
    ht = np.ascontiguousarray(h.transpose(0, 2, 1))
    assert np.allclose(S.mutual_information(h), S.mutual_information(ht), rtol=0, atol=1e-14)
    assert (S.mutual_information(h) >= -1e-14).all()
    p = h[0] / h[0].sum()
    direct = sum(p[i, j] * np.log(p[i, j] / (p[i].sum() * p[:, j].sum())) for i in range(p.shape[0]) for j in range(p.shape[1]) if p[i, j] > 0)
    assert abs(S.mutual_information(h)[0] - direct) < 1e-13
    empty = np.zeros((1, 4, 4), dtype=np.int64)
    for fn in S.METRIC.values():
        assert np.isnan(fn(empty)).all()
    one_bin = np.zeros((1, 4, 4), dtype=np.int64)
    one_bin[0, 1, 2] = 50
    assert S.mutual_information(one_bin)[0] == 0.0 and np.isnan(S.normalized_mutual_information(one_bin)[0])


def test_rigid_pose():
    shape_f, shape_m = (24, 28, 20), (22, 30, 18)
    m, off = S.rigid_pose(np.zeros(6), shape_f, shape_m)
    cf, cm = (np.array(shape_f) - 1) / 2.0, (np.array(shape_m) - 1) / 2.0
    assert np.array_equal(m, np.eye(3)) and np.array_equal(off, cm - cf)          # centre on centre
    rot = S.rotation_matrix((10.0, -20.0, 30.0))
    assert np.abs(rot @ rot.T - np.eye(3)).max() < 1e-15 and abs(np.linalg.det(rot) - 1.0) < 1e-15
    q = S.rotation_matrix((90.0, 0.0, 0.0))                                       # about axis 0: axis 1 turns onto axis 2
    assert np.allclose(q @ np.array([0.0, 1.0, 0.0]), [0.0, 0.0, 1.0], atol=1e-15)
    # the two branches agree where both apply: isotropic 2 mm through the general formula
    p = np.array([3.0, -2.0, 1.5, 1.5, -1.0, 2.0])
    m1, o1 = S.rigid_pose(p, shape_f, shape_m, (2.0, 2.0, 2.0), (2.0, 2.0, 2.0))
    mr, offr = S.rigid_matrix(S.rotation_matrix(p[:3]), np.zeros(3), 2.0 * cf + p[3:])
    assert np.allclose(m1, mr, atol=1e-15) and np.allclose(o1, offr / 2.0 + cm, atol=1e-12)
    # millimetres: the fixed centre reads the moving point R^T (0 - t) from the moving centre
    sf, sm = np.array([1.0, 1.0, 1.5]), np.array([0.7, 0.7, 2.0])
    m2, o2 = S.rigid_pose(p, shape_f, shape_m, sf, sm)
    assert np.allclose((m2 @ cf + o2 - cm) * sm, S.rotation_matrix(p[:3]).T @ (-p[3:]), atol=1e-12)
    x = np.array([3.0, 5.0, 7.0])
    assert np.allclose((m2 @ x + o2 - cm) * sm, S.rotation_matrix(p[:3]).T @ ((x - cf) * sf - p[3:]), atol=1e-12)


def test_pattern_search_improves_the_synthetic_case():
    """Conditions, not tolerances: the final score strictly above the starting one, and the corners nearer the true pose than at the start."""
    params, matrix, offset, score, history, calls = S.registration_ref()
    assert calls == len(history) and history[0][1] == (0.0,) * 6
    assert score > history[0][2]
    levels = [h[0] for h in history]
    assert levels == sorted(levels) and set(levels) == {0, 1, 2}
    assert all(b[2] > a[2] for a, b in zip(history, history[1:]) if a[0] == b[0])            # within a level every call follows a move upwards
    true = S.rigid_pose(S.REG_TRUE, S.REG_SHAPE, S.REG_SHAPE, S.REG_SPACING, S.REG_SPACING)
    start = S.rigid_pose(np.zeros(6), S.REG_SHAPE, S.REG_SHAPE, S.REG_SPACING, S.REG_SPACING)
    assert S.corner_error(S.REG_SHAPE, (matrix, offset), true) < S.corner_error(S.REG_SHAPE, start, true)
    # max_moves ends the search: one move, then the call that scores where it stands
    fixed, moving = S.registration_case()
    p1 = S.register_rigid(fixed, moving, S.REG_SPACING, S.REG_SPACING, max_moves=1, **S.REG_KW)
    assert p1[5] == 2 and p1[4][1][1] == history[1][1] and p1[3] == history[1][2]
