"""tests/texture_ref.py pinned on the host against a triple-loop brute force and Haralick's 4 x 4 example, and the host half of
healthivert-gan_amd/texture.py: haralick_features' closed forms, directions(), and the argument checks that need no device."""
import numpy as np
import pytest

import texture_ref as TR


def _T():
    import hvgan  # noqa: F401
    from hvgan import texture
    return texture


def test_reference_equals_the_brute_force():
    """5 x 4 x 3, two labels and background, a mask, offsets with negative components and the zero offset; asymmetric and symmetric."""
    g = np.random.default_rng(3)
    shape = (5, 4, 3)
    vol = g.integers(-30, 130, shape).astype(np.int16)             # below lo and above lo + G * width: both clamps
    lab = g.integers(0, 3, shape).astype(np.uint8)
    mask = (g.random(shape) > 0.2).astype(np.uint8)
    offsets = [(0, 0, 1), (1, -1, 0), (-1, 2, -1), (0, 0, 0), (2, 0, -2), (-4, 0, 0)]
    for symmetric in (False, True):
        for m in (None, mask):
            out, info = TR.glcm_ref(vol, lab, (1, 2), offsets, 0.0, 12.5, 8, symmetric, m)
            want = TR.glcm_brute(vol, lab, (1, 2), offsets, 0.0, 12.5, 8, symmetric, m.astype(bool) if m is not None else None)
            assert out.tobytes() == want.tobytes(), (symmetric, m is not None)
            assert out.sum() > 0
            keep = np.ones(shape, bool) if m is None else m != 0
            for s, l in enumerate((1, 2)):
                sel = (lab == l) & keep
                assert info[s, 1] == sel.sum() and info[s, 2] == (vol[sel] < 0).sum() and info[s, 3] == (vol[sel] >= 100).sum()
                assert np.trace(out[s, 3]) == sel.sum() * (2 if symmetric else 1)


def test_haralicks_example():
    vol = TR.HARALICK_IMAGE[:, :, None]                             # 4 x 4 x 1: rows along axis 0, the row's direction is axis 1
    out, info = TR.glcm_ref(vol, np.ones(vol.shape, np.uint8), (1,), [(0, 1, 0)], 0.0, 1.0, 4, True)
    assert (out[0, 0] == TR.HARALICK_GLCM).all() and tuple(info[0]) == (0, 16, 0, 0)
    asym, _ = TR.glcm_ref(vol, np.ones(vol.shape, np.uint8), (1,), [(0, 1, 0)], 0.0, 1.0, 4, False)
    assert (asym[0, 0] + asym[0, 0].T == TR.HARALICK_GLCM).all()


def test_haralick_features_closed_forms():
    T = _T()
    one = np.zeros((1, 4, 4), dtype=np.int64)
    one[0, 2, 2] = 17
    f = T.haralick_features(one)
    assert f['contrast'][0] == 0 and f['dissimilarity'][0] == 0 and f['homogeneity'][0] == 1 and f['asm'][0] == 1 and f['energy'][0] == 1
    assert f['entropy'][0] == 0 and f['correlation'][0] == 1 and f['max_probability'][0] == 1
    board = np.array([[[0, 9], [9, 0]]], dtype=np.int64)
    f = T.haralick_features(board)
    assert f['contrast'][0] == 1 and f['dissimilarity'][0] == 1 and f['homogeneity'][0] == 0.5 and f['asm'][0] == 0.5
    assert f['entropy'][0] == 1 and f['correlation'][0] == -1 and f['max_probability'][0] == 0.5 and f['energy'][0] == np.sqrt(0.5)
    both = T.haralick_features(np.stack([np.array([[5, 0], [0, 0]]), board[0]]))
    assert both['contrast'].shape == (2,) and both['mean']['contrast'] == 0.5 and both['mean']['correlation'] == 0.0
    empty = T.haralick_features(np.zeros((2, 3, 4, 4), dtype=np.int64))
    assert empty['entropy'].shape == (2, 3) and all(np.isnan(empty[k]).all() and np.isnan(empty['mean'][k]).all() for k in T.FEATURES)
    # Haralick's example by hand: p = P / 24
    f = T.haralick_features(TR.HARALICK_GLCM[None])
    assert abs(f['contrast'][0] - 14 / 24) <= 1e-15 and abs(f['asm'][0] - 84 / 576) <= 1e-15
    assert abs(f['homogeneity'][0] - (16 + 6 * 0.5 + 2 * 0.2) / 24) <= 1e-15


def test_directions():
    T = _T()
    d = T.directions()
    assert d.shape == (13, 3) and d.dtype == np.int64 and [tuple(x) for x in d] == TR.directions13()
    seen = set(map(tuple, d.tolist()))
    assert len(seen) == 13 and (0, 0, 0) not in seen and all(tuple(-c for c in x) not in seen for x in seen)
    assert (T.directions(3) == 3 * d).all()
    two = T.directions([1, 4])
    assert two.shape == (26, 3) and (two[:13] == d).all() and (two[13:] == 4 * d).all()


def test_misuse_raises_before_any_device_work():
    T = _T()
    vol, lab = np.zeros((4, 4, 4), np.int16), np.ones((4, 4, 4), np.uint8)
    for bad in (0, 5, -1, 1.5, True, [1, 1], [1, 2, 3], []):
        with pytest.raises(ValueError):
            T.directions(bad)
    for kw in (dict(levels=1), dict(levels=65), dict(levels=8.0), dict(width=0.0), dict(width=-1.0), dict(width=float('inf')),
               dict(lo=float('nan')), dict(lo='x'), dict(offsets=[(0, 0, 5)]), dict(offsets=[(0, 0, 1), (0, 0, 1)]), dict(offsets=[(0, 1)]),
               dict(offsets=[(0, 0, 0.5)]), dict(offsets=[]), dict(offsets=[(0, 0, 1)] * 27)):
        with pytest.raises(ValueError):
            T.glcm(vol, lab, (1,), **kw)
    with pytest.raises(ValueError):
        T.vertebra_texture(vol, lab, 1, erode_mm=-1.0)
    with pytest.raises(ValueError):
        T.vertebra_texture(vol, lab, 300)
    with pytest.raises(ValueError):
        T.texture_comparison(vol, vol, lab, lab, 1, neighbours=(1,))
    with pytest.raises(ValueError):
        T.texture_comparison(vol, vol, lab, lab, 1, spacing=(1, 0, 1))
    for bad in (np.zeros((4, 4)), np.zeros((2, 3, 4)), np.zeros((4, 4), dtype='U1')):
        with pytest.raises(ValueError):
            T.haralick_features(bad)
