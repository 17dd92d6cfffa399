"""tests/filter_ref.py -- the numpy restatement the device filters are compared with -- against scipy.ndimage, bit for bit: the boundary maps,
the three summation forms and their detection, the Gaussian weights, and smooth_label's rules.  No GPU."""
import numpy as np
import pytest
from scipy import ndimage

import filter_ref as FR


@pytest.mark.parametrize('shape', FR.SHAPES)
@pytest.mark.parametrize('dtype', FR.DTYPES)
def test_gaussian_filter_restatement_equals_scipy(shape, dtype):
    a = FR.volume(shape, dtype).astype(np.float64)            # the definition: scipy on the float64 copy
    for mode in FR.MODES:
        for sigma, order in FR.SIGMA_ORDER:
            want = ndimage.gaussian_filter(a, sigma, order=order, mode=mode, cval=FR.CVAL)
            got = FR.gaussian_filter(FR.volume(shape, dtype), sigma, order=order, mode=mode, cval=FR.CVAL)
            assert FR.same(got, want), (mode, sigma, order, float(np.abs(got - want).max()))


@pytest.mark.parametrize('shape', FR.SHAPES)
def test_filter1d_restatement_equals_scipy(shape):
    a = FR.volume(shape, np.float64)
    sym = np.r_[FR.GENERAL_W, FR.GENERAL_W[::-1][1:]]
    anti = np.r_[FR.GENERAL_W, [0.0], -FR.GENERAL_W[::-1]]
    for mode in FR.MODES:
        for axis in range(3):
            for w in (FR.GENERAL_W, sym, anti, np.array([2.5])):
                want = ndimage.correlate1d(a, w, axis=axis, mode=mode, cval=FR.CVAL)
                assert FR.same(FR.correlate1d(a, w, axis, mode, FR.CVAL), want), (mode, axis, len(w))
            for sigma, order, radius in ((1.3, 0, None), (0.8, 1, None), (2.0, 2, 8), (1.0, 3, None)):
                want = ndimage.gaussian_filter1d(a, sigma, axis=axis, order=order, mode=mode, cval=FR.CVAL, radius=radius)
                got = FR.gaussian_filter1d(a, sigma, axis, order, mode, FR.CVAL, radius=radius)
                assert FR.same(got, want), (mode, axis, sigma, order, radius)


def test_radius_beyond_the_extent_repeats_the_pattern():
    a = FR.volume((1, 2, 3), np.float64)
    w = np.linspace(-1.0, 2.0, 17)                            # radius 8 on extents 1, 2 and 3
    for mode in FR.MODES:
        for axis in range(3):
            assert FR.same(FR.correlate1d(a, w, axis, mode, FR.CVAL), ndimage.correlate1d(a, w, axis=axis, mode=mode, cval=FR.CVAL)), (mode, axis)
    assert list(FR.index_map(np.arange(-5, 9), 4, 'reflect')) == [3, 3, 2, 1, 0, 0, 1, 2, 3, 3, 2, 1, 0, 0]
    assert list(FR.index_map(np.arange(-4, 8), 4, 'mirror')) == [2, 3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1]
    assert list(FR.index_map(np.arange(-3, 3), 1, 'mirror')) == [0] * 6


def test_gaussian_weights_equal_scipys():
    try:
        from scipy.ndimage._filters import _gaussian_kernel1d
    except ImportError:
        pytest.skip('scipy.ndimage._filters._gaussian_kernel1d has moved')
    for sigma in (0.5, 1.0, 1.0 / 0.7, 3.3, 16.0):
        for order in range(4):
            r = int(4.0 * sigma + 0.5)
            assert np.array_equal(FR.gaussian_kernel1d(sigma, order, r), _gaussian_kernel1d(sigma, order, r)), (sigma, order)


def test_form_detection_is_scipys():
    a = FR.volume((4, 5, 40), np.float64)
    base = np.array([0.1, 0.7, 0.25, 1.0, 0.25, 0.7, 0.1])
    ulp = base.copy()
    ulp[5] = np.nextafter(ulp[5], 1.0)                        # one ulp apart: scipy sums these with the symmetric form
    assert ulp[5] != ulp[1] and FR.detect_form(ulp) == 1
    far = base.copy()
    far[5] += 1e-9                                            # 1e-9 apart: the general form
    assert FR.detect_form(far) == 0
    anti = np.array([-0.3, 0.9, -0.2, 0.0, 0.2, -0.9, 0.3])
    assert FR.detect_form(anti) == -1 and FR.detect_form(base) == 1
    for w in (ulp, far, anti, base):
        want = ndimage.correlate1d(a, w, axis=2)
        assert FR.same(FR.correlate1d(a, w, 2), want), w
    # the forms are different sums: the general form on the one-ulp weights is not what scipy computes
    x = FR.extend(a, 3, 'reflect', 0.0)
    assert not FR.same(FR.correlate_lines(x, ulp, 0, 40), ndimage.correlate1d(a, ulp, axis=2))


def test_smooth_label_restatement():
    vol = FR.staircase()
    for sigma, spacing in ((1.0, None), (1.0, (0.7, 0.7, 1.5)), ((0.0, 0.0, 1.2), None)):
        sig = sigma if spacing is None else tuple(sigma / s for s in spacing)
        mask = ndimage.gaussian_filter((vol == 20).astype(np.float64), sig) >= 0.5
        want = vol.copy()
        for p in np.ndindex(*vol.shape):                      # the merge rules, voxel by voxel
            if mask[p] and vol[p] == 0:
                want[p] = 20
            elif not mask[p] and vol[p] == 20:
                want[p] = 3
        got = FR.smooth_label(vol, 20, sigma, spacing, fill=3)
        assert np.array_equal(got, want), (sigma, spacing)
        assert np.array_equal(got == 19, vol == 19)           # the other label is never overwritten
        assert (got != vol).any()
    w = ndimage.gaussian_filter((vol != 0).astype(np.float64), 1.5)
    a, b = FR.volume(vol.shape, np.int16), FR.volume(vol.shape, np.float64, 1)
    assert np.array_equal(FR.feather_blend(a, b, vol, 1.5), ((1.0 - w) * a.astype(np.float64)) + (w * b))
