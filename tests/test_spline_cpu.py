"""The numpy restatement of cubic B-spline resampling (tests/spline_ref.py) against scipy.ndimage.spline_filter / map_coordinates and against
the reference's own order=3 crops (fixture G23, tools/make_golden_spline.py), on the host.  The two largest differences measured here fix the
device tolerance of tests/test_spline_gpu.py: SPLINE_TOL = 10 x the larger, floor 1e-9.

Measured (scipy 1.15.3): |restatement - scipy| 2.73e-12 over the prefilter cases (divided by max|data| / 255 where the data is larger than
255) and 3.13e-13 over the sample cases; |restatement - G23| 2.84e-13 in each of iso, thick and aniso (scipy at the restated grid gives G23's
bits).  10 x 2.8e-12 = 2.8e-11 is below the floor: SPLINE_TOL = 1e-9."""
import numpy as np
import pytest

import spline_ref as P

_CACHE = {}


def _g23():
    if 'g' not in _CACHE:
        import hvgan  # noqa: F401
        _CACHE['g'] = P.load_g23()
    return _CACHE['g']


def test_prefilter_restatement_matches_scipy():
    from scipy.ndimage import spline_filter
    worst = 0.0
    for k, shape in enumerate(P.prefilter_shapes()):
        v = P.case_volume(shape, k)
        for data in (v, P.window(v)):
            ref = spline_filter(data, 3, mode='mirror', output=np.float64)
            assert np.array_equal(ref, spline_filter(data, 3, mode='constant', output=np.float64))     # 'constant' filters the same way
            err = np.abs(P.spline_filter3(data) - ref).max() / P.scale_of(data)
            worst = max(worst, err)
    print('largest |restatement - scipy.spline_filter| (scaled) %.3g' % worst)
    assert worst <= P.MEASURED_SCIPY


def test_a_line_of_length_one_is_left_alone():
    v = P.case_volume((1, 1, 1))
    assert np.array_equal(P.spline_filter3(v), v)
    v = P.case_volume((1, 6, 1))
    from scipy.ndimage import spline_filter
    assert np.abs(P.spline_filter3(v) - spline_filter(v, 3, mode='mirror')).max() <= P.MEASURED_SCIPY * P.scale_of(v)


def test_sample_restatement_matches_scipy_at_the_borders():
    from scipy.ndimage import map_coordinates
    rng = np.random.RandomState(3)
    v = P.window(P.case_volume((9, 11, 13), 5))
    co = np.stack([rng.uniform(-1.0, s, 4000) for s in v.shape])
    # exactly 0, exactly n - 1, just past n - 1, inside the last cell (the tap at n mirrors to n - 2), just below 0
    co[:, 0] = 0.0
    co[:, 1] = [8.0, 10.0, 12.0]
    co[:, 2] = [8.0 + 1e-7, 5.0, 5.0]
    co[:, 3] = [7.5, 9.9, 11.99]
    co[:, 4] = [4.0, -1e-9, 6.0]
    co[:, 5] = [3.0, 4.0, 5.0]
    mine, ref = P.map_coordinates3(v, co), map_coordinates(v, co, order=3, mode='constant', cval=0.0)
    assert mine[2] == 0.0 and ref[2] == 0.0 and mine[4] == 0.0 and ref[4] == 0.0 and ref[3] != 0.0
    assert abs(mine[5] - v[3, 4, 5]) <= P.MEASURED_SCIPY            # a lattice point: the voxel itself
    err = np.abs(mine - ref).max()
    print('largest |restatement - scipy.map_coordinates| %.3g; range of the samples [%.2f, %.2f]' % (err, ref.min(), ref.max()))
    assert err <= P.MEASURED_SCIPY
    assert ref.min() < 0.0 and ref.max() > 255.0                    # no clipping: cubic samples of [0, 255] data leave the interval
    # degenerate extents: every tap of a length-1 axis is its only coefficient
    v1 = P.window(P.case_volume((1, 4, 2), 6))
    co = np.stack([np.zeros(50), rng.uniform(0, 3, 50), rng.uniform(0, 1, 50)])
    assert np.abs(P.map_coordinates3(v1, co) - map_coordinates(v1, co, order=3)).max() <= P.MEASURED_SCIPY


@pytest.mark.parametrize('name', ['iso', 'thick', 'aniso'])
def test_restatement_matches_the_reference_crops(name):
    from scipy.ndimage import map_coordinates
    c = _g23()[name]
    plan = P.plan_of(c)
    assert np.array_equal(np.array(plan[3]), c['boxes'])
    mine = P.straighten_crops(c['ct'], plan, c['out_size'], c['window'], c['spacing'])
    err = np.abs(mine - c['crop_ct']).max()
    sci = P.straighten_crops(c['ct'], plan, c['out_size'], c['window'], c['spacing'], mapper=lambda v, g: map_coordinates(v, g, order=3))
    print(name, 'largest |restatement - G23| %.3g, |scipy at the restated grid - G23| %.3g' % (err, np.abs(sci - c['crop_ct']).max()))
    assert mine.shape == c['crop_ct'].shape and (c['crop_ct'] != 0).any()
    assert err <= P.MEASURED_G23


def test_the_tolerance_is_ten_times_the_measured_figures_with_the_crop_floor():
    assert P.SPLINE_TOL == max(10 * max(P.MEASURED_SCIPY, P.MEASURED_G23), 1e-9) == 1e-9
    assert set(_g23()) == {'iso', 'thick', 'aniso'}
    assert _g23()['iso']['spacing'] == (1.0, 1.0, 1.0) and _g23()['thick']['spacing'] == (2.5, 0.9, 0.9)
