"""tests/rank_ref.py -- the numpy restatement the device rank filters are compared with -- and the host functions of rank_filters.py
(footprints, origins, percentile ranks, the ball, grey dilation's reversed footprint, the separable box) against scipy.ndimage: np.array_equal
and equal dtype, on inputs without NaN or -0.0.  No GPU."""
import warnings

import numpy as np
import pytest
from scipy import ndimage

import rank_ref as RR


def _RF():
    import hvgan  # noqa: F401
    from hvgan import rank_filters
    return rank_filters


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), what


_RANDOM_553 = np.random.RandomState(11).rand(5, 5, 3) < 0.45
# (footprint array, origin)
FOOTPRINTS = (
    (np.ones((3, 3, 3), dtype=bool), (0, 0, 0)),
    (np.ones((2, 3, 4), dtype=bool), (0, 0, 0)),
    (np.ones((2, 3, 4), dtype=bool), (-1, 1, -2)),
    (_RANDOM_553, (1, -2, 0)),
    (np.ones((1, 1, 9), dtype=bool), (0, 0, 0)),
)


@pytest.mark.parametrize('dtype', RR.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('shape', RR.SHAPES, ids=str)
def test_restatement_equals_scipy(shape, dtype):
    RF = _RF()
    a = RR.volume(shape, dtype)
    for fp, origin in FOOTPRINTS:
        off = RF.footprint_offsets(footprint=fp, origin=origin)
        assert np.array_equal(off, RR.box_offsets(None, origin, fp))
        n = len(off)
        assert n == int(fp.sum()) and n >= 4
        for mode in RR.MODES:
            for rank in (0, 1, n // 2, n - 1):
                want = ndimage.rank_filter(a, rank, footprint=fp, mode=mode, cval=RR.CVAL, origin=origin)
                _same(RR.rank_filter(a, off, rank, mode, RR.CVAL), want, (fp.shape, origin, mode, rank))


def test_footprint_offsets_follow_scipys_rules():
    RF = _RF()
    assert np.array_equal(RF.footprint_offsets(size=3), RR.box_offsets((3, 3, 3)))
    assert np.array_equal(RF.footprint_offsets(size=(2, 3, 4)), RR.box_offsets((2, 3, 4)))          # even extents: the centre is shape // 2
    assert RF.footprint_offsets(size=(2, 1, 1)).tolist() == [[-1, 0, 0], [0, 0, 0]]
    assert RF.footprint_offsets(size=(2, 1, 1), origin=(-1, 0, 0)).tolist() == [[0, 0, 0], [1, 0, 0]]
    assert len(RF.footprint_offsets(size=9)) == 729
    fp = np.zeros((3, 3, 3), dtype=bool)
    fp[0, 1, 2] = fp[2, 2, 0] = True
    with warnings.catch_warnings(record=True) as w:                                               # a footprint wins over size, with a warning
        warnings.simplefilter('always')
        assert RF.footprint_offsets(size=5, footprint=fp).tolist() == [[-1, 0, 1], [1, 1, -1]]
        assert len(w) == 1
    a = RR.volume((5, 6, 7), np.int16)
    for origin in ((2, 0, 0), (0, -2, 0), (0, 0, 2)):                                             # the centre outside the footprint: scipy refuses too
        with pytest.raises(ValueError):
            RF.footprint_offsets(size=3, origin=origin)
        with pytest.raises(ValueError):
            ndimage.rank_filter(a, 0, size=3, origin=origin)
    with pytest.raises(ValueError):
        RF.footprint_offsets(size=(11, 1, 1))                                                     # an offset of 5
    with pytest.raises(ValueError):
        RF.footprint_offsets(size=(8, 1, 1), origin=(-4, 0, 0))                                   # offsets 0 .. 7
    assert RF.footprint_offsets(size=(5, 1, 1), origin=(-2, 0, 0))[:, 0].tolist() == [0, 1, 2, 3, 4]
    with pytest.raises(ValueError):
        RF.footprint_offsets(footprint=np.zeros((3, 3, 3), dtype=bool))
    with pytest.raises(RuntimeError):
        RF.footprint_offsets()


def test_percentile_rank_and_negative_ranks_are_scipys():
    RF = _RF()
    a = RR.volume((5, 6, 7), np.float32)
    fp, origin = FOOTPRINTS[3]
    off = RF.footprint_offsets(footprint=fp, origin=origin)
    n = len(off)
    for p in (-20, 0, 35, 50, 100):
        want = ndimage.percentile_filter(a, p, footprint=fp, mode='mirror', origin=origin)
        _same(RR.rank_filter(a, off, RF.percentile_rank(n, p), 'mirror'), want, p)
    assert RF.percentile_rank(27, 100) == 26 and RF.percentile_rank(27, -100) == 0 and RF.percentile_rank(27, 50) == 13
    for p in (-100.5, 100.5):
        with pytest.raises(RuntimeError):
            RF.percentile_rank(27, p)
    assert RF._rank_of(-1, n) == n - 1 and RF._rank_of(-n, n) == 0
    for r in (n, -n - 1):
        with pytest.raises(RuntimeError):
            RF._rank_of(r, n)
        with pytest.raises(RuntimeError):
            ndimage.rank_filter(a, r, footprint=fp)
    _same(RR.rank_filter(a, RF.footprint_offsets(size=3), 27 // 2), ndimage.median_filter(a, size=3), 'median')


def test_ball_is_the_morphology_ball():
    RF = _RF()
    from hvgan import morphology as M
    for radius, spacing in ((1.5, (0.7, 0.7, 1.5)), (1.0, (1, 1, 1)), (0.0, (1, 1, 1)), (2.9, (1.0, 0.8, 2.0))):
        b = M.ball(radius, spacing)
        off = RF.ball(radius, spacing)
        assert len(off) == int(b.sum()) and np.array_equal(off, RR.box_offsets(None, (0, 0, 0), b))
        s = np.array(spacing, dtype=np.float64)
        assert all((((s[0] * o[0]) ** 2 + (s[1] * o[1]) ** 2) + (s[2] * o[2]) ** 2 <= radius * radius) for o in off)
    assert len(RF.ball(1.5, (0.7, 0.7, 1.5))) == 13 + 2                                           # o0^2 + o1^2 <= 4 in plane (1.5 / 0.7 = 2.14), and one voxel along z
    with pytest.raises(ValueError):
        RF.ball(5.0)


@pytest.mark.parametrize('dtype', (np.uint8, np.float64), ids=lambda d: np.dtype(d).name)
def test_grey_morphology_footprints_are_scipys(dtype):
    RF = _RF()
    a = RR.volume((5, 6, 7), dtype)
    odd = np.random.RandomState(3).rand(3, 3, 5) < 0.6
    even = np.random.RandomState(4).rand(2, 4, 3) < 0.7
    cases = [dict(size=(3, 3, 3)), dict(size=(2, 3, 4)), dict(size=(2, 3, 4), origin=(-1, 1, -2)), dict(footprint=odd),
             dict(footprint=odd, origin=(1, 0, -2)), dict(footprint=even), dict(footprint=even, origin=(0, -2, 1))]
    for kw in cases:
        origin = kw.get('origin', 0)
        for mode in ('reflect', 'constant', 'wrap'):
            ero = RF.footprint_offsets(kw.get('size'), kw.get('footprint'), origin)
            fp, org = RF.dilation_arguments(kw.get('size'), kw.get('footprint'), origin)
            dil = RF.footprint_offsets(kw.get('size'), fp, org)

            def erode(x):
                return RR.rank_filter(x, ero, 0, mode, RR.CVAL)

            def dilate(x):
                return RR.rank_filter(x, dil, -1, mode, RR.CVAL)
            sk = dict(kw, mode=mode, cval=RR.CVAL)
            _same(erode(a), ndimage.grey_erosion(a, **sk), ('erosion', kw, mode))
            _same(dilate(a), ndimage.grey_dilation(a, **sk), ('dilation', kw, mode))
            _same(dilate(erode(a)), ndimage.grey_opening(a, **sk), ('opening', kw, mode))
            _same(erode(dilate(a)), ndimage.grey_closing(a, **sk), ('closing', kw, mode))


def test_box_minimum_is_separable():
    RF = _RF()
    for shape in RR.SHAPES:
        a = RR.volume(shape, np.int16)
        for size, origin in (((3, 2, 5), (0, 0, 0)), ((2, 3, 4), (-1, 1, -2)), ((1, 1, 3), (0, 0, 1))):
            off = RF.footprint_offsets(size, None, origin)
            for mode in RR.MODES:
                for rank, fn in ((0, ndimage.minimum_filter), (-1, ndimage.maximum_filter)):
                    want = fn(a, size=size, mode=mode, cval=RR.CVAL, origin=origin)
                    _same(RR.rank_filter(a, off, rank, mode, RR.CVAL), want, (shape, size, mode, rank))
                    step = a
                    for ax in range(3):                                                           # one line footprint per axis
                        line = np.unique(off[:, ax])
                        lo = np.zeros((len(line), 3), dtype=np.int64)
                        lo[:, ax] = line
                        step = RR.rank_filter(step, lo, rank, mode, RR.CVAL)
                    _same(step, want, (shape, size, mode, rank, 'separable'))
