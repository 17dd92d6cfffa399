"""tests/morph_ref.py pinned on the host: the ball against a brute-force enumeration, the equivalence the kernels of csrc/morph.hip rest on --
{ordered squared distance <= r r} IS scipy's dilation by that ball, border term included, and its dual for the erosion -- and the merge rules
against a case worked out by hand.  Every comparison is exact."""
import itertools

import numpy as np
import pytest

import morph_ref as MR


@pytest.mark.parametrize('spacing', MR.SPACINGS, ids=str)
def test_ball_against_brute_force(spacing):
    for radius in MR.RADII + (5.0, 7.3):
        b = MR.ball(radius, spacing)
        assert all(s % 2 == 1 for s in b.shape) and b[tuple(s // 2 for s in b.shape)]
        c = [s // 2 for s in b.shape]
        got = {tuple(int(x) - cc for x, cc in zip(p, c)) for p in np.argwhere(b)}
        assert got == MR.ball_brute(radius, spacing), (radius, spacing)
        # no empty outer plane: the extents are the reach along each axis
        assert b[0].any() and b[:, 0].any() and b[:, :, 0].any()
    assert MR.ball(0.0, spacing).shape == (1, 1, 1)


def test_ball_on_the_rounding_boundaries():
    """sqrt(3) sqrt(3) rounds below 3 and sqrt(2) sqrt(2) above 2: the corner (1, 1, 1) is outside the first ball, (1, 1, 0) inside the
    second, as the shared expression says."""
    r3, r2 = np.sqrt(3.0), np.sqrt(2.0)
    assert r3 * r3 < 3.0 and r2 * r2 > 2.0
    b = MR.ball(r3)
    assert b.shape == (3, 3, 3) and not b[0, 0, 0] and b.sum() == 19
    b = MR.ball(r2)
    assert b.shape == (3, 3, 3) and b[0, 0, 1] and not b[0, 0, 0] and b.sum() == 19
    assert MR.ball(1.0).sum() == 7 and MR.ball(2.0).sum() == 33


@pytest.mark.parametrize('spacing', MR.SPACINGS, ids=str)
def test_thresholded_squared_distance_is_the_dilation_and_its_dual_the_erosion(spacing):
    shape = (9, 8, 7)
    vols = [MR.random_mask(shape, d, 40 + i) for i, d in enumerate((0.03, 0.3, 0.9))]
    corner = np.zeros(shape, dtype=bool)
    corner[0, 0, shape[2] - 1] = True
    vols += [corner, np.zeros(shape, dtype=bool), np.ones(shape, dtype=bool)]
    for X, b in itertools.product(vols, (0, 1)):
        D, Dc = MR.d2(X, spacing, border=b), MR.d2(~X, spacing, border=1 - b)
        for radius in MR.RADII:
            r2 = np.float64(radius) * np.float64(radius)
            assert np.array_equal(D <= r2, MR.by_ball('dilation', X, radius, spacing, b)), (radius, b)
            assert np.array_equal(~(Dc <= r2), MR.by_ball('erosion', X, radius, spacing, b)), (radius, b)


def test_a_ball_larger_than_the_volume():
    X = MR.random_mask((5, 4, 6), 0.05, 3)
    assert X.any()
    for b in (0, 1):
        assert MR.by_ball('dilation', X, 20.0, border_value=b).all()
        assert np.array_equal(MR.d2(X, border=b) <= 400.0, MR.by_ball('dilation', X, 20.0, border_value=b))
        assert np.array_equal(MR.by_ball('erosion', X, 20.0, border_value=b), np.zeros_like(X))


def test_shared_cases_do_what_they_are_for():
    """A closing by radius r joins what a gap of up to 2 r voxels separates (each side grows r into it): r = 1 joins the slabs across one and
    two empty planes, not across three.  An opening by r = 1 cuts the one-voxel bridge (its stubs at the bodies stay) and keeps the bodies."""
    assert MR.by_ball('closing', MR.slabs(1), 1.0)[4, 4, 6]
    assert MR.by_ball('closing', MR.slabs(2), 1.0)[4, 4, 6:8].all()
    assert not MR.by_ball('closing', MR.slabs(3), 1.0)[4, 4, 6:9].any()
    v, bridge = MR.bridged()
    opened = MR.by_ball('opening', v, 1.0)
    assert v[bridge].all() and not opened[5, 5, 9:11].any() and opened[3:8, 3:8, 3:7].all() and opened[3:8, 3:8, 13:17].all()


def test_merge_rules():
    v = np.array([[[0, 5, 5, 7, 0, 3]]], dtype=np.uint8)
    m = np.array([[[1, 1, 0, 1, 0, 1]]], dtype=np.uint8)
    # grow: only the background voxel under the mask changes; 7 and 3 under the mask stay, label 5 outside the mask stays
    assert MR.merge(v, m, 'grow', 5).tolist() == [[[5, 5, 5, 7, 0, 3]]]
    assert MR.merge(v, m, 'grow', 5, background=3).tolist() == [[[0, 5, 5, 7, 0, 5]]]
    # shrink: only label 5 outside the mask changes
    assert MR.merge(v, m, 'shrink', 5, fill=9).tolist() == [[[0, 5, 9, 7, 0, 3]]]
    assert MR.merge(v, m, 'shrink', 7, fill=9).tolist() == v.tolist()
    f = v.astype(np.float64)
    assert MR.merge(f, m, 'grow', 5.0).dtype == np.float64
    vol = MR.two_fragment_body()
    closed = MR.close_label(vol, 20, 1.0)
    assert (closed[6:16, 6:16, 14] == 20).all() and np.array_equal(closed[vol != 0], vol[vol != 0])
