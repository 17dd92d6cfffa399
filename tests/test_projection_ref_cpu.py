"""Pins tests/projection_ref.py, the numpy restatement of hv_project and of the host formulas of healthivert-gan_amd/projection.py (DESIGN.md
section 8 row f20): the vectorised form against plain loops, every sample against scipy.ndimage.affine_transform bit for bit, the identity
views against vol.sum(axis), the chunked sum's edge words, the info identity, view_pose's geometry, and the radiograph of a ball against the
closed form.  And what needs no GPU of the new entry: the header declarations and the library's exports."""
import ctypes
import os

import numpy as np
import pytest
from scipy import ndimage

import projection_ref as PR
import resample_ref as R

OBLIQUE = (np.array([[0.9, 0.1, 0.3], [-0.1, 0.95, 0.2], [0.05, -0.2, 0.8]]), np.array([0.3, 0.5, -1.0]))
IDENT = (np.eye(3), np.zeros(3))


def _vol(dtype=np.int16, shape=(5, 6, 7), seed=0):
    return R.case_volume(dtype, shape, seed)


def _same(a, b):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


@pytest.mark.parametrize('order', (0, 1, 3))
def test_the_restatement_equals_the_plain_loops(order):
    vol = _vol()
    lab = (np.random.default_rng(3).random(vol.shape) < 0.7).astype(np.uint8) * 5
    poses = [IDENT, OBLIQUE]
    _same(PR.project_ref(vol, poses, (5, 6), 20, order), PR.project_brute(vol, poses, (5, 6), 20, order))
    _same(PR.project_ref(vol, poses, (4, 3), 35, order, lab, 5), PR.project_brute(vol, poses, (4, 3), 35, order, lab, 5))


@pytest.mark.parametrize('order', (0, 1, 3))
@pytest.mark.parametrize('dtype', (np.uint8, np.int16, np.float32, np.float64), ids=lambda d: np.dtype(d).name)
def test_every_sample_is_scipys_bit_for_bit_where_inside(dtype, order):
    vol = _vol(dtype)
    P0, P1, T = 6, 5, 19
    for m, off in (IDENT, OBLIQUE):
        if order == 3:
            coef = ndimage.spline_filter(vol.astype(np.float64), 3, output=np.float64, mode='mirror')
            want = ndimage.affine_transform(coef, m, off, output_shape=(P0, P1, T), output=np.float64, order=3, prefilter=False)
            y, state = PR.samples(vol, (m, off), (P0, P1), T, 3, coef=coef)
        else:
            want = ndimage.affine_transform(vol.astype(np.float64), m, off, output_shape=(P0, P1, T), output=np.float64, order=order)
            y, state = PR.samples(vol, (m, off), (P0, P1), T, order)
        inside = state == 1
        assert inside.any() and (state == 2).any()
        assert y[inside].tobytes() == want[inside].tobytes()


def test_an_identity_view_along_each_axis_is_the_plain_sum():
    vol = _vol(np.int16, (5, 6, 7), 4)
    for view, (a0, a1, ar) in PR.VIEWS.items():
        m, off, det, T, ds, st = PR.view_pose(vol.shape, (1, 1, 1), view, det_spacing=1.0, step_mm=1.0, det_shape=(vol.shape[a0], vol.shape[a1]),
                                              steps=vol.shape[ar])
        assert not off.any() and sorted(np.argwhere(m == 1.0)[:, 0].tolist()) == [0, 1, 2] and np.abs(m).sum() == 3.0
        for order in (0, 1):
            acc, idx, info = PR.project_ref(vol, [(m, off)], det, T, order)
            assert (acc[0, 0] == vol.sum(axis=ar, dtype=np.int64)).all() and (idx[0, 0] == vol.shape[ar]).all()
            assert (acc[0, 1] == vol.min(axis=ar)).all() and (acc[0, 2] == vol.max(axis=ar)).all()
            assert (idx[0, 1] == 0).all() and (idx[0, 2] == vol.shape[ar] - 1).all()
            assert info[0].tolist() == [0, vol.size, 0, 0, 0, 0, 0, 0]


def test_ragged_and_empty_chunks_give_the_stated_words():
    """T = 33 (two full chunks and one step); a label that leaves the middle chunk empty and cuts the first mid-chunk; a ray with nothing."""
    T = 33
    vol = np.zeros((1, 2, T))
    vol[0, 0] = 0.1 * np.arange(1, T + 1)
    vol[0, 1] = -0.0
    lab = np.ones((1, 2, T), dtype=np.uint8)
    lab[0, 0, 5:32] = 0                                                # counted: t = 0 .. 4 and t = 32
    acc, idx, info = PR.project_ref(vol, [IDENT], (1, 2), T, 0, lab, 1)
    c0 = 0.0
    for t in range(5):
        c0 = c0 + vol[0, 0, t]
    want = ((0.0 + c0) + 0.0) + (0.0 + vol[0, 0, 32])
    assert acc[0, 0, 0, 0] == want and idx[0, :, 0, 0].tolist() == [6, 0, 32]
    assert acc[0, 1, 0, 0] == vol[0, 0, 0] and acc[0, 2, 0, 0] == vol[0, 0, 32]
    for w in acc[0, :, 0, 1]:                                          # a ray of -0.0: sum, min and max are all +0.0
        assert w == 0.0 and not np.signbit(w)
    assert idx[0, :, 0, 1].tolist() == [T, 0, T - 1]
    assert info[0].tolist() == [0, 6 + T, 0, 27, 0, 0, 0, 0]
    # the sum differs from numpy's pairwise sum and from a plain sequential sum in general: the order is the definition
    x = np.random.default_rng(1).standard_normal((1, 1, 300)) * 1e3
    acc, idx, _ = PR.project_ref(x, [IDENT], (1, 1), 300, 0)
    seq = 0.0
    for v in x[0, 0]:
        seq = seq + v
    assert acc[0, 0, 0, 0] == PR.project_brute(x, [IDENT], (1, 1), 300, 0)[0][0, 0, 0, 0] and idx[0, 0, 0, 0] == 300
    assert abs(acc[0, 0, 0, 0] - seq) <= 1e-9
    # no counted step
    acc, idx, info = PR.project_ref(vol, [(np.eye(3), np.array([5.0, 0.0, 0.0]))], (1, 2), T, 1)
    assert np.isposinf(acc[0, 1]).all() and np.isneginf(acc[0, 2]).all() and (acc[0, 0] == 0).all() and not np.signbit(acc[0, 0]).any()
    assert (idx[0, 0] == 0).all() and (idx[0, 1] == T).all() and (idx[0, 2] == -1).all()
    assert info[0].tolist() == [PR.EMPTY, 0, 2 * T, 0, 0, 0, 0, 0]


def test_the_info_identity_holds_with_non_finite_voxels():
    vol = _vol(np.float32, (5, 6, 7), 2).copy()
    vol[2, 3, 4], vol[1, 1, 1], vol[4, 0, 6] = np.nan, np.inf, -np.inf
    lab = (np.random.default_rng(5).random(vol.shape) < 0.8).astype(np.int16) * 3
    for order in (0, 1):
        acc, idx, info = PR.project_ref(vol, [IDENT, OBLIQUE], (6, 7), 21, order, lab, 3)
        for k in range(2):
            assert info[k, 1:5].sum() == 6 * 7 * 21 and idx[k, 0].sum() == info[k, 1] and info[k, 4] > 0 and info[k, 3] > 0
            assert info[k, 0] == PR.NONFINITE and not info[k, 5:].any()
            assert np.isfinite(acc[k, 0]).all()


@pytest.mark.parametrize('view', ('lateral', 'ap', 'axial', (20.0, 35.0, 10.0)), ids=str)
def test_view_pose_centres_the_ray_and_covers_the_corners(view):
    shape, sp = (31, 20, 12), (0.7, 0.9, 1.5)
    m, off, det, T, ds, st = PR.view_pose(shape, sp, view)
    mid = (np.array([det[0], det[1], T]) - 1.0) / 2.0
    centre = (np.array(shape) - 1.0) / 2.0
    assert np.abs(m @ mid + off - centre).max() <= 1e-12 * np.abs(centre).max()
    assert np.abs(np.linalg.norm(m[:, 2] * np.array(sp)) - st) <= 1e-12                  # one step is step_mm millimetres
    assert abs((m[:, 0] * np.array(sp)) @ (m[:, 2] * np.array(sp))) <= 1e-12             # the detector is square to the ray
    inv = np.linalg.inv(m)
    for c in np.ndindex(2, 2, 2):
        q = inv @ (np.array(c) * (np.array(shape) - 1.0) - off)
        assert (q >= -1e-9).all() and (q <= np.array([det[0], det[1], T]) - 1.0 + 1e-9).all(), (c, q)
    if isinstance(view, str):
        a0, a1, ar = PR.VIEWS[view]
        assert m[a0, 0] == ds[0] / sp[a0] and m[a1, 1] == ds[1] / sp[a1] and m[ar, 2] == st / sp[ar] and np.count_nonzero(m) == 3


# measured with the restatement (order 1, one ray through the centre, pitch and step 0.7 mm = the smallest spacing): the named views
# |radiograph - v * 24 mm| / (v * 24 mm) = 0.0617 lateral (along the 1.5 mm axis), 0.0208 ap and axial; oblique (20, 35, 10) degrees 0.0213
BALL_ERROR = {'lateral': 148.0, 'ap': 50.0, 'axial': 50.0, (20.0, 35.0, 10.0): 51.17}
# the thickness through the centre (count * step at order 0 on the ball as its own label) against 24 mm, measured the same way, in mm
THICKNESS_ERROR = {'lateral': 1.2, 'ap': 0.5, 'axial': 0.5, (20.0, 35.0, 10.0): 1.2}


@pytest.mark.parametrize('view', list(BALL_ERROR), ids=str)
def test_the_radiograph_of_a_ball_is_value_times_chord(view):
    """A ball of value v = 100 and radius 12 mm in a (41, 41, 21) volume of spacing (0.7, 0.7, 1.5) mm: the ray through its centre measures
    v * 24 mm = 2400 in the closed form.  Measured discretisation error (order 1; the ball is voxelised at the voxel centres and the step is
    0.7 mm): lateral 148.0 (6.17 %: the ray runs along the 1.5 mm axis, where the ball's chord is a whole number of 1.5 mm voxels), ap 50.0 and
    axial 50.0 (2.08 %), oblique (20, 35, 10) degrees 51.16 (2.13 %); the thickness map's count * step against 24 mm: 1.2, 0.5, 0.5 and 1.2 mm.  The assertions
    allow twice the measured errors."""
    shape, sp, v = (41, 41, 21), (0.7, 0.7, 1.5), 100.0
    ball = PR.ball(shape, sp, 12.0, v)
    m, off, det, T, ds, st = PR.view_pose(shape, sp, view, det_shape=(1, 1))
    acc, idx, info = PR.project_ref(ball, [(m, off)], det, T, 1)
    got = PR.radiograph(acc[0], st)[0, 0]
    print('ball radiograph', view, got, abs(got - v * 24.0))
    assert abs(got - v * 24.0) <= 2.0 * BALL_ERROR[view]
    assert abs(acc[0, 2, 0, 0] - v) <= 1e-12 * v and abs(acc[0, 1, 0, 0]) <= 1e-12 * v    # interpolation weights sum to 1 within an ulp
    thick = PR.thickness_map(PR.project_ref(ball, [(m, off)], det, T, 0, ball, v)[1][0], st)[0, 0]
    print('ball thickness', view, thick, abs(thick - 24.0))
    assert abs(thick - 24.0) <= 2.0 * THICKNESS_ERROR[view]


def test_areal_density_of_a_slab_is_value_times_thickness():
    """A slab of value 200 filling the volume, 8 voxels of 1.5 mm thick along the ray: every pixel measures 200 * 8 * 1.5 with the volume's
    own lattice, the area is the face's, the mean path 12 mm."""
    vol = np.full((6, 5, 8), 200, dtype=np.int16)
    lab = np.ones(vol.shape, dtype=np.uint8)
    m, off, det, T, ds, st = PR.view_pose(vol.shape, (0.7, 0.9, 1.5), 'lateral', det_spacing=(0.7, 0.9), step_mm=1.5, det_shape=(6, 5), steps=8)
    acc, idx, _ = PR.project_ref(vol, [(m, off)], det, T, 1, lab, 1)
    a = PR.areal_density(acc[0], idx[0], ds, st)
    assert a['pixels'] == 30 and a['samples'] == 240
    assert abs(a['area'] - 30 * 0.63) <= 1e-12 * a['area'] and abs(a['areal_density'] - 2400.0) <= 1e-9 and abs(a['mean_path'] - 12.0) <= 1e-12


def test_the_header_declares_the_entries_and_the_library_exports_them():
    import hvgan  # noqa: F401
    from hvgan import lib
    src = open(lib.HEADER).read()
    for name in ('hv_project', 'hv_project_workspace_bytes', 'hv_project_tile', 'HV_PROJ_CHUNK = 16', 'HV_PROJ_MAX_POSES = 16', 'HV_PROJ_INFO = 8'):
        assert name in src, name
    _, protos = lib.parse_header()
    assert len(protos['hv_project'][1]) == 26 and protos['hv_project_workspace_bytes'][0] is ctypes.c_size_t
    assert len(protos['hv_project_tile'][1]) == 1
    if not os.path.exists(lib.LIB_PATH):
        pytest.skip('libhvgan.so is not built')
    L = lib.get()
    for name in ('hv_project', 'hv_project_workspace_bytes', 'hv_project_tile'):
        assert hasattr(L.cdll, name), name
    dims = (ctypes.c_int * 5)()
    assert L.cdll.hv_project_tile(dims) == 0 and list(dims) == [16, 16, 16, 64, 4]
    assert L.cdll.hv_project_tile(None) == -1
    assert L.size('hv_project_workspace_bytes', 512, 512, 400, 16, 512, 400, 512) == 0
    from hvgan import projection as P
    assert (P.CHUNK, P.MAX_POSES, P.INFO) == (16, 16, 8) and P.VIEWS == PR.VIEWS
