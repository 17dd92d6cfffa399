"""Pins tests/shape_ref.py, the numpy restatement of hv_shape and of the host formulas of healthivert-gan_amd/shape.py (DESIGN.md section 8 row
f19): the histogram against a triple loop, count and axis intercepts against plain numpy, both Euler numbers against components - tunnels +
cavities on shapes whose topology is known (components and cavities cross-checked with scipy.ndimage.label), the isotropic Crofton weights
against Ohser and Muecklich's constants, the Crofton area of two spheres, the covariance against np.cov.  And what needs no GPU of the new
entry: the header declarations and the library's exports."""
import ctypes
import math

import numpy as np
import pytest
from scipy import ndimage

import shape_ref as SR


def _x(seed=0, shape=(5, 6, 7), p=0.5):
    return np.random.default_rng(seed).random(shape) < p


def test_histogram_equals_the_triple_loop():
    for seed, p in ((0, 0.5), (1, 0.15), (2, 0.9)):
        x = _x(seed, p=p)
        h = SR.histogram_ref(x)
        assert h.dtype == np.int64 and h.tobytes() == SR.histogram_brute(x).tobytes()
        assert h.sum() == 6 * 7 * 8
    assert SR.histogram_ref(np.ones((1, 1, 1), bool)).tolist() == [0] + [1 if c in (1, 2, 4, 8, 16, 32, 64, 128) else 0 for c in range(1, 256)]


def test_record_of_several_labels_counts_a_cell_in_each_slot():
    lab = np.random.default_rng(3).integers(0, 4, (5, 6, 7)).astype(np.uint8)
    rec = SR.record_ref(lab, (1, 3, 9))
    for s, l in enumerate((1, 3)):
        assert rec[s, :256].tobytes() == SR.histogram_brute(lab == l).tobytes() and rec[s, SR.COUNT] == (lab == l).sum()
        p = np.argwhere(lab == l)
        assert rec[s, SR.SUM:SR.SUM + 3].tolist() == p.sum(axis=0).tolist() and rec[s, SR.SUM2 + 4] == (p[:, 1] * p[:, 2]).sum()
        assert rec[s, SR.EXTENT + 2 * 4] == (p[:, 0] - p[:, 1] - p[:, 2]).min() and rec[s, SR.EXTENT + 2 * 12 + 1] == p.sum(axis=1).max()
        assert rec[s, SR.STATUS] == 0 and not rec[s, SR.STATUS + 1:].any()
    assert rec[2, 0] == 6 * 7 * 8 and not rec[2, 1:257].any() and rec[2, SR.STATUS] == SR.EMPTY
    assert (rec[2, SR.EXTENT:SR.STATUS:2] == SR.I64_MAX).all() and (rec[2, SR.EXTENT + 1:SR.STATUS:2] == SR.I64_MIN).all()


def test_count_and_axis_intercepts_are_exact():
    x = _x(4, (6, 5, 9))
    mk = SR.minkowski_ref(SR.histogram_ref(x))
    assert mk['count'] == x.sum()
    for ax, d in enumerate(((1, 0, 0), (0, 1, 0), (0, 0, 1))):
        y = np.moveaxis(x, ax, 0)
        assert mk['intercepts'][SR.DIRS.index(d)] == ((~y[:-1]) & y[1:]).sum() + y[0].sum()
    # a diagonal: the pairs (p, p + d) with p outside the label (or the volume) and p + d inside
    d = (1, -1, 1)
    p = np.pad(x, 1)
    inside, before = p[1:-1, 1:-1, 1:-1], p[0:-2, 2:, 0:-2]
    assert mk['intercepts'][SR.DIRS.index(d)] == (inside & ~before).sum()
    assert mk['face_area'] == 2 * sum(mk['intercepts'][SR.DIRS.index(d)] for d in ((1, 0, 0), (0, 1, 0), (0, 0, 1)))


def _topology(x):
    """(components, cavities) for the label 6-connected (its background 26-connected) and 26-connected (background 6-connected)."""
    full = ndimage.generate_binary_structure(3, 3)
    p = np.pad(x, 1)
    return ((ndimage.label(x)[1], ndimage.label(~p, full)[1] - 1), (ndimage.label(x, full)[1], ndimage.label(~p)[1] - 1))


@pytest.mark.parametrize('name, x, tunnels, e6, e26', (
    ('ball', SR.ball(6), 0, 1, 1), ('hollow ball', SR.hollow_ball(8, 4), 0, 2, 2), ('torus', SR.torus(8, 3), 1, 0, 0)))
def test_euler_numbers_of_known_topology(name, x, tunnels, e6, e26):
    mk = SR.minkowski_ref(SR.histogram_ref(x))
    (c6, v6), (c26, v26) = _topology(x)
    assert (c6, c26) == (1, 1) and v6 == v26 == (1 if name == 'hollow ball' else 0)
    assert mk['euler_6'] == c6 - tunnels + v6 == e6 and mk['euler_26'] == c26 - tunnels + v26 == e26, (name, mk['euler_6'], mk['euler_26'])


def test_two_voxels_touching_at_a_corner():
    x = np.zeros((2, 2, 2), bool)
    x[0, 0, 0] = x[1, 1, 1] = True
    mk = SR.minkowski_ref(SR.histogram_ref(x))
    (c6, _), (c26, _) = _topology(x)
    assert (c6, c26) == (2, 1) and mk['euler_6'] == 2 and mk['euler_26'] == 1 and mk['count'] == 2


def test_isotropic_weights_are_ohser_and_muecklichs():
    w = SR.direction_weights_ref((1, 1, 1))
    assert abs(w.sum() - 1.0) < 1e-12
    for d, x in zip(SR.DIRS, w):
        want = {1: 0.091556, 2: 0.073961, 3: 0.070391}[sum(abs(c) for c in d)]
        assert abs(x - want) <= 1e-3, (d, x, want)
    assert np.array_equal(SR.direction_weights_ref((2.5, 2.5, 2.5)), w)            # a common factor changes no direction


def test_crofton_area_of_spheres():
    """Measured here: 2829.7 against 2827.4 (0.08 %) for the ball of 15 voxels, 1795.9 against 1809.6 (0.75 %) for the 12 mm sphere at
    (0.7, 0.7, 1.5); the cap of 2 % is a little over twice the worse."""
    for x, sp, r in ((SR.ball(15), (1.0, 1.0, 1.0), 15.0), (SR.ellipsoid_mm(12.0, (0.7, 0.7, 1.5)), (0.7, 0.7, 1.5), 12.0)):
        mk = SR.minkowski_ref(SR.histogram_ref(x), sp)
        exact = 4.0 * math.pi * r * r
        print('crofton area r = %g at %s: %.1f against %.1f (%.2f %%)' % (r, sp, mk['surface_area'], exact, 100 * abs(mk['surface_area'] / exact - 1)))
        assert abs(mk['surface_area'] / exact - 1.0) <= 0.02
        assert mk['face_area'] > mk['surface_area']                                  # the staircase over-counts


def test_covariance_and_eigenvalues_are_np_covs():
    sp = (0.7, 0.9, 1.5)
    g = np.indices((14, 17, 11))
    # sheared along every axis: no covariance is zero, so a relative bound means something for each entry
    x = ((g[0] - 6.0) / 6.0) ** 2 + ((g[1] - 8.0 - 0.4 * (g[0] - 6.0)) / 7.5) ** 2 + ((g[2] - 5.0 - 0.3 * (g[1] - 8.0) + 0.2 * (g[0] - 6.0)) / 4.5) ** 2 <= 1.0
    d = SR.descriptors_ref(SR.record_ref(x.astype(np.uint8), (1,))[0], sp)
    mm = np.argwhere(x) * np.asarray(sp)
    cov = np.cov(mm.T, bias=True)
    assert np.allclose(d['covariance'], cov, rtol=1e-12, atol=0) and np.allclose(d['centroid'], mm.mean(axis=0), rtol=1e-12, atol=0)
    lam = np.linalg.eigvalsh(cov)[::-1]
    assert np.allclose(d['principal_moments'], lam, rtol=1e-12, atol=0)
    assert d['major_axis_length'] == 4 * math.sqrt(d['principal_moments'][0]) and 0 < d['flatness'] <= d['elongation'] <= 1
    for lam_k, axis in zip(d['principal_moments'], d['principal_axes']):
        assert np.allclose(cov @ axis, lam_k * axis, rtol=0, atol=1e-10)
    # the calipers: the centre-to-centre width along the physical direction d / s
    for t, dd in enumerate(SR.DIRS):
        u = np.asarray(dd) / np.asarray(sp)
        proj = mm @ (u / np.linalg.norm(u))
        assert abs(d['caliper_widths'][t] - (proj.max() - proj.min())) <= 1e-10
    empty = SR.descriptors_ref(SR.record_ref(np.zeros((3, 3, 3), np.uint8), (1,))[0], sp)
    assert empty['count'] == 0 and math.isnan(empty['sphericity']) and np.isnan(empty['caliper_widths']).all() and empty['euler_6'] == 0


def test_header_declares_hv_shape_and_the_library_exports_it():
    import __graft_entry__ as g
    g.build()
    from hvgan import lib
    _, protos = lib.parse_header()
    assert 'hv_shape' in protos and 'hv_shape_workspace_bytes' in protos
    assert protos['hv_shape'][0] is ctypes.c_int and len(protos['hv_shape'][1]) == 21
    assert protos['hv_shape_workspace_bytes'] == (ctypes.c_size_t, [ctypes.c_int] * 5)
    L = lib.get()
    assert hasattr(L.cdll, 'hv_shape') and hasattr(L.cdll, 'hv_shape_workspace_bytes')
    src = open(lib.HEADER).read()
    assert 'HV_SHAPE_REC = 320' in src and 'HV_SHAPE_STATUS = 292' in src
    # the query is host arithmetic: the per-volume words, and 0 for every refusal
    size = lambda *a: L.size('hv_shape_workspace_bytes', *a)
    assert size(1, 17, 18, 33, 3) == 16 and size(3, 4, 4, 4, 64) == 32
    for bad in ((0, 4, 4, 4, 1), (1, 0, 4, 4, 1), (1, 4, -1, 4, 1), (1, 4, 4, 0, 1), (1, 4, 4, 4, 0), (1, 4, 4, 4, 65), (65536, 4, 4, 4, 1),
                (1, 1 << 11, 1 << 10, (1 << 9) + 1, 1), (1, 1, 1, 1 << 30, 1), (1, 1, 4, 1 << 27, 1)):
        assert size(*bad) == 0, bad
    assert size(1, 1, 1, (1 << 20), 1) == 16                                        # 2^20 * (2^20 - 1)^2 < 2^62
