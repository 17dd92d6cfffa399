"""What needs no GPU of the 3-D connected components (csrc/ccl3d.hip, healthivert-gan_amd/components.py): the
numpy restatement of the device's scheme (tests/ccl_ref.py) against scipy, the numbering and hole-fill identities the kernels rest on, the
filter rules, the host-only entries and the wrappers' argument checks."""
import ctypes

import numpy as np
import pytest
from scipy.ndimage import binary_fill_holes

import ccl_ref as CR

NEW = ('hv_label3d_workspace_bytes', 'hv_label3d_tile', 'hv_label3d', 'hv_clean_components', 'hv_fill_holes')


def _device_tile():
    import hvgan  # noqa: F401
    from hvgan import lib
    if not lib.available():
        pytest.skip('libhvgan.so not built')
    dims = (ctypes.c_int * 3)()
    assert lib.get().cdll.hv_label3d_tile(dims) == 0
    return tuple(dims)


@pytest.mark.parametrize('connectivity', (1, 2, 3))
@pytest.mark.parametrize('density', (0.2, 0.5, 0.8))
def test_restatement_equals_scipy(density, connectivity):
    for tile, shape in (((2, 2, 2), (5, 6, 7)), ((1, 3, 5), (4, 7, 11))):
        m = CR.random_mask(shape, density, 10 * connectivity + int(10 * density))
        lab, n = CR.restate(m, connectivity, tile)
        ref, rn = CR.label(m, connectivity)
        assert n == rn and np.array_equal(lab, ref), (tile, shape)


@pytest.mark.parametrize('connectivity', (1, 2, 3))
def test_restatement_with_the_devices_tile_equals_scipy(connectivity):
    T = _device_tile()
    shape = (T[0] + 1, T[1] + 1, T[2] + 2)
    for density in (0.2, 0.5, 0.8):
        m = CR.random_mask(shape, density, 7 + connectivity)
        lab, n = CR.restate(m, connectivity, T)
        ref, rn = CR.label(m, connectivity)
        assert n == rn and np.array_equal(lab, ref), density


def test_scipy_numbers_components_by_their_smallest_raster_index():
    for seed in range(6):
        for c in (1, 2, 3):
            m = CR.random_mask((6, 7, 8), (0.15, 0.3, 0.45)[seed % 3], 100 + seed)
            lab, n = CR.label(m, c)
            first = [int(np.flatnonzero(lab.ravel() == i)[0]) for i in range(1, n + 1)]
            assert first == sorted(first)
    assert len(CR.backward_offsets(1)) == 3 and len(CR.backward_offsets(2)) == 9 and len(CR.backward_offsets(3)) == 13


def test_fill_holes_is_the_complement_of_the_border_components_of_the_complement():
    for seed in range(6):
        m = CR.random_mask((7, 8, 9), 0.6 + 0.05 * (seed % 3), 200 + seed)
        lab, n = CR.label(~m, 1)
        border = np.zeros(n + 1, dtype=bool)
        for face in (lab[0], lab[-1], lab[:, 0], lab[:, -1], lab[:, :, 0], lab[:, :, -1]):
            border[np.unique(face)] = True
        border[0] = False
        assert np.array_equal(binary_fill_holes(m), ~border[lab])
        out, holes, voxels = CR.fill_holes(m.astype(np.uint8), 1)
        assert np.array_equal(out == 1, binary_fill_holes(m)) and holes == n - border.sum() and voxels == (out != m).sum()


def test_largest_tie_goes_to_the_lowest_label_and_min_size_keeps_the_exact_size():
    v = np.zeros((3, 9, 9), dtype=np.uint8)
    v[0, 0, 0:3] = 5          # label 1: 3 voxels
    v[1, 4, 0:4] = 5          # label 2: 4 voxels
    v[2, 8, 2:6] = 5          # label 3: 4 voxels, the tie
    v[2, 0, 0] = 7
    lab, t = CR.table(v == 5, 1, cap=2)
    assert list(t) == [3, 2, 4, 0, 3, 4]
    out, _ = CR.clean(v, 5, keep_largest=True)
    assert (out == 5).sum() == 4 and (out[1] == 5).sum() == 4 and out[2, 0, 0] == 7
    # the reference's rule: np.sum(labeled == i) < min_size is dropped, so a component of exactly min_size voxels stays
    for min_size, left in ((3, 11), (4, 8), (5, 0), (0, 11), (1, 11)):
        out, _ = CR.clean(v, 5, min_size=min_size, keep_largest=False, fill=9)
        want = v.copy()
        for i in range(1, 4):
            if min_size > 1 and np.sum(lab == i) < min_size:
                want[lab == i] = 9
        assert np.array_equal(out, want) and (out == 5).sum() == left, min_size
    assert list(CR.table(np.zeros((2, 2, 2), dtype=bool), 1, cap=1)[1]) == [0, 0, 0, 1, 0]


def test_serpentine_is_one_path_from_index_zero():
    m, count = CR.serpentine((6, 8, 10))
    lab, n = CR.label(m, 1)
    assert n == 1 and m.ravel()[0] and count == m.sum()
    # a path: every voxel has two face neighbours on it but the two ends
    pad = np.pad(m, 1).astype(int)
    nb = sum(np.roll(pad, s, a) for a in range(3) for s in (-1, 1))[1:-1, 1:-1, 1:-1]
    assert sorted(np.unique(nb[m])) == [1, 2] and (nb[m] == 1).sum() == 2 and nb[0, 0, 0] == 1


def test_header_declares_the_entries_and_the_host_entries_answer():
    import hvgan  # noqa: F401
    from hvgan import lib
    _, protos = lib.parse_header()
    for name in NEW:
        assert name in protos, name
    assert protos['hv_label3d_workspace_bytes'] == (ctypes.c_size_t, [ctypes.c_int] * 3)
    assert len(protos['hv_label3d'][1]) == 17 and len(protos['hv_clean_components'][1]) == 22 and len(protos['hv_fill_holes'][1]) == 19
    T = _device_tile()
    assert len(T) == 3 and all(t >= 1 for t in T) and T[2] == max(T) and T[0] * T[1] * T[2] <= 65536
    L = lib.get()
    for name in NEW:
        assert hasattr(L.cdll, name)
    assert L.cdll.hv_label3d_tile(None) == -1
    up = lambda b: (b + 15) // 16 * 16
    n = 5 * 7 * 9
    assert L.size('hv_label3d_workspace_bytes', 5, 7, 9) == 2 * up(4 * n) + up(4 * (n + 1)) + up(4 * ((n + 1023) // 1024)) + 16
    assert L.size('hv_label3d_workspace_bytes', 0, 7, 9) == 0 and L.size('hv_label3d_workspace_bytes', 5, 7, -1) == 0
    assert L.size('hv_label3d_workspace_bytes', 1024, 1024, 1025) >= 12 * 1024 * 1024 * 1025


def test_entries_refuse_before_any_launch():
    """Refusals come before any device work, so they can be called here with made-up pointers."""
    import hvgan  # noqa: F401
    from hvgan import lib
    if not lib.available():
        pytest.skip('libhvgan.so not built')
    L = lib.get()
    p, q = ctypes.c_void_p(4096), ctypes.c_void_p(8192)
    ll = [ctypes.c_longlong(s) for s in (63, 9, 1)]
    big = ctypes.c_size_t(1 << 40)

    def lab(vol=p, dt=0, dims=(5, 7, 9), mode=0, c=1, labels=q, table=q, cap=0, w=p, wb=big):
        return L.cdll.hv_label3d(vol, dt, *ll, *dims, ctypes.c_double(1.0), mode, c, labels, table, cap, w, wb, None)

    def clean(vol=p, dt=0, dims=(5, 7, 9), mode=0, c=1, ms=0, kl=1, out=q, os=(63, 9, 1), table=q, w=p, wb=big):
        return L.cdll.hv_clean_components(vol, dt, *ll, *dims, ctypes.c_double(1.0), mode, c, ms, kl, ctypes.c_double(0.0), out,
                                          *[ctypes.c_longlong(s) for s in os], table, w, wb, None)

    def fill(vol=p, dt=0, dims=(5, 7, 9), mode=0, out=q, os=(63, 9, 1), table=q, w=p, wb=big):
        return L.cdll.hv_fill_holes(vol, dt, *ll, *dims, ctypes.c_double(1.0), mode, ctypes.c_double(1.0), out,
                                    *[ctypes.c_longlong(s) for s in os], table, w, wb, None)

    need = L.size('hv_label3d_workspace_bytes', 5, 7, 9)
    common = (dict(vol=None), dict(table=None), dict(w=None), dict(dt=1), dict(dt=6), dict(dt=-1), dict(dims=(0, 7, 9)), dict(dims=(5, 7, -9)),
              dict(mode=2), dict(mode=-1), dict(w=ctypes.c_void_p(4104)), dict(wb=ctypes.c_size_t(need - 1)), dict(table=ctypes.c_void_p(8194)))
    for kw in common + (dict(c=0), dict(c=4), dict(labels=None), dict(cap=-1), dict(labels=ctypes.c_void_p(8193))):
        assert lab(**kw) == -1, kw
    for kw in common + (dict(c=0), dict(c=4), dict(kl=2), dict(kl=-1), dict(out=None), dict(out=p, os=(1, 5, 35))):
        assert clean(**kw) == -1, kw
    for kw in common + (dict(out=None), dict(out=p, os=(1, 5, 35))):
        assert fill(**kw) == -1, kw
    # more than 2^30 voxels: refused on the sizes alone
    for fn in (lab, clean, fill):
        assert fn(dims=(1024, 1024, 1025)) == -2
        assert fn(dims=(1 << 15, 1 << 15, 2)) == -2


def test_wrappers_check_their_arguments_before_touching_the_device():
    import hvgan  # noqa: F401
    from hvgan import components as C
    from hvgan import generation_eval as GE
    import torch
    v = np.zeros((4, 5, 6), dtype=np.uint8)
    for bad in (np.zeros((4, 5), dtype=np.uint8), np.zeros((2, 3, 4, 5), dtype=np.uint8)):
        for fn in (lambda x: C.label(x), lambda x: C.component_sizes(x), lambda x: C.clean_label(x, 1), lambda x: C.fill_holes(x, 1),
                   lambda x: C.keep_largest_component(x, 1), lambda x: C.remove_small_components(x, 1, 5), lambda x: C.clean_labels([x], 1)):
            with pytest.raises(ValueError, match='3-D'):
                fn(bad)
    for c in (0, 4, -1, 1.0, '1', None, True):
        with pytest.raises(ValueError, match='connectivity'):
            C.label(v, connectivity=c)
        with pytest.raises(ValueError, match='connectivity'):
            C.clean_label(v, 1, connectivity=c)
        with pytest.raises(ValueError, match='connectivity'):
            C.clean_labels([v, v], [1, 1], connectivity=c)
        with pytest.raises(ValueError, match='connectivity'):
            GE.surface_distances(v, v, largest_component=True, connectivity=c)
        with pytest.raises(ValueError, match='connectivity'):
            GE.surface_distances_batch([(v, v, 1)], largest_component=True, connectivity=c)
    for ms in (-1, 2.5, '3', None, True):
        with pytest.raises(ValueError, match='min_size'):
            C.remove_small_components(v, 1, ms)
        with pytest.raises(ValueError, match='min_size'):
            C.clean_label(v, 1, min_size=ms)
    for val in (None, 'a', True, [1]):
        with pytest.raises(ValueError, match='value'):
            C.clean_label(v, val)
        with pytest.raises(ValueError, match='value'):
            C.fill_holes(v, val)
    with pytest.raises(ValueError, match='value'):
        C.label(v, value='a')
    with pytest.raises(ValueError, match='max_components'):
        C.label(v, max_components=-1)
    for out in (np.zeros((4, 5, 6), dtype=np.int32), torch.zeros(4, 5, 6), torch.zeros(4, 5, 7, dtype=torch.int32),
                torch.zeros(6, 5, 4, dtype=torch.int32).permute(2, 1, 0)):
        with pytest.raises(ValueError, match='out'):
            C.label(v, out=out)
    for out in (np.zeros((4, 5, 6), dtype=np.uint8), torch.zeros(4, 5, 6), torch.zeros(4, 5, 7, dtype=torch.uint8)):
        with pytest.raises(ValueError, match='out'):
            C.clean_label(v, 1, out=out)
        with pytest.raises(ValueError, match='out'):
            C.fill_holes(v, 1, out=out)
    with pytest.raises(ValueError, match='values'):
        C.clean_labels([v, v], [1])
