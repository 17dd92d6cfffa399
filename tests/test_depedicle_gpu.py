"""De-pedicling on the device (hvgan.straighten.depedicle / component_counts / single_component_range: csrc/depedicle.hip) against the
reference's own results in fixture G17 (tools/make_golden_depedicle.py) and the plain-numpy restatement (tests/depedicle_ref.py).  All
outputs are integers: every comparison is exact.  Shapes are the smallest at which the kernel can still go wrong (slices off the 1024-lane
grid, one or several 4096-pixel register words per lane, the 65 536-pixel LDS limit), not the workload's 256 x 256 x 64."""
import ctypes

import numpy as np
import pytest
import torch

import depedicle_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu


def _S():
    import hvgan  # noqa: F401
    from hvgan import straighten as S
    return S


def _g(name):
    cases = {}
    for k, v in load_golden(name).items():
        a, b = k.split('/')
        cases.setdefault(a, {})[b] = v.numpy()
    return cases


def _run(vol, **kw):
    """numpy / tensor volume -> (de-pedicled numpy, counts numpy)"""
    S = _S()
    t = vol if torch.is_tensor(vol) else torch.from_numpy(np.ascontiguousarray(vol)).cuda()
    out = S.depedicle(t, **kw)
    counts = S.component_counts(t)
    torch.cuda.synchronize()
    assert out.dtype == torch.uint8 and out.is_cuda and counts.dtype == torch.int32
    return out.cpu().numpy(), counts.cpu().numpy()


def _check_ref(vol):
    out, counts = _run(vol)
    ref_out, ref_counts = R.depedicle(vol)
    assert np.array_equal(out, ref_out)
    assert np.array_equal(counts, ref_counts)
    return out, counts


def test_g17_volumes_counts_and_ranges():
    S = _S()
    for name, c in _g('g17_depedicle').items():
        out, counts = _run(c['in'])
        assert np.array_equal(out, c['out']), name
        assert np.array_equal(counts, c['counts']), name
        t = torch.from_numpy(c['in']).cuda()
        for l, z0, z1 in c['ranges']:
            assert S.single_component_range(t, int(l)) == (z0, z1), (name, l)
            assert S.single_component_range(t, int(l), offset=2) == R.single_component_range(c['counts'], l, 2), (name, l)


def test_straighten_patient_option_equals_depedicle_of_its_default_result():
    S = _S()
    for name, c in _g('g13_straighten').items():
        ct, label = torch.from_numpy(c['ct']).cuda(), torch.from_numpy(c['label']).cuda()
        ids, size = [int(v) for v in c['ids']], tuple(int(s) for s in c['out_size'])
        plain = S.straighten_patient(ct, label, ids, out_size=size)
        cut = S.straighten_patient(ct, label, ids, out_size=size, depedicle=True)
        torch.cuda.synchronize()
        for k, v in enumerate(ids):
            assert torch.equal(plain[v][1].cpu(), torch.from_numpy(c['crop_label'][k])), (name, v)      # the default still equals G13
            assert torch.equal(cut[v][0], plain[v][0]), (name, v)
            assert torch.equal(cut[v][1], S.depedicle(plain[v][1])), (name, v)
            assert np.array_equal(cut[v][1].cpu().numpy(), R.depedicle(plain[v][1].cpu().numpy())[0]), (name, v)


@pytest.mark.parametrize('shape', [(1, 1), (1, 9), (9, 1), (5, 7)])
@pytest.mark.parametrize('Z', [1, 3])
def test_shapes_off_the_lane_grid(shape, Z):
    rng = np.random.default_rng(shape[0] * 100 + shape[1] * 10 + Z)
    for fill in (1.0, 0.6):
        vol = (rng.integers(1, 3, shape + (Z,)) * (rng.random(shape + (Z,)) < fill)).astype(np.uint8)
        _check_ref(vol)


def test_lds_limit_root_65535_and_full_slice():
    vol = np.zeros((256, 256, 2), np.uint8)
    vol[0, 0, 0] = vol[255, 255, 0] = 9              # raster indices 0 and 65535 of one value: index 0 (column 0) wins
    vol[:, :, 1] = 200                               # one component of 65 536 pixels
    out, counts = _run(vol)
    exp = vol.copy()
    exp[255, 255, 0] = 0
    assert np.array_equal(out, exp)
    assert counts[0, 9] == 2 and counts[1, 200] == 1 and counts.sum() == 3
    vol = np.zeros((256, 256, 1), np.uint8)          # 65535 alone is a root like any other, and survives
    vol[255, 255, 0] = 9
    out, counts = _run(vol)
    assert np.array_equal(out, vol) and counts[0, 9] == 1 and counts.sum() == 1
    vol = np.zeros((1, 65536, 1), np.uint8)          # the largest axis-1 index a slice can have
    vol[0, 65535, 0], vol[0, 100:200, 0] = 3, 4
    out, counts = _run(vol)
    assert np.array_equal(out, vol) and counts[0, 3] == 1 and counts[0, 4] == 1


def test_above_the_limit_is_refused_before_launch():
    S = _S()
    from hvgan import lib as L
    lib = L.get()
    vol = torch.ones(257, 256, 1, dtype=torch.uint8, device='cuda')
    out = torch.full((257, 256, 1), 0xA5, dtype=torch.uint8, device='cuda')
    counts = torch.full((1, 1, 256), -7, dtype=torch.int32, device='cuda')
    status = torch.full((1,), -7, dtype=torch.int32, device='cuda')
    z = [ctypes.c_longlong(0)] * 4
    rc = lib.cdll.hv_depedicle(L.ptr(vol), 0, 256, 1, 1, 0, 257, 256, 1, 1, L.ptr(out), 256, 1, 1, 0, L.ptr(counts), L.ptr(status), L.stream())
    torch.cuda.synchronize()
    assert rc == -2
    assert bool((out == 0xA5).all()) and bool((counts == -7).all()) and int(status[0]) == -7
    rc = lib.cdll.hv_depedicle(L.ptr(vol), 0, *z, 1, 1, 1, 65536, L.ptr(out), *z, None, L.ptr(status), L.stream())    # V past the grid limit
    assert rc == -2 and bool((out == 0xA5).all())
    with pytest.raises(RuntimeError, match='UNSUPPORTED'):
        S.depedicle(vol, out=out)
    assert bool((out == 0xA5).all())


def _mirrors(a):
    return [a, a[::-1], a[:, ::-1], a[::-1, ::-1], a.T, a.T[::-1], a.T[:, ::-1], a.T[::-1, ::-1]]


def test_worst_cases_converge():
    for base in (R.spiral(63), R.comb(64, 31)):
        vol = np.ascontiguousarray(np.stack(_mirrors(base), axis=2)) * np.uint8(6)
        out, counts = _run(vol)                       # a not-converged slice would raise RuntimeError
        assert np.array_equal(out, vol)
        assert (counts[:, 6] == 1).all() and counts.sum() == vol.shape[2]
    big = np.zeros((255, 255, 2), np.uint8)           # the longest one-pixel-wide path a slice can hold, and its transpose
    big[:, :, 0] = R.spiral(255)
    big[:, :, 1] = R.spiral(255).T[::-1]
    out, counts = _run(big)
    assert np.array_equal(out, big) and (counts[:, 1] == 1).all() and counts.sum() == 2


def test_connectivity_is_four_and_values_do_not_merge():
    a = np.zeros((8, 9, 2), np.uint8)
    a[1:3, 3:5, 0], a[3:5, 1:3, 0] = 5, 5             # corner contact only: two components, the one reaching column 1 stays
    a[1:4, 1:4, 1], a[4:7, 1:4, 1] = 3, 4             # different values sharing an edge
    a[1:3, 6:8, 1], a[5:7, 6:8, 1] = 3, 4             # ... each with a detached piece further right
    out, counts = _check_ref(a)
    assert counts[0, 5] == 2 and (out[1:3, 3:5, 0] == 0).all() and (out[3:5, 1:3, 0] == 5).all()
    assert counts[1, 3] == 2 and counts[1, 4] == 2
    assert (out[1:4, 1:4, 1] == 3).all() and (out[4:7, 1:4, 1] == 4).all() and (out[:, 6:8, 1] == 0).all()


def test_tie_breaks():
    a = np.zeros((9, 9, 2), np.uint8)
    a[1, 2:5, 0], a[4:6, 2:4, 0] = 7, 7               # equal smallest column: the smaller raster root (row 1) survives
    a[1, 4:8, 1], a[5:7, 1:3, 1] = 7, 7               # the later component reaches column 1: it survives over the earlier one
    out, counts = _check_ref(a)
    assert (out[1, 2:5, 0] == 7).all() and (out[4:6, :, 0] == 0).all()
    assert (out[1, :, 1] == 0).all() and (out[5:7, 1:3, 1] == 7).all()
    assert counts[0, 7] == 2 and counts[1, 7] == 2


def test_values():
    a = np.zeros((10, 12, 3), np.uint8)
    a[0:3, 0:3, 0], a[0:2, 6:8, 0], a[5:9, 1:4, 0], a[6:8, 6:10, 0] = 1, 1, 255, 255
    for k, v in enumerate((2, 3, 50, 51, 127, 128, 254, 255)):      # 8 values, each twice: one piece at column 0, one further right
        a[k, 0:2, 2] = v
        a[k, 5 + (k % 3):8, 2] = v
    out, counts = _check_ref(a)                       # slice 1 stays all zero
    assert counts[0, 1] == 2 and counts[0, 255] == 2 and counts[0, 2] == 0 and counts[1].sum() == 0 and (out[:, :, 1] == 0).all()
    assert (counts[2][[2, 3, 50, 51, 127, 128, 254, 255]] == 2).all() and (out[:8, 5:, 2] == 0).all()


def test_layouts_and_dtypes_give_the_same_bits():
    S = _S()
    vol = _g('g17_depedicle')['edge1']['in']
    ref = _g('g17_depedicle')['edge1']['out']
    base = torch.from_numpy(vol).cuda()
    variants = {'contiguous': base, 'fortran': torch.from_numpy(np.asfortranarray(vol)).cuda()}
    assert variants['fortran'].stride()[0] == 1
    wide = torch.zeros(tuple(2 * s for s in vol.shape), dtype=torch.uint8, device='cuda')
    wide[::2, ::2, ::2] = base
    variants['view'] = wide[::2, ::2, ::2]
    assert not variants['view'].is_contiguous()
    for dt in (torch.int16, torch.int32, torch.int64, torch.float32, torch.float64):
        variants[str(dt)] = base.to(dt)
    for name, t in variants.items():
        out, counts = _run(t)
        assert np.array_equal(out, ref), name
        assert np.array_equal(counts, _g('g17_depedicle')['edge1']['counts']), name
    inplace = base.clone()
    assert S.depedicle(inplace, out=inplace) is inplace
    assert np.array_equal(inplace.cpu().numpy(), ref)
    view_out = torch.zeros_like(wide)                 # strided output
    S.depedicle(base, out=view_out[1::2, 1::2, 1::2])
    assert np.array_equal(view_out[1::2, 1::2, 1::2].cpu().numpy(), ref) and int(view_out[::2].sum()) == 0


def test_batch_equals_single_calls_and_a_bad_volume_stays_alone():
    S = _S()
    from hvgan import lib as L
    g = _g('g17_depedicle')
    vols = [g[n]['in'] for n in ('curved0', 'curved1', 'edge0')]
    batch = torch.from_numpy(np.stack(vols)).cuda()
    out, counts = _run(batch)
    for k, n in enumerate(('curved0', 'curved1', 'edge0')):
        assert np.array_equal(out[k], g[n]['out']) and np.array_equal(counts[k], g[n]['counts']), n
    bad = batch.to(torch.float32)
    bad[1, 20, 20, 3] = 2.5
    with pytest.raises(ValueError):
        S.depedicle(bad)
    o = torch.zeros(batch.shape, dtype=torch.uint8, device='cuda')
    cn = torch.zeros(3, 16, 256, dtype=torch.int32, device='cuda')
    st = torch.zeros(3, dtype=torch.int32, device='cuda')
    s = [ctypes.c_longlong(x) for x in bad.stride()]
    so = [ctypes.c_longlong(x) for x in o.stride()]
    rc = L.get().cdll.hv_depedicle(L.ptr(bad), 4, s[1], s[2], s[3], s[0], 48, 40, 16, 3, L.ptr(o), so[1], so[2], so[3], so[0], L.ptr(cn), L.ptr(st),
                                   L.stream())
    torch.cuda.synchronize()
    assert rc == 0 and st.tolist() == [0, 1, 0]
    for k, n in ((0, 'curved0'), (2, 'edge0')):
        assert np.array_equal(o[k].cpu().numpy(), g[n]['out']) and np.array_equal(cn[k].cpu().numpy(), g[n]['counts']), n


def test_argument_errors_and_bad_values():
    S = _S()
    from hvgan import lib as L
    fn = L.get().cdll.hv_depedicle
    vol = torch.ones(4, 4, 2, dtype=torch.uint8, device='cuda')
    out = torch.full((4, 4, 2), 0xA5, dtype=torch.uint8, device='cuda')
    cn = torch.zeros(1, 2, 256, dtype=torch.int32, device='cuda')
    st = torch.zeros(1, dtype=torch.int32, device='cuda')

    def call(label=vol, dt=0, A0=4, A1=4, Z=2, V=1, o=out, c=cn, s=st):
        return fn(L.ptr(label), dt, 8, 2, 1, 32, A0, A1, Z, V, L.ptr(o), 8, 2, 1, 32, L.ptr(c), L.ptr(s), L.stream())
    assert call(label=None) == -1 and call(s=None) == -1 and call(o=None, c=None) == -1
    assert call(dt=-1) == -1 and call(dt=6) == -1
    assert call(A0=0) == -1 and call(A1=-1) == -1 and call(Z=0) == -1 and call(V=0) == -1
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())
    assert call() == 0 and call(o=None) == 0                                     # the same arguments are accepted; counts-only form
    torch.cuda.synchronize()
    assert bool((out == 1).all()) and cn[0, :, 1].tolist() == [1, 1]
    for bad in (vol.to(torch.float64) * 0.5, vol.to(torch.int16) * 256, vol.to(torch.int32) * -1, vol.to(torch.float32) * float('nan')):
        with pytest.raises(ValueError):
            S.depedicle(bad)
        with pytest.raises(ValueError):
            S.component_counts(bad)
    with pytest.raises(ValueError):
        S.depedicle(vol[0])                                                      # rank 2
    with pytest.raises(ValueError):
        S.depedicle(vol, out=torch.zeros(4, 4, 3, dtype=torch.uint8, device='cuda'))
    with pytest.raises(ValueError):
        S.single_component_range(vol.unsqueeze(0), 1)
    with pytest.raises(TypeError):
        S.depedicle(vol.to(torch.float16))
    assert np.array_equal(S.depedicle(vol).cpu().numpy(), np.ones((4, 4, 2), np.uint8))   # a following call succeeds


def test_two_runs_give_identical_bytes():
    rng = np.random.default_rng(5)
    vol = (rng.integers(1, 4, (96, 80, 4)) * (rng.random((96, 80, 4)) < 0.62)).astype(np.uint8)     # near the percolation threshold: many
    a, ca = _run(vol)                                                                                # ragged components, 7 680 pixels a slice
    b, cb = _run(vol)
    assert a.tobytes() == b.tobytes() and ca.tobytes() == cb.tobytes()
    ref_out, ref_counts = R.depedicle(vol)
    assert np.array_equal(a, ref_out) and np.array_equal(ca, ref_counts)
