"""generation_eval.surface_distances / surface_distances_batch (hv_surface_distance, csrc/edt.hip) against the numpy restatement
(tests/surface_ref.py) on volumes of at most 40 x 40 x 24: the counts and hd exact at unit spacing, every distance field within EDT_TOL
(relative) otherwise.

The joined list of the percentile has one entry per surface voxel of either set and both sets must have one, so its shortest length is 2: a
list of length 1 cannot reach the kernel (an empty set raises); the restated rule for n = 1 is pinned in tests/test_surface_ref_cpu.py."""
import math

import numpy as np
import pytest
import torch

import surface_ref as SR
from hvtest import ExactWs

pytestmark = pytest.mark.gpu

FIELDS = ('max_ab', 'max_ba', 'asd_ab', 'asd_ba', 'hd', 'hd95', 'assd')
RAW_AT = {'n_a': 0, 'n_b': 1, 'max_ab': 2, 'max_ba': 3, 'asd_ab': 4, 'asd_ba': 5, 'hd': 6, 'hd95': 7, 'assd': 8}


def _ge():
    import hvgan  # noqa: F401
    from hvgan import generation_eval as GE
    return GE


def _compare(a, b, label=1, spacing=(1.0, 1.0, 1.0), what=''):
    """surface_distances(a, b) against the restatement -> (dict, raw 16 doubles)."""
    GE = _ge()
    got, raw = GE.surface_distances(a, b, label=label, spacing=spacing, return_raw=True)
    ref = SR.metrics(np.asarray(a.cpu() if isinstance(a, torch.Tensor) else a), np.asarray(b.cpu() if isinstance(b, torch.Tensor) else b),
                     label, spacing)
    assert raw.shape == (16,) and raw[9] == 0 and raw[10] == 0 and (raw[11:] == 0).all()
    assert got['n_a'] == ref['n_a'] and got['n_b'] == ref['n_b'], (what, got, ref)
    if SR.is_unit(spacing):
        assert got['hd'] == ref['hd'] and raw[2] == ref['max_ab'] and raw[3] == ref['max_ba'], (what, got, ref)
    for k in FIELDS:
        v = raw[RAW_AT[k]]
        assert abs(v - ref[k]) <= SR.EDT_TOL * ref[k], (what, k, v, ref[k])
        if k in got:
            assert got[k] == v
    print(what, spacing, {k: raw[RAW_AT[k]] for k in FIELDS}, 'n', got['n_a'], got['n_b'])
    return got, raw


def _blobs():
    shape = (40, 36, 24)
    a = SR.blob(shape, (19.0, 17.5, 11.0), (12.0, 9.0, 7.0)).astype(np.uint8)
    b = SR.blob(shape, (21.0, 16.0, 12.5), (10.0, 11.0, 6.0)).astype(np.uint8)
    return a, b


def test_analytic_cases():
    for name, a, b, want in SR.analytic_cases():
        got, raw = _compare(a, b, what=name)
        for k, v in want.items():
            assert raw[RAW_AT[k]] == v, (name, k, raw[RAW_AT[k]], v)


@pytest.mark.parametrize('spacing', SR.SPACINGS, ids=lambda s: 'x'.join(str(v) for v in s))
def test_blobs_faces_and_disjoint_parts(spacing):
    a, b = _blobs()
    _compare(a, b, spacing=spacing, what='two blobs')
    # a set that touches every face of the volume against a blob inside it
    full = np.ones((12, 9, 10), dtype=np.uint8)
    inner = SR.blob((12, 9, 10), (5.5, 4.0, 4.5), (3.0, 2.5, 3.0)).astype(np.uint8)
    got, _ = _compare(full, inner, spacing=spacing, what='every face')
    assert got['n_a'] == 12 * 9 * 10 - 10 * 7 * 8
    _compare(inner, full, spacing=spacing, what='every face, swapped')
    # two disjoint blobs against one, other labels around
    shape = (40, 30, 20)
    two = (SR.blob(shape, (8.0, 9.0, 8.0), (5.0, 6.0, 4.0)) | SR.blob(shape, (30.0, 20.0, 12.0), (6.0, 5.0, 5.0))).astype(np.uint8) * 2
    one = SR.blob(shape, (18.0, 14.0, 10.0), (7.0, 6.0, 5.0)).astype(np.uint8) * 2
    two[two == 0] = 1
    one[:3] = 3
    got, _ = _compare(two, one, label=2, spacing=spacing, what='disjoint')
    assert got['hd'] > got['hd95'] > got['assd'] > 0


def test_a_blob_against_itself_shifted_by_one_voxel():
    a, _ = _blobs()
    for axis in range(3):
        b = np.zeros_like(a)
        dst = [slice(None)] * 3
        src = [slice(None)] * 3
        dst[axis], src[axis] = slice(1, None), slice(None, -1)
        b[tuple(dst)] = a[tuple(src)]
        for sp in (SR.SPACINGS[0], SR.SPACINGS[1]):
            got, _ = _compare(a, b, spacing=sp, what='shift along %d' % axis)
            assert got['hd'] == sp[axis] and got['n_a'] == got['n_b'] and 0 < got['assd'] < sp[axis]


def test_the_edges_of_the_percentile():
    shape = (6, 7, 9)
    one = np.zeros(shape, dtype=np.uint8)
    one[1, 2, 3] = 1
    other = np.zeros(shape, dtype=np.uint8)
    other[4, 4, 7] = 1
    got, _ = _compare(one, other, what='list of 2')                       # v = 0.95: between the two equal entries
    assert got['hd95'] == got['hd'] == math.sqrt(29.0)
    pair = other.copy()
    pair[1, 2, 5] = 1
    got, raw = _compare(one, pair, what='list of 3')                      # entries {2, sqrt(29), 2}: v = 1.9
    assert got['n_b'] == 2 and raw[2] == 2.0 and raw[3] == math.sqrt(29.0)
    block = np.zeros(shape, dtype=np.uint8)
    block[3:5, 2:4, 2:7] = 1                                              # 2 x 2 x 5: all 20 voxels are surface
    got, _ = _compare(one, block, what='list of 21')                      # v = 19.0 exactly: t = 0
    assert got['n_a'] + got['n_b'] == 21
    block[3:5, 2:4, 7] = 1                                                # 24 + 1: v = 22.8
    _compare(block, one, what='list of 25')


def test_box_restricted_equals_whole_volume_and_batch_equals_single(monkeypatch):
    GE = _ge()
    a, b = _blobs()
    small = [c for c in SR.analytic_cases()]
    pairs = [(a, b, 1), (small[1][1], small[1][2], 1), (torch.from_numpy(b).cuda(), torch.from_numpy(a).cuda(), 1), (small[2][1], small[2][2], 1)]
    for sp in (SR.SPACINGS[0], SR.SPACINGS[2]):
        raws = []
        for x, y, lab in pairs:
            _, boxed = GE.surface_distances(x, y, label=lab, spacing=sp, return_raw=True)
            _, whole = GE.surface_distances(x, y, label=lab, spacing=sp, restrict=False, return_raw=True)
            _, again = GE.surface_distances(x, y, label=lab, spacing=sp, return_raw=True)
            assert boxed.tobytes() == whole.tobytes() == again.tobytes()
            raws.append(boxed)
        ws = ExactWs(monkeypatch, required=True)                          # exactly hv_surface_distance_workspace_bytes, nothing outside
        batch = GE.surface_distances_batch(pairs, spacing=sp)
        back = GE.surface_distances_batch(pairs[::-1], spacing=sp)
        ws.close()
        assert len(batch) == len(back) == len(pairs)
        for i, raw in enumerate(raws):
            for res in (batch[i], back[len(pairs) - 1 - i]):
                assert set(res) == set(GE.SURFACE_KEYS)
                for k in GE.SURFACE_KEYS:
                    assert np.float64(res[k]).tobytes() == np.float64(raw[RAW_AT[k]]).tobytes(), (i, k)
    assert batch[0]['hd'] == batch[2]['hd'] and batch[0]['asd_ab'] == batch[2]['asd_ba']


def test_label_dtypes_and_a_strided_view():
    GE = _ge()
    a, b = _blobs()
    a, b = a[4:36, 2:34, 2:22] * 2, b[4:36, 2:34, 2:22] * 2
    sp = SR.SPACINGS[1]
    _, want = _compare(a, b, label=2, spacing=sp, what='uint8')
    for dt in (np.float32, np.float64, np.int16):
        _, raw = GE.surface_distances(a.astype(dt), b.astype(dt), label=2, spacing=sp, return_raw=True)
        assert raw.tobytes() == want.tobytes(), dt
    big = torch.full((2, 32, 34, 40), float('nan'), dtype=torch.float32, device='cuda')
    va, vb = big[0, :, 1:-1:1, ::2][:, :32], big[1, :, 1:-1:1, ::2][:, :32]
    va.copy_(torch.from_numpy(a.astype(np.float32)))
    vb.copy_(torch.from_numpy(b.astype(np.float32)))
    assert not va.is_contiguous() and va.stride() == vb.stride()
    keep = big.clone()
    _, raw = GE.surface_distances(va, vb, label=2, spacing=sp, return_raw=True)
    assert raw.tobytes() == want.tobytes()
    assert torch.equal(big.view(torch.int32), keep.view(torch.int32)), 'a device input was modified'


def test_an_empty_set_raises_with_the_flags_in_the_raw_output():
    GE = _ge()
    a, _ = _blobs()
    none = np.zeros_like(a)
    for x, y, fa, fb in ((a, none, 0.0, 1.0), (none, a, 1.0, 0.0), (none, none, 1.0, 1.0)):
        for restrict in (True, False):
            res, raw = GE.surface_distances(x, y, restrict=restrict, return_raw=True)
            assert res is None and raw[9] == fa and raw[10] == fb and np.isnan(raw[2:9]).all()
            assert raw[0] == (0 if fa else SR.surface(a == 1).sum()) and raw[1] == (0 if fb else SR.surface(a == 1).sum())
            with pytest.raises(ValueError):
                GE.surface_distances(x, y, restrict=restrict)
    with pytest.raises(ValueError, match='pair 1'):
        GE.surface_distances_batch([(a, a, 1), (a, none, 1)])
    with pytest.raises(ValueError):
        GE.surface_distances(a, a, label=7)
