"""hv_glrlm and hv_gldm (csrc/texture_runs.hip) and healthivert-gan_amd/texture_runs.py against tests/texture_runs_ref.py (pinned against brute
forces and the pyradiomics documentation's examples by tests/test_texture_runs_ref_cpu.py).  Everything the entries write is an integer count or a
status word: out, dep, ngt and info are compared bit for bit.  The outputs lie between guard words and are pre-filled with 0xA5 bytes, the
workspace is exactly the queried bytes inside a 0xA5 border.  A workgroup covers 2048 voxels of the code volume, 256 at a time: (17, 16, 33) and
(3, 18, 130) take several workgroups, and runs cross their borders in every direction."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import labelstats_ref as LR
import texture_runs_ref as RR
from hvtest import ExactWs, Guarded

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED = -1, -2
_VDT = {torch.uint8: 0, torch.int16: 1, torch.float32: 4, torch.float64: 5}
_LDT = {torch.uint8: 0, torch.int16: 1, torch.int32: 2, torch.int64: 3, torch.float32: 4, torch.float64: 5}
D13 = RR.directions13()
NEG13 = [tuple(-c for c in d) for d in D13]
SHAPES = ((1, 1, 1), (1, 1, 70), (5, 1, 1), (17, 16, 33), (3, 18, 130))
EDGE, LONG = (17, 16, 33), (3, 18, 130)
LO, WIDTH, G = -20.0, 40.0, 8                  # levels of _intensities: 0 .. 5 in blocks, both clamps met


def _lib():
    import hvgan  # noqa: F401
    from hvgan import lib
    return lib, lib.get()


def _R():
    import hvgan  # noqa: F401
    from hvgan import texture_runs
    return texture_runs


def _dev(a):
    return torch.from_numpy(np.array(a, order='C')).cuda()


class _Ws:
    """Exactly `need` bytes, 16-byte aligned (+ off), inside a border of `fill` bytes."""

    def __init__(self, need, fill=0xA5, off=0):
        self.need, self.fill, self.off = need, fill, off
        self.big = torch.full((512 + need + off,), fill, dtype=torch.uint8, device='cuda')
        assert self.big[256:].data_ptr() % 16 == 0
        self.ptr = ctypes.c_void_p(self.big[256:].data_ptr() + off)

    def border_intact(self):
        lo, hi = self.big[:256 + self.off], self.big[256 + self.off + self.need:]
        return bool((lo == self.fill).all()) and bool((hi == self.fill).all())

    def untouched(self):
        return bool((self.big == self.fill).all())


def _ll(st):
    return [ctypes.c_longlong(s) for s in st]


def _st4(t):
    return tuple(t.stride()) if t.dim() == 4 else (0,) + tuple(t.stride())


def _sizes(vol, lab, labels, over):
    shape = tuple(int(s) for s in vol.shape)
    V, A = (shape[0], shape[1:]) if len(shape) == 4 else (1, shape)
    a = dict(V=V, A0=A[0], A1=A[1], A2=A[2], S=len(labels), vol_dtype=_VDT[vol.dtype], label_dtype=_LDT[lab.dtype])
    a.update({k: v for k, v in over.items() if k in a})
    return V, A, a


def _front(lib, vol, lab, mask, labels, a, over):
    """The arguments both entries share with hv_glcm, up to S."""
    nul = ctypes.c_void_p(None)
    return [nul if over.get('vol_null') else lib.ptr(vol), a['vol_dtype'], *_ll(_st4(vol)),
            nul if over.get('label_null') else lib.ptr(lab), a['label_dtype'], *_ll(_st4(lab)),
            lib.ptr(mask), *_ll(_st4(mask) if mask is not None else (0, 0, 0, 0)), a['V'], a['A0'], a['A1'], a['A2'],
            None if over.get('labels_null') else (ctypes.c_int * max(len(labels), 1))(*labels), a['S']]


def _guarded(shape, prefill):
    g = Guarded(shape, torch.int64)
    if prefill is not None:
        g.t.view(torch.uint8).fill_(prefill)
    return g


def _out_ptr(g, over, name):
    return ctypes.c_void_p(None) if over.get(name + '_null') else ctypes.c_void_p(g.t.data_ptr() + over.get(name + '_off', 0))


def _glrlm(vol, lab, labels, offsets, lo, width, levels, R, mask=None, ws=None, ws_bytes=None, prefill=None, **over):
    """One hv_glrlm on device tensors (3-D, or 4-D stacked) -> (return code, out [V][S][D][G][R], info [V][S][17] as numpy, the workspace).
    `over` replaces single arguments (refusal tests); prefill: the byte out and info hold before the call (default: the guards' 0xA5)."""
    lib, L = _lib()
    V, A, a = _sizes(vol, lab, labels, over)
    S, D = len(labels), len(offsets)
    g_out, g_info = _guarded((V, max(S, 1), max(D, 1), levels, max(R, 1)), prefill), _guarded((V, max(S, 1), RR.RLM_INFO), prefill)
    need = L.size('hv_glrlm_workspace_bytes', V, *A, S, D, levels, R)
    ws = ws or _Ws(max(need, 16), off=over.get('ws_off', 0))
    flat = [int(c) for d in offsets for c in d]
    rc = L.cdll.hv_glrlm(*_front(lib, vol, lab, mask, labels, a, over),
                         None if over.get('offsets_null') else (ctypes.c_int * max(3 * D, 3))(*flat), over.get('D', D), ctypes.c_double(lo),
                         ctypes.c_double(width), over.get('nlev', levels), over.get('nbins', R), _out_ptr(g_out, over, 'out'),
                         _out_ptr(g_info, over, 'info'), ctypes.c_void_p(None) if over.get('ws_null') else ws.ptr,
                         ctypes.c_size_t(ws.need if ws_bytes is None else ws_bytes), lib.stream())
    torch.cuda.synchronize()
    assert g_out.intact() and g_info.intact() and ws.border_intact(), 'wrote outside a buffer'
    return rc, g_out.t.cpu().numpy().copy(), g_info.t.cpu().numpy().copy(), ws


def _gldm(vol, lab, labels, lo, width, levels, alpha, mask=None, ws=None, ws_bytes=None, prefill=None, **over):
    """One hv_gldm -> (return code, dep [V][S][G][27], ngt [V][S][G][27][2], info [V][S][4] as numpy, the workspace)."""
    lib, L = _lib()
    V, A, a = _sizes(vol, lab, labels, over)
    S = max(len(labels), 1)
    g_dep, g_ngt, g_info = _guarded((V, S, levels, RR.NB), prefill), _guarded((V, S, levels, RR.NB, 2), prefill), _guarded((V, S, RR.INFO), prefill)
    need = L.size('hv_gldm_workspace_bytes', V, *A, len(labels), levels)
    ws = ws or _Ws(max(need, 16), off=over.get('ws_off', 0))
    rc = L.cdll.hv_gldm(*_front(lib, vol, lab, mask, labels, a, over), ctypes.c_double(lo), ctypes.c_double(width), over.get('nlev', levels),
                        alpha, _out_ptr(g_dep, over, 'out'), _out_ptr(g_ngt, over, 'ngt'), _out_ptr(g_info, over, 'info'),
                        ctypes.c_void_p(None) if over.get('ws_null') else ws.ptr, ctypes.c_size_t(ws.need if ws_bytes is None else ws_bytes),
                        lib.stream())
    torch.cuda.synchronize()
    assert g_dep.intact() and g_ngt.intact() and g_info.intact() and ws.border_intact(), 'wrote outside a buffer'
    return rc, g_dep.t.cpu().numpy().copy(), g_ngt.t.cpu().numpy().copy(), g_info.t.cpu().numpy().copy(), ws


def _same(got, ref, what=None):
    """Device arrays (one volume) against the reference's, bit for bit."""
    for n, (g, r) in enumerate(zip(got, ref)):
        assert g.shape == r.shape and g.dtype == np.int64, (what, n, g.shape, r.shape)
        if g.tobytes() != r.tobytes():
            bad = np.argwhere(g != r)
            raise AssertionError((what, n, len(bad), bad[:5].tolist(), g[tuple(bad[0])], r[tuple(bad[0])]))


def _intensities(shape, dtype, seed=0):
    """Blocks of one level (3 x 4 x 5 voxels, levels 0 .. 5 at lo = -20, width = 40) with a tenth of the voxels replaced by noise that reaches
    below lo and above lo + 8 * width: runs of every length up to the blocks', and both clamps."""
    g = np.random.default_rng(seed)
    i, j, k = np.indices(shape)
    v = ((i // 3 + j // 4 + k // 5) % 6) * 40.0 + 7.0
    noise = g.random(shape) < 0.1
    v[noise] = g.integers(-60, 400, shape)[noise]
    dtype = np.dtype(dtype)
    return (np.clip(v, 0, 255) if dtype == np.uint8 else v).astype(dtype)


def _lo_width(dtype):
    return (0.0, 30.0) if np.dtype(dtype) == np.uint8 else (LO, WIDTH)


def _labels2(shape, seed=0):
    """Label 1 over most of the volume, label 2 from the middle of axis 1 on, a twentieth of the voxels 0."""
    g = np.random.default_rng(100 + seed)
    lab = np.ones(shape, dtype=np.uint8)
    lab[:, (shape[1] + 1) // 2:, :] = 2
    lab[g.random(shape) < 0.05] = 0
    return lab


@functools.lru_cache(maxsize=None)
def _case(shape, dtype=np.int16, seed=0):
    vol, lab = _intensities(shape, dtype, seed), _labels2(shape, seed)
    vol.setflags(write=False)
    lab.setflags(write=False)
    return vol, lab


@functools.lru_cache(maxsize=None)
def _ref(shape, dtype=np.int16, seed=0, offsets=tuple(D13), R=None, alpha=0):
    """(out, info_r, dep, ngt, info_d) of _case under labels (1, 2), read-only and shared."""
    vol, lab = _case(shape, dtype, seed)
    lo, width = _lo_width(dtype)
    ref = RR.glrlm_ref(vol, lab, (1, 2), offsets, lo, width, G, R or max(shape)) + RR.gldm_ref(vol, lab, (1, 2), lo, width, G, alpha)
    for r in ref:
        r.setflags(write=False)
    return ref


def _both(vol, lab, shape, dtype=np.int16, seed=0, offsets=tuple(D13), R=None, alpha=0, mask=None, what=None):
    """hv_glrlm and hv_gldm on device tensors holding _case(shape, dtype, seed), against _ref; -> the device's five arrays [V]..."""
    lo, width = _lo_width(dtype)
    rc, out, info, _ = _glrlm(vol, lab, (1, 2), offsets, lo, width, G, R or max(shape), mask=mask)
    rc2, dep, ngt, info_d, _ = _gldm(vol, lab, (1, 2), lo, width, G, alpha, mask=mask)
    assert rc == 0 and rc2 == 0, (what, rc, rc2)
    if mask is None:
        _same((out[0], info[0], dep[0], ngt[0], info_d[0]), _ref(shape, dtype, seed, tuple(offsets), R, alpha), what)
    return out, info, dep, ngt, info_d


def _identities(out, info, dep, ngt, info_d, vol, lab, dtype=np.int16):
    """On the device result alone: sum_j j P(i, j) is the slot's level histogram in every direction (nothing capped), dep sums to the count,
    ngt's counts have dep's level margin."""
    lo, width = _lo_width(dtype)
    lev, finite, _, _ = RR.levels_of(vol, lo, width, G)
    j = np.arange(1, out.shape[-1] + 1)
    for s, l in enumerate((1, 2)):
        hist = np.bincount(lev[(lab == l) & finite], minlength=G)
        assert ((out[s] * j).sum(axis=-1) == hist[None, :]).all() and not info[s, RR.INFO:].any()
        assert dep[s].sum() == info_d[s, 1] == info[s, 1] == hist.sum() and (ngt[s, ..., 0].sum(axis=-1) == dep[s].sum(axis=-1)).all()


# ------------------------------------------------------------------------------------------------ the entries
def test_the_documented_examples():
    vol, lab = _dev(RR.RUN_IMAGE[None]), torch.ones((1, 5, 5), dtype=torch.uint8, device='cuda')
    rc, out, info, _ = _glrlm(vol, lab, (1,), [(0, 0, 1)], 1.0, 1.0, 5, 5)
    assert rc == 0 and (out[0, 0, 0] == RR.RUN_GLRLM).all() and tuple(info[0, 0]) == (0, 25, 0, 0) + (0,) * 13
    rc, dep, _, _, _ = _gldm(vol, lab, (1,), 1.0, 1.0, 5, 0)
    assert rc == 0 and (dep[0, 0, :, :4] == RR.RUN_GLDM).all() and not dep[0, 0, :, 4:].any()
    rc, _, ngt, _, _ = _gldm(_dev(RR.NGTDM_IMAGE[None]), torch.ones((1, 4, 4), dtype=torch.uint8, device='cuda'), (1,), 1.0, 1.0, 5, 0)
    n, s = RR.ngtdm_table_loop(ngt[0, 0])
    assert rc == 0 and n == RR.NGTDM_N.tolist() and np.abs(np.array(s) - RR.NGTDM_S).max() <= 1e-12


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_shapes_all_directions(shape):
    vol, lab = _case(shape)
    got = _both(_dev(vol), _dev(lab), shape)
    _identities(*(g[0] for g in got), vol, lab)


def test_a_constant_volume_has_one_run_per_line():
    """(3, 18, 130) constant: a run of 130 along axis 2 (a row longer than two wave chunks), diagonal runs through the corners."""
    vol, lab = np.full(LONG, 100, dtype=np.int16), np.ones(LONG, dtype=np.uint8)
    rc, out, info, _ = _glrlm(_dev(vol), _dev(lab), (1,), D13, LO, WIDTH, G, 130)
    assert rc == 0
    _same((out[0], info[0]), RR.glrlm_ref(vol, lab, (1,), D13, LO, WIDTH, G, 130))
    lev = 3
    assert out[0, 0, D13.index((0, 0, 1)), lev, 129] == 3 * 18 and out[0, 0, D13.index((1, 1, 1)), lev, 2] == 16 * 128
    assert (out[0, 0, :, lev].sum(axis=0) * np.arange(1, 131)).sum() == 13 * vol.size and not info[0, 0, RR.INFO:].any()
    rc, capped, c_info, _ = _glrlm(_dev(vol), _dev(lab), (1,), D13, LO, WIDTH, G, 4)         # max_run = 4: the last bin takes the longer runs
    assert rc == 0
    _same((capped[0], c_info[0]), RR.glrlm_ref(vol, lab, (1,), D13, LO, WIDTH, G, 4))
    assert c_info[0, 0, RR.INFO + D13.index((0, 0, 1))] == 3 * 18 == capped[0, 0, D13.index((0, 0, 1)), lev, 3]
    assert (capped[0].sum(axis=-1) == out[0].sum(axis=-1)).all() and (c_info[0, 0, RR.INFO:] == out[0, 0, :, :, 4:].sum(axis=(1, 2))).all()
    rc, dep, ngt, _, _ = _gldm(_dev(vol), _dev(lab), (1,), LO, WIDTH, G, 0)
    assert rc == 0
    _same((dep[0], ngt[0]), RR.gldm_ref(vol, lab, (1,), LO, WIDTH, G, 0)[:2])
    assert dep[0, 0, lev, 26] == 1 * 16 * 128 and not ngt[0, ..., 1].any()


@pytest.mark.parametrize('offsets', ([(0, 0, 1)], [(1, -1, 0)], NEG13), ids=('row', 'one-diagonal', 'negated-13'))
def test_offset_lists(offsets):
    vol, lab = _case(EDGE)
    rc, out, info, _ = _glrlm(_dev(vol), _dev(lab), (1, 2), offsets, LO, WIDTH, G, 33)
    assert rc == 0
    _same((out[0], info[0]), RR.glrlm_ref(vol, lab, (1, 2), offsets, LO, WIDTH, G, 33))
    if offsets is NEG13:                        # -d walks the lines of d from their other end: the same runs
        assert out[0].tobytes() == _ref(EDGE)[0].tobytes()
    else:
        assert out[0, :, 0].tobytes() == np.ascontiguousarray(_ref(EDGE)[0][:, D13.index(offsets[0])]).tobytes()


@pytest.mark.parametrize('ldtype', (np.uint8, np.int32), ids=lambda d: 'label-' + np.dtype(d).name)
@pytest.mark.parametrize('dtype', (np.uint8, np.int16, np.float32, np.float64), ids=lambda d: np.dtype(d).name)
def test_dtype_pairs(dtype, ldtype):
    vol, lab = _case(EDGE, dtype)
    got = _both(_dev(vol), _dev(lab.astype(ldtype)), EDGE, dtype)
    assert got[1][0, 0, 2] > 0 or dtype == np.uint8
    assert got[1][0, 0, 3] > 0


def test_layouts_and_batches_give_the_contiguous_bytes():
    """The smallest stride on axis 0, a step-2 sliced view whose skipped elements would change everything, and V = 2 through a batch stride."""
    shape = EDGE
    (v0, l0), (v1, l1) = _case(shape, np.float32, 0), _case(shape, np.float32, 1)
    fort = lambda a: _dev(a.transpose(2, 1, 0)).permute(2, 1, 0)
    assert fort(v0).stride(0) == 1
    _both(fort(v0), fort(l0), shape, np.float32, what='axis 0 innermost')
    _both(fort(v0), _dev(l0), shape, np.float32, what='volume alone permuted')

    def sliced(a, skip):
        big = np.full((a.shape[0], a.shape[1] * 2, a.shape[2] * 2 + 1), skip, dtype=a.dtype)
        big[:, ::2, 1::2] = a
        return _dev(big)[:, ::2, 1::2]

    _both(sliced(v0, np.nan), sliced(l0, 255), shape, np.float32, what='sliced')
    stack = lambda a, b, skip: _dev(np.stack([a, np.full_like(a, skip), b]))[::2]
    sv, sl = stack(v0, v1, np.nan), stack(l0, l1, 255)
    assert sv.stride(0) == 2 * v0.size
    got = _both(sv, sl, shape, np.float32, what='batch')
    _same(tuple(g[1] for g in got), _ref(shape, np.float32, 1), 'the second volume of the batch')


def test_two_labels_meeting_at_equal_level():
    """A constant volume cut by a label plane: runs break at the plane, neighbours across it do not count -- each slot is its half alone."""
    shape = (4, 10, 9)
    vol = np.full(shape, 100, dtype=np.int16)
    lab = np.ones(shape, dtype=np.uint8)
    lab[:, :, 4:] = 2
    rc, out, info, _ = _glrlm(_dev(vol), _dev(lab), (1, 2), D13, LO, WIDTH, G, 10)
    rc2, dep, ngt, info_d, _ = _gldm(_dev(vol), _dev(lab), (1, 2), LO, WIDTH, G, 0)
    assert rc == 0 and rc2 == 0
    _same((out[0], info[0], dep[0], ngt[0], info_d[0]), RR.glrlm_ref(vol, lab, (1, 2), D13, LO, WIDTH, G, 10) + RR.gldm_ref(vol, lab, (1, 2), LO, WIDTH, G, 0))
    for s, half in enumerate((np.s_[:, :, :4], np.s_[:, :, 4:])):
        one = np.ones(vol[half].shape, np.uint8)
        assert out[0, s].tobytes() == RR.glrlm_ref(vol[half], one, (1,), D13, LO, WIDTH, G, 10)[0][0].tobytes(), s
        assert dep[0, s].tobytes() == RR.gldm_ref(vol[half], one, (1,), LO, WIDTH, G, 0)[0][0].tobytes(), s
    row = D13.index((0, 0, 1))
    assert out[0, 0, row, 3, 3] == 40 and out[0, 1, row, 3, 4] == 40 and out[0, :, row].sum() == 80


def test_a_mask_and_a_nan_split_a_run():
    shape = (2, 3, 70)
    vol = np.full(shape, 100, dtype=np.float32)
    lab = np.ones(shape, dtype=np.uint8)
    mask = np.ones(shape, dtype=np.uint8)
    mask[0, 0, 20] = 0
    nan = vol.copy()
    nan[1, 2, 65] = np.nan
    row = D13.index((0, 0, 1))
    rc, out, info, _ = _glrlm(_dev(vol), _dev(lab), (1,), D13, LO, WIDTH, G, 70, mask=_dev(mask))
    assert rc == 0
    _same((out[0], info[0]), RR.glrlm_ref(vol, lab, (1,), D13, LO, WIDTH, G, 70, mask))
    assert out[0, 0, row, 3, 19] == 1 and out[0, 0, row, 3, 48] == 1 and out[0, 0, row, 3, 69] == 5 and info[0, 0, 0] == 0 and info[0, 0, 1] == 419
    rc, out, info, _ = _glrlm(_dev(nan), _dev(lab), (1,), D13, LO, WIDTH, G, 70)
    assert rc == 0
    _same((out[0], info[0]), RR.glrlm_ref(nan, lab, (1,), D13, LO, WIDTH, G, 70))
    assert out[0, 0, row, 3, 64] == 1 and out[0, 0, row, 3, 3] == 1 and out[0, 0, row, 3, 69] == 5 and info[0, 0, 0] == LR.NONFINITE
    for m, v in ((mask, vol), (None, nan)):
        rc, dep, ngt, info_d, _ = _gldm(_dev(v), _dev(lab), (1,), LO, WIDTH, G, 0, mask=None if m is None else _dev(m))
        assert rc == 0
        _same((dep[0], ngt[0], info_d[0]), RR.gldm_ref(v, lab, (1,), LO, WIDTH, G, 0, m))
        assert dep[0].sum() == 419 and info_d[0, 0, 0] == (0 if m is not None else LR.NONFINITE)


def test_a_label_value_of_300_sets_the_status_bit():
    vol, lab = _case(EDGE)
    l = lab.astype(np.int32)
    l[3, 4, 6] = 300
    rc, out, info, _ = _glrlm(_dev(vol), _dev(l), (1, 2), D13[:3], LO, WIDTH, G, 33)
    rc2, dep, ngt, info_d, _ = _gldm(_dev(vol), _dev(l), (1, 2), LO, WIDTH, G, 1)
    assert rc == 0 and rc2 == 0
    _same((out[0], info[0], dep[0], ngt[0], info_d[0]), RR.glrlm_ref(vol, l, (1, 2), D13[:3], LO, WIDTH, G, 33) + RR.gldm_ref(vol, l, (1, 2), LO, WIDTH, G, 1))
    assert (info[0, :, 0] == LR.BAD_LABEL).all() and (info_d[0, :, 0] == LR.BAD_LABEL).all()


@pytest.mark.parametrize('levels', (2, 64))
def test_level_counts_with_both_clamps(levels):
    vol, lab = _case(EDGE)
    lo, width = 40.0, 160.0 / levels             # 40 .. 200: the blocks of level 0 and 5 and the noise are clamped
    rc, out, info, _ = _glrlm(_dev(vol), _dev(lab), (1, 2), D13, lo, width, levels, 33)
    rc2, dep, ngt, info_d, _ = _gldm(_dev(vol), _dev(lab), (1, 2), lo, width, levels, levels - 1)
    assert rc == 0 and rc2 == 0
    _same((out[0], info[0], dep[0], ngt[0], info_d[0]),
          RR.glrlm_ref(vol, lab, (1, 2), D13, lo, width, levels, 33) + RR.gldm_ref(vol, lab, (1, 2), lo, width, levels, levels - 1))
    assert (info[0, :, 2] > 0).all() and (info[0, :, 3] > 0).all() and out[0, :, :, levels - 1].any()


def test_64_slots_of_one_voxel():
    shape = (4, 4, 4)
    vol = _intensities(shape, np.int16, 3)
    lab = np.arange(64, dtype=np.uint8).reshape(shape)
    labels = tuple(range(63, -1, -1))
    rc, out, info, _ = _glrlm(_dev(vol), _dev(lab), labels, D13, LO, WIDTH, G, 4)
    rc2, dep, ngt, info_d, _ = _gldm(_dev(vol), _dev(lab), labels, LO, WIDTH, G, 0)
    assert rc == 0 and rc2 == 0
    _same((out[0], info[0], dep[0], ngt[0], info_d[0]), RR.glrlm_ref(vol, lab, labels, D13, LO, WIDTH, G, 4) + RR.gldm_ref(vol, lab, labels, LO, WIDTH, G, 0))
    assert (info[0, :, 1] == 1).all() and (out[0].sum(axis=(2, 3)) == 1).all() and (dep[0, :, :, 0].sum(axis=1) == 1).all() and not ngt[0, ..., 1:, :].any()


@pytest.mark.parametrize('alpha', (0, 3, G - 1))
def test_alpha(alpha):
    vol, lab = _case(EDGE)
    _, _, dep, ngt, _ = _both(_dev(vol), _dev(lab), EDGE, alpha=alpha, offsets=(D13[0],))
    if alpha == G - 1:                           # every neighbour of the slot is dependent: k is n for every voxel
        assert dep[0].tobytes() == np.ascontiguousarray(ngt[0, ..., 0]).tobytes()
    else:
        assert dep[0].tobytes() != np.ascontiguousarray(ngt[0, ..., 0]).tobytes()


def test_same_bytes_twice_and_on_junk_buffers():
    vol, lab = _case(LONG, np.float64)
    dv, dl = _dev(vol), _dev(lab)
    rc, first, i1, ws = _glrlm(dv, dl, (1, 2), D13, LO, WIDTH, G, 130)
    rc2, second, i2, _ = _glrlm(dv, dl, (1, 2), D13, LO, WIDTH, G, 130, ws=ws)               # the workspace as the first call left it
    rc3, third, i3, _ = _glrlm(dv, dl, (1, 2), D13, LO, WIDTH, G, 130, ws=_Ws(ws.need, fill=0xFF), prefill=0xFF)
    assert rc == 0 and rc2 == 0 and rc3 == 0
    assert first.tobytes() == second.tobytes() == third.tobytes() and i1.tobytes() == i2.tobytes() == i3.tobytes()
    _same((first[0], i1[0]), _ref(LONG, np.float64)[:2])
    rc, d1, n1, f1, ws = _gldm(dv, dl, (1, 2), LO, WIDTH, G, 0)
    rc2, d2, n2, f2, _ = _gldm(dv, dl, (1, 2), LO, WIDTH, G, 0, ws=ws)
    rc3, d3, n3, f3, _ = _gldm(dv, dl, (1, 2), LO, WIDTH, G, 0, ws=_Ws(ws.need, fill=0xFF), prefill=0xFF)
    assert rc == 0 and rc2 == 0 and rc3 == 0
    assert d1.tobytes() == d2.tobytes() == d3.tobytes() and n1.tobytes() == n2.tobytes() == n3.tobytes() and f1.tobytes() == f2.tobytes() == f3.tobytes()
    _same((d1[0], n1[0], f1[0]), _ref(LONG, np.float64)[2:])


_SHARED_REFUSALS = [
    (dict(vol_null=1), ERR_ARG), (dict(label_null=1), ERR_ARG), (dict(labels_null=1), ERR_ARG), (dict(out_null=1), ERR_ARG),
    (dict(info_null=1), ERR_ARG), (dict(ws_null=1), ERR_ARG), (dict(V=0), ERR_ARG), (dict(A0=0), ERR_ARG), (dict(A1=-1), ERR_ARG),
    (dict(A2=0), ERR_ARG), (dict(vol_dtype=2), ERR_ARG), (dict(vol_dtype=7), ERR_ARG), (dict(label_dtype=6), ERR_ARG),
    (dict(label_dtype=-1), ERR_ARG), (dict(S=0), ERR_ARG), (dict(S=65), ERR_ARG), (dict(nlev=1), ERR_ARG), (dict(nlev=65), ERR_ARG),
    (dict(lo=float('nan')), ERR_ARG), (dict(lo=float('inf')), ERR_ARG), (dict(width=float('nan')), ERR_ARG), (dict(width=float('inf')), ERR_ARG),
    (dict(width=0.0), ERR_ARG), (dict(width=-1.0), ERR_ARG), (dict(out_off=4), ERR_ARG), (dict(info_off=4), ERR_ARG), (dict(ws_off=8), ERR_ARG),
    (dict(ws_bytes=-1), ERR_ARG), (dict(labels=(1, 1)), ERR_ARG), (dict(labels=(1, 256)), ERR_ARG), (dict(labels=(-1, 2)), ERR_ARG),
    (dict(A0=1 << 11, A1=1 << 10, A2=(1 << 9) + 1), ERR_UNSUPPORTED), (dict(V=65536), ERR_UNSUPPORTED),
]
_SENTINEL = np.frombuffer(b'\xa5' * 8, dtype=np.int64)[0]


def test_glrlm_refusals_write_nothing():
    vol, lab = _case(EDGE, np.float32)
    dv, dl = _dev(vol), _dev(lab)
    L = _lib()[1]
    need = L.size('hv_glrlm_workspace_bytes', 1, *EDGE, 2, 2, 8, 6)
    assert need >= 2 * vol.size
    own = [(dict(offsets_null=1), ERR_ARG), (dict(D=0), ERR_ARG), (dict(D=14), ERR_ARG), (dict(nbins=0), ERR_ARG), (dict(nbins=-3), ERR_ARG),
           (dict(offsets=((0, 0, 2), (0, 1, 0))), ERR_ARG), (dict(offsets=((0, 1, 0), (-2, 0, 0))), ERR_ARG),
           (dict(offsets=((0, 0, 0), (0, 1, 0))), ERR_ARG), (dict(offsets=((1, -1, 0), (1, -1, 0))), ERR_ARG),
           (dict(offsets=((1, -1, 0), (-1, 1, 0))), ERR_ARG)]
    for over, code in _SHARED_REFUSALS + own:
        over = dict(over)
        labels, offs = over.pop('labels', (1, 2)), over.pop('offsets', ((0, 0, 1), (1, 0, 0)))
        lo, width = over.pop('lo', 0.0), over.pop('width', 10.0)
        wb = over.pop('ws_bytes', None)
        ws = _Ws(need, off=over.get('ws_off', 0))
        rc, out, info, ws = _glrlm(dv, dl, labels, offs, lo, width, 8, 6, ws=ws, ws_bytes=None if wb is None else need + wb, **over)
        assert rc == code, (over, labels, offs, lo, width, rc)
        assert (out == _SENTINEL).all() and (info == _SENTINEL).all() and ws.untouched(), (over, labels, offs, lo, width)
    for bad in ((0, 4, 4, 4, 1, 1, 8, 4), (1, 4, 4, 4, 0, 1, 8, 4), (1, 4, 4, 4, 65, 1, 8, 4), (1, 4, 4, 4, 1, 0, 8, 4), (1, 4, 4, 4, 1, 14, 8, 4),
                (1, 4, 4, 4, 1, 1, 1, 4), (1, 4, 4, 4, 1, 1, 65, 4), (1, 4, 4, 4, 1, 1, 8, 0), (1, 1 << 11, 1 << 10, (1 << 9) + 1, 1, 1, 8, 4),
                (65536, 4, 4, 4, 1, 1, 8, 4)):
        assert L.size('hv_glrlm_workspace_bytes', *bad) == 0, bad


def test_gldm_refusals_write_nothing():
    vol, lab = _case(EDGE, np.float32)
    dv, dl = _dev(vol), _dev(lab)
    L = _lib()[1]
    need = L.size('hv_gldm_workspace_bytes', 1, *EDGE, 2, 8)
    assert need >= 2 * vol.size
    own = [(dict(ngt_null=1), ERR_ARG), (dict(ngt_off=4), ERR_ARG), (dict(alpha=-1), ERR_ARG), (dict(alpha=8), ERR_ARG)]
    for over, code in _SHARED_REFUSALS + own:
        over = dict(over)
        labels, lo, width, alpha = over.pop('labels', (1, 2)), over.pop('lo', 0.0), over.pop('width', 10.0), over.pop('alpha', 1)
        wb = over.pop('ws_bytes', None)
        ws = _Ws(need, off=over.get('ws_off', 0))
        rc, dep, ngt, info, ws = _gldm(dv, dl, labels, lo, width, 8, alpha, ws=ws, ws_bytes=None if wb is None else need + wb, **over)
        assert rc == code, (over, labels, lo, width, alpha, rc)
        assert (dep == _SENTINEL).all() and (ngt == _SENTINEL).all() and (info == _SENTINEL).all() and ws.untouched(), (over, labels, lo, width, alpha)
    for bad in ((0, 4, 4, 4, 1, 8), (1, 4, 4, 4, 0, 8), (1, 4, 4, 4, 65, 8), (1, 4, 4, 4, 1, 1), (1, 4, 4, 4, 1, 65),
                (1, 1 << 11, 1 << 10, (1 << 9) + 1, 1, 8), (65536, 4, 4, 4, 1, 8)):
        assert L.size('hv_gldm_workspace_bytes', *bad) == 0, bad


# ------------------------------------------------------------------------------------------------ the module
def test_glrlm_and_gldm_on_host_arrays_and_resident_tensors(monkeypatch):
    R = _R()
    vol, lab = _case(EDGE)
    mask = np.random.default_rng(12).random(EDGE) > 0.2
    offs = D13[:4]
    r_out, r_info = RR.glrlm_ref(vol, lab, (1, 2), offs, LO, WIDTH, G, 5, mask)
    r_dep, r_ngt, r_info_d = RR.gldm_ref(vol, lab, (1, 2), LO, WIDTH, G, 1, mask)
    exact = ExactWs(monkeypatch, required=True)
    runs = [R.glrlm(_dev(vol), _dev(lab), (1, 2), offs, G, LO, WIDTH, max_run=5, mask=_dev(mask)),
            R.glrlm(np.array(vol), np.array(lab), (1, 2), offs, G, LO, WIDTH, max_run=5, mask=mask)]
    deps = [R.gldm(_dev(vol), _dev(lab), (1, 2), 1, G, LO, WIDTH, mask=_dev(mask)), R.gldm(np.array(vol), np.array(lab), (1, 2), 1, G, LO, WIDTH, mask=mask)]
    exact.close()
    for res in runs:
        assert res['matrices'].dtype == np.int64 and res['matrices'].shape == (2, 4, G, 5) and res['matrices'].tobytes() == r_out.tobytes()
        assert list(res['labels']) == [1, 2] and res['offsets'].tolist() == [list(d) for d in offs]
        assert res['capped'].shape == (2, 4) and (res['capped'] == r_info[:, RR.INFO:RR.INFO + 4]).all() and res['capped'].sum() > 0
        for k, col in (('status', 0), ('count', 1), ('clamped_low', 2), ('clamped_high', 3)):
            assert res[k].shape == (2,) and (res[k] == r_info[:, col]).all(), k
    for res in deps:
        assert res['dependence'].tobytes() == r_dep.tobytes() and res['ngtdm'].tobytes() == r_ngt.tobytes() and res['ngtdm'].shape == (2, G, 27, 2)
        assert (res['count'] == r_info_d[:, 1]).all() and (res['status'] == r_info_d[:, 0]).all()
    auto = R.glrlm(_dev(vol), _dev(lab), levels=G, lo=LO, width=WIDTH)                             # labels=None, the 13 directions, nothing capped
    assert list(auto['labels']) == [1, 2] and auto['matrices'].tobytes() == _ref(EDGE)[0].tobytes() and not auto['capped'].any()
    stacked = R.gldm(_dev(np.stack([vol, vol])), _dev(np.stack([lab, np.zeros_like(lab)])), (1, 7), levels=G, lo=LO, width=WIDTH)
    assert stacked['dependence'].shape == (2, 2, G, 27) and stacked['dependence'][0, 0].tobytes() == _ref(EDGE)[2][0].tobytes()
    assert not stacked['dependence'][1].any() and (stacked['status'][1] == LR.EMPTY).all()
    with pytest.raises(ValueError):
        R.glrlm(torch.from_numpy(vol.copy()), _dev(lab), (1,))     # a CPU tensor: nothing is counted on the host
    with pytest.raises(ValueError):
        R.gldm(torch.from_numpy(vol.copy()), _dev(lab), (1,))
    with pytest.raises(TypeError):
        R.glrlm(_dev(vol).to(torch.int32), _dev(lab), (1,))


def _equal(a, b, path=''):
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), path
        for k in a:
            _equal(a[k], b[k], '%s/%s' % (path, k))
    else:
        assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True), path


def test_run_texture_comparison_batched_and_in_two_calls(monkeypatch):
    R = _R()
    shape = (12, 14, 18)
    ct, _ = _case(shape)
    synth, _ = _case(shape, seed=1)
    lab = np.zeros(shape, dtype=np.uint8)
    lab[1:11, 2:12, 1:9], lab[1:11, 2:12, 10:17] = 21, 22
    calls = []
    real = R._launch_glrlm
    monkeypatch.setattr(R, '_launch_glrlm', lambda *a: (calls.append(int(a[0].shape[0])), real(*a))[1])
    kw = dict(neighbours=(22,), levels=G, lo=LO, width=WIDTH, alpha=1)
    exact = ExactWs(monkeypatch, required=True)
    batched = R.run_texture_comparison(_dev(ct), _dev(synth), _dev(lab), _dev(lab), 21, **kw)
    split = R.run_texture_comparison(_dev(ct), _dev(synth.transpose(2, 0, 1)).permute(1, 2, 0), _dev(lab), _dev(lab), 21, **kw)
    exact.close()
    assert calls == [2, 1, 1]
    _equal(batched, split)
    out, _ = RR.glrlm_ref(synth, lab, (21, 22), D13, LO, WIDTH, G, 18)
    dep, ngt, info = RR.gldm_ref(synth, lab, (21, 22), LO, WIDTH, G, 1)
    syn = batched['synthesized']
    assert syn['glrlm'].tobytes() == out[0].tobytes() and syn['dependence'].tobytes() == dep[0].tobytes() and syn['ngtdm'].tobytes() == ngt[0].tobytes()
    assert syn['count'] == info[0, 1] == 10 * 10 * 8 and batched['neighbours'][22]['count'] == 10 * 10 * 7
    want = RR.glrlm_features_loop(out[0, 2])
    assert abs(syn['features']['glrlm']['LRE'][2] - want['LRE']) <= 1e-12 * want['LRE']
    ori = batched['original']
    assert batched['difference']['run_anisotropy'] == syn['run_anisotropy'] - ori['run_anisotropy']
    assert batched['difference']['glrlm']['SRE'] == syn['features']['glrlm']['mean']['SRE'] - ori['features']['glrlm']['mean']['SRE']
    assert batched['neighbour_difference'][22]['ngtdm']['coarseness'] == (syn['features']['ngtdm']['coarseness']
                                                                          - batched['neighbours'][22]['features']['ngtdm']['coarseness'])
    one = R.vertebra_run_texture(_dev(synth), _dev(lab), 21, levels=G, lo=LO, width=WIDTH, alpha=1)
    _equal(one, syn)


def test_run_anisotropy_of_slice_wise_synthesis():
    """Constant in plane, alternating along axis 2: runs of length 1 along the slice axis, runs through the whole label inside a slice."""
    R = _R()
    shape = (24, 24, 24)
    k = np.indices(shape)[2]
    vol = np.where(k % 2 == 0, 100, 140).astype(np.int16)
    lab = np.zeros(shape, dtype=np.uint8)
    lab[2:22, 3:21, 1:23] = 5

    def expected(v, l, axis):
        axes = [tuple(1 if c == a else 0 for c in range(3)) for a in [axis] + [a for a in range(3) if a != axis]]
        out, _ = RR.glrlm_ref(v, l, (5,), axes, LO, WIDTH, G, 24)
        m = [RR.glrlm_features_loop(out[0, d])['mean_run'] for d in range(3)]
        return m[0] / ((m[1] + m[2]) / 2)

    got = R.vertebra_run_texture(_dev(vol), _dev(lab), 5, levels=G, lo=LO, width=WIDTH)
    want = expected(vol, lab, 2)
    assert want == 1.0 / ((20 + 18) / 2) and abs(got['run_anisotropy'] - want) <= 1e-12 * want and got['run_anisotropy'] < 1
    vt, lt = np.ascontiguousarray(vol.transpose(2, 1, 0)), np.ascontiguousarray(lab.transpose(2, 1, 0))
    turned = R.vertebra_run_texture(_dev(vt), _dev(lt), 5, levels=G, lo=LO, width=WIDTH)       # the slices now stack along axis 0
    want_t = expected(vt, lt, 2)
    assert abs(turned['run_anisotropy'] - want_t) <= 1e-12 * want_t and turned['run_anisotropy'] > 1
    same = R.vertebra_run_texture(_dev(vt), _dev(lt), 5, levels=G, lo=LO, width=WIDTH, slice_axis=0)
    assert abs(same['run_anisotropy'] - got['run_anisotropy']) <= 1e-12 * want
    assert turned['glrlm'][D13.index((1, 0, 0))].tobytes() == got['glrlm'][D13.index((0, 0, 1))].tobytes()
