"""hv_label_stats (csrc/labelstats.hip) and healthivert-gan_amd/label_statistics.py against tests/labelstats_ref.py (pinned against scipy and numpy
by tests/test_labelstats_ref_cpu.py).  Counts, integer sums, minima, maxima, coordinate sums, boxes, status words and order statistics are
compared bit for bit (an order statistic that is a zero with ==: the select may return either zero); the float dtypes' sum v and sum v^2 to
STATS_TOL = 1e-12 relative against the fsum-exact restatement.  Measured on the device (MI355X): 3.91e-16 for float32 and float64 alike, 0 for the
integer dtypes (test_dtype_pairs prints it).
Records lie between guard words and are pre-filled with a sentinel, the workspace is exactly the queried bytes inside a 0xA5 border."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import labelstats_ref as LR
import morph_ref as MR
from hvtest import Guarded

pytestmark = pytest.mark.gpu

STATS_TOL = 1e-12                      # tests/test_labelstats_ref_cpu.py: max(10 x 3.15e-16, 1e-12)
ERR_ARG, ERR_UNSUPPORTED = -1, -2
_VDT = {torch.uint8: 0, torch.int16: 1, torch.float32: 4, torch.float64: 5}
_LDT = {torch.uint8: 0, torch.int16: 1, torch.int32: 2, torch.int64: 3, torch.float32: 4, torch.float64: 5}
VOL_DTYPES = (np.uint8, np.int16, np.float32, np.float64)
ALL = (0,) + LR.LABELS


def _lib():
    import hvgan  # noqa: F401
    from hvgan import lib
    return lib, lib.get()


def _S():
    import hvgan  # noqa: F401
    from hvgan import label_statistics
    return label_statistics


def _dev(a):
    return torch.from_numpy(np.array(a, order='C')).cuda()          # a copy: the cached cases are read-only


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


def _call(vol, lab, labels, q=(), mask=None, ws=None, ws_bytes=None, **over):
    """One hv_label_stats on device tensors (3-D, or 4-D stacked) -> (return code, records [V][S][REC] as numpy, the workspace).  `over`
    replaces single arguments (refusal tests)."""
    lib, L = _lib()
    shape = tuple(int(s) for s in vol.shape)
    V, A = (shape[0], shape[1:]) if len(shape) == 4 else (1, shape)
    S, Q = len(labels), len(q)
    a = dict(V=V, A0=A[0], A1=A[1], A2=A[2], S=S, Q=Q, vol_dtype=_VDT[vol.dtype], label_dtype=_LDT[lab.dtype])
    a.update({k: v for k, v in over.items() if k in a})
    g = Guarded((V, S, LR.REC), torch.float64)
    g.t.fill_(LR.SENTINEL)
    need = L.size('hv_label_stats_workspace_bytes', V, *A, S, Q)
    ws = ws or _Ws(max(need, 16), off=over.get('ws_off', 0))
    nul = ctypes.c_void_p(None)
    rc = L.cdll.hv_label_stats(
        nul if over.get('vol_null') else lib.ptr(vol), a['vol_dtype'], *_ll(_st4(vol)),
        nul if over.get('label_null') else lib.ptr(lab), a['label_dtype'], *_ll(_st4(lab)),
        lib.ptr(mask), *_ll(_st4(mask) if mask is not None else (0, 0, 0, 0)), a['V'], a['A0'], a['A1'], a['A2'],
        None if over.get('labels_null') else (ctypes.c_int * max(S, 1))(*labels), a['S'],
        None if over.get('q_null') else (ctypes.c_double * max(Q, 1))(*q), a['Q'],
        nul if over.get('out_null') else ctypes.c_void_p(g.t.data_ptr() + over.get('out_off', 0)),
        nul if over.get('ws_null') else ws.ptr, ctypes.c_size_t(ws.need if ws_bytes is None else ws_bytes), lib.stream())
    torch.cuda.synchronize()
    assert g.intact() and ws.border_intact(), 'wrote outside a buffer'
    return rc, g.t.cpu().numpy().copy(), ws


@functools.lru_cache(maxsize=None)
def _case(dtype, seed=0):
    vol = LR.intensities(dtype, seed)
    vol.setflags(write=False)
    return vol, LR.base_label()


@functools.lru_cache(maxsize=None)
def _ref(dtype, labels=ALL, q=LR.QS, seed=0, masked=False):
    vol, lab = _case(dtype, seed)
    rec = LR.label_stats_ref(vol, lab, labels, q, _mask() if masked else None)
    rec.setflags(write=False)
    return rec


def _mask():
    m = np.ones(LR.SHAPE, dtype=np.uint8)
    m[:, :, ::3] = 0
    m[31, 0, 0] = 0                             # empties label 2
    return m


def _check(rec, ref, integer, Q):
    """rec, ref: [S][REC].  -> the largest relative difference of the float sums."""
    worst = 0.0
    S = ref.shape[0]
    for s in range(S):
        a, b = rec[s], ref[s]
        exact = [LR.COUNT, LR.STATUS, LR.STATUS + 1] + [f + c for f in (LR.COORD, LR.LO, LR.HI) for c in range(3)]
        for f in exact:
            assert a[f].tobytes() == b[f].tobytes(), (s, f, a[f], b[f])
        nonfinite = int(b[LR.STATUS]) & LR.NONFINITE
        if not nonfinite:
            assert LR.same_value(a[LR.MIN], b[LR.MIN]) and LR.same_value(a[LR.MAX], b[LR.MAX]), (s, a[LR.MIN:LR.MAX + 1], b[LR.MIN:LR.MAX + 1])
            for f in (LR.SUM, LR.SUMSQ):
                if integer:
                    assert a[f].tobytes() == b[f].tobytes(), (s, f, a[f:f + 1].view(np.int64), b[f:f + 1].view(np.int64))
                else:
                    d = abs(a[f] - b[f]) / max(abs(b[f]), np.finfo(np.float64).tiny) if b[f] != a[f] else 0.0
                    worst = max(worst, d)
                    assert d <= STATS_TOL, (s, f, a[f], b[f], d)
            for t in range(2 * Q):
                x, y = a[LR.ORDER + t], b[LR.ORDER + t]
                assert (np.isnan(x) and np.isnan(y)) or LR.same_value(x, y), (s, t, x, y)
        assert (a[LR.ORDER + 2 * Q:] == LR.SENTINEL).all(), 'fields past the percentiles asked for were written'
    return worst


@pytest.mark.parametrize('ldtype', (np.uint8, np.float32, np.float64), ids=lambda d: 'label-' + np.dtype(d).name)
@pytest.mark.parametrize('dtype', VOL_DTYPES, ids=lambda d: np.dtype(d).name)
def test_dtype_pairs(dtype, ldtype, capsys):
    """Every intensity dtype against every label dtype on the full case: both ends of int16, negative values, denormals, two values one ulp
    apart, label sizes 1 / 2 / 63 / 64 / 65, one label over 24 tiles, an absent label, a label of one value; 9 labels x 12 targets = four LDS
    groups of the select."""
    vol, lab = _case(dtype)
    rc, rec, _ = _call(_dev(vol), _dev(lab.astype(ldtype)), ALL, LR.QS)
    assert rc == 0
    ref = _ref(dtype)
    worst = _check(rec[0], ref, np.dtype(dtype).kind in 'iu', len(LR.QS))
    s9 = ALL.index(9)
    assert rec[0, s9, LR.COUNT] == 0 and tuple(rec[0, s9, LR.LO:LR.LO + 3]) == LR.SHAPE and tuple(rec[0, s9, LR.HI:LR.HI + 3]) == (-1, -1, -1)
    assert int(rec[0, s9, LR.STATUS]) == LR.EMPTY and np.isnan(rec[0, s9, LR.ORDER:LR.ORDER + 12]).all()
    s3, t50 = ALL.index(3), LR.QS.index(50.0)
    if np.dtype(dtype).kind == 'f':             # the last radix pass decides between the two
        lo, hi = rec[0, s3, LR.ORDER + 2 * t50], rec[0, s3, LR.ORDER + 2 * t50 + 1]
        assert np.dtype(dtype).type(hi) == np.nextafter(np.dtype(dtype).type(lo), np.dtype(dtype).type(np.inf))
    with capsys.disabled():
        print('\n%s / %s: largest relative |device - fsum| of sum v, sum v^2: %.3g' % (np.dtype(dtype).name, np.dtype(ldtype).name, worst))


@pytest.mark.parametrize('dtype', VOL_DTYPES, ids=lambda d: np.dtype(d).name)
def test_q0_s1_s64(dtype):
    vol, lab = _case(dtype)
    integer = np.dtype(dtype).kind in 'iu'
    dv, dl = _dev(vol), _dev(lab)
    rc, rec, _ = _call(dv, dl, ALL, ())                                   # Q = 0: no select, the percentile fields keep the sentinel
    assert rc == 0
    _check(rec[0], _ref(dtype, ALL, ()), integer, 0)
    assert (rec[0, :, LR.ORDER:] == LR.SENTINEL).all()
    rc, rec, _ = _call(dv, dl, (1,), (50.0,))                             # S = 1
    assert rc == 0
    _check(rec[0], _ref(dtype, (1,), (50.0,)), integer, 1)
    many = tuple(range(63, -1, -1))                                       # S = 64, label 0 listed: 128 (slot, target) pairs, four groups
    rc, rec, _ = _call(dv, dl, many, (37.0,))
    assert rc == 0
    _check(rec[0], _ref(dtype, many, (37.0,)), integer, 1)


def _layouts(a, skip):
    """The array as a device tensor in C order, Fortran order, two permuted storages and a sliced view whose skipped elements hold `skip`."""
    c = _dev(a)
    out = {'c': c, 'fortran': _dev(a.transpose(2, 1, 0)).permute(2, 1, 0), 'z-fastest-permuted': _dev(a.transpose(1, 0, 2)).permute(1, 0, 2),
           'y-fastest': _dev(a.transpose(0, 2, 1)).permute(0, 2, 1)}
    big = np.full((a.shape[0] + 2, a.shape[1] * 2 + 1, a.shape[2] * 3 + 2), skip, dtype=a.dtype)
    big[1:-1, 1::2, 1:-1:3] = a
    out['sliced'] = _dev(big)[1:-1, 1::2, 1:-1:3]
    for k, t in out.items():
        assert tuple(t.shape) == a.shape and torch.equal(t, c), k
    return out


@pytest.mark.parametrize('dtype', VOL_DTYPES, ids=lambda d: np.dtype(d).name)
def test_layouts_give_the_contiguous_bytes(dtype):
    vol, lab = _case(dtype)
    vols = _layouts(vol, np.nan if np.dtype(dtype).kind == 'f' else 99)
    labs = _layouts(lab.astype(np.float32) if dtype == np.float64 else lab, 255)
    q = (50.0, 95.0)
    rc, base, _ = _call(vols['c'], labs['c'], ALL, q)
    assert rc == 0
    _check(base[0], _ref(dtype, ALL, q), np.dtype(dtype).kind in 'iu', 2)
    for name in vols:
        for lname in ('c', name):
            rc, rec, _ = _call(vols[name], labs[lname], ALL, q)
            assert rc == 0 and rec.tobytes() == base.tobytes(), (name, lname)


@pytest.mark.parametrize('dtype', (np.int16, np.float64), ids=lambda d: np.dtype(d).name)
def test_mask(dtype):
    vol, lab = _case(dtype)
    dv, dl = _dev(vol), _dev(lab)
    rc, base, _ = _call(dv, dl, ALL, LR.QS)
    rc1, ones, _ = _call(dv, dl, ALL, LR.QS, mask=torch.ones(LR.SHAPE, dtype=torch.uint8, device='cuda'))
    assert rc == 0 and rc1 == 0 and ones.tobytes() == base.tobytes()
    m = _mask()
    rc, rec, _ = _call(dv, dl, ALL, LR.QS, mask=_dev(m.transpose(2, 0, 1)).permute(1, 2, 0))       # the mask's own strides
    assert rc == 0
    _check(rec[0], _ref(dtype, ALL, LR.QS, 0, True), np.dtype(dtype).kind in 'iu', len(LR.QS))
    s2 = ALL.index(2)
    assert rec[0, s2, LR.COUNT] == 0 and int(rec[0, s2, LR.STATUS]) == LR.EMPTY


@pytest.mark.parametrize('dtype', (np.int16, np.float32, np.float64), ids=lambda d: np.dtype(d).name)
def test_batch_equals_single_calls(dtype):
    vols = [_case(dtype, seed)[0] for seed in (0, 1, 2)]
    labs = [np.roll(LR.base_label(), r, axis=1) for r in (0, 1, 2)]
    q = (5.0, 50.0)
    singles = [_call(_dev(v), _dev(l), LR.LABELS, q) for v, l in zip(vols, labs)]
    assert all(rc == 0 for rc, _, _ in singles)
    _check(singles[0][1][0], _ref(dtype, LR.LABELS, q), np.dtype(dtype).kind in 'iu', 2)
    for order in ((0, 1, 2), (2, 1, 0)):
        rc, rec, _ = _call(_dev(np.stack([vols[i] for i in order])), _dev(np.stack([labs[i] for i in order])), LR.LABELS, q)
        assert rc == 0
        for n, i in enumerate(order):
            assert rec[n].tobytes() == singles[i][1][0].tobytes(), (order, i)


@pytest.mark.parametrize('dtype', (np.uint8, np.float64), ids=lambda d: np.dtype(d).name)
def test_same_bytes_twice_and_on_a_poisoned_workspace(dtype):
    vol, lab = _case(dtype)
    dv, dl = _dev(vol), _dev(lab)
    rc, first, ws = _call(dv, dl, ALL, LR.QS)
    rc2, second, _ = _call(dv, dl, ALL, LR.QS, ws=ws)                    # the workspace as the first call left it
    rc3, third, _ = _call(dv, dl, ALL, LR.QS, ws=_Ws(ws.need, fill=0xFF))
    assert rc == 0 and rc2 == 0 and rc3 == 0
    assert first.tobytes() == second.tobytes() == third.tobytes()


@pytest.mark.parametrize('dtype', (np.float32, np.float64), ids=lambda d: np.dtype(d).name)
def test_nan_inside_a_label_marks_that_slot_only(dtype):
    vol, lab = _case(dtype)
    bad = vol.copy()
    bad[31, 4, 7] = np.nan                      # label 4
    bad[0, 0, 0] = np.inf                       # label 0, not listed: nobody's business
    rc, base, _ = _call(_dev(vol), _dev(lab), LR.LABELS, LR.QS)
    rc2, rec, _ = _call(_dev(bad), _dev(lab), LR.LABELS, LR.QS)
    assert rc == 0 and rc2 == 0
    s4 = LR.LABELS.index(4)
    for s in range(len(LR.LABELS)):
        if s != s4:
            assert rec[0, s].tobytes() == base[0, s].tobytes(), s
    assert int(rec[0, s4, LR.STATUS]) == LR.NONFINITE and rec[0, s4, LR.COUNT] == 63 and np.isnan(rec[0, s4, LR.SUM])
    for f in (LR.COORD, LR.LO, LR.HI):
        assert rec[0, s4, f:f + 3].tobytes() == base[0, s4, f:f + 3].tobytes()


@pytest.mark.parametrize('ldtype', (np.float32, np.float64), ids=lambda d: np.dtype(d).name)
def test_a_value_that_is_no_label_sets_the_status_bit(ldtype):
    vol, lab = _case(np.int16)
    for value in (2.5, 300.0, -1.0, np.nan):
        l = lab.astype(ldtype)
        l[3, 4, 6] = value                      # inside label 1
        rc, rec, _ = _call(_dev(vol), _dev(l), ALL, (50.0,))
        assert rc == 0
        _check(rec[0], LR.label_stats_ref(vol, l, ALL, (50.0,)), True, 1)
        assert (rec[0, :, LR.STATUS].astype(np.int64) & LR.BAD_LABEL).all()
        assert rec[0, ALL.index(1), LR.COUNT] == (lab == 1).sum() - 1


def test_refusals_write_nothing():
    vol, lab = _case(np.float32)
    dv, dl = _dev(vol), _dev(lab)
    L = _lib()[1]
    need = L.size('hv_label_stats_workspace_bytes', 1, *LR.SHAPE, 2, 1)
    assert need > 0
    cases = [
        (dict(vol_null=1), ERR_ARG), (dict(label_null=1), ERR_ARG), (dict(labels_null=1), ERR_ARG), (dict(out_null=1), ERR_ARG),
        (dict(ws_null=1), ERR_ARG), (dict(q_null=1), ERR_ARG), (dict(V=0), ERR_ARG), (dict(A0=0), ERR_ARG), (dict(A1=-1), ERR_ARG),
        (dict(A2=0), ERR_ARG), (dict(vol_dtype=2), ERR_ARG), (dict(vol_dtype=7), ERR_ARG), (dict(label_dtype=6), ERR_ARG),
        (dict(label_dtype=-1), ERR_ARG), (dict(S=0), ERR_ARG), (dict(S=65), ERR_ARG), (dict(Q=9), ERR_ARG), (dict(Q=-1), ERR_ARG),
        (dict(ws_off=8), ERR_ARG), (dict(out_off=4), ERR_ARG), (dict(ws_bytes=need - 1), ERR_ARG),
        (dict(labels=(1, 1)), ERR_ARG), (dict(labels=(1, 256)), ERR_ARG), (dict(labels=(-1, 2)), ERR_ARG),
        (dict(q=(101.0,)), ERR_ARG), (dict(q=(-0.5,)), ERR_ARG), (dict(q=(float('nan'),)), ERR_ARG), (dict(q=(float('inf'),)), ERR_ARG),
        (dict(A0=1 << 11, A1=1 << 10, A2=(1 << 9) + 1), ERR_UNSUPPORTED), (dict(V=65536), ERR_UNSUPPORTED),
    ]
    for over, code in cases:
        over = dict(over)
        labels, q = over.pop('labels', (1, 2)), over.pop('q', (50.0,))
        ws = _Ws(need, off=over.get('ws_off', 0))
        rc, rec, ws = _call(dv, dl, labels, q, ws=ws, ws_bytes=over.pop('ws_bytes', None), **over)
        assert rc == code, (over, labels, q, rc)
        assert (rec == LR.SENTINEL).all() and ws.untouched(), (over, labels, q)
    for bad in ((0, 4, 4, 4, 1, 0), (1, 4, 4, 4, 0, 0), (1, 4, 4, 4, 65, 0), (1, 4, 4, 4, 1, 9), (1, 1 << 11, 1 << 10, (1 << 9) + 1, 1, 0)):
        assert L.size('hv_label_stats_workspace_bytes', *bad) == 0, bad


# ------------------------------------------------------------------------------------------------ the module
def test_label_statistics_against_the_host_chain():
    S = _S()
    sp = (0.7, 0.7, 1.5)
    for dtype in (np.int16, np.float64):
        vol, lab = _case(dtype)
        res = S.label_statistics(_dev(vol), _dev(lab), LR.LABELS, LR.QS, spacing=sp)
        ref = LR.scipy_chain(vol, lab, LR.LABELS, LR.QS)
        assert list(res['labels']) == list(LR.LABELS) and res['count'].shape == (len(LR.LABELS),)
        for s, l in enumerate(LR.LABELS):
            n = ref['count'][s]
            assert res['count'][s] == n and res['volume_mm3'][s] == n * float(np.prod(np.asarray(sp)))
            if n == 0:
                assert np.isnan(res['mean'][s]) and np.isnan(res['percentiles'][s]).all() and res['box_slices'][s] is None
                assert tuple(res['box'][s, 0]) == LR.SHAPE and tuple(res['box'][s, 1]) == (-1, -1, -1)
                continue
            assert res['box_slices'][s] == ref['box'][s] and res['min'][s] == ref['min'][s] and res['max'][s] == ref['max'][s]
            assert tuple(res['centroid'][s]) == tuple(np.float64(c) for c in ref['centroid'][s])
            for t in range(len(LR.QS)):
                assert LR.same_value(res['percentiles'][s, t], ref['percentiles'][s][t]), (l, t)
            assert abs(res['mean'][s] - ref['mean'][s]) <= STATS_TOL * abs(ref['mean'][s])
            assert abs(res['variance'][s] - ref['variance'][s]) <= STATS_TOL * (ref['variance'][s] + ref['mean'][s] ** 2)
            if dtype == np.int16:
                assert np.float64(res['mean'][s]).tobytes() == np.float64(ref['mean'][s]).tobytes()
    vol, lab = _case(np.int16)
    auto = S.label_statistics(_dev(vol), _dev(lab))                       # labels=None: the non-zero labels present
    assert list(auto['labels']) == [1, 2, 3, 4, 5, 6, 7]
    assert list(auto['count']) == [int((lab == l).sum()) for l in range(1, 8)]
    stacked = S.label_statistics(_dev(np.stack([vol, vol])), _dev(np.stack([lab, np.zeros_like(lab)])), (1, 7), (50.0,))
    assert stacked['count'].shape == (2, 2) and list(stacked['count'][1]) == [0, 0] and np.isnan(stacked['mean'][1]).all()
    assert stacked['mean'][0, 1] == 77.0 and stacked['variance'][0, 1] == 0.0 and stacked['percentiles'][0, 1, 0] == 77.0


def test_misuse_raises():
    S = _S()
    vol, lab = _case(np.int16)
    dv, dl = _dev(vol), _dev(lab)
    with pytest.raises(ValueError):
        S.label_statistics(torch.from_numpy(vol.copy()), dl, (1,))        # a CPU tensor: no fallback to the host
    with pytest.raises(TypeError):
        S.label_statistics(vol, dl, (1,))
    with pytest.raises(TypeError):
        S.label_statistics(dv.to(torch.int32), dl, (1,))
    with pytest.raises(ValueError):
        S.label_statistics(dv, dl[:, :, 1:], (1,))
    with pytest.raises(ValueError):
        S.label_statistics(dv, dl, (1, 1))
    with pytest.raises(ValueError):
        S.label_statistics(dv, dl, (1,), percentiles=(101,))
    with pytest.raises(ValueError):
        S.label_statistics(dv, dl, (1,), spacing=(1, 0, 1))
    with pytest.raises(ValueError):
        S.vertebra_density(dv, dl, 1, erode_mm=-1.0)


def test_vertebra_density_is_the_statistics_under_scipys_erosion():
    from scipy import ndimage
    S = _S()
    sp = (0.7, 0.7, 1.5)
    vol, lab = _case(np.float32)
    dv, dl = _dev(vol), _dev(lab)
    for r in (0.0, 1.6):
        got = S.vertebra_density(dv, dl, 1, erode_mm=r, spacing=sp)
        mask = ndimage.binary_erosion(lab == 1, MR.ball(r, sp), border_value=0).astype(np.uint8) if r else None
        want = S.label_statistics(dv, dl, (1,), (5, 50, 95), None if mask is None else _dev(mask), sp)
        assert 0 < got['count'] and (r == 0.0) == (got['count'] == (lab == 1).sum())
        for k in ('count', 'sum', 'mean', 'variance', 'min', 'max', 'volume_mm3'):
            assert np.float64(got[k]).tobytes() == np.float64(want[k][0]).tobytes(), (r, k)
        assert got['percentiles'].tobytes() == want['percentiles'][0].tobytes() and got['box'].tobytes() == want['box'][0].tobytes()
        ref = LR.scipy_chain(vol, lab, (1,), (5, 50, 95), mask)
        assert got['count'] == ref['count'][0] and all(LR.same_value(got['percentiles'][t], ref['percentiles'][0][t]) for t in range(3))


@pytest.mark.parametrize('same_strides', (True, False))
def test_density_comparison_returns_the_known_offset(same_strides):
    """The synthesized body is the neighbour's intensities plus 16 (exact in float32 at these magnitudes), voxel for voxel: the differences of
    the means and medians against that neighbour are 16, whatever the fractured original holds."""
    S = _S()
    g = np.random.default_rng(5)
    shape = (20, 24, 40)
    lab = np.zeros(shape, dtype=np.uint8)
    lab[3:17, 4:20, 2:12], lab[3:17, 4:20, 14:24], lab[3:17, 4:20, 26:36] = 20, 21, 22
    ct = np.round(g.standard_normal(shape) * 40 + 300).astype(np.float32)
    ct[lab == 21] += 150                         # the fracture: denser
    synth = ct.copy()
    synth[lab == 21] = ct[lab == 20] + 16
    d_ct, d_lab, d_syn = _dev(ct), _dev(lab), _dev(synth)
    d_slab = _dev(lab) if same_strides else _dev(lab.transpose(2, 0, 1)).permute(1, 2, 0)
    for r in (0.0, 1.0):
        res = S.density_comparison(d_ct, d_syn, d_lab, d_slab, 21, neighbours=(20, 22), erode_mm=r)
        # the sums are integers below 2^53 (exact in any order), each mean their correctly rounded quotient: half an ulp of ~460 each
        assert abs(res['neighbour_mean_difference'][20] - 16.0) <= 2 * np.spacing(512.0) and res['neighbour_median_difference'][20] == 16.0
        one = S.vertebra_density(d_ct, d_lab, 21, erode_mm=r)
        syn = S.vertebra_density(d_syn, d_slab, 21, erode_mm=r)
        nb = S.vertebra_density(d_ct, d_lab, 22, erode_mm=r)
        for k in ('count', 'mean', 'variance', 'min', 'max'):
            assert res['original'][k] == one[k] and res['synthesized'][k] == syn[k] and res['neighbours'][22][k] == nb[k], (r, k)
        assert res['original']['percentiles'].tobytes() == one['percentiles'].tobytes()
        assert res['mean_difference'] == syn['mean'] - one['mean'] and res['median_difference'] == syn['percentiles'][1] - one['percentiles'][1]
        assert res['original']['count'] == (14 * 16 * 10 if r == 0.0 else 12 * 14 * 8)
