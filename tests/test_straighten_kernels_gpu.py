"""The four kernels of csrc/straighten.hip through their C entries (hv_straighten_stats, hv_straighten_sample_sp, hv_straighten_crop) against the
numpy restatement tests/straighten_ref.py (pinned on the host by tests/test_straighten_ref_cpu.py), at the shapes, layouts and bit patterns
the end-to-end straightening tests never reach.

Agreement is exact everywhere: the stats are integers and an order-independent min / max; the sampler and the crop are IEEE doubles in a fixed
operation order (-ffp-contract=off).  Every output lies inside a larger buffer filled with a sentinel (CT -7.0, labels 255, words -1) whose
border must survive; every source that is a view lies in a parent filled with NaN (floats), 32767 (int16 CT; extreme values for the min /
max tests, where a NaN would go unnoticed) or label 77 outside the view, so a read outside the view shows in the result."""
import ctypes

import numpy as np
import pytest
import torch

import spline_ref as P
import straighten_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64
NP = {0: np.uint8, 1: np.int16, 2: np.int32, 3: np.int64, 4: np.float32, 5: np.float64}      # HV_DT_* codes
LAYOUTS = ('c', 'f', 'zxy', 'sub', 'expand')
WIN = (ctypes.c_double(P.WINDOW[0]), ctypes.c_double(P.WINDOW[1]))
ONES = (1.0, 1.0, 1.0)
ANISO = (0.5, 0.75, 3.0)


def _lib():
    import hvgan  # noqa: F401
    from hvgan import lib
    return lib, lib.get()


def _dev(a):
    return torch.from_numpy(np.array(a, order='C')).cuda()          # a writable copy, whatever `a` is a view of


def _st(t):
    return [ctypes.c_longlong(s) for s in t.stride()]


def _code(t):
    from hvgan import straighten as S
    return S._DT[t.dtype]


def _view(a, layout, pad):
    """The values `a` ([D0][D1][D2] numpy) on the device in one memory layout -> (values the view holds, tensor view).
    c: C order; f: Fortran order; zxy: stored [D2][D0][D1] (the innermost axis is axis 1); sub: v[1:-1, 2:-2, ::2] of a parent filled with
    `pad` (its last axis 2 D2 - 1 long, so one step past either end of a line lands on padding); expand: axis 1 broadcast with stride 0."""
    D0, D1, D2 = a.shape
    if layout == 'c':
        t = _dev(a)
    elif layout == 'f':
        t = _dev(a.transpose(2, 1, 0)).permute(2, 1, 0)
    elif layout == 'zxy':
        t = _dev(a.transpose(2, 0, 1)).permute(1, 2, 0)
    elif layout == 'sub':
        parent = np.full((D0 + 2, D1 + 4, 2 * D2 - 1), pad, dtype=a.dtype)
        parent[1:-1, 2:-2, ::2] = a
        t = _dev(parent)[1:-1, 2:-2, ::2]
    else:
        a = np.ascontiguousarray(np.broadcast_to(a[:, :1, :], a.shape))
        t = _dev(a[:, :1, :]).expand(D0, D1, D2)
        assert t.stride()[1] == 0 or D1 == 1
    assert tuple(t.shape) == a.shape and np.array_equal(t.cpu().numpy(), a, equal_nan=True)
    return a, t


class _Guarded:
    """n elements of `dtype` in the middle of a buffer filled with `fill`."""

    def __init__(self, n, dtype, fill):
        self.n, self.fill = n, fill
        self.buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device='cuda')
        self.t = self.buf[GUARD:GUARD + n]

    def border_intact(self):
        return bool((self.buf[:GUARD] == self.fill).all() and (self.buf[GUARD + self.n:] == self.fill).all())

    def untouched(self):
        return bool((self.buf == self.fill).all())


# ------------------------------------------------------------------------------------------------ hv_straighten_stats
def _stats_call(ct, label, dims, rec, nbytes=None, ct_code=None, label_code=None, rec_ptr=None):
    lib, L = _lib()
    full = L.size('hv_straighten_stats_bytes', dims[1])
    zero = [ctypes.c_longlong(0)] * 3
    return L.cdll.hv_straighten_stats(lib.ptr(ct), (0 if ct is None else _code(ct)) if ct_code is None else ct_code, *(zero if ct is None else _st(ct)),
                                      lib.ptr(label), (0 if label is None else _code(label)) if label_code is None else label_code,
                                      *(zero if label is None else _st(label)), *dims, lib.ptr(rec.t) if rec_ptr is None else rec_ptr,
                                      ctypes.c_size_t(full if nbytes is None else nbytes), lib.stream())


def _stats(ct, label):
    """One hv_straighten_stats call into a guarded record -> (decoded record, the whole buffer's words)."""
    _, L = _lib()
    D1 = label.shape[1]
    rec = _Guarded(L.size('hv_straighten_stats_bytes', D1) // 8, torch.int64, -1)
    assert rec.n == R.PRES + 256 * R.rows_words(D1)
    assert _stats_call(ct, label, tuple(label.shape), rec) == 0
    torch.cuda.synchronize()
    assert rec.border_intact(), 'hv_straighten_stats wrote outside its record'
    return R.decode_stats(rec.t.cpu().numpy(), D1), rec.buf.clone()


def _same_label_part(got, ref):
    assert got['bad'] == ref['bad'] and got['word3'] == 0
    assert np.array_equal(got['counts'], ref['counts']), np.nonzero(got['counts'] != ref['counts'])
    assert np.array_equal(got['sums'], ref['sums']), np.nonzero(got['sums'] != ref['sums'])
    assert np.array_equal(got['presence'], ref['presence']), np.nonzero(got['presence'] != ref['presence'])


def _ct_pad(dtype):
    """Padding of a CT parent for the min / max tests: more extreme than any value of the cases (a NaN would not show in a min / max)."""
    return {np.int16: 32767, np.float32: 3e38, np.float64: 1.5e300}[dtype]


@pytest.mark.parametrize('shape', [(1, 1, 1), (3, 5, 300), (50, 50, 3), (7, 1, 9)], ids=lambda s: 'x'.join(str(d) for d in s))
@pytest.mark.parametrize('dtype', [np.int16, np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_stats_ct_min_max(dtype, shape):
    """(3, 5, 300): a line longer than the 256 lanes; (50, 50, 3): more rows than the 2048-block grid; a size-1 axis; one voxel.  All negative,
    all positive, mixed; the extreme at the first voxel, the last voxel and the end of the first line along each axis (the last lane of a
    partial tail, whichever axis the walk takes as its inner one), and in the long line once in each of the block's four waves."""
    base = P.case_volume(shape, 80)
    label = _dev(np.random.RandomState(81).randint(0, 4, size=shape).astype(np.uint8))
    lab_ref = R.stats_ref(None, label.cpu().numpy())
    vols = [base, base - 3000.0, base + 3000.0]
    where = [(0, 0, 0), (-1, -1, -1), (0, 0, -1), (0, -1, 0), (-1, 0, 0)]
    if shape[2] > 256:          # lanes 70, 130, 200 and 255 of a line: one per wave of the block, so each wave's partial result is the answer once
        where += [(1, 2, 70), (1, 2, 130), (1, 2, 200), (2, 4, 255)]
    for pos in where:
        for extreme in (-9000.0, 9000.0):
            v = base.copy()
            v[pos] = extreme
            vols.append(v)
    for layout in LAYOUTS:
        pad = _ct_pad(dtype)
        for k, v in enumerate(vols):
            vals, t = _view(v.astype(dtype), layout, -pad - (dtype == np.int16) if k % 2 else pad)
            got, _ = _stats(t, label)
            want = (float(vals.astype(np.float64).min()), float(vals.astype(np.float64).max()))
            assert (got['min'], got['max']) == want, (layout, k, got['min'], got['max'], want)
            _same_label_part(got, lab_ref)


def test_stats_ct_special_values_and_no_ct():
    shape = (3, 5, 70)
    label = _dev(np.random.RandomState(82).randint(0, 4, size=shape).astype(np.uint8))
    # -0.0 and +0.0 compare equal: whichever the reduction keeps, the decoded floats are == 0
    for dtype in (np.float32, np.float64):
        for v in (np.zeros(shape), -np.zeros(shape)):
            for flip in ((0, 0, 0), (2, 4, 69), None):
                v = v.copy()
                if flip is not None:
                    v[flip] = -v[flip]
                got, _ = _stats(_dev(v.astype(dtype)), label)
                assert got['min'] == 0.0 and got['max'] == 0.0
    v = np.zeros(shape, dtype=np.int16)
    v[1, 2, 3], v[2, 4, 69] = -32768, 32767
    got, _ = _stats(_dev(v), label)
    assert (got['min'], got['max']) == (-32768.0, 32767.0)
    for lo, hi in ((-1e300, 1e300), (5e-324, 1e300), (-1e300, -5e-324), (0.0, 5e-324), (-5e-324, 0.0)):
        v = np.full(shape, (lo + hi) / 2 if lo < 0 < hi else lo, dtype=np.float64)
        v[0, 0, 0], v[2, 4, 69] = hi, lo
        got, _ = _stats(_dev(v), label)
        assert (got['min'], got['max']) == (lo, hi) and got['min'] == v.min() and got['max'] == v.max(), (lo, hi, got['min'], got['max'])
    # ct = NULL: words 0 and 1 stay as the entry's memset leaves them, the label part is what it is with a CT
    with_ct, _ = _stats(_dev(v), label)
    without, _ = _stats(None, label)
    assert without['raw'] == (0, 0) and with_ct['raw'] != (0, 0)
    _same_label_part(without, R.stats_ref(None, label.cpu().numpy()))
    _same_label_part(with_ct, R.stats_ref(None, label.cpu().numpy()))


def _label_volumes(shape):
    n = int(np.prod(shape))
    rng = np.random.RandomState(83)
    x, y, z = np.indices(shape)
    last = np.zeros(shape, dtype=np.int64)
    last[-1, -1, -1] = 255
    return {'all 255 labels': rng.permutation(np.arange(n) % 256).reshape(shape),
            'a change at every voxel along every axis': 1 + (x + 2 * y + 3 * z) % 7,
            'a single label': np.full(shape, 5, dtype=np.int64),
            'all zero': np.zeros(shape, dtype=np.int64),
            '255 at the very last voxel': last}


@pytest.mark.parametrize('code', sorted(NP), ids=lambda c: np.dtype(NP[c]).name)
def test_stats_label_counts_sums_and_presence(code):
    """Every label dtype in every layout: the walk's inner axis is axis 2 in C order, axis 0 in Fortran order, axis 1 in the [D2][D0][D1]
    storage and for the stride-0 axis 1 (the smallest stride sorts first); label 77 lies around the sub-box."""
    shape = (16, 20, 12)
    vols = _label_volumes(shape)
    assert len(np.unique(vols['all 255 labels'])) == 256
    inner = set()
    for layout in LAYOUTS:
        for name, v in vols.items():
            vals, t = _view(v.astype(NP[code]), layout, 77)
            got, _ = _stats(None, t)
            ref = R.stats_ref(None, vals)
            assert not ref['bad'] and not got['bad'], (layout, name)
            _same_label_part(got, ref)
        st = t.stride()
        inner.add(min(range(3), key=lambda a: abs(st[a])))
    assert inner == {0, 1, 2}


@pytest.mark.parametrize('D2', [4, 5])
@pytest.mark.parametrize('D1', [1, 2, 7, 128, 129, 131])
def test_stats_presence_words_of_the_raw_geometry(D1, D2):
    """R = D1 - D1 // 2 rows from D1 // 2 on, Rw = ceil(R / 64) words per label: one word up to D1 = 128, two from 129 on.  Labels that occur
    only in row D1 // 2 - 1 or only beside the centre column set no bit."""
    D0, row0, zc = 3, D1 // 2, D2 // 2
    R_, Rw = D1 - row0, R.rows_words(D1)
    assert Rw == {1: 1, 2: 1, 7: 1, 128: 1, 129: 2, 131: 2}[D1]
    rng = np.random.RandomState(84 + D1 + D2)
    v = rng.randint(0, 6, size=(D0, D1, D2)) * (rng.rand(D0, D1, D2) < 0.5)
    v[1, :, zc + 1:] = 0
    v[1, :, :zc] = 0
    v[1, row0:, zc] = 12                      # every row: all R bits
    v[2, D1 - 1, zc] = 13                     # the last row only: the top bit
    v[0, :, zc - 1] = 10                      # beside the centre column, below and (where there is one) above
    if zc + 1 < D2:
        v[0, :, zc + 1] = 11
    if row0 >= 1:
        v[0, row0 - 1, zc] = 9                # the row before the first
    for code, layouts in ((0, LAYOUTS), (5, ('zxy', 'sub')), (3, ('f',))):
        for layout in layouts:
            vals, t = _view(v.astype(NP[code]), layout, 77)
            got, _ = _stats(None, t)
            ref = R.stats_ref(None, vals)
            _same_label_part(got, ref)
            p = [[int(w) for w in row] for row in got['presence']]
            assert p[77] == [0] * Rw and p[0] == [0] * Rw
            if layout != 'expand':            # (the broadcast volume repeats row 0)
                assert p[9] == [0] * Rw and p[10] == [0] * Rw and p[11] == [0] * Rw
                assert sum(w << (64 * i) for i, w in enumerate(p[12])) == (1 << R_) - 1
                assert sum(w << (64 * i) for i, w in enumerate(p[13])) == 1 << (R_ - 1)


def test_stats_bad_label_flag():
    """One bad value as the last voxel of a valid volume: the flag is set, the voxel counts as 0 and every other count is unchanged."""
    shape = (5, 6, 7)
    v = np.random.RandomState(85).randint(0, 200, size=shape)
    v[-1, -1, -1] = 3
    clean = R.stats_ref(None, v)
    for code in sorted(NP):
        got, _ = _stats(None, _dev(v.astype(NP[code])))
        assert not got['bad']
        _same_label_part(got, clean)
    bads = {4: (256.0, -1.0, 0.5, np.nan, np.inf), 5: (256.0, -1.0, 0.5, np.nan, np.inf, -np.inf, 255.5), 1: (256, -1), 2: (256, -1), 3: (256, -1, 2 ** 40)}
    for code, values in bads.items():
        for bad in values:
            w = v.astype(NP[code])
            w[-1, -1, -1] = bad
            for layout in ('c', 'f'):
                vals, t = _view(w, layout, 77)
                got, _ = _stats(None, t)
                ref = R.stats_ref(None, vals)
                assert ref['bad'] and got['bad'], (code, bad)
                _same_label_part(got, ref)
                assert got['counts'][3] == clean['counts'][3] - 1 and got['counts'].sum() == clean['counts'].sum() - 1


def test_stats_refusals_leave_the_record_untouched():
    lib, L = _lib()
    dims = (4, 9, 5)
    ct, label = _dev(P.case_volume(dims, 86)), _dev(np.ones(dims, dtype=np.uint8))
    u8ct = _dev(np.ones(dims, dtype=np.uint8))
    nbytes = L.size('hv_straighten_stats_bytes', dims[1])
    rec = _Guarded(nbytes // 8, torch.int64, -1)
    assert _stats_call(ct, label, dims, rec, nbytes=nbytes - 1) == -3
    assert _stats_call(ct, label, dims, rec, rec_ptr=ctypes.c_void_p(rec.t.data_ptr() + 4)) == -3
    assert _stats_call(ct, None, dims, rec) == -1
    assert _stats_call(ct, label, dims, rec, rec_ptr=ctypes.c_void_p(0)) == -1
    for bad_dims in ((0, 9, 5), (4, 0, 5), (4, 9, 0), (-1, 9, 5), (4, -1, 5), (4, 9, -1)):
        assert _stats_call(ct, label, bad_dims, rec) == -1, bad_dims
    assert _stats_call(u8ct, label, dims, rec) == -1                  # a uint8 CT
    for code in (0, 2, 3, 6, -1):
        assert _stats_call(ct, label, dims, rec, ct_code=code) == -1, code
    for code in (6, -1):
        assert _stats_call(ct, label, dims, rec, label_code=code) == -1, code
        assert _stats_call(None, label, dims, rec, label_code=code) == -1, code
    torch.cuda.synchronize()
    assert rec.untouched()
    assert _stats_call(None, label, dims, rec, ct_code=0) == 0        # without a CT its dtype code is not looked at
    torch.cuda.synchronize()
    assert rec.border_intact() and not rec.untouched()


# ------------------------------------------------------------------------------------------------ hv_straighten_sample_sp, order 1
def _sample_call(ct, label, dims, knots, basis, N, PA, PB, win, sct, slab, pres, spacing=ONES, pbytes=None, ct_code=None):
    lib, L = _lib()
    full = L.size('hv_straighten_presence_bytes', PA)
    zero = [ctypes.c_longlong(0)] * 3
    sp = None if spacing is None else (ctypes.c_double * 3)(*spacing)
    return L.cdll.hv_straighten_sample_sp(lib.ptr(ct), (0 if ct is None else _code(ct)) if ct_code is None else ct_code, *(zero if ct is None else _st(ct)),
                                          lib.ptr(label), 0 if label is None else _code(label), *(zero if label is None else _st(label)), *dims,
                                          lib.ptr(knots), lib.ptr(basis), N, PA, PB, int(win), *WIN, lib.ptr(sct), lib.ptr(slab), lib.ptr(pres),
                                          ctypes.c_size_t(full if pbytes is None else pbytes), sp, lib.stream())


class _Straight:
    """Guarded outputs of one sampling call: sct [N][PA][PB] in -7.0, slab in 255, the presence words in -1."""

    def __init__(self, N, PA, PB):
        _, L = _lib()
        self.shape = (N, PA, PB)
        self.sct = _Guarded(N * PA * PB, torch.float64, -7.0)
        self.slab = _Guarded(N * PA * PB, torch.uint8, 255)
        self.pres = _Guarded(L.size('hv_straighten_presence_bytes', PA) // 8, torch.int64, -1)
        assert self.pres.n == 256 * R.rows_words(PA)

    def borders_intact(self):
        return self.sct.border_intact() and self.slab.border_intact() and self.pres.border_intact()

    def untouched(self):
        return self.sct.untouched() and self.slab.untouched() and self.pres.untouched()

    def numpy(self):
        return (self.sct.t.cpu().numpy().reshape(self.shape), self.slab.t.cpu().numpy().reshape(self.shape),
                self.pres.t.cpu().numpy().view(np.uint64).reshape(256, -1))

    def bits(self):
        return self.sct.buf.view(torch.int64).clone(), self.slab.buf.clone(), self.pres.buf.clone()


def _sample(ct, label, knots, basis, PA, PB, spacing, win):
    N = len(knots)
    out = _Straight(N, PA, PB)
    dk, db = _dev(np.asarray(knots, dtype=np.float64)), _dev(np.asarray(basis, dtype=np.float64))
    assert _sample_call(ct, label, tuple(ct.shape), dk, db, N, PA, PB, win, out.sct.t, out.slab.t, out.pres.t, spacing) == 0
    torch.cuda.synchronize()
    assert out.borders_intact(), 'hv_straighten_sample_sp wrote outside its outputs'
    return out


def _same_straight(out, ct_vals, lab_vals, knots, basis, PA, PB, spacing, win, what):
    want_ct, want_lab, want_pres = R.sample_ref(ct_vals, lab_vals, knots, basis, PA, PB, spacing, win, *P.WINDOW)
    got_ct, got_lab, got_pres = out.numpy()
    assert not np.isnan(got_ct).any(), (what, 'a NaN of the padding reached the output')
    assert np.array_equal(got_lab, want_lab), (what, int((got_lab != want_lab).sum()))
    assert np.array_equal(got_pres, want_pres), (what, np.nonzero(got_pres != want_pres))
    assert np.array_equal(got_ct.view(np.int64), want_ct.view(np.int64)), (what, np.abs(got_ct - want_ct).max())
    return want_ct, want_lab, want_pres


def _eye(n):
    return np.tile(np.eye(3), (n, 1, 1))


def _frame(kind, shape, N, PA, PB, spacing):
    """knots [N][3] (millimetres) and basis [N][3][3] of one frame over a scan of `shape` voxels at `spacing`."""
    from hvgan import straighten as S
    sp = np.asarray(spacing)
    if kind in ('lattice', 'half'):
        # identity frame: sample (n, a, b) at (x_n voxels, b - b0 + frac mm, a - a0 + frac mm).  Column b0 and row a0 land on voxel 0: a few
        # before the centre, so the centre column and the rows after PA // 2 are inside; a plane with two presence words ends at the scan's
        # last voxel instead, so that its last row (bit 64) is inside too
        frac = 0.0 if kind == 'lattice' else 0.5
        x = np.minimum(np.arange(N) % shape[0] + (frac if N > 1 else 0.0), shape[0] - 1.0)
        b0 = max(0, PB // 2 - 4)
        a0 = PA - shape[2] if PA > 64 else max(0, PA // 2 - 3)
        knots = np.stack([x * sp[0], np.full(N, PB / 2.0 - b0 + frac), np.full(N, PA / 2.0 - a0 + frac)], axis=1)
        return knots, _eye(N)
    if kind == 'curve':
        curve = np.array([[5.0, 5.0, 3.0], [6.0, 6.0, 6.0], [8.0, 6.5, 9.0], [9.0, 7.0, 13.0]])
        knots, basis = S.curve_frame(curve, 1, spacing)
        assert len(knots) >= N and np.abs(basis - basis[0]).max() > 0.05
        return knots[:N], basis[:N]
    # 'faces': a tilted orthonormal frame whose knots run from outside the volume through it and out again
    q, _ = np.linalg.qr(np.random.RandomState(87).randn(3, 3))
    lo, hi = -1.5 * np.ones(3), np.asarray(shape, dtype=np.float64) + 0.5
    t = np.linspace(0.0, 1.0, N)[:, None] if N > 1 else np.array([[0.5]])
    return (lo + (hi - lo) * t) * sp, np.tile(q, (N, 1, 1))


PLANES = [(1, 1, 1), (2, 8, 6), (9, 16, 16), (3, 29, 31), (2, 130, 3), (1, 129, 2)]


@pytest.mark.parametrize('kind', ['lattice', 'half', 'curve', 'faces'])
@pytest.mark.parametrize('plane', PLANES, ids=lambda p: 'x'.join(str(d) for d in p))
def test_sample_order_1_against_the_restatement(plane, kind):
    """(1, 1, 1): one sample; (2, 8, 6): under one block; (9, 16, 16): exactly 9 blocks in a grid of 16, so the renumbered blocks 9 .. 15 leave
    at blk >= nblk; (3, 29, 31): an odd, unequal plane with a partial last block; 130 and 129 rows: two presence words per label.  Every CT
    dtype with the window off and on, both spacings, the layouts and the label dtypes in rotation (each at least once per frame)."""
    N, PA, PB = plane
    shape = (14, 12, 16) if kind == 'curve' else (9, 11, 13)
    rng = np.random.RandomState(88)
    ct64 = P.case_volume(shape, 89) + rng.randint(0, 8, size=shape) / 8.0          # exact in float32
    lab = rng.randint(0, 5, size=shape)
    lab[:, 3, :] = 77                                                              # the padding's label, in the volume too
    k = PLANES.index(plane)
    for spacing in (ONES, ANISO):
        knots, basis = _frame(kind, shape, N, PA, PB, spacing)
        grid = P.straight_grid(knots, basis, spacing, plane=(PB, PA))
        if kind == 'lattice' and spacing == ONES:
            assert (grid == np.floor(grid)).all()
        if kind == 'half' and spacing == ONES:
            assert ((grid[1:] + 0.5) == np.floor(grid[1:] + 0.5)).all()            # every nearest sample is a tie on axes 1 and 2
        if kind == 'faces' and PA >= 29:
            for a in range(3):
                assert grid[a].min() < 0.0 and grid[a].max() > shape[a] - 1        # the planes leave through every face
        for ct_dtype in (np.int16, np.float32, np.float64):
            for win in (0, 1):
                ct_layout, lab_layout = LAYOUTS[k % 5], LAYOUTS[(k + 2) % 5]
                code = sorted(NP)[k % 6]
                k += 1
                src = np.round(ct64) if ct_dtype == np.int16 else ct64
                ct_vals, ct = _view(src.astype(ct_dtype), ct_layout, 32767 if ct_dtype == np.int16 else np.nan)
                lab_vals, label = _view(lab.astype(NP[code]), lab_layout, 77)
                what = (spacing, np.dtype(ct_dtype).name, win, ct_layout, np.dtype(NP[code]).name, lab_layout)
                out = _sample(ct, label, knots, basis, PA, PB, spacing, win)
                want_ct, want_lab, _ = _same_straight(out, ct_vals, lab_vals, knots, basis, PA, PB, spacing, win, what)
        if kind in ('curve', 'lattice') and N * PA * PB > 1:
            assert want_lab.any() and (want_ct != 0.0).any()


def test_sample_faces_exactly_on_and_just_past_each_face():
    """Identity frame as in tests/test_spline_gpu.py::test_boundary_rule_matches_scipy: PB = 11, ky = 5.5 puts axis 1 at 0 .. 10 = D1 - 1, PA = 13,
    kz = 6.5 axis 2 at 0 .. 12 = D2 - 1, the knots axis 0 at 0 and D0 - 1.  Adding 1e-7 or -1e-9 to one knot component moves the last / first
    sample of that axis just outside: 0 in both outputs, no presence bit.  The float CT and label sit in NaN / 77 padding: an upper-corner
    read at c = D - 1 would show."""
    shape = (9, 11, 13)
    PA, PB = 13, 11
    rng = np.random.RandomState(90)
    ct64 = P.case_volume(shape, 91) + 0.5
    lab = rng.randint(1, 5, size=shape)
    base = np.array([[0.0, 5.5, 6.5], [8.0, 5.5, 6.5], [4.0, 5.5, 6.5]])
    for axis in range(3):
        for eps in (0.0, 1e-7, -1e-9):
            knots = base.copy()
            knots[:, axis] += eps
            grid = P.straight_grid(knots, _eye(3), ONES, plane=(PB, PA))
            if eps == 0.0:
                for a in range(3):
                    assert grid[a].min() == 0.0 and grid[a].max() == shape[a] - 1.0
            for ct_dtype, layout in ((np.float64, 'sub'), (np.float32, 'sub'), (np.int16, 'zxy')):
                ct_vals, ct = _view(ct64.astype(ct_dtype), layout, np.nan)
                lab_vals, label = _view(lab.astype(np.uint8), 'sub', 77)
                for win in (0, 1):
                    out = _sample(ct, label, knots, _eye(3), PA, PB, ONES, win)
                    _same_straight(out, ct_vals, lab_vals, knots, _eye(3), PA, PB, ONES, win, (axis, eps, np.dtype(ct_dtype).name, win))
                    got_ct, got_lab, got_pres = out.numpy()
                    outside = ((grid < 0.0) | (grid > np.array(shape, dtype=np.float64).reshape(3, 1, 1, 1) - 1.0)).any(0)
                    assert outside.any() == (eps != 0.0)
                    assert (got_ct[outside] == 0.0).all() and (got_lab[outside] == 0).all() and (got_lab[~outside] != 0).all()
                    if eps == 0.0 and not win:       # on the lattice, the faces included: the voxels themselves
                        assert np.array_equal(got_ct[1], ct_vals[8].astype(np.float64).T) and np.array_equal(got_lab[0], lab_vals[0].T)
                    if eps != 0.0 and axis == 2:     # the row that left the volume (a = 12 or a = 0) holds no label: no bit for it
                        gone = 12 if eps > 0 else 0
                        assert outside[:, gone, :].all()
                        if gone >= PA // 2:
                            assert not ((got_pres[:, 0] >> np.uint64(gone - PA // 2)) & np.uint64(1)).any()


def test_sample_nearest_ties_and_presence_beside_the_centre():
    """Coordinates at x.5 take the label at floor(c + 0.5), the upper voxel.  Labels that occur only in column PB // 2 - 1 or row PA // 2 - 1
    of the straight volume set no presence bit; the same labels in the centre column from row PA // 2 on do."""
    shape = (9, 11, 13)
    N, PA, PB = 3, 10, 8
    ct = _dev(P.case_volume(shape, 92))
    # identity frame, plane at voxels (b + 1, a + 1) of axes 1, 2: straight (n, a, b) = scan (n + 2, b + 1, a + 1)
    knots = np.array([[n + 2.0, PB / 2.0 + 1.0, PA / 2.0 + 1.0] for n in range(N)])
    lab = np.zeros(shape, dtype=np.uint8)
    lab[2:5, 1:9, 1:11] = 1
    lab[3, PB // 2 - 1 + 1, 1:11] = 20              # straight column b = PB // 2 - 1, every row
    lab[4, 1:9, PA // 2 - 1 + 1] = 21               # straight row a = PA // 2 - 1, every column
    lab[2, PB // 2 + 1, PA // 2 + 1 + 3] = 22       # centre column, row PA // 2 + 3
    out = _sample(ct, _dev(lab), knots, _eye(N), PA, PB, ONES, 0)
    _, want_lab, want_pres = _same_straight(out, ct.cpu().numpy(), lab, knots, _eye(N), PA, PB, ONES, 0, 'beside the centre')
    assert (want_lab == 20).sum() == PA and (want_lab == 21).sum() == PB and (want_lab == 22).sum() == 1
    p = out.numpy()[2]
    assert p[20, 0] == 0 and p[21, 0] == 0 and p[22, 0] == 1 << 3 and p[1, 0] != 0
    # ties: every sample half-way between two voxels on all three axes
    lab = np.random.RandomState(93).randint(1, 9, size=shape).astype(np.uint8)
    half = knots + 0.5
    out = _sample(ct, _dev(lab), half, _eye(N), PA, PB, ONES, 0)
    _same_straight(out, ct.cpu().numpy(), lab, half, _eye(N), PA, PB, ONES, 0, 'ties')
    assert np.array_equal(out.numpy()[1], lab[3:6, 2:10, 2:12].transpose(0, 2, 1))        # the upper voxel on every axis


def test_sample_refusals_leave_the_outputs_untouched():
    lib, L = _lib()
    dims = (6, 5, 7)
    ct, label = _dev(P.case_volume(dims, 94)), _dev(np.ones(dims, dtype=np.uint8))
    u8 = _dev(np.ones(dims, dtype=np.uint8))
    N, PA, PB = 2, 4, 4
    out = _Straight(N, PA, PB)
    dk, db = _dev(np.array([[2.0, 2.0, 3.0], [3.0, 2.0, 3.0]])), _dev(_eye(2))

    def call(ct=ct, label=label, dims=dims, k=dk, b=db, n=N, pa=PA, pb=PB, sct=out.sct.t, slab=out.slab.t, pres=out.pres.t, **kw):
        return _sample_call(ct, label, dims, k, b, n, pa, pb, 0, sct, slab, pres, **kw)

    inf, nan = float('inf'), float('nan')
    for sp in ((0.0, 1.0, 1.0), (1.0, -1.0, 1.0), (1.0, 1.0, nan), (inf, 1.0, 1.0), (1.0, 1.0, -inf), None):
        assert call(spacing=sp) == -1, sp
    for kw in (dict(n=0), dict(n=-1), dict(pa=0), dict(pb=0), dict(ct=None), dict(label=None), dict(k=None), dict(b=None), dict(sct=None),
               dict(slab=None), dict(pres=None), dict(ct=u8), dict(ct_code=0), dict(ct_code=6), dict(dims=(6, 0, 7)), dict(dims=(0, 5, 7))):
        assert call(**kw) == -1, kw
    pbytes = L.size('hv_straighten_presence_bytes', PA)
    assert call(pbytes=pbytes - 1) == -3
    torch.cuda.synchronize()
    assert out.untouched()
    assert call() == 0
    torch.cuda.synchronize()
    assert out.borders_intact() and not out.sct.untouched()


# ------------------------------------------------------------------------------------------------ hv_straighten_crop
def _crop_call(ct, label, D1, win, pres, boxes, V, O, out_ct, out_lab, ct_code=None):
    lib, L = _lib()
    zero = [ctypes.c_longlong(0)] * 3
    return L.cdll.hv_straighten_crop(lib.ptr(ct), (0 if ct is None else _code(ct)) if ct_code is None else ct_code, *(zero if ct is None else _st(ct)),
                                     lib.ptr(label), 0 if label is None else _code(label), *(zero if label is None else _st(label)), D1, int(win),
                                     *WIN, lib.ptr(pres), lib.ptr(boxes), V, *O, lib.ptr(out_ct), lib.ptr(out_lab), lib.stream())


def _crop(ct, label, D1, win, pres, boxes, O):
    """One hv_straighten_crop call into guarded outputs -> (ct [V][*O], label [V][*O], the two buffers)."""
    V, vol = len(boxes), int(np.prod(O))
    oc, ol = _Guarded(V * vol, torch.float64, -7.0), _Guarded(V * vol, torch.uint8, 255)
    d_boxes = _dev(np.asarray(boxes, dtype=np.int32).reshape(V, 9))
    assert _crop_call(ct, label, D1, win, pres, d_boxes, V, O, oc.t, ol.t) == 0
    torch.cuda.synchronize()
    assert oc.border_intact() and ol.border_intact(), 'hv_straighten_crop wrote outside its outputs'
    return oc.t.cpu().numpy().reshape((V,) + tuple(O)), ol.t.cpu().numpy().reshape((V,) + tuple(O)), (oc.buf.view(torch.int64).clone(), ol.buf.clone())


def _boxes(src, O):
    """Named boxes of an out_size O crop from a source of shape src, each inside the source; `full` and `inside` lie around the source's
    centre, where the rows from D1 // 2 on (the ones a cutoff can remove) are."""
    n = [min(O[i], src[i]) for i in range(3)]
    mid = lambda ln: [max(0, min(src[i] - ln[i], src[i] // 2 - ln[i] // 2)) for i in range(3)]    # noqa: E731
    full = mid(n) + n + [(O[i] - n[i]) // 2 for i in range(3)]                         # len == O wherever the source is long enough
    ln = [max(1, n[i] - 1 - (src[i] > 2)) for i in range(3)]
    inside = mid(ln) + ln + [O[i] - ln[i] for i in range(3)]                           # low-side padding on every axis
    ln = [max(1, n[i] // 2) for i in range(3)]
    far = [src[i] - ln[i] for i in range(3)] + ln + [(O[i] - ln[i]) // 2 for i in range(3)]       # ends at the source's far corner
    out = {'full': full, 'inside': inside, 'far': far}
    for a in range(3):
        z = list(full)
        z[3 + a] = 0
        out['zero%d' % a] = z
    for b in out.values():
        assert all(0 <= b[i] and b[i] + b[3 + i] <= src[i] and 0 <= b[6 + i] and b[6 + i] + b[3 + i] <= O[i] for i in range(3)), b
    assert all(s > 0 for s in inside[6:9])
    return out


OUT_SIZES = [(5, 7, 3), (16, 16, 2), (9, 10, 11)]         # 105 voxels: under one block; 512: exactly two; 990: a partial last block


def _crop_cases(src, O):
    b = _boxes(src, O)
    singles = [[b[k]] for k in ('full', 'inside', 'far', 'zero0', 'zero1', 'zero2')]
    triples = [[b['inside'], b['far'], b['zero0']], [b['full'], b['full'], b['zero1']], [b['zero2'], b['inside'], b['full']]]
    return singles + triples


@pytest.mark.parametrize('O', OUT_SIZES, ids=lambda s: 'x'.join(str(d) for d in s))
@pytest.mark.parametrize('plane', [(9, 16, 16), (3, 29, 31), (2, 130, 3)], ids=lambda p: 'x'.join(str(d) for d in p))
def test_crop_of_straight_volumes(plane, O):
    """The first source form: the sampler's own outputs (float64 CT, uint8 label, contiguous, window off, D1 = PA) with the presence words it
    wrote, V = 1 and V = 3: boxes inside, with low-side padding, with a zero-length axis, with len == O, ending at the far corner, twice the
    same."""
    N, PA, PB = plane
    shape = (14, 12, 16)
    rng = np.random.RandomState(95)
    ct_vals = P.case_volume(shape, 96) + 0.25
    lab_vals = rng.randint(0, 5, size=shape).astype(np.uint8)
    knots, basis = _frame('curve', shape, N, PA, PB, ONES)
    out = _sample(_dev(ct_vals), _dev(lab_vals), knots, basis, PA, PB, ONES, 1)
    sct, slab, pres = _same_straight(out, ct_vals, lab_vals, knots, basis, PA, PB, ONES, 1, plane)
    cut = R.cutoffs(PA, pres)
    present = [l for l in range(1, 5) if (slab == l).any()]
    assert len(present) >= 2 and len({int(cut[l]) for l in present}) >= 2, 'the labels of one crop should not all share a cutoff'
    t_ct, t_lab = out.sct.t.view(N, PA, PB), out.slab.t.view(N, PA, PB)
    cut_something = False
    for boxes in _crop_cases((N, PA, PB), O):
        got_ct, got_lab, _ = _crop(t_ct, t_lab, PA, 0, out.pres.t, boxes, O)
        want_ct, want_lab = R.crop_ref(sct, slab, PA, 0, *P.WINDOW, pres, boxes, O)
        assert np.array_equal(got_lab, want_lab), (boxes, int((got_lab != want_lab).sum()))
        assert np.array_equal(got_ct.view(np.int64), want_ct.view(np.int64)), boxes
        for v, bx in enumerate(boxes):
            if min(bx[3:6]) == 0:
                assert not got_ct[v].any() and not got_lab[v].any()
        uncut = R.crop_ref(sct, slab, PA, 0, *P.WINDOW, np.full_like(pres, ~np.uint64(0)), boxes, O)[1]
        cut_something |= not np.array_equal(uncut, want_lab)
    assert cut_something


@pytest.mark.parametrize('O', OUT_SIZES, ids=lambda s: 'x'.join(str(d) for d in s))
def test_crop_of_a_raw_scan_with_the_stats_presence_words(O):
    """The second source form (one centroid): the raw scan in a permuted layout, any CT and label dtype, windowed in the crop, cut by the
    presence words hv_straighten_stats left in its record."""
    shape = (12, 21, 13)
    rng = np.random.RandomState(97)
    ct64 = P.case_volume(shape, 98) + rng.randint(0, 8, size=shape) / 8.0
    lab = rng.randint(0, 5, size=shape)
    lab[:, 10:, 6] = 0
    for l in range(1, 5):
        lab[l, 10:10 + l, 6] = l                # the centre column from row D1 // 2 on: label l in its first l rows, so its cutoff is 10 + l
    _, L = _lib()
    combos = [(np.int16, 'zxy', 0, 'f'), (np.float32, 'f', 3, 'sub'), (np.float64, 'sub', 5, 'zxy'), (np.float64, 'zxy', 1, 'c'), (np.float32, 'sub', 2, 'f'),
              (np.int16, 'f', 4, 'zxy')]
    for ct_dtype, ct_layout, code, lab_layout in combos:
        src = np.round(ct64) if ct_dtype == np.int16 else ct64
        ct_vals, ct = _view(src.astype(ct_dtype), ct_layout, 32767 if ct_dtype == np.int16 else np.nan)
        lab_vals, label = _view(lab.astype(NP[code]), lab_layout, 77)
        rec = _Guarded(L.size('hv_straighten_stats_bytes', shape[1]) // 8, torch.int64, -1)
        assert _stats_call(ct, label, shape, rec) == 0
        ref = R.stats_ref(ct_vals, lab_vals)
        cut = R.cutoffs(shape[1], ref['presence'])
        assert [int(cut[l]) for l in range(1, 5)] == [11, 12, 13, 14]
        for win in (0, 1):
            for boxes in _crop_cases(shape, O):
                got_ct, got_lab, _ = _crop(ct, label, shape[1], win, rec.t[R.PRES:], boxes, O)
                want_ct, want_lab = R.crop_ref(ct_vals, lab_vals, shape[1], win, *P.WINDOW, ref['presence'], boxes, O)
                if boxes[0][3:6] == [min(O[i], shape[i]) for i in range(3)]:      # the centred full box: the cutoff removes something
                    assert (want_lab[0] != R.crop_ref(ct_vals, lab_vals, shape[1], win, *P.WINDOW, ref['presence'] | ~np.uint64(0), boxes, O)[1][0]).any()
                what = (np.dtype(ct_dtype).name, ct_layout, code, lab_layout, win, boxes)
                assert not np.isnan(got_ct).any(), what
                assert np.array_equal(got_lab, want_lab), what
                assert np.array_equal(got_ct.view(np.int64), want_ct.view(np.int64)), what
        assert rec.border_intact()


FULL = (1 << 64) - 1


def _cut_cases(D1):
    """{label: (presence words, expected cutoff row)} written by hand for a source of D1 rows."""
    row0 = D1 // 2
    R_ = D1 - row0
    Rw = R.rows_words(D1)
    allR = (1 << R_) - 1
    cases = {1: (0, row0),                                   # no bit: everything from row D1 // 2 on goes
             2: (allR, D1),                                  # all R bits (R = 64: the full word; R = 65: the full word and one bit): nothing goes
             3: (allR & ~1, row0),                           # first clear bit at h = 0, set bits after it
             4: ((allR | (FULL << R_)) & ~(1 << (R_ + 2)), D1),      # set bits at positions >= R and a clear one past R: ignored
             9: (allR | (FULL << R_), D1),                   # every bit of every word
             5: (allR & ~(1 << (R_ - 1)), D1 - 1),           # first clear bit at the last row
             6: (allR & ~(1 << (R_ // 2)) & ~(1 << (R_ - 1)), row0 + R_ // 2)}      # two clear bits: the first one counts
    if R_ > 63:
        cases[7] = ((allR | (FULL << R_)) & ~(1 << 63), row0 + 63)     # first clear bit at h = 63, everything after it set
    if R_ > 64:
        cases[8] = ((allR | (FULL << R_)) & ~(1 << 64), row0 + 64)     # first clear bit at h = 64: the second word's bit 0
    words = np.zeros((256, Rw), dtype=np.uint64)
    for l, (bits, _) in cases.items():
        for w in range(Rw):
            words[l, w] = (bits >> (64 * w)) & FULL
    return words, {l: c for l, (_, c) in cases.items()}


@pytest.mark.parametrize('D1', [7, 128, 130])
def test_crop_cutoff_from_hand_written_presence_words(D1):
    """R = 4, 64 and 65 rows from D1 // 2 on (one word, exactly one full word, a second word).  The source is D1 + 3 rows tall while the entry
    is told D1: a label voxel in a row >= D1 is at or past every cutoff and goes, even for a label whose words have bits set at and past R --
    which is how an unclamped first-clear-bit position shows."""
    D0, D2, tall = 3, 4, D1 + 3
    words, expect = _cut_cases(D1)
    labs = sorted(expect)
    x, y, z = np.indices((D0, tall, D2))
    lab = np.array(labs)[(x * D2 + z + y) % len(labs)].astype(np.uint8)               # every row holds every label
    ct_vals = P.case_volume((D0, tall, D2), 99) + 0.5
    assert [int(c) for c in R.cutoffs(D1, words)[labs]] == [expect[l] for l in labs]
    ct, label, pres = _dev(ct_vals), _dev(lab), _dev(words.view(np.int64))
    O = (D0, tall, D2)
    box = [[0, 0, 0, D0, tall, D2, 0, 0, 0]]
    got_ct, got_lab, _ = _crop(ct, label, D1, 0, pres, box, O)
    want = lab.copy()
    for l in labs:
        rows = np.arange(tall)[None, :, None] >= expect[l]
        want[(lab == l) & rows] = 0
    assert np.array_equal(R.crop_ref(ct_vals, lab, D1, 0, *P.WINDOW, words, box, O)[1][0], want)
    assert np.array_equal(got_lab[0], want), {l: int(((got_lab[0] != want) & (lab == l)).sum()) for l in labs}
    assert np.array_equal(got_lab[0][:, :D1 // 2], lab[:, :D1 // 2]) and not got_lab[0][:, D1:].any()      # never below D1 // 2, always from D1 on
    assert (got_lab[0][:, :D1] == 2).sum() == (lab[:, :D1] == 2).sum() and (got_lab[0][:, :D1] == 4).sum() == (lab[:, :D1] == 4).sum()
    assert len({expect[l] for l in labs}) >= 4                                       # several cutoffs in the one crop
    assert np.array_equal(got_ct[0], ct_vals)
    # the CT does not depend on the cutoff: the same bytes with every bit set, and with none
    for fill in (-1, 0):
        other = _crop(ct, label, D1, 0, torch.full_like(pres, fill), box, O)
        assert np.array_equal(other[0].view(np.int64), got_ct.view(np.int64))
        if fill == -1:
            assert np.array_equal(other[1][0][:, :D1], lab[:, :D1]) and not other[1][0][:, D1:].any()
    # a sub-range of the rows, shifted in the output: the cutoff goes by the source row
    lo, n = D1 // 2 - 1, min(5, tall - (D1 // 2 - 1))
    sub = [[0, lo, 1, D0, n, 2, 0, 2, 1]]
    got = _crop(ct, label, D1, 0, pres, sub, (D0, 8, D2))
    want_sub = np.zeros((D0, 8, D2), dtype=np.uint8)
    want_sub[:, 2:2 + n, 1:3] = want[:, lo:lo + n, 1:3]
    assert np.array_equal(got[1][0], want_sub)


def test_crop_refusals_leave_the_outputs_untouched():
    dims = (6, 5, 7)
    ct, label = _dev(P.case_volume(dims, 100)), _dev(np.ones(dims, dtype=np.uint8))
    u8 = _dev(np.ones(dims, dtype=np.uint8))
    pres = _dev(np.zeros(256, dtype=np.int64))
    boxes = _dev(np.array([[0, 0, 0, 4, 4, 4, 0, 0, 0]], dtype=np.int32))
    O = (4, 4, 4)
    oc, ol = _Guarded(64, torch.float64, -7.0), _Guarded(64, torch.uint8, 255)

    def call(ct=ct, label=label, d1=5, pres=pres, boxes=boxes, v=1, o=O, oc=oc.t, ol=ol.t, **kw):
        return _crop_call(ct, label, d1, 0, pres, boxes, v, o, oc, ol, **kw)

    for kw in (dict(v=0), dict(v=-1), dict(ct=None), dict(label=None), dict(pres=None), dict(boxes=None), dict(oc=None), dict(ol=None), dict(ct=u8),
               dict(ct_code=0), dict(ct_code=6), dict(d1=0), dict(o=(0, 4, 4)), dict(o=(4, 4, -1))):
        assert call(**kw) == -1, kw
    assert call(v=65536) == -2
    torch.cuda.synchronize()
    assert oc.untouched() and ol.untouched()
    assert call() == 0
    torch.cuda.synchronize()
    assert oc.border_intact() and ol.border_intact() and not oc.untouched()


# ------------------------------------------------------------------------------------------------ determinism
def test_two_runs_give_the_same_bytes():
    shape = (14, 12, 16)
    rng = np.random.RandomState(101)
    ct_vals, ct = _view((P.case_volume(shape, 102) + 0.125).astype(np.float32), 'zxy', np.nan)
    lab_vals, label = _view(rng.randint(0, 200, size=shape).astype(np.int16), 'f', 77)
    a, b = _stats(ct, label), _stats(ct, label)
    assert torch.equal(a[1], b[1])
    N, PA, PB = 9, 16, 16
    knots, basis = _frame('curve', shape, N, PA, PB, ANISO)
    runs = [_sample(ct, label, knots, basis, PA, PB, ANISO, 1) for _ in range(2)]
    assert all(torch.equal(x, y) for x, y in zip(runs[0].bits(), runs[1].bits()))
    out = runs[0]
    boxes = _crop_cases((N, PA, PB), (9, 10, 11))[-1]
    crops = [_crop(out.sct.t.view(N, PA, PB), out.slab.t.view(N, PA, PB), PA, 0, out.pres.t, boxes, (9, 10, 11))[2] for _ in range(2)]
    assert all(torch.equal(x, y) for x, y in zip(crops[0], crops[1]))
