"""hv_rank_filter (csrc/rankfilt.hip) and healthivert-gan_amd/rank_filters.py against tests/rank_ref.py (pinned against scipy by
tests/test_rank_filters_ref_cpu.py): by value and dtype, and by bytes wherever the input holds neither NaN nor a -0.0 beside a +0.0.  Inputs come
C-ordered, Fortran-ordered, as a permuted view and as a sub-box of a NaN-filled (for integers: sentinel-filled) parent; the calls through the C
ABI write between guard words into an output whose strides are never the input's.  Extents are built from the tile the library reports
(hv_rank_tile) and never exceed a few tiles."""
import ctypes

import numpy as np
import pytest
import torch

import rank_ref as RR
from hvtest import Guarded

pytestmark = pytest.mark.gpu

_DT = {torch.uint8: 0, torch.int16: 1, torch.float32: 4, torch.float64: 5}
MODE = {m: i for i, m in enumerate(RR.MODES)}
ERR_ARG, ERR_UNSUPPORTED = -1, -2
LAYOUTS = ('c', 'f', 'perm', 'box')


def _lib():
    import hvgan  # noqa: F401
    from hvgan import lib
    return lib, lib.get()


def _RF():
    import hvgan  # noqa: F401
    from hvgan import rank_filters
    return rank_filters


def _tile():
    _, L = _lib()
    dims = (ctypes.c_int * 3)()
    assert L.cdll.hv_rank_tile(dims) == 0
    return tuple(dims)


def _ll(st):
    return [ctypes.c_longlong(s) for s in st]


def _layout(a, how, fill=None):
    """The numpy array `a` on the device with the same logical content, laid out as `how` says; box: inside a parent filled with `fill` bytes
    (None: NaN, for integers a sentinel)."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if how == 'c':
        return t.cuda()
    if how == 'f':                                            # Fortran order: axis 0 has unit stride
        return t.permute(2, 1, 0).contiguous().cuda().permute(2, 1, 0)
    if how == 'perm':                                         # stored as [A1][A2][A0]
        return t.permute(1, 2, 0).contiguous().cuda().permute(2, 0, 1)
    pad = (2, 3, 1)
    shape = tuple(n + 2 * p for n, p in zip(t.shape, pad))
    if fill is None:
        big = torch.full(shape, float('nan') if t.dtype.is_floating_point else (0xA5 if t.dtype == torch.uint8 else -23131), dtype=t.dtype)
    else:
        big = torch.full((int(np.prod(shape)) * t.element_size(),), fill, dtype=torch.uint8).view(t.dtype).view(shape)
    big[pad[0]:pad[0] + t.shape[0], pad[1]:pad[1] + t.shape[1], pad[2]:pad[2] + t.shape[2]] = t
    return big.cuda()[pad[0]:pad[0] + t.shape[0], pad[1]:pad[1] + t.shape[1], pad[2]:pad[2] + t.shape[2]]


def _footprint(offsets, n=None, extra_bits=()):
    _, L = _lib()
    fp = L.hv_rank_footprint()
    words = [0] * 12
    for o in np.asarray(offsets).reshape(-1, 3).tolist():
        b = ((o[0] + 4) * 9 + (o[1] + 4)) * 9 + (o[2] + 4)
        words[b // 64] |= 1 << (b % 64)
    for b in extra_bits:
        words[b // 64] |= 1 << (b % 64)
    for i, w in enumerate(words):
        fp.bits[i] = w
    fp.n = len(np.asarray(offsets).reshape(-1, 3)) if n is None else n
    return fp


def _call(src, offsets, rank, mode='reflect', cval=0.0, out=None, fp=None, dtype=None, A=None, src_ptr=None, out_ptr=None, fp_ptr=True):
    """One hv_rank_filter on the device tensor `src` -> (return code, the guarded output).  The output's strides are those of a [A2][A0][A1]
    array: never the input's."""
    lib, L = _lib()
    shape = tuple(int(s) for s in src.shape)
    g = Guarded((shape[2], shape[0], shape[1]), src.dtype) if out is None else out
    o = g.t.permute(1, 2, 0)
    fp = _footprint(offsets) if fp is None else fp
    rc = L.cdll.hv_rank_filter(lib.ptr(src) if src_ptr is None else src_ptr, _DT[src.dtype] if dtype is None else dtype, *_ll(src.stride()),
                               *(shape if A is None else A), ctypes.byref(fp) if fp_ptr else None, int(rank), MODE.get(mode, mode),
                               ctypes.c_double(float(cval)), lib.ptr(o) if out_ptr is None else out_ptr, *_ll(o.stride()), lib.stream())
    torch.cuda.synchronize()
    assert g.intact(), 'wrote outside the output'
    return rc, g


def _result(g):
    return g.t.permute(1, 2, 0).cpu().numpy()


def _check(a, how, offsets, rank, mode='reflect', cval=0, by_value=False, what=None):
    rc, g = _call(_layout(a, how), offsets, rank, mode, cval)
    assert rc == 0, (what, rc)
    got, want = _result(g), RR.rank_filter(a, offsets, rank, mode, cval)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if by_value:
        assert np.array_equal(got, want), (what, int((got != want).sum()))
    else:
        assert RR.same_bytes(got, want), (what, int((got != want).sum()))


def _ranks(n):
    return sorted({r for r in (0, 1, n // 2, n - 2, n - 1) if 0 <= r < n})


BOX3 = RR.box_offsets((3, 3, 3))


# ------------------------------------------------------------------------------------------------ tile edges
@pytest.mark.parametrize('mode', RR.MODES)
def test_tile_edges(mode):
    T = _tile()
    assert all(2 <= t <= 64 for t in T)
    k = 0
    for axis in range(3):
        for extent in (T[axis] - 1, T[axis], T[axis] + 1, 1):     # 1: an extent below the footprint's reach
            shape = [3, 5, 4]
            shape[axis] = extent
            a = RR.volume(tuple(shape), np.int16, seed=extent)
            _check(a, LAYOUTS[k % 4], BOX3, 13, mode, RR.CVAL, what=(axis, extent))
            k += 1
    a = RR.volume((T[0] + 1, 2 * T[1] + 3, T[2] + 2), np.int16)   # several workgroups along every axis at once
    for how in ('c', 'perm'):
        _check(a, how, BOX3, 13, mode, RR.CVAL, what=how)
    a = RR.volume((1, 1, 1), np.float32)
    _check(a, 'c', RR.box_offsets((9, 9, 9)), 364, mode, RR.CVAL, what='one voxel')


# ------------------------------------------------------------------------------------------------ footprints and ranks
def _footprints():
    corners = [(a, b, c) for a in (-4, 4) for b in (-4, 4) for c in (-4, 4)]
    lines = []
    for ax in range(3):
        shape = [1, 1, 1]
        shape[ax] = 9
        lines.append(('line%d' % ax, RR.box_offsets(tuple(shape))))
    return [('shift', np.array([(-4, 3, 1)])), ('corners', np.array(corners))] + lines + [('ball', _RF().ball(1.5, (0.7, 0.7, 1.5)))]


@pytest.mark.parametrize('dtype', (np.int16, np.float32), ids=lambda d: np.dtype(d).name)
def test_footprints_and_ranks(dtype):
    T = _tile()
    a = RR.volume((T[0] + 1, T[1] - 1, T[2] + 2), dtype)
    k = 0
    for name, off in _footprints():
        for rank in _ranks(len(off)):
            _check(a, LAYOUTS[k % 4], off, rank, RR.MODES[k % 5], RR.CVAL, what=(name, rank))
            k += 1
    shift = RR.rank_filter(a, [(-4, 3, 1)], 0, 'wrap')            # a single cell is a pure shift: out[p] = a[p + o]
    assert np.array_equal(shift, np.roll(a, (4, -3, -1), axis=(0, 1, 2)))


def test_full_box_on_one_tile():
    T = _tile()
    a = RR.volume((T[0] - 2, T[1] - 1, T[2]), np.uint8)
    off = RR.box_offsets((9, 9, 9))
    assert len(off) == 729
    for k, rank in enumerate(_ranks(729)):
        _check(a, LAYOUTS[k % 4], off, rank, RR.MODES[k % 5], RR.CVAL, what=rank)
    _check(RR.volume((3, 4, 5), np.float64), 'f', off, 364, 'mirror', what='float64')


def test_even_footprint_with_origin_through_python():
    RF = _RF()
    a = RR.volume((9, 7, 10), np.float32)
    off = RF.footprint_offsets(size=(2, 3, 4), origin=(-1, 1, -2))
    for rank in (0, 5, -3, -1):
        got = RF.rank_filter(_layout(a, 'perm'), rank, size=(2, 3, 4), mode='mirror', origin=(-1, 1, -2))
        assert got.is_cuda and got.dtype == torch.float32
        assert RR.same_bytes(got.cpu().numpy(), RR.rank_filter(a, off, rank, 'mirror')), rank
    fp = np.random.RandomState(2).rand(2, 3, 4) < 0.6
    got = RF.rank_filter(_layout(a, 'c'), 3, footprint=fp, origin=(0, -1, 1))
    assert RR.same_bytes(got.cpu().numpy(), RR.rank_filter(a, RF.footprint_offsets(footprint=fp, origin=(0, -1, 1)), 3))


# ------------------------------------------------------------------------------------------------ ties and keys
def test_ties_and_integer_extremes():
    T = _tile()
    shape = (T[0] + 1, 5, T[2] + 1)
    r = np.random.RandomState(1)
    vols = [np.full(shape, 9, dtype=np.uint8), (r.rand(*shape) < 0.5).astype(np.uint8) * 200,
            np.full(shape, -5, dtype=np.int16), r.choice(np.array([-32768, 32767, 0, -1], dtype=np.int16), shape)]
    for a in vols:
        for rank in _ranks(27):
            _check(a, 'c', BOX3, rank, 'reflect', what=(a.dtype, rank))
    _check(vols[3], 'box', BOX3, 13, 'constant', -32768, what='cval at the bottom')
    _check(vols[3], 'box', BOX3, 13, 'constant', 32767, what='cval at the top')
    _check(vols[1], 'f', BOX3, 13, 'constant', 255, what='uint8 cval 255')


@pytest.mark.parametrize('dtype', (np.float32, np.float64), ids=lambda d: np.dtype(d).name)
def test_float_keys(dtype):
    T = _tile()
    shape = (T[0] + 1, 5, T[2] + 1)
    r = np.random.RandomState(2)
    fi = np.finfo(dtype)
    one = dtype(1.0)
    pool = np.array([np.inf, -np.inf, fi.smallest_subnormal, -fi.smallest_subnormal, fi.tiny / 2, one, np.nextafter(one, dtype(2.0)),
                     np.nextafter(one, dtype(0.0)), -1e30, 1e-30, -3.5, fi.max, -fi.max], dtype=dtype)
    a = r.choice(pool, shape)
    for rank in _ranks(27):
        for how in ('c', 'box'):
            _check(a, how, BOX3, rank, 'nearest', what=(rank, how))
    z = r.choice(np.array([0.0, -0.0, 1.0, -1.0], dtype=dtype), shape)          # -0.0 beside +0.0: compared by value
    for rank in _ranks(27):
        _check(z, 'c', BOX3, rank, 'reflect', by_value=True, what=('zeros', rank))
    # the key order: -0.0 sorts just below +0.0
    z = np.zeros((5, 5, 5), dtype=dtype)
    z[2, 2, 2] = -0.0
    near = np.zeros((5, 5, 5), dtype=bool)
    near[1:4, 1:4, 1:4] = True
    for rank, want in ((0, near), (26, np.zeros_like(near))):
        rc, g = _call(_layout(z, 'c'), BOX3, rank, 'constant', 0.0)
        assert rc == 0 and np.array_equal(np.signbit(_result(g)), want), rank


@pytest.mark.parametrize('dtype', (np.float32, np.float64), ids=lambda d: np.dtype(d).name)
def test_windows_without_nan_are_exact(dtype):
    T = _tile()
    a = RR.volume((T[0] + 2, T[1] + 1, T[2] + 3), dtype)
    r = np.random.RandomState(3)
    hit = r.rand(*a.shape) < 0.02
    a[hit] = np.where(r.rand(int(hit.sum())) < 0.5, np.nan, -np.nan).astype(dtype)
    for mode in ('reflect', 'constant'):
        clean = ~np.isnan(RR.windows(a, BOX3, mode, RR.CVAL)).any(axis=-1)
        assert 0.2 < clean.mean() < 0.9
        for rank in (0, 13, 26):
            rc, g = _call(_layout(a, 'box'), BOX3, rank, mode, RR.CVAL)
            got, want = _result(g), RR.rank_filter(a, BOX3, rank, mode, RR.CVAL)
            assert rc == 0 and got[clean].tobytes() == want[clean].tobytes(), (mode, rank)


# ------------------------------------------------------------------------------------------------ constant mode
@pytest.mark.parametrize('dtype', RR.DTYPES, ids=lambda d: np.dtype(d).name)
def test_constant_mode_cval(dtype):
    a = RR.volume((6, 9, 7), dtype)
    lo, hi = float(a.min()), float(a.max())
    inside = float(a[3, 4, 2])
    below = 0 if dtype == np.uint8 and lo == 0 else lo - 1
    for cval in (float(dtype(below)), inside, float(dtype(hi + 3))):      # (rounded to the dtype: cval must be one of its values)
        for rank in (0, 9, 13, 26):
            _check(a, 'perm', BOX3, rank, 'constant', cval, what=(cval, rank))
        _check(a, 'c', RR.box_offsets((1, 1, 9)), 4, 'constant', cval, what=(cval, 'line'))


# ------------------------------------------------------------------------------------------------ dtypes x layouts
@pytest.mark.parametrize('how', LAYOUTS)
@pytest.mark.parametrize('dtype', RR.DTYPES, ids=lambda d: np.dtype(d).name)
def test_dtypes_and_layouts(dtype, how):
    T = _tile()
    a = RR.volume((T[0] + 3, 6, 2 * T[2] + 1), dtype)
    d = _layout(a, how)
    assert how == 'c' or not d.is_contiguous()
    _check(a, how, BOX3, 13, 'mirror', what='median')
    _check(a, how, BOX3, 0, 'wrap', what='minimum')


# ------------------------------------------------------------------------------------------------ the Python entries
def test_median_percentile_and_separable_minimum():
    RF = _RF()
    a = RR.volume((10, 9, 12), np.int16)
    d = _layout(a, 'f')
    got = RF.median_filter(d, size=3)
    assert got.dtype == torch.int16 and RR.same_bytes(got.cpu().numpy(), RR.rank_filter(a, BOX3, 13))
    fp = np.random.RandomState(5).rand(3, 5, 3) < 0.5
    off = RF.footprint_offsets(footprint=fp)
    assert RR.same_bytes(RF.median_filter(d, footprint=fp, mode='wrap').cpu().numpy(), RR.rank_filter(a, off, len(off) // 2, 'wrap'))
    for p in (-20, 0, 35, 50, 100):
        got = RF.percentile_filter(d, p, footprint=fp, mode='constant', cval=RR.CVAL)
        assert RR.same_bytes(got.cpu().numpy(), RR.rank_filter(a, off, RF.percentile_rank(len(off), p), 'constant', RR.CVAL)), p
    box = RF.footprint_offsets(size=(3, 2, 5))
    for mode in RR.MODES:                                         # one launch per axis against the 3-D footprint call and the restatement
        for fn, rank in ((RF.minimum_filter, 0), (RF.maximum_filter, -1)):
            sep = fn(d, size=(3, 2, 5), mode=mode, cval=RR.CVAL)
            full = fn(d, footprint=np.ones((3, 2, 5), dtype=bool), mode=mode, cval=RR.CVAL)
            assert torch.equal(sep, full) and RR.same_bytes(sep.cpu().numpy(), RR.rank_filter(a, box, rank, mode, RR.CVAL)), (mode, rank)
    out = torch.empty(a.shape, dtype=torch.int16, device='cuda')
    assert RF.minimum_filter(d, size=3, out=out) is out and RR.same_bytes(out.cpu().numpy(), RR.rank_filter(a, BOX3, 0))
    assert RR.same_bytes(RF.minimum_filter(d, size=1).cpu().numpy(), a)
    # numpy arrays are uploaded, bool becomes uint8, other dtypes and a shared output are refused
    assert RR.same_bytes(RF.median_filter(a, size=3).cpu().numpy(), RR.rank_filter(a, BOX3, 13))
    b = a > 0
    got = RF.maximum_filter(b, size=(1, 1, 3))
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), RR.rank_filter(b.astype(np.uint8), RR.box_offsets((1, 1, 3)), -1))
    with pytest.raises(TypeError):
        RF.median_filter(a.astype(np.int32), size=3)
    with pytest.raises(ValueError):
        RF.median_filter(d, size=3, out=d)
    with pytest.raises(ValueError):
        RF.median_filter(d, size=3, mode='constant', cval=0.5)
    with pytest.raises(ValueError):
        RF.median_filter(d, size=3, mode='grid-wrap')
    with pytest.raises(ValueError):
        RF.median_filter(d[0], size=3)


def test_grey_morphology():
    RF = _RF()
    a = RR.volume((9, 10, 11), np.float64)
    d = _layout(a, 'perm')
    even = np.random.RandomState(4).rand(2, 4, 3) < 0.7
    for kw in (dict(size=(3, 3, 3)), dict(size=(2, 3, 4), origin=(-1, 1, -2)), dict(footprint=even, origin=(0, -2, 1))):
        ero = RF.footprint_offsets(kw.get('size'), kw.get('footprint'), kw.get('origin', 0))
        dil = RF.footprint_offsets(kw.get('size'), *RF.dilation_arguments(kw.get('size'), kw.get('footprint'), kw.get('origin', 0)))
        for mode in ('reflect', 'constant'):
            e = RR.rank_filter(a, ero, 0, mode, RR.CVAL)
            m = RR.rank_filter(a, dil, -1, mode, RR.CVAL)
            args = dict(kw, mode=mode, cval=RR.CVAL)
            assert RR.same_bytes(RF.grey_erosion(d, **args).cpu().numpy(), e), (kw, mode)
            assert RR.same_bytes(RF.grey_dilation(d, **args).cpu().numpy(), m), (kw, mode)
            assert RR.same_bytes(RF.grey_opening(d, **args).cpu().numpy(), RR.rank_filter(e, dil, -1, mode, RR.CVAL)), (kw, mode)
            assert RR.same_bytes(RF.grey_closing(d, **args).cpu().numpy(), RR.rank_filter(m, ero, 0, mode, RR.CVAL)), (kw, mode)
    with pytest.raises(ValueError):
        RF.grey_erosion(d)


def test_median_ct_and_deflicker():
    RF = _RF()
    a = RR.volume((12, 11, 10), np.int16)
    a[:, :, 4] += 500                                             # one slice that flickers
    d = _layout(a, 'c')
    sp = (0.7, 0.7, 1.5)
    off = RF.ball(1.5, sp)
    assert RR.same_bytes(RF.median_ct(d, radius_mm=1.5, spacing=sp).cpu().numpy(), RR.rank_filter(a, off, len(off) // 2, 'nearest'))
    assert RR.same_bytes(RF.median_ct(d, radius_mm=1.0).cpu().numpy(), RR.rank_filter(a, RF.ball(1.0), 7 // 2, 'nearest'))
    assert RR.same_bytes(RF.median_ct(d, size=3, mode='reflect').cpu().numpy(), RR.rank_filter(a, BOX3, 13))
    for axis in (2, 0, -2):
        shape = [1, 1, 1]
        shape[axis] = 3
        want = RR.rank_filter(a, RR.box_offsets(tuple(shape)), 1, 'nearest')
        assert RR.same_bytes(RF.deflicker(d, axis=axis).cpu().numpy(), want), axis
    assert abs(int(RF.deflicker(d)[5, 5, 4]) - int(a[5, 5, 4])) > 150
    with pytest.raises(ValueError):
        RF.median_ct(d)
    with pytest.raises(ValueError):
        RF.median_ct(d, radius_mm=1.0, size=3)


def test_vertebra_density_median_size():
    RF = _RF()
    from hvgan import label_statistics as LS
    r = np.random.RandomState(7)
    ct = r.randint(-200, 900, (20, 18, 14)).astype(np.int16)
    label = np.zeros(ct.shape, dtype=np.uint8)
    label[4:16, 3:15, 2:12] = 20
    d, dl = _layout(ct, 'c'), _layout(label, 'c')

    def same(x, y):
        assert x.keys() == y.keys()

        def eq(u, v):
            u, v = np.asarray(u), np.asarray(v)
            return np.array_equal(u, v, equal_nan=True) if u.dtype.kind == 'f' and v.dtype.kind == 'f' else np.array_equal(u, v)
        return all(eq(x[k], y[k]) for k in x)
    plain = LS.vertebra_density(d, dl, 20, erode_mm=1.0, spacing=(0.7, 0.7, 1.5))
    assert same(plain, LS.vertebra_density(d, dl, 20, erode_mm=1.0, spacing=(0.7, 0.7, 1.5), median_size=None))
    host = torch.from_numpy(RR.rank_filter(ct, BOX3, 13)).cuda()                # the host chain: the median, then the same statistics
    want = LS.vertebra_density(host, dl, 20, erode_mm=1.0, spacing=(0.7, 0.7, 1.5))
    got = LS.vertebra_density(d, dl, 20, erode_mm=1.0, spacing=(0.7, 0.7, 1.5), median_size=3)
    assert same(got, want) and not same(got, plain)
    assert torch.equal(d.cpu(), torch.from_numpy(ct))


# ------------------------------------------------------------------------------------------------ refusals, determinism, ABI
def test_refusals_write_nothing():
    lib, L = _lib()
    a = RR.volume((6, 7, 8), np.int16)
    d = _layout(a, 'c')
    f32 = _layout(a.astype(np.float32), 'c')
    g16, g32 = Guarded((8, 6, 7), torch.int16), Guarded((8, 6, 7), torch.float32)
    before16, before32 = g16.big.view(torch.uint8).clone(), g32.big.view(torch.uint8).clone()
    null = ctypes.c_void_p(0)
    cases = [
        (dict(src_ptr=null), ERR_ARG), (dict(out_ptr=null), ERR_ARG), (dict(fp_ptr=False), ERR_ARG),
        (dict(A=(6, 0, 8)), ERR_ARG), (dict(A=(-1, 7, 8)), ERR_ARG), (dict(A=(1 << 11, 1 << 10, (1 << 9) + 1)), ERR_UNSUPPORTED),
        (dict(dtype=2), ERR_ARG), (dict(dtype=3), ERR_ARG), (dict(dtype=9), ERR_ARG), (dict(mode=5), ERR_ARG), (dict(mode=-1), ERR_ARG),
        (dict(fp=_footprint(np.zeros((0, 3)), n=0)), ERR_ARG), (dict(fp=_footprint(BOX3, n=26)), ERR_ARG), (dict(fp=_footprint(BOX3, n=28)), ERR_ARG),
        (dict(fp=_footprint(BOX3, n=28, extra_bits=(729,))), ERR_ARG), (dict(fp=_footprint(BOX3, n=28, extra_bits=(767,))), ERR_ARG),
        (dict(rank=-1), ERR_ARG), (dict(rank=27), ERR_ARG),
        (dict(cval=np.inf), ERR_ARG), (dict(cval=np.nan), ERR_ARG), (dict(cval=0.5), ERR_ARG), (dict(cval=40000.0), ERR_ARG),
    ]
    for kw, code in cases:
        args = dict(offsets=BOX3, rank=13, mode='constant', cval=0.0, out=g16)
        args.update(kw)
        rc, _ = _call(d, args.pop('offsets'), args.pop('rank'), **args)
        assert rc == code, (kw, rc)
    for cval in (0.1, 1e39, np.inf):                              # 0.1 is no float32
        rc, _ = _call(f32, BOX3, 13, 'constant', cval, out=g32)
        assert rc == ERR_ARG, cval
    # out intersecting the bytes vol spans: the volume itself, and a shifted view of its buffer
    assert _call(d, BOX3, 13, out=g16, out_ptr=lib.ptr(d))[0] == ERR_ARG
    assert _call(d, BOX3, 13, out=g16, out_ptr=ctypes.c_void_p(d.data_ptr() + 2 * 300))[0] == ERR_ARG
    assert L.cdll.hv_rank_tile(None) == ERR_ARG
    torch.cuda.synchronize()
    assert torch.equal(g16.big.view(torch.uint8), before16) and torch.equal(g32.big.view(torch.uint8), before32)
    assert torch.equal(d.cpu(), torch.from_numpy(a))
    # the accepted calls: bit 728 is the last legal one, 0.5 and 0.0 are values of float32
    rc, g = _call(d, [(4, 4, 4)], 0, 'wrap', out=g16)
    assert rc == 0 and np.array_equal(_result(g), np.roll(a, (-4, -4, -4), axis=(0, 1, 2)))
    rc, g = _call(f32, BOX3, 13, 'constant', 0.5, out=g32)
    assert rc == 0 and RR.same_bytes(_result(g), RR.rank_filter(a.astype(np.float32), BOX3, 13, 'constant', 0.5))


def test_determinism_and_parent_content():
    T = _tile()
    a = RR.volume((T[0] + 2, T[1] + 1, T[2] + 3), np.float32)
    off = _RF().ball(1.5, (0.7, 0.7, 1.5))
    raws = []
    for fill in (None, None, 0x5A):                               # twice in a NaN-filled parent, once in a 0x5A-filled one
        rc, g = _call(_layout(a, 'box', fill), off, len(off) // 2, 'mirror')
        assert rc == 0
        raws.append(g.big.view(torch.uint8).clone())
    assert torch.equal(raws[0], raws[1]) and torch.equal(raws[0], raws[2])
    assert RR.same_bytes(_result(g), RR.rank_filter(a, off, len(off) // 2, 'mirror'))


def test_abi():
    _, L = _lib()
    for name in ('hv_rank_filter', 'hv_rank_tile'):
        assert name in L.protos and getattr(L.cdll, name) is not None
    assert ctypes.sizeof(L.hv_rank_footprint) == 104
    assert _RF().REACH == 4 and all(t >= 2 for t in _tile())
