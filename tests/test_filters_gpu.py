"""hv_separable_filter / hv_blend_lerp (csrc/filter3d.hip) and healthivert-gan_amd/filters.py against tests/filter_ref.py (pinned against scipy
bit for bit by tests/test_filters_ref_cpu.py): every comparison is bit for bit on finite values, with NaN exactly where the reference has NaN.
Inputs come C-ordered, Fortran-ordered, as a permuted view and as a sub-box of a NaN-filled (for integers: sentinel-filled) parent; the calls
through the C ABI write between guard words and get exactly the queried workspace inside a border.  Extents are built from the tile the library
reports (hv_filter_tile)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import ccl_ref as CR
import filter_ref as FR
import morph_ref as MR
from hvtest import Guarded

pytestmark = pytest.mark.gpu

_DT = {torch.uint8: 0, torch.int16: 1, torch.float32: 4, torch.float64: 5}
F64, U8 = 5, 0
IN_VALUE, IN_EQ = 0, 1
MODE = {m: i for i, m in enumerate(FR.MODES)}
ERR_ARG, ERR_UNSUPPORTED = -1, -2
MAX_RADIUS = 64
LAYOUTS = ('c', 'f', 'perm', 'box')


def _lib():
    import hvgan  # noqa: F401
    from hvgan import lib
    return lib, lib.get()


def _F():
    import hvgan  # noqa: F401
    from hvgan import filters
    return filters


def _tile():
    _, L = _lib()
    dims = (ctypes.c_int * 3)()
    assert L.cdll.hv_filter_tile(dims) == 0
    return tuple(dims)


def _ll(st):
    return [ctypes.c_longlong(s) for s in st]


def _layout(a, how):
    """The numpy array `a` on the device with the same logical content, laid out as `how` says."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if how == 'c':
        return t.cuda()
    if how == 'f':                                            # Fortran order: axis 0 has unit stride
        return t.permute(2, 1, 0).contiguous().cuda().permute(2, 1, 0)
    if how == 'perm':                                         # stored as [A1][A2][A0]
        return t.permute(1, 2, 0).contiguous().cuda().permute(2, 0, 1)
    pad = (2, 3, 1)
    fill = float('nan') if t.dtype.is_floating_point else (0xA5 if t.dtype == torch.uint8 else -23131)
    big = torch.full(tuple(n + 2 * p for n, p in zip(t.shape, pad)), fill, dtype=t.dtype)
    big[pad[0]:pad[0] + t.shape[0], pad[1]:pad[1] + t.shape[1], pad[2]:pad[2] + t.shape[2]] = t
    return big.cuda()[pad[0]:pad[0] + t.shape[0], pad[1]:pad[1] + t.shape[1], pad[2]:pad[2] + t.shape[2]]


def _same(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape)
    ok = FR.same(got, want)
    assert ok, (what, int((~((got == want) | (np.isnan(got) & np.isnan(want)))).sum()))


class _Ws:
    """Exactly `need` bytes, 16-byte aligned (+ off), filled with `fill` bytes like the border around them."""

    def __init__(self, need, fill=0xFF, off=0):
        self.need, self.fill, self.off = need, fill, off
        self.big = torch.full((512 + need + off,), fill, dtype=torch.uint8, device='cuda')
        assert self.big[256:].data_ptr() % 16 == 0
        self.ptr = ctypes.c_void_p(self.big[256:].data_ptr() + off)

    def border_intact(self):
        lo, hi = self.big[:256 + self.off], self.big[256 + self.off + self.need:]
        return bool((lo == self.fill).all()) and bool((hi == self.fill).all())

    def untouched(self):
        return bool((self.big == self.fill).all())


def _axes(weights):
    """(ctypes array of three hv_filter_axis, kept alive by the caller) from three weight arrays or None; a tuple (radius, form, w) passes raw."""
    _, L = _lib()
    desc = (L.hv_filter_axis * 3)()
    for a, w in enumerate(weights):
        if w is None:
            desc[a].radius = -1
            continue
        if isinstance(w, tuple):
            desc[a].radius, desc[a].form = w[0], w[1]
            w = w[2]
        else:
            desc[a].radius, desc[a].form = len(w) // 2, FR.detect_form(w)
        for i, x in enumerate(w):
            desc[a].w[i] = float(x)
    return desc


def _need(A, desc):
    return _lib()[1].size('hv_filter_workspace_bytes', *A, desc)


def _call(src, weights, mode='reflect', cval=0.0, in_mode=IN_VALUE, value=0.0, out_dtype=F64, threshold=0.5, ws=None, ws_bytes=None,
          out=None, dtype=None, A=None, src_ptr=None):
    """One hv_separable_filter on the device tensor `src` -> (return code, the guarded output, the workspace).  The output's strides are
    those of a [A2][A0][A1] array: never the input's."""
    lib, L = _lib()
    A = tuple(int(s) for s in src.shape) if A is None else A
    desc = weights if isinstance(weights, ctypes.Array) else _axes(weights)
    shape = tuple(int(s) for s in src.shape)
    g = Guarded((shape[2], shape[0], shape[1]), torch.float64 if out_dtype != U8 else torch.uint8) if out is None else out
    o = g.t.permute(1, 2, 0)
    ws = ws or _Ws(max(_need(shape, desc), 16))
    rc = L.cdll.hv_separable_filter(lib.ptr(src) if src_ptr is None else src_ptr, _DT[src.dtype] if dtype is None else dtype, *_ll(src.stride()),
                                    *A, in_mode, ctypes.c_double(float(value)), desc, MODE.get(mode, mode), ctypes.c_double(float(cval)),
                                    lib.ptr(o), out_dtype, ctypes.c_double(float(threshold)), *_ll(o.stride()), ws.ptr,
                                    ctypes.c_size_t(ws.need if ws_bytes is None else ws_bytes), lib.stream())
    torch.cuda.synchronize()
    assert g.intact() and ws.border_intact(), 'wrote outside a buffer'
    return rc, g, ws


def _result(g):
    return g.t.permute(1, 2, 0).cpu().numpy()


# ------------------------------------------------------------------------------------------------ the grid of the restatement
@functools.lru_cache(maxsize=None)
def _grid_ref(shape, dtype, mode, case):
    sigma, order = FR.SIGMA_ORDER[case]
    return FR.gaussian_filter(FR.volume(shape, dtype), sigma, order=order, mode=mode, cval=FR.CVAL)


@pytest.mark.parametrize('dtype', FR.DTYPES, ids=lambda d: np.dtype(d).name)
def test_full_grid(dtype):
    F = _F()
    for shape in FR.SHAPES:
        a = FR.volume(shape, dtype)
        for how in LAYOUTS:
            d = _layout(a, how)
            assert how == 'c' or not d.is_contiguous() or 1 in shape
            for mode in FR.MODES:
                for case, (sigma, order) in enumerate(FR.SIGMA_ORDER):
                    got = F.gaussian_filter(d, sigma, order=order, mode=mode, cval=FR.CVAL)
                    assert got.dtype == torch.float64 and got.is_cuda
                    _same(got, _grid_ref(shape, dtype, mode, case), (shape, how, mode, sigma, order))


# ------------------------------------------------------------------------------------------------ tile edges
def _weights(radius, form, seed):
    r = np.random.RandomState(seed)
    h = r.randn(radius) if radius else np.zeros(0)
    c = r.randn(1)
    if form > 0:
        return np.r_[h, c, h[::-1]]
    if form < 0:
        return np.r_[h, [0.0], -h[::-1]]
    return r.randn(2 * radius + 1)


@pytest.mark.parametrize('axis', (0, 1, 2))
def test_tile_edges(axis):
    F = _F()
    T = _tile()[axis]
    assert 1 <= T <= MAX_RADIUS
    n = 0
    for extent in (T - 1, T, T + 1, 2 * T + 3):
        shape = [5, 9, 7]
        shape[axis] = extent
        a = FR.volume(tuple(shape), np.float64, seed=extent)
        for radius in sorted({1, T, MAX_RADIUS}):
            for how in ('c', 'f'):                            # the filtered axis across the lanes, and along them
                form, mode = (1, -1, 0)[n % 3], FR.MODES[n % 5]
                n += 1
                w = _weights(radius, form, n)
                assert FR.detect_form(w) == form
                got = F.correlate1d(_layout(a, how), w, axis, mode, FR.CVAL)
                _same(got, FR.correlate1d(a, w, axis, mode, FR.CVAL), (axis, extent, radius, how, form, mode))


@pytest.mark.parametrize('how', ('c', 'f', 'perm'))
def test_several_workgroups_per_axis(how):
    """More than one column tile, more than one group of lines and more than one tile along the filtered axis at once."""
    F = _F()
    T = max(_tile())
    shape = (T + 5, 40, 70)
    a = FR.volume(shape, np.float32)
    got = F.gaussian_filter(_layout(a, how), (1.0, 2.0, 0.8), order=(0, 1, 0), mode='mirror')
    _same(got, FR.gaussian_filter(a, (1.0, 2.0, 0.8), order=(0, 1, 0), mode='mirror'), how)


# ------------------------------------------------------------------------------------------------ degenerate extents, skipped axes, orders
@pytest.mark.parametrize('mode', FR.MODES)
def test_degenerate_extents_and_radius_beyond_the_extent(mode):
    F = _F()
    wide = np.linspace(-1.0, 2.0, 17)                         # general, radius 8
    for shape in ((1, 6, 5), (6, 1, 5), (6, 5, 1), (1, 1, 1), (2, 1, 3)):
        a = FR.volume(shape, np.float64)
        for how in ('c', 'f'):
            d = _layout(a, how)
            _same(F.gaussian_filter(d, 1.5, mode=mode, cval=FR.CVAL), FR.gaussian_filter(a, 1.5, mode=mode, cval=FR.CVAL), (shape, how))
            for axis in range(3):
                _same(F.correlate1d(d, wide, axis, mode, FR.CVAL), FR.correlate1d(a, wide, axis, mode, FR.CVAL), (shape, how, axis))


@pytest.mark.parametrize('dtype', FR.DTYPES, ids=lambda d: np.dtype(d).name)
def test_skipped_axes(dtype):
    F = _F()
    a = FR.volume((7, 6, 10), dtype)
    for how in LAYOUTS:
        d = _layout(a, how)
        for sigma in ((0, 0, 1.3), (1.3, 0, 0), (0, 0.9, 0)):
            _same(F.gaussian_filter(d, sigma), FR.gaussian_filter(a, sigma), (how, sigma))
        got = F.gaussian_filter(d, 0)                         # all three skipped: the float64 copy
        _same(got, a.astype(np.float64), how)
        _same(F.gaussian_filter(d, (2.0, 2.0, 2.0), spacing=(0.7, 0.7, 1.5)), FR.gaussian_filter(a, 2.0, spacing=(0.7, 0.7, 1.5)), how)


def test_derivative_orders_and_general_weights():
    F = _F()
    a = FR.volume((9, 8, 11), np.float64)
    d = _layout(a, 'c')
    for order in ((1, 0, 0), (0, 2, 0), (0, 0, 1), (2, 1, 3)):
        _same(F.gaussian_filter(d, 1.2, order=order, mode='nearest'), FR.gaussian_filter(a, 1.2, order=order, mode='nearest'), order)
    for axis in range(3):
        _same(F.correlate1d(d, FR.GENERAL_W, axis), FR.correlate1d(a, FR.GENERAL_W, axis), axis)
        _same(F.gaussian_filter1d(d, 1.4, axis, order=1, mode='wrap'), FR.gaussian_filter1d(a, 1.4, axis, 1, 'wrap'), axis)
    ulp = np.array([0.1, 0.7, 0.25, 1.0, 0.25, 0.7, 0.1])
    ulp[5] = np.nextafter(ulp[5], 1.0)                        # scipy's symmetric form, although the halves differ
    assert F.weights_form(ulp) == 1 and F.weights_form(FR.GENERAL_W) == 0
    _same(F.correlate1d(d, ulp, 2), FR.correlate1d(a, ulp, 2), 'ulp')
    for w in FR.GENERAL_W, FR.GENERAL_W[::-1]:                # the order of the taps is the correlation's
        assert np.array_equal(F.correlate1d(d, w, 1).cpu().numpy(), FR.correlate1d(a, w, 1))
    with pytest.raises(ValueError):
        F.correlate1d(d, [1.0, 2.0], 0)
    with pytest.raises(ValueError):
        F.correlate1d(d, [1.0, 2.0, 1.0], 0, origin=1)
    with pytest.raises(ValueError):
        F.gaussian_filter(d, 20.0)                            # radius 80
    with pytest.raises(ValueError):
        F.gaussian_filter(d, 1.0, mode='grid-wrap')


# ------------------------------------------------------------------------------------------------ indicator input, threshold output
@pytest.mark.parametrize('dtype', (np.uint8, np.int16, np.float32))
def test_indicator_and_threshold(dtype):
    vol = FR.staircase().astype(dtype)
    for how in ('c', 'box'):
        d = _layout(vol, how)
        for sigma in ((1.0, 0.8, 1.3), (0, 1.0, 1.0), (0, 0, 1.5), (0, 0, 0)):
            weights = [None if s == 0 else FR.gaussian_kernel1d(s, 0, int(4.0 * s + 0.5))[::-1] for s in sigma]
            want = FR.gaussian_filter((vol == 20).astype(np.float64), sigma, mode='constant', cval=1.0)
            rc, g, _ = _call(d, weights, 'constant', 1.0, IN_EQ, 20.0)
            assert rc == 0
            _same(_result(g), want, (how, sigma))
            for thr in (0.5, 0.0, 1.0):
                rc, g, _ = _call(d, weights, 'constant', 1.0, IN_EQ, 20.0, out_dtype=U8, threshold=thr)
                assert rc == 0
                assert np.array_equal(_result(g), (want >= thr).astype(np.uint8)), (how, sigma, thr)


def test_smooth_label():
    F = _F()
    vol = FR.staircase()
    for sigma, spacing in ((1.0, None), (1.0, (0.7, 0.7, 1.5)), ((0.0, 0.0, 1.2), None)):
        want = FR.smooth_label(vol, 20, sigma, spacing, fill=3)
        assert (want != vol).any() and np.array_equal(want == 19, vol == 19)
        d = _layout(vol, 'perm')
        got = F.smooth_label(d, 20, sigma, spacing, fill=3)
        assert got.dtype == torch.uint8 and torch.equal(d.cpu(), torch.from_numpy(vol))
        assert np.array_equal(got.cpu().numpy(), want), (sigma, spacing)
        assert np.array_equal(got.cpu().numpy() == 19, vol == 19)              # the second label's voxels are untouched
        assert F.smooth_label(d, 20, sigma, spacing, fill=3, out=d) is d        # in place
        assert np.array_equal(d.cpu().numpy(), want)
        mask = F.smooth_mask(_layout(vol, 'f'), 20, sigma, spacing)
        assert np.array_equal(mask.cpu().numpy(), FR.smooth_mask(vol, 20, sigma, spacing).astype(np.uint8))
    f = vol.astype(np.float32)
    assert np.array_equal(F.smooth_label(_layout(f, 'c'), 20, 1.0, threshold=0.3).cpu().numpy(), FR.smooth_label(f, 20, 1.0, threshold=0.3))


# ------------------------------------------------------------------------------------------------ the composite
def test_blend_lerp_and_feather_blend():
    F = _F()
    lib, L = _lib()
    shape = (9, 12, 70)
    a16, b = FR.volume(shape, np.int16), FR.volume(shape, np.float64, 1)
    w = np.random.RandomState(5).rand(*shape)
    w[0, 0, :4] = (0.0, 1.0, 0.5, np.nextafter(1.0, 0.0))
    want = ((1.0 - w) * a16.astype(np.float64)) + (w * b)
    got = F.blend_lerp(_layout(a16, 'perm'), _layout(b, 'f'), _layout(w, 'box'))
    assert np.array_equal(got.cpu().numpy(), want)
    a64 = a16.astype(np.float64)                              # out is a
    g = Guarded(shape, torch.float64, data=torch.from_numpy(a64))
    assert F.blend_lerp(g.t, _layout(b, 'c'), _layout(w, 'c'), out=g.t) is g.t
    torch.cuda.synchronize()
    assert g.intact() and np.array_equal(g.t.cpu().numpy(), want)
    m = np.random.RandomState(6).rand(*shape) < 0.4           # a uint8 mask as the weight
    got = F.blend_lerp(_layout(a16, 'c'), _layout(b.astype(np.float32), 'c'), _layout(m.astype(np.uint8) * 7, 'f'))
    assert np.array_equal(got.cpu().numpy(), FR.blend_lerp(a16, b.astype(np.float32), m))
    label = FR.staircase()
    a16, b = FR.volume(label.shape, np.int16), FR.volume(label.shape, np.float64, 1)
    for spacing in (None, (0.7, 0.7, 1.5)):
        want = FR.feather_blend(a16, b, label, 1.5, spacing)
        assert np.array_equal(F.feather_blend(_layout(a16, 'f'), _layout(b, 'c'), _layout(label, 'perm'), 1.5, spacing).cpu().numpy(), want)
    want = FR.feather_blend(a16, b, label == 20, 1.5)
    assert np.array_equal(F.feather_blend(_layout(a16, 'c'), _layout(b, 'c'), _layout(label, 'c'), 1.5, value=20).cpu().numpy(), want)
    assert np.array_equal(F.feather_blend(_layout(a16, 'c'), _layout(b, 'c'), _layout(label == 20, 'c'), 1.5).cpu().numpy(), want)
    # refusals of the entry point: nothing is written
    A = tuple(label.shape)
    da, db, dw = _layout(a16, 'c'), _layout(b, 'c'), _layout(label == 20, 'c').to(torch.uint8)
    g = Guarded(A, torch.float64)
    before = g.big.view(torch.uint8).clone()

    def blend(pa=None, adt=1, wdt=0, dims=A, out=None):
        return L.cdll.hv_blend_lerp(lib.ptr(da) if pa is None else pa, adt, *_ll(da.stride()), lib.ptr(db), 5, *_ll(db.stride()), lib.ptr(dw), wdt,
                                    *_ll(dw.stride()), *dims, lib.ptr(g.t) if out is None else out, *_ll(g.t.stride()), lib.stream())
    assert blend(pa=ctypes.c_void_p(0)) == ERR_ARG and blend(adt=0) == ERR_ARG and blend(wdt=4) == ERR_ARG
    assert blend(dims=(A[0], 0, A[2])) == ERR_ARG and blend(out=lib.ptr(db)) == ERR_ARG
    assert blend(pa=lib.ptr(g.t)) == ERR_ARG                  # out is a, but a is not float64
    torch.cuda.synchronize()
    assert torch.equal(g.big.view(torch.uint8), before)
    assert blend() == 0
    torch.cuda.synchronize()
    assert g.intact() and np.array_equal(g.t.cpu().numpy(), FR.blend_lerp(a16, b, label == 20))


# ------------------------------------------------------------------------------------------------ clean_label(smooth_mm=...)
def test_clean_label_smooth_mm():
    import hvgan  # noqa: F401
    from hvgan import components as C
    from hvgan import morphology as M
    F = _F()
    vol = MR.two_fragment_body()
    vol[4:18, 4:18, 4:14:2][:, :2] = 0                        # a staircase on one face of the body
    sp = (0.7, 0.7, 1.5)
    d = _layout(vol, 'c')
    # without smooth_mm: the bytes of the calls that existed before
    assert np.array_equal(C.clean_label(d, 20).cpu().numpy(), CR.clean_label(vol, 20)[0])
    closed = M.close_label(d, 20, 1.6, sp)
    assert torch.equal(C.clean_label(d, 20, closing_mm=1.6, spacing=sp), C.clean_label(closed, 20))
    # with it: the composition of the public steps, after the closing and before the component rules
    for kw in ({}, {'closing_mm': 1.6}, {'closing_mm': 1.6, 'opening_mm': 0.7}):
        step = d
        if 'opening_mm' in kw:
            step = M.open_label(step, 20, kw['opening_mm'], sp, fill=7)
        if 'closing_mm' in kw:
            step = M.close_label(step, 20, kw['closing_mm'], sp, background=7, fill=7)
        step = F.smooth_label(step, 20, 1.0, spacing=sp, background=7, fill=7)
        want = C.clean_label(step, 20, min_size=3, fill=7, fill_holes=True)
        got, table = C.clean_label(d, 20, min_size=3, fill=7, fill_holes=True, smooth_mm=1.0, spacing=sp, return_table=True, **kw)
        assert torch.equal(got, want), kw
        assert torch.equal(d.cpu(), torch.from_numpy(vol))
    ref = CR.clean_label(FR.smooth_label(vol, 20, 1.0, sp, background=7, fill=7), 20, min_size=3, holes=True, fill=7)[0]
    got = C.clean_label(d, 20, min_size=3, fill=7, fill_holes=True, smooth_mm=1.0, spacing=sp)
    assert np.array_equal(got.cpu().numpy(), ref) and (ref != CR.clean_label(vol, 20, min_size=3, holes=True, fill=7)[0]).any()
    outs, tables = C.clean_labels([d, _layout(vol, 'f')], 20, min_size=3, fill=7, fill_holes=True, smooth_mm=1.0, spacing=sp)
    assert tables.shape == (2, 4) and all(torch.equal(o, got) for o in outs)
    with pytest.raises(ValueError):
        C.clean_label(d, 20, smooth_mm=-1.0)


# ------------------------------------------------------------------------------------------------ guard bands, determinism, refusals, ABI
@pytest.mark.parametrize('out_dtype', (F64, U8))
def test_workspace_content_does_not_matter(out_dtype):
    T = _tile()[0]
    a = FR.volume((T + 3, 9, 37), np.float32)
    d = _layout(a, 'box')
    weights = [FR.gaussian_kernel1d(s, 0, int(4.0 * s + 0.5))[::-1] for s in (1.0, 0.7, 1.5)]
    for active in ((0, 1, 2), (0, 2), (1,), ()):
        ws_ = [w if i in active else None for i, w in enumerate(weights)]
        want = FR.gaussian_filter(a, tuple((1.0, 0.7, 1.5)[i] if i in active else 0.0 for i in range(3)), mode='mirror')
        raw = []
        for fill in (0xFF, 0x5A):                             # 0xFF: every double of the workspace is a NaN
            need = _need(a.shape, _axes(ws_))
            assert need >= 16 and need % 16 == 0
            rc, g, ws = _call(d, ws_, 'mirror', out_dtype=out_dtype, threshold=10.0, ws=_Ws(need, fill))
            assert rc == 0
            raw.append(g.big.view(torch.uint8).clone())
            if out_dtype == F64:
                _same(_result(g), want, active)
            else:
                assert np.array_equal(_result(g), (want >= 10.0).astype(np.uint8)), active
        assert torch.equal(raw[0], raw[1]), active


def test_refusals_write_nothing():
    lib, L = _lib()
    a = FR.volume((6, 7, 8), np.float32)
    d = _layout(a, 'c')
    w3 = np.array([0.25, 0.5, 0.25])
    good = [w3, w3, w3]
    need = _need(a.shape, _axes(good))
    assert need == 2 * 6 * 7 * 8 * 8
    g64, g8 = Guarded((8, 6, 7), torch.float64), Guarded((8, 6, 7), torch.uint8)
    before64, before8 = g64.big.view(torch.uint8).clone(), g8.big.clone()
    ws = _Ws(need, 0xA5)
    null = ctypes.c_void_p(0)
    bad_w = np.array([0.25, np.inf, 0.25])
    wide = (MAX_RADIUS + 1, 1, np.zeros(3))
    cases = [
        (dict(src_ptr=null), ERR_ARG), (dict(A=(6, 0, 8)), ERR_ARG), (dict(A=(-1, 7, 8)), ERR_ARG), (dict(dtype=2), ERR_ARG), (dict(dtype=9), ERR_ARG),
        (dict(in_mode=2), ERR_ARG), (dict(mode=5), ERR_ARG), (dict(mode=-1), ERR_ARG), (dict(weights=[w3, (1, 2, w3), w3]), ERR_ARG),
        (dict(weights=[w3, bad_w, w3]), ERR_ARG), (dict(weights=[w3, w3, np.array([np.nan])]), ERR_ARG), (dict(cval=np.inf), ERR_ARG),
        (dict(cval=np.nan), ERR_ARG), (dict(out_dtype=4), ERR_ARG), (dict(out_dtype=1), ERR_ARG), (dict(ws_bytes=need - 1), ERR_ARG),
        (dict(ws=_Ws(need, 0xA5, off=8)), ERR_ARG), (dict(weights=[w3, wide, w3]), ERR_UNSUPPORTED),
        (dict(A=(1 << 11, 1 << 10, (1 << 9) + 1)), ERR_UNSUPPORTED),
    ]
    for kw, code in cases:
        for g, od in ((g64, F64), (g8, U8)):
            if 'out_dtype' in kw and od == U8:
                continue
            args = dict(weights=good, ws=ws, out=g, out_dtype=od)
            args.update(kw)
            rc, _, used = _call(d, args.pop('weights'), **args)
            assert rc == code, (kw, rc)
            assert used.untouched(), kw
    assert torch.equal(g64.big.view(torch.uint8), before64) and torch.equal(g8.big, before8)
    # NULL out / workspace / axes, and an output that overlaps the input
    o = g64.t.permute(1, 2, 0)
    desc = _axes(good)

    def raw(vol=None, axes=desc, out=None, wsp=ws.ptr, ost=None, dt=4):
        return L.cdll.hv_separable_filter(lib.ptr(d) if vol is None else vol, dt, *_ll(d.stride()), 6, 7, 8, IN_VALUE, ctypes.c_double(0.0), axes, 0,
                                          ctypes.c_double(0.0), lib.ptr(o) if out is None else out, F64, ctypes.c_double(0.0),
                                          *_ll(o.stride() if ost is None else ost), wsp, ctypes.c_size_t(need), lib.stream())
    assert raw(out=null) == ERR_ARG and raw(wsp=null) == ERR_ARG and raw(axes=None) == ERR_ARG
    d64 = torch.zeros(6, 7, 8, dtype=torch.float64, device='cuda')
    assert raw(vol=lib.ptr(d64), out=lib.ptr(d64), ost=d64.stride(), dt=5) == ERR_ARG
    assert raw(vol=lib.ptr(d64), out=ctypes.c_void_p(d64.data_ptr() + 8 * 100), ost=d64.stride(), dt=5) == ERR_ARG
    assert L.size('hv_filter_workspace_bytes', 6, 0, 8, desc) == 0 and L.size('hv_filter_workspace_bytes', 6, 7, 8, _axes([w3, wide, w3])) == 0
    assert L.cdll.hv_filter_tile(None) == ERR_ARG
    torch.cuda.synchronize()
    assert torch.equal(g64.big.view(torch.uint8), before64) and ws.untouched() and not bool(d64.any())
    assert raw() == 0
    torch.cuda.synchronize()
    _same(_result(g64), FR.correlate1d(FR.correlate1d(FR.correlate1d(a, w3, 0), w3, 1), w3, 2), 'the accepted call')
    with pytest.raises(ValueError):
        _F().gaussian_filter(d64, 1.0, out=d64)


def test_abi():
    _, L = _lib()
    for name in ('hv_separable_filter', 'hv_filter_workspace_bytes', 'hv_filter_tile', 'hv_blend_lerp'):
        assert name in L.protos and getattr(L.cdll, name) is not None
    assert ctypes.sizeof(L.hv_filter_axis) == 8 + 8 * (2 * MAX_RADIUS + 1)
    assert all(1 <= t <= MAX_RADIUS for t in _tile())
    assert _F().MAX_RADIUS == MAX_RADIUS
