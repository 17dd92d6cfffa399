"""hv_morph_ball / hv_morph_struct / hv_morph_merge (csrc/morph.hip) and healthivert-gan_amd/morphology.py against tests/morph_ref.py (scipy
with the ball of the shared expression, pinned by tests/test_morph_ref_cpu.py): every comparison is byte for byte.  Outputs lie between guard
words, with strides other than the input's; the workspace is exactly the queried bytes inside a 0xA5 border.  Shapes are built from the tile
shape the library reports (hv_morph_tile); one volume is long enough along axis 0 / axis 2 for the 16-bit carrier."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import ccl_ref as CR
import morph_ref as MR
from hvtest import Guarded

pytestmark = pytest.mark.gpu

EQ, NE = 0, 1
OP = {'dilation': 0, 'erosion': 1, 'opening': 2, 'closing': 3}
GROW, SHRINK = 0, 1
_DT = {torch.uint8: 0, torch.float32: 4, torch.float64: 5}
UNIT, ANISO = (1.0, 1.0, 1.0), (0.7, 0.7, 1.5)
BALLS = [(r, UNIT) for r in (0.0, 1.0, np.sqrt(2.0), np.sqrt(3.0), 2.5)] + [(r, ANISO) for r in (1.0, 1.6, 3.1)]


def _lib():
    import hvgan  # noqa: F401
    from hvgan import lib
    return lib, lib.get()


def _M():
    import hvgan  # noqa: F401
    from hvgan import morphology
    return morphology


def _tile():
    _, L = _lib()
    dims = (ctypes.c_int * 3)()
    assert L.cdll.hv_morph_tile(dims) == 0
    return tuple(dims)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


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


def _need(A, radius=0.0, sp=None):
    return _lib()[1].size('hv_morph_workspace_bytes', *A, ctypes.c_double(float(radius)), None if sp is None else (ctypes.c_double * 3)(*sp))


def _ll(st):
    return [ctypes.c_longlong(s) for s in st]


def _out_view(A):
    """A guarded uint8 output of shape A whose strides are those of a [A2][A0][A1] array: never the input's."""
    g = Guarded((A[2], A[0], A[1]), torch.uint8)
    return g, g.t.permute(1, 2, 0)


def _ball(src, op, radius, sp=UNIT, border=0, value=0.0, mode=NE, ws=None, ws_bytes=None, opcode=None, sp_arg=True):
    """One hv_morph_ball on the device tensor `src` -> (return code, the mask as numpy, the raw guarded bytes, the workspace)."""
    lib, L = _lib()
    A = tuple(int(s) for s in src.shape)
    g, out = _out_view(A)
    ws = ws or _Ws(max(_need(A, radius, sp), 16))
    rc = L.cdll.hv_morph_ball(lib.ptr(src), _DT[src.dtype], *_ll(src.stride()), *A, ctypes.c_double(float(value)), mode,
                              OP[op] if opcode is None else opcode, ctypes.c_double(float(radius)),
                              (ctypes.c_double * 3)(*sp) if sp_arg else None, border, lib.ptr(out), *_ll(out.stride()), ws.ptr,
                              ctypes.c_size_t(ws.need if ws_bytes is None else ws_bytes), lib.stream())
    torch.cuda.synchronize()
    assert g.intact() and ws.border_intact(), 'wrote outside a buffer'
    return rc, out.cpu().numpy(), g.big.clone(), ws


def _struct(src, op, conn, iters=1, border=0, value=0.0, mode=NE, ws=None, ws_bytes=None):
    lib, L = _lib()
    A = tuple(int(s) for s in src.shape)
    g, out = _out_view(A)
    ws = ws or _Ws(_need(A))
    rc = L.cdll.hv_morph_struct(lib.ptr(src), _DT[src.dtype], *_ll(src.stride()), *A, ctypes.c_double(float(value)), mode, OP[op], conn, iters,
                                border, lib.ptr(out), *_ll(out.stride()), ws.ptr, ctypes.c_size_t(ws.need if ws_bytes is None else ws_bytes),
                                lib.stream())
    torch.cuda.synchronize()
    assert g.intact() and ws.border_intact(), 'wrote outside a buffer'
    return rc, out.cpu().numpy(), g.big.clone(), ws


def _merge(src, mask, rule, value, background=0.0, fill=0.0, out=None, out_strides=None):
    lib, L = _lib()
    A = tuple(int(s) for s in src.shape)
    g = None
    if out is None:
        g = Guarded(A, src.dtype)
        out = g.t
    rc = L.cdll.hv_morph_merge(lib.ptr(src), _DT[src.dtype], *_ll(src.stride()), *A, lib.ptr(mask), *_ll(mask.stride()), rule,
                               ctypes.c_double(float(value)), ctypes.c_double(float(background)), ctypes.c_double(float(fill)), lib.ptr(out),
                               *_ll(out.stride() if out_strides is None else out_strides), lib.stream())
    torch.cuda.synchronize()
    assert g is None or g.intact(), 'wrote outside a buffer'
    return rc, out.cpu().numpy()


def _check_ball(X, src, op, radius, sp, border, what, **kw):
    rc, got, _, _ = _ball(src, op, radius, sp, border, **kw)
    assert rc == 0, what
    want = MR.by_ball(op, X, radius, sp, border).astype(np.uint8)
    assert np.array_equal(got, want), (what, op, radius, sp, border, int((got != want).sum()))
    return got


def _check_struct(X, src, op, conn, iters, border, what, **kw):
    rc, got, _, _ = _struct(src, op, conn, iters, border, **kw)
    assert rc == 0, what
    want = MR.by_struct(op, X, conn, iters, border).astype(np.uint8)
    assert np.array_equal(got, want), (what, op, conn, iters, border, int((got != want).sum()))
    return got


def _edge_shape(case):
    """('tile', axis, which): the axis at T - 1, T, T + 1 or 2 T + 1 for the tile extent T the library reports, the other axes 5 to 9; or a
    fixed shape."""
    if case[0] != 'tile':
        return case
    T = _tile()
    other = ((0, 7, 9), (5, 0, 9), (7, 5, 0))
    s = list(other[case[1]])
    s[case[1]] = (T[case[1]] - 1, T[case[1]], T[case[1]] + 1, 2 * T[case[1]] + 1)[case[2]]
    return tuple(s)


_EDGE_CASES = [('tile', axis, which) for axis in range(3) for which in range(4)] + [(1, 1, 1), (1, 7, 9), (7, 1, 9), (7, 9, 1), (19, 23, 70)]


# ------------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize('case', _EDGE_CASES, ids=lambda c: '-'.join(str(d) for d in c))
def test_shapes_at_the_edges_of_the_tiles(case):
    shape = _edge_shape(case)
    big = shape == (19, 23, 70)
    for name, X in MR.contents(shape, seed=sum(shape)).items():
        if big and name not in ('d0.02', 'd0.50'):
            continue
        src = _dev(X.astype(np.uint8))
        for op, border in itertools.product(MR.OPS, (0, 1)):
            _check_ball(X, src, op, 2.5, UNIT, border, (shape, name))
            _check_ball(X, src, op, 1.6, ANISO, border, (shape, name))
            _check_struct(X, src, op, 2, 2, border, (shape, name))


# ------------------------------------------------------------------------------------------------ every op, border value, radius, structure
@pytest.mark.parametrize('name', ('d0.02', 'd0.50', 'd0.98', 'empty', 'full', 'corner'))
def test_every_op_border_and_ball(name):
    T = _tile()
    shape = (T[0] + 1, T[1] + 3, T[2] + 5)
    X = MR.contents(shape, seed=7)[name]
    src = _dev(X.astype(np.uint8))
    for (radius, sp), op, border in itertools.product(BALLS, MR.OPS, (0, 1)):
        got = _check_ball(X, src, op, radius, sp, border, name)
        if radius == 0.0:
            assert np.array_equal(got, X.astype(np.uint8))                  # the ball is the origin alone


@pytest.mark.parametrize('connectivity', (1, 2, 3))
@pytest.mark.parametrize('iterations', (1, 2, 3))
def test_every_op_border_and_structure(connectivity, iterations):
    T = _tile()
    shape = (T[0] + 1, T[1] + 3, T[2] + 5)
    for name, X in MR.contents(shape, seed=11).items():
        src = _dev(X.astype(np.uint8))
        for op, border in itertools.product(MR.OPS, (0, 1)):
            _check_struct(X, src, op, connectivity, iterations, border, name)


def test_package_ball_is_the_shared_expression():
    M = _M()
    for (radius, sp) in BALLS + [(3.2, (2.5, 0.9, 0.9)), (7.3, ANISO)]:
        b = M.ball(radius, sp)
        assert b.dtype == np.bool_ and np.array_equal(b, MR.ball(radius, sp)), (radius, sp)


def test_gaps_and_bridges():
    """r = 1 closes a gap of one and of two planes (each side grows one voxel into it), not of three; an opening cuts a one-voxel bridge."""
    M = _M()
    for gap in (1, 2, 3):
        X = MR.slabs(gap)
        got = _check_ball(X, _dev(X.astype(np.uint8)), 'closing', 1.0, UNIT, 0, gap)
        assert bool(got[4, 4, 6:6 + gap].all()) == (gap <= 2) and bool(got[4, 4, 6:6 + gap].any()) == (gap <= 2)
        assert CR.label(got, 1)[1] == (1 if gap <= 2 else 2)
    X, bridge = MR.bridged()
    assert CR.label(X, 1)[1] == 1
    got = _check_ball(X, _dev(X.astype(np.uint8)), 'opening', 1.0, UNIT, 0, 'bridge')
    assert CR.label(got, 1)[1] == 2 and not got[5, 5, 9:11].any()
    assert np.array_equal(M.binary_opening(X, radius=1.0).cpu().numpy(), got)


def test_a_ball_larger_than_the_volume():
    for shape in ((5, 4, 6), (1, 7, 9), (1, 1, 1)):
        for name, X in MR.contents(shape, seed=2).items():
            src = _dev(X.astype(np.uint8))
            for op, border in itertools.product(MR.OPS, (0, 1)):
                _check_ball(X, src, op, 12.0, UNIT, border, (shape, name))
                _check_ball(X, src, op, 12.0, ANISO, border, (shape, name))


def test_sixteen_bit_carrier():
    """A reach above 254 steps along axis 0 or axis 2 takes the uint16 counts.  scipy would need a 521^3 structure: the reference here is the
    thresholded ordered squared distance, which tests/test_morph_ref_cpu.py holds against scipy."""
    r2 = 260.0 * 260.0
    for shape in ((300, 3, 2), (2, 3, 300)):
        assert _need(shape, 260.0) > _need(shape, 2.0)
        X = np.zeros(shape, dtype=bool)
        X[0, 1, 0] = True
        src = _dev(X.astype(np.uint8))
        for border in (0, 1):
            rc, got, _, _ = _ball(src, 'dilation', 260.0, UNIT, border)
            assert rc == 0 and np.array_equal(got, (MR.d2(X, UNIT, border) <= r2).astype(np.uint8)), (shape, border)
            if border == 0:
                assert got.sum() == 260 * 6 + 1              # 259^2 + 2 <= 260^2 < 260^2 + 1: the plane 260 steps away holds one voxel
            rc, got, _, _ = _ball(src, 'erosion', 260.0, UNIT, border)
            assert rc == 0 and np.array_equal(got, (~(MR.d2(~X, UNIT, 1 - border) <= r2)).astype(np.uint8)), (shape, border)


# ------------------------------------------------------------------------------------------------ layouts, dtypes, modes
def test_layouts_dtypes_and_modes():
    T = _tile()
    shape = (T[0] + 2, T[1] + 1, T[2] + 3)
    m = MR.random_mask(shape, 0.4, 9)
    vol = np.where(m, 3, np.where(MR.random_mask(shape, 0.5, 10), 0, 7))
    for dt, pad in ((np.uint8, 255), (np.float32, np.nan), (np.float64, np.nan)):
        c = _dev(vol.astype(dt))
        z = _dev(np.ascontiguousarray(vol.astype(dt).transpose(2, 0, 1))).permute(1, 2, 0)               # z-fastest permuted strides
        big = torch.full((shape[0] + 3, shape[1] + 2, 2 * shape[2] + 1), pad, dtype=c.dtype, device='cuda')
        sub = big[2:2 + shape[0], 1:1 + shape[1], 1:1 + 2 * shape[2]:2]
        sub.copy_(c)
        keep = big.clone()
        for src in (c, z, sub):
            assert tuple(src.shape) == shape
            for X, value, mode in ((vol == 3, 3, EQ), (vol != 0, 0, NE), (vol != 7, 7, NE)):
                _check_ball(X, src, 'closing', 1.6, ANISO, 0, (dt, src.stride()), value=value, mode=mode)
                _check_ball(X, src, 'erosion', np.sqrt(2.0), UNIT, 1, (dt, src.stride()), value=value, mode=mode)
                _check_struct(X, src, 'opening', 3, 2, 0, (dt, src.stride()), value=value, mode=mode)
        assert torch.equal(big.view(torch.uint8), keep.view(torch.uint8))                                # the source is only read


# ------------------------------------------------------------------------------------------------ identities
def test_identities():
    shape = (9, 12, 70)
    X = MR.random_mask(shape, 0.6, 5) | CR.ellipsoid(shape, (4.0, 6.0, 30.0), (3.0, 4.0, 20.0))
    src, neg = _dev(X.astype(np.uint8)), _dev((~X).astype(np.uint8))
    for radius, sp in ((1.0, UNIT), (2.5, UNIT), (1.6, ANISO)):
        # idempotent where the faces of the volume do not interfere -- the opening with the outside clear, the closing with the outside set
        # (both are then the operation on the unbounded grid); with the other border value the second application is still scipy's
        for op, border in itertools.product(('opening', 'closing'), (0, 1)):
            _, once, _, _ = _ball(src, op, radius, sp, border)
            _, twice, _, _ = _ball(_dev(once), op, radius, sp, border)
            assert np.array_equal(twice, MR.by_ball(op, once.astype(bool), radius, sp, border).astype(np.uint8)), (op, border)
            if (op, border) in (('opening', 0), ('closing', 1)):
                assert np.array_equal(once, twice), (op, radius, sp)
        _, e0, _, _ = _ball(src, 'erosion', radius, sp, 0)
        _, d1, _, _ = _ball(neg, 'dilation', radius, sp, 1)
        assert np.array_equal(e0, 1 - d1)
    for c in (1, 2, 3):
        _, e0, _, _ = _struct(src, 'erosion', c, 2, 0)
        _, d1, _, _ = _struct(neg, 'dilation', c, 2, 1)
        assert np.array_equal(e0, 1 - d1)


def test_surface_counts_of_hv_surface_distance():
    """X & ~erode(X, connectivity 1, border_value 0) is the surface hv_surface_distance counts in out[0] / out[1]."""
    import hvgan  # noqa: F401
    from hvgan import generation_eval as GE
    shape = (20, 18, 16)
    a = CR.ellipsoid(shape, (9.0, 9.0, 8.0), (6.0, 7.0, 5.0)).astype(np.uint8)
    b = CR.ellipsoid(shape, (10.0, 8.0, 7.0), (9.5, 5.0, 7.5)).astype(np.uint8)     # touches the face i = 0
    _, raw = GE.surface_distances(a, b, label=1, return_raw=True)
    for v, n in ((a, raw[0]), (b, raw[1])):
        _, er, _, _ = _struct(_dev(v), 'erosion', 1, 1, 0, value=1, mode=EQ)
        assert int((v.astype(bool) & ~er.astype(bool)).sum()) == int(n) > 0


# ------------------------------------------------------------------------------------------------ determinism
def test_two_calls_and_a_poisoned_workspace_give_the_same_bytes():
    T = _tile()
    shape = (2 * T[0] + 1, T[1] + 3, T[2] + 5)
    src = _dev(MR.random_mask(shape, 0.45, 21).astype(np.uint8))
    for call in (lambda ws: _ball(src, 'closing', 3.1, ANISO, 0, ws=ws), lambda ws: _ball(src, 'opening', 2.5, UNIT, 1, ws=ws),
                 lambda ws: _struct(src, 'closing', 2, 3, 1, ws=ws), lambda ws: _struct(src, 'erosion', 1, 1, 0, ws=ws)):
        raws = []
        for fill in (0xA5, 0xA5, 0xFF, 0x00):
            rc, _, raw, _ = call(_Ws(_need(shape, 3.1, ANISO), fill=fill))
            assert rc == 0
            raws.append(raw)
        assert all(torch.equal(raws[0], r) for r in raws[1:])


# ------------------------------------------------------------------------------------------------ the merge and the label forms
def test_merge_rules_layouts_and_in_place():
    shape = (5, 9, 70)
    vol = np.where(MR.random_mask(shape, 0.3, 1), 5, np.where(MR.random_mask(shape, 0.3, 2), 7, 0))
    mask = MR.random_mask(shape, 0.5, 3).astype(np.uint8)
    for dt in (np.uint8, np.float32, np.float64):
        v = vol.astype(dt)
        c = _dev(v)
        z = _dev(np.ascontiguousarray(v.transpose(2, 0, 1))).permute(1, 2, 0)
        mz = _dev(np.ascontiguousarray(mask.transpose(1, 2, 0))).permute(2, 0, 1)
        for src, mk in ((c, _dev(mask)), (z, mz), (c, mz)):
            for rule, name, kw in ((GROW, 'grow', dict(background=0, fill=9)), (GROW, 'grow', dict(background=7, fill=9)),
                                   (SHRINK, 'shrink', dict(background=0, fill=9))):
                want = MR.merge(v, mask, name, 5, **kw)
                rc, got = _merge(src, mk, rule, 5, **kw)
                assert rc == 0 and got.dtype == want.dtype and np.array_equal(got, want), (dt, name, kw)
                keepers = (v != kw['background']) if rule == GROW else (v != 5)
                assert np.array_equal(got[keepers], v[keepers])                  # other labels are never overwritten
                inplace = src.clone(memory_format=torch.preserve_format)
                assert inplace.stride() == src.stride()
                rc, got2 = _merge(inplace, mk, rule, 5, out=inplace, **kw)
                assert rc == 0 and np.array_equal(got2, want)


def test_close_label_and_open_label():
    M = _M()
    vol = MR.two_fragment_body()
    for dt in (np.uint8, np.float32):
        v = vol.astype(dt)
        for radius, sp in ((1.0, UNIT), (1.6, ANISO)):
            want = MR.close_label(v, 20, radius, sp)
            got = M.close_label(v, 20, radius, sp)
            assert got.is_cuda and got.cpu().numpy().dtype == v.dtype and np.array_equal(got.cpu().numpy(), want)
            assert np.array_equal(want[v != 0], v[v != 0]) and (want != v).any()
            d = _dev(v)
            assert M.close_label(d, 20, radius, sp, out=d) is d and np.array_equal(d.cpu().numpy(), want)      # in place
    b, bridge = MR.bridged()
    v = np.where(b, 4, 0).astype(np.uint8)
    v[0, 0, :] = 6
    want = MR.open_label(v, 4, 1.0, fill=1)
    got = M.open_label(v, 4, 1.0, fill=1)
    assert np.array_equal(got.cpu().numpy(), want) and (want[5, 5, 9:11] == 1).all() and np.array_equal(want[v != 4], v[v != 4])
    d = _dev(v)
    out = torch.empty_like(d)
    assert M.open_label(d, 4, 1.0, fill=1, out=out) is out and np.array_equal(out.cpu().numpy(), want) and np.array_equal(d.cpu().numpy(), v)
    assert M.open_label(d, 4, 1.0, fill=1, out=d) is d and np.array_equal(d.cpu().numpy(), want)


def test_wrappers():
    M = _M()
    shape = (6, 10, 66)
    X = MR.random_mask(shape, 0.5, 8)
    vol = np.where(X, 2.0, 0.0)
    fns = {'dilation': M.binary_dilation, 'erosion': M.binary_erosion, 'opening': M.binary_opening, 'closing': M.binary_closing}
    for op, fn in fns.items():
        got = fn(X, radius=1.6, spacing=ANISO, border_value=1)                  # a host bool array is uploaded
        assert got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), MR.by_ball(op, X, 1.6, ANISO, 1))
        got = fn(_dev(vol), value=2, connectivity=2, iterations=2)
        assert np.array_equal(got.cpu().numpy(), MR.by_struct(op, X, 2, 2, 0))
        out = torch.empty(shape, dtype=torch.uint8, device='cuda')
        assert fn(vol, value=0, radius=2.0, out=out) is out and np.array_equal(out.cpu().numpy(), MR.by_ball(op, ~X, 2.0))
    for kw in (dict(), dict(radius=1.0, connectivity=1), dict(radius=-1.0), dict(radius=float('nan')), dict(radius=1.0, spacing=(1, 0, 1)),
               dict(connectivity=4), dict(connectivity=1, iterations=0), dict(radius=1.0, border_value=2), dict(radius=1.0, iterations=2),
               dict(radius=1.0, out=torch.empty(shape, dtype=torch.float32, device='cuda'))):
        with pytest.raises(ValueError):
            M.binary_closing(X, **kw)
    with pytest.raises(ValueError):
        M.binary_closing(X[0], radius=1.0)


def test_clean_label_with_a_closing_keeps_the_fragment():
    """The fragment a one-voxel gap separates from the body: without closing_mm keep_largest drops it, with closing_mm=1.0 it stays."""
    import hvgan  # noqa: F401
    from hvgan import components as C
    vol = MR.two_fragment_body()
    fragment = np.zeros(vol.shape, dtype=bool)
    fragment[6:16, 6:16, 15:19] = True
    want = CR.clean_label(MR.close_label(vol, 20, 1.0), 20, 1, 0, True, True)[0]          # closing -> label -> largest -> binary_fill_holes
    got, table = C.clean_label(vol, 20, fill_holes=True, closing_mm=1.0, return_table=True)
    assert np.array_equal(got.cpu().numpy(), want) and (want[fragment] == 20).all() and want[20, 19, 26] == 0 and (want[9:12, 9:12, 7:10] == 20).all()
    assert list(table.cpu().numpy()[:2]) == [2, 1]                                          # the body with its fragment, and the speckle
    plain = C.clean_label(vol, 20, fill_holes=True).cpu().numpy()
    assert np.array_equal(plain, CR.clean_label(vol, 20, 1, 0, True, True)[0]) and (plain[fragment] == 0).all()
    assert np.array_equal(got.cpu().numpy()[vol == 19], vol[vol == 19])
    # anisotropic spacing, the opening before the closing, in place, and the list form with its one readback
    sp = (0.7, 0.7, 1.5)
    chain = MR.close_label(MR.open_label(vol, 20, 0.7, sp), 20, 1.5, sp)
    want2 = CR.clean_label(chain, 20, 2, 5, True, False)[0]
    d = _dev(vol)
    assert C.clean_label(d, 20, 2, 5, out=d, closing_mm=1.5, opening_mm=0.7, spacing=sp) is d and np.array_equal(d.cpu().numpy(), want2)
    outs, tables = C.clean_labels([vol, vol.astype(np.float32)], 20, fill_holes=True, closing_mm=1.0)
    assert tables.shape == (2, 4) and all(np.array_equal(o.cpu().numpy(), want) for o in outs)
    with pytest.raises(ValueError):
        C.clean_label(vol, 20, closing_mm=-1.0)
    with pytest.raises(ValueError):
        C.clean_labels([vol], 20, opening_mm=1.0, spacing=(1, 1))


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_every_buffer_untouched():
    shape = (5, 9, 66)
    X = MR.random_mask(shape, 0.5, 4)
    src = _dev(X.astype(np.uint8))
    need = _need(shape, 2.0)
    assert need > 0 and need % 16 == 0
    inf, nan = float('inf'), float('nan')
    ball_cases = [dict(radius=-1.0), dict(radius=inf), dict(radius=nan), dict(radius=1e200), dict(sp=(1.0, 0.0, 1.0)), dict(sp=(1.0, -2.0, 1.0)),
                  dict(sp=(inf, 1.0, 1.0)), dict(sp=(1.0, 1.0, nan)), dict(sp_arg=False), dict(border=2), dict(border=-1), dict(opcode=4),
                  dict(opcode=-1), dict(mode=2), dict(ws_bytes=need - 1), dict(ws=_Ws(need, off=8))]
    for kw in ball_cases:
        args = dict(dict(op='closing', radius=2.0, sp=UNIT, border=0, ws=_Ws(need)), **kw)
        rc, out, _, ws = _ball(src, **args)
        assert rc == -1 and (out == 0xA5).all() and ws.untouched(), kw
    for kw in (dict(conn=0), dict(conn=4), dict(iters=0), dict(iters=-2), dict(border=2), dict(mode=3), dict(ws_bytes=_need(shape) - 1),
               dict(ws=_Ws(_need(shape), off=4))):
        args = dict(dict(op='opening', conn=1, iters=1, border=0, ws=_Ws(_need(shape))), **kw)
        rc, out, _, ws = _struct(src, **args)
        assert rc == -1 and (out == 0xA5).all() and ws.untouched(), kw
    lib, L = _lib()
    g, out = _out_view(shape)
    ws = _Ws(need)
    sp = (ctypes.c_double * 3)(*UNIT)
    nul = ctypes.c_void_p(0)
    for vol_p, out_p, ws_p, dtype, A in ((nul, lib.ptr(out), ws.ptr, 0, shape), (lib.ptr(src), nul, ws.ptr, 0, shape),
                                         (lib.ptr(src), lib.ptr(out), nul, 0, shape), (lib.ptr(src), lib.ptr(out), ws.ptr, 1, shape),
                                         (lib.ptr(src), lib.ptr(out), ws.ptr, 0, (5, 0, 66)), (lib.ptr(src), lib.ptr(out), ws.ptr, 0, (-1, 9, 66))):
        rc = L.cdll.hv_morph_ball(vol_p, dtype, *_ll(src.stride()), *A, ctypes.c_double(0.0), NE, 0, ctypes.c_double(1.0), sp, 0, out_p,
                                  *_ll(out.stride()), ws_p, ctypes.c_size_t(need), lib.stream())
        assert rc == -1
        rc = L.cdll.hv_morph_struct(vol_p, dtype, *_ll(src.stride()), *A, ctypes.c_double(0.0), NE, 0, 1, 1, 0, out_p, *_ll(out.stride()), ws_p,
                                    ctypes.c_size_t(need), lib.stream())
        assert rc == -1
    # more than 2^30 voxels, and a line the staging does not hold: refused on the sizes alone, nothing of that size is allocated
    rc = L.cdll.hv_morph_ball(lib.ptr(src), 0, *_ll((1, 1, 1)), 1024, 1024, 1025, ctypes.c_double(0.0), NE, 0, ctypes.c_double(1.0), sp, 0,
                              lib.ptr(out), *_ll((0, 0, 0)), ws.ptr, ctypes.c_size_t(1 << 40), lib.stream())
    assert rc == -2
    rc = L.cdll.hv_morph_struct(lib.ptr(src), 0, *_ll((1, 1, 1)), 1024, 1024, 1025, ctypes.c_double(0.0), NE, 0, 1, 1, 0, lib.ptr(out),
                                *_ll((0, 0, 0)), ws.ptr, ctypes.c_size_t(1 << 40), lib.stream())
    assert rc == -2
    rc = L.cdll.hv_morph_ball(lib.ptr(src), 0, *_ll((1, 1, 1)), 1, 1, 32769, ctypes.c_double(0.0), NE, 0, ctypes.c_double(1.0), sp, 0, lib.ptr(out),
                              *_ll((0, 0, 0)), ws.ptr, ctypes.c_size_t(1 << 40), lib.stream())
    assert rc == -2
    rc = L.cdll.hv_morph_ball(lib.ptr(src), 0, *_ll((1, 1, 1)), 70000, 1, 1, ctypes.c_double(0.0), NE, 0, ctypes.c_double(69000.0), sp, 0,
                              lib.ptr(out), *_ll((0, 0, 0)), ws.ptr, ctypes.c_size_t(1 << 40), lib.stream())
    assert rc == -2                                                                         # a reach beyond the 16-bit carrier
    assert _need((5, 0, 66)) == 0 and _need(shape, -1.0) == 0 and _need(shape, 1.0, (1.0, 0.0, 1.0)) == 0
    assert L.cdll.hv_morph_tile(None) == -1
    # the merge: NULL pointers, an unknown rule or dtype, out == vol with other strides
    mask = _dev(X.astype(np.uint8))
    keep = src.clone()
    for kw in (dict(rule=2), dict(rule=-1)):
        rc, got = _merge(src, mask, kw['rule'], 1)
        assert rc == -1 and (got == 0xA5).all()
    rc, _ = _merge(src, mask, GROW, 1, out=src, out_strides=src.permute(0, 2, 1).stride())
    assert rc == -1
    rc = L.cdll.hv_morph_merge(lib.ptr(src), 0, *_ll(src.stride()), *shape, nul, *_ll(mask.stride()), GROW, ctypes.c_double(1.0),
                               ctypes.c_double(0.0), ctypes.c_double(0.0), lib.ptr(src), *_ll(src.stride()), lib.stream())
    assert rc == -1
    rc = L.cdll.hv_morph_merge(lib.ptr(src), 2, *_ll(src.stride()), *shape, lib.ptr(mask), *_ll(mask.stride()), GROW, ctypes.c_double(1.0),
                               ctypes.c_double(0.0), ctypes.c_double(0.0), lib.ptr(src), *_ll(src.stride()), lib.stream())
    assert rc == -1
    torch.cuda.synchronize()
    assert torch.equal(src, keep) and g.intact() and (out.cpu().numpy() == 0xA5).all() and ws.untouched()


# ------------------------------------------------------------------------------------------------ one vertebra-sized case
def test_vertebra_sized_closing():
    M = _M()
    v = CR.full_size_case()
    sp = (0.7, 0.7, 1.5)
    got = M.binary_closing(_dev(v), value=20, radius=2.0, spacing=sp)
    want = MR.by_ball('closing', v == 20, 2.0, sp, 0)
    assert np.array_equal(got.cpu().numpy(), want.astype(np.uint8)) and (want != (v == 20)).any()
