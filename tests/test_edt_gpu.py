"""hv_edt (csrc/edt.hip) and generation_eval.distance_transform against the numpy restatement (tests/surface_ref.py, pinned against scipy by
tests/test_surface_ref_cpu.py): bit for bit at unit spacing, to EDT_TOL (relative) otherwise.

Shapes (surface_ref.edt_shapes): each axis in turn at 1, 2 and around the widths of the kernels -- ED_KT = 32 columns per tile of the axis-1
pass, ED_LINES = 32 lines per workgroup of the axis-2 pass, ED_THREADS = 256 lines per workgroup of the axis-0 pass -- with the other axes at
most 8, one line of 257 on the unit-stride axis, and one volume long enough (46 341 along axis 0) for the int64 carrier."""
import ctypes

import numpy as np
import pytest
import torch

import surface_ref as SR

pytestmark = pytest.mark.gpu

GUARD = 64
VALUE = 3


def _lib():
    import hvgan  # noqa: F401
    from hvgan import lib
    return lib, lib.get()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_DT = {torch.uint8: 0, torch.float32: 4, torch.float64: 5}


def _edt(src, value, sp, box=None, ws_bytes=None, out_fill=float('nan')):
    """One hv_edt call on the device tensor `src`: the output lies between guard words, the workspace is exactly the queried bytes inside a
    0xA5 border.  -> (return code, out numpy, the whole output buffer's bits, status word)."""
    lib, L = _lib()
    A = tuple(int(s) for s in src.shape)
    n = int(np.prod(A))
    buf = torch.full((n + 2 * GUARD,), out_fill, dtype=torch.float64, device='cuda')
    out = buf[GUARD:GUARD + n]
    need = L.size('hv_edt_workspace_bytes', *A) if ws_bytes is None else ws_bytes
    big = torch.full((512 + need,), 0xA5, dtype=torch.uint8, device='cuda')
    status = torch.full((3,), -7, dtype=torch.int32, device='cuda')
    rc = L.cdll.hv_edt(lib.ptr(src), _DT[src.dtype], *[ctypes.c_longlong(s) for s in src.stride()], *A, ctypes.c_double(float(value)),
                       (ctypes.c_double * 3)(*sp), None if box is None else (ctypes.c_int * 6)(*box), lib.ptr(out), lib.ptr(status[1:]),
                       lib.ptr(big[256:]), ctypes.c_size_t(need), lib.stream())
    torch.cuda.synchronize()
    assert bool((big[:256] == 0xA5).all()) and bool((big[256 + need:] == 0xA5).all()), 'wrote outside the queried workspace'
    st = status.cpu().numpy()
    assert st[0] == -7 and st[2] == -7
    bits = buf.view(torch.int64).clone()
    if rc == 0:
        assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[GUARD + n:]).all(), 'the guard words did not survive'
    return rc, out.cpu().numpy().reshape(A), bits, int(st[1])


def _check(got, ref, sp, what):
    if SR.is_unit(sp):
        assert np.array_equal(got, ref), what
        return 0.0
    inf = np.isinf(ref)
    assert np.array_equal(np.isinf(got), inf), what
    err = np.abs(got[~inf] - ref[~inf])
    assert (err <= SR.EDT_TOL * ref[~inf]).all(), (what, float(err.max()))
    return float(err.max()) if err.size else 0.0


def _volume(T, dtype=np.uint8, value=VALUE):
    """T marked with `value`, everything else with other values (0 and value + 1)."""
    v = np.where(T, value, 0).astype(dtype)
    other = ~T
    other[::2] = False
    v[other] = value + 1
    return v


@pytest.mark.parametrize('case', list(enumerate(SR.edt_shapes())), ids=lambda c: 'x'.join(str(d) for d in c[1]))
def test_edt_at_the_edges_of_its_tiles(case):
    si, shape = case
    worst = 0.0
    for kind in SR.TARGET_SETS:
        T = SR.target_set(shape, kind, si)
        src = _dev(_volume(T))
        for sp in SR.SPACINGS:
            rc, got, bits, status = _edt(src, VALUE, sp)
            assert rc == 0
            ref = SR.edt(T, sp)
            worst = max(worst, _check(got, ref, sp, (shape, kind, sp)))
            assert status == (0 if T.any() else 1), (shape, kind, status)
            if not T.any():
                assert np.isposinf(got).all()
        _, _, again, _ = _edt(src, VALUE, SR.SPACINGS[1])
        _, _, first, _ = _edt(src, VALUE, SR.SPACINGS[1])
        assert torch.equal(first, again), 'two runs differ'
    print(shape, 'largest |device - restatement| at the anisotropic spacings: %.3g' % worst)


def test_edt_float_volumes_and_a_view_with_nan_padding():
    shape = (6, 8, 33)
    for si, kind in enumerate(('random', 'checker', 'planes')):
        T = SR.target_set(shape, kind, 50 + si) if kind != 'random' else np.random.RandomState(7).rand(*shape) < 0.05
        for dt in (np.float32, np.float64):
            v = _volume(T, dt, 2.5)
            for sp in SR.SPACINGS:
                ref = SR.edt(T, sp)
                rc, got, _, status = _edt(_dev(v), 2.5, sp)
                assert rc == 0 and status == 0
                _check(got, ref, sp, (kind, dt, sp))
                # the same values inside a buffer of NaN: every second element along axis 2, a border along axis 1, axes 0 and 1 swapped in memory
                big = torch.full((shape[1] + 2, shape[0], 2 * shape[2]), float('nan'), dtype=torch.from_numpy(v).dtype, device='cuda')
                view = big[1:-1, :, ::2].permute(1, 0, 2)
                view.copy_(_dev(v))
                assert tuple(view.shape) == shape and not view.is_contiguous()
                rc, got2, _, status = _edt(view, 2.5, sp)
                assert rc == 0 and status == 0 and np.array_equal(got2, got)
    # NaN never equals: a NaN `value` has an empty target set
    rc, got, _, status = _edt(_dev(np.full((2, 3, 4), np.nan)), float('nan'), SR.SPACINGS[0])
    assert rc == 0 and status == 1 and np.isposinf(got).all()


def test_edt_of_a_sub_box_writes_and_reads_the_box_only():
    shape, box = (9, 40, 37), (2, 3, 5, 5, 33, 30)
    T = np.random.RandomState(11).rand(*shape) < 0.03
    sl = tuple(slice(box[a], box[a] + box[3 + a]) for a in range(3))
    assert T[sl].any() and T.sum() > T[sl].sum()
    src = _dev(_volume(T))
    for sp in SR.SPACINGS:
        rc, got, _, status = _edt(src, VALUE, sp, box=box)
        assert rc == 0 and status == 0
        _check(got[sl], SR.edt(T[sl], sp), sp, ('box', sp))
        outside = np.ones(shape, dtype=bool)
        outside[sl] = False
        assert np.isnan(got[outside]).all(), 'written outside the box'
    # a box without a target voxel, in a volume that has some
    T2 = np.zeros(shape, dtype=bool)
    T2[0, 0, 0] = True
    rc, got, _, status = _edt(_dev(_volume(T2)), VALUE, SR.SPACINGS[0], box=box)
    assert rc == 0 and status == 1 and np.isposinf(got[sl]).all()
    # a box of one voxel, and the whole volume given as a box
    rc, got, _, status = _edt(src, VALUE, SR.SPACINGS[0], box=(0, 0, 0) + shape)
    assert rc == 0 and np.array_equal(got, SR.edt(T))
    p = tuple(int(x) for x in np.argwhere(T)[0])
    rc, got, _, status = _edt(src, VALUE, SR.SPACINGS[0], box=p + (1, 1, 1))
    assert rc == 0 and status == 0 and got[p] == 0.0 and np.isnan(got).sum() == got.size - 1


def test_edt_carries_int64_where_int32_could_overflow():
    """46 341^2 > 2^31 - 1: the squared distances live in the output's own slots as int64.  Two target voxels, distances by the formula."""
    n = 46341
    v = np.zeros((n, 1, 2), dtype=np.uint8)
    v[5, 0, 0] = v[40000, 0, 1] = VALUE
    rc, got, _, status = _edt(_dev(v), VALUE, SR.SPACINGS[0])
    assert rc == 0 and status == 0
    i = np.arange(n, dtype=np.int64)[:, None]
    k = np.arange(2, dtype=np.int64)[None, :]
    ref = np.sqrt(np.minimum((i - 5) ** 2 + k ** 2, (i - 40000) ** 2 + (1 - k) ** 2).astype(np.float64))
    assert np.array_equal(got[:, 0, :], ref)
    assert got[n - 1, 0, 0] == np.sqrt(np.float64((n - 1 - 40000) ** 2 + 1))
    # one target at the far end: the largest squared distance, 46 340^2 + 1 = 2 147 395 601 > 2^31 - 1
    v[:] = 0
    v[n - 1, 0, 1] = VALUE
    rc, got, _, _ = _edt(_dev(v), VALUE, SR.SPACINGS[0])
    assert rc == 0 and got[0, 0, 0] == np.sqrt(np.float64(46340 ** 2 + 1)) and got[0, 0, 1] == 46340.0


def test_edt_refusals_leave_the_output_untouched():
    lib, L = _lib()
    shape = (5, 7, 9)
    src = _dev(_volume(SR.target_set(shape, 'corners')))
    need = L.size('hv_edt_workspace_bytes', *shape)
    assert need == (5 * 7 * 9 * 4 + 15) // 16 * 16
    for kw in (dict(sp=(1.0, 0.0, 1.0)), dict(sp=(1.0, float('nan'), 1.0)), dict(sp=(-1.0, 1.0, 1.0)), dict(sp=(1.0, 1.0, float('inf'))),
               dict(box=(0, 0, 0, 5, 7, 10)), dict(box=(4, 0, 0, 2, 7, 9)), dict(box=(0, -1, 0, 5, 7, 9)), dict(box=(0, 0, 0, 5, 0, 9)),
               dict(ws_bytes=need - 16)):
        args = dict(sp=SR.SPACINGS[0])
        args.update(kw)
        rc, got, bits, status = _edt(src, VALUE, out_fill=7.0, **args)
        assert rc == -1 and (got == 7.0).all() and status == -7, kw
        assert bool((bits == torch.tensor(7.0, dtype=torch.float64).view(torch.int64).item()).all())
    # unknown dtypes and NULL pointers
    out = torch.full((5 * 7 * 9,), 7.0, dtype=torch.float64, device='cuda')
    ws = torch.zeros(need, dtype=torch.uint8, device='cuda')
    status = torch.full((1,), -7, dtype=torch.int32, device='cuda')
    ones = (ctypes.c_double * 3)(1.0, 1.0, 1.0)

    def call(vol=lib.ptr(src), dt=0, sp=ones, o=lib.ptr(out), s=lib.ptr(status), w=lib.ptr(ws)):
        return L.cdll.hv_edt(vol, dt, *[ctypes.c_longlong(x) for x in src.stride()], *shape, ctypes.c_double(VALUE), sp, None, o, s, w,
                             ctypes.c_size_t(need), lib.stream())

    for kw in (dict(vol=None), dict(o=None), dict(s=None), dict(w=None), dict(sp=None), dict(dt=1), dict(dt=2), dict(dt=3), dict(dt=6), dict(dt=-1),
               dict(o=ctypes.c_void_p(out.data_ptr() + 4)), dict(w=ctypes.c_void_p(ws.data_ptr() + 8))):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert (out == 7.0).all() and int(status[0]) == -7 and (ws == 0).all()
    assert call() == 0


def test_distance_transform_wrapper():
    _lib()
    from scipy.ndimage import distance_transform_edt
    from hvgan import generation_eval as GE
    mask = SR.blob((20, 18, 12), (9.5, 8.0, 6.0), (7.0, 6.0, 4.0))
    for sp in (1.0, (0.7, 0.7, 1.5)):
        ref = distance_transform_edt(mask, sampling=sp)            # distance to the background: value 0
        tol = 0.0 if sp == 1.0 else SR.EDT_TOL
        for src in (mask, mask.astype(np.uint8), torch.from_numpy(mask.astype(np.float32)).cuda(), mask.astype(np.int64)):
            got = GE.distance_transform(src, spacing=sp)
            assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == mask.shape and got.is_contiguous()
            assert (np.abs(got.cpu().numpy() - ref) <= tol * ref).all()
    # value: the distance to the mask itself; out=; the status word
    out = torch.full(mask.shape, -1.0, dtype=torch.float64, device='cuda')
    res, status = GE.distance_transform(mask, value=1, out=out, return_status=True)
    assert res is out and int(status[0]) == 0 and np.array_equal(out.cpu().numpy(), distance_transform_edt(~mask))
    res, status = GE.distance_transform(mask, value=5, return_status=True)
    assert int(status[0]) == 1 and bool(torch.isinf(res).all())
    box = (3, 2, 1, 12, 10, 8)
    sl = tuple(slice(box[a], box[a] + box[3 + a]) for a in range(3))
    res = GE.distance_transform(mask, value=1, box=box).cpu().numpy()
    assert np.array_equal(res[sl], SR.edt(mask[sl])) and np.isnan(res).sum() == mask.size - 12 * 10 * 8
    dmask = torch.from_numpy(mask.astype(np.uint8)).cuda()
    keep = dmask.clone()
    GE.distance_transform(dmask)
    assert torch.equal(dmask, keep)
