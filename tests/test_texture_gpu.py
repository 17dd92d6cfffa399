"""hv_glcm (csrc/texture.hip) and healthivert-gan_amd/texture.py against tests/texture_ref.py (pinned against a brute force and Haralick's example
by tests/test_texture_ref_cpu.py).  Everything the entry writes is an integer count or a status word: out and info are compared bit for bit.
out and info lie between guard words and are pre-filled with 0xA5 bytes, the workspace is exactly the queried bytes inside a 0xA5 border.
The kernel's tiles are 16 x 16 x 16 with a halo of the offsets' reach; its LDS tables hold as many offsets per pass as fit beside the staging
(26 offsets of reach 4 at G = 32: four passes; G = 64: two offsets per pass)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import labelstats_ref as LR
import morph_ref as MR
import texture_ref as TR
from hvtest import ExactWs, Guarded

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED = -1, -2
SYM = 1
_VDT = {torch.uint8: 0, torch.int16: 1, torch.float32: 4, torch.float64: 5}
_LDT = {torch.uint8: 0, torch.int16: 1, torch.int32: 2, torch.int64: 3, torch.float32: 4, torch.float64: 5}
VOL_DTYPES = (np.uint8, np.int16, np.float32, np.float64)
D13 = TR.directions13()
D26 = D13 + [tuple(TR.MAX_REACH * c for c in d) for d in D13]
EDGE = (17, 18, 33)                            # one voxel past the 16^3 tile in every axis, three tiles along axis 2


def _lib():
    import hvgan  # noqa: F401
    from hvgan import lib
    return lib, lib.get()


def _T():
    import hvgan  # noqa: F401
    from hvgan import texture
    return texture


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


def _call(vol, lab, labels, offsets, lo, width, G, flags=SYM, mask=None, ws=None, ws_bytes=None, prefill=None, **over):
    """One hv_glcm on device tensors (3-D, or 4-D stacked) -> (return code, out [V][S][D][G][G], info [V][S][4] as numpy, the workspace).
    `over` replaces single arguments (refusal tests); prefill: the byte out and info hold before the call (default: the guards' 0xA5)."""
    lib, L = _lib()
    shape = tuple(int(s) for s in vol.shape)
    V, A = (shape[0], shape[1:]) if len(shape) == 4 else (1, shape)
    S, D = len(labels), len(offsets)
    a = dict(V=V, A0=A[0], A1=A[1], A2=A[2], S=S, D=D, G=G, vol_dtype=_VDT[vol.dtype], label_dtype=_LDT[lab.dtype])
    a.update({k: v for k, v in over.items() if k in a})
    a['G'] = over.get('levels', G)
    g_out, g_info = Guarded((V, max(S, 1), max(D, 1), G, G), torch.int64), Guarded((V, max(S, 1), TR.INFO), torch.int64)
    if prefill is not None:
        g_out.t.view(torch.uint8).fill_(prefill)
        g_info.t.view(torch.uint8).fill_(prefill)
    need = L.size('hv_glcm_workspace_bytes', V, *A, S, D, G)
    ws = ws or _Ws(max(need, 16), off=over.get('ws_off', 0))
    nul = ctypes.c_void_p(None)
    flat = [int(c) for d in offsets for c in d]
    rc = L.cdll.hv_glcm(
        nul if over.get('vol_null') else lib.ptr(vol), a['vol_dtype'], *_ll(_st4(vol)),
        nul if over.get('label_null') else lib.ptr(lab), a['label_dtype'], *_ll(_st4(lab)),
        lib.ptr(mask), *_ll(_st4(mask) if mask is not None else (0, 0, 0, 0)), a['V'], a['A0'], a['A1'], a['A2'],
        None if over.get('labels_null') else (ctypes.c_int * max(S, 1))(*labels), a['S'],
        None if over.get('offsets_null') else (ctypes.c_int * max(3 * D, 3))(*flat), a['D'],
        ctypes.c_double(lo), ctypes.c_double(width), a['G'], flags,
        nul if over.get('out_null') else ctypes.c_void_p(g_out.t.data_ptr() + over.get('out_off', 0)),
        nul if over.get('info_null') else ctypes.c_void_p(g_info.t.data_ptr() + over.get('info_off', 0)),
        nul if over.get('ws_null') else ws.ptr, ctypes.c_size_t(ws.need if ws_bytes is None else ws_bytes), lib.stream())
    torch.cuda.synchronize()
    assert g_out.intact() and g_info.intact() and ws.border_intact(), 'wrote outside a buffer'
    return rc, g_out.t.cpu().numpy().copy(), g_info.t.cpu().numpy().copy(), ws


def _same(out, info, ref, what=None):
    """Device (out [S][D][G][G], info [S][4]) against the reference pair, bit for bit."""
    r_out, r_info = ref
    assert out.shape == r_out.shape and out.dtype == np.int64 and info.dtype == np.int64
    assert info.tobytes() == r_info.tobytes(), (what, info, r_info)
    if out.tobytes() != r_out.tobytes():
        bad = np.argwhere(out != r_out)
        raise AssertionError((what, len(bad), bad[:5].tolist(), out[tuple(bad[0])], r_out[tuple(bad[0])]))


def _intensities(shape, dtype, seed=0):
    """Smooth plus noise, about -150 .. 650: both clamps of the default lo = -100, width = 20, G = 32 are met."""
    g = np.random.default_rng(seed)
    i, j, k = np.meshgrid(*(np.arange(n) for n in shape), indexing='ij')
    v = 250.0 + 150.0 * np.sin(i / 3.0) * np.cos(j / 4.0) + 100.0 * np.sin(k / 5.0) + g.standard_normal(shape) * 60.0
    dtype = np.dtype(dtype)
    if dtype == np.uint8:
        return np.clip(np.round(v / 3.0), 0, 255).astype(np.uint8)
    return np.round(v).astype(dtype) if dtype.kind == 'i' else v.astype(dtype)


def _labels2(shape, seed=0):
    """Label 1 over most of the volume, label 2 a slab that crosses the tile faces, label 3 scattered single voxels, the rest 0."""
    g = np.random.default_rng(100 + seed)
    lab = np.ones(shape, dtype=np.uint8)
    lab[:, shape[1] // 2:, :] = 2
    lab[g.random(shape) < 0.05] = 3
    lab[g.random(shape) < 0.05] = 0
    return lab


@functools.lru_cache(maxsize=None)
def _edge_case(dtype, seed=0):
    vol, lab = _intensities(EDGE, dtype, seed), _labels2(EDGE, seed)
    vol.setflags(write=False)
    lab.setflags(write=False)
    return vol, lab


LO, WIDTH = -100.0, 20.0


def _lo_width(dtype):
    return (0.0, 3.0) if np.dtype(dtype) == np.uint8 else (LO, WIDTH)


@functools.lru_cache(maxsize=None)
def _edge_ref(dtype, offsets, G=32, flags=SYM, seed=0, labels=(1, 2, 3)):
    vol, lab = _edge_case(dtype, seed)
    lo, width = _lo_width(dtype)
    out, info = TR.glcm_ref(vol, lab, labels, offsets, lo, width, G, bool(flags & SYM))
    out.setflags(write=False)
    info.setflags(write=False)
    return out, info


# ------------------------------------------------------------------------------------------------ the entry
def test_haralicks_example():
    vol = _dev(TR.HARALICK_IMAGE[:, :, None])
    lab = torch.ones((4, 4, 1), dtype=torch.uint8, device='cuda')
    rc, out, info, _ = _call(vol, lab, (1,), [(0, 1, 0)], 0.0, 1.0, 4)
    assert rc == 0 and (out[0, 0, 0] == TR.HARALICK_GLCM).all() and tuple(info[0, 0]) == (0, 16, 0, 0)
    rc, out, _, _ = _call(vol, lab, (1,), [(0, 1, 0)], 0.0, 1.0, 4, flags=0)
    assert rc == 0 and (out[0, 0, 0] + out[0, 0, 0].T == TR.HARALICK_GLCM).all() and out.sum() == 12


@pytest.mark.parametrize('shape', ((1, 1, 5), (5, 1, 1), (1, 1, 1)))
def test_degenerate_shapes(shape):
    """Most offsets have no pair at all here; the zero offset still gives the histogram."""
    vol = np.arange(int(np.prod(shape)), dtype=np.int16).reshape(shape) * 7
    lab = np.ones(shape, dtype=np.uint8)
    offs = D13 + [(0, 0, 0), (0, 0, -4), (-4, 0, 0)]
    rc, out, info, _ = _call(_dev(vol), _dev(lab), (1,), offs, 0.0, 5.0, 8)
    assert rc == 0
    _same(out[0], info[0], TR.glcm_ref(vol, lab, (1,), offs, 0.0, 5.0, 8))
    assert out[0, 0, 13].sum() == 2 * vol.size and out[0, 0, 14].sum() == (2 if shape == (1, 1, 5) else 0)


@pytest.mark.parametrize('negated', (False, True), ids=('d', 'minus-d'))
def test_tile_edges_all_directions(negated):
    """(17, 18, 33): pairs at distances 1 and 4 in all 13 directions (26 offsets, four passes of the LDS tables) cross every tile face, edge and
    corner; the negatives in a second call."""
    offs = tuple(tuple(-c for c in d) for d in D26) if negated else tuple(D26)
    vol, lab = _edge_case(np.int16)
    rc, out, info, _ = _call(_dev(vol), _dev(lab), (1, 2, 3), offs, LO, WIDTH, 32)
    assert rc == 0
    _same(out[0], info[0], _edge_ref(np.int16, offs))
    assert info[0, 0, 2] > 0 and info[0, 0, 3] > 0 and out[0, 0].min(axis=(1, 2)).shape == (26,) and (out[0, :2].sum(axis=(2, 3)) > 0).all()
    if negated:                                 # the matrix of -d is the transpose of d's: here both are symmetric already, so they are equal
        assert out[0].tobytes() == _edge_ref(np.int16, tuple(D26))[0].tobytes()


def test_negated_offsets_transpose_the_asymmetric_matrix():
    vol, lab = _edge_case(np.float32)
    neg = tuple(tuple(-c for c in d) for d in D13)
    rc, a, _, _ = _call(_dev(vol), _dev(lab), (1, 2, 3), D13, LO, WIDTH, 32, flags=0)
    rc2, b, _, _ = _call(_dev(vol), _dev(lab), (1, 2, 3), neg, LO, WIDTH, 32, flags=0)
    assert rc == 0 and rc2 == 0 and a.tobytes() == np.ascontiguousarray(b.swapaxes(-1, -2)).tobytes()
    assert a[0].tobytes() == _edge_ref(np.float32, tuple(D13), 32, 0)[0].tobytes() and (a[0, 0, 0] != a[0, 0, 0].T).any()


@pytest.mark.parametrize('ldtype', (np.uint8, np.float32, np.float64), ids=lambda d: 'label-' + np.dtype(d).name)
@pytest.mark.parametrize('dtype', VOL_DTYPES, ids=lambda d: np.dtype(d).name)
def test_dtype_pairs(dtype, ldtype):
    vol, lab = _edge_case(dtype)
    lo, width = _lo_width(dtype)
    rc, out, info, _ = _call(_dev(vol), _dev(lab.astype(ldtype)), (1, 2, 3), D13, lo, width, 32)
    assert rc == 0
    _same(out[0], info[0], _edge_ref(dtype, tuple(D13)))


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


@pytest.mark.parametrize('dtype', (np.int16, np.float32, np.float64), ids=lambda d: np.dtype(d).name)
def test_layouts_give_the_contiguous_bytes(dtype):
    vol, lab = _edge_case(dtype)
    mask = (np.random.default_rng(9).random(EDGE) > 0.1).astype(np.uint8)
    vols = _layouts(vol, np.nan if np.dtype(dtype).kind == 'f' else 99)
    labs = _layouts(lab.astype(np.float32) if dtype == np.float64 else lab, 255)
    masks = _layouts(mask, 1)
    offs = D13 + [(0, 0, 0), (-2, 3, -4)]
    rc, b_out, b_info, _ = _call(vols['c'], labs['c'], (1, 2, 3), offs, LO, WIDTH, 32, mask=masks['c'])
    assert rc == 0
    _same(b_out[0], b_info[0], TR.glcm_ref(vol, lab, (1, 2, 3), offs, LO, WIDTH, 32, True, mask))
    for name in vols:
        for other in ('c', name):
            rc, out, info, _ = _call(vols[name], labs[other], (1, 2, 3), offs, LO, WIDTH, 32, mask=masks[other])
            assert rc == 0 and out.tobytes() == b_out.tobytes() and info.tobytes() == b_info.tobytes(), (name, other)


@pytest.mark.parametrize('dtype', (np.int16, np.float64), ids=lambda d: np.dtype(d).name)
def test_batch_equals_single_calls(dtype):
    cases = [_edge_case(dtype, seed) for seed in (0, 1, 2)]
    singles = [_call(_dev(v), _dev(l), (1, 2, 3), D13, LO, WIDTH, 32) for v, l in cases]
    assert all(rc == 0 for rc, _, _, _ in singles)
    _same(singles[0][1][0], singles[0][2][0], _edge_ref(dtype, tuple(D13)))
    for order in ((0, 1, 2), (2, 1, 0)):
        rc, out, info, _ = _call(_dev(np.stack([cases[i][0] for i in order])), _dev(np.stack([cases[i][1] for i in order])), (1, 2, 3), D13,
                                 LO, WIDTH, 32)
        assert rc == 0
        for n, i in enumerate(order):
            assert out[n].tobytes() == singles[i][1][0].tobytes() and info[n].tobytes() == singles[i][2][0].tobytes(), (order, i)


def test_two_labels_meeting_at_a_plane():
    """No pair across the plane is counted in either slot: each slot's matrix is that of its own half alone."""
    shape = (6, 20, 7)
    vol = _intensities(shape, np.int16, 4)
    lab = np.ones(shape, dtype=np.uint8)
    lab[:, 16:, :] = 2                           # the plane is a tile face as well
    rc, out, info, _ = _call(_dev(vol), _dev(lab), (1, 2), D13, LO, WIDTH, 16)
    assert rc == 0
    _same(out[0], info[0], TR.glcm_ref(vol, lab, (1, 2), D13, LO, WIDTH, 16))
    for s, half in enumerate((np.s_[:, :16, :], np.s_[:, 16:, :])):
        alone, _ = TR.glcm_ref(vol[half], np.ones(vol[half].shape, np.uint8), (1,), D13, LO, WIDTH, 16)
        assert out[0, s].tobytes() == alone[0].tobytes(), s
    whole, _ = TR.glcm_ref(vol, np.ones(shape, np.uint8), (1,), D13, LO, WIDTH, 16)
    assert whole.sum() > out[0].sum()


def test_a_mask_removes_exactly_the_pairs_through_its_voxel():
    shape = (5, 17, 6)
    vol = _intensities(shape, np.float32, 2)
    lab = np.ones(shape, dtype=np.uint8)
    mask = np.ones(shape, dtype=np.uint8)
    p = (2, 15, 3)
    mask[p] = 0
    offs = D13 + [(0, 0, 0)]
    rc, full, _, _ = _call(_dev(vol), _dev(lab), (1,), offs, LO, WIDTH, 32, flags=0)
    rc2, out, info, _ = _call(_dev(vol), _dev(lab), (1,), offs, LO, WIDTH, 32, flags=0, mask=_dev(mask))
    assert rc == 0 and rc2 == 0 and info[0, 0, 1] == vol.size - 1
    lev = TR.levels_of(vol, LO, WIDTH, 32)[0]
    gone = np.zeros_like(full[0, 0])
    for n, d in enumerate(offs):
        q, r = tuple(a + b for a, b in zip(p, d)), tuple(a - b for a, b in zip(p, d))
        if all(0 <= c < e for c, e in zip(q, shape)):
            gone[n, lev[p], lev[q]] += 1
        if d != (0, 0, 0) and all(0 <= c < e for c, e in zip(r, shape)):
            gone[n, lev[r], lev[p]] += 1
    assert (full[0, 0] - out[0, 0]).tobytes() == gone.tobytes()


def test_zero_offset_is_the_histogram_and_agrees_with_label_statistics():
    import hvgan  # noqa: F401
    from hvgan import label_statistics
    vol, lab = _edge_case(np.float64)
    mask = (np.random.default_rng(11).random(EDGE) > 0.3).astype(np.uint8)
    rc, out, info, _ = _call(_dev(vol), _dev(lab), (2, 1), [(0, 0, 0)], LO, WIDTH, 32, flags=0, mask=_dev(mask))
    assert rc == 0
    lev = TR.levels_of(vol, LO, WIDTH, 32)[0]
    stats = label_statistics.label_statistics(_dev(vol), _dev(lab), (2, 1), mask=_dev(mask))
    for s, l in enumerate((2, 1)):
        hist = np.bincount(lev[(lab == l) & (mask != 0)], minlength=32)
        assert (np.diagonal(out[0, s, 0]) == hist).all() and out[0, s, 0].sum() == hist.sum() == stats['count'][s] == info[0, s, 1]


@pytest.mark.parametrize('flags', (0, SYM), ids=('asymmetric', 'symmetric'))
def test_contention_and_counter_width(flags):
    """A constant 40^3 volume puts every pair of an offset into one bin: it must hold exactly the number of pairs.  Then uniform random levels."""
    A = 40
    lab = np.ones((A, A, A), dtype=np.uint8)
    const = np.full((A, A, A), 503, dtype=np.int16)
    rc, out, info, _ = _call(_dev(const), _dev(lab), (1,), D26, 0.0, 8.0, 64, flags=flags)
    assert rc == 0 and tuple(info[0, 0]) == (0, A ** 3, 0, 0)
    b = 503 // 8
    for n, d in enumerate(D26):
        want = (A - abs(d[0])) * (A - abs(d[1])) * (A - abs(d[2])) * (2 if flags else 1)
        assert out[0, 0, n, b, b] == want and out[0, 0, n].sum() == want, (d, out[0, 0, n, b, b], want)
    rand = np.random.default_rng(6).integers(0, 512, (A, A, A)).astype(np.int16)
    rc, out, info, _ = _call(_dev(rand), _dev(lab), (1,), D26, 0.0, 8.0, 64, flags=flags)
    assert rc == 0
    _same(out[0], info[0], TR.glcm_ref(rand, lab, (1,), D26, 0.0, 8.0, 64, bool(flags)))


def test_s1_s64_g2_g64_d1_d26():
    shape = (16, 8, 17)
    vol = _intensities(shape, np.int16, 7)
    i, j, _ = np.indices(shape)
    lab = ((i // 2) * 8 + j).astype(np.uint8)                           # 64 labels of 2 x 1 x 17 voxels, label 0 among them
    many = tuple(range(63, -1, -1))
    for labels, offs, G in ((many, D26, 2), (many, [(1, 0, 0)], 64), ((5,), D26, 64), ((5,), [(0, 0, 1)], 2), (many, D13, 32)):
        rc, out, info, _ = _call(_dev(vol), _dev(lab), labels, offs, LO, WIDTH * 32 / G, G)
        assert rc == 0
        _same(out[0], info[0], TR.glcm_ref(vol, lab, labels, offs, LO, WIDTH * 32 / G, G), (len(labels), len(offs), G))
        assert (info[0, :, 1] == 34).all()


def test_quantisation_edges():
    """Values exactly on bin edges, below lo, at and above lo + G * width, -0.0; 0.1 is no binary fraction, so k * 0.1 / 0.1 lands on either side of
    k: the device's division must give numpy's bits.  int16 with lo = -1000, width = 25."""
    G = 16
    k = np.arange(-3, 2 * G + 3)
    edges = np.concatenate([k * 0.1, np.nextafter(k * 0.1, np.inf), np.nextafter(k * 0.1, -np.inf), k / 10.0, [-0.0, 0.0, 1.6, 1.6000000000000003, 1e300,
                            -1e300, 5e-324]])
    vol = np.resize(edges, (4, 6, 20)).astype(np.float64)
    lab = np.ones(vol.shape, dtype=np.uint8)
    offs = [(0, 0, 0), (0, 0, 1), (1, 1, -1)]
    rc, out, info, _ = _call(_dev(vol), _dev(lab), (1,), offs, 0.0, 0.1, G)
    assert rc == 0
    ref = TR.glcm_ref(vol, lab, (1,), offs, 0.0, 0.1, G)
    _same(out[0], info[0], ref)
    t = vol / 0.1
    assert info[0, 0, 2] == (t < 0).sum() > 0 and info[0, 0, 3] == (t >= G).sum() > 0 and info[0, 0, 1] == vol.size
    rc, out, info, _ = _call(_dev(vol), _dev(lab), (1,), offs, 0.30000000000000004, 0.1, G, flags=0)           # a lo that is no bin edge of 0
    assert rc == 0
    _same(out[0], info[0], TR.glcm_ref(vol, lab, (1,), offs, 0.30000000000000004, 0.1, G, False))
    g = np.random.default_rng(8)
    hu = g.integers(-1100, 700, (4, 6, 20)).astype(np.int16)
    hu[0, 0, :8] = (-1001, -1000, -999, -976, -975, 599, 600, 601)
    rc, out, info, _ = _call(_dev(hu), _dev(lab), (1,), offs, -1000.0, 25.0, 64)
    assert rc == 0
    _same(out[0], info[0], TR.glcm_ref(hu, lab, (1,), offs, -1000.0, 25.0, 64))
    assert info[0, 0, 2] == (hu < -1000).sum() > 0 and info[0, 0, 3] == (hu >= 600).sum() > 0


@pytest.mark.parametrize('dtype', (np.float32, np.float64), ids=lambda d: np.dtype(d).name)
def test_non_finite_inside_a_label_marks_that_slot_only(dtype):
    vol, lab = _edge_case(dtype)
    bad = vol.copy()
    spots = [(3, 2, 15), (16, 1, 16), (8, 5, 32)]                       # inside label 1 unless scattered away: forced below
    l2 = lab.copy()
    for p, x in zip(spots, (np.nan, np.inf, -np.inf)):
        bad[p], l2[p] = x, 1
    bad[0, 17, 0], l2[0, 17, 0] = np.nan, 0                            # label 0 is not listed: nobody's business
    rc, base, b_info, _ = _call(_dev(vol), _dev(l2), (1, 2, 3), D13, LO, WIDTH, 32)
    rc2, out, info, _ = _call(_dev(bad), _dev(l2), (1, 2, 3), D13, LO, WIDTH, 32)
    assert rc == 0 and rc2 == 0
    _same(out[0], info[0], TR.glcm_ref(bad, l2, (1, 2, 3), D13, LO, WIDTH, 32))
    assert out[0, 1:].tobytes() == base[0, 1:].tobytes() and info[0, 1:].tobytes() == b_info[0, 1:].tobytes()
    assert info[0, 0, 0] == LR.NONFINITE and info[0, 0, 1] == b_info[0, 0, 1] - 3 and (info[0, 1:, 0] == 0).all()
    mask = np.ones(EDGE, dtype=np.uint8)
    for p in spots:
        mask[p] = 0                              # a non-finite voxel is absent from every pair: the same matrix as with the voxel masked out
    rc, masked, m_info, _ = _call(_dev(vol), _dev(l2), (1, 2, 3), D13, LO, WIDTH, 32, mask=_dev(mask))
    assert rc == 0 and masked.tobytes() == out.tobytes() and m_info[0, 0, 0] == 0


@pytest.mark.parametrize('ldtype', (np.float32, np.float64), ids=lambda d: np.dtype(d).name)
def test_a_value_that_is_no_label_sets_the_status_bit(ldtype):
    vol, lab = _edge_case(np.int16)
    for value in (2.5, 300.0, -1.0, np.nan):
        l = lab.astype(ldtype)
        l[3, 4, 6] = value
        rc, out, info, _ = _call(_dev(vol), _dev(l), (1, 2, 3), D13[:3], LO, WIDTH, 32)
        assert rc == 0
        _same(out[0], info[0], TR.glcm_ref(vol, l, (1, 2, 3), D13[:3], LO, WIDTH, 32))
        assert (info[0, :, 0] & LR.BAD_LABEL).all()


def test_an_absent_label_is_empty():
    vol, lab = _edge_case(np.int16)
    rc, out, info, _ = _call(_dev(vol), _dev(lab), (9, 1), D13, LO, WIDTH, 32)
    assert rc == 0 and tuple(info[0, 0]) == (LR.EMPTY, 0, 0, 0) and not out[0, 0].any() and out[0, 1].any() and info[0, 1, 0] == 0


@pytest.mark.parametrize('dtype', (np.uint8, np.float64), ids=lambda d: np.dtype(d).name)
def test_same_bytes_twice_and_on_poisoned_buffers(dtype):
    vol, lab = _edge_case(dtype)
    lo, width = _lo_width(dtype)
    dv, dl = _dev(vol), _dev(lab)
    rc, first, i1, ws = _call(dv, dl, (1, 2, 3), D26, lo, width, 32)
    rc2, second, i2, _ = _call(dv, dl, (1, 2, 3), D26, lo, width, 32, ws=ws)                    # the workspace as the first call left it
    rc3, third, i3, _ = _call(dv, dl, (1, 2, 3), D26, lo, width, 32, ws=_Ws(ws.need, fill=0xFF), prefill=0xFF)
    assert rc == 0 and rc2 == 0 and rc3 == 0
    assert first.tobytes() == second.tobytes() == third.tobytes() and i1.tobytes() == i2.tobytes() == i3.tobytes()
    _same(first[0], i1[0], _edge_ref(dtype, tuple(D26)))


def test_refusals_write_nothing():
    vol, lab = _edge_case(np.float32)
    dv, dl = _dev(vol), _dev(lab)
    L = _lib()[1]
    need = L.size('hv_glcm_workspace_bytes', 1, *EDGE, 2, 2, 8)
    assert need > 0
    nan, inf = float('nan'), float('inf')
    cases = [
        (dict(vol_null=1), ERR_ARG), (dict(label_null=1), ERR_ARG), (dict(labels_null=1), ERR_ARG), (dict(offsets_null=1), ERR_ARG),
        (dict(out_null=1), ERR_ARG), (dict(info_null=1), ERR_ARG), (dict(ws_null=1), ERR_ARG),
        (dict(V=0), ERR_ARG), (dict(A0=0), ERR_ARG), (dict(A1=-1), ERR_ARG), (dict(A2=0), ERR_ARG),
        (dict(vol_dtype=2), ERR_ARG), (dict(vol_dtype=7), ERR_ARG), (dict(label_dtype=6), ERR_ARG), (dict(label_dtype=-1), ERR_ARG),
        (dict(S=0), ERR_ARG), (dict(S=65), ERR_ARG), (dict(D=0), ERR_ARG), (dict(D=27), ERR_ARG), (dict(levels=1), ERR_ARG), (dict(levels=65), ERR_ARG),
        (dict(offsets=((0, 0, 5), (0, 1, 0))), ERR_ARG), (dict(offsets=((0, 1, 0), (-5, 0, 0))), ERR_ARG),
        (dict(offsets=((1, -1, 0), (1, -1, 0))), ERR_ARG),
        (dict(lo=nan), ERR_ARG), (dict(lo=inf), ERR_ARG), (dict(width=nan), ERR_ARG), (dict(width=inf), ERR_ARG), (dict(width=0.0), ERR_ARG),
        (dict(width=-1.0), ERR_ARG), (dict(flags=2), ERR_ARG), (dict(flags=-1), ERR_ARG),
        (dict(out_off=4), ERR_ARG), (dict(info_off=4), ERR_ARG), (dict(ws_off=8), ERR_ARG), (dict(ws_bytes=need - 1), ERR_ARG),
        (dict(labels=(1, 1)), ERR_ARG), (dict(labels=(1, 256)), ERR_ARG), (dict(labels=(-1, 2)), ERR_ARG),
        (dict(A0=1 << 11, A1=1 << 10, A2=(1 << 9) + 1), ERR_UNSUPPORTED), (dict(V=65536), ERR_UNSUPPORTED),
    ]
    for over, code in cases:
        over = dict(over)
        labels, offs = over.pop('labels', (1, 2)), over.pop('offsets', ((0, 0, 1), (1, 0, 0)))
        lo, width, flags = over.pop('lo', 0.0), over.pop('width', 10.0), over.pop('flags', SYM)
        ws = _Ws(need, off=over.get('ws_off', 0))
        rc, out, info, ws = _call(dv, dl, labels, offs, lo, width, 8, flags=flags, ws=ws, ws_bytes=over.pop('ws_bytes', None), **over)
        assert rc == code, (over, labels, offs, lo, width, flags, rc)
        sentinel = np.frombuffer(b'\xa5' * 8, dtype=np.int64)[0]
        assert (out == sentinel).all() and (info == sentinel).all() and ws.untouched(), (over, labels, offs, lo, width, flags)
    for bad in ((0, 4, 4, 4, 1, 1, 8), (1, 4, 4, 4, 0, 1, 8), (1, 4, 4, 4, 65, 1, 8), (1, 4, 4, 4, 1, 0, 8), (1, 4, 4, 4, 1, 27, 8),
                (1, 4, 4, 4, 1, 1, 1), (1, 4, 4, 4, 1, 1, 65), (1, 1 << 11, 1 << 10, (1 << 9) + 1, 1, 1, 8), (65536, 4, 4, 4, 1, 1, 8)):
        assert L.size('hv_glcm_workspace_bytes', *bad) == 0, bad


# ------------------------------------------------------------------------------------------------ the module
def test_glcm_on_host_arrays_and_resident_tensors(monkeypatch):
    T = _T()
    vol, lab = _edge_case(np.int16)
    mask = (np.random.default_rng(12).random(EDGE) > 0.2)
    offs = D13[:4] + [(0, 0, 0)]
    r_out, r_info = TR.glcm_ref(vol, lab, (1, 2, 3), offs, LO, WIDTH, 16, True, mask)
    exact = ExactWs(monkeypatch, required=True)
    res_dev = T.glcm(_dev(vol), _dev(lab), (1, 2, 3), offs, 16, LO, WIDTH, mask=_dev(mask))
    res_host = T.glcm(np.array(vol), np.array(lab), (1, 2, 3), offs, 16, LO, WIDTH, mask=mask)
    exact.close()
    for res in (res_dev, res_host):
        assert res['matrices'].dtype == np.int64 and res['matrices'].shape == (3, 5, 16, 16) and res['matrices'].tobytes() == r_out.tobytes()
        assert list(res['labels']) == [1, 2, 3] and res['offsets'].tolist() == [list(d) for d in offs]
        for k, col in (('status', 0), ('count', 1), ('clamped_low', 2), ('clamped_high', 3)):
            assert res[k].shape == (3,) and (res[k] == r_info[:, col]).all(), k
    auto = T.glcm(_dev(vol), _dev(lab), levels=16, lo=LO, width=WIDTH, symmetric=False)             # labels=None, the 13 directions
    a_out, _ = TR.glcm_ref(vol, lab, (1, 2, 3), D13, LO, WIDTH, 16, False)
    assert list(auto['labels']) == [1, 2, 3] and auto['matrices'].tobytes() == a_out.tobytes()
    stacked = T.glcm(_dev(np.stack([vol, vol])), _dev(np.stack([lab, np.zeros_like(lab)])), (1, 7), offs, 16, LO, WIDTH)
    assert stacked['matrices'].shape == (2, 2, 5, 16, 16) and stacked['matrices'][0, 0].tobytes() == r_out_unmasked(vol, lab, offs).tobytes()
    assert not stacked['matrices'][1].any() and (stacked['status'][1] == LR.EMPTY).all() and stacked['count'].tolist()[1] == [0, 0]


def r_out_unmasked(vol, lab, offs):
    return TR.glcm_ref(vol, lab, (1,), offs, LO, WIDTH, 16, True)[0][0]


def test_vertebra_texture_is_glcm_under_scipys_erosion():
    from scipy import ndimage
    T = _T()
    sp = (0.7, 0.7, 1.5)
    vol, _ = _edge_case(np.float32)
    lab = np.zeros(EDGE, dtype=np.uint8)
    lab[2:15, 1:17, 3:30] = 1
    dv, dl = _dev(vol), _dev(lab)
    for r in (0.0, 1.6):
        got = T.vertebra_texture(dv, dl, 1, erode_mm=r, spacing=sp, levels=16, lo=LO, width=2 * WIDTH, distance=2)
        mask = ndimage.binary_erosion(lab == 1, MR.ball(r, sp), border_value=0).astype(np.uint8) if r else None
        want = T.glcm(dv, dl, (1,), T.directions(2), 16, LO, 2 * WIDTH, mask=None if mask is None else _dev(mask))
        ref, _ = TR.glcm_ref(vol, lab, (1,), T.directions(2).tolist(), LO, 2 * WIDTH, 16, True, mask)
        assert got['matrices'].tobytes() == want['matrices'][0].tobytes() == ref[0].tobytes() and got['matrices'].any()
        assert got['count'] == want['count'][0] == int((lab == 1).sum() if mask is None else (mask != 0).sum()) and got['label'] == 1
        feats = T.haralick_features(ref[0])
        for k in T.FEATURES:
            assert np.allclose(got['features'][k], feats[k], rtol=1e-12, atol=1e-12) and abs(got['features']['mean'][k] - feats['mean'][k]) <= 1e-12, k
    med = T.vertebra_texture(dv, dl, 1, levels=16, lo=LO, width=2 * WIDTH, median_size=3)
    filtered = ndimage.median_filter(vol, size=3, mode='reflect')
    assert med['matrices'].tobytes() == TR.glcm_ref(filtered, lab, (1,), D13, LO, 2 * WIDTH, 16)[0][0].tobytes()


@pytest.mark.parametrize('same_strides', (True, False))
def test_texture_comparison_of_a_constant_against_a_checkerboard(same_strides, monkeypatch):
    """The original vertebra is constant (one bin: contrast 0, homogeneity 1, asm 1, entropy 0, correlation 1), the synthesized one a 3-D
    checkerboard of two levels: along the three axes every pair joins the two levels ([[0, n], [n, 0]]: contrast 1, asm 0.5, entropy 1 bit,
    correlation -1).  One V = 2 batch when the strides agree, two calls when they do not: the same result."""
    T = _T()
    shape = (12, 20, 18)
    lab = np.zeros(shape, dtype=np.uint8)
    lab[1:11, 2:18, 1:9], lab[1:11, 2:18, 10:17] = 21, 22
    i, j, k = np.indices(shape)
    ct = np.full(shape, 120, dtype=np.int16)
    ct[lab == 22] = (100 + 50 * ((i + j) % 2))[lab == 22]               # the neighbour: stripes, contrast along two axes of three
    synth = np.where((i + j + k) % 2 == 0, 100, 150).astype(np.int16)
    axes = [(1, 0, 0), (0, 1, 0), (0, 0, 1)]
    d_ct, d_lab = _dev(ct), _dev(lab)
    d_syn = _dev(synth) if same_strides else _dev(synth.transpose(2, 0, 1)).permute(1, 2, 0)
    calls = []
    real = T._launch
    monkeypatch.setattr(T, '_launch', lambda *a: (calls.append(int(a[0].shape[0])), real(*a))[1])
    exact = ExactWs(monkeypatch, required=True)
    res = T.texture_comparison(d_ct, d_syn, d_lab, _dev(lab), 21, neighbours=(22,), levels=2, lo=100.0, width=25.0, offsets=axes)
    exact.close()
    assert calls == ([2] if same_strides else [1, 1])
    closed = {'original': dict(contrast=0.0, homogeneity=1.0, asm=1.0, entropy=0.0, correlation=1.0),
              'synthesized': dict(contrast=1.0, homogeneity=0.5, asm=0.5, entropy=1.0, correlation=-1.0)}
    for who, want in closed.items():
        for k, x in want.items():
            assert (res[who]['features'][k] == x).all() and res[who]['features']['mean'][k] == x, (who, k)
    for k in closed['original']:
        assert res['difference'][k] == closed['synthesized'][k] - closed['original'][k], k
    n = 10 * 16 * 8
    assert res['original']['count'] == res['synthesized']['count'] == n and res['original']['matrices'][0, 0, 0] == 2 * 9 * 16 * 8
    assert res['synthesized']['matrices'][2].tolist() == [[0, 10 * 16 * 7], [10 * 16 * 7, 0]]
    nb = res['neighbours'][22]
    assert nb['features']['contrast'].tolist() == [1.0, 1.0, 0.0] and res['neighbour_difference'][22]['contrast'] == 1.0 - 2.0 / 3.0
    one = T.vertebra_texture(d_syn, _dev(lab), 21, levels=2, lo=100.0, width=25.0, offsets=axes)
    assert one['matrices'].tobytes() == res['synthesized']['matrices'].tobytes()
    eroded = T.texture_comparison(d_ct, d_syn, d_lab, _dev(lab), 21, neighbours=(22,), erode_mm=1.0, levels=2, lo=100.0, width=25.0, offsets=axes)
    assert eroded['original']['count'] == 8 * 14 * 6 and eroded['difference']['contrast'] == 1.0


def test_misuse_raises():
    T = _T()
    vol, lab = _edge_case(np.int16)
    dv, dl = _dev(vol), _dev(lab)
    with pytest.raises(ValueError):
        T.glcm(torch.from_numpy(vol.copy()), dl, (1,))                 # a CPU tensor: nothing is counted on the host
    with pytest.raises(TypeError):
        T.glcm(vol.tolist(), dl, (1,))
    with pytest.raises(TypeError):
        T.glcm(dv.to(torch.int32), dl, (1,))
    with pytest.raises(ValueError):
        T.glcm(dv, dl[:, :, 1:], (1,))
    with pytest.raises(ValueError):
        T.glcm(dv, dl, (1, 1))
    with pytest.raises(ValueError):
        T.glcm(dv, dl, (1,), levels=65)
    with pytest.raises(ValueError):
        T.glcm(dv, dl, (1,), offsets=[(0, 0, 5)])
    with pytest.raises(ValueError):
        T.glcm(dv, dl, (1,), width=0.0)
    with pytest.raises(ValueError):
        T.glcm(dv, torch.zeros_like(dl))                                # labels=None and nothing present
    with pytest.raises(ValueError):
        T.vertebra_texture(dv[None], dl[None], 1)
    with pytest.raises(TypeError):
        T.texture_comparison(dv, dv.to(torch.float32), dl, dl, 1)
