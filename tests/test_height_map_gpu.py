"""Per-column height-loss maps and profiles on the device (hv_rhlv_maps / hv_rhlv_maps_batch through hvgan.evaluation) against the float64
restatement tests/height_map_ref.py, which tests/test_height_map_cpu.py pins to the reference's own per-slice arrays (fixture G16).
Column counts, thirds, selections and the heights of the original are integers: exact.  A generated height is one float64 product and a
loss one quotient of the reference's own operations; a profile is a sum of at most a few hundred such heights in ascending order on both
sides: 1e-12 relative with a floor of 1, the tolerance of every RHLV double.  The shapes are the smallest that reach every path: columns
below and above the 256 lanes of a block (the stride loop and its tail), Z != W, both memory layouts of the counting kernels."""
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden
import height_map_ref as M

pytestmark = pytest.mark.gpu
TOL = 1e-12
VIEWS = ('sagittal', 'coronal')
MAPS = ('loss', 'height_fake', 'height_label')
PROFILES = ('profile_fake', 'profile_label', 'curve', 'slice_profile_fake', 'slice_profile_label', 'slice_curve')
SHAPES = {'small': (24, 37, 19), 'wide': (8, 300, 21)}
IDX, DIV, THR = 20, 2, (0.64, 0.7)


def _close(a, b):
    """Same NaN positions, and 1e-12 relative (floor 1) elsewhere."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(b)
    return bool(np.all(np.abs(a[ok] - b[ok]) <= TOL * np.maximum(1.0, np.abs(b[ok]))))


def _bits(t):
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _volumes(shape, seed=0):
    """uint8 id volumes [H, W, Z]: columns of vertebra IDX standing on row 0, the original wedge-shaped along w, the generated one shorter than the
    original on every fourth z (a rescale ratio applies there), ragged ends along both axes, another id on the top row."""
    H, W, Z = SHAPES[shape]
    rng = np.random.default_rng(1000 + seed + W)
    w, z = np.meshgrid(np.arange(W), np.arange(Z), indexing='ij')
    w0, w1 = W // 6, W - W // 8
    inside = (w >= w0 + z % 3) & (w < w1 - z % 2) & (z >= 2) & (z < Z - 2)
    hl = np.rint(H * (0.3 + 0.45 * (w - w0) / (w1 - w0))).astype(int) + rng.integers(-1, 2, (W, Z))
    hf = int(round(H * 0.8)) + rng.integers(-1, 2, (W, Z)) - (z % 4 == 0) * (H // 2)
    rows = np.arange(H)[:, None, None]
    vols = []
    for h in (hf, hl):
        v = ((rows < np.clip(h, 1, H - 1)[None]) & inside[None]).astype(np.uint8) * IDX
        v[H - 1] = IDX + 1
        vols.append(v)
    return vols[0], vols[1]


@functools.lru_cache(maxsize=None)
def _reference(shape, view):
    """The restatement's maps of a shape; checks that the inputs reach what they are meant to: slices with and without a rescale ratio."""
    fake, label = _volumes(shape)
    m = M.view_maps(fake, label, IDX, DIV, THR[VIEWS.index(view)], view)
    if view == 'sagittal':
        hf = m['height_fake'][m['flags'][:, 0] & M.VISITED != 0]
        scaled = np.any(hf != np.round(hf), axis=1)
        assert scaled.any() and not scaled.all(), shape
    return m


def _layout(v, layout, dtype):
    """A numpy id volume -> a device tensor [H, W, Z] of the given dtype in one of three memory layouts."""
    t = torch.from_numpy(v).to(dtype).cuda()
    if layout == 'zfast':
        t = t.contiguous()
        assert t.stride(2) == 1
    elif layout == 'wfast':
        t = t.permute(0, 2, 1).contiguous().permute(0, 2, 1)
        assert t.stride(1) == 1 and t.stride(2) != 1
    else:                                                   # a strided window of a larger tensor
        H, W, Z = t.shape
        big = torch.full((H + 3, W + 2, 2 * Z + 1), float(IDX), dtype=dtype, device='cuda')
        big[1:H + 1, 1:W + 1, 1::2] = t
        t = big[1:H + 1, 1:W + 1, 1::2]
        assert not t.is_contiguous() and t.stride(2) == 2
    return t


def _check_view(got, ref, what):
    assert got['range'] == ref['range'], (what, got['range'], ref['range'])
    flags = got['flags'].cpu().numpy()
    assert flags.dtype == np.uint8 and np.array_equal(flags, ref['flags']), what
    assert np.array_equal(got['height_label'].cpu().numpy(), ref['height_label']), what
    for k in MAPS + PROFILES:
        assert got[k].dtype == torch.float64 and got[k].is_cuda
        assert _close(got[k].cpu().numpy(), ref[k]), (what, k)
    S, C = ref['flags'].shape
    assert got['loss'].shape == (S, C) and got['curve'].shape == (C,) and got['slice_curve'].shape == (S,)


@pytest.mark.parametrize('dtype', [torch.uint8, torch.float32], ids=['uint8', 'float32'])
@pytest.mark.parametrize('layout', ['zfast', 'wfast', 'window'])
@pytest.mark.parametrize('shape', sorted(SHAPES))
def test_maps_match_the_restatement(shape, layout, dtype):
    import hvgan  # noqa: F401
    from hvgan import evaluation
    fake, label = _volumes(shape)
    f, l = _layout(fake, layout, dtype), _layout(label, layout, dtype)
    got = evaluation.height_loss_map(f, l, IDX, DIV, THR)
    assert set(got) == {'sagittal', 'coronal', 'records'} and got['records'].shape == (2, 16)
    for view in VIEWS:
        ref = _reference(shape, view)
        assert ref['flags'].any() and (ref['flags'] & M.VISITED == 0).any() and not ref['raises']
        _check_view(got[view], ref, (shape, layout, view))
    # the records are hv_rhlv_views' own, bit for bit
    rec = evaluation._run_views(f, l, float(IDX), evaluation.SAGITTAL | evaluation.CORONAL, DIV, evaluation.INT_MIN, 0, THR).cpu().numpy()
    assert np.array_equal(got['records'].view(np.int64), rec.view(np.int64))
    # the selected heights of a whole map average to the means the records carry (all_height_fake, all_height_label)
    for v, view in enumerate(VIEWS):
        fl = got[view]['flags']
        for bit, k, col in ((evaluation.FLAG_SEL_FAKE, 'height_fake', 5), (evaluation.FLAG_SEL_LABEL, 'height_label', 6)):
            sel = (fl & bit) != 0
            mean = float(got[view][k][sel].sum().cpu()) / int(sel.sum().cpu())
            assert abs(mean - rec[v, col]) <= TOL * max(1.0, abs(rec[v, col])), (view, k, mean, rec[v, col])
            assert rec[v, col] > 0


def test_null_outputs_are_skipped_and_the_rest_keeps_its_bits():
    """Through the C entry: only `loss` and `column_profile` of the sagittal view asked for, nothing of the coronal view (a NULL struct).  What is
    asked for has the bits of the full call, what is not is left untouched, the records are the same."""
    import ctypes
    import hvgan  # noqa: F401
    from hvgan import evaluation, lib
    assert SHAPES['wide'][1] > 256 and SHAPES['small'][1] % 64 and all(s[1] != s[2] for s in SHAPES.values())
    L = lib.get()
    fake, label = _volumes('wide')
    f, l = _layout(fake, 'zfast', torch.uint8), _layout(label, 'zfast', torch.uint8)
    H, W, Z = f.shape
    both = evaluation.SAGITTAL | evaluation.CORONAL
    full_rec, full, _ = evaluation._run_maps(f, l, float(IDX), both, DIV, evaluation.INT_MIN, 0, THR)
    loss = torch.full((Z, W), 7.0, dtype=torch.float64, device='cuda')
    colp = torch.full((3, W), 7.0, dtype=torch.float64, device='cuda')
    out = torch.zeros(2, 16, dtype=torch.float64, device='cuda')
    ws, _ = evaluation.ops._ws(L.size('hv_rhlv_maps_workspace_bytes', W, Z, both, 1), f.device, slot=3)
    sag, cor = evaluation._view_args(L, both, DIV, evaluation.INT_MIN, 0, THR)
    want = L.hv_rhlv_map_out(loss.data_ptr(), None, None, None, colp.data_ptr(), None, None)
    L.call('hv_rhlv_maps', lib.ptr(f), lib.ptr(l), *evaluation._geometry(f), ctypes.c_float(float(IDX)), both, sag, cor, ctypes.byref(want), None,
           lib.ptr(out), lib.ptr(ws), ctypes.c_size_t(ws.numel()), lib.stream())
    assert _same_bits(loss, full['sagittal']['loss'][0]) and _same_bits(colp, full['sagittal']['column_profile'][0])
    assert _same_bits(out, full_rec)
    assert not bool(torch.isnan(colp).all()) and not bool((loss == 7.0).any())


@pytest.mark.parametrize('shape', sorted(SHAPES))
def test_each_view_alone_is_the_same_bits(shape):
    import hvgan  # noqa: F401
    from hvgan import evaluation
    fake, label = _volumes(shape)
    f, l = _layout(fake, 'zfast', torch.uint8), _layout(label, 'zfast', torch.uint8)
    both = evaluation.height_loss_map(f, l, IDX, DIV, THR)
    for v, view in enumerate(VIEWS):
        one = evaluation.height_loss_map(f, l, IDX, DIV, THR[v], views=(view,))
        assert set(one) == {view, 'records'} and one['records'].shape == (1, 16)
        assert np.array_equal(one['records'][0].view(np.int64), both['records'][v].view(np.int64))
        assert one[view]['range'] == both[view]['range']
        for k in MAPS + PROFILES + ('flags',):
            assert _same_bits(one[view][k], both[view][k]), (view, k)
    with pytest.raises(ValueError):
        evaluation.height_loss_map(f, l, IDX, DIV, THR, views=('axial',))


def test_absent_vertebra_and_coronal_raise():
    import hvgan  # noqa: F401
    from hvgan import evaluation
    fake, label = _volumes('small')
    f, l = torch.from_numpy(fake).cuda(), torch.from_numpy(label).cuda()
    assert evaluation.height_loss_map(f, l, 33) is None and M.view_maps(fake, label, 33) is None
    assert evaluation.height_loss_map(f, l, 33, views='coronal') is None
    # the generated vertebra two columns wide in the coronal view: the coronal script raises, the sagittal one does not
    g = {k: np.asarray(v) for k, v in load_golden('g16_height_map').items()}
    assert g['narrow/coronal/raises'] and not g['narrow/sagittal/raises']
    idx, div, thr = (float(v) for v in g['narrow/params'])
    f, l = torch.from_numpy(g['narrow/fake']).cuda(), torch.from_numpy(g['narrow/label']).cuda()
    with pytest.raises(ValueError, match='coronal'):
        evaluation.height_loss_map(f, l, idx, int(div), thr)
    with pytest.raises(ValueError, match='coronal'):
        evaluation.height_loss_map(f, l, idx, int(div), thr, views=('coronal',))
    got = evaluation.height_loss_map(f, l, idx, int(div), thr, views=('sagittal',))
    _check_view(got['sagittal'], M.view_maps(g['narrow/fake'], g['narrow/label'], idx, int(div), thr, 'sagittal'), 'narrow')
    # the batched form records the flag and still delivers the rows
    res = evaluation.height_loss_dataset([f], [l], [idx], int(div), thr)
    assert res['present'][0] and res['records'][0, 1, 14] == 1.0 and res['records'][0, 0, 14] == 0.0
    ref = M.view_maps(g['narrow/fake'], g['narrow/label'], idx, int(div), thr, 'coronal')
    assert ref['raises']
    _check_view({k: (v[0] if k != 'range' else tuple(int(x) for x in v[0].cpu())) for k, v in res['coronal'].items()}, ref, 'narrow coronal')


def test_batched_entry_is_bit_identical_to_single_calls_and_between_runs():
    import hvgan  # noqa: F401
    from hvgan import evaluation
    fake, label = _volumes('small')
    fakes = [torch.from_numpy(fake).cuda(), torch.from_numpy(np.ascontiguousarray(fake[:, ::-1, :])).cuda(), torch.from_numpy(fake).cuda()]
    labels = [torch.from_numpy(label).cuda(), torch.from_numpy(np.ascontiguousarray(label[:, ::-1, :])).cuda(), torch.from_numpy(label).cuda()]
    ids = [IDX, IDX, 33]                       # pair 2: the original lacks vertebra 33
    runs = [evaluation.height_loss_dataset(fakes, labels, ids, DIV, THR, chunk=2) for _ in range(2)]
    whole = evaluation.height_loss_dataset(fakes, labels, ids, DIV, THR)
    a = runs[0]
    assert list(a['present']) == [True, True, False] and a['records'].shape == (3, 2, 16)
    for other in (runs[1], whole):
        assert np.array_equal(a['records'].view(np.int64), other['records'].view(np.int64))
        for view in VIEWS:
            for k in MAPS + PROFILES + ('flags', 'range'):
                assert _same_bits(a[view][k], other[view][k]), (view, k)
    H, W, Z = fake.shape
    assert a['sagittal']['loss'].shape == (3, Z, W) and a['coronal']['flags'].shape == (3, W, Z) and a['coronal']['curve'].shape == (3, Z)
    for i in range(3):
        one = evaluation.height_loss_map(fakes[i], labels[i], ids[i], DIV, THR)
        if ids[i] == 33:
            assert one is None
            for view in VIEWS:
                assert not a[view]['flags'][i].any() and bool(torch.isnan(a[view]['loss'][i]).all()) and not a[view]['height_fake'][i].any()
                assert bool(torch.isnan(a[view]['curve'][i]).all()) and a[view]['range'][i].tolist() == [0, 0]
            continue
        assert np.array_equal(one['records'].view(np.int64), a['records'][i].view(np.int64))
        for view in VIEWS:
            assert one[view]['range'] == tuple(a[view]['range'][i].tolist())
            for k in MAPS + PROFILES + ('flags',):
                assert _same_bits(one[view][k], a[view][k][i]), (i, view, k)
    # the mirrored pair is not a copy of the first
    assert not _same_bits(a['sagittal']['loss'][0], a['sagittal']['loss'][1])
    # and the records are hv_rhlv_views_batch's
    rec, present = evaluation.rhlv_dataset(fakes, labels, ids, DIV, THR, chunk=2)
    assert np.array_equal(rec.view(np.int64), a['records'].view(np.int64)) and list(present) == list(a['present'])


def test_reference_golden_volumes_on_the_device():
    import hvgan  # noqa: F401
    from hvgan import evaluation
    g = {k: np.asarray(v) for k, v in load_golden('g16_height_map').items()}
    names = sorted({k.split('/')[0] for k in g})
    assert len(names) >= 6
    for n in names:
        idx, div, thr = (float(v) for v in g[n + '/params'])
        f, l = torch.from_numpy(g[n + '/fake']).cuda(), torch.from_numpy(g[n + '/label']).cuda()
        for view in VIEWS:
            key = '%s/%s/' % (n, view)
            if g[key + 'raises']:
                with pytest.raises(ValueError):
                    evaluation.height_loss_map(f, l, idx, int(div), thr, views=(view,))
                continue
            got = evaluation.height_loss_map(f, l, idx, int(div), thr, views=(view,))
            _check_view(got[view], M.view_maps(g[n + '/fake'], g[n + '/label'], idx, int(div), thr, view), key)
            lo, hi = (int(v) for v in g[key + 'range'][2:])
            assert got[view]['range'] == (lo, hi)
            # the reference's own arrays, slice by slice: the selected columns of a row in column order, and its whole-volume means
            flags, hf, hl = (got[view][k].cpu().numpy() for k in ('flags', 'height_fake', 'height_label'))
            values, offsets = g[key + 'values'], g[key + 'offsets']
            for i, s in enumerate(range(lo, hi)):
                ref_f, ref_l = (values[offsets[8 * i + k]:offsets[8 * i + k + 1]] for k in range(2))
                assert _close(hf[s][flags[s] & M.SEL_FAKE != 0], ref_f), (key, s)
                assert np.array_equal(hl[s][flags[s] & M.SEL_LABEL != 0], ref_l), (key, s)
            assert _close(got['records'][0, :5], g[key + 'out']) and _close(got['records'][0, 5:13], g[key + 'means']), key
