"""The set form of generation evaluation (hv_gen_eval_batch, hvgan.generation_eval.process_images_batch / evaluate_experiments) against
the single-pair entry hv_gen_eval and the float64 host restatement tests/gen_eval_ref.py.

The contract is bit-identity with hv_gen_eval: the batch kernels call the device functions the single-pair kernels call and sum in the
same orders, so every out[i][e][0:16] and every slice record is compared by bit pattern (NaNs included), with no tolerance.  Against the
restatement the bound is that module's own `close` (rtol 1e-9, atol 1e-12), the integer-derived fields exact.

Shapes: (37, 45, 29) one SSIM column tile and two row tiles; (37, 77, 13) 71 interior columns cross the 64-column tile edge; (38, 78, 30)
has even extents, so the strides allow the 2-wide loads of pass 1 and the block's own alignment check decides (the odd shapes never take
them).  C order, Fortran order and a permuted layout run the three lane layouts of pass 1 (slices, rows, columns fastest)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import gen_eval_ref as ref

pytestmark = pytest.mark.gpu
LABEL = 20
SHAPES = [(37, 45, 29), (37, 77, 13)]
EVEN = (38, 78, 30)
DTYPES = [(np.float64, np.uint8), (np.float32, np.float32), (np.float64, np.float64), (np.float32, np.uint8)]


def _ellipsoid(shape, centre, radii):
    g = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing='ij')
    return sum(((x - c) / r) ** 2 for x, c, r in zip(g, centre, radii)) <= 1.0


def _random_case(seed, shape=(37, 45, 29)):
    rng = np.random.default_rng(seed)
    H, W, Z = shape
    ori = np.zeros(shape, np.uint8)
    ori[_ellipsoid(shape, (H / 2, W / 2, Z / 2), (H * 0.38, W * 0.38, Z * 0.42))] = LABEL
    ori[:3] = LABEL - 1
    fake = np.zeros(shape, np.uint8)
    fake[_ellipsoid(shape, (H / 2 + 1, W / 2, Z / 2 - 1), (H * 0.36, W * 0.4, Z * 0.42))] = LABEL
    ct = rng.uniform(-200.0, 900.0, size=shape)
    fct = ct + rng.normal(0.0, 40.0, size=shape) * (fake == LABEL)
    return ct, fct, ori, fake


def _set(shape, n=3, seed=20):
    """n items x 3 experiments: a perturbed volume, the original itself, a volume whose label is empty."""
    originals, fakes = [], []
    for i in range(n):
        ct, fct, ori, fake = _random_case(seed + i, shape)
        originals.append((ct, ori, LABEL))
        fakes.append([(fct, fake), (ct.copy(), ori.copy()), (fct, np.zeros_like(fake))])
    return originals, fakes


def _dev(a):
    return a if isinstance(a, torch.Tensor) or a is None else torch.from_numpy(a).cuda()


def _to_device(originals, fakes):
    return [(_dev(c), _dev(s), l) for c, s, l in originals], [[(_dev(c), _dev(s)) for c, s in row] for row in fakes]


def _single(original, fake, view):
    """hv_gen_eval's raw output of one pair: (out[16], records [S][9]), both from zeroed buffers like the batch wrapper's."""
    from hvgan import generation_eval as GE
    S = original[1].shape[GE.VIEWS[view]]
    buf = torch.zeros(16 + 9 * S, dtype=torch.float64, device='cuda')
    GE._launch(original[0], fake[0], original[1], fake[1], original[2], view, buf[:16], buf[16:])
    o = buf.cpu().numpy()
    return o[:16], o[16:].reshape(S, 9)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def _assert_same_bits(got, want, what):
    assert np.array_equal(_bits(got), _bits(want)), (what, got, want)


def _batch(originals, fakes, view, chunk=None):
    from hvgan import generation_eval as GE
    return GE._batch_outputs(originals, fakes, view, True, chunk)


_CACHE = {}


def _reference_set(shape, view):
    """Device copies of _set(shape) and hv_gen_eval's raw output for each of its pairs, computed once per (shape, view)."""
    if ('set', shape) not in _CACHE:
        host = _set(shape)
        _CACHE[('set', shape)] = host + _to_device(*host)
    ho, hf, do, df = _CACHE[('set', shape)]
    if (shape, view) not in _CACHE:
        _CACHE[(shape, view)] = [[_single(do[i], df[i][e], view) for e in range(3)] for i in range(3)]
    return ho, hf, do, df, _CACHE[(shape, view)]


def _assert_matches_singles(out, rec, singles, order_i, order_e, what):
    for a, i in enumerate(order_i):
        for b, e in enumerate(order_e):
            _assert_same_bits(out[a, b], singles[i][e][0], (what, 'out', i, e))
            _assert_same_bits(rec[a][b], singles[i][e][1], (what, 'slices', i, e))


@pytest.mark.parametrize('view', ['sagittal', 'coronal'])
@pytest.mark.parametrize('shape', SHAPES)
def test_batch_is_bit_identical_to_single_pairs(shape, view):
    _, _, do, df, singles = _reference_set(shape, view)
    if shape == SHAPES[0]:
        assert all(math.isinf(row[1][0][0]) and row[1][0][1] == 1.0 for row in singles)   # the original against itself
        assert all(row[0][0][9] >= 5 and row[0][0][15] >= 5 for row in singles)      # slices are evaluated
        assert all(0.0 < row[0][0][1] < 1.0 for row in singles)
    out, rec = _batch(do, df, view)
    assert out.shape == (3, 3, 16)
    _assert_matches_singles(out, rec, singles, range(3), range(3), 'N3E3')
    # a pair alone
    out, rec = _batch(do[1:2], [df[1][0:1]], view)
    _assert_matches_singles(out, rec, singles, [1], [0], 'N1E1')
    # the experiments in reversed order
    out, rec = _batch(do, [row[::-1] for row in df], view)
    _assert_matches_singles(out, rec, singles, range(3), [2, 1, 0], 'reversed experiments')
    # one item per call
    out, rec = _batch(do, df, view, chunk=1)
    _assert_matches_singles(out, rec, singles, range(3), range(3), 'chunk=1')
    # the item list reversed
    out, rec = _batch(do[::-1], df[::-1], view)
    _assert_matches_singles(out, rec, singles, [2, 1, 0], range(3), 'reversed items')


def test_more_experiments_than_one_register_group():
    """Pass 1 keeps four experiments' accumulators in registers; E = 6 runs a full group and a partial one per item."""
    shape = SHAPES[0]
    _, _, do, df, singles = _reference_set(shape, 'sagittal')
    order = [0, 1, 2, 0, 2, 1]
    out, rec = _batch(do[:2], [[row[e] for e in order] for row in df[:2]], 'sagittal')
    _assert_matches_singles(out, rec, singles, [0, 1], order, 'E6')


@pytest.mark.parametrize('view', ['sagittal', 'coronal'])
@pytest.mark.parametrize('shape', SHAPES)
def test_batch_matches_host_restatement(shape, view):
    from hvgan import generation_eval as GE
    ho, hf, do, df, _ = _reference_set(shape, view)
    got, sl = GE.process_images_batch(do, df, view=view, return_slices=True)
    assert got.shape == (3, 3, 7)
    for i in range(3):
        for e in range(3):
            recs = []
            want = ref.process_images(ho[i][0], hf[i][e][0], ho[i][1], hf[i][e][1], LABEL, view=view, record=recs)
            for q in range(4):
                assert ref.close(got[i, e, q], want[q]), (i, e, q, got[i, e], want)
            assert list(got[i, e, 4:]) == [float(v) for v in want[4:]], (i, e, got[i, e], want)
            for k in ('z', 'x1', 'x2'):
                np.testing.assert_array_equal(sl[i][e][k], [r[k] for r in recs])
            for k in ('R_patch', 'R_global', 'psnr_patch', 'ssim_patch', 'psnr_global', 'ssim_global'):
                assert len(sl[i][e][k]) == len(recs)
                for a, b in zip(sl[i][e][k], [r[k] for r in recs]):
                    assert ref.close(a, b), (i, e, k, a, b)


def test_error_flags_stay_with_their_item():
    """Item 1 has no vertebra, item 2 a selected slice whose patch has 6 rows (20 x 90 x 12, rows 5..10); item 0 has 7 rows and passes."""
    from hvgan import generation_eval as GE
    shape = (20, 90, 12)
    ok = np.zeros(shape, np.uint8)
    ok[5:12, 2:88, 1:11] = LABEL
    thin = np.zeros(shape, np.uint8)
    thin[5:11, 2:88, 1:11] = LABEL
    rng = np.random.default_rng(1)
    originals, fakes = [], []
    for seg in (ok, np.zeros(shape, np.uint8), thin):
        ct = rng.uniform(0, 100, size=shape)
        originals.append((ct, seg, LABEL))
        fakes.append([(ct + 1, seg.copy()), (ct + rng.normal(0, 3, size=shape), ok.copy())])
    with pytest.raises(ValueError):
        ref.process_images(originals[2][0], fakes[2][0][0], thin, thin, LABEL)
    do, df = _to_device(originals, fakes)
    out, rec = _batch(do, df, 'sagittal')
    np.testing.assert_array_equal(out[:, :, 7], [[0, 0], [1, 1], [0, 0]])
    np.testing.assert_array_equal(out[:, :, 8], [[0, 0], [0, 0], [1, 1]])
    for i in range(3):
        for e in range(2):
            o, r = _single(do[i], df[i][e], 'sagittal')
            _assert_same_bits(out[i, e], o, ('out', i, e))
            _assert_same_bits(rec[i][e], r, ('slices', i, e))
    for e in range(2):
        want = ref.process_images(originals[0][0], fakes[0][e][0], ok, fakes[0][e][1], LABEL)
        assert all(ref.close(a, b) for a, b in zip(out[0, e, :4], want[:4])) and list(out[0, e, 4:7]) == [float(v) for v in want[4:]]
    with pytest.raises(ValueError, match=r'item 1, experiment 0\).*does not contain'):
        GE.process_images_batch(do, df)
    with pytest.raises(ValueError, match=r'item 1, experiment 0\).*shorter than 7'):
        GE.process_images_batch([do[0], do[2]], [df[0], df[2]])
    assert GE.process_images_batch(do[:1], df[:1]).shape == (1, 2, 7)


def _offset_by_one(t):
    """The same values and strides in storage whose base is one element past an aligned address."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % (2 * t.element_size()) != 0
    return v


def _layouts(arrays):
    """name -> the arrays as device tensors of that layout, all [H, W, Z]: C order (slices or columns fastest, by view), Fortran order
    (rows fastest), memory order z, h, w (columns or slices fastest)."""
    def perm(a, p):
        return torch.from_numpy(np.ascontiguousarray(a.transpose(p))).cuda().permute(*[int(q) for q in np.argsort(p)])
    return {'C': [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays],
            'F': [torch.from_numpy(np.asfortranarray(a)).cuda() for a in arrays],
            'zhw': [perm(a, (2, 0, 1)) for a in arrays]}


@pytest.mark.parametrize('view', ['sagittal', 'coronal'])
@pytest.mark.parametrize('ct_dtype,label_dtype', DTYPES)
def test_layouts_and_dtypes_bit_identical(ct_dtype, label_dtype, view):
    """N = 2, E = 2 in every layout.  With the float32 CT, item 0's first synthesized CT starts one element off an 8-byte boundary: the
    blocks of item 0 refuse the 2-wide loads, those of item 1 take them (even shape), and the bits are the single entry's either way."""
    for shape in (SHAPES[1], EVEN):
        items = []
        for i in range(2):
            ct, fct, ori, fake = _random_case(40 + i, shape)
            fct2 = ct + (fct - ct)[::-1]
            items.append([a.astype(ct_dtype) for a in (ct, fct, fct2)] + [a.astype(label_dtype) for a in (ori, fake, fake[::-1].copy())])
        lay = [_layouts(arrays) for arrays in items]
        for name in ['C', 'F', 'zhw'] + (['offset'] if ct_dtype == np.float32 else []):
            vols = [list(lay[i]['C' if name == 'offset' else name]) for i in range(2)]
            if name == 'offset':      # (ct, fct, fct2, ...): item 0's first synthesized CT gets the misaligned base
                vols[0][1] = _offset_by_one(vols[0][1])
            originals = [(v[0], v[3], LABEL) for v in vols]
            fakes = [[(v[1], v[4]), (v[2], v[5])] for v in vols]
            assert originals[0][0].stride() == fakes[0][0][0].stride() == originals[1][0].stride()
            out, rec = _batch(originals, fakes, view)
            for i in range(2):
                for e in range(2):
                    o, r = _single(originals[i], fakes[i][e], view)
                    _assert_same_bits(out[i, e], o, (shape, name, 'out', i, e))
                    _assert_same_bits(rec[i][e], r, (shape, name, 'slices', i, e))
            if shape == EVEN:
                assert out[0, 0, 9] >= 5 and 0.0 < out[0, 0, 3] < 1.0, (name, out[0, 0])


def test_evaluate_experiments_equals_evaluate_generation_per_experiment():
    """Three experiments over four vertebrae.  'failed' holds synthesized CTs that are NaN throughout (an export that went wrong): every
    volume's patch PSNR / SSIM are NaN-dropped to 0 and skipped, so its means are NaN and its count 0."""
    from hvgan import generation_eval as GE
    originals, exps = [], {'noisy': [], 'failed': [], 'shifted': []}
    for seed in (11, 12, 13, 14):
        ct, fct, ori, fake = _random_case(seed)
        originals.append((_dev(ct), _dev(ori), LABEL))
        exps['noisy'].append((_dev(fct), _dev(fake)))
        exps['failed'].append((_dev(np.full_like(ct, math.nan)), _dev(fake)))
        exps['shifted'].append((_dev(fct + 3.0), _dev(ori.copy())))
    got = GE.evaluate_experiments(originals, exps, view='sagittal')
    assert list(got) == ['noisy', 'failed', 'shifted']
    for name, vols in exps.items():
        want = GE.evaluate_generation([(o[0], f[0], o[1], f[1], o[2]) for o, f in zip(originals, vols)], view='sagittal')
        assert set(got[name]) == set(want) == set(GE.KEYS) | {'count', 'per_volume'}
        assert got[name]['count'] == want['count']
        for k in GE.KEYS:
            _assert_same_bits(got[name][k], want[k], (name, k))
        _assert_same_bits(got[name]['per_volume'], want['per_volume'], (name, 'per_volume'))
    assert got['failed']['count'] == 0 and all(math.isnan(got['failed'][k]) for k in GE.KEYS)
    assert got['noisy']['count'] == 4 and got['shifted']['count'] == 4 and got['shifted']['iou'] == 1.0
    assert math.isfinite(got['noisy']['patch_psnr']) and 0.0 < got['noisy']['patch_ssim'] < 1.0
    assert GE.evaluate_experiments(originals, {}) == {}


def test_counts_only_form():
    """Both CT tables NULL: out[4..12] only, the bits of calculate_iou / calculate_dice / relative_volume_difference per pair."""
    from hvgan import generation_eval as GE
    originals, fakes = [], []
    for seed in (31, 32, 33):
        _, _, ori, fake = _random_case(seed)
        o, f = _dev((ori == LABEL).astype(np.uint8)), _dev((fake == LABEL).astype(np.uint8))
        originals.append((None, o, 1.0))
        fakes.append([(None, f), (None, o.clone()), (None, torch.zeros_like(f))])
    out, _ = GE._batch_outputs(originals, fakes, 'sagittal', False, None, counts_only=True)
    assert not out[:, :, :4].any() and not out[:, :, 13:].any()          # nothing but the counts is written
    for i in range(3):
        for e in range(3):
            o, f = originals[i][1], fakes[i][e][1]
            _assert_same_bits(out[i, e, 4:7], [GE.calculate_iou(o, f), GE.relative_volume_difference(o, f), GE.calculate_dice(o, f)], (i, e))
            assert out[i, e, 10] == int(o.sum()) and out[i, e, 11] == int(f.sum()) and out[i, e, 12] == int((o & f).sum())
    assert out[0, 1, 4] == 1.0 and out[0, 2, 4] == 0.0 and out[0, 2, 5] == 1.0


def test_argument_errors_launch_nothing():
    from hvgan import lib
    L = lib.get()
    shape = SHAPES[0]
    _, _, do, df, _ = _reference_set(shape, 'sagittal')
    N, E = 2, 3
    cts = [do[i][0] for i in range(N)], [df[i][e][0] for i in range(N) for e in range(E)]
    segs = [do[i][1] for i in range(N)], [df[i][e][1] for i in range(N) for e in range(E)]
    table = lambda ts: torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64, device='cuda')
    oc, fc, os_, fs = table(cts[0]), table(cts[1]), table(segs[0]), table(segs[1])
    labels = torch.full((N,), float(LABEL), dtype=torch.float64, device='cuda')
    H, W, Z = shape
    need = L.size('hv_gen_eval_batch_workspace_bytes', H, W, Z, 2, N, E)
    ws = torch.empty(need + 64, dtype=torch.uint8, device='cuda')
    out = torch.full((N, E, 16), 7.25, dtype=torch.float64, device='cuda')

    def call(n, e, wsz):
        return L.cdll.hv_gen_eval_batch(lib.ptr(oc), lib.ptr(fc), 5, *[ctypes.c_longlong(v) for v in cts[0][0].stride()], lib.ptr(os_),
                                        lib.ptr(fs), 0, *[ctypes.c_longlong(v) for v in segs[0][0].stride()], H, W, Z, 2, lib.ptr(labels),
                                        n, e, lib.ptr(out), None, lib.ptr(ws), ctypes.c_size_t(wsz), lib.stream())
    HV_ERR_ARG = -1
    assert call(0, E, need) == HV_ERR_ARG
    assert call(N, 0, need) == HV_ERR_ARG
    assert call(N, E, need - 1) == HV_ERR_ARG
    torch.cuda.synchronize()
    assert bool((out == 7.25).all())
    # and the same call with the workspace it asked for runs
    assert call(N, E, need) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    _, _, _, _, singles = _reference_set(shape, 'sagittal')
    for i in range(N):
        for e in range(E):
            _assert_same_bits(got[i, e], singles[i][e][0], (i, e))
