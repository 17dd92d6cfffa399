"""Device generation-quality evaluation (hvgan.generation_eval: csrc/gen_eval.hip) against what the reference's own process_images decided
on fixture G14 (tools/make_golden_gen_eval.py) and against the float64 host restatement tests/gen_eval_ref.py on random volumes.

Slice selection, crop rows and data ranges are integer / min-max decisions: exact.  IoU, Dice and RVD come from exact integer counts:
bit-identical.  PSNR and SSIM are float64 sums in another grouping than numpy's and scipy's running means: 1e-9 relative, with a 1e-12
absolute floor for SSIM means that are rounding noise around 0 (a flat original crop against a varying generated one)."""
import math

import numpy as np
import pytest
import torch

from conftest import load_golden
import gen_eval_ref as ref

pytestmark = pytest.mark.gpu
LABEL = 20


def _g14():
    g = load_golden('g14_gen_eval')
    cases = {}
    for k, v in g.items():
        name, rest = k.split('/', 1)
        cases.setdefault(name, {})[rest] = v.numpy()
    return cases


def _assert_close(got, want):
    got, want = list(got), list(want)
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert ref.close(a, b), (i, a, b, got, want)


def _assert_result(got, want):
    """The seven values: PSNR / SSIM close, IoU / RVD / Dice bit-identical."""
    _assert_close(got[:4], want[:4])
    assert list(got[4:]) == [float(v) for v in want[4:]], (got, want)


@pytest.mark.parametrize('view', ['sagittal', 'coronal'])
def test_g14_matches_reference_decisions(view):
    from hvgan import generation_eval as GE
    cases = _g14()
    dev = torch.device('cuda:0')
    for name, c in sorted(cases.items()):
        label = int(c['label'])
        vols = [torch.from_numpy(c[k]).to(dev) for k in ('ori_ct', 'fake_ct', 'ori_seg', 'fake_seg')]
        if c[view + '/raises']:
            with pytest.raises(ValueError):
                GE.process_images(*vols, label, view=view)
            continue
        out, sl = GE.process_images(*vols, label, view=view, return_slices=True)
        _assert_result(out, c[view + '/out'])
        calls = c[view + '/calls']
        patch, glob = calls[calls[:, 0] == 0], calls[calls[:, 0] == 1]
        n = len(sl['z'])
        assert 2 * n == len(patch) == len(glob), name
        np.testing.assert_array_equal(sl['z'], patch[0::2, 2])
        np.testing.assert_array_equal(sl['x1'], patch[0::2, 3])
        np.testing.assert_array_equal(sl['x2'] - sl['x1'] + 1, patch[0::2, 4])
        np.testing.assert_array_equal(sl['R_patch'], patch[0::2, 6])
        np.testing.assert_array_equal(sl['R_global'], glob[0::2, 6])
        for k, rows in (('psnr_patch', patch[0::2]), ('ssim_patch', patch[1::2]), ('psnr_global', glob[0::2]), ('ssim_global', glob[1::2])):
            _assert_close(sl[k], rows[:, 7])
        ov = c[view + '/overlap']
        assert GE.calculate_iou(vols[2] == label, vols[3] == label) == ov[0]
        assert GE.calculate_dice(vols[2] == label, vols[3] == label) == ov[1]
        assert GE.relative_volume_difference(vols[2] == label, vols[3] == label) == ov[2]


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


@pytest.mark.parametrize('view', ['sagittal', 'coronal'])
@pytest.mark.parametrize('ct_dtype,label_dtype', [(np.float64, np.uint8), (np.float32, np.float32), (np.float64, np.float64),
                                                  (np.float32, np.uint8)])
def test_random_volumes_match_restatement(view, ct_dtype, label_dtype):
    from hvgan import generation_eval as GE
    ct, fct, ori, fake = _random_case(3)
    ct, fct = ct.astype(ct_dtype), fct.astype(ct_dtype)
    ori, fake = ori.astype(label_dtype), fake.astype(label_dtype)
    rec = []
    want = ref.process_images(ct, fct, ori, fake, LABEL, view=view, record=rec)
    assert len(rec) >= 10
    dev = torch.device('cuda:0')
    vols = [torch.from_numpy(a).to(dev) for a in (ct, fct, ori, fake)]
    got, sl = GE.process_images(*vols, LABEL, view=view, return_slices=True)
    _assert_result(got, want)
    np.testing.assert_array_equal(sl['z'], [r['z'] for r in rec])
    np.testing.assert_array_equal(sl['x1'], [r['x1'] for r in rec])
    np.testing.assert_array_equal(sl['x2'], [r['x2'] for r in rec])
    for k in ('R_patch', 'R_global', 'psnr_patch', 'ssim_patch', 'psnr_global', 'ssim_global'):
        _assert_close(sl[k], [r[k] for r in rec])
    # numpy arrays are uploaded, and the same volumes in other layouts give the same answer
    _assert_result(GE.process_images(ct, fct, ori, fake, LABEL, view=view), want)
    perms = {'zhw': (2, 0, 1), 'wzh': (1, 2, 0), 'hzw': (0, 2, 1)}
    for key, p in perms.items():
        inv = tuple(np.argsort(p))
        lay = [torch.from_numpy(np.ascontiguousarray(a.transpose(p))).to(dev).permute(*inv) for a in (ct, fct, ori, fake)]
        assert lay[0].shape == ct.shape and not lay[0].is_contiguous()
        _assert_result(GE.process_images(*lay, LABEL, view=view), want)
    fo = [np.asfortranarray(a) for a in (ct, fct, ori, fake)]
    _assert_result(GE.process_images(*fo, LABEL, view=view), want)


@pytest.mark.parametrize('view', ['sagittal', 'coronal'])
def test_identical_and_flat_volumes(view):
    """fake == ori: every PSNR is +inf and kept, every SSIM exactly 1.  A flat original crop that the generated CT reproduces: that slice's
    patch PSNR / SSIM are NaN and dropped from the means, its global PSNR +inf."""
    from hvgan import generation_eval as GE
    ct, fct, ori, fake = _random_case(5, shape=(41, 38, 33))
    ct = np.round(ct)
    got = GE.process_images(ct, ct.copy(), ori, ori.copy(), LABEL, view=view)
    assert got[0] == math.inf and got[2] == math.inf and got[1] == 1.0 and got[3] == 1.0 and got[4:] == (1.0, 0.0, 1.0)
    _assert_result(got, ref.process_images(ct, ct.copy(), ori, ori.copy(), LABEL, view=view))
    ax = ref.VIEW_AXIS[view]
    c, f = ct.copy(), np.round(fct)
    rows = np.flatnonzero((ori == LABEL).any(axis=(1, 2)))
    sel = [slice(None)] * 3
    sel[ax] = slice(0, ct.shape[ax] // 2)
    sel = tuple(sel)
    band = c[rows[0]:rows[-1] + 1]
    band[sel] = 321.0
    f[sel] = c[sel]
    rec = []
    want = ref.process_images(c, f, ori, fake, LABEL, view=view, record=rec)
    assert any(math.isnan(r['ssim_patch']) for r in rec) and not all(math.isnan(r['ssim_patch']) for r in rec)
    got, sl = GE.process_images(c, f, ori, fake, LABEL, view=view, return_slices=True)
    _assert_result(got, want)
    _assert_close(sl['ssim_patch'], [r['ssim_patch'] for r in rec])
    _assert_close(sl['psnr_global'], [r['psnr_global'] for r in rec])


def test_errors_and_odd_shapes():
    from hvgan import generation_eval as GE
    ct, fct, ori, fake = _random_case(7)
    with pytest.raises(ValueError):
        GE.process_images(ct, fct, np.zeros_like(ori), fake, LABEL)
    # a selected slice whose patch has 6 rows: structural_similarity raises in the reference
    thin = np.zeros((20, 90, 12), np.uint8)
    thin[5:11, 2:88, 1:11] = LABEL
    tct = np.random.default_rng(1).uniform(0, 100, size=thin.shape)
    with pytest.raises(ValueError):
        ref.process_images(tct, tct + 1, thin, thin, LABEL)
    with pytest.raises(ValueError):
        GE.process_images(tct, tct + 1, thin, thin, LABEL)
    # 7 rows pass, in both
    thin[11] = thin[10]
    _assert_result(GE.process_images(tct, tct + 1, thin, thin, LABEL), ref.process_images(tct, tct + 1, thin, thin, LABEL))
    with pytest.raises(ValueError):
        GE.process_images(ct, fct, ori, fake, LABEL, view='axial')


def test_evaluate_generation_skip_and_average():
    from hvgan import generation_eval as GE
    items = []
    for seed in (11, 12, 13):
        ct, fct, ori, fake = _random_case(seed)
        items.append((ct, fct, ori, fake, LABEL))
    # patch metrics NaN / 0: a vertebra whose crop rows are flat and reproduced in every slice -> empty patch lists -> 0 -> skipped
    ct, fct, ori, fake = _random_case(14)
    ct = np.round(ct)
    rows = np.flatnonzero((ori == LABEL).any(axis=(1, 2)))
    ct[rows[0]:rows[-1] + 1] = 55.0
    items.insert(1, (ct, ct.copy(), ori, fake, LABEL))
    # a vertebra with no evaluated slice (every slice <= 400 voxels): zeros -> skipped
    small = np.zeros_like(ori)
    small[10:20, 10:20, 5:20] = LABEL
    items.append((ct, fct, small, small, LABEL))
    want_each = [ref.process_images(*it) for it in items]
    assert want_each[1][2] == 0 and want_each[-1][2] == 0
    want, n = ref.main_average(want_each)
    dev = torch.device('cuda:0')
    dev_items = [tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in it[:4]) + (it[4],) for it in items]
    got = GE.evaluate_generation(iter(dev_items), view='sagittal')
    assert got['count'] == n == 3
    for k in GE.KEYS:
        assert ref.close(got[k], want[k]), (k, got[k], want[k])
    for a, b in zip(got['per_volume'], want_each):
        _assert_result(a, b)
    empty = GE.evaluate_generation([])
    assert empty['count'] == 0 and all(math.isnan(empty[k]) for k in GE.KEYS)


def test_process_volume_output_end_to_end():
    """One infer.process_volume output (float64 [H, W, Z] numpy arrays) straight into process_images, against the restatement on the same
    arrays (model setup of tests/test_infer_gpu.py)."""
    from hvgan import synth, infer
    from hvgan import generation_eval as GE
    from hvgan.models.inpaint_networks import Generator
    torch.manual_seed(5)
    net = Generator({'input_dim': 1, 'ngf': 16}, True)
    net.fine_generator.fc_height.bias.data.fill_(0.41)
    net.fine_generator.fc_height.weight.data.mul_(1e-2)
    net.cuda().train()
    dev = torch.device('cuda:0')
    b = synth.to_model_inputs(synth.make_batch(2, 256, seed=3))
    for _ in range(3):
        net.run_forward(b['real_A'].to(dev), b['mask'].to(dev), (1 - b['CAM']).to(dev), b['slice_ratio'].to(dev), training=True)
    net.eval()
    ct, label, cam = synth.make_volume(nz=16, size=256, seed=2)
    out_ct, out_seg = infer.process_volume(net, ct, label, cam * 255, 20, dev)
    assert out_ct.dtype == np.float64 and out_seg.shape == label.shape
    for view in ('sagittal', 'coronal'):
        rec = []
        want = ref.process_images(ct, out_ct, label, out_seg, 20, view=view, record=rec)
        assert len(rec) >= 5
        got = GE.process_images(ct, out_ct, label, out_seg, 20, view=view)
        _assert_result(got, want)
        res = GE.evaluate_generation([(ct, out_ct, label, out_seg, 20)], view=view)
        _assert_result([res[k] for k in GE.KEYS], list(ref.main_average([want])[0].values()))
