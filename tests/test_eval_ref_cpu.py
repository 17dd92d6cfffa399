"""tests/eval_ref.py pinned on the CPU: both forms against fixture G11's per-sample values (outputs of the reference's own evaluate_model around the
restated skimage algorithm), and the conditioning of every input tests/test_eval_edges_gpu.py uses -- there the float32 form must lie within ONE QUARTER of
the device tolerance of the float64 form, so a device result within tolerance of the float32 form is within 1.25 tolerances of the definition, and a
failure of the device test cannot be blamed on an input whose float32 rounding alone eats the tolerance."""
import numpy as np
import pytest
import torch

import eval_ref as ER
from oracle import restate as R
from test_oracle_golden import g11_cases


def _g11_samples():
    for name, b, outs, exp in g11_cases():
        coarse, fine, _, stage2, _, _, pred2 = outs
        pred_h = (pred2.T * b['maxheight'])[0]
        inp = R.shrm_composite(stage2, b['real_B'], pred_h, b['height'], b['x1'], b['x2'])
        cb, fb = (coarse > 0.5).float(), (fine > 0.5).float()
        for i in range(stage2.shape[0]):
            n = lambda t: t[i, 0].numpy()
            yield '%s/%d' % (name, i), (n(inp), n(b['real_B']), n(b['mask']), n(cb), n(b['normal_vert']), n(fb), n(b['real_B_mask']),
                                        float(pred_h[i]), int(b['height'][i])), exp['per_sample'][i]


def test_both_forms_reproduce_fixture_g11():
    n = 0
    for name, args, want in _g11_samples():
        f32, f64 = ER.metrics_f32(*args), ER.metrics_f64(*args)
        assert np.allclose(f32[:2], want[:2], rtol=1e-9, atol=0), (name, f32, want)          # the fixture's own restated functions
        assert np.allclose(f32[2:], want[2:], rtol=1e-6, atol=1e-7), (name, f32, want)       # the reference's torch arithmetic
        for k, tol in enumerate(ER.TOL):
            assert abs(f64[k] - want[k]) <= tol, (name, k, f64[k], want[k])
        n += 1
    assert n >= 8


def _conditioned(name, args):
    f32, f64 = ER.metrics_f32(*args), ER.metrics_f64(*args)
    assert np.isfinite(f64).all() and np.isfinite(f32).all(), (name, f32, f64)
    for k, tol in enumerate(ER.TOL):
        d = abs(f32[k] - f64[k])
        assert d <= tol / 4, (name, k, f32[k], f64[k], d)
    return np.abs(f32 - f64) / np.array(ER.TOL)


@pytest.mark.parametrize('shape', ER.SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_float32_form_within_a_quarter_tolerance_of_float64_on_the_gpu_inputs(shape):
    d = ER.edge_inputs(*shape)
    worst = np.zeros(5)
    for i in range(shape[0]):
        worst = np.maximum(worst, _conditioned((shape, i), ER.sample(d, i)))
    print('f32 vs f64 / tolerance', shape, worst)


def test_batch_case_is_conditioned_and_is_what_the_oracle_composites():
    outs, b = ER.batch_case()
    m, inp = R.eval_sample_metrics(outs['stage2'], outs['fine_seg'], outs['coarse_seg'], outs['pred2'], b)
    cb, fb = (outs['coarse_seg'] > 0.5).float(), (outs['fine_seg'] > 0.5).float()
    pred_h = (outs['pred2'].T * b['maxheight'])[0]
    for i in range(inp.shape[0]):
        n = lambda t: t[i, 0].numpy()
        x1, x2 = int(b['x1'][i]), int(b['x2'][i])
        assert torch.equal(inp[i, 0, x1:x2], outs['stage2'][i, 0, x1:x2]) and torch.equal(inp[i, 0, :x1], b['real_B'][i, 0, :x1])
        assert torch.equal(inp[i, 0, x2:], b['real_B'][i, 0, x2:])
        args = (n(inp), n(b['real_B']), n(b['mask']), n(cb), n(b['normal_vert']), n(fb), n(b['real_B_mask']), float(pred_h[i]), int(b['height'][i]))
        _conditioned(('batch', i), args)
        assert np.allclose(ER.metrics_f32(*args), m[i], rtol=1e-6, atol=1e-7)


def test_float64_form_on_closed_cases():
    """identical images: SSIM 1, PSNR inf; an all-zero mask: SSIM 1; empty maps: Dice = IoU = 1; a constant shift of a flat image: the closed SSIM
    expression (variances 0, means c and c + d)"""
    d = ER.edge_inputs(1, 12, 9)
    a = list(ER.sample(d, 0))
    a[1] = a[0]
    m = ER.metrics_f64(*a)
    assert abs(m[0] - 1.0) <= 1e-15 and m[1] == float('inf')
    a = list(ER.sample(d, 0))
    a[2] = np.zeros_like(a[2])
    assert ER.metrics_f64(*a)[0] == 1.0
    a[3] = a[4] = a[5] = a[6] = np.zeros_like(a[2])
    m = ER.metrics_f64(*a)
    assert m[2] == 1.0 and m[3] == 1.0
    x, y = np.full((9, 9), 0.5), np.full((9, 9), 0.25)
    C1 = (0.01 * 2.0) ** 2
    assert abs(ER.ssim_f64(x, y, 2.0) - (2 * 0.5 * 0.25 + C1) / (0.25 + 0.0625 + C1)) <= 1e-15
