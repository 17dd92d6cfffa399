"""The fp64 references of tests/pointwise_ref.py against torch autograd (fp64, CPU): the same computation built from F.batch_norm / F.instance_norm,
the activation and F.binary_cross_entropy_with_logits.  Inputs are drawn so that no pre-activation lies within 1e-3 of a kink, where autograd's
derivative at v and the references' rule-from-y agree."""
import pytest
import torch
import torch.nn.functional as F

import pointwise_ref as PR

RTOL = 1e-12
B, C, H, W = 2, 5, 3, 8
EPS, MOM = 1e-5, 0.1


def close(a, b, what):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = (a - b).abs().max().item()
    assert err <= RTOL * max(b.abs().max().item(), 1e-300), (what, err, b.abs().max().item())


def torch_act(v, act):
    return {'none': lambda t: t, 'elu': F.elu, 'relu': F.relu, 'lrelu': lambda t: F.leaky_relu(t, 0.2), 'sigmoid': torch.sigmoid,
            'clamp': lambda t: t.clamp(-1, 1)}[act](v)


def away_from_kinks(v):
    return bool(((v.abs() > 1e-3) & ((v.abs() - 1).abs() > 1e-3)).all())


def torch_norm(x, norm, training, gamma, beta, rm, rv, groups):
    """Pre-activation of the normalisation; rm / rv are updated in place, one call per group in order."""
    if norm == 'instance':
        return F.instance_norm(x, weight=gamma, bias=beta, eps=EPS), 0
    calls = 0
    outs = []
    for s in PR.group_slices(x.shape[0], norm, groups):
        outs.append(F.batch_norm(x[s], rm, rv, gamma, beta, training, MOM, EPS))
        calls += int(training)
    return torch.cat(outs), calls


def draw(norm, training, groups, seed0):
    for seed in range(seed0, seed0 + 200):
        gen = torch.Generator().manual_seed(seed)
        r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
        x = r(B, C, H, W) * (r(1, C, 1, 1).abs() + 0.5) + 2 * r(1, C, 1, 1)
        gamma, beta = r(C), r(C)
        gamma[1] = -gamma[1].abs()
        rm, rv = r(C), r(C).abs() + 0.5
        dy = r(B, C, H, W)
        if norm == 'instance':
            gamma, beta = torch.ones(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
        v, _ = torch_norm(x, norm, training, gamma, beta, rm.clone(), rv.clone(), groups)
        if away_from_kinks(v):
            return x, gamma, beta, rm, rv, dy
    raise AssertionError('no draw away from the kinks')


CASES = [(norm, training, groups, act, ps)
         for norm, training, groups in (('batch', True, 1), ('batch', True, 2), ('batch', False, 1), ('instance', True, 1))
         for act, ps in [(a, False) for a in PR.ACTS] + [('none', True), ('relu', True), ('lrelu', True)]]


@pytest.mark.parametrize('norm,training,groups,act,ps', CASES)
def test_norm_act_refs_match_autograd(norm, training, groups, act, ps):
    x, gamma, beta, rm, rv, dy = draw(norm, training, groups, 100)
    xa, ga, ba = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    trm, trv = rm.clone(), rv.clone()
    v, calls = torch_norm(xa, norm, training, ga, ba, trm, trv, groups)
    ty = torch_act(v, act)
    if ps:
        ty = torch.sigmoid(ty)
    (ty * dy).sum().backward()

    y, stats, nrm, nrv, nbt = PR.norm_act_forward_ref(x, norm, training, gamma, beta, rm, rv, EPS, MOM, groups, act, ps)
    close(y, ty.detach(), 'y')
    if norm == 'batch':
        close(nrm, trm, 'running_mean')
        close(nrv, trv, 'running_var')
        assert nbt == calls == (groups if training else 0)
        if not training:
            assert torch.equal(nrm, rm) and torch.equal(nrv, rv)
            close(stats[0, 0], rm, 'eval mean')
            close(stats[0, 1], 1 / torch.sqrt(rv + EPS), 'eval rstd')
    else:
        assert nbt == 0 and torch.equal(nrm, rm) and torch.equal(nrv, rv)
    assert stats.shape == ((B if norm == 'instance' else groups), 2, C)
    if training:      # batch statistics of every group
        for k, s in enumerate(PR.group_slices(B, norm, groups)):
            close(stats[k, 0], x[s].mean(dim=(0, 2, 3)), 'mean')
            close(stats[k, 1], 1 / torch.sqrt(x[s].var(dim=(0, 2, 3), unbiased=False) + EPS), 'rstd')

    dx, dgamma, dbeta = PR.norm_act_backward_ref(dy, y, x, stats, gamma, norm, training, groups, act, ps)
    close(dx, xa.grad, 'dx')
    close(dgamma, ga.grad, 'dgamma')
    close(dbeta, ba.grad, 'dbeta')
    if act == 'none' and not ps:      # y is not read
        dx2, _, _ = PR.norm_act_backward_ref(dy, torch.full_like(y, float('nan')), x, stats, gamma, norm, training, groups, act, ps)
        assert torch.equal(dx2, dx)


@pytest.mark.parametrize('act', ['elu', 'sigmoid', 'clamp'])
def test_post_sigmoid_rule_is_refused_where_it_is_not_the_derivative(act):
    with pytest.raises(ValueError):
        PR.act_grad_from_out_formula(torch.full((2,), 0.25, dtype=torch.float64), act, True)


def test_running_update_with_one_row_uses_the_plain_variance():
    x = torch.randn(1, 3, 1, 1, dtype=torch.float64)
    z = torch.zeros(3, dtype=torch.float64)
    _, stats, rm, rv, nbt = PR.norm_act_forward_ref(x, 'batch', True, z + 1, z, z.clone(), z + 1, EPS, MOM, 1, 'none', False)
    close(rm, MOM * x.view(3), 'rm')
    close(rv, (1 - MOM) * (z + 1), 'rv')      # var == 0, R == 1: no R / (R - 1)
    assert nbt == 1


@pytest.mark.parametrize('act', [a for a in PR.ACTS if a != 'none'])
def test_act_backward_and_head_seed_refs_match_autograd(act):
    for seed in range(200):
        gen = torch.Generator().manual_seed(seed)
        v = torch.randn(B, C, H, W, generator=gen, dtype=torch.float64) * 1.5
        if away_from_kinks(v):
            break
    dy = torch.randn(B, C, H, W, generator=gen, dtype=torch.float64)
    va = v.clone().requires_grad_(True)
    y = torch_act(va, act)
    (y * dy).sum().backward()
    g, dbias = PR.act_backward_ref(dy, y.detach(), act)
    close(g, va.grad, 'g')
    close(dbias, va.grad.sum(dim=(0, 2, 3)), 'dbias')
    close(PR.head_seed_ref(dy[:, :1], y.detach()[:, :1], act), va.grad[:, :1], 'head seed')
    close(PR.act_formula(v, act), y.detach(), 'act')


def test_act_none_passes_the_gradient_through():
    dy = torch.randn(B, C, H, W, dtype=torch.float64)
    g, dbias = PR.act_backward_ref(dy, torch.zeros_like(dy), 'none')
    assert torch.equal(g, dy)
    close(dbias, dy.sum(dim=(0, 2, 3)), 'dbias')
    assert torch.equal(PR.head_seed_ref(dy, torch.zeros_like(dy), 'none'), dy)


@pytest.mark.parametrize('mode', ['vanilla', 'lsgan'])
@pytest.mark.parametrize('real', [True, False])
def test_gan_loss_ref_matches_autograd(mode, real):
    gen = torch.Generator().manual_seed(5)
    z = torch.cat([torch.randn(231, generator=gen, dtype=torch.float64) * 3,
                   torch.tensor([0.0, 1e-4, -1e-4, 30.0, -30.0, 90.0, -90.0], dtype=torch.float64)])
    za = z.clone().requires_grad_(True)
    t = torch.full_like(z, 1.0 if real else 0.0)
    tl = F.binary_cross_entropy_with_logits(za, t) if mode == 'vanilla' else F.mse_loss(za, t)
    tl.backward()
    loss, dz = PR.gan_loss_ref(z, real, mode)
    close(loss, tl.detach(), 'loss')
    # element by element: a logit of +-90 has a gradient of 1e-39 / n next to ones of 1 / n
    assert ((dz - za.grad).abs() <= RTOL * za.grad.abs() + 1e-300).all()
    l, _ = PR.gan_loss_terms_formula(z, real, mode)
    close(l.sum() / z.numel(), loss, 'terms')


# ---------------------------------------------------------------------------------------------------------------- generator loss tail
import os  # noqa: E402

import numpy as np  # noqa: E402

from oracle import restate  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def loss_batch(seed, Bn=3, Hn=6, Wn=10):
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=gen, dtype=torch.float64)
    I = {k: r(Bn, 1, Hn, Wn) * 2 - 1 for k in ('fake_B', 'fake_B_coarse', 'real_B')}
    I.update({k: r(Bn, 1, Hn, Wn) for k in ('fine_seg', 'coarse_seg', 'fake_edges', 'real_edges')})
    I.update({k: (r(Bn, 1, Hn, Wn) > 0.5).double() for k in ('mask', 'real_B_mask', 'normal_vert')})
    I['pred1'], I['pred2'] = r(Bn, 1), r(Bn, 1)
    I['height'] = torch.tensor([20, 24, 31][:Bn])
    I['maxheight'] = torch.tensor([40, 48, 36][:Bn])
    return I


@pytest.mark.parametrize('grad_scale', [0.0, 1.0, 1024.0])
def test_generator_losses_ref_matches_the_restated_step(grad_scale):
    """oracle/restate.py::_pix2pix_step_phases, the generator's loss lines, in fp64 with restate.dice_coeff.  Its `W * W / cnt` divides by an integer
    tensor, which gives the DEFAULT floating type: the lines run under a float64 default, as a double-precision run of the restated step would."""
    I = loss_batch(11)
    torch.set_default_dtype(torch.float64)
    try:
        _check_generator_losses_ref(I, grad_scale)
    finally:
        torch.set_default_dtype(torch.float32)


def _check_generator_losses_ref(I, grad_scale):
    lam = 200.0
    leaves = ('fake_B', 'fake_B_coarse', 'fine_seg', 'coarse_seg', 'pred1', 'pred2')
    o = {k: (v.clone().requires_grad_(True) if k in leaves else v) for k, v in I.items()}
    p1h, p2h = o['pred1'].T * I['maxheight'], o['pred2'].T * I['maxheight']
    cnt = torch.count_nonzero(I['mask'])
    Wn = I['mask'].shape[-1]
    l_l1 = ((o['fake_B'] - I['real_B']).abs().mean() + (o['fake_B_coarse'] - I['real_B']).abs().mean()) * 0.5 * lam * (Wn * Wn / cnt) * 2
    l_cdice = (1 - restate.dice_coeff(o['coarse_seg'], I['normal_vert'])) * 10
    l_dice = (1 - restate.dice_coeff(o['fine_seg'], I['real_B_mask'])) * 15
    l_edge = F.mse_loss(I['fake_edges'], I['real_edges']) * 800
    hh = I['height']
    l_h = torch.mean((abs(p1h - hh) / hh) * 40 + (abs(p2h - hh) / hh) * 40)
    total = l_l1 + l_dice + l_edge + l_cdice + l_h
    total.backward()
    gan = torch.tensor([0.3, 0.7, 0.11], dtype=torch.float64)
    add = torch.randn(I['fake_B'].shape, dtype=torch.float64)
    ref = PR.generator_losses_ref(I, lam, grad_scale, gan_terms=gan, add_d_fake_B=add)
    close(ref['losses'], torch.stack([l_l1, l_dice, l_cdice, l_edge, l_h, total]).detach(), 'losses')
    close(ref['loss_G_GAN'], gan.sum(), 'loss_G_GAN')
    close(ref['loss_G'], total.detach() + gan.sum(), 'loss_G')
    gs = grad_scale if grad_scale > 0 else 1.0
    for k in leaves:
        want = o[k].grad * gs + (add if k == 'fake_B' else 0)
        close(ref['d_' + k], want, 'd_' + k)
    close(ref['pred1_h'], p1h.detach(), 'pred1_h')
    # the closed forms the device tests evaluate in fp32 for their error floors are the same seeds
    N, Bn = I['mask'].numel(), I['mask'].shape[0]
    coef = 0.5 * lam * (Wn * Wn / cnt.double()) * 2 / N
    close(PR.l1_seed_formula(coef, I['fake_B'], I['real_B'], gs) + add, ref['d_fake_B'], 'l1 seed formula')
    pf, gf = I['fine_seg'].reshape(Bn, -1), I['real_B_mask'].reshape(Bn, -1)
    A, Tt = (pf.sum(1) + gf.sum(1) + 1e-5).view(Bn, 1, 1, 1), (2 * (pf * gf).sum(1) + 1e-5).view(Bn, 1, 1, 1)
    close(PR.dice_seed_formula(I['real_B_mask'], A, Tt, 15.0, Bn, gs), ref['d_fine_seg'], 'dice seed formula')
    close(PR.height_seed_formula(ref['pred2_h'][0], hh.double(), I['maxheight'].double(), Bn, gs), ref['d_pred2'].view(-1), 'height seed formula')


def test_generator_losses_ref_has_a_zero_subgradient_at_ties():
    I = loss_batch(12)
    I['fake_B'][0, 0, 0, :4] = I['real_B'][0, 0, 0, :4]
    I['pred1'][1, 0] = 0.5
    I['height'][1], I['maxheight'][1] = 24, 48
    ref = PR.generator_losses_ref(I, 200.0, 1.0)
    assert bool((ref['d_fake_B'][0, 0, 0, :4] == 0).all()) and ref['d_pred1'][1, 0] == 0 and bool((ref['d_fake_B'][1] != 0).all())


def test_sobel_ref_matches_the_restated_sobel_and_fixture_g4():
    g = np.load(os.path.join(GOLD, 'g4_small_ops.npz'))
    for k in ('soft', 'm'):
        x = torch.from_numpy(g[k]).double()
        close(PR.sobel_ref(x), restate.sobel(x), 'sobel ' + k)
    got = PR.sobel_ref(torch.from_numpy(g['soft']).double())
    assert (got - torch.from_numpy(g['sobel_soft']).double()).abs().max().item() <= 2e-6      # the stored output is single precision
    assert (got == 1.0).any() and (got < 1.0).any()
    x = torch.randn(3, 1, 1, 9, dtype=torch.float64)      # H == 1: all three rows are the one row
    close(PR.sobel_ref(x), restate.sobel(x), 'sobel H=1')
    x = torch.randn(2, 1, 5, 1, dtype=torch.float64)
    close(PR.sobel_ref(x), restate.sobel(x), 'sobel W=1')


def test_post_generator_ref_reproduces_fixture_g12():
    from oracle.make_golden_shrm import build_inputs
    g = np.load(os.path.join(GOLD, 'g12_shrm.npz'))
    I = build_inputs()
    I['fine_seg'], I['coarse_seg'] = I['fine'], I['coarse']
    o = PR.post_generator_ref(I, 35)
    names = dict(fake_B='fake_B', fake_B_coarse='fake_B_coarse', fake_B_local='fake_B_local', real_B_local='real_B_local', fine_bin='fake_B_mask_raw',
                 coarse_bin='coarse_seg_binary')
    for k, rk in names.items():
        assert np.array_equal(o[k].numpy()[..., ::4], g['res::' + rk]), k
    assert np.array_equal(o['pred1_h'].numpy(), g['res::pred1_h']) and np.array_equal(o['pred2_h'].numpy(), g['res::pred2_h'])
    for i in range(8):      # the generated rows are where fake_B differs from real_B's pattern: read the bounds back from the composited image
        xu, xb = int(o['rows'][i, 0]), int(o['rows'][i, 1])
        assert torch.equal(o['fake_B'][i, :, xu:xb], I['x_stage2'][i, :, xu:xb]) and xb - xu >= int(I['height'][i])


@pytest.mark.parametrize('which', [0, 1])
def test_shrm_backward_ref_is_the_row_and_band_selection(which):
    Bn, Hn, Wn, half = 3, 6, 7, 3
    rows = torch.tensor([[0, 3, 2, 6], [1, 1, 0, 6], [2, 6, 3, 3]], dtype=torch.int32)
    d_fake, d_local = torch.randn(Bn, 1, Hn, Wn, dtype=torch.float64), torch.randn(Bn, 1, Hn, Wn, dtype=torch.float64)
    mask = (torch.rand(Bn, 1, Hn, Wn, dtype=torch.float64) > 0.4).double()
    want = torch.zeros_like(d_fake)
    for b in range(Bn):
        xu, xb = int(rows[b, 2 * which]), int(rows[b, 2 * which + 1])
        want[b, :, xu:xb] = d_fake[b, :, xu:xb]
        want[b, :, xu:xb, 0:6] += (d_local * mask)[b, :, xu:xb, 0:6]
    close(PR.shrm_backward_ref(d_fake, d_local, mask, rows, which, half), want, 'both')
    assert torch.equal(PR.shrm_backward_ref(None, None, mask, rows, which, half), torch.zeros_like(want))
    only = PR.shrm_backward_ref(d_fake, None, None, rows, which, half)
    close(only + PR.shrm_backward_ref(None, d_local, mask, rows, which, half), want, 'sum of the parts')
    assert torch.equal(PR.shrm_backward_ref(d_fake, d_local, mask, rows, which, 0), only)      # an empty band


@pytest.mark.parametrize('act', [None] + list(PR.ACTS))
def test_gap_fc_refs_match_autograd(act):
    Bn, HW, Cn = 3, 7, 5
    for seed in range(200):
        gen = torch.Generator().manual_seed(seed)
        pre = torch.randn(Bn, HW, Cn, generator=gen, dtype=torch.float64) * 1.5
        if away_from_kinks(pre):
            break
    w, b = torch.randn(Cn, generator=gen, dtype=torch.float64), torch.randn((), generator=gen, dtype=torch.float64)
    dpred = torch.randn(Bn, generator=gen, dtype=torch.float64)
    pa, wa, ba = pre.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    xa = pa if act is None else torch_act(pa, act)
    tpooled = xa.mean(dim=1)
    tpred = torch.sigmoid(tpooled @ wa + ba)
    (tpred * dpred).sum().backward()
    x = xa.detach()
    pooled, pred = PR.gap_fc_sigmoid_ref(x, w, b)
    close(pooled, tpooled.detach(), 'pooled')
    close(pred, tpred.detach(), 'pred')
    dx, dw, db = PR.gap_fc_sigmoid_backward_ref(dpred, pred, pooled, w, HW, None if act is None else x, act or 'none')
    close(dx, pa.grad, 'dx')
    close(dw, wa.grad, 'dw')
    close(db, ba.grad, 'db')


def test_copy_modes_are_adjoint_pairs():
    gen = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    Bn, Cn, Hn, Wn = 2, 3, 4, 6
    for m, mt in ((1, 3), (2, 4), (0, 0)):
        hs, ws = PR.copy_src_size(m, Hn, Wn)
        x, y = r(Bn, Cn, hs, ws), r(Bn, Cn, Hn, Wn)
        fx, fty = PR.copy_channels_ref(x, m), PR.copy_channels_ref(y, mt)
        assert fx.shape == y.shape and fty.shape == x.shape and PR.copy_src_size(mt, hs, ws) == (Hn, Wn)
        close((fx * y).sum(), (x * fty).sum(), 'adjoint %d %d' % (m, mt))
    x = r(1, 1, 2, 2)
    assert torch.equal(PR.copy_channels_ref(x, 1)[0, 0], torch.tensor([[x[0, 0, 0, 0]] * 2 + [x[0, 0, 0, 1]] * 2] * 2 + [[x[0, 0, 1, 0]] * 2 + [x[0, 0, 1, 1]] * 2] * 2))
    odd = r(1, 1, 6, 10)
    assert torch.equal(PR.copy_channels_ref(odd, 2), odd[:, :, ::2, ::2]) and PR.copy_channels_ref(odd, 2).shape == (1, 1, 3, 5)


def test_glue_and_small_operator_refs():
    gen = torch.Generator().manual_seed(4)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    x = r(2, 3, 4, 5)
    assert torch.equal(PR.nhwc_to_nchw_ref(PR.nchw_to_nhwc_ref(x)), x) and PR.nchw_to_nhwc_ref(x)[1, 2, 3, 1] == x[1, 1, 2, 3]
    assert torch.equal(PR.add_channels_ref(x, 2 * x), 3 * x)
    p, seg, mask = r(2, 1, 3, 4), r(2, 1, 3, 4), r(2, 1, 3, 4)
    ratio = torch.tensor([0.1, 1 / 3], dtype=torch.float64)
    rp = restate._ratio_plane(p, ratio).double()
    g0, g1 = PR.gen_input_ref(p, None, mask, ratio, 8, 0), PR.gen_input_ref(p, seg, mask, ratio, 4, 1)
    assert torch.equal(g0[..., :3], torch.cat([p, rp, mask], 1).permute(0, 2, 3, 1)) and bool((g0[..., 3:] == 0).all())
    assert torch.equal(g1, torch.cat([p, seg, mask, rp], 1).permute(0, 2, 3, 1)) and bool((rp[1] != 1 / 3).all())
    y, z = r(9), r(9)
    xs = r(9)
    assert torch.equal(PR.axpy_formula(y, xs, 0.5), y + 0.5 * xs) and torch.equal(PR.affine_formula(xs, -1.0, 1.0), 1 - xs)
    assert torch.equal(PR.mul_formula(y, xs), y * xs) and torch.equal(PR.mul3_formula(y, xs, z), y * xs * z)
    t = torch.tensor([0.25, 0.5, 0.75], dtype=torch.float64)
    assert PR.threshold_ref(t, 0.5, 3.0).tolist() == [0.0, 0.0, 3.0] and PR.fill_ref(3, 2.0).tolist() == [2.0] * 3
