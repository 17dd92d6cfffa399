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
