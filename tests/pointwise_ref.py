"""Plain references of the kernels between the convolutions: normalisation + activation (forward, backward), the in-place activation
gradient with its bias column sums, the 1-channel head seed and the GAN loss heads.  torch on the CPU, no device code.

Tensors are (B, C, H, W); statistics are [G][2][C] (mean, rstd).  The `*_ref` functions take and return fp64: the inputs are the STORED values
(fp32 or fp16 data converted exactly).  The `*_formula` functions evaluate one element-wise formula in the dtype of their arguments: the references
call them in fp64, the device tests call them in fp32 to measure what a plain fp32 evaluation of the same formula loses (their error floor).
tests/test_pointwise_ref_cpu.py pins all of it against torch autograd."""
import torch

ACTS = ('none', 'elu', 'relu', 'lrelu', 'sigmoid', 'clamp')


def act_formula(v, act):
    """hv_act."""
    if act == 'none':
        return v
    if act == 'elu':
        return torch.where(v > 0, v, torch.expm1(v))
    if act == 'relu':
        return torch.where(v > 0, v, torch.zeros_like(v))
    if act == 'lrelu':
        return torch.where(v > 0, v, 0.2 * v)
    if act == 'sigmoid':
        return 1 / (1 + torch.exp(-v))
    if act == 'clamp':
        return v.clamp(-1, 1)
    raise ValueError(act)


def act_grad_from_out_formula(y, act, post_sigmoid=False):
    """d(final output) / d(pre-activation) from the final output y (hv_act_grad_from_out; norm_act_bwd under post_sigmoid, where the activation's
    branch is read off y > 0.5 <=> act(v) > 0)."""
    one, zero = torch.ones_like(y), torch.zeros_like(y)
    if post_sigmoid:
        if act not in ('none', 'relu', 'lrelu'):      # the derivative of elu / sigmoid / clamp cannot be read off sigmoid's output by this rule
            raise ValueError('post_sigmoid with ' + act)
        ds = y * (1 - y)
        if act == 'relu':
            return ds * torch.where(y > 0.5, one, zero)
        if act == 'lrelu':
            return ds * torch.where(y > 0.5, one, 0.2 * one)
        return ds
    if act == 'none':
        return one
    if act == 'elu':
        return torch.where(y > 0, one, y + 1)
    if act == 'relu':
        return torch.where(y > 0, one, zero)
    if act == 'lrelu':
        return torch.where(y > 0, one, 0.2 * one)
    if act == 'sigmoid':
        return y * (1 - y)
    if act == 'clamp':
        return torch.where((y > -1) & (y < 1), one, zero)
    raise ValueError(act)


def _bc(p):      # [C] -> (1, C, 1, 1)
    return p.view(1, -1, 1, 1)


def norm_apply_formula(x, mean, rstd, gamma, beta, act, post_sigmoid):
    """y of one group: x (b, C, H, W); mean, rstd, gamma, beta [C] (gamma None: no affine)."""
    v = (x - _bc(mean)) * _bc(rstd)
    if gamma is not None:
        v = v * _bc(gamma) + _bc(beta)
    v = act_formula(v, act)
    return 1 / (1 + torch.exp(-v)) if post_sigmoid else v


def norm_bwd_apply_formula(g, x, mean, rstd, gamma, sum_g, sum_gx, R, batch_stats):
    """dx of one group from g = dy * act'(y): sum_g, sum_gx [C] are the group's sums of g and g * xhat over its R rows."""
    gr = _bc(rstd) if gamma is None else _bc(gamma) * _bc(rstd)
    if not batch_stats:
        return gr * g
    xhat = (x - _bc(mean)) * _bc(rstd)
    inv = 1.0 / R
    return gr * (g - _bc(sum_g) * inv - xhat * _bc(sum_gx) * inv)


def group_slices(B, norm, groups):
    """The batch rows of each statistics group: instance norm one image each, batch norm `groups` equal shares in order."""
    G = B if norm == 'instance' else max(int(groups), 1)
    per = B // G
    assert per * G == B
    return [slice(g * per, (g + 1) * per) for g in range(G)]


def norm_act_forward_ref(x, norm, training, gamma, beta, running_mean, running_var, eps, momentum, groups, act, post_sigmoid):
    """-> y, stats [G][2][C], running_mean, running_var, num_batches_tracked (the number of updates: add it to the counter's value before).
    Batch-norm groups are visited in order and each updates the running statistics, as consecutive forward calls on each share would."""
    assert x.dtype == torch.float64
    B, C, H, W = x.shape
    sl = group_slices(B, norm, groups)
    use_running = norm == 'batch' and not training
    rm = None if running_mean is None else running_mean.clone()
    rv = None if running_var is None else running_var.clone()
    nbt = 0
    y = torch.empty_like(x)
    stats = torch.empty(len(sl), 2, C, dtype=torch.float64)
    for g, s in enumerate(sl):
        xs = x[s]
        R = xs.shape[0] * H * W
        if use_running:
            mean, rstd = rm.clone(), 1 / torch.sqrt(rv + eps)
        else:
            mean = xs.sum(dim=(0, 2, 3)) / R
            var = ((xs - _bc(mean)) ** 2).sum(dim=(0, 2, 3)) / R        # two-pass, biased
            rstd = 1 / torch.sqrt(var + eps)
            if norm == 'batch' and training and rm is not None:
                unb = var * R / (R - 1) if R > 1 else var
                rm = (1 - momentum) * rm + momentum * mean
                rv = (1 - momentum) * rv + momentum * unb
                nbt += 1
        stats[g, 0], stats[g, 1] = mean, rstd
        affine = norm == 'batch'
        y[s] = norm_apply_formula(xs, mean, rstd, gamma if affine else None, beta if affine else None, act, post_sigmoid)
    return y, stats, rm, rv, nbt


def norm_backward_terms(dy, y, x, stats, norm, groups, act, post_sigmoid):
    """-> g = dy * act'(y) and xhat = (x - mean) * rstd, both (B, C, H, W), with every group's own statistics."""
    g = dy * act_grad_from_out_formula(y, act, post_sigmoid) if (act != 'none' or post_sigmoid) else dy.clone()      # act none: y is not read
    xhat = torch.empty_like(x)
    for k, s in enumerate(group_slices(x.shape[0], norm, groups)):
        xhat[s] = (x[s] - _bc(stats[k, 0])) * _bc(stats[k, 1])
    return g, xhat


def norm_act_backward_ref(dy, y, x, stats, gamma, norm, training, groups, act, post_sigmoid):
    """-> dx, dgamma, dbeta (the sums over all groups; instance norm has no affine: they are the sums at gamma = 1).  The activation derivative is
    taken from the given y.  Eval batch norm: dx = gamma * rstd * g."""
    assert dy.dtype == torch.float64
    B, C, H, W = x.shape
    g, xhat = norm_backward_terms(dy, y, x, stats, norm, groups, act, post_sigmoid)
    batch_stats = norm == 'instance' or bool(training)
    dx = torch.empty_like(x)
    for k, s in enumerate(group_slices(B, norm, groups)):
        R = (s.stop - s.start) * H * W
        sg, sgx = g[s].sum(dim=(0, 2, 3)), (g[s] * xhat[s]).sum(dim=(0, 2, 3))
        dx[s] = norm_bwd_apply_formula(g[s], x[s], stats[k, 0], stats[k, 1], gamma if norm == 'batch' else None, sg, sgx, R, batch_stats)
    return dx, (g * xhat).sum(dim=(0, 2, 3)), g.sum(dim=(0, 2, 3))


def act_backward_ref(dy, y, act):
    """-> g = dy * act'(y) (B, C, H, W), dbias [C]."""
    g = dy * act_grad_from_out_formula(y, act)
    return g, g.sum(dim=(0, 2, 3))


def head_seed_ref(seed, y, act):
    """-> g = seed * act'(y) (what channel 0 of the carrier holds before its rounding to fp16)."""
    return seed * act_grad_from_out_formula(y, act)


def gan_loss_terms_formula(z, target_is_real, mode):
    """-> per-logit loss terms l_i and d l_i / d z_i.  vanilla: BCE with logits, written stably; lsgan: squared error."""
    t = 1.0 if target_is_real else 0.0
    if mode == 'vanilla':
        l = z.clamp(min=0) - z * t + torch.log1p(torch.exp(-z.abs()))
        e = torch.exp(-z.abs())
        sig = torch.where(z >= 0, 1 / (1 + e), e / (1 + e))
        return l, sig - t
    if mode == 'lsgan':
        return (z - t) ** 2, 2 * (z - t)
    raise ValueError(mode)


def gan_loss_ref(z, target_is_real, mode):
    """-> loss (mean over n), dz = d loss / d z."""
    assert z.dtype == torch.float64
    l, g = gan_loss_terms_formula(z, target_is_real, mode)
    return l.sum() / z.numel(), g / z.numel()
