"""Plain references of the kernels between the convolutions: normalisation + activation (forward, backward), the in-place activation
gradient with its bias column sums, the 1-channel head seed and the GAN loss heads; the generator loss tail (losses and seeds, SHRM compositing and its
gradient, Sobel), the pooled height head, the channel / layout glue and the small element-wise operators.  torch on the CPU, no device code.

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


# ---------------------------------------------------------------------------------------------------------------- generator loss tail
def generator_loss_terms(I, lambda_L1):
    """The five loss terms as differentiable fp64 scalars (G_maskL1, G_Dice, coarse_Dice, edge, h) of the tensors in I, `mag` [5] (see
    generator_losses_ref) and pred1_h / pred2_h (1, B)."""
    assert all(v.dtype == torch.float64 for k, v in I.items() if k not in ('height', 'maxheight'))
    B, W = I['mask'].shape[0], I['mask'].shape[-1]
    N = I['mask'].numel()
    hh, mh = I['height'], I['maxheight']
    p1h, p2h = I['pred1'].T * mh, I['pred2'].T * mh
    cnt = torch.count_nonzero(I['mask']).double()      # (int / integer tensor would be a single-precision quotient)
    scale = 0.5 * lambda_L1 * (W * W / cnt) * 2
    a1, a2 = (I['fake_B'] - I['real_B']).abs(), (I['fake_B_coarse'] - I['real_B']).abs()
    l_l1 = (a1.mean() + a2.mean()) * scale

    def dice(pred, gt, eps=1e-5):      # restate.dice_coeff, per sample
        p, g = pred.reshape(B, -1), gt.reshape(B, -1)
        return (2 * (g * p).sum(1) + eps) / (p.sum(1) + g.sum(1) + eps)

    qf, qc = dice(I['fine_seg'], I['real_B_mask']), dice(I['coarse_seg'], I['normal_vert'])
    l_dice, l_cdice = (1 - qf.sum() / B) * 15, (1 - qc.sum() / B) * 10
    e2 = (I['fake_edges'] - I['real_edges']) ** 2
    l_edge = e2.mean() * 800
    ht = (abs(p1h - hh) / hh) * 40 + (abs(p2h - hh) / hh) * 40
    l_h = torch.mean(ht)
    mag = torch.stack([(a1.sum() + a2.sum()) / N * scale, 2 * qf.sum() / B * 15, 2 * qc.sum() / B * 10, e2.sum() / N * 800, ht.sum() / B]).detach()
    return (l_l1, l_dice, l_cdice, l_edge, l_h), mag, p1h, p2h


def generator_losses_ref(inputs, lambda_L1, grad_scale, gan_terms=None, add_d_fake_B=None):
    """hv_generator_losses: the five generator losses of oracle/restate.py::_pix2pix_step_phases (the L1 pair with the mask-count scale, both Dice
    terms through dice_coeff, the edge term, the height term), their sum, loss_G_GAN / loss_G, and the six seeds = grad_scale (0 stands for 1, as the
    header says) x torch.autograd.grad of that fp64 sum wrt fake_B, fake_B_coarse, fine_seg, coarse_seg, pred1, pred2 (pred_h = pred * maxheight),
    plus add_d_fake_B on the first.  The edge maps are inputs: the edge term has no gradient.
    inputs (fp64; images (B, 1, H, W)): fake_B fake_B_coarse real_B mask fine_seg coarse_seg real_B_mask normal_vert fake_edges real_edges;
    pred1 pred2 (B, 1); height maxheight (B,).
    -> dict: losses [6], loss_G_GAN, loss_G, d_fake_B .. d_pred2, pred1_h / pred2_h (1, B), and `mag` [5]: the sum of |terms| x scale of every loss
    (what a summation error of the loss is relative to; for a Dice quotient numerator and denominator both carry one: twice the quotients)."""
    I = {k: v.detach().clone() for k, v in inputs.items()}
    leaves = ('fake_B', 'fake_B_coarse', 'fine_seg', 'coarse_seg', 'pred1', 'pred2')
    for k in leaves:
        I[k].requires_grad_(True)
    B = I['mask'].shape[0]
    l, mag, p1h, p2h = generator_loss_terms(I, lambda_L1)
    l_l1, l_dice, l_cdice, l_edge, l_h = l
    total = l_l1 + l_dice + l_cdice + l_edge + l_h
    grads = torch.autograd.grad(total, [I[k] for k in leaves])
    gs = float(grad_scale) if grad_scale > 0 else 1.0
    out = {'d_' + k: g * gs for k, g in zip(leaves, grads)}
    if add_d_fake_B is not None:
        out['d_fake_B'] = out['d_fake_B'] + add_d_fake_B
    out['losses'] = torch.stack([l_l1, l_dice, l_cdice, l_edge, l_h, total]).detach()
    out['mag'] = mag
    out['pred1_h'], out['pred2_h'] = p1h.detach(), p2h.detach()
    if gan_terms is not None:
        out['loss_G_GAN'] = gan_terms.sum()
        out['loss_G'] = out['losses'][5] + out['loss_G_GAN']
    return out


def l1_seed_formula(coef_l1, fake, real, gs):
    """d_fake_B / d_fake_B_coarse before add_d_fake_B: coef_l1 = scale / N of the loss reference, in the dtype of the arguments."""
    e = fake - real
    return (coef_l1 * gs) * torch.sign(e)


def dice_seed_formula(gt, A, T, weight, B, gs):
    """d_fine_seg (weight 15) / d_coarse_seg (weight 10) from the per-sample A = sum p + sum g + eps and T = 2 sum g p + eps ((B, 1, 1, 1)), in the dtype
    of the arguments."""
    return -weight * (gs / B) * (2 * gt * A - T) / (A * A)


def height_seed_formula(pred_h, height, maxheight, B, gs):
    """d_pred1 / d_pred2 [B] from pred_h [B]."""
    return gs * (40 * torch.sign(pred_h - height) / height * maxheight / B)


def rows_to_composite_args(rows2):
    """(xu, xb) [B][2] -> (pred_h, height, x1, x2) at which restate.shrm_rows gives these bounds (no growth: h = height = xb - xu)."""
    xu, xb = rows2[:, 0].long(), rows2[:, 1].long()
    return torch.zeros(len(xu), dtype=torch.float64), xb - xu, xu, xb


def shrm_backward_ref(d_fake, d_local, mask, rows, which, half_band):
    """hv_shrm_backward: torch.autograd.grad of <d_fake, fake> + <d_local, mask * fake * center_band> wrt the generated image, fake =
    restate.shrm_composite at the row bounds rows[b][2 which .. 2 which + 1].  d_fake / d_local None: that term is absent.  half_band <= W // 2 (the
    restated band is a slice)."""
    from oracle import restate
    ref = d_fake if d_fake is not None else d_local
    gen = torch.zeros_like(ref if ref is not None else mask, dtype=torch.float64).requires_grad_(True)
    assert half_band <= gen.shape[3] // 2
    ph, hh, x1, x2 = rows_to_composite_args(rows[:, 2 * which:2 * which + 2])
    fake = restate.shrm_composite(gen, torch.zeros_like(gen), ph, hh, x1, x2)
    tot = (fake * 0).sum()
    if d_fake is not None:
        tot = tot + (d_fake * fake).sum()
    if d_local is not None:
        tot = tot + (d_local * (mask * fake * restate.center_band(mask, half_band))).sum()
    return torch.autograd.grad(tot, gen)[0]


def post_generator_ref(I, half_band):
    """hv_post_generator from restate.shrm_rows / shrm_composite / center_band: I holds real_B mask x_stage1 x_stage2 fine_seg coarse_seg (B, 1, H, W),
    pred1 pred2 (B, 1), height x1 x2 maxheight (B,) int64.  pred_h is the fp32 product pred * maxheight (the value the reference's ceil sees); everything
    else is a selection, a product with 0 / 1 or a threshold, in the dtype of the images.  -> dict with rows [B][4] = {xu2, xb2, xu1, xb1}."""
    from oracle import restate
    o = {}
    dt = I['real_B'].dtype
    o['pred1_h'] = I['pred1'].float().T * I['maxheight'].float()
    o['pred2_h'] = I['pred2'].float().T * I['maxheight'].float()
    o['fine_bin'] = (I['fine_seg'] > 0.5).to(dt)
    o['coarse_bin'] = (I['coarse_seg'] > 0.5).to(dt)
    o['fake_B'] = restate.shrm_composite(I['x_stage2'], I['real_B'], o['pred2_h'][0], I['height'], I['x1'], I['x2'])
    o['fake_B_coarse'] = restate.shrm_composite(I['x_stage1'], I['real_B'], o['pred1_h'][0], I['height'], I['x1'], I['x2'])
    mc = restate.center_band(I['mask'], half_band)
    o['fake_B_local'] = I['mask'] * o['fake_B'] * mc
    o['real_B_local'] = I['mask'] * I['real_B'] * mc
    rows = []
    for i in range(I['real_B'].shape[0]):
        _, xu2, xb2, _ = restate.shrm_rows(o['pred2_h'][0, i], I['height'][i], I['x1'][i])
        _, xu1, xb1, _ = restate.shrm_rows(o['pred1_h'][0, i], I['height'][i], I['x1'][i])
        rows.append([xu2, xb2, xu1, xb1])
    o['rows'] = torch.tensor(rows, dtype=torch.int32)
    return o


def sobel_ref(img):
    """hv_sobel: 3x3 Sobel pair over the replicate-padded image, magnitude clamped at 1; (B, 1, H, W) in, same out, in the dtype of img."""
    p = torch.nn.functional.pad(img, (1, 1, 1, 1), mode='replicate')
    H, W = img.shape[2], img.shape[3]
    s = lambda dh, dw: p[:, :, dh:dh + H, dw:dw + W]
    a, b, c, d, f, g, hh, k = s(0, 0), s(0, 1), s(0, 2), s(1, 0), s(1, 2), s(2, 0), s(2, 1), s(2, 2)
    gx = (c - a) + 2 * (f - d) + (k - g)
    gy = (a + 2 * b + c) - (g + 2 * hh + k)
    return torch.sqrt(gx * gx + gy * gy).clamp(max=1.0)


# ---------------------------------------------------------------------------------------------------------------- pooled height head
def gap_fc_sigmoid_ref(x, w, b):
    """x (B, HW, C), w [C], b scalar -> pooled (B, C) = mean over HW, pred [B] = sigmoid(pooled . w + b)."""
    pooled = x.mean(dim=1)
    return pooled, 1 / (1 + torch.exp(-(pooled @ w + b)))


def gap_fc_sigmoid_backward_ref(dpred, pred, pooled, w, HW, mul_out=None, mul_act='none'):
    """Backward of mean-pool -> fc -> sigmoid from the stored pred [B] and pooled (B, C): -> the increment of dx (B, HW, C), dw [C], db.  mul_out
    (B, HW, C): the pooled tensor is act(pre) and mul_out its stored value; the increment is then the gradient wrt pre (act' read off the output)."""
    dl = dpred * pred * (1 - pred)
    dx = (dl.view(-1, 1, 1) * w.view(1, 1, -1) / HW).expand(-1, HW, -1)
    if mul_out is not None:
        dx = dx * act_grad_from_out_formula(mul_out, mul_act)
    return dx.contiguous(), (dl.view(-1, 1) * pooled).sum(dim=0), dl.sum()


# ---------------------------------------------------------------------------------------------------------------- channel glue
def copy_channels_ref(src, mode):
    """hv_copy_channels without its accumulate: src (B, C, Hs, Ws) -> what is stored (or added) at the destination size.  0 same size; 1 nearest x2 up;
    2 even indices of a double-size source; 3 sum of the 2x2 block of a double-size source (in the order (0,0), (0,1), (1,0), (1,1)); 4 the source at the
    even indices of a double-size destination, zero elsewhere."""
    if mode == 0:
        return src.clone()
    if mode == 1:
        return src.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    if mode == 2:
        return src[:, :, ::2, ::2].clone()
    if mode == 3:
        return ((src[:, :, 0::2, 0::2] + src[:, :, 0::2, 1::2]) + src[:, :, 1::2, 0::2]) + src[:, :, 1::2, 1::2]
    if mode == 4:
        out = torch.zeros(src.shape[0], src.shape[1], 2 * src.shape[2], 2 * src.shape[3], dtype=src.dtype)
        out[:, :, ::2, ::2] = src
        return out
    raise ValueError(mode)


def copy_src_size(mode, H, W):
    """Source size of a copy whose destination is H x W."""
    return {0: (H, W), 1: (H // 2, W // 2), 2: (2 * H, 2 * W), 3: (2 * H, 2 * W), 4: (H // 2, W // 2)}[mode]


def add_channels_ref(a, b):
    return a + b


def gen_input_ref(x, seg, mask, slice_ratio, CP, order):
    """hv_gen_input: (B, 1, H, W) planes and slice_ratio [B] (double) -> (B, H, W, CP): order 0 [x, ratio, mask, 0..], order 1 [x, seg, mask, ratio, 0..];
    the ratio plane is the double rounded to fp32 (restate._ratio_plane)."""
    r = slice_ratio.float().to(x.dtype).view(-1, 1, 1, 1).expand_as(x)
    planes = [x, r, mask] if order == 0 else [x, seg, mask, r]
    out = torch.zeros(x.shape[0], x.shape[2], x.shape[3], CP, dtype=x.dtype)
    for c, p in enumerate(planes):
        out[..., c] = p[:, 0]
    return out


def nchw_to_nhwc_ref(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nhwc_to_nchw_ref(x):
    return x.permute(0, 3, 1, 2).contiguous()


# ---------------------------------------------------------------------------------------------------------------- small operators
def fill_ref(n, value, dtype=torch.float64):
    return torch.full((n,), value, dtype=dtype)


def axpy_formula(y, x, a):
    return y + a * x


def affine_formula(x, a, b):
    return a * x + b


def mul_formula(y, x):
    return y * x


def mul3_formula(y, x, z):
    return (y * x) * z


def threshold_ref(x, thr, value):
    return torch.where(x > thr, torch.full_like(x, value), torch.zeros_like(x))
