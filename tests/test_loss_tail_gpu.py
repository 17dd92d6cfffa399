"""The rest of csrc/pointwise.hip and the small operators of csrc/prep.hip against the fp64 references of tests/pointwise_ref.py (pinned by
tests/test_pointwise_ref_cpu.py): hv_generator_losses (partial / finalize incl. the B > 64 spill path / seeds), hv_shrm_backward, the chain
post_generator -> sobel x 2 -> generator_losses -> shrm_backward, the pooled height head and its backward, hv_copy_channels, hv_add_channels, hv_gen_input,
the layout pair, hv_sobel, hv_post_generator and hv_fill / hv_axpy / hv_affine / hv_mul / hv_mul3 / hv_threshold.

The C entries are called through lib.get().call on hvtest.Guarded buffers (NaN around every buffer and in every output before the call); intact() is
asserted after every call, and the channels around a view hold a sentinel that has to survive.  hv_generator_losses and hv_gap_fc_sigmoid get exactly
the queried workspace bytes inside a guarded buffer.

Bounds (tests/test_norm_act_gpu.py's rules; u = 2^-24), all from fp64 reference quantities, never from the kernel's output:
  exact outputs         copies, products with 0 / 1, thresholds, layout changes, rows: the bits, after round-to-nearest-even where the store is fp16;
  element-wise values   4 x (the largest error of a plain fp32 CPU evaluation of the same formula) + 4u |ref|, + max(2^-11 |ref|, 2^-25) where the store
                        is fp16, + 2^-11 |ref| more where the kernel adds to an fp16 value;
  loss scalars          64u x scale x sum |terms| + u |ref| (per-thread fp32 sums, then double); a Dice quotient carries that in numerator and
                        denominator (twice the quotients); the sum of the five adds the five bounds and 4u sum |l_k| for its own fp32 additions;
  Dice seeds            the element-wise rule, the floor from an fp32 evaluation on the fp64 A and T rounded to fp32;
  pooled mean           (ceil(log2 HW) + 16) u mean |x|; pred: that, times |w_c| summed over the channels and the sigmoid's derivative, + 4u |ref| for
                        the fp32 sigmoid; dw, db: 16u sum |terms| + u |ref|.
Signs and thresholds are decided on the same stored fp32 values on both sides: fake - real and pred_h - height are fp32 differences of stored values,
whose sign is the exact one; pred * maxheight is chosen exact in fp32 (pred a multiple of 2^-10, maxheight <= 64) or >= 1e-3 away from an integer in
the chained check, where its fp32 product is the value both sides take the ceil of; the backward of the height head reads the stored pred, pooled and
activation output on both sides.  No element is left out of a comparison.  The worst error / bound ratio of every family is printed at the end; a
family whose store is fp16 (tail.copy, tail.add; tail.gap_dx with two such terms) comes out near 1 (near 0.5): the conversion's own error reaches
half an fp16 ulp and that half ulp is nearly the whole bound, so the ratio measures the rounding, not a margin of the kernel.
Left out: the i >= 2^31 branch of pw_div (an 8 GB tensor) and a mask without a non-zero element (the reference divides by zero as well)."""
import ctypes
import functools
import math

import pytest
import torch

import pointwise_ref as PR
from test_norm_act_gpu import Check, U, dtype_of, print_ratios, same_bits, tol_elem

pytestmark = pytest.mark.gpu

SENT = 7.5
T = lib = L = None
IMG = ('fake_B', 'fake_B_coarse', 'real_B', 'mask', 'fine_seg', 'coarse_seg', 'real_B_mask', 'normal_vert', 'fake_edges', 'real_edges')


@pytest.fixture(scope='module', autouse=True)
def _env():
    global T, lib, L
    import hvgan  # noqa: F401
    from hvgan import lib as _lib
    import hvtest as _T
    T, lib = _T, _lib
    L = _lib.get()
    yield
    print_ratios('tail.')


class Pool:
    """The guarded buffers of one call."""

    def __init__(self):
        self.all = []

    def put(self, data, dtype=None, offset=0):
        g = T.Guarded(tuple(data.shape), dtype or data.dtype, data=data, offset=offset)
        self.all.append(g)
        return g

    def out(self, shape, dtype=torch.float32):
        g = T.Guarded(shape, dtype)
        self.all.append(g)
        return g

    def intact(self):
        torch.cuda.synchronize()
        return all(g.intact() for g in self.all)


def p_(g):
    return None if g is None else lib.ptr(g.t)


def half_ulp16(ref):
    return 2.0 ** -11 * ref.abs()


def rnd(gen, *shape):
    return torch.rand(*shape, generator=gen)


# ---------------------------------------------------------------------------------------------------------------- hv_generator_losses
@functools.lru_cache(maxsize=None)
def gloss_inputs(B, H, W):
    """fp32 inputs.  Ties fake_B == real_B at every flat index = 2 mod 5 (fake_B_coarse: 3 mod 7); the mask holds zeros and non-zero values other than 1
    and is non-zero at the first pixel; height, maxheight and (through the mask) the count differ per sample; pred * maxheight is exact in fp32 and
    pred1_h == height in sample 0."""
    gen = torch.Generator().manual_seed(B * 10007 + H * 101 + W)
    n = B * H * W
    I = {k: rnd(gen, B, 1, H, W) * 2 - 1 for k in ('fake_B', 'fake_B_coarse', 'real_B')}
    idx = torch.arange(n)
    I['fake_B'].view(-1)[idx % 5 == 2] = I['real_B'].view(-1)[idx % 5 == 2]
    I['fake_B_coarse'].view(-1)[idx % 7 == 3] = I['real_B'].view(-1)[idx % 7 == 3]
    m = rnd(gen, B, 1, H, W)
    I['mask'] = torch.where(m > 0.5, m, torch.zeros_like(m))
    I['mask'][0, 0, 0, 0] = 1.0
    for k in ('fine_seg', 'coarse_seg', 'fake_edges', 'real_edges'):
        I[k] = rnd(gen, B, 1, H, W)
    for k in ('real_B_mask', 'normal_vert'):
        I[k] = (rnd(gen, B, 1, H, W) > 0.5).float()
    b = torch.arange(B)
    I['height'] = 20 + b % 11
    I['maxheight'] = 40 + 4 * (b % 5)
    I['pred1'] = (((b * 37 + 200) % 1024).float() / 1024).view(B, 1)
    I['pred2'] = (((b * 101 + 700) % 1024).float() / 1024).view(B, 1)
    I['pred1'][0, 0] = 0.5      # 0.5 * 40 == 20 == height[0]
    return I


def gloss_case(ck, B, H, W, gs, with_extras, image_seeds=True, pred_seeds=True, lam=200.0):
    what = 'B=%d H=%d W=%d gs=%g extras=%d img=%d pred=%d' % (B, H, W, gs, with_extras, image_seeds, pred_seeds)
    I = gloss_inputs(B, H, W)
    gen = torch.Generator().manual_seed(5)
    gan = torch.tensor([0.3, -0.7, 0.11]) if with_extras else None
    add = torch.randn(B, 1, H, W, generator=gen) * (gs if gs > 0 else 1.0) * 1e-3 if (with_extras and image_seeds) else None
    I64 = {k: (v.double() if v.is_floating_point() else v) for k, v in I.items()}
    ref = PR.generator_losses_ref(I64, lam, gs, gan_terms=None if gan is None else gan.double(), add_d_fake_B=None if add is None else add.double())
    p1h, p2h = ref['pred1_h'].float(), ref['pred2_h'].float()
    assert torch.equal(p1h.double(), ref['pred1_h']) and torch.equal(p2h.double(), ref['pred2_h']), 'test inputs: pred * maxheight not exact in fp32'
    assert ref['pred1_h'][0, 0] == I['height'][0]

    pool = Pool()
    d = L.hv_gloss_desc()
    bufs = {k: pool.put(I[k]) for k in IMG}
    bufs['pred1_h'], bufs['pred2_h'] = pool.put(p1h), pool.put(p2h)
    bufs['height'], bufs['maxheight'] = pool.put(I['height']), pool.put(I['maxheight'])
    outs = {'losses': pool.out(6)}
    if image_seeds:
        outs.update({k: pool.out((B, 1, H, W)) for k in ('d_fake_B', 'd_fake_B_coarse', 'd_fine_seg', 'd_coarse_seg')})
    if pred_seeds:
        outs.update({k: pool.out((B, 1)) for k in ('d_pred1', 'd_pred2')})
    if with_extras:
        bufs['gan_terms'] = pool.put(gan)
        outs['loss_G_GAN'], outs['loss_G'] = pool.out(1), pool.out(1)
        d.n_gan_terms = 3
        if add is not None:
            bufs['add_d_fake_B'] = pool.put(add)
    for k, g in list(bufs.items()) + list(outs.items()):
        setattr(d, k, lib.ptr(g.t).value)
    d.lambda_L1, d.B, d.H, d.W, d.grad_scale = lam, B, H, W, gs
    need = L.size('hv_generator_losses_workspace_bytes', B)
    assert need % 4 == 0
    ws = pool.out(need // 4)
    d.workspace, d.workspace_bytes = lib.ptr(ws.t).value, need
    L.call('hv_generator_losses', ctypes.byref(d), lib.stream())
    ck.true(pool.intact(), 'guards: ' + what)
    for k in IMG:
        ck.true(same_bits(bufs[k].cpu(), I[k]), 'input %s changed: %s' % (k, what))

    # ---- losses
    lo = outs['losses'].cpu().double()
    lb = 64 * U * ref['mag'] + U * ref['losses'][:5].abs()
    ck.le('tail.loss', (lo[:5] - ref['losses'][:5]).abs(), lb, what)
    sb = lb.sum() + 4 * U * ref['losses'][:5].abs().sum()
    ck.le('tail.loss', (lo[5] - ref['losses'][5]).abs(), sb, 'sum: ' + what)
    if with_extras:
        gb = 64 * U * gan.double().abs().sum()
        ck.le('tail.loss', (outs['loss_G_GAN'].cpu().double()[0] - ref['loss_G_GAN']).abs(), gb, 'loss_G_GAN: ' + what)
        ck.le('tail.loss', (outs['loss_G'].cpu().double()[0] - ref['loss_G']).abs(), sb + gb + U * ref['loss_G'].abs(), 'loss_G: ' + what)

    # ---- seeds
    g1 = gs if gs > 0 else 1.0
    N = B * H * W
    if image_seeds:
        cnt = torch.count_nonzero(I['mask']).double()
        coef32 = (0.5 * lam * (W * W / cnt) * 2 / N).float()
        gs32 = torch.tensor(g1, dtype=torch.float32)
        for k, src in (('d_fake_B', 'fake_B'), ('d_fake_B_coarse', 'fake_B_coarse')):
            e32 = PR.l1_seed_formula(coef32, I[src], I['real_B'], gs32)
            if k == 'd_fake_B' and add is not None:
                e32 = e32 + add
            floor = (e32.double() - ref[k]).abs().max().item()
            ck.le('tail.l1seed', (outs[k].cpu().double() - ref[k]).abs(), tol_elem(ref[k], floor, False), k + ': ' + what)
        for k, p, g, wgt in (('d_fine_seg', 'fine_seg', 'real_B_mask', 15.0), ('d_coarse_seg', 'coarse_seg', 'normal_vert', 10.0)):
            pf, gf = I64[p].reshape(B, -1), I64[g].reshape(B, -1)
            A = (pf.sum(1) + gf.sum(1) + 1e-5).view(B, 1, 1, 1)
            Tt = (2 * (pf * gf).sum(1) + 1e-5).view(B, 1, 1, 1)
            e32 = PR.dice_seed_formula(I[g], A.float(), Tt.float(), torch.tensor(wgt), B, gs32)
            floor = (e32.double() - ref[k]).abs().max().item()
            ck.le('tail.diceseed', (outs[k].cpu().double() - ref[k]).abs(), tol_elem(ref[k], floor, False), k + ': ' + what)
    if pred_seeds:
        for k, ph in (('d_pred1', p1h), ('d_pred2', p2h)):
            e32 = PR.height_seed_formula(ph[0], I['height'].float(), I['maxheight'].float(), torch.tensor(float(B)), torch.tensor(g1, dtype=torch.float32))
            r = ref[k].view(-1)
            floor = (e32.double() - r).abs().max().item()
            ck.le('tail.dpred', (outs[k].cpu().double().view(-1) - r).abs(), tol_elem(r, floor, False), k + ': ' + what)
        ck.true(outs['d_pred1'].cpu()[0, 0].item() == 0.0, 'd_pred1 at pred_h == height is not 0: ' + what)
    return outs


GLOSS_SHAPES = [(1, 1, 1), (2, 5, 7), (3, 8, 24), (2, 33, 31), (64, 8, 8), (65, 8, 8), (129, 4, 4), (1, 1, 32 * 256 * 4 + 3)]


@pytest.mark.parametrize('B,H,W', GLOSS_SHAPES, ids=['%dx%dx%d' % s for s in GLOSS_SHAPES])
def test_generator_losses(B, H, W):
    """Every shape with two of the three loss scales, once with gan_terms (n = 3) / add_d_fake_B and once without; (2, 5, 7) with all three scales in both
    forms, the losses-only call (no seed buffer at all) and the call without d_pred1 / d_pred2."""
    ck = Check()
    k = GLOSS_SHAPES.index((B, H, W))
    scales = (0.0, 1.0, 1024.0)
    gloss_case(ck, B, H, W, scales[k % 3], True)
    gloss_case(ck, B, H, W, scales[(k + 1) % 3], False)
    if (B, H, W) == (2, 5, 7):
        for gs in scales:
            for extras in (True, False):
                gloss_case(ck, B, H, W, gs, extras)
        full = gloss_case(ck, B, H, W, 1024.0, True)
        only = gloss_case(ck, B, H, W, 1024.0, True, image_seeds=False, pred_seeds=False)
        ck.true(same_bits(only['losses'].cpu(), full['losses'].cpu()) and same_bits(only['loss_G'].cpu(), full['loss_G'].cpu()), 'losses only: other bits')
        nop = gloss_case(ck, B, H, W, 1024.0, True, pred_seeds=False)
        ck.true(all(same_bits(nop[k_].cpu(), full[k_].cpu()) for k_ in ('d_fake_B', 'd_fake_B_coarse', 'd_fine_seg', 'd_coarse_seg', 'losses')),
                'no d_pred: other bits')
    ck.done()


def test_generator_losses_refuses_a_short_workspace():
    I = gloss_inputs(2, 5, 7)
    pool = Pool()
    d = L.hv_gloss_desc()
    for k in IMG:
        setattr(d, k, lib.ptr(pool.put(I[k]).t).value)
    for k in ('pred1_h', 'pred2_h'):
        setattr(d, k, lib.ptr(pool.put(torch.ones(1, 2)).t).value)
    d.height, d.maxheight = lib.ptr(pool.put(I['height']).t).value, lib.ptr(pool.put(I['maxheight']).t).value
    d.losses = lib.ptr(pool.out(6).t).value
    d.lambda_L1, d.B, d.H, d.W = 200.0, 2, 5, 7
    need = L.size('hv_generator_losses_workspace_bytes', 2)
    ws = pool.out(need // 4)
    d.workspace, d.workspace_bytes = lib.ptr(ws.t).value, need - 1
    with pytest.raises(RuntimeError, match='HV_ERR_WORKSPACE'):
        L.call('hv_generator_losses', ctypes.byref(d), lib.stream())
    assert pool.intact()


# ---------------------------------------------------------------------------------------------------------------- hv_shrm_backward
# (B, H, W, half_band, rows [B][4]): W odd; half_band == W // 2 puts the band's first column at 0, half_band 0 leaves it empty; rows with xu == 0, xb == H, xu == xb
SHRM_CASES = {
    'band_from_0': (3, 6, 7, 3, [[0, 3, 2, 6], [1, 1, 0, 6], [2, 6, 3, 3]]),
    'band_empty': (3, 6, 7, 0, [[0, 3, 2, 6], [1, 1, 0, 6], [2, 6, 3, 3]]),
    'band_inside': (2, 5, 9, 2, [[0, 5, 1, 4], [4, 5, 2, 2]]),
}


@pytest.mark.parametrize('which', [0, 1])
@pytest.mark.parametrize('case', sorted(SHRM_CASES))
def test_shrm_backward(case, which):
    B, H, W, half, rows = SHRM_CASES[case]
    ck = Check()
    rows = torch.tensor(rows, dtype=torch.int32)
    gen = torch.Generator().manual_seed(40 + which)
    d_fake, d_local, prior = (torch.randn(B, 1, H, W, generator=gen) for _ in range(3))
    mask = rnd(gen, B, 1, H, W)
    mask[:, :, ::2, ::3] = 0.0
    one = torch.ones(B, 1, H, W, dtype=torch.float64)
    sel = PR.shrm_backward_ref(one, None, None, rows, which, half).float()            # 0 / 1: the generated rows
    selb = PR.shrm_backward_ref(None, one, one, rows, which, half).float()             # 0 / 1: the generated rows inside the band
    ck.true(bool(sel.sum() > 0) and bool(selb.sum() > 0) == (half > 0) and (half != W // 2 or bool(selb[..., 0].sum() > 0)), 'test inputs: ' + case)
    for has_fake in (True, False):
        for has_local in (True, False):
            for acc in (0, 1):
                what = '%s which=%d fake=%d local=%d acc=%d' % (case, which, has_fake, has_local, acc)
                ref = PR.shrm_backward_ref(d_fake.double() if has_fake else None, d_local.double() if has_local else None, mask.double(), rows, which, half)
                g32 = (d_fake * sel if has_fake else torch.zeros_like(sel)) + ((d_local * mask) * selb if has_local else torch.zeros_like(sel))
                if acc:
                    ref, g32 = prior.double() + ref, prior + g32
                pool = Pool()
                bf, bl = (pool.put(d_fake) if has_fake else None), (pool.put(d_local) if has_local else None)
                bm, br = (pool.put(mask) if has_local else None), pool.put(rows)
                out = pool.put(prior) if acc else pool.out((B, 1, H, W))
                L.call('hv_shrm_backward', p_(bf), p_(bl), p_(bm), p_(br), which, p_(out), B, H, W, half, acc, lib.stream())
                ck.true(pool.intact(), 'guards: ' + what)
                got = out.cpu()
                if not has_local and not acc:
                    ck.true(same_bits(got, ref.float()), 'selection: other bits: ' + what)
                floor = (g32.double() - ref).abs().max().item()
                ck.le('tail.shrm_bwd', (got.double() - ref).abs(), tol_elem(ref, floor, False), what)
    ck.done()


# ---------------------------------------------------------------------------------------------------------------- post_generator and the chain
def call_post_generator(pool, I, B, H, W, half):
    d = L.hv_postg_desc()
    ins = {k: pool.put(I[k]) for k in ('real_B', 'mask', 'x_stage1', 'x_stage2', 'fine_seg', 'coarse_seg', 'pred1', 'pred2', 'height', 'x1', 'x2', 'maxheight')}
    outs = {k: pool.out((B, 1, H, W)) for k in ('fake_B', 'fake_B_coarse', 'fake_B_local', 'real_B_local', 'fine_bin', 'coarse_bin')}
    outs['pred1_h'], outs['pred2_h'] = pool.out((1, B)), pool.out((1, B))
    outs['rows'] = pool.out((B, 4), torch.int32)
    for k, g in list(ins.items()) + list(outs.items()):
        setattr(d, k, lib.ptr(g.t).value)
    d.B, d.H, d.W, d.half_band = B, H, W, half
    L.call('hv_post_generator', ctypes.byref(d), lib.stream())
    return ins, outs


def postg_inputs(B, H, W, height, x1, maxheight, pred1, pred2, seed):
    gen = torch.Generator().manual_seed(seed)
    I = {k: rnd(gen, B, 1, H, W) * 2 - 1 for k in ('real_B', 'x_stage1', 'x_stage2')}
    I['mask'] = (rnd(gen, B, 1, H, W) > 0.4).float()
    I['fine_seg'], I['coarse_seg'] = rnd(gen, B, 1, H, W), rnd(gen, B, 1, H, W)
    I['fine_seg'].view(-1)[::7] = 0.5      # exactly at the threshold: stays 0
    I['coarse_seg'].view(-1)[::5] = 0.5
    I['height'], I['x1'], I['maxheight'] = torch.tensor(height), torch.tensor(x1), torch.tensor(maxheight)
    I['x2'] = I['x1'] + I['height']
    I['pred1'], I['pred2'] = torch.tensor(pred1).view(B, 1), torch.tensor(pred2).view(B, 1)
    return I


def check_post_generator(ck, outs, ref, what):
    for k, r in ref.items():
        ck.true(same_bits(outs[k].cpu(), r), '%s: other bits: %s' % (k, what))


def test_post_generator_rectangular():
    """(3, 12, 20), half_band 3, bit for bit: pred2 * maxheight an exact integer (0.75 * 8), below the measured height, xu == 0, xb == H; odd growth."""
    B, H, W, half = 3, 12, 20, 3
    I = postg_inputs(B, H, W, [4, 5, 6], [3, 0, 4], [8, 10, 10], [0.6, 0.5, 0.71], [0.75, 0.33, 0.99], 61)
    ref = PR.post_generator_ref(I, half)
    assert ref['rows'].tolist() == [[2, 8, 3, 8], [0, 5, 0, 5], [2, 12, 3, 11]]
    ck = Check()
    pool = Pool()
    _, outs = call_post_generator(pool, I, B, H, W, half)
    ck.true(pool.intact(), 'guards')
    check_post_generator(ck, outs, ref, 'post_generator')
    ck.done()


def test_chain_post_generator_to_shrm_backward():
    """post_generator -> sobel x 2 -> generator_losses -> shrm_backward x 2 at (4, 24, 40), half_band 6, against torch.autograd.grad of the whole
    restated tail wrt x_stage1 / x_stage2 in fp64: the loss sum x the loss scale + <dD, fake_B> + <dD_local, fake_B_local> (the two discriminator
    gradients that enter as add_d_fake_B and d_local).  pred * maxheight: 12 exactly (0.75 * 16) and 5 exactly (0.3125 * 16 == height), the others
    >= 0.2 away from an integer."""
    from oracle import restate
    B, H, W, half, lam, gs = 4, 24, 40, 6, 200.0, 1024.0
    I = postg_inputs(B, H, W, [8, 10, 5, 12], [6, 3, 0, 8], [16, 20, 16, 20], [0.6, 0.71, 0.3125, 0.81], [0.75, 0.33, 0.3, 0.99], 62)
    gen = torch.Generator().manual_seed(63)
    I['real_B_mask'], I['normal_vert'] = (rnd(gen, B, 1, H, W) > 0.5).float(), (rnd(gen, B, 1, H, W) > 0.5).float()
    dD, dDl = torch.randn(B, 1, H, W, generator=gen) * gs * 1e-3, torch.randn(B, 1, H, W, generator=gen) * gs * 1e-3
    pg = PR.post_generator_ref(I, half)
    ph = torch.cat([pg['pred1_h'], pg['pred2_h']]).double()
    frac = (ph - ph.round()).abs()
    assert pg['pred2_h'][0, 0] == 12.0 and pg['pred1_h'][0, 2] == 5.0 and bool(((frac == 0) | (frac >= 1e-3)).all())
    assert pg['rows'].tolist() == [[4, 16, 5, 15], [3, 13, 1, 16], [0, 5, 0, 5], [4, 24, 6, 23]]

    # ---- fp64: one graph from x_stage1 / x_stage2 to the scalar
    D = {k: (v.double() if v.is_floating_point() else v) for k, v in I.items()}
    xs1, xs2 = D['x_stage1'].clone().requires_grad_(True), D['x_stage2'].clone().requires_grad_(True)
    J = {k: D[k] for k in ('real_B', 'mask', 'fine_seg', 'coarse_seg', 'real_B_mask', 'normal_vert', 'pred1', 'pred2', 'height', 'maxheight')}
    J['fake_B'] = restate.shrm_composite(xs2, D['real_B'], pg['pred2_h'][0], I['height'], I['x1'], I['x2'])
    J['fake_B_coarse'] = restate.shrm_composite(xs1, D['real_B'], pg['pred1_h'][0], I['height'], I['x1'], I['x2'])
    J['fake_edges'], J['real_edges'] = PR.sobel_ref((D['fine_seg'] > 0.5).double()), PR.sobel_ref(D['real_B_mask'])
    terms, mag, _, _ = PR.generator_loss_terms(J, lam)
    local = D['mask'] * J['fake_B'] * restate.center_band(D['mask'], half)
    scalar = sum(terms) * gs + (dD.double() * J['fake_B']).sum() + (dDl.double() * local).sum()
    r1, r2 = torch.autograd.grad(scalar, [xs1, xs2])
    lref = torch.stack([t.detach() for t in terms])

    # ---- device
    ck = Check()
    pool = Pool()
    ins, po = call_post_generator(pool, I, B, H, W, half)
    ck.true(pool.intact(), 'guards: post_generator')
    check_post_generator(ck, po, pg, 'chain')
    rbm, nv = pool.put(I['real_B_mask']), pool.put(I['normal_vert'])
    fe, re_ = pool.out((B, 1, H, W)), pool.out((B, 1, H, W))
    L.call('hv_sobel', p_(po['fine_bin']), p_(fe), B, H, W, lib.stream())
    L.call('hv_sobel', p_(rbm), p_(re_), B, H, W, lib.stream())
    ck.true(pool.intact(), 'guards: sobel')
    d = L.hv_gloss_desc()
    seeds = {k: pool.out((B, 1, H, W)) for k in ('d_fake_B', 'd_fake_B_coarse', 'd_fine_seg', 'd_coarse_seg')}
    losses, add = pool.out(6), pool.put(dD)
    fields = dict(fake_B=po['fake_B'], fake_B_coarse=po['fake_B_coarse'], real_B=ins['real_B'], mask=ins['mask'], fine_seg=ins['fine_seg'],
                  coarse_seg=ins['coarse_seg'], real_B_mask=rbm, normal_vert=nv, fake_edges=fe, real_edges=re_, pred1_h=po['pred1_h'], pred2_h=po['pred2_h'],
                  height=ins['height'], maxheight=ins['maxheight'], losses=losses, add_d_fake_B=add, **seeds)
    for k, g in fields.items():
        setattr(d, k, lib.ptr(g.t).value)
    d.lambda_L1, d.B, d.H, d.W, d.grad_scale = lam, B, H, W, gs
    need = L.size('hv_generator_losses_workspace_bytes', B)
    ws = pool.out(need // 4)
    d.workspace, d.workspace_bytes = lib.ptr(ws.t).value, need
    L.call('hv_generator_losses', ctypes.byref(d), lib.stream())
    ck.true(pool.intact(), 'guards: generator_losses')
    dl, g1, g2 = pool.put(dDl), pool.out((B, 1, H, W)), pool.out((B, 1, H, W))
    L.call('hv_shrm_backward', p_(seeds['d_fake_B']), p_(dl), p_(ins['mask']), p_(po['rows']), 0, p_(g2), B, H, W, half, 0, lib.stream())
    L.call('hv_shrm_backward', p_(seeds['d_fake_B_coarse']), None, None, p_(po['rows']), 1, p_(g1), B, H, W, half, 0, lib.stream())
    ck.true(pool.intact(), 'guards: shrm_backward')

    ck.le('tail.loss', (losses.cpu().double()[:5] - lref).abs(), 64 * U * mag + U * lref.abs(), 'chain losses')
    # fp32 evaluation of the same formulas: seed, then the selection
    cnt = torch.count_nonzero(I['mask']).double()
    coef32 = (0.5 * lam * (W * W / cnt) * 2 / (B * H * W)).float()
    gs32 = torch.tensor(gs, dtype=torch.float32)
    one = torch.ones(B, 1, H, W, dtype=torch.float64)
    for which, got, ref, fake, extra in ((0, g2, r2, pg['fake_B'], True), (1, g1, r1, pg['fake_B_coarse'], False)):
        sel = PR.shrm_backward_ref(one, None, None, pg['rows'], which, half).float()
        s32 = PR.l1_seed_formula(coef32, fake, I['real_B'], gs32)
        if extra:
            selb = PR.shrm_backward_ref(None, one, one, pg['rows'], which, half).float()
            s32 = (s32 + dD) * sel + (dDl * I['mask']) * selb
        else:
            s32 = s32 * sel
        floor = (s32.double() - ref).abs().max().item()
        ck.le('tail.chain', (got.cpu().double() - ref).abs(), tol_elem(ref, floor, False), 'd_x_stage%d' % (2 - which))
        ck.true(bool((ref != 0).any()) and bool((ref == 0).any()), 'test inputs: the gradient has no zero / non-zero rows')
    ck.done()


# ---------------------------------------------------------------------------------------------------------------- pooled height head
GAP_C, GAP_HW, GAP_B = (1, 16, 64, 256), (1, 31, 33, 1024), 3


@functools.lru_cache(maxsize=None)
def gap_inputs(C, HW, f16):
    gen = torch.Generator().manual_seed(C * 7919 + HW * 13 + int(f16))
    x = (torch.randn(GAP_B, HW, C, generator=gen) + 0.5).to(dtype_of(f16))
    w, b = torch.randn(C, generator=gen) / math.sqrt(C), torch.randn(1, generator=gen)
    pooled, pred = PR.gap_fc_sigmoid_ref(x.double(), w.double(), b.double()[0])
    return x, w, b, pooled, pred


def widen(x, ld, fill=SENT):
    """(.., C) -> (.., ld) with the channels past C holding the sentinel."""
    out = torch.full(x.shape[:-1] + (ld,), fill, dtype=x.dtype)
    out[..., :x.shape[-1]] = x
    return out


@pytest.mark.parametrize('f16', [False, True], ids=['f32', 'f16'])
@pytest.mark.parametrize('C', GAP_C)
def test_gap_fc_sigmoid_forward(C, f16):
    ck = Check()
    for HW in GAP_HW:
        x, w, b, pooled, pred = gap_inputs(C, HW, f16)
        depth = (math.ceil(math.log2(HW)) if HW > 1 else 0) + 16
        pb = depth * U * x.double().abs().mean(dim=1)                                       # (B, C)
        z = pooled @ w.double() + b.double()[0]
        prb = pred * (1 - pred) * ((pb * w.double().abs()).sum(dim=1) + 2 * U * (z.abs() + b.double()[0].abs())) + 4 * U * pred
        for ld in (C, C + 4):
            what = 'C=%d HW=%d ld=%d f16=%d' % (C, HW, ld, f16)
            pool = Pool()
            bx, bw, bb = pool.put(widen(x, ld)), pool.put(w), pool.put(b)
            op, opr = pool.out((GAP_B, C)), pool.out(GAP_B)
            need = L.size('hv_gap_fc_workspace_bytes', GAP_B, C)
            ws = pool.out(need // 4)
            L.call('hv_gap_fc_sigmoid', p_(bx), int(f16), GAP_B, HW, C, ld, p_(bw), p_(bb), p_(op), p_(opr), p_(ws), need, lib.stream())
            ck.true(pool.intact(), 'guards: ' + what)
            ck.true(same_bits(bx.cpu(), widen(x, ld)), 'x changed: ' + what)
            ck.le('tail.pooled', (op.cpu().double() - pooled).abs(), pb, what)
            ck.le('tail.pred', (opr.cpu().double() - pred).abs(), prb, what)
    ck.done()


MULS = (None,) + PR.ACTS


@pytest.mark.parametrize('C', GAP_C)
def test_gap_fc_sigmoid_backward(C):
    """The backward reads the stored (fp32) pred and pooled and, with mul_src, the stored output of the activation: the reference is evaluated on the same
    stored values.  dx always accumulates: it holds prior values of its storage type."""
    ck = Check()
    k = GAP_C.index(C)
    for HW in GAP_HW:
        for dx16 in (False, True):
            k += 1
            act = MULS[k % len(MULS)]
            acc, mul16, dx_ld = k & 1, bool((k >> 1) & 1), C + 4 * ((k >> 2) & 1)
            what = 'C=%d HW=%d dx16=%d acc=%d mul=%s mul16=%d dx_ld=%d' % (C, HW, dx16, acc, act, mul16, dx_ld)
            x, w, b, pooled, pred = gap_inputs(C, HW, False)
            gen = torch.Generator().manual_seed(900 + k)
            dpred = torch.randn(GAP_B, generator=gen)
            pred32, pooled32 = pred.float(), pooled.float()
            prior = torch.randn(GAP_B, HW, C, generator=gen).to(dtype_of(dx16))
            mul = None if act is None else PR.act_formula(torch.randn(GAP_B, HW, C, generator=gen) * 1.5, act).to(dtype_of(mul16))
            dwp, dbp = torch.linspace(-1, 1, C), torch.tensor([0.75])
            inc, dwr, dbr = PR.gap_fc_sigmoid_backward_ref(dpred.double(), pred32.double(), pooled32.double(), w.double(), HW,
                                                           None if mul is None else mul.double(), act or 'none')
            inc32, _, _ = PR.gap_fc_sigmoid_backward_ref(dpred, pred32, pooled32, w, HW, None if mul is None else mul.float(), act or 'none')
            ref = prior.double() + inc
            floor = ((prior.float() + inc32).double() - ref).abs().max().item()
            dl = dpred.double() * pred32.double() * (1 - pred32.double())
            wb = 16 * U * (dl.abs().view(-1, 1) * pooled32.double().abs()).sum(dim=0) + U * dwr.abs()
            bb = 16 * U * dl.abs().sum() + U * dbr.abs()
            if acc:
                dwr, dbr = dwr + dwp.double(), dbr + dbp.double()[0]
                wb, bb = wb + U * dwr.abs(), bb + U * dbr.abs()
            pool = Pool()
            bdx = pool.put(widen(prior, dx_ld))
            bmul = None if mul is None else pool.put(widen(mul, C + 4))
            bdw, bdb = (pool.put(dwp), pool.put(dbp)) if acc else (pool.out(C), pool.out(1))
            ins = [pool.put(t) for t in (dpred, pred32, pooled32, w)]
            L.call('hv_gap_fc_sigmoid_backward', p_(ins[0]), p_(ins[1]), p_(ins[2]), p_(ins[3]), p_(bdx), int(dx16), GAP_B, HW, C, dx_ld, p_(bdw), p_(bdb), acc,
                   p_(bmul), int(mul16), C + 4, lib.ACT[act or 'none'], lib.stream())
            ck.true(pool.intact(), 'guards: ' + what)
            got = bdx.cpu()
            ck.true(bool((got[..., C:] == SENT).all()), 'channels past C changed: ' + what)
            tol = tol_elem(ref, floor, dx16) + (half_ulp16(ref) if dx16 else 0)
            ck.le('tail.gap_dx', (got[..., :C].double() - ref).abs(), tol, what)
            ck.le('tail.gap_dwdb', (bdw.cpu().double() - dwr).abs(), wb, 'dw: ' + what)
            ck.le('tail.gap_dwdb', (bdb.cpu().double()[0] - dbr).abs(), bb, 'db: ' + what)
    ck.done()


def test_gap_fc_sigmoid_refusals():
    pool = Pool()
    x, w, b = pool.put(torch.zeros(2, 4, 512)), pool.put(torch.zeros(512)), pool.put(torch.zeros(1))
    op, opr, ws = pool.out((2, 512)), pool.out(2), pool.out(2 * 32 * 512)
    for C in (24, 512):      # not a power of two; wider than a workgroup
        with pytest.raises(RuntimeError, match='HV_ERR_UNSUPPORTED'):
            L.call('hv_gap_fc_sigmoid', p_(x), 0, 2, 4, C, C, p_(w), p_(b), p_(op), p_(opr), p_(ws), ws.n * 4, lib.stream())
    need = L.size('hv_gap_fc_workspace_bytes', 2, 16)
    assert need == 2 * 32 * 16 * 4
    with pytest.raises(RuntimeError, match='HV_ERR_WORKSPACE'):
        L.call('hv_gap_fc_sigmoid', p_(x), 0, 2, 4, 16, 16, p_(w), p_(b), p_(op), p_(opr), p_(ws), need - 1, lib.stream())
    assert pool.intact() and bool(torch.isnan(op.cpu()).all())


# ---------------------------------------------------------------------------------------------------------------- hv_copy_channels
# form: (C, src_ld, src_coff, dst_ld, dst_coff)
COPY_FORMS = {'vec8': (8, 16, 4, 12, 4), 'one_into_5_of_8': (1, 3, 1, 8, 5), 'six': (6, 6, 0, 7, 1)}
PAIRS = [(False, False), (True, False), (False, True), (True, True)]


def nhwc_view(x_nchw, ld, coff, dtype, fill=SENT):
    B, C, H, W = x_nchw.shape
    t = torch.full((B, H, W, ld), fill, dtype=dtype)
    t[..., coff:coff + C] = x_nchw.permute(0, 2, 3, 1).to(dtype)
    return t


def copy_case(ck, B, H, W, form, mode, s16, d16, acc, dst_offset=0, seed=0):
    C, s_ld, s_co, d_ld, d_co = COPY_FORMS[form]
    what = '%s mode=%d %dx%dx%d s16=%d d16=%d acc=%d off=%d' % (form, mode, B, H, W, s16, d16, acc, dst_offset)
    hs, ws = PR.copy_src_size(mode, H, W)
    gen = torch.Generator().manual_seed(seed + mode * 31 + H)
    src = torch.randn(B, C, hs, ws, generator=gen).to(dtype_of(s16))
    prior = torch.randn(B, C, H, W, generator=gen).to(dtype_of(d16))
    inc = PR.copy_channels_ref(src.double(), mode)
    ref = prior.double() + inc if acc else inc
    pool = Pool()
    bs = pool.put(nhwc_view(src, s_ld, s_co, dtype_of(s16)))
    d0 = nhwc_view(prior if acc else torch.full_like(prior, float('nan')), d_ld, d_co, dtype_of(d16))
    bd = pool.put(d0, offset=dst_offset)
    L.call('hv_copy_channels', p_(bs), int(s16), p_(bd), int(d16), B, H, W, C, s_ld, s_co, d_ld, d_co, mode, acc, lib.stream())
    ck.true(pool.intact(), 'guards: ' + what)
    got = bd.cpu()
    keep = torch.ones(d_ld, dtype=torch.bool)
    keep[d_co:d_co + C] = False
    ck.true(bool((got[..., keep] == SENT).all()), 'channels around the slice changed: ' + what)
    got = got[..., d_co:d_co + C].permute(0, 3, 1, 2)
    if not acc and mode != 3:      # a copy (with zeros in mode 4): the bits, after the conversion
        ck.true(same_bits(got.contiguous(), ref.to(dtype_of(d16))), 'copy: other bits: ' + what)
    v32 = PR.copy_channels_ref(src.float(), mode)
    floor = (((prior.float() + v32) if acc else v32).double() - ref).abs().max().item()
    tol = tol_elem(ref, floor, d16) + (half_ulp16(ref) if (d16 and acc) else 0)
    ck.le('tail.copy', (got.double() - ref).abs(), tol, what)


@pytest.mark.parametrize('mode', [0, 1, 2, 3, 4])
@pytest.mark.parametrize('form', sorted(COPY_FORMS))
def test_copy_channels(form, mode):
    ck = Check()
    sizes = [(2, 2), (6, 10)] + ([(3, 5)] if mode in (0, 2, 3) else [])
    k = 0
    for H, W in sizes:
        for s16, d16 in PAIRS:
            for acc in (0, 1):
                copy_case(ck, 2, H, W, form, mode, s16, d16, acc, seed=k)
                k += 1
    ck.done()


@pytest.mark.parametrize('mode', [1, 4])
def test_copy_channels_refuses_odd_sizes_from_a_half_size_source(mode):
    pool = Pool()
    s, d = pool.put(torch.zeros(2, 3, 5, 8)), pool.out((2, 3, 5, 8))
    for H, W in ((3, 4), (2, 5), (3, 5)):
        with pytest.raises(RuntimeError, match='HV_ERR_UNSUPPORTED'):
            L.call('hv_copy_channels', p_(s), 0, p_(d), 0, 2, H, W, 8, 8, 0, 8, 0, mode, 0, lib.stream())
    assert pool.intact() and bool(torch.isnan(d.cpu()).all())


def test_copy_channels_row_loop_and_unaligned_base():
    """B * H = 32769 rows of one pixel: the grid has 32768 rows, row 0's workgroup also takes row 32768.  A vector-shaped copy whose destination starts 4
    bytes off a 16-byte boundary has to take the scalar kernel."""
    ck = Check()
    for mode in (0, 2):
        for s16, d16 in ((False, False), (True, True)):
            copy_case(ck, 1, 32769, 1, 'one_into_5_of_8', mode, s16, d16, 1, seed=5)
    for mode in (0, 1, 3):
        for acc in (0, 1):
            copy_case(ck, 2, 6, 10, 'vec8', mode, False, False, acc, dst_offset=1, seed=6)
    ck.done()


# ---------------------------------------------------------------------------------------------------------------- hv_add_channels, hv_gen_input, layout
@pytest.mark.parametrize('C', [1, 3])
def test_add_channels(C):
    ck = Check()
    npix = 300
    k = 0
    for a16, b16 in PAIRS:
        for d16 in (False, True):
            gen = torch.Generator().manual_seed(70 + k)
            a, b = torch.randn(1, C, 1, npix, generator=gen).to(dtype_of(a16)), torch.randn(1, C, 1, npix, generator=gen).to(dtype_of(b16))
            (a_ld, a_co), (b_ld, b_co), (d_ld, d_co) = (C + 2, 1), (C + 1, 0), (C + 4, 3)
            what = 'C=%d a16=%d b16=%d d16=%d' % (C, a16, b16, d16)
            ref = PR.add_channels_ref(a.double(), b.double())
            floor = ((a.float() + b.float()).double() - ref).abs().max().item()
            pool = Pool()
            ba, bb = pool.put(nhwc_view(a, a_ld, a_co, dtype_of(a16))), pool.put(nhwc_view(b, b_ld, b_co, dtype_of(b16)))
            bd = pool.put(nhwc_view(torch.full_like(a, float('nan')), d_ld, d_co, dtype_of(d16)))
            L.call('hv_add_channels', p_(ba), int(a16), a_ld, a_co, p_(bb), int(b16), b_ld, b_co, p_(bd), int(d16), d_ld, d_co, npix, C, lib.stream())
            ck.true(pool.intact(), 'guards: ' + what)
            got = bd.cpu()
            ck.true(bool((got[..., :d_co] == SENT).all()) and bool((got[..., d_co + C:] == SENT).all()), 'channels around the slice changed: ' + what)
            ck.le('tail.add', (got[..., d_co:d_co + C].permute(0, 3, 1, 2).double() - ref).abs(), tol_elem(ref, floor, d16), what)
            k += 1
    ck.done()


@pytest.mark.parametrize('f16', [False, True], ids=['f32', 'f16'])
@pytest.mark.parametrize('CP', [4, 8])
@pytest.mark.parametrize('order', [0, 1])
def test_gen_input(order, CP, f16):
    B, H, W = 2, 3, 5
    gen = torch.Generator().manual_seed(80)
    x, seg, mask = (torch.randn(B, 1, H, W, generator=gen) for _ in range(3))
    ratio = torch.tensor([0.1, 1.0 / 3.0], dtype=torch.float64)
    assert bool((ratio.float().double() != ratio).all())
    ref = PR.gen_input_ref(x.double(), seg.double(), mask.double(), ratio, CP, order).to(dtype_of(f16))
    pool = Pool()
    bx, bs, bm, br = pool.put(x), pool.put(seg), pool.put(mask), pool.put(ratio)
    out = pool.out((B, H, W, CP), dtype_of(f16))
    L.call('hv_gen_input', p_(bx), p_(bs) if order else None, p_(bm), p_(br), p_(out), int(f16), B, H, W, CP, order, lib.stream())
    assert pool.intact()
    assert same_bits(out.cpu(), ref) and bool((out.cpu()[..., 4:] == 0).all())
    if order == 1:
        with pytest.raises(RuntimeError, match='HV_ERR_ARG'):
            L.call('hv_gen_input', p_(bx), None, p_(bm), p_(br), p_(out), int(f16), B, H, W, CP, order, lib.stream())
        assert pool.intact()


@pytest.mark.parametrize('f16', [False, True], ids=['f32', 'f16'])
@pytest.mark.parametrize('C', [1, 3, 5])
def test_layout_pair(C, f16):
    B, H, W, ld, coff = 2, 3, 5, C + 3, 2
    gen = torch.Generator().manual_seed(90 + C)
    x = torch.randn(B, C, H, W, generator=gen)
    dt = dtype_of(f16)
    pool = Pool()
    src = pool.put(x)
    dst = pool.put(torch.full((B, H, W, ld), SENT, dtype=dt))
    L.call('hv_nchw_to_nhwc', p_(src), p_(dst), int(f16), B, C, H, W, ld, coff, lib.stream())
    assert pool.intact()
    got = dst.cpu()
    want = torch.full((B, H, W, ld), SENT, dtype=dt)
    want[..., coff:coff + C] = PR.nchw_to_nhwc_ref(x.double()).to(dt)
    assert same_bits(got, want)
    # and back, out of the view: plain, then accumulated onto prior values (one fp32 addition: the bits of the fp32 CPU sum)
    xs = x.to(dt)
    prior = torch.randn(B, C, H, W, generator=gen)
    for acc in (0, 1):
        pool = Pool()
        s = pool.put(nhwc_view(xs, ld, coff, dt))
        o = pool.put(prior) if acc else pool.out((B, C, H, W))
        L.call('hv_nhwc_to_nchw', p_(s), int(f16), p_(o), B, C, H, W, ld, coff, acc, lib.stream())
        assert pool.intact()
        back = PR.nhwc_to_nchw_ref(PR.nchw_to_nhwc_ref(xs.double())).float()
        assert same_bits(o.cpu(), prior + back if acc else back), acc


# ---------------------------------------------------------------------------------------------------------------- hv_sobel
BIG_N = 8192 * 256 + 257      # one element more than a grid of 8192 x 256 lanes covers in one pass of the grid-stride loop, and a ragged tail


@pytest.mark.parametrize('B,H,W', [(3, 1, 9), (3, 9, 1), (2, 5, 7), (1, 1, 1), (1, 1, BIG_N)], ids=['3x1x9', '3x9x1', '2x5x7', '1x1x1', 'flat_big'])
def test_sobel(B, H, W):
    ck = Check()
    gen = torch.Generator().manual_seed(B * 100 + H * 10 + W % 10)
    x = rnd(gen, B, 1, H, W) * 0.6
    ref = PR.sobel_ref(x.double())
    if H * W > 1:
        assert bool((ref == 1.0).any()) and bool(((ref < 1.0) & (ref > 0)).any()), 'test inputs: one branch of the clip is missing'
    floor = (PR.sobel_ref(x).double() - ref).abs().max().item()
    pool = Pool()
    bi, bo = pool.put(x), pool.out((B, 1, H, W))
    L.call('hv_sobel', p_(bi), p_(bo), B, H, W, lib.stream())
    ck.true(pool.intact(), 'guards')
    ck.true(same_bits(bi.cpu(), x), 'input changed')
    ck.le('tail.sobel', (bo.cpu().double() - ref).abs(), tol_elem(ref, floor, False), 'sobel')
    if H * W == 1:
        ck.true(bo.cpu().item() == 0.0, 'one pixel: not 0')
    ck.done()


# ---------------------------------------------------------------------------------------------------------------- small operators
def small_case(ck, n):
    what = 'n=%d' % n
    gen = torch.Generator().manual_seed(n)
    x, y, z = torch.randn(n, generator=gen), torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    a, b = 0.3, -1.7
    a32, b32 = torch.tensor(a, dtype=torch.float32), torch.tensor(b, dtype=torch.float32)
    af, bf = float(a32), float(b32)      # the values the C float arguments hold

    def run(entry, out_data, *args_of):
        pool = Pool()
        o = pool.put(out_data) if out_data is not None else pool.out(n)
        bufs = {'o': o, 'x': pool.put(x), 'z': pool.put(z)}
        L.call(entry, *[p_(bufs[v]) if isinstance(v, str) else v for v in args_of], lib.stream())
        ck.true(pool.intact(), 'guards: %s %s' % (entry, what))
        ck.true(same_bits(bufs['x'].cpu(), x) and same_bits(bufs['z'].cpu(), z), 'input changed: %s %s' % (entry, what))
        return o.cpu()

    def elem(entry, got, ref, v32):
        floor = (v32.double() - ref).abs().max().item()
        ck.le('tail.small', (got.double() - ref).abs(), tol_elem(ref, floor, False), '%s %s' % (entry, what))

    ck.true(same_bits(run('hv_fill', None, 'o', n, 2.5), PR.fill_ref(n, 2.5, torch.float32)), 'hv_fill ' + what)
    elem('hv_axpy', run('hv_axpy', y, 'o', 'x', n, af), PR.axpy_formula(y.double(), x.double(), af), PR.axpy_formula(y, x, a32))
    elem('hv_affine', run('hv_affine', None, 'o', 'x', n, af, bf), PR.affine_formula(x.double(), af, bf), PR.affine_formula(x, a32, b32))
    elem('hv_affine in place', run('hv_affine', y, 'o', 'o', n, af, bf), PR.affine_formula(y.double(), af, bf), PR.affine_formula(y, a32, b32))
    elem('hv_mul', run('hv_mul', y, 'o', 'x', n), PR.mul_formula(y.double(), x.double()), PR.mul_formula(y, x))
    ck.true(same_bits(run('hv_mul3', y, 'o', 'x', 'z', n), PR.mul3_formula(y, x, z)), 'hv_mul3: not the fp32 product (y * x) * z: ' + what)
    thr = 0.5
    t = x.clone()
    t[::3] = thr      # exactly at the threshold: 0
    pool = Pool()
    bt, bo = pool.put(t), pool.out(n)
    L.call('hv_threshold', p_(bt), p_(bo), n, thr, 3.0, lib.stream())
    ck.true(pool.intact(), 'guards: hv_threshold ' + what)
    want = PR.threshold_ref(t.double(), thr, 3.0).float()
    ck.true(same_bits(bo.cpu(), want) and want[0] == 0, 'hv_threshold ' + what)


@pytest.mark.parametrize('n', [1, 255, 257])
def test_small_operators(n):
    ck = Check()
    small_case(ck, n)
    ck.done()


def test_affine_grid_stride_loop():
    ck = Check()
    n = BIG_N
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(n, generator=gen)
    a32, b32 = torch.tensor(0.3), torch.tensor(-1.7)
    ref = PR.affine_formula(x.double(), float(a32), float(b32))
    floor = (PR.affine_formula(x, a32, b32).double() - ref).abs().max().item()
    pool = Pool()
    bx, bo = pool.put(x), pool.out(n)
    L.call('hv_affine', p_(bo), p_(bx), n, float(a32), float(b32), lib.stream())
    ck.true(pool.intact(), 'guards')
    ck.le('tail.small', (bo.cpu().double() - ref).abs(), tol_elem(ref, floor, False), 'hv_affine n=%d' % n)
    ck.done()
