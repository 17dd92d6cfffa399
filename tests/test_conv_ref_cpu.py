"""tests/conv_ref.py (the float64 references the device convolution tests compare against) pinned against torch's own float64 convolutions, torch
autograd and a nested-loop convolution.  No device code: runs without a GPU."""
import pytest
import torch
import torch.nn.functional as F

import conv_ref as CR
import pointwise_ref as PR

F64 = torch.float64
TOL = 1e-12


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=F64)


def ohwi(w):      # [Cout][Cin][kh][kw] -> [Cout][taps][Cin]
    Co, Ci, kh, kw = w.shape
    return w.permute(0, 2, 3, 1).reshape(Co, kh * kw, Ci).contiguous()


def ohwi_T(w):    # [Cout][Cin][kh][kw] -> the data-gradient table [Cin][taps][Cout]
    Co, Ci, kh, kw = w.shape
    return w.permute(1, 2, 3, 0).reshape(Ci, kh * kw, Co).contiguous()


def close(a, b, tol=TOL):
    assert a.shape == b.shape, (a.shape, b.shape)
    assert (a - b).abs().max().item() <= tol * max(1.0, b.abs().max().item()), (a - b).abs().max().item()


FWD = [  # B, H, W, Cin, Cout, (kh, kw), stride, pad, dil
    (2, 12, 10, 6, 10, (3, 3), 1, 1, 1), (2, 12, 10, 6, 10, (3, 3), 2, 1, 1), (2, 12, 10, 6, 10, (3, 3), 1, 2, 2), (2, 9, 11, 5, 3, (4, 4), 1, 1, 1),
    (1, 20, 22, 1, 8, (4, 4), 2, 1, 1), (2, 7, 9, 4, 2, (5, 5), 1, 2, 1), (2, 8, 9, 3, 4, (3, 2), 2, 0, 1), (1, 17, 17, 2, 2, (3, 3), 1, 8, 8),
]


@pytest.mark.parametrize('case', FWD)
def test_forward_matches_conv2d_and_S_is_the_contraction_of_absolute_values(case):
    B, H, W, Cin, Cout, k, s, p, d = case
    x, w, b = rnd(B, Cin, H, W, seed=1), rnd(Cout, Cin, *k, seed=2), rnd(Cout, seed=3)
    y, S = CR.conv_ref(x, ohwi(w), b, s, p, d, k=k)
    close(y, F.conv2d(x, w, b, stride=s, padding=p, dilation=d))
    close(S, F.conv2d(x.abs(), w.abs(), None, stride=s, padding=p, dilation=d))
    assert y.dtype == F64 and bool((S >= (y - b.view(1, -1, 1, 1)).abs() - 1e-12).all())


@pytest.mark.parametrize('case', [(2, 6, 5, 4, 3, 4, 2, 1, 1), (2, 6, 5, 4, 3, 3, 1, 1, 1), (1, 5, 7, 3, 2, 3, 2, 1, 1), (2, 5, 4, 3, 2, 3, 1, 2, 2), (2, 6, 6, 2, 3, 5, 1, 2, 1)])
def test_transposed_matches_conv_transpose2d(case):
    B, H, W, Cin, Cout, k, s, p, d = case
    x, wt = rnd(B, Cin, H, W, seed=4), rnd(Cin, Cout, k, k, seed=5)      # ConvTranspose2d weight [Cin][Cout][kh][kw]
    tab = wt.permute(1, 2, 3, 0).reshape(Cout, k * k, Cin)
    y, S = CR.conv_ref(x, tab, None, s, p, d, transposed=True)
    close(y, F.conv_transpose2d(x, wt, None, stride=s, padding=p, dilation=d))
    close(S, F.conv_transpose2d(x.abs(), wt.abs(), None, stride=s, padding=p, dilation=d))
    if s == 2:      # the data gradient of an even-sized stride-2 layer: one more row / column than the minimal size
        y2, _ = CR.conv_ref(x, tab, None, s, p, d, transposed=True, out_hw=(y.shape[2] + 1, y.shape[3] + 1))
        close(y2, F.conv_transpose2d(x, wt, None, stride=s, padding=p, dilation=d, output_padding=1))


@pytest.mark.parametrize('case', [(2, 12, 10, 6, 10, 3, 1, 1, 1), (2, 12, 10, 6, 10, 3, 2, 1, 1), (2, 12, 12, 4, 6, 3, 1, 2, 2), (2, 8, 8, 3, 5, 4, 2, 1, 1), (2, 9, 9, 3, 5, 4, 1, 1, 1)])
def test_data_and_weight_gradients_match_autograd(case):
    B, H, W, Cin, Cout, k, s, p, d = case
    x = rnd(B, Cin, H, W, seed=6).requires_grad_(True)
    w = rnd(Cout, Cin, k, k, seed=7).requires_grad_(True)
    y = F.conv2d(x, w, None, stride=s, padding=p, dilation=d)
    g = rnd(*y.shape, seed=8)
    y.backward(g)
    dx, _ = CR.conv_ref(g, ohwi_T(w.detach()), None, s, p, d, transposed=True, out_hw=(H, W))
    close(dx, x.grad)
    dw, db, Sw, Sb = CR.wgrad_ref(x.detach(), g, k, s, p, d)
    close(dw, ohwi(w.grad))
    close(db, g.sum(dim=(0, 2, 3)))
    dwa, _, _, _ = CR.wgrad_ref(x.detach().abs(), g.abs(), k, s, p, d)
    close(Sw, dwa)
    close(Sb, g.abs().sum(dim=(0, 2, 3)))


def test_fused_upsampling_matches_interpolate_forward_and_weight_gradient():
    x = rnd(2, 5, 6, 4, seed=9)
    w = rnd(3, 5, 3, 3, seed=10).requires_grad_(True)
    up = F.interpolate(x, scale_factor=2, mode='nearest')
    ref = F.conv2d(up, w, None, padding=1)
    y, S = CR.conv_ref(x, ohwi(w.detach()), None, 1, 1, 1, in_shift=1)
    close(y, ref.detach())
    g = rnd(*ref.shape, seed=11)
    ref.backward(g)
    dw, _, _, _ = CR.wgrad_ref(x, g, 3, 1, 1, 1, in_shift=1)
    close(dw, ohwi(w.grad))


def naive(x, w, b, k, s, p, d):
    B, Cin, H, W = x.shape
    Cout = w.shape[0]
    Ho, Wo = CR.conv_out_size(H, k, s, p, d), CR.conv_out_size(W, k, s, p, d)
    y = torch.zeros(B, Cout, Ho, Wo, dtype=F64)
    for n in range(B):
        for co in range(Cout):
            for ho in range(Ho):
                for wo in range(Wo):
                    acc = 0.0
                    for r in range(k):
                        for q in range(k):
                            hi, wi = ho * s - p + r * d, wo * s - p + q * d
                            if 0 <= hi < H and 0 <= wi < W:
                                for ci in range(Cin):
                                    acc += x[n, ci, hi, wi].item() * w[co, r * k + q, ci].item()
                    y[n, co, ho, wo] = acc + b[co].item()
    return y


@pytest.mark.parametrize('s,p,d', [(1, 1, 1), (2, 1, 1), (1, 2, 2)])
def test_against_nested_loops(s, p, d):
    x, w, b = rnd(2, 3, 5, 4, seed=12), rnd(4, 9, 3, seed=13), rnd(4, seed=14)
    y, _ = CR.conv_ref(x, w, b, s, p, d)
    close(y, naive(x, w, b, 3, s, p, d))


def test_alpha_channel_scale_bias_and_per_sample_filters():
    B, Cin, Cout = 2, 4, 6
    x = rnd(B, Cin, 8, 8, seed=15)
    ws = rnd(B, Cout, Cin, 3, 3, seed=16)
    sc, b = rnd(B, Cout, seed=17), rnd(Cout, seed=18)
    tab = torch.stack([ohwi(ws[i]) for i in range(B)])
    r = CR.conv_ref(x, tab, b, 1, 1, 1, alpha=0.25, ch_scale=sc)
    ref = torch.cat([0.25 * F.conv2d(x[i:i + 1], ws[i], None, padding=1) * sc[i].view(1, -1, 1, 1) for i in range(B)]) + b.view(1, -1, 1, 1)
    close(r.y, ref)
    close(r.S, torch.cat([F.conv2d(x[i:i + 1].abs(), ws[i].abs(), None, padding=1) for i in range(B)]))      # S carries no alpha / scale
    r1 = CR.conv_ref(x, tab[0], None, 1, 1, 1, ch_scale=sc[0])
    close(r1.y, F.conv2d(x, ws[0], None, padding=1) * sc[0].view(1, -1, 1, 1))


@pytest.mark.parametrize('act', PR.ACTS)
def test_activations_and_accumulate_modes(act):
    x, w, b = rnd(2, 4, 7, 6, seed=19), rnd(5, 4, 3, 3, seed=20), rnd(5, seed=21)
    pre = F.conv2d(x, w, b, padding=1)
    fn = {'none': lambda t: t, 'elu': F.elu, 'relu': F.relu, 'lrelu': lambda t: F.leaky_relu(t, 0.2), 'sigmoid': torch.sigmoid, 'clamp': lambda t: t.clamp(-1, 1)}[act]
    y0 = rnd(*pre.shape, seed=22)
    close(CR.conv_ref(x, ohwi(w), b, 1, 1, 1, act=act).y, fn(pre))
    close(CR.conv_ref(x, ohwi(w), b, 1, 1, 1, act=act, accumulate=1, y_old=y0).y, y0 + fn(pre))
    close(CR.conv_ref(x, ohwi(w), b, 1, 1, 1, act=act, accumulate=2, y_old=y0).y, fn(pre + y0))


@pytest.mark.parametrize('mact', ['elu', 'lrelu', 'relu', 'sigmoid', 'clamp'])
def test_order_is_act_then_factor_then_accumulate_1(mact):
    x, w = rnd(2, 4, 6, 6, seed=23), rnd(5, 4, 3, 3, seed=24)
    m = rnd(2, 5, 6, 6, seed=25) * 1.5
    if mact == 'sigmoid':
        m = torch.sigmoid(m)
    y0 = rnd(2, 5, 6, 6, seed=26)
    fac = PR.act_grad_from_out_formula(m, mact)
    a = F.elu(F.conv2d(x, w, None, padding=1))
    r = CR.conv_ref(x, ohwi(w), None, 1, 1, 1, act='elu', mul=m, mul_act=mact, accumulate=1, y_old=y0)
    close(r.y, y0 + a * fac)
    close(r.a, a)
    close(r.r, a * fac)
    assert bool((fac != 1).any())
    # the factor is decided on the STORED m: an fp16-stored tiny positive m that rounded to 0 takes the non-positive branch
    m16 = torch.full((2, 5, 6, 6), 1e-9).half()
    if mact in ('lrelu', 'relu'):
        want = {'lrelu': 0.2, 'relu': 0.0}[mact]
        assert bool((CR.conv_ref(x, ohwi(w), None, 1, 1, 1, mul=m16, mul_act=mact).fac == want).all())


def test_mul_factor_is_the_autograd_data_gradient_of_the_producer():
    """conv_ref(transposed, mul = (producer output, its activation)) == d/d(pre-activation) through act and the convolution."""
    pre = rnd(2, 4, 8, 6, seed=27).requires_grad_(True)
    w = rnd(5, 4, 3, 3, seed=28)
    low = F.elu(pre)
    y = F.conv2d(low, w, None, stride=2, padding=1)
    g = rnd(*y.shape, seed=29)
    y.backward(g)
    r = CR.conv_ref(g, ohwi_T(w), None, 2, 1, 1, transposed=True, out_hw=(8, 6), mul=low.detach(), mul_act='elu')
    close(r.y, pre.grad)


@pytest.mark.parametrize('act', ['none', 'elu', 'relu'])
def test_pooled_data_gradient_matches_autograd_through_interpolate(act):
    pre = rnd(2, 4, 5, 6, seed=30).requires_grad_(True)
    fn = {'none': lambda t: t, 'elu': F.elu, 'relu': F.relu}[act]
    low = fn(pre)
    w = rnd(3, 4, 3, 3, seed=31)
    y = F.conv2d(F.interpolate(low, scale_factor=2, mode='nearest'), w, None, padding=1)
    g = rnd(*y.shape, seed=32)
    y.backward(g)
    y0 = rnd(2, 4, 5, 6, seed=33)
    kw = dict(mul=low.detach(), mul_act=act) if act != 'none' else {}
    r = CR.conv_ref(g, ohwi_T(w), None, 1, 1, 1, transposed=True, pool2=True, **kw)
    close(r.y, pre.grad)
    close(CR.conv_ref(g, ohwi_T(w), None, 1, 1, 1, transposed=True, pool2=True, accumulate=1, y_old=y0, **kw).y, y0 + pre.grad)
    full = CR.conv_ref(g, ohwi_T(w), None, 1, 1, 1, transposed=True).y.abs()
    close(r.P, 4 * F.avg_pool2d(full, 2))


def test_extra_channel_matches_the_materialised_concat():
    K = 4
    low, x1 = rnd(2, K, 5, 6, seed=34), rnd(2, 1, 10, 12, seed=35)
    w, b = rnd(3, K + 1, 3, 3, seed=36), rnd(3, seed=37)
    cat = torch.cat([F.interpolate(low, scale_factor=2, mode='nearest'), x1], 1)
    tab = ohwi(w)
    r = CR.conv_ref(low, tab[:, :, :K], b, 1, 1, 1, in_shift=1, act='elu', x1=x1, w1=tab[:, :, K])
    close(r.y, F.elu(F.conv2d(cat, w, b, padding=1)))
    close(r.S, F.conv2d(cat.abs(), w.abs(), None, padding=1))


def test_operands_are_taken_as_stored():
    x16 = rnd(1, 2, 4, 4, seed=38).half()
    w16 = rnd(2, 9, 2, seed=39).half()
    close(CR.conv_ref(x16, w16, None, 1, 1, 1).y, CR.conv_ref(x16.double(), w16.double(), None, 1, 1, 1).y, 0.0)


def test_statistics_of_the_stored_output():
    y = rnd(3, 5, 4, 6, seed=40).half()
    s, q = CR.stats_ref(y)
    assert s.shape == q.shape == (3, 5) and s.dtype == F64
    for n in range(3):
        for c in range(5):
            v = [float(t) for t in y[n, c].flatten()]
            assert abs(s[n, c].item() - sum(v)) <= 1e-12 and abs(q[n, c].item() - sum(t * t for t in v)) <= 1e-12
