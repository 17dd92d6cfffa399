"""Pins tests/weight_ref.py (the fp64 references of the weight path of csrc/prep.hip) against torch -- torch.nn.utils.spectral_norm, float64 autograd,
torch.optim.Adam -- and measures that the a-priori bounds tests/test_weight_path_gpu.py uses have teeth.  No GPU.

The mutation check.  For every small device case, each mutant below -- the reference with one subtle defect of the kind a kernel could have -- is compared
with the true reference on the case's own inputs, in units of the bound the device test applies to that output.  A case's figure for a mutant is the
largest such ratio over the outputs the device test checks for that case, the run on exact-arithmetic inputs included (multiples of 1/8: the device
value must equal the fp64 value bit for bit, so ANY difference is infinitely far outside); it must exceed 8, which leaves the kernel's own rounding
(at most 1x the bound) no room to hide the defect.  The figures are printed (pytest -s).  The single-element mutants of a long dot are caught by the
exact-arithmetic run and not by the random one, whose order-independent dot bound grows with n^2 -- which is what that run is for.
Exempt: the limit-size spectral-norm cases (K = 4608, Cout = 1024), whose dot bound is too loose for single-element mutants on random inputs; they
are run on the device all the same, with the exact-arithmetic inputs too."""
import math

import pytest
import torch
import torch.nn as nn

import weight_ref as WR

INF = float('inf')


def ratio(mut, ref, bound):
    err = (torch.as_tensor(mut, dtype=torch.float64) - torch.as_tensor(ref, dtype=torch.float64)).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(err)
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)      # a difference against a zero bound (bit-exact outputs): inf
    return r.max().item() if r.numel() else 0.0


# ---------------------------------------------------------------------------------------------------------------- the references against torch
@pytest.mark.parametrize('cout,cin,k', [(7, 5, 3), (16, 3, 1), (5, 12, 4)])
def test_spectral_norm_ref_is_torch_spectral_norm(cout, cin, k):
    torch.manual_seed(cout + cin)
    m = nn.utils.spectral_norm(nn.Conv2d(cin, cout, k).double())
    x = torch.randn(1, cin, k, k, dtype=torch.float64)
    W = m.weight_orig.detach().reshape(cout, -1).clone()
    with torch.no_grad():      # not unit vectors: the hook has to normalise, not to keep
        m.weight_u.mul_(0.7)
        m.weight_v.mul_(1.3)
    u0, v0 = m.weight_u.clone(), m.weight_v.clone()
    m.train()
    m(x)
    sigma, u1, v1 = WR.spectral_norm_ref(W, u0, v0, True)
    for got, want in ((u1, m.weight_u), (v1, m.weight_v), (W / sigma, m.weight.detach().reshape(cout, -1))):
        assert (got - want).abs().max().item() <= 1e-13 * max(1.0, want.abs().max().item())
    m.eval()
    m(x)
    s0, u2, v2 = WR.spectral_norm_ref(W, u1, v1, False)
    assert torch.equal(u2, u1) and torch.equal(v2, v1)
    assert abs(float(s0 - torch.dot(m.weight_u, W @ m.weight_v))) <= 1e-13 * abs(float(s0))
    assert (W / s0 - m.weight.detach().reshape(cout, -1)).abs().max().item() <= 1e-13
    # eps: a zero W^T u stays zero instead of dividing by zero
    z, _, vz = WR.spectral_norm_ref(torch.zeros(3, 4), torch.ones(3), torch.ones(4), True)
    assert float(z) == 0.0 and float(vz.abs().max()) == 0.0


@pytest.mark.parametrize('transposed', [False, True])
@pytest.mark.parametrize('accumulate', [False, True])
def test_weight_prep_backward_ref_is_autograd_of_w_over_sigma(transposed, accumulate):
    """d/dW of <dW_sn, W / (u . (W_mat v))> with u, v detached; for the conv-transpose layout W is [Cin][Cout][taps] and W_mat its dim-1 matricisation
    (torch.nn.utils.spectral_norm(..., dim=1))."""
    cout, cin, taps = 6, 5, 4
    gen = torch.Generator().manual_seed(3)
    shape = (cin, cout, taps) if transposed else (cout, cin, taps)
    W = torch.randn(*shape, generator=gen, dtype=torch.float64, requires_grad=True)
    u, v = torch.randn(cout, generator=gen, dtype=torch.float64), torch.randn(cin * taps, generator=gen, dtype=torch.float64)
    dWsn = torch.randn(*shape, generator=gen, dtype=torch.float64)
    before = torch.randn(W.numel(), generator=gen, dtype=torch.float64)
    mat = (W.permute(1, 0, 2) if transposed else W).reshape(cout, cin * taps)
    sigma = torch.dot(u, mat @ v)
    Wsn = W / sigma
    (Wsn * dWsn).sum().backward()
    # kernel-side tensors: [rows][taps][CinP], the padding channels holding a sentinel (gradient) / zero (weights)
    width = cout if transposed else cin
    CinP = WR.rup(width, 4)
    dw = torch.full((shape[0], taps, CinP), 7.5, dtype=torch.float64)
    dw[:, :, :width] = dWsn.permute(0, 2, 1)
    wf = torch.zeros(shape[0], taps, CinP, dtype=torch.float64)
    wf[:, :, :width] = Wsn.detach().permute(0, 2, 1)
    dot, out = WR.weight_prep_backward_ref(dw, wf, u, v, sigma.detach(), cout, cin, taps, CinP, True, transposed, before, accumulate)
    want = W.grad.reshape(-1) + (before if accumulate else 0)
    assert abs(float(dot - (dWsn * Wsn.detach()).sum())) <= 1e-13
    assert (out - want).abs().max().item() <= 1e-12 * want.abs().max().item()
    _, plain = WR.weight_prep_backward_ref(dw, wf, None, None, None, cout, cin, taps, CinP, False, transposed, before, accumulate)
    assert torch.equal(plain, dWsn.reshape(-1) + (before if accumulate else 0))


@pytest.mark.parametrize('step', WR.ADAM_STEPS)
def test_adam_ref_is_torch_adam_on_the_rounded_hyper_parameters(step):
    h = WR.adam_hyper32()
    p, g, m, v = (t.double() for t in WR.adam_inputs(4099, step))
    q = p.clone().requires_grad_(True)
    q.grad = g.clone()
    opt = torch.optim.Adam([q], lr=h['lr'], betas=(h['beta1'], h['beta2']), eps=h['eps'])
    opt.state[q] = {'step': torch.tensor(float(step - 1)), 'exp_avg': m.clone(), 'exp_avg_sq': v.clone()}
    opt.step()
    rp, rm, rv, upd = WR.adam_ref(p, g, m, v, step, h['lr'], h['beta1'], h['beta2'], h['eps'])
    st = opt.state[q]
    assert float(st['step']) == step
    assert ((rm - st['exp_avg']).abs() <= 1e-14 * rm.abs()).all()
    assert ((rv - st['exp_avg_sq']).abs() <= 1e-14 * rv.abs()).all()
    assert ((rp - q.detach()).abs() <= 1e-12 * upd.abs() + 1e-18).all()
    # the Python double 0.999 is not the kernel's beta2: 1 - beta2^step differs by 3e-5 relative at step 1 (the reason for the rounded hyper-parameters)
    if step == 1:
        assert abs((1 - h['beta2']) / (1 - 0.999) - 1) > 1e-5


def test_unscale_check_ref_pins_the_guard_contract():
    g = torch.tensor([0.0, -0.0, 1e-40, -3.0e38, 3.0e38, 1.5])
    out, bad = WR.unscale_check_ref(g, 2.0 ** -7)
    assert not bad and torch.equal(out, g.double() / 128)
    for x in (float('inf'), -float('inf'), float('nan'), 3.4e38, -3.1e38):
        assert WR.unscale_check_ref(torch.tensor([1.0, x, 2.0]), 1.0)[1], x


def test_weight_tables_ref_layouts():
    cout, cin, taps = 3, 5, 2
    W = torch.arange(1, cout * cin * taps + 1, dtype=torch.float32)
    t = WR.weight_tables_ref(W, 2.0, cout, cin, taps, 8, cout, 4, 8)
    assert t['w_fwd'].shape == (3, 2, 8) and t['w_bwd'].shape == (8, 2, 4)
    for co in range(cout):
        for ci in range(cin):
            for tap in range(taps):
                want = W[(co * cin + ci) * taps + tap] / 2
                assert t['w_fwd'][co, tap, ci] == want and t['w_bwd'][ci, tap, co] == want
    assert float(t['w_fwd'][:, :, cin:].abs().max()) == 0 and float(t['w_bwd'][cin:].abs().max()) == 0 and float(t['w_bwd'][:, :, cout:].abs().max()) == 0
    tt = WR.weight_tables_ref(W, 2.0, cout, cin, taps, 8, cout, 4, 8, transposed_src=True)
    assert tt['w_fwd'][2, 1, 4] == W[(4 * cout + 2) * taps + 1] / 2
    # fragment order: 16 rows x 32 channels, lane-major pieces of 8 halfs
    f = WR.weight_tables_ref(torch.randn(16 * 32), 1.0, 16, 32, 1, 32, 16, 16, 32)
    assert f['w_fwd_t'][(2 * 16 + 5) * 8 + 3] == f['w_fwd_h'][5, 0, 2 * 8 + 3] and bool(f['w_fwd_t_real'].all())


# ---------------------------------------------------------------------------------------------------------------- the mutation check
def sn_mutant(W, u, v, power_iter, kind):
    W, u, v = W.double(), u.double(), v.double()
    co, K = W.shape
    rows = co - 1 if kind == 'row_last' else co      # the last filter row dropped from every sum over rows
    u_in = u

    def Wv(x):
        s = W @ x
        if kind == 'k_last':                          # the last element of K dropped from one dot
            s[co - 1] -= W[co - 1, K - 1] * x[K - 1]
        return s

    if power_iter:
        t = W[:rows].t() @ u[:rows]
        v = t if kind == 'v_raw' else WR.normalize(t)      # v not renormalised
        s = Wv(v)
        un = torch.zeros_like(u)
        un[:rows] = WR.normalize(s[:rows])
        u = un
        sig_u = u_in if kind == 'sigma_pre_u' else u         # sigma from the pre-iteration u
        return torch.dot(sig_u[:rows], s[:rows]), u, v
    return torch.dot(u[:rows], Wv(v)[:rows]), u, v


SN_MUTANTS = {'k_last': (0, 1), 'row_last': (0, 1), 'sigma_pre_u': (1,), 'v_raw': (1,)}      # mutant -> the power_iter modes it lives in


@pytest.mark.parametrize('shape', WR.SN_SMALL, ids=['%dx%dx%d' % s for s in WR.SN_SMALL])
def test_mutants_of_spectral_norm_land_outside_the_bounds(shape):
    """A shape's device checks: sigma, u', v' with power_iter on random inputs, sigma without on random inputs and -- bit for bit -- on exact-arithmetic
    inputs.  The W v loop (k_last, row_last) is the same code in both modes; on the two largest small shapes its single-element mutant stays inside
    the propagated bound of the power_iter run (0.2 and 3 x) and is caught by the exact-arithmetic run of the same loop."""
    We, ue, ve = WR.sn_inputs(*shape, exact=True)
    assert WR.exact_ok((ue.double().abs() @ We.double().abs() @ ve.double().abs()), 512)
    W, u, v = WR.sn_inputs(*shape)
    for kind, modes in SN_MUTANTS.items():
        r = {}
        for pi in modes:
            ref, bounds, mut = WR.spectral_norm_ref(W, u, v, pi), WR.spectral_norm_bounds(W, u, v, pi), sn_mutant(W, u, v, pi, kind)
            r['sigma pi=%d' % pi] = ratio(mut[0], ref[0], bounds[0])
            if pi:
                r['u'], r['v'] = ratio(mut[1], ref[1], bounds[1]), ratio(mut[2], ref[2], bounds[2])
            else:
                r['exact-input sigma'] = ratio(sn_mutant(We, ue, ve, 0, kind)[0], WR.spectral_norm_ref(We, ue, ve, 0)[0], 0.0)
        print('sn %-10s %-12s %s' % ('%dx%dx%d' % shape, kind, '  '.join('%s %.3g' % kv for kv in r.items())))
        assert max(r.values()) > 8, (shape, kind, r)


def test_mutant_transposed_indexing_changes_the_tables():
    for cout, cin, k in WR.TRANSPOSED_SHAPES + WR.SN_SMALL[1:]:
        taps = k * k
        W = torch.randn(cout * cin * taps, generator=torch.Generator().manual_seed(1))
        a = WR.weight_tables_ref(W, 1.25, cout, cin, taps, WR.rup(cin, 4), cout, WR.rup(cout, 4), WR.rup(cin, 4), transposed_src=True)
        b = WR.weight_tables_ref(W, 1.25, cout, cin, taps, WR.rup(cin, 4), cout, WR.rup(cout, 4), WR.rup(cin, 4), transposed_src=False)
        for name in ('w_fwd', 'w_bwd', 'w_fwd_h', 'w_bwd_h'):      # compared bit for bit on the device: any difference is outside
            r = ratio(a[name].double(), b[name].double(), 0.0)
            print('tables %dx%dx%d transposed_src swapped %-8s %.3g' % (cout, cin, k, name, r))
            assert r > 8


@pytest.mark.parametrize('accumulate', [0, 1])
@pytest.mark.parametrize('sn', [0, 1])
@pytest.mark.parametrize('name', sorted(WR.BWD_CASES))
def test_mutants_of_the_backward_land_outside_the_bounds(name, sn, accumulate):
    cout, cin, taps = WR.BWD_CASES[name]
    figures = {}
    for exact in (False, True):
        I = WR.bwd_inputs(cout, cin, taps, exact=exact)
        ref_dot, ref, bdot, bout = WR.bwd_bounds(I, cout, cin, taps, sn, accumulate, exact)
        if accumulate:      # `accumulate` ignored
            _, mut = WR.weight_prep_backward_ref(I['dw_ohwi'], I['w_fwd'], I['u'], I['v'], I['sigma'], cout, cin, taps, I['CinP'], sn, False, I['before'], 0)
            figures.setdefault('accumulate_ignored', []).append(ratio(mut, ref, bout))
        if sn:              # the dot's last float4 dropped
            last4 = (I['dw_ohwi'].double() * I['w_fwd'].double()).reshape(-1)[-4:].sum()
            _, mut = WR.weight_prep_backward_ref(I['dw_ohwi'], I['w_fwd'], I['u'], I['v'], I['sigma'], cout, cin, taps, I['CinP'], sn, False, I['before'],
                                                 accumulate, dot=ref_dot - last4)
            figures.setdefault('dot_last_float4', []).extend([ratio(ref_dot - last4, ref_dot, bdot), ratio(mut, ref, bout)])
    for kind, r in figures.items():
        print('bwd %-7s sn=%d acc=%d %-18s %s' % (name, sn, accumulate, kind, ' '.join('%.3g' % x for x in r)))
        assert max(r) > 8, (name, sn, accumulate, kind, r)


@pytest.mark.parametrize('name', sorted(WR.BWD_TRANSPOSED))
def test_mutant_transposed_indexing_changes_the_backward(name):
    cout, cin, taps = WR.BWD_TRANSPOSED[name]
    I = WR.bwd_inputs(cout, cin, taps, transposed_src=True)
    _, ref = WR.weight_prep_backward_ref(I['dw_ohwi'], I['w_fwd'], None, None, None, cout, cin, taps, I['CinP'], 0, True, I['before'], 0)
    mut = ref.reshape(cin, cout, taps).permute(1, 0, 2).reshape(-1)      # written [Cout][Cin][taps]
    r = ratio(mut, ref, 0.0)
    print('bwd %s transposed_src swapped %.3g' % (name, r))
    assert r > 8


def adam_mutant(p, g, m, v, step, h, kind):
    d = lambda x: torch.as_tensor(x, dtype=torch.float64)
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    b1, b2, lr, eps = d(h['beta1']), d(h['beta2']), d(h['lr']), d(h['eps'])
    bc1 = 1 - b1 ** step
    bc2 = 1 - b2 ** (step - 1 if kind == 'beta2_step_minus_1' else step)
    m1 = m + (g - m) * (1 - b1)
    v1 = v * b2 + (1 - b2) * g * g
    denom = torch.sqrt(v1 / bc2 + eps) if kind == 'eps_inside_root' else torch.sqrt(v1) / torch.sqrt(bc2) + eps
    return p - (lr / bc1) * (m1 / denom), m1, v1


@pytest.mark.parametrize('step', WR.ADAM_STEPS)
def test_mutants_of_adam_land_outside_the_bounds(step):
    """The device test's table: tensors of ADAM_SIZES elements back to back in one flat buffer, one reference and one set of bounds over all of it."""
    h = WR.adam_hyper32()
    N = sum(WR.ADAM_SIZES)
    p, g, m, v = WR.adam_inputs(N, step)
    ref, bounds = WR.adam_bounds(p, g, m, v, step, h)
    for kind in ('beta2_step_minus_1', 'eps_inside_root'):
        mut = adam_mutant(p, g, m, v, step, h, kind)
        r = ratio(torch.nan_to_num(mut[0], nan=INF), ref[0], bounds[0])
        print('adam step %-4d %-20s p %.3g' % (step, kind, r))
        assert r > 8, (step, kind, r)
    end = 0
    for n in WR.ADAM_SIZES:      # the last element of a tensor not updated
        end += n
        r = [ratio(before[end - 1].double(), rf[end - 1], b[end - 1]) for before, rf, b in zip((p, m, v), ref[:3], bounds)]
        print('adam step %-4d last element of n=%-5d p %.3g  m %.3g  v %.3g' % (step, n, *r))
        assert max(r) > 8, (step, n, r)
