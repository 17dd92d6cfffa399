"""hv_conv2d / hv_conv2d_wgrad on channel-slice views inside guarded buffers against the float64 references of tests/conv_ref.py (pinned by
tests/test_conv_ref_cpu.py).

Every operand lives in a hvtest.Guarded buffer (NaN guards on both sides) and is an ops.Act over channels [coff, coff + C) of an ld-wide pixel row.  The
channels outside a view hold NaN where the kernel reads (x, mul, g, x1, bn_x) and the fp16-exact 7.5 where it writes; after every call the guards must be
intact, the foreign channels of a written buffer must still hold 7.5 bit for bit, and the result must be finite (a NaN = a neighbour's channel was
read, or an element was never written).  Workspaces are exactly the queried bytes (hvtest.ExactWs).  The forms without a fallback (pool2, x1, xn, stats,
bstats) run on all five view settings too: where ConvCall.supported() says no, launch() must raise and the output buffer must keep every bit.

View settings (ld - C, coff, base offset in elements): whole (0, 0, 0) -- the control; slice8 (16, 8, 0) -- every fast path kept; slice4 (12, 4, 0) -- the
16-byte epilogues off; odd (3, 1, 0) -- every vector path off, or the next family; base -- whole, but the base pointer only 8-, 4-, 2-byte aligned.  The
kernel path is asserted on whole and slice8 and only recorded on the others.  hv_conv2d_wgrad has no element-wise form: it refuses (HV_ERR_UNSUPPORTED
from its validation, conv_igemm.hip wgrad_validate) views whose strides / offsets are not multiples of 4 or whose bases are not 16-byte aligned -- there
the test asserts the refusal and that nothing was written.

Bounds, per element, from float64 reference quantities only (u = 2^-24; n = taps x Cin, or B x Ho x Wo for a weight gradient; S = the contraction over
|x| and |w|):  fp16 operands with fp32 accumulation (n + 16) u alpha S; fp32 mode (2n + 16) u alpha S; + ONE 4u |ref| for bias / scale / factor / accumulate,
|ref| being the largest stage of the element (argument of act, act, times factor, final); through an
activation (all of them are 1-Lipschitz) + 4 x the largest error of a plain fp32 torch evaluation of it on the CPU; with an act' factor into fp16 storage
+ max(2^-11 |a|, 2^-25) |factor| ONLY for the kernels named in STAGED below, whose fp16 epilogue rounds the tile to fp16 before it applies the factor
(the gather kernel and conv_px_kernel multiply in fp32: no such term); a value stored as fp16
+ max(2^-11 |ref|, 2^-25), with accumulate = 1 once more on |y_old + r|; pool2 + 2^-11 x the sum of the four |outputs|.  In the fp16 mode all operand
values are fp16-exact whatever their storage, so a kernel that rounds an fp32-stored image at staging and one that does not compute the same sum.
The worst error / bound per family is printed at the end of the module (pytest -s)."""
import functools

import pytest
import torch

import conv_ref as CR
import pointwise_ref as PR
from test_norm_act_gpu import Check, SENT, U, others_untouched, print_ratios, same_bits, tol_elem

pytestmark = pytest.mark.gpu

ops = T = lib = None
VIEWS = {'whole': (0, 0), 'slice8': (16, 8), 'slice4': (12, 4), 'odd': (3, 1), 'base': (0, 0)}


@pytest.fixture(scope='module', autouse=True)
def _env():
    global ops, T, lib
    import hvgan  # noqa: F401
    from hvgan import lib as _lib, ops as _ops
    import hvtest as _T
    ops, T, lib = _ops, _T, _lib
    yield
    print_ratios('conv.')


@pytest.fixture(autouse=True)
def _no_launch_after_a_device_error():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:      # a faulted context fails every later call: end the session instead of launching on
        pytest.exit('device error, nothing more is launched: %s' % e, returncode=3)


def path():
    return lib.get().size('hv_last_kernel_path')


def kname():
    return (lib.get().cdll.hv_last_kernel_name() or b'').decode()


def bits(t):
    return t.contiguous().view(torch.uint8).clone()


def operand(data, dtype, view, off, fill):
    """(B, C, H, W) CPU values -> (Guarded, Act) over channels [coff, coff + C) of an ld-wide buffer whose other channels hold `fill`."""
    B, C, H, W = data.shape
    extra, coff = VIEWS[view]
    buf = torch.full((B, H, W, C + extra), fill, dtype=dtype)
    buf[..., coff:coff + C] = data.permute(0, 2, 3, 1).to(dtype)
    G = T.Guarded((B, H, W, C + extra), dtype=dtype, guard=64, offset=off, data=buf)
    return G, ops.Act(G.t, C, coff)


def view_of(a):
    return a.t[..., a.coff:a.coff + a.C].permute(0, 3, 1, 2).contiguous().cpu()


def offsets(dtype):      # base pointers 8-, 4- (and 2-) byte aligned, in elements
    return (4, 2, 1) if dtype == torch.float16 else (2, 1)


# ---------------------------------------------------------------------------------------------------------------- forward / data gradient
CASES = {}


def case(name, fam, B, H, W, Cin, Cout, k, path=None, **kw):
    d = dict(fam=fam, B=B, H=H, W=W, Cin=Cin, Cout=Cout, k=k, s=1, p=1, d=1, tr=False, shift=0, prec='fp16', act='none', bias=False, alpha=1.0, scale=False,
             per_sample=False, acc=0, mul=None, wh=True, wt=False, path=path, kname=None, s2t=None, xdt=None, ydt=None, live=None, out_hw=None, pool2=False,
             x1=False, stats=False, p8=path, nofb=False)
    d.update(kw)
    CASES[name] = d


# gather kernel (path 0): no fp16 filter copy, so no tiled family applies
for pr in ('fp32', 'fp16'):
    g = dict(prec=pr, wh=False)
    case('gather_%s_k3' % pr, 'gather', 2, 12, 10, 6, 10, 3, 0, bias=True, act='elu', **g)
    case('gather_%s_vec' % pr, 'gather', 2, 12, 10, 8, 12, 3, 0, bias=True, act='lrelu', alpha=0.5, **g)
    case('gather_%s_s2' % pr, 'gather', 2, 12, 10, 6, 10, 3, 0, s=2, act='relu', **g)
    case('gather_%s_d2' % pr, 'gather', 2, 12, 10, 6, 10, 3, 0, p=2, d=2, bias=True, act='sigmoid', **g)
    case('gather_%s_tr4' % pr, 'gather', 2, 12, 10, 6, 10, 4, 0, s=2, tr=True, **g)
    case('gather_%s_persample' % pr, 'gather', 2, 16, 8, 6, 10, 3, 0, per_sample=True, scale=True, **g)
    case('gather_%s_acc1' % pr, 'gather', 2, 12, 10, 8, 12, 3, 0, act='elu', acc=1, mul='lrelu', **g)
    case('gather_%s_acc2' % pr, 'gather', 2, 12, 10, 6, 10, 3, 0, act='clamp', acc=2, bias=True, **g)
    case('gather_%s_mul_elu' % pr, 'gather', 2, 12, 10, 8, 12, 3, 0, tr=True, mul='elu', **g)
    case('gather_%s_shift' % pr, 'gather', 2, 6, 5, 6, 10, 3, 0, shift=1, bias=True, **g)
# narrow / thin-input VALU kernels (paths 1 and 4), fp32
case('narrow3_12to1', 'narrow', 2, 12, 10, 12, 1, 3, 1, prec='fp32', wh=False, bias=True, act='sigmoid')
case('narrow_16to1_s2', 'narrow', 2, 12, 10, 16, 1, 3, 1, prec='fp32', wh=False, s=2, bias=True, act='clamp')
case('thin1_1to64', 'thin1', 2, 20, 22, 1, 64, 4, 4, prec='fp32', wh=False, s=2, bias=True, act='lrelu')
# one-channel stems (fp32 image in, fp16 map out) and the 5x5 stems
case('stem1_16', 'stem1', 3, 20, 22, 1, 16, 4, 4, bias=True, act='elu', xdt='f32', kname='stem1_mfma_kernel')
case('stem1_64_s2', 'stem1', 2, 18, 14, 1, 64, 4, 4, s=2, bias=True, act='lrelu', xdt='f32', kname='stem1_mfma_kernel<true>')
case('stem1_64_acc1', 'stem1', 2, 18, 14, 1, 64, 4, 4, s=2, bias=True, act='lrelu', acc=1, xdt='f32', kname='stem1_mfma_kernel')
case('stem5_fwd', 'stem5', 2, 16, 16, 4, 16, 5, 4, p=2, bias=True, act='elu', kname='stem5_lds_kernel')
case('stem5_dgrad', 'stem5', 2, 16, 16, 16, 4, 5, 4, p=2, tr=True, kname='stem5_dgrad_kernel')
# 3x3 halo families
case('halo_16to16', 'halo', 2, 16, 16, 16, 16, 3, (2, 3), bias=True, act='elu')      # (16-channel chunks on 8x16 tiles: conv_halo2_kernel has an instantiation)
case('halo_32to48_k4', 'halo', 2, 9, 11, 32, 48, 4, 2, bias=True, act='lrelu')
case('halo_64to32_s2', 'halo', 2, 18, 22, 64, 32, 3, 2, s=2, bias=True, act='elu')
case('halo_16to16_dgrad_mul', 'halo', 2, 16, 16, 16, 16, 3, (2, 3), tr=True, mul='elu', acc=1)
case('halo2_32to16', 'halo2', 2, 18, 22, 32, 16, 3, 3, bias=True, act='elu')
case('halo2_64to64_d2', 'halo2', 2, 20, 12, 64, 64, 3, 3, p=2, d=2, bias=True, act='elu')
case('halo2_64to64_d2_dgrad', 'halo2', 2, 20, 12, 64, 64, 3, 3, p=2, d=2, tr=True, mul='elu')
# filters in LDS (path 7): the fragment-ordered table
case('lf_32to32', 'lf', 2, 18, 22, 32, 32, 3, 7, wt=True, bias=True, act='elu', kname='conv_lf_kernel')
case('lf_32to32_dgrad', 'lf', 2, 18, 22, 32, 32, 3, 7, wt=True, tr=True, mul='elu', acc=1, kname='conv_lf_kernel')
case('lf2_16to32_s2', 'lf', 2, 33, 47, 16, 32, 3, 7, wt=True, s=2, bias=True, act='elu', kname='conv_lf2_kernel')
case('lfd_64to64_d8', 'lf', 1, 64, 64, 64, 64, 3, 7, wt=True, p=8, d=8, bias=True, act='elu', kname='conv_lfd_kernel')
case('pool2_32to32', 'pool2', 2, 16, 24, 32, 32, 3, 7, wt=True, tr=True, pool2=True, mul='elu', nofb=True)
case('pool2_32to32_acc1', 'pool2', 2, 16, 24, 32, 32, 3, 7, wt=True, tr=True, pool2=True, mul='relu', acc=1, nofb=True)
case('x1_32', 'x1', 2, 8, 12, 32, 32, 3, 7, wt=True, shift=1, x1=True, bias=True, act='elu', nofb=True)
# conv_g4_kernel (path 8)
case('g4_fwd_s2', 'g4', 2, 16, 16, 32, 128, 4, 8, wt=True, s=2, bias=True, act='lrelu', stats=True)
case('g4_fwd_s1', 'g4', 2, 9, 9, 32, 128, 4, 8, wt=True, bias=True, stats=True)
case('g4_dgrad_s2', 'g4', 2, 8, 8, 128, 64, 4, 8, wt=True, s=2, tr=True, out_hw=(16, 16))
case('g4_dgrad_s2_mul', 'g4', 2, 8, 8, 128, 64, 4, 8, wt=True, s=2, tr=True, out_hw=(16, 16), mul='lrelu', acc=1)
case('g4_dgrad_s1_mul', 'g4', 2, 8, 8, 128, 128, 4, 8, wt=True, tr=True, mul='lrelu')
case('g4_dgrad_s2_mul0', 'g4', 2, 8, 8, 128, 64, 4, 8, wt=True, s=2, tr=True, out_hw=(16, 16), mul='lrelu')
# conv_s2t_kernel (path 6), mode 2
case('s2t_k3', 's2t', 2, 8, 12, 16, 16, 3, 6, s=2, tr=True, out_hw=(16, 24), mul='lrelu', s2t=2)
case('s2t_k3_acc1', 's2t', 2, 8, 12, 16, 16, 3, 6, s=2, tr=True, out_hw=(16, 24), acc=1, s2t=2)
case('s2t_k4', 's2t', 3, 6, 10, 72, 40, 4, 6, s=2, tr=True, out_hw=(12, 20), mul='lrelu', s2t=2)
# head_gemm_kernel (path 5): Cout == 1 with the [pixel][tap] table in the workspace
case('head_64to1', 'head', 2, 9, 11, 64, 1, 4, 5, bias=True, act='sigmoid')
case('head_64to1_acc2', 'head', 2, 9, 11, 64, 1, 4, 5, act='lrelu', acc=2)
case('head_128_tr', 'head', 2, 15, 15, 128, 1, 3, 5, tr=True, mul='lrelu')
# taps-as-contraction data gradients (path 9) and conv_px_kernel (path 14)
case('logits_dgrad', 'taps', 2, 6, 6, 4, 32, 4, 9, tr=True, live=1, mul='lrelu', p8=None)
case('logits_dgrad_acc1', 'taps', 2, 6, 6, 4, 32, 4, 9, tr=True, live=1, acc=1, p8=None)
case('thin3_dgrad', 'taps', 3, 19, 16, 4, 16, 3, (9, 14), tr=True, mul='elu', acc=1, p8=None)
case('px_8to1', 'px', 1, 5, 3, 8, 1, 3, 14)
case('px_8to1_clamp', 'px', 2, 9, 260, 8, 1, 3, 14, bias=True, act='clamp')
case('px_4to8_tr_mul', 'px', 2, 9, 260, 4, 8, 3, 14, tr=True, mul='elu', p8=None)


def dt_of(c, which):
    o = c['xdt'] if which == 'x' else c['ydt']
    if o is not None:
        return torch.float32 if o == 'f32' else torch.float16
    if c['prec'] == 'fp32':
        return torch.float32
    return torch.float32 if (which == 'y' and c['Cout'] == 1) else torch.float16


# Kernels whose fp16 epilogue stages the (alpha, bias, activation) tile in LDS AS fp16 and applies the act' factor to that rounded value -- conv_halo.hip:226
# then :247 `v8[e] = (_Float16)((float)v8[e] * f0[e])`, the same form at conv_halo2.hip:301, conv_s2t.hip:189, conv_lf.hip:370, conv_g4.hip:155 and
# conv_thin.hip:182 (logits_dgrad_kernel / thin_dgrad_kernel).  The gather kernel and conv_px_kernel apply the factor in fp32: no such term for them.
STAGED = ('conv_halo_kernel', 'conv_halo2_kernel', 'conv_s2t_kernel', 'conv_lf', 'conv_g4', 'logits_dgrad_kernel', 'thin_dgrad_kernel')


@functools.lru_cache(maxsize=None)
def bn_inputs(name):
    """bn_x (stored values, the output's pixels and channels) and the saved [1][2][Cout] mean / rstd of a batch-norm backward-sums case."""
    I = conv_inputs(name)
    gen = torch.Generator().manual_seed(900 + sorted(CASES).index(name))
    Cout = CASES[name]['Cout']
    x = torch.randn(CASES[name]['B'], Cout, I['Ho'], I['Wo'], generator=gen).to(I['ydt']).float()
    stats = torch.stack([torch.randn(Cout, generator=gen) * 0.1, torch.rand(Cout, generator=gen) + 0.5]).view(1, 2, Cout).contiguous()
    return dict(x=x, stats=stats)


@functools.lru_cache(maxsize=None)
def conv_inputs(name, acc=None):
    """Operand values of a case (storage-exact; fp16-exact in the fp16 mode whatever the storage) and its float64 reference with the per-element bound.
    acc: the case with another accumulate mode."""
    c = CASES[name] if acc is None else dict(CASES[name], acc=acc)
    gen = torch.Generator().manual_seed(sorted(CASES).index(name) + 100)
    r = lambda *s: torch.randn(*s, generator=gen)
    h16 = c['prec'] == 'fp16'
    q = (lambda t: t.half().float()) if h16 else (lambda t: t)
    B, H, W, Cin, Cout, k = c['B'], c['H'], c['W'], c['Cin'], c['Cout'], c['k']
    taps = k * k
    x = q(r(B, Cin, H, W))
    wshape = (B, Cout, taps, Cin) if c['per_sample'] else (Cout, taps, Cin)
    w = q(r(*wshape) / (taps * Cin) ** 0.5)
    if c['live'] is not None:
        x[:, c['live']:] = 0
        w[..., c['live']:] = 0
    Hl, Wl = H << c['shift'], W << c['shift']
    if c['out_hw'] is not None:
        Ho, Wo = c['out_hw']
    elif c['tr'] and c['s'] == 1:
        Ho, Wo = (CR.conv_out_size(v, k, 1, c['p'], c['d'], True) for v in (Hl, Wl))
    else:
        Ho, Wo = (CR.conv_out_size(v, k, c['s'], c['p'], c['d'], c['tr']) for v in (Hl, Wl))
    Hs, Ws = (Ho // 2, Wo // 2) if c['pool2'] else (Ho, Wo)
    ydt = dt_of(c, 'y')
    bias = r(Cout) * 0.1 if c['bias'] else None
    scale = (torch.rand(B, Cout, generator=gen) + 0.5) if c['scale'] else None
    y_old = (r(B, Cout, Hs, Ws) * 0.5).to(ydt).float() if c['acc'] else None
    m = None
    if c['mul']:
        m = r(B, Cout, Hs, Ws).clamp(min=-0.9)      # an activation's output: ELU stays above -1
        m = m.half().float() if h16 else m
    x1 = w1 = None
    if c['x1']:
        x1, w1 = q(r(B, 1, Hl, Wl)), q(r(Cout, taps) / (taps * Cin) ** 0.5)
    R = CR.conv_ref(x, w, bias, c['s'], c['p'], c['d'], transposed=c['tr'], in_shift=c['shift'], alpha=c['alpha'], ch_scale=scale, act=c['act'],
                    accumulate=c['acc'], y_old=y_old, mul=m, mul_act=c['mul'] or 'none', pool2=c['pool2'], x1=x1, w1=w1, k=k, out_hw=(Ho, Wo))
    # ---- the bound: contraction + ONE 4u |ref| term (|ref| = the largest stage of the element: every fp32 step of the epilogue -- bias, scale, factor,
    # accumulate -- rounds a value no larger) + 4 x the activation's fp32 floor (tol_elem) + the storage terms
    n = taps * (Cin + (1 if c['x1'] else 0))
    cs = abs(c['alpha']) * (scale.double().abs().view(B, Cout, 1, 1) if scale is not None else 1.0)
    E = ((n + 16) if h16 else (2 * n + 16)) * U * cs * R.S
    floor = (PR.act_formula(R.z.float(), c['act']).double() - R.a).abs().max().item() if c['act'] != 'none' else 0.0
    st = lambda v: torch.clamp(2.0 ** -11 * v.abs(), min=2.0 ** -25)
    f16y = ydt == torch.float16
    big = torch.maximum(R.z.abs(), R.a.abs())
    Estage = None      # one more fp16 rounding of |a| in front of the act' factor: only the kernels of STAGED below
    if c['pool2']:
        pool = lambda v: v[:, :, 0::2, 0::2] + v[:, :, 0::2, 1::2] + v[:, :, 1::2, 0::2] + v[:, :, 1::2, 1::2]
        E, big = pool(E) + 2.0 ** -11 * R.P, pool(big)
        val = pool(R.a)
        if R.fac is not None:
            E, val = E * R.fac.abs(), val * R.fac
    else:
        val = R.r
        if R.fac is not None:
            E = E * R.fac.abs()
            if f16y:
                Estage = st(R.a) * R.fac.abs()
    big = torch.maximum(torch.maximum(big, val.abs()), R.y.abs())
    E = E + tol_elem(big, floor, False)
    if c['acc'] == 1 and f16y:
        E = E + st(val)
    if f16y:
        E = E + st(R.y)
    return dict(c=c, x=x, w=w, bias=bias, scale=scale, y_old=y_old, m=m, x1=x1, w1=w1, R=R, E=E, Estage=Estage, Ho=Hs, Wo=Ws, ydt=ydt, xdt=dt_of(c, 'x'))


def run_conv(name, view, which, off, ck, monkeypatch, stats=False, expect_path=True, acc=None, bstats=False):
    """One launch of case `name` with the view setting applied to the operands in `which` (x, y, m, 1 = x1); -> (ya, y Guarded, stats Guarded)."""
    I = conv_inputs(name, acc)
    c = I['c']
    dev = T.dev()
    tag = '%s %s/%s/%d' % (name, view, which, off)
    vw = lambda o: view if o in which else 'whole'
    of = lambda o: off if o in which else 0
    B, Cout = c['B'], c['Cout']
    Gx, xa = operand(I['x'], I['xdt'], vw('x'), of('x'), float('nan'))
    y0 = I['y_old'] if I['y_old'] is not None else torch.full((B, Cout, I['Ho'], I['Wo']), float('nan'))
    Gy, ya = operand(y0, I['ydt'], vw('y'), of('y'), SENT)
    guards = [Gx, Gy]
    mul = None
    if I['m'] is not None:
        mdt = I['ydt'] if (Cout == 1 or c['prec'] == 'fp32') else torch.float16      # (the 1-channel images and their act' operands stay fp32)
        Gm, ma = operand(I['m'], mdt, vw('m'), of('m'), float('nan'))
        guards.append(Gm)
        mul = (ma, c['mul'])
    w = I['w'].to(dev).contiguous()
    wh = w.half() if (c['wh'] and c['prec'] == 'fp16') else None
    bn = None
    if bstats:      # the raw input of the batch normalisation whose output gradient this launch writes, and its saved mean / rstd
        Bn = bn_inputs(name)
        Gbx, bxa = operand(Bn['x'], I['ydt'], vw('b'), of('b'), float('nan'))
        guards.append(Gbx)
        bstat = Bn['stats'].to(dev)
        bn = (bxa, bstat, 1, None)
    wt = ops.tile_weights(wh, Cout, c['k'] ** 2, c['Cin']) if c['wt'] else None
    kw = {}
    if c['per_sample']:
        kw['w_bstride'] = w[0].numel()
    if I['scale'] is not None:
        kw.update(ch_scale=I['scale'].to(dev), ch_scale_bstride=Cout)
    if c['x1']:
        G1, x1a = operand(I['x1'], torch.float16, vw('1'), of('1'), float('nan'))
        guards.append(G1)
        kw['x1'] = (x1a, I['w1'].to(dev).contiguous(), 0, c['k'] ** 2, 1)
    bias = None if I['bias'] is None else I['bias'].to(dev)      # (held until the launch is done: the descriptor keeps only its address)
    ws = T.ExactWs(monkeypatch)
    prev = lib.get().size('hv_set_s2t_mode', c['s2t']) if c['s2t'] is not None else None
    try:
        call = ops.ConvCall(xa, w, ya, c['k'], c['s'], c['p'], c['d'], bias=bias, act=c['act'],
                            transposed=c['tr'], in_shift=c['shift'], alpha=c['alpha'], accumulate=c['acc'], precision=c['prec'], w_h=wh, w_t=wt, mul=mul,
                            pool2=c['pool2'], bn=bn, **kw)
        Gs = None
        if bstats:      # (the partials go in by hand so that a view without the epilogue is asked for it too, and must refuse)
            Gs = T.Guarded((max(call.bstats_parts(), 1) * Cout * 2,), dtype=torch.float32)
            call.d.bstats = ops.ptr(Gs.t).value
        if stats:
            parts = call.stats_parts()
            Gs = T.Guarded((max(parts, 1) * Cout * 2,), dtype=torch.float32)
            if not parts:
                call.d.stats = ops.ptr(Gs.t).value
        if (c['nofb'] or stats or bstats) and not call.supported():
            ck.true(view not in ('whole', 'slice8') or (c['acc'] and (stats or bstats)) or (view == 'slice8' and c['p8'] is None),
                    tag + ': an aligned view was refused')
            before = bits(Gy.big)
            with pytest.raises(RuntimeError):
                call.launch(Gs.t if stats else None)
            torch.cuda.synchronize()
            ck.true(torch.equal(bits(Gy.big), before), tag + ': a refused launch wrote to y')
            return None, Gy, None
        call.launch(Gs.t if stats else None)
        p, kn = path(), kname()
        torch.cuda.synchronize()
    finally:
        if prev is not None:
            lib.get().size('hv_set_s2t_mode', prev)
        ws.close()
    tag += ' [path %d %s]' % (p, kn)
    want = c['path'] if view == 'whole' else c['p8'] if view == 'slice8' else None
    if want is not None and expect_path:
        ck.true(p in (want if isinstance(want, tuple) else (want,)), tag + ': kernel path, expected %s' % (want,))
        if c['kname']:
            ck.true(kn == c['kname'] if c['kname'].startswith('stem1') else kn.startswith(c['kname']), tag + ': kernel name, expected ' + c['kname'])
    for G in guards + ([Gs] if Gs is not None else []):
        ck.true(G.intact(), tag + ': guard overwritten')
    ck.true(others_untouched(ya), tag + ": a neighbour's channel of y was overwritten")
    got = view_of(ya).double()
    ck.true(bool(torch.isfinite(got).all()), tag + ': non-finite output (a foreign channel read, or an element not written)')
    E = I['E'] + I['Estage'] if (I['Estage'] is not None and kn.startswith(STAGED)) else I['E']
    ck.le('conv.' + c['fam'], (got - I['R'].y).abs(), E, tag)
    return ya, Gy, Gs


def variants(c, view, extra=()):
    """(which operands, base offset): one operand at a time, then all together."""
    ops_ = ['x', 'y'] + (['m'] if c['mul'] else []) + (['1'] if c['x1'] else []) + list(extra)
    if view == 'whole':
        return [('', 0)]
    if view == 'base':
        alls = [(''.join(ops_), o) for o in offsets(torch.float16 if c['prec'] == 'fp16' else torch.float32)]
        return [(o, 1) for o in ops_] + alls
    return [(o, 0) for o in ops_] + [(''.join(ops_), 0)]


@pytest.mark.parametrize('view', list(VIEWS))
@pytest.mark.parametrize('name', list(CASES))
def test_conv_on_views(name, view, monkeypatch):
    c, I = CASES[name], conv_inputs(name)
    ck = Check()
    for which, off in variants(c, view):
        # slice8 keeps the family only when every operand keeps its alignment AND its exact width where the family needs one: asserted with all operands sliced
        run_conv(name, view, which, off, ck, monkeypatch, expect_path=(view == 'whole' or len(which) > 1))
    ck.done()


# ---------------------------------------------------------------------------------------------------------------- statistics epilogue
@pytest.mark.parametrize('view', list(VIEWS))
@pytest.mark.parametrize('name', [n for n in CASES if CASES[n]['stats']])
def test_conv_statistics_epilogue_sums_the_stored_output(name, view, monkeypatch):
    """hv_conv_desc.stats of the conv_g4 forward launches: the per-image sums of consecutive parts against stats_ref of the read-back fp16 output, bound
    16u sum |y| + u |ref| (and likewise for the squares); a view without the epilogue must refuse the launch and write nothing (run_conv)."""
    c = CASES[name]
    ck = Check()
    B, Cout = c['B'], c['Cout']
    served = 0
    for which, off in variants(c, view):
        ya, Gy, Gs = run_conv(name, view, which, off, ck, monkeypatch, stats=True, expect_path=(view == 'whole' or len(which) > 1))
        if ya is None:
            continue
        served += 1
        y = view_of(ya)
        parts = Gs.t.cpu().double().view(-1, Cout, 2)
        ck.true(parts.shape[0] % B == 0, 'parts are not whole images')
        per = parts.view(B, -1, Cout, 2).sum(dim=1)
        s, q = CR.stats_ref(y)
        ya_ = y.double().abs().sum(dim=(2, 3))
        ck.le('conv.stats.sum', (per[..., 0] - s).abs(), 16 * U * ya_ + U * s.abs(), name)
        ck.le('conv.stats.sumsq', (per[..., 1] - q).abs(), 16 * U * q + U * q.abs(), name)
    ck.true(served or view not in ('whole', 'slice8'), 'the statistics epilogue never ran on an aligned view')
    ck.done()


BSTATS = ['g4_dgrad_s2_mul0', 'g4_dgrad_s1_mul', 'logits_dgrad']


@pytest.mark.parametrize('view', list(VIEWS))
@pytest.mark.parametrize('name', BSTATS)
def test_conv_batch_norm_backward_sums_epilogue(name, view, monkeypatch):
    """hv_conv_desc.bstats (conv_g4 data gradients, logits_dgrad_kernel): sum g and sum g * xhat over the batch (one normalisation group; the parts summed in
    fp64) against fp64 sums of the read-back stored g with xhat = (bn_x - mean) * rstd from the stored operands.  bn_x is a guarded view with NaN neighbours.
    Bounds (the reductions of tests/test_norm_act_gpu.py): 16u sum |g| + u |ref| and 16u sum |g| (|xhat| + |mean| rstd) + u |ref|.  A view without the
    epilogue must refuse the launch and write nothing."""
    c = CASES[name]
    ck = Check()
    Cout = c['Cout']
    Bn = bn_inputs(name)
    mean, rstd = (Bn['stats'][0, i].double().view(1, Cout, 1, 1) for i in (0, 1))
    xhat = (Bn['x'].double() - mean) * rstd
    served = 0
    for which, off in variants(c, view, extra='b'):
        ya, Gy, Gp = run_conv(name, view, which, off, ck, monkeypatch, bstats=True, expect_path=(view == 'whole' or len(which) > 1))
        if ya is None:
            continue
        served += 1
        g = view_of(ya).double()
        got = Gp.t.cpu().double().view(-1, Cout, 2).sum(dim=0)
        ck.true(bool(torch.isfinite(got).all()), name + ': sums not finite (a neighbour of bn_x read, or a part not written)')
        r0, r1 = g.sum(dim=(0, 2, 3)), (g * xhat).sum(dim=(0, 2, 3))
        a0, a1 = g.abs().sum(dim=(0, 2, 3)), (g.abs() * (xhat.abs() + mean.abs() * rstd)).sum(dim=(0, 2, 3))
        ck.le('conv.bstats.sum_g', (got[:, 0] - r0).abs(), 16 * U * a0 + U * r0.abs(), name)
        ck.le('conv.bstats.sum_gxhat', (got[:, 1] - r1).abs(), 16 * U * a1 + U * r1.abs(), name)
    ck.true(served or view not in ('whole', 'slice8'), 'the backward-sums epilogue never ran on an aligned view')
    ck.done()


def test_conv_statistics_epilogue_refuses_an_accumulating_launch(monkeypatch):
    ck = Check()
    ya, Gy, _ = run_conv('g4_fwd_s2', 'whole', '', 0, ck, monkeypatch, stats=True, acc=1)
    assert ya is None, 'accumulate = 1 with stats was launched'
    ck.done()


def test_conv_logits_layer_with_input_normalised_at_staging(monkeypatch):
    """hv_conv_desc.xn_*: the convolution against conv_ref over the normalised map the kernel stored (whose bits tests/test_conv_gpu.py pins against the
    separate normalisation pass); an unaligned raw input is refused and writes nothing."""
    ck = Check()
    dev = T.dev()
    B, H, W, C = 3, 7, 9, 128
    gen = torch.Generator().manual_seed(77)
    z = (torch.randn(B, C, H, W, generator=gen) * 1.7 + 0.3).half()
    w = (torch.randn(1, 16, C, generator=gen) / (16 * C) ** 0.5).half().float()
    b = torch.randn(1, generator=gen) * 0.1
    gam, bet = (torch.rand(C, generator=gen) + 0.5).to(dev), (torch.randn(C, generator=gen) * 0.2).to(dev)
    stats = torch.zeros(2 * C, device=dev)      # the statistics come from an aligned copy: this test is about the convolution's own staging
    ops.norm_act_forward(T.to_act(z.float(), dtype=torch.float16), None, 'batch', True, stats, act='lrelu', gamma=gam, beta=bet,
                         running_mean=torch.zeros(C, device=dev), running_var=torch.ones(C, device=dev), nbt=torch.zeros(1, dtype=torch.long, device=dev))
    torch.cuda.synchronize()
    for view, off in [(v, 0) for v in ('whole', 'slice8', 'slice4', 'odd')] + [('base', o) for o in (4, 2, 1)]:
        Gz, za = operand(z, torch.float16, view, off, float('nan'))
        Gn, na = operand(torch.full((B, C, H, W), float('nan')), torch.float16, view, off, SENT)
        Gy, ya = operand(torch.full((B, 1, H - 1, W - 1), float('nan')), torch.float32, view, min(off, 2), SENT)
        view = '%s/%d' % (view, off)
        ws = T.ExactWs(monkeypatch)
        try:
            wd = w.to(dev).contiguous()
            bd, wdh = b.to(dev), wd.half()      # (held until the launch is done)
            call = ops.ConvCall(za, wd, ya, 4, 1, 1, 1, bias=bd, precision='fp16', w_h=wdh, xn=(stats, gam, bet, 1, 'lrelu', na))
            if not call.supported():
                ck.true(view.startswith(('odd', 'base')), view + ': the fused form refused an aligned view')
                before = bits(Gy.big), bits(Gn.big)
                with pytest.raises(RuntimeError):
                    call.launch()
                torch.cuda.synchronize()
                ck.true(torch.equal(bits(Gy.big), before[0]) and torch.equal(bits(Gn.big), before[1]), view + ': a refused launch wrote')
                continue
            call.launch()
            ck.true(path() == 5, view + ': path %d' % path())
            torch.cuda.synchronize()
        finally:
            ws.close()
        ck.true(Gz.intact() and Gn.intact() and Gy.intact(), view + ': guard overwritten')
        ck.true(others_untouched(ya) and others_untouched(na), view + ": a neighbour's channel of y or of the normalised map was overwritten")
        xn = view_of(na)
        ck.true(bool(torch.isfinite(xn).all()), view + ': normalised map not finite')
        R = CR.conv_ref(xn, w, b, 1, 1, 1, k=4)
        E = (16 * C + 16) * U * R.S + 4 * U * R.y.abs()
        got = view_of(ya).double()
        ck.true(bool(torch.isfinite(got).all()), view + ': logits not finite')
        ck.le('conv.head_xn', (got - R.y).abs(), E, view)
    ck.done()


# ---------------------------------------------------------------------------------------------------------------- weight gradients
WCASES = {}


def wcase(name, fam, B, H, W, Cin, Cout, k, path, prec='fp16', s=1, p=1, d=1, dbias=True, kname=None):
    WCASES[name] = dict(fam=fam, B=B, H=H, W=W, Cin=Cin, Cout=Cout, k=k, path=path, prec=prec, s=s, p=p, d=d, dbias=dbias, kname=kname)


wcase('wgather_fp32', 'wgather', 2, 12, 10, 8, 12, 3, 10, prec='fp32')
wcase('wgather_fp16_s2', 'wgather', 2, 12, 10, 8, 12, 3, 10, s=2)
wcase('whalo_8to12', 'whalo', 2, 12, 10, 8, 12, 3, 11, kname='wgrad_halo_kernel')
wcase('wtr_16to32', 'wtr', 2, 16, 16, 16, 32, 3, 12, kname='wgrad_tr_kernel')
wcase('wtr_64to128_k4s2', 'wtr', 2, 16, 16, 64, 128, 4, 12, s=2, kname='wgrad_tr_kernel')
wcase('wtr_32to64_d2', 'wtr', 2, 20, 12, 32, 64, 3, 12, p=2, d=2, kname='wgrad_tr_kernel')
wcase('wtr_24to40', 'wtr', 4, 16, 16, 24, 40, 3, 12, kname='wgrad_tr_kernel')
wcase('wthin_x_4to16_k5', 'wthin', 2, 16, 16, 4, 16, 5, 12, p=2, kname='wgrad_thinx_kernel')
wcase('wthin_g_64to4_k4', 'wthin', 2, 9, 9, 64, 4, 4, 12, dbias=False, kname='wgrad_thing_kernel')
wcase('wthin_g_12to4_k3', 'wthin', 2, 12, 10, 12, 4, 3, 12, dbias=False, kname='wgrad_thing_kernel')
PRE = 0.5      # what dw / dbias hold before the accumulating call


@functools.lru_cache(maxsize=None)
def wgrad_inputs(name):
    c = WCASES[name]
    gen = torch.Generator().manual_seed(sorted(WCASES).index(name) + 500)
    dt = torch.float16 if c['prec'] == 'fp16' else torch.float32
    x = torch.randn(c['B'], c['Cin'], c['H'], c['W'], generator=gen).to(dt)
    Ho, Wo = (CR.conv_out_size(v, c['k'], c['s'], c['p'], c['d']) for v in (c['H'], c['W']))
    g = torch.randn(c['B'], c['Cout'], Ho, Wo, generator=gen).to(dt)
    dw, db, Sw, Sb = CR.wgrad_ref(x, g, c['k'], c['s'], c['p'], c['d'])
    n = c['B'] * Ho * Wo
    f = (n + 16) if c['prec'] == 'fp16' else (2 * n + 16)
    return dict(x=x, g=g, dt=dt, dw=dw, db=db, Ew=f * U * Sw + 4 * U * dw.abs(), Eb=f * U * Sb + 4 * U * db.abs())


def wgrad_refusable(view, which, off):
    """wgrad_validate refuses strides / offsets that are not multiples of 4 and bases that are not 16-byte aligned."""
    return which and (view == 'odd' or (view == 'base' and off))


def run_wgrad(name, view, which, off, ck, monkeypatch):
    c, I = WCASES[name], wgrad_inputs(name)
    tag = '%s %s/%s/%d' % (name, view, which, off)
    vw = lambda o: view if o in which else 'whole'
    of = lambda o: off if o in which else 0
    Gx, xa = operand(I['x'], I['dt'], vw('x'), of('x'), float('nan'))
    Gg, ga = operand(I['g'], I['dt'], vw('g'), of('g'), float('nan'))
    Gw = T.Guarded((c['Cout'], c['k'] ** 2, c['Cin']))
    Gb = T.Guarded((c['Cout'],)) if c['dbias'] else None
    kw = dict(precision=c['prec'], dbias=None if Gb is None else Gb.t)
    args = (c['k'], c['s'], c['p'], c['d'])
    ws = T.ExactWs(monkeypatch)
    try:
        if wgrad_refusable(view, which, off):      # wgrad_validate decides on these fields alone
            before = bits(Gw.big), (bits(Gb.big) if Gb is not None else None)
            with pytest.raises(RuntimeError):
                ops.conv2d_wgrad(xa, ga, Gw.t, *args, **kw)
            torch.cuda.synchronize()
            ck.true(torch.equal(bits(Gw.big), before[0]), tag + ': a refused weight gradient wrote to dw')
            ck.true(Gb is None or torch.equal(bits(Gb.big), before[1]), tag + ': a refused weight gradient wrote to dbias')
            return
        ops.conv2d_wgrad(xa, ga, Gw.t, *args, **kw)      # assign over the NaN the buffers hold
        p, kn = path(), kname()
        torch.cuda.synchronize()
        tag += ' [path %d %s]' % (p, kn)
        if view in ('whole', 'slice8'):
            ck.true(p == c['path'], tag + ': kernel path, expected %d' % c['path'])
            if c['kname']:
                ck.true(kn.startswith(c['kname']), tag + ': kernel name, expected ' + c['kname'])
        got = Gw.cpu().double()
        ck.true(bool(torch.isfinite(got).all()), tag + ': dw not finite')
        ck.le('conv.' + c['fam'] + '.dw', (got - I['dw']).abs(), I['Ew'], tag)
        if Gb is not None:
            gb = Gb.cpu().double()
            ck.true(bool(torch.isfinite(gb).all()), tag + ': dbias not finite')
            ck.le('conv.' + c['fam'] + '.dbias', (gb - I['db']).abs(), I['Eb'], tag)
        # the accumulate form over a known finite content
        Gw.t.fill_(PRE)
        if Gb is not None:
            Gb.t.fill_(PRE)
        ops.conv2d_wgrad(xa, ga, Gw.t, *args, accumulate=True, dbias_accumulate=True, **kw)
        torch.cuda.synchronize()
        ck.le('conv.' + c['fam'] + '.dw', (Gw.cpu().double() - (PRE + I['dw'])).abs(), I['Ew'] + 4 * U * (PRE + I['dw']).abs(), tag + ' accumulate')
        if Gb is not None:
            ck.le('conv.' + c['fam'] + '.dbias', (Gb.cpu().double() - (PRE + I['db'])).abs(), I['Eb'] + 4 * U * (PRE + I['db']).abs(), tag + ' accumulate')
    finally:
        ws.close()
    for G in (Gx, Gg, Gw) + ((Gb,) if Gb is not None else ()):
        ck.true(G.intact(), tag + ': guard overwritten')


@pytest.mark.parametrize('view', list(VIEWS))
@pytest.mark.parametrize('name', list(WCASES))
def test_wgrad_on_views(name, view, monkeypatch):
    ck = Check()
    dt = wgrad_inputs(name)['dt']
    if view == 'whole':
        vs = [('', 0)]
    elif view == 'base':
        vs = [('x', 1), ('g', 1)] + [('xg', o) for o in offsets(dt)]
    else:
        vs = [('x', 0), ('g', 0), ('xg', 0)]
    for which, off in vs:
        run_wgrad(name, view, which, off, ck, monkeypatch)
    ck.done()


@pytest.mark.parametrize('name', ['wgather_fp16_s2', 'wtr_16to32'])
def test_wgrad_fold_chain_pending_and_carry_on_exact_workspaces(name, monkeypatch):
    """Two weight gradients of one FoldChain: the first leaves its slabs pending, the second carries their fold, flush() runs the last one."""
    c, I = WCASES[name], wgrad_inputs(name)
    ck = Check()
    tw = T.ExactWs(monkeypatch, required=True)
    chain = ops.FoldChain(torch.cuda.current_stream().cuda_stream)
    args = (c['k'], c['s'], c['p'], c['d'])
    outs = []
    for view in ('slice8', 'whole'):
        Gx, xa = operand(I['x'], I['dt'], view, 0, float('nan'))
        Gg, ga = operand(I['g'], I['dt'], view, 0, float('nan'))
        Gw, Gb = T.Guarded((c['Cout'], c['k'] ** 2, c['Cin'])), T.Guarded((c['Cout'],))
        ops.conv2d_wgrad(xa, ga, Gw.t, *args, precision=c['prec'], dbias=Gb.t, chain=chain)
        ck.true(path() == c['path'], '%s %s: path %d' % (name, view, path()))
        outs.append((Gx, Gg, Gw, Gb))
    chain.flush()
    tw.close()
    for Gx, Gg, Gw, Gb in outs:
        ck.true(all(G.intact() for G in (Gx, Gg, Gw, Gb)), name + ': guard overwritten')
        got, gb = Gw.cpu().double(), Gb.cpu().double()
        ck.true(bool(torch.isfinite(got).all()) and bool(torch.isfinite(gb).all()), name + ': not finite')
        ck.le('conv.' + c['fam'] + '.chain', (got - I['dw']).abs(), I['Ew'], name)
        ck.le('conv.' + c['fam'] + '.chain', (gb - I['db']).abs(), I['Eb'], name)
    ck.true(same_bits(outs[0][2].cpu(), outs[1][2].cpu()), name + ': the carried fold and the flushed one differ')
    ck.done()
