"""Plain float64 references of hv_conv2d, hv_conv2d_wgrad and the convolution's statistics epilogue: the formula of include/hvgan.h (hv_conv_desc)
restated with torch on the CPU, no device code.  tests/test_conv_ref_cpu.py pins them against F.conv2d / F.conv_transpose2d / F.interpolate, torch
autograd and a nested-loop convolution.

Tensors are (B, C, H, W); filters are in the kernels' own layout [Cout][KH*KW][Cin] (a leading batch dimension = per-sample filters).  Every operand is
taken AS STORED: whatever dtype it arrives in (fp16 storage, the fp16 filter copy) is promoted exactly to float64, so the caller rounds first.

    y[n,ho,wo,co] (op)= act( alpha * ch_scale[co] * sum_{r,s,ci} x[n,hi,wi,ci] * w[co,(r,s),ci] + bias[co] )
    transposed = 0: hi = ho*stride - pad + r*dil;   transposed = 1: hi = (ho + pad - r*dil) / stride where divisible
"""
import torch

import pointwise_ref as PR


def conv_out_size(n, k, stride, pad, dil, transposed=False):
    if transposed:
        return (n - 1) * stride - 2 * pad + dil * (k - 1) + 1
    return (n + 2 * pad - dil * (k - 1) - 1) // stride + 1


def _tap_index(no, n, r, stride, pad, dil, transposed):
    """input index and validity of every output index along one axis for tap offset r."""
    o = torch.arange(no)
    if transposed:
        v = o + pad - r * dil
        ok = (v % stride == 0)
        i = torch.div(v, stride, rounding_mode='floor')
    else:
        i = o * stride - pad + r * dil
        ok = torch.ones(no, dtype=torch.bool)
    ok = ok & (i >= 0) & (i < n)
    return i.clamp(0, n - 1), ok


def _gather(x, t, KW, Ho, Wo, stride, pad, dil, transposed):
    """x (B, C, H, W) as seen by tap t at every output pixel -> (B, C, Ho, Wo), zero outside the image."""
    r, s = divmod(t, KW)
    hi, hok = _tap_index(Ho, x.shape[2], r, stride, pad, dil, transposed)
    wi, wok = _tap_index(Wo, x.shape[3], s, stride, pad, dil, transposed)
    g = x[:, :, hi][:, :, :, wi]
    return g * (hok.view(-1, 1) & wok.view(1, -1)).to(x.dtype)


def up2(x):
    """nearest x2 up-sampling: logical index -> physical index >> 1 (in_shift = 1)."""
    return x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)


class ConvRef:
    """y: the result; S: the same contraction over |x| and |w| (no alpha / ch_scale; the x1 term included); z: the argument of act; a: act(z);
    fac: the act' factor (None without mul); r: a * fac (what accumulate = 1 adds, or the full-resolution value that pool2 pools); P: pool2's sum of
    the four |r|.  Iterates as (y, S)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __iter__(self):
        return iter((self.y, self.S))


def conv_ref(x, w, bias=None, stride=1, pad=0, dil=1, transposed=False, in_shift=0, alpha=1.0, ch_scale=None, act='none', accumulate=0, y_old=None,
             mul=None, mul_act='none', pool2=False, x1=None, w1=None, k=None, out_hw=None):
    """x (B, Cin, H, W) stored input (physical size: in_shift = 1 reads it through the nearest x2 up-sampling); w [Cout][taps][Cin] or [B][Cout][taps][Cin];
    ch_scale [Cout] or [B][Cout]; mul: the stored output m of activation mul_act at the output's pixels (the pooled ones under pool2); x1 (B, 1, H, W) with
    w1 [Cout][taps]; k = KH or (KH, KW) (default: square, from the tap count); out_hw: the output size of a transposed convolution when it is not the
    minimal one."""
    f64 = torch.float64
    x = x.to(f64)
    w = w.to(f64)
    if in_shift:
        x = up2(x)
    taps = w.shape[-2]
    if k is None:
        k = int(round(taps ** 0.5))
    KH, KW = (k, k) if isinstance(k, int) else k
    assert KH * KW == taps and w.shape[-1] == x.shape[1]
    B, Cin, H, W = x.shape
    Cout = w.shape[-3]
    Ho, Wo = out_hw if out_hw is not None else (conv_out_size(H, KH, stride, pad, dil, transposed), conv_out_size(W, KW, stride, pad, dil, transposed))
    eq = 'bchw,boc->bohw' if w.dim() == 4 else 'bchw,oc->bohw'
    acc = torch.zeros(B, Cout, Ho, Wo, dtype=f64)
    S = torch.zeros_like(acc)
    for t in range(taps):
        xs = _gather(x, t, KW, Ho, Wo, stride, pad, dil, transposed)
        wt = w[..., t, :]
        acc += torch.einsum(eq, xs, wt)
        S += torch.einsum(eq, xs.abs(), wt.abs())
    if x1 is not None:
        x1 = x1.to(f64)
        w1 = w1.to(f64)
        assert x1.shape == (B, 1, H, W) and w1.shape == (Cout, taps) and not transposed
        for t in range(taps):
            xs = _gather(x1, t, KW, Ho, Wo, stride, pad, dil, False)
            acc += xs * w1[:, t].view(1, -1, 1, 1)
            S += xs.abs() * w1[:, t].abs().view(1, -1, 1, 1)
    z = alpha * acc
    if ch_scale is not None:
        cs = ch_scale.to(f64)
        z = z * (cs.view(B, Cout, 1, 1) if cs.dim() == 2 else cs.view(1, Cout, 1, 1))
    if bias is not None:
        z = z + bias.to(f64).view(1, Cout, 1, 1)
    if accumulate == 2:
        z = z + y_old.to(f64)
    a = PR.act_formula(z, act)
    fac, P = None, None
    if pool2:
        r = a
        pooled = r[:, :, 0::2, 0::2] + r[:, :, 0::2, 1::2] + r[:, :, 1::2, 0::2] + r[:, :, 1::2, 1::2]
        ra = r.abs()
        P = ra[:, :, 0::2, 0::2] + ra[:, :, 0::2, 1::2] + ra[:, :, 1::2, 0::2] + ra[:, :, 1::2, 1::2]
        if mul is not None:
            fac = PR.act_grad_from_out_formula(mul.to(f64), mul_act)
            pooled = pooled * fac
        y = pooled
    else:
        r = a
        if mul is not None:      # decided on the stored m, like the kernel
            fac = PR.act_grad_from_out_formula(mul.to(f64), mul_act)
            r = a * fac
        y = r
    if accumulate == 1:
        y = y_old.to(f64) + y
    return ConvRef(y=y, S=S, z=z, a=a, fac=fac, r=r, P=P)


def wgrad_ref(x, g, k, stride=1, pad=0, dil=1, in_shift=0):
    """dw[co][(r,s)][ci] = sum_{n,ho,wo} g[n,co,ho,wo] * x[n,ci,ho*stride-pad+r*dil,...], dbias[co] = sum g -> dw, dbias, and the same sums over the
    absolute values (S_dw, S_dbias)."""
    f64 = torch.float64
    x, g = x.to(f64), g.to(f64)
    if in_shift:
        x = up2(x)
    KH, KW = (k, k) if isinstance(k, int) else k
    Cout, Cin, (Ho, Wo) = g.shape[1], x.shape[1], g.shape[2:]
    dw = torch.zeros(Cout, KH * KW, Cin, dtype=f64)
    S = torch.zeros_like(dw)
    for t in range(KH * KW):
        xs = _gather(x, t, KW, Ho, Wo, stride, pad, dil, False)
        dw[:, t, :] = torch.einsum('bohw,bchw->oc', g, xs)
        S[:, t, :] = torch.einsum('bohw,bchw->oc', g.abs(), xs.abs())
    return dw, g.sum(dim=(0, 2, 3)), S, g.abs().sum(dim=(0, 2, 3))


def stats_ref(y_stored):
    """per-image, per-channel sum and sum of squares of the stored output (B, C, H, W) -> two (B, C) tensors."""
    y = y_stored.to(torch.float64)
    return y.sum(dim=(2, 3)), (y * y).sum(dim=(2, 3))
