"""Test-side helpers (CPU<->device plumbing with torch; never used by the product path)."""
import torch

import hvgan
from hvgan import ops


def dev():
    return torch.device('cuda:0')


def st(prec):
    """Storage dtype of activation tensors for a compute precision (fp16 mode: fp16 storage)."""
    return torch.float16 if prec in ('fp16', 'f16') else torch.float32


def to_act(x_nchw, CP=None, dtype=torch.float32):
    """CPU (B,C,H,W) -> device NHWC Act with channel stride CP (zero padded), stored as `dtype`."""
    B, C, H, W = x_nchw.shape
    CP = C if CP is None else CP
    t = torch.zeros(B, H, W, CP)
    t[..., :C] = x_nchw.permute(0, 2, 3, 1)
    return ops.Act(t.to(dev()).to(dtype).contiguous(), C, 0)


def to_act_view(x_nchw, ld=None, coff=0, fill=0.0):
    """CPU (B,C,H,W) of the storage dtype -> device Act over channels [coff, coff + C) of an ld-wide buffer whose other channels hold `fill`."""
    B, C, H, W = x_nchw.shape
    ld = C if ld is None else ld
    t = torch.full((B, H, W, ld), fill, dtype=x_nchw.dtype)
    t[..., coff:coff + C] = x_nchw.permute(0, 2, 3, 1)
    return ops.Act(t.to(dev()).contiguous(), C, coff)


def from_act(a):
    """device Act -> CPU (B,C,H,W)."""
    return a.t[..., a.coff:a.coff + a.C].permute(0, 3, 1, 2).contiguous().float().cpu()


def ohwi(w, CinP=None, CoutF=None):
    """CPU [Cout,Cin,kh,kw] -> device [CoutF][kh*kw][CinP] (zero padded)."""
    Co, Ci, kh, kw = w.shape
    CinP = Ci if CinP is None else CinP
    CoutF = Co if CoutF is None else CoutF
    o = torch.zeros(CoutF, kh * kw, CinP)
    o[:Co, :, :Ci] = w.permute(0, 2, 3, 1).reshape(Co, kh * kw, Ci)
    return o.to(dev()).contiguous()


def ohwi_T(w, CoutP=None, CinB=None):
    """CPU [Cout,Cin,kh,kw] -> device data-gradient layout [CinB][kh*kw][CoutP]."""
    Co, Ci, kh, kw = w.shape
    CoutP = Co if CoutP is None else CoutP
    CinB = Ci if CinB is None else CinB
    o = torch.zeros(CinB, kh * kw, CoutP)
    o[:Ci, :, :Co] = w.permute(1, 2, 3, 0).reshape(Ci, kh * kw, Co)
    return o.to(dev()).contiguous()


def maxerr(a, b):
    return (a.double() - b.double()).abs().max().item()


def _flow_close(got, ref, name):
    """offset_flow: uint8 colour codes / 255.  The arg-max of near-tied scores may pick a different patch on the device than the CPU
    reference did (a different colour for that pixel's 8x8 block), and floor(255*col) can fall either side of an integer: allow a
    handful of pixels; everything else must agree to half a colour step."""
    d = (got.detach().cpu() - ref).abs()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    frac = (d > 0.5 / 255).float().mean().item()
    assert frac <= 5e-3, (name, frac, d.max().item())


class Guarded:
    """A device tensor `t` of `shape` inside a sentinel-filled buffer (NaN; 0xA5 bytes for integers) with `guard` elements on both sides; `offset` shifts
    its base by that many elements off the buffer's 256-byte alignment.  `data` (a CPU tensor of the shape) initialises it.  intact(): the guards still hold
    the sentinel, bit for bit."""

    def __init__(self, shape, dtype=torch.float32, guard=64, offset=0, data=None):
        shape = tuple(int(s) for s in ((shape,) if isinstance(shape, int) else shape))
        n = 1
        for s in shape:
            n *= s
        self.sentinel = float('nan') if dtype.is_floating_point else int.from_bytes(b'\xa5' * torch.empty(0, dtype=dtype).element_size(), 'little', signed=True)
        self.big = torch.full((2 * guard + offset + n,), self.sentinel, dtype=dtype, device=dev())
        self.lo, self.n = guard + offset, n
        self.t = self.big[self.lo:self.lo + n].view(shape)
        if data is not None:
            self.t.copy_(data.to(dtype).reshape(shape))

    def intact(self):
        raw = self.big.view(torch.uint8)
        e = self.big.element_size()
        want = torch.full((1,), self.sentinel, dtype=self.big.dtype, device=self.big.device).view(torch.uint8)
        lo, hi = raw[:self.lo * e].view(-1, e), raw[(self.lo + self.n) * e:].view(-1, e)
        return bool((lo == want).all()) and bool((hi == want).all())

    def cpu(self):
        return self.t.cpu()


class ExactWs:
    """ops._ws replaced (through pytest's monkeypatch) by one that hands out EXACTLY the queried bytes, each time a fresh 16-byte aligned view into its own
    0xA5-filled buffer -- so the two alternating buffers of an ops.FoldChain are covered as well.  close() puts ops._ws back and checks that nothing was
    written outside any of the queried ranges; required: at least one workspace must have been asked for."""

    def __init__(self, monkeypatch, required=False):
        self.all, self.mp, self.required = [], monkeypatch, required
        monkeypatch.setattr(ops, '_ws', self.ws)

    def ws(self, nbytes, device, slot=0):
        import ctypes
        n = int(nbytes)
        big = torch.full((512 + n,), 0xA5, dtype=torch.uint8, device=device)
        self.all.append((big, n))
        assert big[256:].data_ptr() % 16 == 0
        return big[256:256 + n], ctypes.c_size_t(n)

    def close(self):
        self.mp.undo()
        torch.cuda.synchronize()
        assert self.all or not self.required, 'no workspace was asked for'
        for big, n in self.all:
            assert bool((big[:256] == 0xA5).all()) and bool((big[256 + n:] == 0xA5).all()), 'wrote outside the queried workspace'
