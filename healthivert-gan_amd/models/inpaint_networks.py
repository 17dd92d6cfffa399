"""Two-stage inpainting generator on hand-written gfx950 kernels.

API mirror of the reference `models/inpaint_networks.py` (same class names, constructor signatures,
state-dict keys and 7-tuple return: reference :16-32, :36-117, :120-232, :235-410, :413-503), but
the forward/backward are explicit kernel sequences from `engine.py` over NHWC buffers; the torch
modules created here are parameter containers only (their own forward is never run).
"""
import contextlib
import os

import torch
import torch.nn as nn
from torch.nn.utils import spectral_norm as _sn_register

from ._backend import engine as E
from ._backend import lib as _lib
from ._backend import ops
ptr, stream = _lib.ptr, _lib.stream
Act = ops.Act

_ACTS = ('relu', 'elu', 'lrelu', 'prelu', 'selu', 'tanh', 'sigmoid', 'none')


class Conv2dBlock(nn.Module):
    """Parameter container with the reference's keys: conv.bias, conv.weight_orig, conv.weight_u, conv.weight_v
    (reference :420-503).  Only the configuration the generator uses is executable on the HIP path:
    zero padding, spectral norm, no norm layer, activation in {elu, relu, sigmoid, none}."""

    def __init__(self, input_dim, output_dim, kernel_size, stride, padding=0, conv_padding=0, dilation=1, weight_norm='sn',
                 norm='none', activation='relu', pad_type='zero', transpose=False):
        super().__init__()
        assert pad_type in ('reflect', 'replicate', 'zero', 'none'), "Unsupported padding type: {}".format(pad_type)
        assert norm in ('bn', 'in', 'none'), "Unsupported normalization: {}".format(norm)
        assert weight_norm in ('sn', 'wn', 'none'), "Unsupported normalization: {}".format(weight_norm)
        assert activation in _ACTS, "Unsupported activation: {}".format(activation)
        if pad_type != 'zero' or padding != 0 or norm != 'none' or weight_norm != 'sn' or transpose or \
                activation not in ('elu', 'relu', 'sigmoid', 'none'):
            raise NotImplementedError("Conv2dBlock: only the generator's configuration (zero pad, spectral norm, no norm layer, "
                                      "elu/relu/sigmoid/none) has a HIP kernel path")
        self.use_bias = True
        self.activation_name = activation
        self.cin, self.cout, self.k, self.stride, self.conv_padding, self.dilation = input_dim, output_dim, kernel_size, stride, conv_padding, dilation
        # identical parameter creation (and RNG consumption) to nn.Conv2d + spectral_norm; the hook is removed so the
        # power iteration runs in hv_weight_prep instead.
        conv = _sn_register(nn.Conv2d(input_dim, output_dim, kernel_size, stride, padding=conv_padding, dilation=dilation, bias=True))
        for hid, hook in list(conv._forward_pre_hooks.items()):
            if type(hook).__name__ == 'SpectralNorm':
                del conv._forward_pre_hooks[hid]
        if 'weight' in conv.__dict__:
            del conv.__dict__['weight']
        self.conv = conv

    def params(self, name, cin_fwd=None):
        c = self.conv
        return E.ConvParams(name, c.weight_orig, c.bias, self.cin, self.cout, self.k, cin_fwd=cin_fwd, cin_wg=cin_fwd,
                            u=c.weight_u, v=c.weight_v)

    def forward(self, x):
        raise RuntimeError("Conv2dBlock is executed through Generator (explicit HIP kernel sequence), not stand-alone")


def gen_conv(input_dim, output_dim, kernel_size=3, stride=1, padding=0, rate=1, activation='elu'):
    return Conv2dBlock(input_dim, output_dim, kernel_size, stride, conv_padding=padding, dilation=rate, activation=activation)


class CoarseGenerator(nn.Module):
    def __init__(self, input_dim, cnum, use_cuda):
        super().__init__()
        self.use_cuda = use_cuda
        self.cnum = cnum
        self.conv1 = gen_conv(input_dim + 2, cnum, 5, 1, 2)
        self.conv2_downsample = gen_conv(cnum, cnum * 2, 3, 2, 1)
        self.conv3 = gen_conv(cnum * 2, cnum * 2, 3, 1, 1)
        self.conv4_downsample = gen_conv(cnum * 2, cnum * 4, 3, 2, 1)
        self.conv5 = gen_conv(cnum * 4, cnum * 4, 3, 1, 1)
        self.conv6 = gen_conv(cnum * 4, cnum * 4, 3, 1, 1)
        self.conv7_atrous = gen_conv(cnum * 4, cnum * 4, 3, 1, 2, rate=2)
        self.conv8_atrous = gen_conv(cnum * 4, cnum * 4, 3, 1, 4, rate=4)
        self.conv9_atrous = gen_conv(cnum * 4, cnum * 4, 3, 1, 8, rate=8)
        self.conv10_atrous = gen_conv(cnum * 4, cnum * 4, 3, 1, 16, rate=16)
        self.conv11 = gen_conv(cnum * 4, cnum * 4, 3, 1, 1)
        self.conv12 = gen_conv(cnum * 4, cnum * 4, 3, 1, 1)
        self.conv20 = gen_conv(cnum * 4 + 1, cnum * 4, 3, 1, 1)
        self.conv13 = gen_conv(cnum * 4, cnum * 2, 3, 1, 1)
        self.conv14 = gen_conv(cnum * 2, cnum * 2, 3, 1, 1)
        self.conv19 = gen_conv(cnum * 2 + 1, cnum * 2, 3, 1, 1)
        self.conv15 = gen_conv(cnum * 2, cnum, 3, 1, 1)
        self.conv16 = gen_conv(cnum, cnum // 2, 3, 1, 1)
        self.conv17 = gen_conv(cnum // 2, input_dim, 3, 1, 1, activation='none')
        self.conv18 = gen_conv(cnum // 2, input_dim, 3, 1, 1, activation='sigmoid')
        self.global_pool = nn.AdaptiveAvgPool2d(1)
        self.fc_height = nn.Linear(cnum * 4, 1)

    def forward(self, x, mask, CAM, slice_ratio):
        raise RuntimeError("CoarseGenerator runs as part of Generator's fused kernel sequence")


class FineGenerator(nn.Module):
    def __init__(self, input_dim, cnum, use_cuda=True):
        super().__init__()
        self.use_cuda = use_cuda
        self.cnum = cnum
        self.conv1 = gen_conv(input_dim + 3, cnum, 5, 1, 2)
        self.conv2_downsample = gen_conv(cnum, cnum, 3, 2, 1)
        self.conv3 = gen_conv(cnum, cnum * 2, 3, 1, 1)
        self.conv4_downsample = gen_conv(cnum * 2, cnum * 2, 3, 2, 1)
        self.conv5 = gen_conv(cnum * 2, cnum * 4, 3, 1, 1)
        self.conv6 = gen_conv(cnum * 4, cnum * 4, 3, 1, 1)
        self.conv7_atrous = gen_conv(cnum * 4, cnum * 4, 3, 1, 2, rate=2)
        self.conv8_atrous = gen_conv(cnum * 4, cnum * 4, 3, 1, 4, rate=4)
        self.conv9_atrous = gen_conv(cnum * 4, cnum * 4, 3, 1, 8, rate=8)
        self.conv10_atrous = gen_conv(cnum * 4, cnum * 4, 3, 1, 16, rate=16)
        self.pmconv1 = gen_conv(input_dim + 3, cnum, 5, 1, 2)
        self.pmconv2_downsample = gen_conv(cnum, cnum, 3, 2, 1)
        self.pmconv3 = gen_conv(cnum, cnum * 2, 3, 1, 1)
        self.pmconv4_downsample = gen_conv(cnum * 2, cnum * 4, 3, 2, 1)
        self.pmconv5 = gen_conv(cnum * 4, cnum * 4, 3, 1, 1)
        self.pmconv6 = gen_conv(cnum * 4, cnum * 4, 3, 1, 1, activation='relu')
        self.contextul_attention = ContextualAttention(self.use_cuda, ksize=3, stride=1, rate=2, fuse_k=3, softmax_scale=10, fuse=True)
        self.pmconv9 = gen_conv(cnum * 4, cnum * 4, 3, 1, 1)
        self.pmconv10 = gen_conv(cnum * 4, cnum * 4, 3, 1, 1)
        self.allconv11 = gen_conv(cnum * 8, cnum * 4, 3, 1, 1)
        self.allconv19 = gen_conv(cnum * 4, cnum * 4, 3, 1, 1)
        self.allconv12 = gen_conv(cnum * 4, cnum * 4, 3, 1, 1)
        self.allconv13 = gen_conv(cnum * 4, cnum * 2, 3, 1, 1)
        self.allconv14 = gen_conv(cnum * 2, cnum * 2, 3, 1, 1)
        self.allconv15 = gen_conv(cnum * 2, cnum, 3, 1, 1)
        self.allconv16 = gen_conv(cnum, cnum // 2, 3, 1, 1)
        self.allconv17 = gen_conv(cnum // 2 + 1, 1, 3, 1, 1, activation='none')
        self.allconv18 = gen_conv(cnum // 2 + 1, 1, 3, 1, 1, activation='sigmoid')
        self.global_pool = nn.AdaptiveAvgPool2d(1)
        self.fc_height = nn.Linear(cnum * 4, 1)

    def forward(self, xin, x_stage1, mask, coarse_seg, slice_ratio):
        raise RuntimeError("FineGenerator runs as part of Generator's fused kernel sequence")


class ContextualAttention(nn.Module):
    """Contextual attention (Yu et al.) with the reference's signature (reference :235-410).  Stand-alone calls take
    NCHW tensors with f is b; inside Generator the NHWC plan is used directly."""

    def __init__(self, use_cuda, ksize=3, stride=1, rate=1, fuse_k=3, softmax_scale=10, fuse=False):
        super().__init__()
        self.ksize, self.stride, self.rate, self.fuse_k, self.softmax_scale, self.fuse, self.use_cuda = \
            ksize, stride, rate, fuse_k, softmax_scale, fuse, use_cuda
        self._plans = {}

    def check(self):
        if not (self.ksize == 3 and self.stride == 1 and self.rate == 2 and self.fuse_k == 3):
            raise NotImplementedError("ContextualAttention HIP path: ksize=3, stride=1, rate=2, fuse_k=3 only")

    def plan(self, B, H, W, C, device, img_hw):
        self.check()
        key = (B, H, W, C, str(device), img_hw)
        if key not in self._plans:
            self._plans[key] = E.AttentionPlan(B, H, W, C, device, img_hw, float(self.softmax_scale), bool(self.fuse))
        return self._plans[key]

    def forward(self, f, b, mask=None):
        if f is not b and not torch.equal(f, b):
            raise NotImplementedError("ContextualAttention HIP path expects foreground and background to be the same tensor")
        _lib.require_gpu(f)
        B, C, H, W = f.shape
        if mask is None:
            mask = torch.zeros(B, 1, 4 * H, 4 * W, device=f.device)
        fa = ops.from_nchw(f.detach())
        out = Act.empty(B, H, W, C, f.device)
        pl = self.plan(B, H, W, C, f.device, (mask.shape[2], mask.shape[3]))
        pl.forward(fa, mask.contiguous().float(), out, ops.default_precision(), want_argmax=True)
        y = out.nchw()
        flow = offsets_to_flow(pl.argmax, B, pl.h, pl.w, self.rate)
        if f.requires_grad and torch.is_grad_enabled():
            return _AttentionFn.apply(f, y, pl, fa), flow
        return y, flow


class _AttentionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, f, y, plan, fa):
        ctx.plan, ctx.shape = plan, f.shape
        return y.clone()

    @staticmethod
    def backward(ctx, gy):
        B, C, H, W = ctx.shape
        g = ops.from_nchw(gy.contiguous())
        df = Act.empty(B, H, W, C, gy.device)
        ctx.plan.backward(g, df, False, ops.default_precision())
        return df.nchw(), None, None, None


def offsets_to_flow(argmax, B, h, w, rate):
    """offset_flow slot of the 7-tuple (reference :368,:389-410): the arg-max offsets coloured with the Middlebury wheel and nearest-
    upsampled by rate*4.  The reference does this with NumPy on the host (inpaint_tools.py:73-100), one device sync per forward; here
    it is one small kernel on the arg-max indices the soft-max already produced (hv_ca_flow)."""
    flow = torch.empty(B, 3, h * rate * 4, w * rate * 4, dtype=torch.float32, device=argmax.device)
    _lib.get().call('hv_ca_flow', ptr(argmax), B, h, w, rate * 4, ptr(flow), stream())
    return flow


# ================================================================================================ generator plan
def _buffers(c):
    """The NHWC buffers of both generators at width c, stated once: (name -> channels) per resolution (side >> 0, 1, 2), and the channel ranges of them that
    layers write or read under a name of their own (name -> (buffer, first channel, channels))."""
    full = dict(c_in=3, c1=c, cat19=2 * c + 1, c19=2 * c, c15=c, c16=c // 2, f_in=4, f1=c, p1=c, a15=c, cat17=c // 2 + 1)
    half = dict(c2=2 * c, c3=2 * c, cat20=4 * c + 1, c20=4 * c, c13=2 * c, c14=2 * c, f2=c, f3=2 * c, p2=c, p3=2 * c, a13=2 * c, a14=2 * c)
    quarter = dict(c4=4 * c, f4=2 * c, cat11=8 * c, **{n: 4 * c for n in 'c5 c6 c7 c8 c9 c10 c11 c12 f5 f6 f7 f8 f9 p4 p5 p6 ca p9 a11 a12 a19'.split()})
    views = dict(f10=('cat11', 0, 4 * c), p10=('cat11', 4 * c, 4 * c), a16=('cat17', 0, c // 2))      # cat11 = [conv10_atrous | pmconv10], cat17 = [allconv16 | x_stage1]
    return (full, half, quarter), views


_IMAGES = ('x_stage1', 'coarse_seg', 'x_stage2', 'fine_seg')      # the heads' outputs: (B,1,H,W) fp32 in every mode (reference API)


def _layers(c):
    """The two generators as data: generator -> chain -> rows (reference layer, input buffer, output buffer, stride, pad, dilation, activation[, ConvNode flags:
    need_dx, dx_c, shift]) in forward order.  A chain is a run of layers the executors walk as one; _GenPlan builds one ConvNode per row."""
    e = (1, 1, 1, 'elu')
    dil = lambda r: (1, r, r, 'elu')
    down = (2, 1, 1, 'elu')
    return {
        'coarse_generator': dict(
            enc=[('conv1', 'c_in', 'c1', 1, 2, 1, 'elu', dict(need_dx=False)), ('conv2_downsample', 'c1', 'c2', *down), ('conv3', 'c2', 'c3', *e),
                 ('conv4_downsample', 'c3', 'c4', *down), ('conv5', 'c4', 'c5', *e), ('conv6', 'c5', 'c6', *e), ('conv7_atrous', 'c6', 'c7', *dil(2)),
                 ('conv8_atrous', 'c7', 'c8', *dil(4)), ('conv9_atrous', 'c8', 'c9', *dil(8)), ('conv10_atrous', 'c9', 'c10', *dil(16))],      # c10 feeds the height head
            mid=[('conv11', 'c10', 'c11', *e), ('conv12', 'c11', 'c12', *e)],
            up20=[('conv20', 'cat20', 'c20', *e, dict(dx_c=4 * c))],      # [up(c12) | CAM at half size]; the CAM channel is an input: no gradient
            dec20=[('conv13', 'c20', 'c13', *e), ('conv14', 'c13', 'c14', *e)],
            up19=[('conv19', 'cat19', 'c19', *e, dict(dx_c=2 * c))],      # [up(c14) | CAM]
            dec19=[('conv15', 'c19', 'c15', *e), ('conv16', 'c15', 'c16', *e)],
            heads=[('conv17', 'c16', 'x_stage1', 1, 1, 1, 'clamp'), ('conv18', 'c16', 'coarse_seg', 1, 1, 1, 'sigmoid')]),
        'fine_generator': dict(
            dilated=[('conv1', 'f_in', 'f1', 1, 2, 1, 'elu'), ('conv2_downsample', 'f1', 'f2', *down), ('conv3', 'f2', 'f3', *e), ('conv4_downsample', 'f3', 'f4', *down),
                     ('conv5', 'f4', 'f5', *e), ('conv6', 'f5', 'f6', *e), ('conv7_atrous', 'f6', 'f7', *dil(2)), ('conv8_atrous', 'f7', 'f8', *dil(4)),
                     ('conv9_atrous', 'f8', 'f9', *dil(8)), ('conv10_atrous', 'f9', 'f10', *dil(16))],
            pm_in=[('pmconv1', 'f_in', 'p1', 1, 2, 1, 'elu')],      # (on its own: the backward runs it after the branches join)
            pm=[('pmconv2_downsample', 'p1', 'p2', *down), ('pmconv3', 'p2', 'p3', *e), ('pmconv4_downsample', 'p3', 'p4', *down), ('pmconv5', 'p4', 'p5', *e),
                ('pmconv6', 'p5', 'p6', 1, 1, 1, 'relu')],
            pm_out=[('pmconv9', 'ca', 'p9', *e), ('pmconv10', 'p9', 'p10', *e)],      # behind the attention block (p6 -> ca)
            merge=[('allconv11', 'cat11', 'a11', *e)],      # a11 feeds the height head
            trunk=[('allconv12', 'a11', 'a12', *e), ('allconv19', 'a12', 'a19', *e), ('allconv13', 'a19', 'a13', *e, dict(shift=1)), ('allconv14', 'a13', 'a14', *e),
                   ('allconv15', 'a14', 'a15', *e, dict(shift=1)), ('allconv16', 'a15', 'a16', *e)],
            heads=[('allconv17', 'cat17', 'x_stage2', 1, 1, 1, 'clamp'), ('allconv18', 'cat17', 'fine_seg', 1, 1, 1, 'sigmoid')])}


# the coarse layers that read [nearest x2 up-sampling of a low-resolution map | CAM channel]: layer -> (its chain, the layer that produces the low map, hv_copy_channels
# mode that resamples the CAM image to the layer's resolution)
_UP_CONCAT = {'coarse_generator.conv19': ('up19', 'coarse_generator.conv14', 0), 'coarse_generator.conv20': ('up20', 'coarse_generator.conv12', 2)}


class _UpConcat:
    """One layer of _UP_CONCAT.  Where the dispatch serves it (ConvNode.split_forward) the forward reads `low` with the fused up-sampling and takes the CAM channel in
    its epilogue (hv_conv_desc.x1), so the up-sampled part of the concat buffer `cat` is only built for the layer's weight gradient; where the pooled data gradient
    serves the shape (fp16 mode) the gradient of `low` comes 2x2-pooled and times act' straight from the convolution's epilogue."""
    __slots__ = ('node', 'low', 'cat', 'k', 'cam_mode', 'pooled')

    def __init__(self, node, producer, cam_mode):
        self.node, self.low, self.cat, self.k, self.cam_mode = node, producer.y, node.x, node.dx_c, cam_mode
        assert self.low.C == self.k and self.cat.C == self.k + 1
        self.pooled = None      # the dispatch's answer in the last backward
        node.split = (self.low, self.cat.slice(self.k, 1))
        node.pool_to = (self.low, producer.act)

    def forward(self, cam, prec):
        if not self.node.split_forward(prec):
            ops.copy_channels(self.low, self.cat.slice(0, self.k), mode=1)
        ops.copy_channels(cam, self.cat.slice(self.k, 1), mode=self.cam_mode)
        self.node.forward(prec)

    def materialise(self, prec):
        """The up-sampled part of the concat buffer for the weight gradient, where the forward did not build it."""
        if self.node.split_forward(prec):
            ops.copy_channels(self.low, self.cat.slice(0, self.k), mode=1)

    def backward(self, above, book, prec, premultiplied_first):
        """Backward of the pure chain `above` (backward order) that ends in this layer, then of the layer.  -> True where the gradient of `low` left pooled and
        times act' (its producer then starts premultiplied); otherwise full-resolution gradient + adjoint-of-up-sampling pass."""
        self.pooled = self.node.pooled(book, prec, 'pool_to')
        E.conv_backward_chain([*above, self.node], book, prec, premultiplied_first=premultiplied_first)
        if not self.pooled:
            g = book.twin(self.low)
            ops.copy_channels(book.twin(self.cat).slice(0, self.k), g, mode=3, accumulate=book.mark(g))
        return self.pooled


class _Head:
    """One 1-channel head: its output's gradient lives in a channel-padded carrier ([B,H,W,4], channel 0 live), registered as the output's twin once."""
    __slots__ = ('node', 'carrier')

    def __init__(self, node, book):
        y, x = node.y, node.x
        self.node = node
        self.carrier = Act(torch.zeros(y.B, y.H, y.W, ops.cpad(1), dtype=x.t.dtype, device=x.t.device), 1, 0)
        book.twins[id(y.t)] = self.carrier.t

    def fused_seed(self, seed):
        """seed -> act' -> carrier -> bias gradient in one pass (instead of: copy, in-place act' pass, column sums)?"""
        return bool(self.carrier.f16 and seed.dtype == torch.float32 and seed.is_contiguous() and self.node.p.bias is not None and self.node.use_bias)

    def backward(self, seed, book, prec, mul_x=None):
        """seed (B,1,H,W) -> padded carrier -> activation/bias gradient -> wgrad + dgrad."""
        node, carrier = self.node, self.carrier
        if self.fused_seed(seed):
            ops.head_seed_backward(seed, node.y, Act(carrier.t, 4, 0), node.act, dbias=node.p.bias.grad)
            E.conv_backward(node, book, prec, premultiplied=True, dbias_done=True, mul_x=mul_x)
            return
        ops.copy_channels(Act(seed.view(carrier.B, carrier.H, carrier.W, 1)), carrier, mode=0)
        E.conv_backward(node, book, prec, mul_x=mul_x)


class _GenPlan:
    """Buffers, nodes and layer owners of Generator for one (B, H, W), built from _buffers / _layers: `a` name -> Act, `node` reference layer name -> ConvNode,
    `chain` (generator, chain) -> its nodes in forward order, `up` / `head` reference layer name -> owner."""
    __slots__ = ('B', 'H', 'W', 'dev', 'book', 'a', 'node', 'chain', 'up', 'head', 'attn', 'x_stage1', 'coarse_seg', 'x_stage2', 'fine_seg', 'c_pool', 'pred1',
                 'f_pool', 'pred2', 'd_xs1_total', 'd_cs_total', 'mask_img', 'generation')

    def __init__(self, gen, B, H, W, device):
        c = gen.cnum
        self.B, self.H, self.W, self.dev = B, H, W, device
        dt = ops.storage_dtype(gen.precision)        # fp16 buffers in the fp16 mode; the (B,1,H,W) image outputs stay fp32
        self.book = E.GradBook()
        levels, views = _buffers(c)
        a = self.a = {n: Act(torch.zeros(B, H >> lv, W >> lv, ops.cpad(C), dtype=dt, device=device), C, 0) for lv, bufs in enumerate(levels) for n, C in bufs.items()}
        a.update({n: a[src].slice(coff, C) for n, (src, coff, C) in views.items()})
        for n in _IMAGES:
            setattr(self, n, torch.zeros(B, 1, H, W, dtype=torch.float32, device=device))
            a[n] = Act(getattr(self, n).view(B, H, W, 1))
        self.node, self.chain = {}, {}
        for gname, chains in _layers(c).items():
            for chain, rows in chains.items():
                for layer, src, dst, s, pad, d, act, *flags in rows:
                    self.node['%s.%s' % (gname, layer)] = E.ConvNode(gen._pset_convs['%s.%s' % (gname, layer)], a[src], a[dst], s, pad, d, act, **(flags[0] if flags else {}))
                self.chain[gname, chain] = tuple(self.node['%s.%s' % (gname, row[0])] for row in rows)
        self.up = {n: _UpConcat(self.node[n], self.node[producer], cam_mode) for n, (_, producer, cam_mode) in _UP_CONCAT.items()}
        self.head = {n: _Head(node, self.book) for n, node in self.node.items() if node.p.cout == 1}
        self.c_pool, self.f_pool = torch.zeros(B, 4 * c, device=device), torch.zeros(B, 4 * c, device=device)
        self.pred1, self.pred2 = torch.zeros(B, 1, device=device), torch.zeros(B, 1, device=device)
        self.attn = gen.fine_generator.contextul_attention.plan(B, H // 4, W // 4, 4 * c, device, (H, W))
        # x_stage1 / coarse_seg also feed the refinement generator: their seeds plus what its backward adds
        self.d_xs1_total, self.d_cs_total = torch.zeros_like(self.x_stage1), torch.zeros_like(self.coarse_seg)
        self.mask_img = None      # the last forward's mask
        self.generation = 0       # forwards through the nn.Module API (_GeneratorFn refuses a stale backward)

    def forward(self, prec, gname, *chains):
        for chain in chains:
            for n in self.chain[gname, chain]:
                n.forward(prec)


class Generator(nn.Module):
    def __init__(self, config, use_cuda):
        super().__init__()
        self.input_dim = config['input_dim']
        self.cnum = config['ngf']
        self.use_cuda = use_cuda
        if self.input_dim != 1:
            raise NotImplementedError("Generator HIP path: input_dim == 1 (single-channel CT slices)")
        self.coarse_generator = CoarseGenerator(self.input_dim, self.cnum, self.use_cuda)
        self.fine_generator = FineGenerator(self.input_dim, self.cnum, self.use_cuda)
        self.precision = None          # None -> HV_PRECISION env (fp32 parity mode by default)
        self._plans = {}
        self._pset = None
        self._eval_graphs = {}
        self.use_graph = os.environ.get('HV_GRAPH', '1') != '0'
        self._pset_convs = None
        self.time_fine = None          # bench.py: a list that receives a pair of HIP events around each refinement-generator forward
        self._fine_graph_keep = None

    # ---------------------------------------------------------------- parameters
    def paramset(self):
        if self._pset is None:
            convs = {}
            for gname in ('coarse_generator', 'fine_generator'):
                g = getattr(self, gname)
                for n, m in g.named_children():
                    if isinstance(m, Conv2dBlock):
                        convs['%s.%s' % (gname, n)] = m.params('%s.%s' % (gname, n), cin_fwd=ops.cpad(m.cin))
            # the _UP_CONCAT layers read [up-sampled feature map | CAM]: their first dx_c input channels also as a filter table of their own, so that the
            # forward can read the small map with the fused up-sampling and take the CAM channel in its epilogue (ConvNode.split, hv_conv_desc.x1)
            chains = _layers(self.cnum)['coarse_generator']
            for n, (chain, _, _) in _UP_CONCAT.items():
                k2 = chains[chain][0][-1]['dx_c']
                if k2 % 32 == 0 and convs[n].cin == k2 + 1:
                    convs[n].split_k = k2
            self._pset_convs = convs
            cg, fg = self.coarse_generator, self.fine_generator
            self._pset = E.ParamSet(convs.values(), [cg.fc_height.weight, cg.fc_height.bias, fg.fc_height.weight, fg.fc_height.bias])
        return self._pset

    def _plan(self, B, H, W, device):
        key = (B, H, W, str(device), ops.precision_id(self.precision))
        if key not in self._plans:
            if H % 8 or W % 8 or H != W:
                raise NotImplementedError("Generator HIP path expects square inputs with a side divisible by 8")
            self.paramset()
            self._plans[key] = _GenPlan(self, B, H, W, device)
        return self._plans[key]

    # ---------------------------------------------------------------- explicit forward / backward
    def run_forward(self, x, mask, CAM, slice_ratio, training=None, per_sample_mask=False):
        """x, mask, CAM: (B,1,H,W) fp32 device tensors; slice_ratio: (B,) fp64.  Returns the plan (all activations
        stay in its buffers); outputs are plan.coarse_seg/fine_seg/x_stage1/x_stage2 (B,1,H,W) and plan.pred1/pred2 (B,1).
        per_sample_mask: the batch stands for B independent batch-1 calls (attention masks per sample, see AttentionPlan.forward)."""
        _lib.require_gpu(x, mask, CAM)
        training = self.training if training is None else training
        prec = ops.precision_id(self.precision)
        B, _, H, W = x.shape
        dev = x.device
        P = self._plan(B, H, W, dev)
        self.paramset().prep(dev, power_iter=training)
        x = x.contiguous().float(); mask = mask.contiguous().float(); CAM = CAM.contiguous().float()
        ratio = slice_ratio.to(device=dev, dtype=torch.float64).contiguous()
        P.mask_img = mask
        cg, cgn, a = self.coarse_generator, 'coarse_generator', P.a
        cam = Act(CAM.view(B, H, W, 1))
        # ---- coarse
        ops.gen_input(x, None, mask, ratio, a['c_in'], 0)
        P.forward(prec, cgn, 'enc')
        ops.gap_fc_sigmoid(a['c10'], cg.fc_height.weight, cg.fc_height.bias, P.c_pool, P.pred1)
        P.forward(prec, cgn, 'mid')
        # (split layers read c12 / c14 themselves: the up-sampled part of the concat buffer is then built by the backward, on its side stream)
        P.up['coarse_generator.conv20'].forward(cam, prec)
        P.forward(prec, cgn, 'dec20')
        P.up['coarse_generator.conv19'].forward(cam, prec)
        P.forward(prec, cgn, 'dec19', 'heads')
        # ---- fine
        tf = self.time_fine
        if tf is not None and not torch.cuda.is_current_stream_capturing():     # bench.py: HIP events around the refinement generator
            tf.append((torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)))
            tf[-1][0].record()
        else:
            tf = None
        self._fine_forward(P, x, mask, ratio, prec, per_sample_mask)
        if tf is not None:
            tf[-1][1].record()
        return P

    def _fine_forward(self, P, x, mask, ratio, prec, per_sample_mask=False):
        """FineGenerator.forward (reference models/inpaint_networks.py:169-232) over the plan's buffers: reads x, mask, P.coarse_seg, P.x_stage1."""
        fg, fgn, a = self.fine_generator, 'fine_generator', P.a
        ops.gen_input(x, P.coarse_seg, mask, ratio, a['f_in'], 1)
        # the dilated-conv branch and the attention branch only share their input: two streams (two branches of the step graph)
        side = E.branch_stream()
        main = torch.cuda.current_stream()
        if side is not None:
            side.wait_stream(main)
        with (torch.cuda.stream(side) if side is not None else contextlib.nullcontext()):
            P.forward(prec, fgn, 'pm_in', 'pm')
            P.attn.forward(a['p6'], mask, a['ca'], prec, want_argmax=True, per_sample_mask=per_sample_mask)
            P.forward(prec, fgn, 'pm_out')
        P.forward(prec, fgn, 'dilated')
        if side is not None:
            main.wait_stream(side)
        P.forward(prec, fgn, 'merge')
        ops.gap_fc_sigmoid(a['a11'], fg.fc_height.weight, fg.fc_height.bias, P.f_pool, P.pred2)
        P.forward(prec, fgn, 'trunk')
        ops.copy_channels(a['x_stage1'], a['cat17'].slice(a['a16'].C, 1), mode=0)
        P.forward(prec, fgn, 'heads')

    def fine_forward_graph(self, P, x, mask, slice_ratio):
        """bench.py: the refinement generator's training forward alone as ONE captured hipGraph over the buffers of plan P (which a full
        run_forward has filled: coarse outputs, prepared weight tables) -- both branches on their two streams, as inside the step graphs."""
        prec = ops.precision_id(self.precision)
        ratio = slice_ratio.to(device=x.device, dtype=torch.float64).contiguous()
        x = x.contiguous().float(); mask = mask.contiguous().float()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=E.named_stream('capture', x.device), capture_error_mode='thread_local'):
            self._fine_forward(P, x, mask, ratio, prec)
        self._fine_graph_keep = (x, mask, ratio)
        return g

    def run_backward(self, P, d_coarse_seg, d_fine_seg, d_x_stage1, d_x_stage2, d_pred1, d_pred2):
        """Gradients of a scalar loss wrt the six differentiable outputs -> .grad of every parameter.
        All seeds are dense fp32 device tensors shaped like the outputs (None = zero)."""
        prec = ops.precision_id(self.precision)
        B, H, W = P.B, P.H, P.W
        book, a, N, head = P.book, P.a, P.node, P.head
        book.reset()
        cg, fg = self.coarse_generator, self.fine_generator
        coarse, fine = (lambda chain: reversed(P.chain['coarse_generator', chain])), (lambda chain: reversed(P.chain['fine_generator', chain]))
        up19, up20 = P.up['coarse_generator.conv19'], P.up['coarse_generator.conv20']
        zero = lambda t, ref: torch.zeros_like(ref) if t is None else t.contiguous().float()
        d_fine_seg, d_x_stage2 = zero(d_fine_seg, P.fine_seg), zero(d_x_stage2, P.x_stage2)
        d_coarse_seg, d_x_stage1 = zero(d_coarse_seg, P.coarse_seg), zero(d_x_stage1, P.x_stage1)
        d_pred1, d_pred2 = zero(d_pred1, P.pred1), zero(d_pred2, P.pred2)
        # the refinement generator's weight gradients as ONE block on a side stream beside the coarse generator's whole backward (round 4):
        # they only feed the optimiser, and the coarse backward -- a chain of small launches that leave most of a CU's registers and LDS free -- does not
        # depend on them.  One fork and one join (per-layer forks cost more than they returned and are gone).  Measured against it, three
        # same-box pairs each: a first block launched before the two branches (three streams busy there) +0.13 ms; the coarse generator's own weight
        # gradients in two more blocks +0.14 ms -- both removed.
        wg = book.wgrad_block
        wg.open(self.paramset(), d_x_stage2.device)
        # the concat inputs of the split layers (forward: never built) for their weight gradients: up-sampled now, beside the head kernels -- or, where the
        # layer's weight gradient goes to the side stream, on that stream right in front of it: 35 + 20 us of copies (67 + 33 MB written) off the head of
        # the backward's critical path
        wg.before_next_block(lambda: up19.materialise(prec))
        wg.before_next_block(lambda: up20.materialise(prec))
        # ---- fine: heads
        head['fine_generator.allconv17'].backward(d_x_stage2, book, prec)
        head['fine_generator.allconv18'].backward(d_fine_seg, book, prec)
        # x_stage1 also feeds the fine heads (the channel of cat17 behind allconv16's)
        ops.add_channels(Act(d_x_stage1.view(B, H, W, 1)), book.twin(a['cat17']).slice(a['a16'].C, 1), Act(P.d_xs1_total.view(B, H, W, 1)))
        # pure links (single producer, single consumer): the consumer's data gradient applies the producer's act'
        # (allconv15 and allconv13 read their input up-sampled: they link too where their data gradient can leave pooled, otherwise the chain breaks there)
        allconv11, allconv12 = N['fine_generator.allconv11'], N['fine_generator.allconv12']
        E.conv_backward_chain(list(fine('trunk')), book, prec, stop_before=allconv11)
        # a11 (allconv11's output, input of allconv12) also feeds the height head: both writers of its gradient apply elu'(a11)
        pre11 = E.chain_link(allconv12, allconv11, book, prec)
        ops.gap_fc_sigmoid_backward(d_pred2, P.pred2, P.f_pool, fg.fc_height.weight, book.twin(a['a11']),
                                    fg.fc_height.weight.grad, fg.fc_height.bias.grad, mul=(a['a11'], allconv11.act) if pre11 else None)
        # cat11 = [conv10_atrous | pmconv10], both ELU: allconv11's data gradient applies elu' for both producers
        E.conv_backward(allconv11, book, prec, premultiplied=pre11, mul_x='elu')
        # the two branches run concurrently; both end in the gradient of f_in: the attention branch stops before its first conv,
        # which is run after the join (assign / accumulate order of the shared buffer stays that of the single-stream schedule)
        side = E.branch_stream()
        main = torch.cuda.current_stream()
        pmconv1, pmconv2 = N['fine_generator.pmconv1'], N['fine_generator.pmconv2_downsample']
        if side is not None:
            side.wait_stream(main)
        with (torch.cuda.stream(side) if side is not None else contextlib.nullcontext()):
            E.conv_backward_chain(list(fine('pm_out')), book, prec, premultiplied_first=True)
            gp6 = book.twin(a['p6'])
            P.attn.backward(book.twin(a['ca']), gp6, book.mark(gp6), prec)
            E.conv_backward_chain([*fine('pm'), *(fine('pm_in') if side is None else ())], book, prec, stop_before=None if side is None else pmconv1)
            if side is not None:
                self.paramset().fold_chain().flush()      # (weight gradients issued in line on the branch stream: their last slab fold, before the join)
        E.conv_backward_chain(list(fine('dilated')), book, prec, premultiplied_first=True)
        if side is not None:
            main.wait_stream(side)
            E.conv_backward(pmconv1, book, prec, premultiplied=E.chain_link(pmconv2, pmconv1, book, prec))
        # coarse_seg enters the fine generator as channel 1 of its input
        ops.add_channels(Act(d_coarse_seg.view(B, H, W, 1)), book.twin(a['f_in']).slice(1, 1), Act(P.d_cs_total.view(B, H, W, 1)))
        wg.launch(keep_collecting=True)      # (the first coarse layers' weight gradients queue up behind this block: see below)
        # ---- coarse
        # both heads read c16 (output of conv16, ELU): each applies elu'(c16) to its share of the gradient
        head['coarse_generator.conv17'].backward(P.d_xs1_total, book, prec, mul_x='elu')
        head['coarse_generator.conv18'].backward(P.d_cs_total, book, prec, mul_x='elu')
        # Round 5: the coarse generator's first backward layers -- its heads and the 256 x 256 / 128 x 128 decoder, the most expensive weight
        # gradients of the chain -- hand their weight gradients to the side stream too (ONE more fork: it queues them behind the refinement generator's
        # block), so that the main stream walks these layers with data gradients only; the rest of the coarse backward keeps its weight gradients in line
        # (everything on the side stream made the block outlast the chain: +0.14 ms, round 4)
        p19 = up19.backward(coarse('dec19'), book, prec, True)
        p20 = up20.backward(coarse('dec20'), book, prec, p19)
        wg.launch()      # (behind the heads and the 256 x 256 / 128 x 128 decoder)
        conv10, conv11 = N['coarse_generator.conv10_atrous'], N['coarse_generator.conv11']
        E.conv_backward_chain(list(coarse('mid')), book, prec, premultiplied_first=p20, stop_before=conv10)
        pre10 = E.chain_link(conv11, conv10, book, prec)      # c10 feeds conv11 and the height head: both apply elu'(c10)
        ops.gap_fc_sigmoid_backward(d_pred1, P.pred1, P.c_pool, cg.fc_height.weight, book.twin(a['c10']),
                                    cg.fc_height.weight.grad, cg.fc_height.bias.grad, mul=(a['c10'], conv10.act) if pre10 else None)
        E.conv_backward_chain(list(coarse('enc')), book, prec, premultiplied_first=pre10)
        wg.join()     # side-stream weight gradients
        self.paramset().finish_backward(accumulate=False)
        self.paramset().attach_grads()

    # ---------------------------------------------------------------- nn.Module API
    def forward(self, x, mask, CAM, slice_ratio):
        """Same signature and 7-tuple as the reference (inpaint_networks.py:28-32):
        (coarse_seg, fine_seg, x_stage1, x_stage2, offset_flow, pred1_h, pred2_h)."""
        if not torch.is_tensor(slice_ratio):
            slice_ratio = torch.as_tensor(slice_ratio, dtype=torch.float64).reshape(-1)
        if self.use_graph and not self.training and not torch.is_grad_enabled() and ops.timer() is None and x.is_cuda:
            P = self._eval_replay(x, mask, CAM, slice_ratio)
        else:
            P = self.run_forward(x, mask, CAM, slice_ratio)
        outs = (P.coarse_seg, P.fine_seg, P.x_stage1, P.x_stage2, P.pred1, P.pred2)
        flow = offsets_to_flow(P.attn.argmax, P.B, P.attn.h, P.attn.w, 2)
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            anchor = next(p for p in self.parameters() if p.requires_grad)
            o = _GeneratorFn.apply(anchor, self, P, *outs)
        else:
            o = tuple(t.clone() for t in outs)
        return o[0], o[1], o[2], o[3], flow, o[4], o[5]

    def _eval_replay(self, x, mask, CAM, slice_ratio):
        """Eval-mode forward as a captured hipGraph per input shape: the ~250 launches of a bs=1 inference call (launch-bound when
        issued eagerly: the reference's eval loop runs ~130 of them per volume) become one graph launch.  Inputs are copied into
        the graph's fixed buffers; the weights are re-prepared from the current parameters inside the graph on every replay."""
        key = (tuple(x.shape), x.device.index, next(self.parameters()).data_ptr())
        ent = self._eval_graphs.get(key)
        if ent is None:
            dev = x.device
            static = [x.detach().to(dev, torch.float32).contiguous().clone(), mask.detach().to(dev, torch.float32).contiguous().clone(),
                      CAM.detach().to(dev, torch.float32).contiguous().clone(), slice_ratio.detach().to(dev, torch.float64).contiguous().clone()]
            self.run_forward(*static)                       # eager warm-up: plan buffers, weight tables, kernel attributes
            torch.cuda.synchronize(dev)
            g = torch.cuda.CUDAGraph()
            try:
                with torch.cuda.graph(g, stream=E.named_stream('capture', dev), capture_error_mode='thread_local'):
                    P = self.run_forward(*static)
            except RuntimeError:
                self.use_graph = False
                torch.cuda.synchronize(dev)
                return self.run_forward(x, mask, CAM, slice_ratio)
            if len(self._eval_graphs) >= 8:                 # a handful of shapes at most (bs=1 loop, batched stages)
                self._eval_graphs.clear()
            ent = self._eval_graphs[key] = (g, static, P)
        g, static, P = ent
        for dst, src in zip(static, (x, mask, CAM, slice_ratio)):
            dst.copy_(src, non_blocking=True)
        g.replay()
        return P


class _GeneratorFn(torch.autograd.Function):
    """Autograd bridge: lets user code call loss.backward() on the generator outputs; parameter gradients are
    written into .grad by the explicit backward (the anchor parameter only carries the graph edge)."""

    @staticmethod
    def forward(ctx, anchor, gen, plan, *outs):
        ctx.gen, ctx.plan = gen, plan
        plan.generation = ctx.generation = plan.generation + 1
        return tuple(t.clone() for t in outs)

    @staticmethod
    def backward(ctx, g_cs, g_fs, g_x1, g_x2, g_p1, g_p2):
        # gradients are ASSIGNED into .grad (the reference always zero_grad()s before backward)
        if ctx.plan.generation != ctx.generation:
            raise RuntimeError("Generator: a later forward pass of the same shape overwrote this pass's activations before its backward ran "
                               "(one activation plan per input shape); run backward before the next forward")
        S = ops.grad_scale(ctx.gen.precision)       # fp16 storage mode: scaled seeds, parameter gradients unscaled afterwards (grad_factor 1)
        sc = (lambda t: None if t is None else t * S) if S != 1.0 else (lambda t: t)
        ctx.gen.run_backward(ctx.plan, sc(g_cs), sc(g_fs), sc(g_x1), sc(g_x2), sc(g_p1), sc(g_p2))
        ops.scale_inplace(ctx.gen.paramset().flat_grad, 1.0 / S)
        return (None,) * 9
