"""PatchGAN discriminator, GAN loss, schedulers and initialisers on the HIP path.

API mirror of the parts of the reference `models/networks.py` that Pix2PixModel uses (define_D :163-206,
NLayerDiscriminator :555-602, GANLoss :212-278, get_scheduler :39-65, init_net/init_weights :68-117,
get_norm_layer :18-36).  The nn.Sequential built here is a parameter container with the reference's
state-dict keys (model.0.weight ... model.11.bias); forward/backward are explicit kernel sequences.
Generators/discriminators the hot path never instantiates (ResNet/U-Net G, pixel/seg D, WGAN-GP) are
out of scope and raise NotImplementedError.
"""
import functools

import torch
import torch.nn as nn
from torch.nn import init
from torch.optim import lr_scheduler

from ._backend import engine as E
from ._backend import lib as _lib
from ._backend import ops
Act, rup = ops.Act, ops.rup


class Identity(nn.Module):
    def forward(self, x):
        return x


def get_norm_layer(norm_type='instance'):
    if norm_type == 'batch':
        return functools.partial(nn.BatchNorm2d, affine=True, track_running_stats=True)
    if norm_type == 'instance':
        return functools.partial(nn.InstanceNorm2d, affine=False, track_running_stats=False)
    if norm_type == 'none':
        return lambda x: Identity()
    raise NotImplementedError('normalization layer [%s] is not found' % norm_type)


def get_scheduler(optimizer, opt):
    if opt.lr_policy == 'linear':
        def lambda_rule(epoch):
            return 1.0 - max(0, epoch + opt.epoch_count - opt.n_epochs) / float(opt.n_epochs_decay + 1)
        return lr_scheduler.LambdaLR(optimizer, lr_lambda=lambda_rule)
    if opt.lr_policy == 'step':
        return lr_scheduler.StepLR(optimizer, step_size=opt.lr_decay_iters, gamma=0.1)
    if opt.lr_policy == 'plateau':
        return lr_scheduler.ReduceLROnPlateau(optimizer, mode='min', factor=0.2, threshold=0.01, patience=5)
    if opt.lr_policy == 'cosine':
        return lr_scheduler.CosineAnnealingLR(optimizer, T_max=opt.n_epochs, eta_min=0)
    return NotImplementedError('learning rate policy [%s] is not implemented', opt.lr_policy)


def init_weights(net, init_type='normal', init_gain=0.02):
    def init_func(m):
        classname = m.__class__.__name__
        if hasattr(m, 'weight') and (classname.find('Conv') != -1 or classname.find('Linear') != -1):
            if init_type == 'normal':
                init.normal_(m.weight.data, 0.0, init_gain)
            elif init_type == 'xavier':
                init.xavier_normal_(m.weight.data, gain=init_gain)
            elif init_type == 'kaiming':
                init.kaiming_normal_(m.weight.data, a=0, mode='fan_in')
            elif init_type == 'orthogonal':
                init.orthogonal_(m.weight.data, gain=init_gain)
            else:
                raise NotImplementedError('initialization method [%s] is not implemented' % init_type)
            if hasattr(m, 'bias') and m.bias is not None:
                init.constant_(m.bias.data, 0.0)
        elif classname.find('BatchNorm2d') != -1:
            init.normal_(m.weight.data, 1.0, init_gain)
            init.constant_(m.bias.data, 0.0)

    print('initialize network with %s' % init_type)
    net.apply(init_func)


def init_net(net, init_type='normal', init_gain=0.02, gpu_ids=[]):
    """The reference wraps multi-GPU nets in nn.DataParallel (:112-116); here every process drives ONE GPU and
    data parallelism is gradient all-reduce over RCCL (healthivert-gan_amd/ddp.py), so the net just moves to its device."""
    init_weights(net, init_type, init_gain=init_gain)   # on the host RNG: the same seed gives the same weights as a CPU run
    if len(gpu_ids) > 0:
        assert torch.cuda.is_available()
        net.to(gpu_ids[0])
    return net


def define_G(input_nc, output_nc, ngf, netG, norm='batch', use_dropout=False, init_type='normal', init_gain=0.02, gpu_ids=[]):
    if netG in ('resnet_9blocks', 'resnet_6blocks', 'unet_128', 'unet_256'):
        raise NotImplementedError("define_G('%s'): not on the HealthiVert-GAN hot path (Pix2PixModel builds inpaint_networks.Generator; "
                                  "UnetG_CT_mask.define_G is the U-Net variant provided)" % netG)
    raise NotImplementedError('Generator model name [%s] is not recognized' % netG)


def define_D(input_nc, ndf, netD, n_layers_D=3, norm='batch', init_type='normal', init_gain=0.02, gpu_ids=[]):
    norm_layer = get_norm_layer(norm_type=norm)
    if netD == 'basic':
        net = NLayerDiscriminator(input_nc, ndf, n_layers=3, norm_layer=norm_layer)
    elif netD == 'n_layers':
        net = NLayerDiscriminator(input_nc, ndf, n_layers_D, norm_layer=norm_layer)
    elif netD in ('pixel', 'seg'):
        raise NotImplementedError("define_D('%s'): not on the HealthiVert-GAN hot path" % netD)
    else:
        raise NotImplementedError('Discriminator model name [%s] is not recognized' % netD)
    return init_net(net, init_type, init_gain, gpu_ids)


# ================================================================================================ GAN loss
class _GanLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target_is_real, mode):
        loss = torch.zeros((), device=pred.device)
        dz = torch.empty_like(pred)
        ops.gan_loss(pred.contiguous(), target_is_real, mode, loss=loss, dz=dz)
        ctx.save_for_backward(dz)
        return loss

    @staticmethod
    def backward(ctx, g):
        (dz,) = ctx.saved_tensors
        return dz * g, None, None


class GANLoss(nn.Module):
    def __init__(self, gan_mode, target_real_label=1.0, target_fake_label=0.0):
        super().__init__()
        self.register_buffer('real_label', torch.tensor(target_real_label))
        self.register_buffer('fake_label', torch.tensor(target_fake_label))
        self.gan_mode = gan_mode
        if gan_mode not in ('lsgan', 'vanilla', 'wgangp'):
            raise NotImplementedError('gan mode %s not implemented' % gan_mode)
        if target_real_label != 1.0 or target_fake_label != 0.0:
            raise NotImplementedError("GANLoss HIP path: labels 1.0 / 0.0")

    def get_target_tensor(self, prediction, target_is_real):
        return (self.real_label if target_is_real else self.fake_label).expand_as(prediction)

    def __call__(self, prediction, target_is_real):
        if self.gan_mode == 'wgangp':
            raise NotImplementedError("GANLoss('wgangp') is not on the HealthiVert-GAN hot path")
        _lib.require_gpu(prediction)
        return _GanLossFn.apply(prediction, bool(target_is_real), self.gan_mode)


# ================================================================================================ PatchGAN
CONV_BSTATS = True   # BatchNorm backward sums from the epilogue of the data gradient that writes dy (False: a test's reference)
HEAD_NORM = True     # (same bits) the last normalisation + LeakyReLU made where the logits layer stages its input (False: a test's reference)


class _Stem:
    """Layer 0 of a PatchGAN plan: conv + LeakyReLU straight off the input image.  The input tensor changes every call, so the node is bound per
    forward (_DiscPlan.bind_input)."""
    __slots__ = ('p', 'y', 'node')

    def __init__(self, p, y):
        self.p, self.y, self.node = p, y, None


class _Normed:
    """conv -> raw map z -> normalisation + LeakyReLU -> y.  Owns what its neighbours' kernels hand it or take from it; each hand-over is asked of the C
    dispatch once and its buffer is allocated on that first use (a shape's eager warm-up step), never at construction."""
    __slots__ = ('p', 'node', 'z', 'y', 'stats', 'norm', 'bparts_used', 'head_fused', '_fstats', '_bsums', '_head_ok')

    def __init__(self, p, node, z, y, stats, norm):
        self.p, self.node, self.z, self.y, self.stats, self.norm = p, node, z, y, stats, norm
        self.bparts_used = 0          # partial-sum rows the last backward's normalisation took from its consumer's data gradient (0: it reduced itself)
        self.head_fused = False       # the last forward normalised this layer's output where the logits layer stages it
        self._fstats = None           # (partials, rows) of the forward statistics epilogue
        self._bsums = {}              # statistics groups -> (partials, rows) of the backward sums
        self._head_ok = {}            # statistics groups -> the dispatch serves head_call

    def _partials(self, parts):
        return torch.zeros(max(1, parts) * self.p.cout * 2, dtype=torch.float32, device=self.z.t.device), parts

    def forward_stats(self, prec):
        """-> (partials, rows): the BatchNorm statistics leave this conv's own epilogue where its kernel has one (the 4x4 stride-2 layers) and the
        normalisation skips its reduction pass over z; (None, 0) otherwise.  With statistics groups the partials are per image tile, in image order:
        the finalize sums each group's share."""
        if self._fstats is None:
            self._fstats = self._partials(int(self.node.stats_parts(prec)))
        return self._fstats if self._fstats[1] else (None, 0)

    def backward_sums(self, consumer, book, prec, mul_x, groups):
        """-> (partials, rows): the sums of this batch normalisation's backward (sum g, sum g * xhat over the gradient `consumer`'s data gradient writes)
        leave that launch's epilogue and the normalisation's backward skips its reduction pass over g and z; (None, 0) where that kernel has no such
        epilogue.  Asked of the plain data gradient conv_backward issues (none when it accumulates -- not a whole sum, never the case in this chain).
        A buffer per group count: a plan serves the batched fake | real pass (two groups) and a plain pass of the same size, and captured graphs of
        both uses keep their own addresses."""
        if groups not in self._bsums:
            gx = consumer.dx_view(book, 'plain')
            call = consumer.dx_call(book, prec, 'plain', gx, book.accumulates(gx), mul_x=mul_x, bn=(self.z, self.stats, groups, None))
            self._bsums[groups] = self._partials(call.bstats_parts())
        return self._bsums[groups] if self._bsums[groups][1] else (None, 0)

    def head_call(self, head, prec, groups):
        """-> the logits layer's call that applies this layer's normalisation + LeakyReLU where it stages its input (hv_conv_desc.xn_*; that kernel also
        stores the normalised map y the backward reads) -- the normalisation call then only finalises the statistics --, or None where the C
        dispatch has no such kernel (HV_HEAD_NORM=0: always) and the separate pass runs."""
        nm = self.norm
        bn = isinstance(nm, nn.BatchNorm2d)
        xn = (self.stats, nm.weight if bn else None, nm.bias if bn else None, groups if bn else self.z.B, 'lrelu', self.y)
        call = head.node.forward_call(prec, xn=xn, x_raw=self.z)
        if groups not in self._head_ok:
            self._head_ok[groups] = call.supported()
        return call if self._head_ok[groups] else None


class _Logits:
    """The 1-channel logits layer.  Owns the 4-channel carrier of d loss / d logit its backward starts from."""
    __slots__ = ('p', 'node', 'y', 'carrier')

    def __init__(self, p, node, y, carrier):
        self.p, self.node, self.y, self.carrier = p, node, y, carrier

    @property
    def loss_head_ready(self):
        """The single-launch loss head (ops.gan_loss_pair) can write the carrier: fp16 storage, four channels."""
        g = self.carrier
        return g.f16 and g.t.shape[-1] == 4 and g.coff == 0


class _DiscPlan:
    def __init__(self, net, B, H, W, device):
        self.B, self.H, self.W = B, H, W
        dt = ops.storage_dtype(net.precision)        # fp16 buffers in the fp16 mode; input image, logits and dx stay fp32
        z = lambda h, w, C: Act(torch.zeros(B, h, w, rup(C, 4), dtype=dt, device=device), C, 0)
        self.book = E.GradBook()
        self.x4 = z(H, W, 1)
        self.layers = []
        h, w = H, W
        prev = None
        for li, L in enumerate(net._spec):
            ho, wo = ops.conv_out_size(h, 4, L['stride'], 1, 1), ops.conv_out_size(w, 4, L['stride'], 1, 1)
            p = net._pset_convs[li]
            if li == 0:
                ent = _Stem(p, z(ho, wo, p.cout))
            elif L['last']:
                self.logits = torch.zeros(B, 1, ho, wo, dtype=torch.float32, device=device)
                y = Act(self.logits.view(B, ho, wo, 1))
                ent = _Logits(p, E.ConvNode(p, prev, y, L['stride'], 1, 1, 'none', use_bias=True), y, z(ho, wo, 1))
                self.book.twins[id(y.t)] = ent.carrier.t      # the gradient of the logits lives in the carrier
            else:
                zraw = z(ho, wo, p.cout)
                ent = _Normed(p, E.ConvNode(p, prev, zraw, L['stride'], 1, 1, 'none', use_bias=L['bias']), zraw, z(ho, wo, p.cout),
                              torch.zeros(2 * B * p.cout, dtype=torch.float32, device=device), net.model[L['norm']])
            prev = ent.y
            h, w = ho, wo
            self.layers.append(ent)
        self.dx = torch.zeros(B, 1, H, W, dtype=torch.float32, device=device)
        self.pending = None        # weakref to the autograd token of the nn.Module-API forward that owns these activations
        self.x_in = None           # the input view of the last forward (bind_input)
        self.training, self.groups = False, 1      # ... and its mode and statistics groups

    def bind_input(self, x, training, groups):
        """A forward on x (B,1,H,W) begins: the stem reads it, and its gradient lives in self.dx (the previous input's twin is dropped)."""
        if self.x_in is not None:
            self.book.twins.pop(id(self.x_in.t), None)
        self.x_in = Act(x.view(self.B, self.H, self.W, 1))
        self.book.twins[id(self.x_in.t)] = self.dx.view(self.B, self.H, self.W, 1)
        stem = self.layers[0]
        stem.node = E.ConvNode(stem.p, self.x_in, stem.y, 2, 1, 1, 'lrelu', use_bias=True)
        self.training, self.groups = training, groups


def _stat_momentum(m, order):
    if order == 'swapped_first':
        return m / (1.0 - m * (1.0 - m))
    if order == 'swapped_second':
        return m * (1.0 - m)
    return m


class NLayerDiscriminator(nn.Module):
    """PatchGAN: Conv(k4,s2)+LReLU, (n_layers-1)x[Conv(k4,s2)+Norm+LReLU], Conv(k4,s1)+Norm+LReLU, Conv(k4,s1)->1."""

    def __init__(self, input_nc, ndf=64, n_layers=3, norm_layer=nn.BatchNorm2d):
        super().__init__()
        if type(norm_layer) == functools.partial:
            use_bias = norm_layer.func == nn.InstanceNorm2d
            norm_cls = norm_layer.func
        else:
            use_bias = norm_layer == nn.InstanceNorm2d
            norm_cls = norm_layer
        print(norm_layer)
        if input_nc != 1:
            raise NotImplementedError("NLayerDiscriminator HIP path: input_nc == 1")
        if norm_cls not in (nn.BatchNorm2d, nn.InstanceNorm2d):
            raise NotImplementedError("NLayerDiscriminator HIP path: norm in {batch, instance}")
        self.norm_kind = 'batch' if norm_cls == nn.BatchNorm2d else 'instance'
        kw, padw = 4, 1
        seq = [nn.Conv2d(input_nc, ndf, kernel_size=kw, stride=2, padding=padw), nn.LeakyReLU(0.2, True)]
        spec = [dict(conv=0, norm=None, stride=2, bias=True, last=False)]
        nf_mult = 1
        for n in range(1, n_layers):
            nf_prev, nf_mult = nf_mult, min(2 ** n, 8)
            spec.append(dict(conv=len(seq), norm=len(seq) + 1, stride=2, bias=use_bias, last=False))
            seq += [nn.Conv2d(ndf * nf_prev, ndf * nf_mult, kernel_size=kw, stride=2, padding=padw, bias=use_bias),
                    norm_layer(ndf * nf_mult), nn.LeakyReLU(0.2, True)]
        nf_prev, nf_mult = nf_mult, min(2 ** n_layers, 8)
        spec.append(dict(conv=len(seq), norm=len(seq) + 1, stride=1, bias=use_bias, last=False))
        seq += [nn.Conv2d(ndf * nf_prev, ndf * nf_mult, kernel_size=kw, stride=1, padding=padw, bias=use_bias),
                norm_layer(ndf * nf_mult), nn.LeakyReLU(0.2, True)]
        spec.append(dict(conv=len(seq), norm=None, stride=1, bias=True, last=True))
        seq += [nn.Conv2d(ndf * nf_mult, 1, kernel_size=kw, stride=1, padding=padw)]
        self.model = nn.Sequential(*seq)
        self._spec = spec
        self.precision = None
        self._pset = None
        self._pset_convs = None
        self._plans = {}

    def paramset(self):
        if self._pset is None:
            convs, extra = [], []
            for li, L in enumerate(self._spec):
                m = self.model[L['conv']]
                cin, cout = m.in_channels, m.out_channels
                if li == 0:
                    convs.append(E.ConvParams('model.%d' % L['conv'], m.weight, m.bias, cin, cout, 4, cin_fwd=1, cin_wg=4))
                else:
                    convs.append(E.ConvParams('model.%d' % L['conv'], m.weight, m.bias, cin, cout, 4))
                if L['norm'] is not None and self.norm_kind == 'batch':
                    nm = self.model[L['norm']]
                    extra += [nm.weight, nm.bias]
            self._pset_convs = convs
            self._pset = E.ParamSet(convs, extra)
        return self._pset

    def load_state_dict(self, *args, **kwargs):
        r = super().load_state_dict(*args, **kwargs)
        if self._pset is not None:
            self._pset.weights_changed()      # (copied into the same storage: the prepared weight tables are stale)
        return r

    def _plan(self, B, H, W, device, slot=0):
        """slot 0 is the explicit executor's plan (Pix2PixModel's fused step); the nn.Module API takes one plan per forward whose
        autograd graph is still alive (slot 1, 2, ...): `pred_fake = D(fake); pred_real = D(real); loss.backward()` -- the
        reference's own backward_D (pix2pix_model.py:267-283) -- keeps both passes' activations until their backward ran."""
        key = (B, H, W, str(device), slot, ops.precision_id(self.precision))
        if key not in self._plans:
            self.paramset()
            self._plans[key] = _DiscPlan(self, B, H, W, device)
        return self._plans[key]

    def _free_plan_slot(self, B, H, W, device):
        slot = 1
        while True:
            P = self._plans.get((B, H, W, str(device), slot, ops.precision_id(self.precision)))
            if P is None or P.pending is None or P.pending() is None:
                return slot
            slot += 1

    # ---------------------------------------------------------------- explicit forward / backward
    def run_forward(self, x, training=None, prep=True, groups=1, stat_order=None, slot=0):
        """x: (B,1,H,W) device tensor -> plan; logits in plan.logits (B,1,Ho,Wo).  BatchNorm running statistics are
        updated when training (every call, like the reference's three calls per step).  groups=2 treats the two halves of
        the batch as two consecutive calls (separate batch statistics, running stats updated half by half): the fake and
        the real pass of one discriminator update in a single launch sequence.
        stat_order: the train step runs the REAL pass before the FAKE pass (so that it overlaps the generator forward) while the
        reference updates the running statistics fake-then-real; 'swapped_first' / 'swapped_second' use momenta m/(1-m(1-m)) and
        m(1-m), which leave exactly the reference's running statistics after the pair:
        (1-m)^2 r + m(1-m) fake + m real."""
        _lib.require_gpu(x)
        training = self.training if training is None else training
        prec = ops.precision_id(self.precision)
        x = x.contiguous().float()
        B, _, H, W = x.shape
        P = self._plan(B, H, W, x.device, slot)
        P.book.join()   # weight gradients of the previous backward still read this plan's activations on the side stream
        if prep:      # prep='if_stale': skipped when the tables in memory were written from the current weights (the train step: engine.ParamSet.prep)
            self.paramset().prep(x.device, power_iter=False, only_if_stale=(prep == 'if_stale'))
        P.bind_input(x, training, groups)
        bn = self.norm_kind == 'batch'
        head = P.layers[-1]
        P.layers[0].node.forward(prec)
        for ent in P.layers[1:-1]:
            nm = ent.norm
            fused = ent.head_call(head, prec, groups) if (HEAD_NORM and ent is P.layers[-2] and ent.z.f16) else None      # (the layer below the logits)
            ent.head_fused = fused is not None
            partials, parts = ent.forward_stats(prec) if (bn and training) else (None, 0)
            ent.node.forward(prec, stats=partials)
            y_out = None if fused is not None else ent.y
            if bn:
                ops.norm_act_forward(ent.z, y_out, 'batch', training, ent.stats, nm.weight, nm.bias, nm.running_mean,
                                     nm.running_var, nm.num_batches_tracked, act='lrelu', eps=nm.eps, momentum=_stat_momentum(nm.momentum, stat_order),
                                     groups=groups, partials=partials, n_partials=parts)
            else:
                ops.norm_act_forward(ent.z, y_out, 'instance', training, ent.stats, act='lrelu', eps=nm.eps)
        (fused or head.node.forward_call(prec)).launch()
        return P

    def _loss_seed(self, P, ranges, mode, grad_weight, loss_weight=1.0, param_grads=True, accumulate=False, dz=None):
        """GAN loss of each (rows, target_is_real, loss) range of P.logits -> (dlogits, logits_ready) for run_backward.  fp16 storage mode: ONE loss kernel
        writes d loss / d logit straight into the logits layer's gradient carrier and sums its bias gradient (hv_gan_loss_head_pair) -- the copy, the
        column-sum pass and its finalize leave the chain between forward and backward."""
        head = P.layers[-1]
        if head.loss_head_ready:
            want_db = param_grads and head.p.bias is not None and head.node.use_bias
            args = [a for rows, real, loss in ranges for a in (P.logits[rows], real, loss, Act(head.carrier.t[rows], 4, 0))]
            ops.gan_loss_pair(*args, mode=mode, loss_weight=loss_weight, grad_weight=grad_weight, dbias=head.p.bias.grad if want_db else None,
                              dbias_accumulate=accumulate)
            return None, True
        if dz is None:
            dz = torch.empty_like(P.logits)
        for rows, real, loss in ranges:
            ops.gan_loss(P.logits[rows], real, mode, loss=loss, loss_weight=loss_weight, dz=dz[rows], grad_weight=grad_weight)
        return dz, False

    def loss_backward(self, P, target_is_real, mode, loss, grad_weight, need_dx=False, param_grads=True, accumulate=False, loss_weight=1.0, dz=None,
                      backward=True):
        """GAN loss on P.logits + backward (backward=False: the loss value only; the gradient it also writes is read by nobody)."""
        dz, ready = self._loss_seed(P, [(slice(None), target_is_real, loss)], mode, grad_weight, loss_weight, param_grads, accumulate, dz)
        if not backward:
            return None
        return self.run_backward(P, dz, need_dx=need_dx, param_grads=param_grads, accumulate=accumulate, logits_ready=ready)

    def loss_backward_halves(self, P, mode, loss_fake, loss_real, grad_weight, dz=None):
        """The batched fake | real pass (run_forward(..., groups=2) on [fake; real]): GAN loss of each half against its own target + ONE backward
        (fp16 storage mode: both halves in one launch -- four tiny dependent launches between forward and backward -> one)."""
        B = P.B // 2
        dz, ready = self._loss_seed(P, [(slice(0, B), False, loss_fake), (slice(B, None), True, loss_real)], mode, grad_weight, dz=dz)
        return self.run_backward(P, dz, need_dx=False, param_grads=True, accumulate=False, logits_ready=ready)

    def run_backward(self, P, dlogits, need_dx=False, param_grads=True, accumulate=False, logits_ready=False):
        """dlogits: (B,1,Ho,Wo) gradient of the loss wrt the logits.  Fills kernel-layout weight gradients and the
        bias / affine .grad (accumulating when `accumulate`); call finish() afterwards.  Returns d loss / d input."""
        prec = ops.precision_id(self.precision)
        book = P.book
        book.reset()
        B = P.B
        stem, head = P.layers[0], P.layers[-1]
        if not logits_ready:      # (loss_backward: the loss kernel already wrote the carrier and the logits layer's bias gradient)
            ops.copy_channels(Act(dlogits.contiguous().view(B, head.y.H, head.y.W, 1)), head.carrier, mode=0)
        bn = self.norm_kind == 'batch'
        fuse0 = stem.node.act != 'none' and not P.layers[1].node.shift
        # a normalised layer's LeakyReLU' rides in the data-gradient epilogue of the layer that consumes its output z (one consumer), so the
        # normalisation's backward starts from the gradient at ITS output and never reads z
        sums = (None, 0)      # (partials, rows) the data gradient of the layer above summed for this layer's normalisation (_Normed.backward_sums)
        for li in range(len(P.layers) - 1, 0, -1):
            ent, below = P.layers[li], P.layers[li - 1]
            node = ent.node
            prev_normed = li >= 2 and not node.shift       # layer li - 1 has a norm + LeakyReLU
            if ent is not head:
                nm = ent.norm
                ent.bparts_used = sums[1]
                ops.norm_act_backward(book.twin(ent.y), ent.y, ent.z, book.twin(ent.z), self.norm_kind, P.training, ent.stats,
                                      gamma=nm.weight if bn else None, act='none', dgamma=nm.weight.grad if (bn and param_grads) else None,
                                      dbeta=nm.bias.grad if (bn and param_grads) else None, param_accumulate=accumulate,
                                      groups=P.groups, partials=sums[0], n_partials=sums[1])
            # the stem's output has one consumer (layer 1): its LeakyReLU' rides in layer 1's data-gradient epilogue
            mul_x = stem.node.act if (li == 1 and fuse0) else ('lrelu' if prev_normed else None)
            # ... and where layer li - 1 is batch-normalised, the sums of ITS backward leave this data gradient's epilogue (HV_CONV_BSTATS=0: it reduces)
            sums = (None, 0)
            if prev_normed and mul_x and CONV_BSTATS and bn and P.training:
                sums = below.backward_sums(node, book, prec, mul_x, P.groups)
            E.conv_backward(node, book, prec, dbias_accumulate=accumulate, wgrad_accumulate=accumulate, wgrad=param_grads, dbias_done=bool(logits_ready and ent is head),
                            mul_x=mul_x, bn=(below.z, below.stats, P.groups, sums[0]) if sums[1] else None)
        if param_grads:
            ops.copy_channels(P.x_in, P.x4, mode=0)
        stem.node.need_dx = need_dx
        E.conv_backward(stem.node, book, prec, dbias_accumulate=accumulate, wgrad_accumulate=accumulate, wgrad=param_grads,
                        x_wg=P.x4 if param_grads else None, premultiplied=fuse0)
        return book.twin(P.x_in).t.view(B, 1, P.H, P.W) if need_dx else None

    def finish(self):
        for P in self._plans.values():
            P.book.join()
        self.paramset().finish_backward(accumulate=False)
        self.paramset().attach_grads()

    # ---------------------------------------------------------------- nn.Module API
    def forward(self, input):
        if torch.is_grad_enabled() and (input.requires_grad or any(p.requires_grad for p in self.parameters())):
            B, _, H, W = input.shape
            P = self.run_forward(input, slot=self._free_plan_slot(B, H, W, input.device))
            anchor = next((p for p in self.parameters() if p.requires_grad), None)   # carries the graph edge when only the weights need gradients
            return _DiscFn.apply(input, anchor, self, P, P.logits)
        return self.run_forward(input).logits.clone()


class _PlanToken:
    """Alive as long as the autograd node that owns a plan's activations is."""


def grads_are_fresh(net):
    """True when nothing has been written into the net's gradients since the last zero_grad(): the next backward ASSIGNS, later
    ones accumulate -- torch.autograd's .grad semantics for the nn.Module API of the explicit-backward networks.  FusedAdam.zero_grad
    flags the first parameter; torch optimisers either drop .grad (set_to_none) or zero it (then accumulating is right anyway)."""
    ps = list(net.parameters())
    fresh = getattr(ps[0], '_hv_fresh', False) or ps[0].grad is None
    for p in ps:
        p._hv_fresh = False
    return fresh


class _DiscFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, anchor, net, plan, logits):
        import weakref
        ctx.net, ctx.plan, ctx.need_dx = net, plan, x.requires_grad
        ctx.token = _PlanToken()
        plan.pending = weakref.ref(ctx.token)
        return logits.clone()

    @staticmethod
    def backward(ctx, g):
        net, plan = ctx.net, ctx.plan
        if plan.pending is None or plan.pending() is not ctx.token:
            raise RuntimeError("NLayerDiscriminator: the activations of this forward pass were overwritten before its backward ran")
        pg = any(p.requires_grad for p in net.parameters())
        acc = pg and not grads_are_fresh(net)
        # fp16 storage mode: scaled seeds (ops.grad_scale), parameter gradients unscaled afterwards; gradients accumulated onto go from grad_factor to S first
        S = ops.grad_scale(net.precision)
        pset = net.paramset()
        if acc:
            ops.scale_inplace(pset.flat_grad, S / pset.grad_factor)
        if pg:
            pset.attach_grads()
        dx = net.run_backward(plan, g.contiguous() * S if S != 1.0 else g.contiguous(), need_dx=ctx.need_dx, param_grads=pg, accumulate=acc)
        if pg:
            net.finish()
            ops.scale_inplace(pset.flat_grad, 1.0 / S)
        plan.pending = None
        if dx is not None:
            dx = dx.clone()
            ops.scale_inplace(dx, 1.0 / S)
        return dx, None, None, None, None
