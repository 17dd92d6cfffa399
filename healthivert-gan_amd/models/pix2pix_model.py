"""Pix2PixModel on the HIP path: the 2.5D coarse-to-fine generator + three PatchGAN discriminators train step.

API mirror of the reference `models/pix2pix_model.py` (options :51-72, construction :74-135, set_input :137-175,
forward :180-264, backward_D_1/2/3 :267-314, backward_G :317-354, optimize_parameters :356-382).  Same attribute,
loss and visual names (train.py:56-99 reads them), but the step is an explicit sequence of libhvgan kernels:
no autograd tape, no per-sample Python loops, no `.item()` host syncs (the SHRM row bounds are computed on the
device), fused multi-tensor Adam.  Losses stay on the device until get_current_losses() converts them.
"""
import ctypes
import os

import torch

from ._backend import ddp
from ._backend import lib as _lib
from ._backend import ops
from ._backend import optim
from ._backend import step_runner
ptr, stream = _lib.ptr, _lib.stream
EAGER, ShapeState, StepRunner = step_runner.EAGER, step_runner.ShapeState, step_runner.StepRunner
FusedAdam = optim.FusedAdam
from . import networks
from .base_model import BaseModel
from .edge_operator import Sobel
from .inpaint_networks import Generator


def diceCoeff(pred, gt, eps=1e-5, activation='sigmoid'):
    """Dice coefficient (reference :13-39); host-side helper kept for API parity (the train step uses the fused
    hv_generator_losses kernel instead)."""
    if activation not in (None, 'none', 'sigmoid', 'softmax2d'):
        raise NotImplementedError("Activation implemented for sigmoid and softmax2d")
    if activation == 'sigmoid':
        pred = torch.sigmoid(pred)
    elif activation == 'softmax2d':
        pred = torch.softmax(pred, dim=1)
    n = gt.shape[0]
    p, g = pred.reshape(n, -1), gt.reshape(n, -1)
    return ((2 * (g * p).sum(1) + eps) / (p.sum(1) + g.sum(1) + eps)).sum() / n


class Pix2PixModel(BaseModel):
    @staticmethod
    def modify_commandline_options(parser, is_train=True):
        parser.set_defaults(norm='batch', netG='unet_256', dataset_mode='aligned')
        if is_train:
            parser.set_defaults(pool_size=0, gan_mode='vanilla')
            parser.add_argument('--lambda_L1', type=float, default=200.0, help='weight for L1 loss')
        return parser

    def __init__(self, opt):
        # launched by `python -m torch.distributed.run --nproc-per-node N train.py ...`: join the job and drive THIS rank's GPU
        # (train.py itself stays unedited; it passes --gpu_ids 0 to every rank)
        local = ddp.init_from_env()
        if local is not None and opt.gpu_ids:
            opt.gpu_ids = [local]
            torch.cuda.set_device(local)
        BaseModel.__init__(self, opt)
        if not self.gpu_ids:
            raise RuntimeError("Pix2PixModel (healthivert-gan_amd) needs an MI355X: set --gpu_ids 0; there is no CPU path")
        _lib.get()   # fail loudly if libhvgan.so is missing
        self.loss_names = ['G_GAN', 'G_maskL1', 'G_Dice', 'coarse_Dice', 'edge', 'D_real_1', 'D_fake_1', 'D_real_2', 'D_fake_2',
                           'D_real_3', 'D_fake_3', 'h']
        self.visual_names = ['real_A', 'fake_B', 'fake_B_mask_raw', 'normal_vert', 'coarse_seg_binary', 'fake_B_coarse', 'real_B',
                             'mask', 'fake_B_raw', 'real_B_mask', 'CAM', 'real_edges', 'fake_B_local']
        self.model_names = ['G', 'D_1', 'D_2', 'D_3'] if self.isTrain else ['G']
        self.netG = Generator({'input_dim': 1, 'ngf': 16}, True)
        self.netG.to(self.device)
        self.sobel_edge = Sobel(requires_grad=False).to(self.device)
        self.half_band = 35
        self._loss_buf = torch.zeros(32, dtype=torch.float32, device=self.device)
        self._bufs = {}
        self._shapes, self._cur = {}, None      # ShapeState per batch shape, and the active one
        self.grad_sync = self._runner = None
        if self.isTrain:
            if opt.gan_mode not in ('vanilla', 'lsgan'):
                raise NotImplementedError("Pix2PixModel HIP path: gan_mode in {vanilla, lsgan}")
            nets = {'G': self.netG}
            for k in (1, 2, 3):
                nets['D_%d' % k] = networks.define_D(opt.input_nc, opt.ndf, opt.netD, opt.n_layers_D, opt.norm, opt.init_type, opt.init_gain, self.gpu_ids)
            self.criterionGAN = networks.GANLoss(opt.gan_mode).to(self.device)
            self.criterionL1 = torch.nn.L1Loss()
            pairs = {n: (net, FusedAdam(net.parameters(), lr=opt.lr, betas=(opt.beta1, 0.999), paramset=net.paramset)) for n, net in nets.items()}
            for n, (net, optimizer) in pairs.items():      # netD_k / optimizer_D_k: the checkpoint and API contract
                setattr(self, 'net' + n, net)
                setattr(self, 'optimizer_' + n, optimizer)
                self.optimizers.append(optimizer)
            self._D = {k: pairs['D_%d' % k] for k in (1, 2, 3)}      # what the step itself reads
            self.grad_sync = ddp.GradSync()
            ddp.broadcast_parameters(list(nets.values()))      # every rank starts from rank 0's initial weights (a no-op without a process group)
            self._runner = StepRunner((self._phase_a, self._phase_b, self._phase_c), list(pairs.values()), self.grad_sync, self.device, extra_state=[self._loss_buf])
        # gradient scale S (ops.grad_scale; 1 in the fp32 mode): the explicit backward's seeds carry S, so each network's flat gradient holds S times the true
        # one (ParamSet.grad_factor) until its bound optimiser takes 1/S out in the pass that checks it for inf / nan and skips the update if it finds one
        # (overflow_steps(); head room in DESIGN.md section 3).  Under data parallelism that pass reads the reduced gradient: every rank decides alike.
        self.grad_scale = ops.grad_scale(None)
        # fake | real discriminator passes as ONE 2B-sample launch sequence (per-half BatchNorm groups).  Round 2: no gain beside the three-stream overlap;
        # re-measured at the end of round 3 with the pipelined 4x4 kernels (one round of one workgroup per CU at bs 16): 8.18 -> 8.09 ms in three same-box
        # pairs, although it gives up the real-image passes' overlap with the generator forward.  Both the single-process and the data-parallel step take it.
        self.batch_d = os.environ.get('HV_BATCH_D', '1') != '0'

    # names that callers outside the model read (write=True: and set) on it
    GRAPH_WARMUP = StepRunner.GRAPH_WARMUP
    def _runner_attr(name, write=False):
        return property(lambda self: getattr(self._runner, name), (lambda self, v: setattr(self._runner, name, v)) if write else None)
    use_graph, strict_graph = _runner_attr('use_graph', True), _runner_attr('strict_graph', True)
    dp_schedule, dp_preflight_record, dp_capture_error = _runner_attr('dp_schedule'), _runner_attr('dp_preflight_record'), _runner_attr('dp_capture_error')
    _graphs = property(lambda self: self._cur.graphs if self._cur is not None else None)
    _inline_exchange = property(lambda self: self._runner.inline is not None)
    del _runner_attr

    def _bind(self, name, value):
        """Every name a step binds goes through here, into the active ShapeState: set_input() binds them again when the shape comes back (a graph
        replay does not run this Python).  The loss_* attributes are views of the shape-independent _loss_buf and stay plain attributes."""
        self._cur.bound[name] = value
        setattr(self, name, value)
        return value

    # discriminator k's batched input [fake_k | real_k] (2B samples): the step's producers write straight into its halves
    _PAIRED = {'real_B': 1, 'real_B_mask': 2}

    def _pair_buffer(self, k, shape):
        """D_k's 2B-sample input buffer for the current batch shape (lives with the inputs: its upper half IS an input)."""
        key, ins = 'dcat%d' % k, self._cur.inputs
        b = ins.get(key)
        if b is None or b.shape[1:] != tuple(shape[1:]) or b.shape[0] != 2 * shape[0]:
            b = ins[key] = torch.zeros((2 * shape[0],) + tuple(shape[1:]), dtype=torch.float32, device=self.device)
        return b

    # ---------------------------------------------------------------- inputs
    def set_input(self, input):
        """Unpack a batch dict (reference models/pix2pix_model.py:137-175).  The tensors land in persistent device buffers, one ShapeState
        per batch shape: the captured step graphs read their inputs from fixed addresses, and a shape that comes back (the partial
        last batch of every epoch, then full batches again) is not captured again.  The attributes (and get_current_visuals()) are views
        of these buffers: the next set_input of the same shape overwrites them -- clone what must outlive a step."""
        AtoB = self.opt.direction == 'AtoB'
        key = tuple(input['A_mask'].shape)
        st = self._shapes.get(key)
        if st is None:
            st = self._shapes[key] = ShapeState()
        if st is not self._cur:
            self._cur = st
            for n, v in st.bound.items():     # a graph replay does not re-run the Python that binds these names
                setattr(self, n, v)

        def put(name, t, dtype):
            b = st.inputs.get(name)
            if b is None or b.shape != t.shape or b.dtype != dtype:
                pair = self._PAIRED.get(name) if (self.isTrain and self.batch_d) else None
                if pair is not None:      # the real image of D_k is the upper half of D_k's 2B-sample input buffer (fake | real): no copy into it per step
                    b = self._pair_buffer(pair, t.shape)[t.shape[0]:]
                else:
                    b = torch.empty(t.shape, dtype=dtype, device=self.device)
                st.inputs[name] = b
                st.reset()      # input addresses changed
            b.copy_(t, non_blocking=True)
            return b
        self.real_B = put('real_B', input['B' if AtoB else 'A'], torch.float32)
        self.real_B_mask = put('real_B_mask', input['A_mask'], torch.float32)
        self.real_A = put('real_A', input['A' if AtoB else 'B'], torch.float32)
        self.CAM = put('CAM', input['CAM'], torch.float32)
        self.normal_vert = put('normal_vert', input['normal_vert'], torch.float32)
        self.mask = put('mask', input['mask'], torch.float32)
        self.height = put('height', input['height'], torch.int64)
        self.slice_ratio = put('slice_ratio', input['slice_ratio'], torch.float64)
        self.x1 = put('x1', input['x1'], torch.int64)
        self.x2 = put('x2', input['x2'], torch.int64)
        self.maxheight = put('maxheight', input['h2'], torch.int64)
        self.image_paths = input['A_paths' if AtoB else 'B_paths']

    def _buf(self, name, like=None, shape=None, dtype=torch.float32):
        key = (name, tuple(like.shape) if like is not None else tuple(shape))
        b = self._bufs.get(key)
        if b is None:
            b = torch.zeros(key[1], dtype=dtype, device=self.device)
            self._bufs[key] = b
        return b

    @property
    def offset_flow(self):
        """The 5th output of netG (reference :187): coloured arg-max offsets of the contextual attention, built on demand from the
        indices the last forward left on the device (nothing in the train step consumes it)."""
        from .inpaint_networks import offsets_to_flow
        P = getattr(self, '_gplan', None)
        return None if P is None else offsets_to_flow(P.attn.argmax, P.B, P.attn.h, P.attn.w, 2)

    # ---------------------------------------------------------------- forward
    def forward(self):
        L = _lib.get()
        B, _, H, W = self.real_A.shape
        cam_t = self._buf('cam_temp', self.CAM)
        L.call('hv_affine', ptr(cam_t), ptr(self.CAM), ctypes.c_longlong(cam_t.numel()), ctypes.c_float(-1.0), ctypes.c_float(1.0), stream())
        P = self.netG.run_forward(self.real_A, self.mask, cam_t, self.slice_ratio, training=self.netG.training)
        self._bind('_gplan', P)
        for n, t in (('coarse_seg_sigmoid', P.coarse_seg), ('fake_B_mask_sigmoid', P.fine_seg), ('x_stage1', P.x_stage1), ('fake_B_raw', P.x_stage2)):
            self._bind(n, t)
        d = L.hv_postg_desc()
        outs = {}
        paired = self.isTrain and self.batch_d and 'dcat1' in self._cur.inputs
        halves = {'fake_B': (1, 0), 'fake_B_mask_raw': (2, 0), 'fake_B_local': (3, 0), 'real_B_local': (3, 1)} if paired else {}
        for n in ('fake_B', 'fake_B_coarse', 'fake_B_local', 'real_B_local', 'fake_B_mask_raw', 'coarse_seg_binary'):
            if n in halves:      # written by the compositing kernel straight into D_k's [fake | real] input buffer
                k, hi = halves[n]
                outs[n] = self._pair_buffer(k, self.real_B.shape)[hi * B:(hi + 1) * B]
            else:
                outs[n] = self._buf(n, self.real_B)
            self._bind(n, outs[n])
        p1h, p2h = self._bind('pred1_h', self._buf('pred1_h', shape=(1, B))), self._bind('pred2_h', self._buf('pred2_h', shape=(1, B)))
        self._bind('_rows', self._buf('rows', shape=(B, 4), dtype=torch.int32))
        for f, t in (('real_B', self.real_B), ('mask', self.mask), ('x_stage1', P.x_stage1), ('x_stage2', P.x_stage2),
                     ('fine_seg', P.fine_seg), ('coarse_seg', P.coarse_seg), ('pred1', P.pred1), ('pred2', P.pred2),
                     ('height', self.height), ('x1', self.x1), ('x2', self.x2), ('maxheight', self.maxheight),
                     ('fake_B', outs['fake_B']), ('fake_B_coarse', outs['fake_B_coarse']), ('fake_B_local', outs['fake_B_local']),
                     ('real_B_local', outs['real_B_local']), ('fine_bin', outs['fake_B_mask_raw']), ('coarse_bin', outs['coarse_seg_binary']),
                     ('pred1_h', p1h), ('pred2_h', p2h), ('rows', self._rows)):
            setattr(d, f, ptr(t).value)
        d.B, d.H, d.W, d.half_band = B, H, W, self.half_band
        L.call('hv_post_generator', ctypes.byref(d), stream())
        self._bind('real_edges', ops.sobel(self.real_B_mask, self._buf('real_edges', self.real_B)))
        self._bind('fake_edges', ops.sobel(self.fake_B_mask_raw, self._buf('fake_edges', self.real_B)))

    # ---------------------------------------------------------------- discriminator updates
    def _loss_slot(self, i):
        return self._loss_buf[i:i + 1].view(())

    def _backward_D(self, k, fake, real):
        """loss_D_k = 0.5 * (BCE(D_k(fake), 0) + BCE(D_k(real), 1)); backward (reference :267-314).  With batch_d the fake and
        the real pass run as ONE 2B-sample launch sequence whose BatchNorm layers keep separate statistics per half and update
        their running statistics half by half -- arithmetically the reference's two consecutive calls, with twice the work per
        kernel launch."""
        net = self._D[k][0]
        mode = self.opt.gan_mode
        L = _lib.get()
        lf, lr = self._loss_slot(2 * k), self._loss_slot(2 * k + 1)
        if self.batch_d:
            B = fake.shape[0]
            x2 = self._cur.inputs.get('dcat%d' % k)
            if not (x2 is not None and x2.shape[0] == 2 * B and fake.data_ptr() == x2.data_ptr() and real.data_ptr() == x2[B:].data_ptr()):
                # (callers with tensors of their own: gather the two halves)
                x2 = self._buf('dcat%d' % k, shape=(2 * B,) + tuple(fake.shape[1:]))
                n = ctypes.c_longlong(fake.numel())
                L.call('hv_affine', ptr(x2[:B]), ptr(fake), n, ctypes.c_float(1.0), ctypes.c_float(0.0), stream())
                L.call('hv_affine', ptr(x2[B:]), ptr(real), n, ctypes.c_float(1.0), ctypes.c_float(0.0), stream())
            P = net.run_forward(x2, training=True, prep='if_stale', groups=2)      # (step t + 1 finds the tables step t's generator part laid out after D_k's Adam step)
            net.loss_backward_halves(P, mode, lf, lr, 0.5 * self.grad_scale, dz=self._buf('dzz%d' % k, P.logits))
        else:
            P = net.run_forward(fake, training=True, prep='if_stale')
            dz = self._buf('dz%d' % k, P.logits)
            ops.gan_loss(P.logits, False, mode, loss=lf, dz=dz, grad_weight=0.5 * self.grad_scale)
            net.run_backward(P, dz, need_dx=False, param_grads=True, accumulate=False)
            P = net.run_forward(real, training=True, prep=False)
            ops.gan_loss(P.logits, True, mode, loss=lr, dz=dz, grad_weight=0.5 * self.grad_scale)
            net.run_backward(P, dz, need_dx=False, param_grads=True, accumulate=True)
        net.finish()
        net.paramset().grad_factor = self.grad_scale
        setattr(self, 'loss_D_fake_%d' % k, lf)
        setattr(self, 'loss_D_real_%d' % k, lr)

    def _d_real_first(self, k, real):
        """Real-image half of loss_D_k (reference :285-296), run FIRST: it needs nothing from the generator, so its stream overlaps
        the generator forward.  Gradients are assigned; BatchNorm running statistics use the swapped-order momentum."""
        net = self._D[k][0]
        lr = self._loss_slot(2 * k + 1)
        P = net.run_forward(real, training=True, prep='if_stale', stat_order='swapped_first')
        net.loss_backward(P, True, self.opt.gan_mode, lr, 0.5 * self.grad_scale, need_dx=False, param_grads=True, accumulate=False,
                          dz=self._buf('dz%d' % k, P.logits))
        setattr(self, 'loss_D_real_%d' % k, lr)

    def _d_fake_second(self, k, fake):
        """Fake half of loss_D_k, accumulated onto the real half's gradients (a + b == b + a in IEEE arithmetic: same bits as the
        reference's fake-then-real order)."""
        net = self._D[k][0]
        lf = self._loss_slot(2 * k)
        P = net.run_forward(fake, training=True, prep=False, stat_order='swapped_second')
        net.loss_backward(P, False, self.opt.gan_mode, lf, 0.5 * self.grad_scale, need_dx=False, param_grads=True, accumulate=True,
                          dz=self._buf('dz%d' % k, P.logits))
        net.finish()
        net.paramset().grad_factor = self.grad_scale
        setattr(self, 'loss_D_fake_%d' % k, lf)

    def _real_local_early(self):
        """real_B_local = mask * real_B * centre band (reference :254-258,:263) without waiting for the generator."""
        B, _, H, W = self.real_B.shape
        mc = self._bufs.get(('mc', (B, 1, H, W)))
        if mc is None:
            mc = torch.zeros(B, 1, H, W, dtype=torch.float32, device=self.device)
            mc[:, :, :, W // 2 - self.half_band:W // 2 + self.half_band] = 1
            self._bufs[('mc', (B, 1, H, W))] = mc
        out = self._buf('real_B_local_early', self.real_B)
        n = ctypes.c_longlong(out.numel())
        L = _lib.get()
        L.call('hv_affine', ptr(out), ptr(self.mask), n, ctypes.c_float(1.0), ctypes.c_float(0.0), stream())
        L.call('hv_mul3', ptr(out), ptr(self.real_B), ptr(mc), n, stream())      # (mask * real_B) * band, the reference's order
        return out

    def _d_images(self, k):      # (fake, real) that D_k judges
        return ((self.fake_B, self.real_B), (self.fake_B_mask_raw, self.real_B_mask), (self.fake_B_local, self.real_B_local))[k - 1]

    def backward_D_1(self):
        self._backward_D(1, *self._d_images(1))

    def backward_D_2(self):
        self._backward_D(2, *self._d_images(2))

    def backward_D_3(self):
        self._backward_D(3, *self._d_images(3))

    # ---------------------------------------------------------------- generator update
    def _g_step_D(self, k):
        """D_k(fake_k) with the freshly updated D_k, its share of loss_G_GAN and (k != 2) the gradient wrt fake_k."""
        net = self._D[k][0]
        P = net.run_forward(self._d_images(k)[0], training=True, prep=True)
        dz = self._buf('dz%d' % k, P.logits)
        # D_2 sees a thresholded mask: no gradient path to G (reference :201,:324) -- only its loss value is wanted
        dx = net.loss_backward(P, True, self.opt.gan_mode, self._loss_slot(15 + k), self.grad_scale / 6.0, need_dx=True, param_grads=False,
                               loss_weight=1.0 / 6.0, dz=dz, backward=k != 2)
        if k != 2:
            self._dxs[k] = dx

    def backward_G(self, d_done=False):
        L = _lib.get()
        B, _, H, W = self.real_B.shape
        lg = self._loss_slot(0)
        if not d_done:
            self._bind('_dxs', {})
            for k in (1, 2, 3):
                self._g_step_D(k)
        dxs = self._dxs
        g = L.hv_gloss_desc()
        seeds = {n: self._buf(n, self.real_B) for n in ('d_fake_B', 'd_fake_B_coarse', 'd_fine_seg', 'd_coarse_seg')}
        dp1, dp2 = self._buf('d_pred1', shape=(B, 1)), self._buf('d_pred2', shape=(B, 1))
        losses = self._loss_buf[8:14]
        for f, t in (('fake_B', self.fake_B), ('fake_B_coarse', self.fake_B_coarse), ('real_B', self.real_B), ('mask', self.mask),
                     ('fine_seg', self.fake_B_mask_sigmoid), ('coarse_seg', self.coarse_seg_sigmoid), ('real_B_mask', self.real_B_mask),
                     ('normal_vert', self.normal_vert), ('fake_edges', self.fake_edges), ('real_edges', self.real_edges),
                     ('pred1_h', self.pred1_h), ('pred2_h', self.pred2_h), ('height', self.height), ('maxheight', self.maxheight),
                     ('losses', losses), ('d_fake_B', seeds['d_fake_B']), ('d_fake_B_coarse', seeds['d_fake_B_coarse']),
                     ('d_fine_seg', seeds['d_fine_seg']), ('d_coarse_seg', seeds['d_coarse_seg']), ('d_pred1', dp1), ('d_pred2', dp2)):
            setattr(g, f, ptr(t).value)
        g.lambda_L1 = float(self.opt.lambda_L1)
        g.grad_scale = self.grad_scale
        # loss_G_GAN = the three discriminators' terms, loss_G, and the discriminator's gradient wrt fake_B added to its seed: folded into the loss
        # kernels (they were six 1-element / 4-MB launches in a row at the head of the generator backward)
        self.loss_G = self._loss_slot(14)
        g.gan_terms, g.n_gan_terms = ptr(self._loss_buf[16:19]).value, 3
        g.loss_G_GAN, g.loss_G = ptr(lg).value, ptr(self.loss_G).value
        g.add_d_fake_B = ptr(dxs[1]).value
        g.B, g.H, g.W = B, H, W
        need = L.size('hv_generator_losses_workspace_bytes', B)
        ws, _ = ops._ws(need, self.device, slot=1)
        g.workspace, g.workspace_bytes = ptr(ws).value, ws.numel()
        L.call('hv_generator_losses', ctypes.byref(g), stream())
        self.loss_G_GAN = lg
        self.loss_G_maskL1, self.loss_G_Dice, self.loss_coarse_Dice = losses[0], losses[1], losses[2]
        self.loss_edge, self.loss_h = losses[3], losses[4]
        # gradient wrt the composited images -> wrt the raw generator outputs (rows [xu, xb) only)
        d_x2, d_x1 = self._buf('d_x_stage2', self.real_B), self._buf('d_x_stage1', self.real_B)
        L.call('hv_shrm_backward', ptr(seeds['d_fake_B']), ptr(dxs[3]), ptr(self.mask), ptr(self._rows), 0, ptr(d_x2), B, H, W,
               self.half_band, 0, stream())
        L.call('hv_shrm_backward', ptr(seeds['d_fake_B_coarse']), None, None, ptr(self._rows), 1, ptr(d_x1), B, H, W, self.half_band, 0, stream())
        self.netG.run_backward(self._gplan, seeds['d_coarse_seg'], seeds['d_fine_seg'], d_x1, d_x2, dp1, dp2)
        self.netG.paramset().grad_factor = self.grad_scale

    # ---------------------------------------------------------------- the step, in three device-only phases
    def _phase_a(self, mode=EAGER):
        """forward; D_1, D_2, D_3 forward/backward (reference :356-370 up to the optimiser steps), each discriminator on its own stream
        (StepRunner.sides).  `mode` (step_runner.StepMode) says how the runner is taking the step."""
        main = torch.cuda.current_stream(self.device)
        sides = self._runner.sides(main)
        self._bind('_dxs', {})
        split = not self.batch_d
        def on(k):
            if sides[k - 1] is not main:
                sides[k - 1].wait_stream(main)
            return sides[k - 1]
        if split:      # the discriminators' real-image passes do not depend on the generator: they start now, on their streams
            reals = {1: self.real_B, 2: self.real_B_mask, 3: self._real_local_early()}
            for k, (net, optimizer) in self._D.items():
                with torch.cuda.stream(on(k)):
                    self.set_requires_grad(net, True)
                    optimizer.zero_grad()
                    self._d_real_first(k, reals[k])
        # (Measured and not kept: the batched passes' weight tables laid out on the discriminator streams BEFORE the generator forward -- the early
        # fork of the three streams in the step graph costs more than the 25 us it hides: 7.89 -> 8.05-8.38 ms over four same-box pairs.)
        self.forward()
        for k, (net, optimizer) in self._D.items():
            with torch.cuda.stream(on(k)):
                if split:
                    self._d_fake_second(k, self._d_images(k)[0])
                else:
                    self.set_requires_grad(net, True)
                    optimizer.zero_grad()
                    self._backward_D(k, *self._d_images(k))
                if mode.inline == 'overlapped':       # D_k's mean over the ranks, beside the other discriminators' passes
                    self.grad_sync.reduce_branch(net.paramset().flat_grad)
        if not mode.through:
            self._runner.join(main)

    def _phase_b(self, mode=EAGER):
        """D_k optimiser step, D_k forward on the fakes with the updated weights (its own stream), generator losses and
        backward (reference :370-382 up to optimizer_G.step)."""
        main = torch.cuda.current_stream(self.device)
        for (k, (_, optimizer)), side in zip(self._D.items(), self._runner.sides(main)):
            if side is not main and not mode.through:
                side.wait_stream(main)
            with torch.cuda.stream(side):
                optimizer.step(sync_lr=False)
                self._g_step_D(k)
        self._runner.join(main)
        self.set_requires_grad([self.netD_1, self.netD_2, self.netD_3], False)
        self.optimizer_G.zero_grad()
        self.backward_G(d_done=True)

    def _phase_c(self, mode=EAGER):
        self.optimizer_G.step(sync_lr=False)

    def optimize_parameters(self):
        """forward; D_1, D_2, D_3 updates; G update (reference :356-382): the three phases above, taken by the StepRunner -- eagerly at first, then
        as a captured hipGraph per batch shape, in a multi-GPU job with the four networks' flat gradients averaged over the ranks inside the step."""
        return self._runner.step(self._cur)

    def overflow_steps(self):
        """{network: optimiser steps skipped by the overflow guard so far} (a host read)."""
        return {n: getattr(self, 'optimizer_' + n).skipped_steps() for n in ('G', 'D_1', 'D_2', 'D_3')}

    OVERFLOW_WARN_RUN = 3      # consecutive loss reads that each saw new skipped steps before the scale is called too large

    def get_current_losses(self):
        """The reference's loss dict (base_model.py:136-142).  The losses are read on the host here anyway, so the overflow guard's counters are read
        with them: a step skipped by the guard is reported on the spot, and skips seen at OVERFLOW_WARN_RUN reads in a row say that HV_GRAD_SCALE is
        too large for this data (a persistent overflow would otherwise freeze a network's weights behind normal-looking losses)."""
        out = BaseModel.get_current_losses(self)
        if self.isTrain and self.grad_scale != 1.0:
            now = self.overflow_steps()
            last = getattr(self, '_overflow_seen', None) or dict.fromkeys(now, 0)
            new = {n: now[n] - last[n] for n in now if now[n] > last[n]}
            self._overflow_seen = now
            self._overflow_run = getattr(self, '_overflow_run', 0) + 1 if new else 0
            if new:
                import warnings
                msg = 'fp16 overflow guard skipped optimiser steps since the last loss read: %s (HV_GRAD_SCALE=%g)' % (new, self.grad_scale)
                if self._overflow_run >= self.OVERFLOW_WARN_RUN:
                    msg += ' -- %d reads in a row: the gradient scale is too large for this data, restart with HV_GRAD_SCALE=%g' % (self._overflow_run, self.grad_scale / 4)
                warnings.warn(msg)
        return out
