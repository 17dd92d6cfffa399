"""Explicit forward/backward executors of the hot path: sequences of libhvgan kernel launches over
pre-allocated NHWC buffers, with no autograd tape, no host synchronisation and no allocation after
the first call for a given shape (so a whole train step can be captured in a hipGraph).

The nn.Modules of `models/` hold the parameters (reference state-dict keys) and delegate here.
"""
import contextlib
import ctypes
import os
import types

import torch

from . import lib as _lib
from . import ops
from .lib import ptr, stream
from .ops import Act, rup


def precision_note(precision):
    """What the precision mode means, for bench.py's config record."""
    if precision in ('fp16', 'f16'):
        return 'fp16 MFMA operands / fp32 accumulate; activations and gradients stored as fp16 (image tensors, attention scores, weights, statistics fp32)'
    return 'fp32 MFMA (v_mfma_f32_16x16x4_f32), fp32 storage'


# ================================================================================================ parameters
# weight_prep_kernel (csrc/prep.hip) stages a spectral-norm layer's v and u in LDS arrays of PREP_MAXK = 4608 and PREP_MAXCO = 1024 floats
SN_MAX_K, SN_MAX_COUT = 4608, 1024


class ConvParams:
    """One convolution's parameters and their kernel-layout copies.

    weight: [cout,cin,k,k] (or [cin,cout,k,k] with transposed_src, i.e. nn.ConvTranspose2d).
    cin_fwd / cin_wg: channel width consumed by the forward gather / by the weight-gradient kernel
    (equal except for a 1-channel image input, which the forward reads unpadded)."""

    def __init__(self, name, weight, bias, cin, cout, k, cin_fwd=None, cin_wg=None, u=None, v=None, transposed_src=False):
        self.name, self.weight, self.bias = name, weight, bias
        self.cin, self.cout, self.k, self.taps = cin, cout, k, k * k
        self.cin_fwd = rup(cin, 4) if cin_fwd is None else cin_fwd
        self.cin_wg = rup(cin, 4) if cin_wg is None else cin_wg
        self.coutP = rup(cout, 4)
        self.u, self.v = u, v
        self.sn = u is not None
        self.transposed_src = transposed_src
        if self.sn and transposed_src:
            # the sigma kernel reads the source as [cout][cin*taps]; a conv-transpose source is [cin][cout][taps] (no model builds the combination)
            raise ValueError('%s: spectral norm on a transposed_src (conv-transpose) weight is not supported' % name)
        if self.sn and (cin * self.taps > SN_MAX_K or cout > SN_MAX_COUT):
            raise ValueError('%s: spectral norm takes cin * k * k <= %d and cout <= %d (got %d, %d)' % (name, SN_MAX_K, SN_MAX_COUT, cin * self.taps, cout))
        self.w_fwd = self.w_bwd = self.sigma = self.dw = None
        self.w_fwd_t = self.w_bwd_t = None      # fp16 tables in MFMA-fragment order (None: the shape has no tiled form)
        # which prepared tables the layer's forward / data-gradient convolutions have read so far (hv_last_weight_tables bits: 1 fp32, 2 fp16 rows, 4 fp16
        # fragment order; 0 = not seen yet): ParamSet.prep writes only those inside a lean_tables() context
        self.use_fwd = self.use_bwd = 0
        self.owner = None
        self.split_k = None                     # K2: also keep the first K2 input channels as a fragment-ordered table of their own (w_fwd_t2: conv2d's x1 layers)
        self.w_fwd_t2 = None

    def sizes(self):
        return (self.cout * self.taps * self.cin_fwd, self.cin_fwd * self.taps * self.coutP, self.coutP * self.taps * self.cin_wg)


class ParamSet:
    """All convolutions of one network: batched weight preparation (spectral norm + layouts), batched
    weight-gradient finalisation, flat gradient storage (one all-reduce per network under DDP)."""

    def __init__(self, convs, extra_params=()):
        self.convs = list(convs)
        self.extra = list(extra_params)          # other trainable tensors (fc, BN affine, biases are added automatically)
        self.device = None
        self.t_prep = {True: ops.LayerTable('hv_wprep_layer'), False: ops.LayerTable('hv_wprep_layer')}
        self.t_bwd = {True: ops.LayerTable('hv_wprep_bwd_layer'), False: ops.LayerTable('hv_wprep_bwd_layer')}
        # lean tables by (parameter storage, power iteration, the layers' table-use bits): a captured step graph keeps the DEVICE address of the table it was
        # captured with, and the use bits can still grow afterwards (another batch shape's first eager step, an eval forward at another size), so a table
        # is never rebuilt in place or freed -- a new bit pattern gets a new table and the old graphs keep theirs (a superset of bits stays correct for them:
        # the layout pass then merely writes a table they do not read)
        self.t_lean = {}
        # the slab-fold chains of this network's weight gradients, one per stream they are issued on (ops.FoldChain)
        self.fold_chains = {}
        for c in self.convs:
            c.owner = self
        self.flat_grad = None
        # the factor by which flat_grad differs from the true gradient: S (ops.grad_scale) from Pix2PixModel's backward until the bound FusedAdam step, else 1
        self.grad_factor = 1.0
        self._key = None
        # which weights the prepared tables belong to: `version` counts the changes of the parameters that this code knows of (weights_changed(), new
        # storage), `prepared` = (version, table set) of the last prep launch.  prep(only_if_stale=True) skips the launch when both still match --
        # the discriminators' tables written for the generator's part of step t are the ones the discriminator update of step t + 1 reads
        self.version = 0
        self.prepared = None

    def trainable(self):
        seen, out = set(), []
        for c in self.convs:
            for p in (c.weight, c.bias):
                if p is not None and id(p) not in seen:
                    seen.add(id(p))
                    out.append(p)
        for p in self.extra:
            if id(p) not in seen:
                seen.add(id(p))
                out.append(p)
        return out

    def _ensure(self, device):
        key = tuple(p.data_ptr() for p in self.trainable()) + tuple(c.u.data_ptr() for c in self.convs if c.sn)
        if key == self._key and self.device == device:
            return
        self._key, self.device = key, device
        self.version += 1
        tot = sum(sum(c.sizes()) + 4 for c in self.convs)
        store = torch.zeros(tot, dtype=torch.float32, device=device)
        off = 0
        for c in self.convs:
            a, b, d = c.sizes()
            c.w_fwd = store[off:off + a]; off += a
            c.w_bwd = store[off:off + b]; off += b
            c.dw = store[off:off + d]; off += d
            c.sigma = store[off:off + 4]; off += 4
            c.sigma[0] = 1.0            # (layers without spectral norm: hv_weight_prep2 skips the sigma kernel when a net has none)
        self._store = store
        # fp16 copies of the prepared weights (halo-tiled conv kernel, HV_F16 precision)
        hstore = torch.zeros(sum(c.sizes()[0] + c.sizes()[1] + 16 for c in self.convs), dtype=torch.float16, device=device)
        off = 0
        for c in self.convs:
            a, b, _ = c.sizes()
            c.w_fwd_h = hstore[off:off + a]; off += (a + 7) // 8 * 8
            c.w_bwd_h = hstore[off:off + b]; off += (b + 7) // 8 * 8
        self._hstore = hstore
        # the same fp16 tables in MFMA-fragment order, for the kernels that fetch filter rows straight into MFMA registers (zero-filled once:
        # the prep kernel never writes the padding rows)
        tsz = [(ops.tiled_elems(c.cout, c.taps, c.cin_fwd), ops.tiled_elems(c.cin_fwd, c.taps, c.coutP),
                ops.tiled_elems(c.cout, c.taps, c.split_k) if c.split_k else 0) for c in self.convs]
        tstore = torch.zeros(sum(a + b + e for a, b, e in tsz) + 8, dtype=torch.float16, device=device)
        off = 0
        for c, (a, b, e) in zip(self.convs, tsz):
            c.w_fwd_t = tstore[off:off + a] if a else None; off += a
            c.w_bwd_t = tstore[off:off + b] if b else None; off += b
            c.w_fwd_t2 = tstore[off:off + e] if e else None; off += e
        self._tstore = tstore
        # flat gradients; .grad of every trainable tensor is a view into it
        ps = self.trainable()
        n = sum(p.numel() for p in ps)
        # (grad_home: a caller-provided slice of a larger buffer -- the data-parallel step keeps the three discriminators' flat gradients
        # back to back so that ONE all-reduce averages them all)
        home = getattr(self, 'grad_home', None)
        if home is not None and home.numel() == n and home.device == torch.device(device) and home.dtype == torch.float32:
            self.flat_grad = home
            self.flat_grad.zero_()
        else:
            self.flat_grad = torch.zeros(n, dtype=torch.float32, device=device)
        self.grad_factor = 1.0
        off = 0
        for p in ps:
            p.grad = self.flat_grad[off:off + p.numel()].view_as(p)
            off += p.numel()
        for pi in (True, False):
            self.t_prep[pi].update(self._prep_rows(pi, False), key, device)
        for acc in (True, False):
            rows = []
            for c in self.convs:
                rows.append(dict(dw_ohwi=c.dw, w_fwd=c.w_fwd, u=c.u if c.sn else None, v=c.v if c.sn else None, sigma=c.sigma,
                                 dw_orig=c.weight.grad, Cout=c.cout, Cin=c.cin, taps=c.taps,
                                 CinP=c.coutP if c.transposed_src else c.cin_wg, sn=int(c.sn),
                                 transposed_src=int(c.transposed_src), accumulate=int(acc)))
            self.t_bwd[acc].update(rows, key, device)

    def attach_grads(self):
        """Re-point .grad at the flat buffer (optimizer.zero_grad(set_to_none=True) drops the views).  Ends every explicit backward: grad_factor 1."""
        self.grad_factor = 1.0
        off = 0
        for p in self.trainable():
            n = p.numel()
            if p.grad is None or p.grad.data_ptr() != self.flat_grad.data_ptr() + 4 * off:
                p.grad = self.flat_grad[off:off + n].view_as(p)
            off += n

    def _prep_rows(self, pi, lean):
        rows = []
        for c in self.convs:
            # lean: only the tables the layer's convolutions have been seen to read (0 = not seen yet: all of them); conv_transpose sources keep all (their
            # layout kernels write every table), spectral-norm layers keep the fp32 forward table (hv_weight_prep_backward reads it)
            mf = mb = 7
            if lean and not c.transposed_src:
                mf = (c.use_fwd or 7) | (1 if c.sn else 0)
                mb = c.use_bwd or 7
            rows.append(dict(w_orig=c.weight.data, u=c.u if c.sn else None, v=c.v if c.sn else None, sigma=c.sigma,
                             w_fwd=c.w_fwd if mf & 1 else None, w_bwd=c.w_bwd if mb & 1 else None, w_fwd_h=c.w_fwd_h if mf & 2 else None,
                             w_bwd_h=c.w_bwd_h if mb & 2 else None, w_fwd_t=c.w_fwd_t if mf & 4 else None, w_bwd_t=c.w_bwd_t if mb & 4 else None,
                             Cout=c.cout, Cin=c.cin, taps=c.taps, CinP=c.cin_fwd, CoutF=c.cout, CoutP=c.coutP, CinB=c.cin_fwd, sn=int(c.sn),
                             power_iter=int(pi and c.sn), transposed_src=int(c.transposed_src), w_fwd_t2=c.w_fwd_t2, K2=int(c.split_k or 0)))
        return rows

    def weights_changed(self):
        """The parameters were written by something other than this ParamSet's own launches: the next prep(only_if_stale=True) must run.  Bound FusedAdam
        steps, load_state_dict and ddp.broadcast_parameters call it; code that writes `p.data` itself must too (that moves no torch version counter)."""
        self.version += 1

    def prep(self, device, power_iter, only_if_stale=False):
        self._ensure(device)
        pi = bool(power_iter)
        table = self.t_prep[pi]
        tset = 'full'
        if LEAN and ops.precision_id(None) == ops.F16:
            tset = tuple((c.use_fwd, c.use_bwd) for c in self.convs)
        if only_if_stale and not pi and PREP_SKIP and self.prepared is not None and self.prepared[0] == self.version and self.prepared[1] in ('full', tset):
            return      # the tables in memory were written from these very weights (and cover the tables asked for)
        self.prepared = (self.version, tset)
        if LEAN and ops.precision_id(None) == ops.F16:
            # inside the train step, after the step has been seen once for this batch shape: the layout pass skips the tables no kernel of the layer reads
            # (fp16 mode: the big layers read the fragment-ordered tables only -- 4 of 20 bytes per weight)
            key = (self._key, pi, tuple((c.use_fwd, c.use_bwd) for c in self.convs))
            table = self.t_lean.get(key)
            if table is None:
                table = self.t_lean[key] = ops.LayerTable('hv_wprep_layer')
                table.update(self._prep_rows(pi, True), key, device)
        ops.weight_prep(table, max(c.sizes()[0] + c.sizes()[1] for c in self.convs), any_sn=any(c.sn for c in self.convs),
                        any_legacy=any(c.transposed_src for c in self.convs))

    def fold_chain(self):
        """The FoldChain of the current stream (weight gradients of this network issued there carry each other's slab folds)."""
        h = torch.cuda.current_stream().cuda_stream
        c = self.fold_chains.get(h)
        if c is None:
            c = self.fold_chains[h] = ops.FoldChain(h)
        return c

    def flush_folds(self):
        """The current stream's last recorded fold as a launch of its own; chains of other streams must have been flushed there before the join."""
        h = torch.cuda.current_stream().cuda_stream
        for k, c in self.fold_chains.items():
            if k == h:
                c.flush()
            else:
                assert c.pending is None, 'a weight-gradient fold chain of another stream was not flushed before finish_backward()'

    def finish_backward(self, accumulate=False):
        """Kernel-layout weight gradients -> .grad of weight_orig / weight (spectral-norm backward included)."""
        self.flush_folds()
        ops.weight_prep_backward(self.t_bwd[bool(accumulate)], max(c.cout * c.cin * c.taps for c in self.convs), any(c.sn for c in self.convs))


class ConvNode:
    """conv (+bias +activation) between two NHWC views; knows how to run forward and backward."""
    __slots__ = ('p', 'x', 'y', 'k', 's', 'pad', 'd', 'act', 'shift', 'need_dx', 'transposed', 'use_bias', 'dx_c', 'pool_to', 'split', 'full')

    def __init__(self, p, x, y, s=1, pad=0, d=1, act='none', shift=0, need_dx=True, transposed=False, use_bias=True, dx_c=None):
        self.p, self.x, self.y, self.k, self.s, self.pad, self.d = p, x, y, p.k, s, pad, d
        self.act, self.shift, self.need_dx, self.transposed, self.use_bias = act, shift, need_dx, transposed, use_bias
        # dx_c: only the first dx_c input channels' gradient is wanted (a concat input whose tail channels are network inputs): the data
        # gradient is then a convolution with fewer output channels (the first dx_c rows of the transposed filter table)
        self.dx_c = dx_c
        # pool_to = (Act low, activation of low's producer): x is a concat buffer whose first dx_c channels are the nearest x2 up-sampling of `low`.  Set once by
        # the layer's owner; conv_backward takes the pooled data gradient (dx_call form 'pool_to') where pooled() says the dispatch serves it
        self.pool_to = None
        # split = (Act low, Act x1): x is the concat [nearest x2 up-sampling of low (p.split_k channels) | x1 (one channel) | padding]; where the
        # filters-in-LDS kernel serves the shape the forward reads `low` with the fused up-sampling and adds x1's taps in its epilogue, so the
        # up-sampled part of x is only materialised for the backward (split_forward() tells)
        self.split = None
        self.full = None      # full_scratch()

    def forward_call(self, prec, xn=None, x_raw=None):
        """The call that runs this node's forward (ops.ConvCall).  Where `split` is set and the dispatch serves that form (the x1 kernel exists for two
        channel shapes only and follows the HV_CONV_LF knob) it reads [up-sampled low | x1] without the concat; otherwise x -- or, with xn, the
        normalisation's raw input x_raw, normalised + activated where the kernel stages it (xn's `out` fills x)."""
        p = self.p
        kw = dict(bias=p.bias if self.use_bias else None, act=self.act, w_h=p.w_fwd_h, precision=prec, cout=p.cout, wuse=(p, 'use_fwd'))
        if self.split is not None and p.w_fwd_t2 is not None and ops.precision_id(prec) == ops.F16:
            low, x1 = self.split
            if low.f16 and self.y.f16 and low.C == p.split_k:
                call = ops.ConvCall(low, p.w_fwd, self.y, self.k, self.s, self.pad, self.d, w_t=p.w_fwd_t2, in_shift=1, cin=p.split_k,
                                    x1=(x1, p.w_fwd, p.split_k, p.taps * p.cin_fwd, p.cin_fwd), **kw)
                if call.supported():
                    return call
        src = self.x if x_raw is None else x_raw
        return ops.ConvCall(Act(src.t, p.cin_fwd, src.coff), p.w_fwd, self.y, self.k, self.s, self.pad, self.d, w_t=p.w_fwd_t, in_shift=self.shift,
                            transposed=self.transposed, xn=xn, **kw)

    def split_forward(self, prec):
        """True when the forward reads [up-sampled low | x1] without the concat; otherwise the materialised concat is built and read."""
        return bool(self.forward_call(prec).d.x1)

    def forward(self, prec, stats=None, xn=None, x_raw=None):
        self.forward_call(prec, xn, x_raw).launch(stats)

    def stats_parts(self, prec):
        """Partial-sum rows this node's forward kernel writes when handed a statistics buffer (0: that kernel has no such epilogue)."""
        return self.forward_call(prec).stats_parts()

    def dx_view(self, book, form):
        """The gradient view the data gradient of `form` (dx_call) writes: that of pool_to's tensor for 'pool_to', else x's (its first dx_c channels)."""
        a = self.pool_to[0] if form == 'pool_to' else self.x
        g = book.twin(a)
        C = a.C if form == 'pool_to' else self.p.cin_fwd
        return Act(g.t, C if form == 'src' else self.dx_c or C, g.coff)

    def dx_call(self, book, prec, form, dst, accumulate, mul_x=None, bn=None):
        """The call that writes this node's data gradient into the gradient view dst (ops.ConvCall) in one of conv_backward's forms: 'src' (transposed
        node: plain convolution), 'pool_to' (2x2-pooled into pool_to's gradient, times act' of it), 'pool' (fused up-sampling: 2x2-pooled into x's),
        'full' (fused up-sampling: full resolution, the caller adds the adjoint copy) or 'plain'.  mul_x ('pool', 'plain'): times act'(x); bn: see
        conv_backward.  accumulate: the caller's book.mark(dst), or book.accumulates(dst) when it asks ahead of the write."""
        p = self.p
        gy = book.twin(self.y)
        mul = None
        if form == 'pool_to' and self.pool_to[1] != 'none':
            mul = (Act(self.pool_to[0].t, dst.C, self.pool_to[0].coff), self.pool_to[1])
        elif form in ('pool', 'plain') and mul_x:
            mul = (Act(self.x.t, p.cin_fwd, self.x.coff), mul_x)
        return ops.ConvCall(Act(gy.t, p.coutP, gy.coff), p.w_bwd, dst, self.k, self.s, self.pad, self.d, transposed=form != 'src', pool2=form in ('pool', 'pool_to'),
                            accumulate=int(accumulate), precision=prec, w_h=p.w_bwd_h, w_t=p.w_bwd_t, mul=mul, bn=bn, wuse=(p, 'use_bwd'))

    def full_scratch(self):
        """Full-resolution buffer for the data gradient of a node with fused up-sampling (dx_call form 'full'): built where that fallback first runs."""
        if self.full is None:
            x = self.x
            self.full = Act(torch.zeros(x.B, x.H * 2, x.W * 2, x.ld, dtype=x.t.dtype, device=x.t.device), self.p.cin_fwd, 0)
        return self.full

    def pooled(self, book, prec, form='pool', mul_x=None):
        """Can the data gradient leave 2x2-pooled in `form` ('pool' or 'pool_to')?  Asked of the call conv_backward would launch."""
        dst = self.dx_view(book, form)
        return self.dx_call(book, prec, form, dst, book.accumulates(dst), mul_x=mul_x).supported()


# streams on which weight gradients stay in line instead of forking to a side stream: the per-discriminator streams of
# the train step (three chains already run concurrently there, and a fork nested inside a forked stream crashes
# hipStreamEndCapture on ROCm 7.2 when the step is captured as a graph)
NO_FORK_STREAMS = set()
_named_streams = {}


def named_stream(name, device, priority=0):
    """Process-wide HIP stream for a role (a discriminator's stream, the capture stream, the weight-gradient side stream of a parent stream ...).
    torch hands out streams from a pool of 32 per device and priority, round-robin: models that each create their own streams wrap that
    pool after a few instances, two roles then share one HIP stream handle and handle-keyed state (NO_FORK_STREAMS, the per-stream scratch
    buffers) changes the launch order from one model to the next.  A role keeps one stream for the life of the process instead."""
    dev = torch.device(device)
    key = (name, dev.index if dev.index is not None else torch.cuda.current_device(), priority)
    st = _named_streams.get(key)
    if st is None:
        st = _named_streams[key] = torch.cuda.Stream(device=dev, priority=priority)
    return st


PREP_SKIP = os.environ.get('HV_PREP_SKIP', '1') != '0'      # A/B knob: ParamSet.prep(only_if_stale=True) may skip (see there)
LEAN = False              # set by lean_tables(): the caller vouches that every convolution of its networks has run once for the current shapes


@contextlib.contextmanager
def lean_tables(on=True):
    """Inside: ParamSet.prep writes only the weight tables the layers' convolutions have been seen to read (ConvParams.use_fwd / use_bwd).  For
    the train step after its first eager step for a batch shape: the same kernels are dispatched again (dispatch is a function of the shapes),
    so the unread tables may go stale.  Outside (eval forwards, the nn.Module API, another shape's first step) every table is written."""
    global LEAN
    prev, LEAN = LEAN, bool(on)
    try:
        yield
    finally:
        LEAN = prev


SERIAL = False            # True: no side streams at all (per-kernel timing with HIP events needs the GPU to itself)


class GradBook:
    """Gradient twins of activation buffers; first write assigns, later writes accumulate."""

    def __init__(self):
        self.twins = {}
        self.written = set()
        self.side = None          # side HIP stream for weight gradients (they overlap the data-gradient chain)
        self._side_of = None      # ... of this parent stream
        self.wgrad_block = WgradBlock()

    def fork(self):
        """Side stream, ordered after everything queued so far on the current stream."""
        cur = torch.cuda.current_stream()
        if self.side is None or self._side_of != cur.cuda_stream:
            self.side, self._side_of = named_stream('wgrad-side-of-%x' % cur.cuda_stream, cur.device), cur.cuda_stream
        self.side.wait_stream(cur)
        return self.side

    def join(self):
        """The current stream waits for the side stream's weight gradients."""
        if self.side is not None:
            torch.cuda.current_stream().wait_stream(self.side)

    def twin(self, a):
        t = self.twins.get(id(a.t))
        if t is None:
            t = torch.zeros_like(a.t)
            self.twins[id(a.t)] = t
        return Act(t, a.C, a.coff)

    def reset(self):
        self.written.clear()

    def accumulates(self, a):
        """-> accumulate flag of the next write into the gradient of view `a` (mark() records that write)."""
        return (id(a.t), a.coff, a.C) in self.written

    def mark(self, a):
        """-> accumulate flag for a write into the gradient of view `a`."""
        acc = self.accumulates(a)
        self.written.add((id(a.t), a.coff, a.C))
        return acc


class WgradBlock:
    """Weight gradients of one backward that run as a block on ONE side stream beside an independent part of the backward (round 4): they only feed the
    optimiser.  open() decides once per backward whether it may fork (no side streams at all under SERIAL, no fork nested in a NO_FORK_STREAMS stream); while the
    block collects, conv_backward queues its weight gradient here instead of launching it (its operands -- the layer's input and the finished gradient of its
    output -- stay as they are until the next backward); launch() is one fork: the queue in order on the side stream, then that stream's last slab fold; join()
    is the one join.  A backward that does not fork never collects: everything runs in line where it is issued."""
    __slots__ = ('side', 'collecting', 'queue', 'later', 'pset')

    def __init__(self):
        self.side, self.collecting, self.queue, self.later, self.pset = None, False, [], [], None

    def open(self, pset, device):
        """Start of a backward of the network whose parameters are `pset`: collecting starts here where the backward may fork."""
        fork = not SERIAL and torch.cuda.current_stream().cuda_stream not in NO_FORK_STREAMS
        self.side = named_stream('generator-wgrad-block', device) if fork else None
        self.collecting, self.queue, self.later, self.pset = fork, [], [], pset

    def add(self, run):
        self.queue.append(run)

    def before_next_block(self, run):
        """`run` writes an operand that only weight gradients of the block AFTER the next launch read: it heads that block's queue (off the critical path of the
        backward, in front of its readers on their stream) -- or runs now where this backward does not fork."""
        if self.collecting:
            self.later.append(run)
        else:
            run()

    def launch(self, keep_collecting=False):
        # (several side streams with the launches dealt round-robin, HV_G_WGRAD_STREAMS 2 / 3, measured slower in round 5: 6.94 -> 6.98-7.36 ms)
        if self.side is None:
            return
        self.side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self.side):
            for run in self.queue:
                run()
            self.pset.fold_chain().flush()      # the side stream's last slab fold, on that stream (before the join)
        self.queue, self.later, self.collecting = self.later, [], keep_collecting

    def join(self):
        assert not self.queue and not self.later, 'WgradBlock.join(): queued weight gradients were never launched'
        if self.side is not None:
            torch.cuda.current_stream().wait_stream(self.side)
        self.side, self.collecting = None, False


def _wgrad(node, p, xin, gfull, accumulate, prec, dbias=None, dbias_accumulate=False):
    # the split-K slab fold of this weight gradient rides in the NEXT weight gradient of the network on this stream (ops.FoldChain; the last one is
    # launched by ParamSet.finish_backward / the owner of a side stream) -- round 4's 62 fold launches per step were each a dependent 5-us node
    chain = p.owner.fold_chain() if p.owner is not None else None
    if node.transposed:
        # y = conv_transpose(x): the weight gradient is that of a strided conv with the roles of x and g swapped;
        # the result is laid out [cin][taps][coutP] (hv_weight_prep_backward knows, transposed_src)
        ops.conv2d_wgrad(gfull, xin, p.dw, node.k, node.s, node.pad, node.d, accumulate=accumulate, precision=prec, chain=chain)
    else:
        ops.conv2d_wgrad(xin, gfull, p.dw, node.k, node.s, node.pad, node.d, in_shift=node.shift, accumulate=accumulate, precision=prec,
                         dbias=dbias, dbias_accumulate=dbias_accumulate, chain=chain)


def conv_backward(node, book, prec, dbias_accumulate=False, wgrad_accumulate=False, wgrad=True, x_wg=None, premultiplied=False,
                  mul_x=None, dbias_done=False, bn=None):
    """Backward of one ConvNode: activation gradient (+bias gradient), weight gradient, data gradient.
    x_wg: channel-padded copy of the input for the weight-gradient kernel (1-channel image inputs).
    premultiplied: the gradient buffer of node.y already holds the PRE-activation gradient (its only writer applied act').
    mul_x: activation name of the layer that produced node.x -- the data gradient is multiplied by act'(node.x) in the conv
    epilogue, so that layer's backward starts `premultiplied` (conv_backward_chain).
    bn: (Act raw input of the batch normalisation that produced node.x, its stats, groups, partials) -- the normalisation's backward sums leave
    this data gradient's epilogue (ops.ConvCall bn=; the caller asked node.dx_call(...).bstats_parts() first)."""
    p = node.p
    # the batch-norm sums ride in the plain data gradient only: a caller that set them up for a transposed / pooled / shifted node would skip its reduction
    # pass and read partials nobody wrote
    assert bn is None or (node.need_dx and not node.transposed and node.pool_to is None and not node.shift), 'conv_backward: bn= needs the plain data-gradient branch'
    gy = book.twin(node.y)
    want_dbias = p.bias is not None and node.use_bias and wgrad and not dbias_done      # dbias_done: the caller's seed pass already summed it
    # the bias gradient (column sums of the activation gradient) rides in the weight-gradient kernels, which stream g anyway;
    # conv_transpose nodes (roles of x and g swapped there) and unpadded channel counts keep the stand-alone reduction
    fuse_dbias = want_dbias and not node.transposed and p.coutP == p.cout
    if (node.act != 'none' and not premultiplied) or (want_dbias and not fuse_dbias):
        ops.act_backward(gy, node.y, 'none' if premultiplied else node.act, dbias=p.bias.grad if (want_dbias and not fuse_dbias) else None, dbias_accumulate=dbias_accumulate)
    gfull = Act(gy.t, p.coutP, gy.coff)
    if wgrad:
        xs = node.x if x_wg is None else x_wg
        xin = Act(xs.t, p.cin_wg, xs.coff)
        # the weight gradient only feeds the optimiser: queue it on the side stream so that it overlaps the data-gradient
        # chain (joined by GradBook.join() before the gradients are finalised / the activations are overwritten)
        if book.wgrad_block.collecting:
            book.wgrad_block.add(lambda node=node, p=p, xin=xin, gfull=gfull, acc=wgrad_accumulate, db=p.bias.grad if fuse_dbias else None, dba=dbias_accumulate:
                                 _wgrad(node, p, xin, gfull, acc, prec, dbias=db, dbias_accumulate=dba))
        else:
            # (in line: per-layer forks to a side stream lost their A/B twice -- 8.25 -> 8.15 ms at the end of round 3, 7.36 -> 7.6-7.8 ms in round 4 -- and are gone;
            # the refinement generator's weight gradients go to a side stream as ONE block, see WgradBlock)
            _wgrad(node, p, xin, gfull, wgrad_accumulate, prec, dbias=p.bias.grad if fuse_dbias else None, dbias_accumulate=dbias_accumulate)
    if not node.need_dx:
        return
    # (pool_to / fused up-sampling: the gradient of the up-sampled tensor leaves 2x2 sum-pooled from the conv's own epilogue where the dispatch serves it --
    # no full-resolution gradient in memory, no hv_copy_channels mode 3 pass; the owner of pool_to, who asked the same memoised question, runs its producer
    # premultiplied)
    if node.transposed:
        form = 'src'
    elif node.pool_to is not None and node.pooled(book, prec, 'pool_to'):
        form = 'pool_to'
    elif node.shift:
        form = 'pool' if node.pooled(book, prec, 'pool', mul_x) else 'full'
    else:
        form = 'plain'
    if form == 'full':
        assert not mul_x
        full = node.full_scratch()
        node.dx_call(book, prec, 'full', full, False).launch()
        gx = node.dx_view(book, 'plain')
        ops.copy_channels(full, gx, mode=3, accumulate=book.mark(gx))
    else:
        dst = node.dx_view(book, form)
        node.dx_call(book, prec, form, dst, book.mark(dst), mul_x=mul_x, bn=bn).launch()


# independent generator branches on two HIP streams / graph branches
#   (step-level A/B under graph replay, three pairs in one call: 14.80 / 14.81 / 14.85 ms on vs 15.01 / 14.96 / 15.05 ms off)
_branch_streams = {}


def branch_stream():
    """Side stream for an independent branch of the generator (None when everything must stay on one stream).  Weight gradients
    issued on it stay in line (no nested fork: see NO_FORK_STREAMS)."""
    if SERIAL:
        return None
    cur = torch.cuda.current_stream()
    if cur.cuda_stream in NO_FORK_STREAMS:
        return None
    key = cur.device.index
    st = _branch_streams.get(key)
    if st is None:
        st = _branch_streams[key] = named_stream('generator-branch', cur.device)
        NO_FORK_STREAMS.add(st.cuda_stream)
    return st


def chain_link(n, nxt, book, prec):
    """True when n's data gradient can carry act' of nxt (the producer of n.x): see conv_backward_chain.  A node with fused up-sampling links when
    its data gradient can leave pooled (conv_backward)."""
    if not (nxt is not None and n.need_dx and not n.transposed and nxt.act != 'none'
            and n.x.t is nxt.y.t and n.x.coff == nxt.y.coff and n.p.cin_fwd <= nxt.y.t.shape[-1] - nxt.y.coff):
        return False
    return not n.shift or n.pooled(book, prec, 'pool', nxt.act)


def conv_backward_chain(nodes, book, prec, premultiplied_first=False, stop_before=None):
    """Backward of a PURE chain of ConvNodes given in backward order: nodes[i].x is exactly the output buffer of nodes[i+1] and
    nothing else reads or writes that buffer's gradient.  Inside the chain the data gradient of nodes[i] is multiplied by
    act'(output of nodes[i+1]) in its conv epilogue, so nodes[i+1] starts from its pre-activation gradient: the in-place
    act-gradient pass (read g, read y, write g) between two convs disappears.
    stop_before: the node that follows nodes[-1] in the chain but is run by the caller later (with
    premultiplied=chain_link(nodes[-1], stop_before, book, prec))."""
    pre = premultiplied_first     # every writer of nodes[0]'s output gradient already applied its act'
    for i, n in enumerate(nodes):
        nxt = nodes[i + 1] if i + 1 < len(nodes) else stop_before
        link = chain_link(n, nxt, book, prec)
        conv_backward(n, book, prec, premultiplied=pre, mul_x=nxt.act if link else None)
        pre = link


# ================================================================================================ contextual attention
CA_GRAM = True     # GEMM route: matching scores and their gradient on the pixel Gram matrix (csrc/attention_gram.hip); False: the patch-table GEMMs (a test's reference)
CA_GEMM = True     # fp16 mode: the attention block's five contractions as batched NT GEMMs (csrc/bgemm.hip); False: the conv kernels (a test's reference)


def _bgemm(A, B, C, M, N, K, batch, alpha=1.0, colscale=None, b_split=0):
    """C[b] = alpha * colscale[b] (.) A[b] @ B[b]^T over contiguous per-sample matrices A [batch][M][K], B [batch][N][K] (fp32 or fp16),
    C [batch][M][N] fp32 (or fp16: hv_bgemm_nt_h); b_split: B's rows taken in (outer, inner = b_split) order (hv_bgemm_nt)."""
    _lib.get().call('hv_bgemm_nt_h' if C.dtype == torch.float16 else 'hv_bgemm_nt', ptr(A), int(A.dtype == torch.float16), K, ctypes.c_longlong(M * K), ptr(B), int(B.dtype == torch.float16), K,
                    ctypes.c_longlong(N * K), ptr(C), N, ctypes.c_longlong(M * N), M, N, K, batch, ctypes.c_float(alpha), ptr(colscale),
                    ctypes.c_longlong(N if colscale is not None else 0), int(b_split), stream())


def attention_route(prec, f, C, h, w):
    """Route of one AttentionPlan.forward over the map `f`: 'conv' (exact fp32: the contractions as per-sample-filter convolutions), 'gemm' (fp16: batched GEMMs, the scores on the
    3x3 patch tables) or, where its kernels serve the shape, 'gram' (... the scores on the pixel Gram matrix).  The flags are read at the call."""
    if not (CA_GEMM and ops.precision_id(prec) == ops.F16 and (9 * C) % 32 == 0 and (h * w) % 32 == 0 and C % 4 == 0):
        return 'conv'
    return 'gram' if CA_GRAM and f.f16 and C == 64 and w in (32, 64) and f.ld % 8 == 0 and f.coff == 0 else 'gemm'


# The tables each route alone reads, per pass, and the score-side ones every route shares.  f32 / out32 / dout32 / df32: fp32 copies of boundary maps, held where the map is stored as
# fp16 (the GEMM routes' boundary kernels read / write such maps themselves).  Tables that are only GEMM operands are fp16, written so by their producers (wp_h beside the fp32 wp, A_h).
CA_TABLES = dict(conv=dict(forward='fd wp wpT raw rawT A f32 out32', backward='AT dOrawT dwp dout32 df32'),
                 gemm=dict(forward='fd wp wp_h raw_h rawT_h A_h O', backward='wpT_h dwp dOraw_h dOrawT_h AT_h df32'),
                 gram=dict(forward='fd_h fdT_h q raw_h rawT_h A_h O', backward='dOraw_h dOrawT_h AT_h df32'),
                 shared=dict(forward='S0 S1 norm rnorm mm argmax', per_sample='mm_b', backward='dA dS1 dS0 Gs coef'))


class AttentionPlan:
    """ContextualAttention(ksize=3, stride=1, rate=2, fuse_k=3, softmax_scale=10, fuse=True) on an NHWC feature map (reference models/inpaint_networks.py:235-410).
    forward / backward are one skeleton around the steps of the call's route (`steps`); a plan that has served two routes holds two sets of tables that share nothing."""

    def __init__(self, B, H, W, C, device, img_hw, scale=10.0, fuse=True):
        self.B, self.H, self.W, self.C, self.dims, self.device = B, H, W, C, (B, H, W, C), device
        self.h, self.w, self.L = h, w, L = H // 2, W // 2, (H // 2) * (W // 2)
        assert h == w and H % 2 == 0, "contextual attention expects a square, even-sized feature map"
        self.img_hw, self.scale, self.fuse = img_hw, scale, fuse
        self.fused_adjoint = fuse and h == 32 and w == 32      # hv_ca_fuse_backward_prep: one pass, the plain scores' gradient (dS0) stays on chip
        self.unused = set() if fuse and not self.fused_adjoint else {'dS0'} if fuse else {'S1', 'dS0'}      # shared tables this plan never reads
        f32, f16 = torch.float32, torch.float16      # name -> dtype, shape (four-dimensional: held as an Act) of every table a plan may hold
        LL, fmap, vec, tab, tabT = (f32, (B, h, w, L)), (f32, (B, H, W, C)), (f32, (B, L)), (f16, (B, L, 16 * C)), (f16, (B, 16 * C, L))
        self.spec = dict(S0=LL, S1=LL, dS0=LL, A=LL, AT=LL, dA=LL, dS1=LL, Gs=LL, f32=fmap, out32=fmap, dout32=fmap, df32=fmap, norm=vec, rnorm=vec, q=vec, mm_b=vec, mm=(f32, (L,)),
                         argmax=(torch.int32, (B * L,)), coef=(f32, (33 * B, L)), fd=(f32, (B, h, w, C)), dwp=(f32, (B, h, w, 9 * C)), wp=(f32, (B, L, 9 * C)), wpT=(f32, (B, 9 * C, L)),
                         raw=(f32, (B, L, 16 * C)), rawT=(f32, (B, C, 16 * L)), dOrawT=(f32, (B, C, 16 * L)), wp_h=(f16, (B, L, 9 * C)), wpT_h=(f16, (B, 9 * C, L)), raw_h=tab, rawT_h=tabT,
                         O=tab, dOraw_h=tab, dOrawT_h=tabT, A_h=(f16, (B, L, L)), AT_h=(f16, (B, L, L)), fd_h=(f16, (B, L, C)), fdT_h=(f16, (B, C, L)))
        # (route, name) -> every tensor the plan holds; route -> the namespace of that route's tables; route and (precision, per-sample mask) of the last completed forward
        self.owned, self.sets, self.route, self.last = {}, {}, None, None
        self.buffers('shared', 'forward')

    gemm = property(lambda self: self.route in ('gemm', 'gram'))
    gram = property(lambda self: self.route == 'gram')
    nbytes = lambda self: sum(t.numel() * t.element_size() for t in self.owned.values())      # device bytes of every tensor the plan owns now

    def buffers(self, route, stage, skip=()):
        """-> the holder of `route`'s tables ('shared': the plan itself) once those of `stage` are in it, bar `skip`: zeroed on first use and kept for the life of the plan."""
        r = self if route == 'shared' else self.sets.setdefault(route, types.SimpleNamespace())
        for n in CA_TABLES[route][stage].split():
            if (route, n) in self.owned or n in self.unused or n in skip:
                continue
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError('AttentionPlan%s: %s route, %s would allocate %s inside a stream capture -- run it eagerly once first' % (self.dims, route, stage, n))
            t = self.owned[route, n] = torch.zeros(*self.spec[n][1], dtype=self.spec[n][0], device=self.device)
            setattr(r, n, Act(t) if t.dim() == 4 else t)
        return r

    def forward(self, f, mask_img, out, prec, want_argmax=False, per_sample_mask=False):
        """f: Act [B,H,W,C] (foreground == background), mask_img: (B,1,Himg,Wimg) tensor, out: Act [B,H,W,C].  per_sample_mask: every sample's own mask decides its valid patches --
        the batch stands for B independent batch-1 calls (the reference's inference loop); False = the reference's batched behaviour (sample 0's mask for all, inpaint_networks.py:314)."""
        route, self.route, self.last = attention_route(prec, f, self.C, self.h, self.w), None, None      # (recorded once every launch is out: a forward that raises leaves no backward)
        L_, B, L, (patches, scores, paste) = _lib.get(), self.B, self.L, self.steps[route][:3]
        r = self.buffers(route, 'forward', skip=[n for n, a in (('f32', f), ('out32', out)) if not a.f16])
        mm, mm_stride = (self.buffers('shared', 'per_sample').mm_b, L) if per_sample_mask else (self.mm, 0)
        patches(self, r, f)
        mask = ('hv_ca_mask_batched', ptr(mask_img), B, ctypes.c_longlong(self.img_hw[0] * self.img_hw[1])) if per_sample_mask else ('hv_ca_mask', ptr(mask_img))
        L_.call(*mask, *self.img_hw, self.h, self.w, ptr(mm), stream())
        scores(self, r, prec)
        if self.fuse:
            L_.call('hv_ca_fuse', ptr(self.S0.t), ptr(self.S1.t), B, self.h, self.w, 0, stream())
        s = self.S1 if self.fuse else self.S0      # (the score matrices stay fp32 on every route: they feed a x10 soft-max)
        if route != 'conv':
            L_.call('hv_ca_softmax_f16', ptr(s.t), ptr(mm), ctypes.c_longlong(mm_stride), ptr(r.A_h), B, L, ctypes.c_float(self.scale), ptr(self.argmax) if want_argmax else None, stream())
        elif per_sample_mask:
            L_.call('hv_ca_softmax_batched', ptr(s.t), ptr(mm), ctypes.c_longlong(mm_stride), ptr(r.A.t), B, L, ctypes.c_float(self.scale), ptr(self.argmax) if want_argmax else None, stream())
        else:
            L_.call('hv_ca_softmax', ptr(s.t), ptr(mm), ptr(r.A.t), B, L, ctypes.c_float(self.scale), ptr(self.argmax) if want_argmax else None, stream())
        paste(self, r, out, prec)
        self.route, self.last = route, (ops.precision_id(prec), per_sample_mask)

    def backward(self, dout, df, accumulate, prec):
        """dout: Act grad of the output; df: Act grad of the input feature map (assigned or accumulated).  Runs on the route and the tables of the forward
        before it; refused (nothing launched) without one, in another precision than its, or after a per-sample-mask forward (the soft-max gradient reads mm)."""
        if self.route is None or self.last != (ops.precision_id(prec), False):
            raise RuntimeError('AttentionPlan%s: backward(prec=%s) does not follow the last forward: route %s, (precision, per-sample mask) %s' % (self.dims, prec, self.route, self.last))
        L_, B, L, (paste_grad, score_grad) = _lib.get(), self.B, self.L, self.steps[self.route][3:]
        r = self.buffers(self.route, 'backward', skip=[n for n, a in (('dout32', dout), ('df32', df)) if not a.f16])
        self.buffers('shared', 'backward')
        df_user, df = df, r.df32 if df.f16 else df      # (two kernels add into df: it stays fp32 until both are in, one rounding)
        paste_grad(self, r, dout, df, accumulate and df is df_user, prec)
        name, A = ('hv_ca_softmax_backward', r.A.t) if self.route == 'conv' else ('hv_ca_softmax_backward_f16', r.A_h)
        L_.call(name, ptr(self.dA.t), ptr(A), ptr(self.mm), ptr(self.dS1.t), B, L, ctypes.c_float(self.scale), stream())
        if self.fused_adjoint:
            L_.call('hv_ca_fuse_backward_prep', ptr(self.dS1.t), ptr(self.S0.t), ptr(self.norm), ptr(self.rnorm), ptr(self.Gs.t), ptr(self.coef), B, self.h, self.w, stream())
        else:
            if self.fuse:
                L_.call('hv_ca_fuse', ptr(self.dS1.t), ptr(self.dS0.t), B, self.h, self.w, 1, stream())
            L_.call('hv_ca_score_backward_prep', ptr((self.dS0 if self.fuse else self.dS1).t), ptr(self.S0.t), ptr(self.norm), ptr(self.rnorm), ptr(self.Gs.t), ptr(self.coef), B, L, stream())
        score_grad(self, r, df, prec)
        if df is not df_user:
            ops.copy_channels(df, df_user, mode=0, accumulate=bool(accumulate))

    # ---- the routes' own steps over r, the route's tables (the plan's are the shared ones): patches, scores, paste | paste_grad (dA and d(raw patches)), score_grad
    def _conv_patches(self, r, f):
        if f.f16:
            ops.copy_channels(f, r.f32, mode=0)
            f = r.f32
        _lib.get().call('hv_ca_patches', ptr(f.t), f.f16, *self.dims, f.ld, ptr(r.fd.t), ptr(r.wp), ptr(r.wpT), ptr(self.norm), ptr(self.rnorm), stream())
        _lib.get().call('hv_ca_raw_patches', ptr(f.t), *self.dims, f.ld, ptr(r.raw), ptr(r.rawT), stream())

    def _conv_scores(self, r, prec):
        ops.conv2d(r.fd, r.wp, self.S0, 3, 1, 1, 1, w_bstride=self.L * 9 * self.C, ch_scale=self.rnorm, ch_scale_bstride=self.L, precision=prec)

    def _conv_paste(self, r, out, prec):
        ops.conv2d(r.A, r.rawT, r.out32 if out.f16 else out, 4, 2, 1, 1, transposed=True, alpha=0.25, w_bstride=self.C * 16 * self.L, precision=prec)
        if out.f16:
            ops.copy_channels(r.out32, out, mode=0)

    def _conv_paste_grad(self, r, dout, df, accumulate, prec):
        if dout.f16:
            ops.copy_channels(dout, r.dout32, mode=0)
            dout = r.dout32
        ops.conv2d(dout, r.raw, self.dA, 4, 2, 1, 1, alpha=0.25, w_bstride=self.L * 16 * self.C, precision=prec)
        _lib.get().call('hv_transpose_batched', ptr(r.A.t), ptr(r.AT.t), self.B, self.L, self.L, stream())
        _lib.get().call('hv_ca_raw_patches', ptr(dout.t), *self.dims, dout.ld, None, ptr(r.dOrawT), stream())
        ops.conv2d(r.AT, r.dOrawT, df, 4, 2, 1, 1, transposed=True, alpha=0.25, w_bstride=self.C * 16 * self.L, accumulate=int(accumulate), precision=prec)

    def _conv_score_grad(self, r, df, prec):      # through the normalised patch matching (patches act as both filters and inputs)
        ops.conv2d(self.Gs, r.wpT, r.dwp, 1, 1, 0, 1, w_bstride=9 * self.C * self.L, precision=prec)
        _lib.get().call('hv_ca_patches_backward', ptr(r.dwp.t), ptr(r.wp), ptr(self.coef), ptr(df.t), *self.dims, df.ld, 1, stream())

    def _gemm_patches(self, r, f):
        _lib.get().call('hv_ca_patches_h', ptr(f.t), f.f16, *self.dims, f.ld, ptr(r.fd.t), ptr(r.wp), ptr(r.wp_h), ptr(self.norm), ptr(self.rnorm), stream())
        _lib.get().call('hv_ca_raw_patches_f16', ptr(f.t), f.f16, *self.dims, f.ld, ptr(r.raw_h), ptr(r.rawT_h), stream())

    def _gemm_scores(self, r, prec):      # the 3x3 patches of the (zero-padded) map are both the conv's input columns and its filters: scores = rnorm (.) wp wp^T
        _bgemm(r.wp_h, r.wp_h, self.S0.t, self.L, self.L, 9 * self.C, self.B, colscale=self.rnorm)

    def _gemm_paste(self, r, out, prec):      # paste = (A rawT^T) folded: O[p][(c, tap)], then every output pixel sums the 4 taps that reach it
        _bgemm(r.A_h, r.rawT_h, r.O, self.L, 16 * self.C, self.L, self.B, b_split=self.C)          # rows of rawT [c][tap] taken as (tap, c): O[p][tap][c]
        _lib.get().call('hv_ca_fold_h', ptr(r.O), ptr(out.t), out.f16, *self.dims, out.ld, ctypes.c_float(0.25), 0, stream())

    def _gemm_paste_grad(self, r, dout, df, accumulate, prec):
        _lib.get().call('hv_ca_raw_patches_f16', ptr(dout.t), dout.f16, *self.dims, dout.ld, ptr(r.dOraw_h), ptr(r.dOrawT_h), stream())
        _bgemm(r.dOraw_h, r.raw_h, self.dA.t, self.L, self.L, 16 * self.C, self.B, alpha=0.25)
        _lib.get().call('hv_transpose_batched_h2h', ptr(r.A_h), ptr(r.AT_h), self.B, self.L, self.L, stream())
        _bgemm(r.AT_h, r.dOrawT_h, r.O, self.L, 16 * self.C, self.L, self.B, b_split=self.C)      # d(raw patches)[l][tap][c] (the forward's O buffer is free by now)
        _lib.get().call('hv_ca_fold_h', ptr(r.O), ptr(df.t), df.f16, *self.dims, df.ld, ctypes.c_float(0.25), int(bool(accumulate)), stream())

    def _gemm_score_grad(self, r, df, prec):
        _lib.get().call('hv_transpose_batched_f16', ptr(r.wp), ptr(r.wpT_h), self.B, self.L, 9 * self.C, stream())      # (the transpose of wp has this one reader)
        _bgemm(self.Gs.t, r.wpT_h, r.dwp.t, self.L, 9 * self.C, self.L, self.B)
        _lib.get().call('hv_ca_patches_backward', ptr(r.dwp.t), ptr(r.wp), ptr(self.coef), ptr(df.t), *self.dims, df.ld, 1, stream())

    def _gram_patches(self, r, f):
        _lib.get().call('hv_ca_gram_down', ptr(f.t), f.f16, *self.dims, f.ld, ptr(r.fd_h), ptr(r.fdT_h), ptr(r.q), stream())
        _lib.get().call('hv_ca_raw_patches_f16', ptr(f.t), f.f16, *self.dims, f.ld, ptr(r.raw_h), ptr(r.rawT_h), stream())

    def _gram_scores(self, r, prec):
        _lib.get().call('hv_ca_gram_scores', ptr(r.fd_h), ptr(r.q), self.B, self.h, self.w, self.C, ptr(self.S0.t), ptr(self.norm), ptr(self.rnorm), stream())

    def _gram_score_grad(self, r, df, prec):      # d fd = box(Gs) fd + (3x3 sum of coef) fd, added to the even positions of df: one K = L product instead of the L x 9C GEMM + col2im
        _lib.get().call('hv_ca_gram_backward', ptr(self.Gs.t), ptr(r.fd_h), ptr(r.fdT_h), ptr(self.coef), self.B, self.h, self.w, self.C, ptr(df.t), df.ld, stream())

    steps = dict(conv=(_conv_patches, _conv_scores, _conv_paste, _conv_paste_grad, _conv_score_grad), gemm=(_gemm_patches, _gemm_scores, _gemm_paste, _gemm_paste_grad, _gemm_score_grad),
                 gram=(_gram_patches, _gram_scores, _gemm_paste, _gemm_paste_grad, _gram_score_grad))
