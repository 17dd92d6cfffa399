"""How Pix2PixModel's train step is run: the per-batch-shape state (ShapeState) and the scheduler of the model's three phases (StepRunner)."""
import os
import warnings
from collections import namedtuple

import torch

from . import engine, ops


# inline: None, or the schedule ('captured' / 'overlapped') whose collectives are part of the phases' launch sequence
# through: the three phases are ONE capture, so each discriminator stream runs on from phase A into phase B without the join between them
StepMode = namedtuple('StepMode', 'inline through')
EAGER = StepMode(None, False)


class ShapeState:
    """What belongs to one batch shape and is found again when the shape comes back: the input buffers (the discriminators' 2B-sample `dcat{k}`
    pair buffers among them), the tensors a step binds as model attributes, the captured graphs and the count of eager steps taken."""
    __slots__ = ('inputs', 'bound', 'graphs', 'eager_steps', '_kept')

    def __init__(self):
        self.inputs, self.bound, self._kept = {}, {}, {}
        self.reset()

    def reset(self):      # new input addresses or another schedule: captured graphs are stale, and an eager warm-up (plans, tables) comes before the next capture
        self.graphs, self.eager_steps = None, 0

    def keep(self, tag):
        self._kept[tag] = (self.graphs, self.eager_steps)

    def take(self, tag):
        self.graphs, self.eager_steps = self._kept[tag]
        self._kept = {}          # (the graphs kept under other tags go)


class StepRunner:
    """Runs phases (a, b, c) -- callables taking a StepMode -- over `pairs`, the (network, optimiser) pairs of G, D_1, D_2, D_3 in that order.

    The step is device-only (no host reads, learning rate and Adam step count live on the device), so after GRAPH_WARMUP eager steps it is
    captured once per batch shape as a hipGraph and replayed: ~490 kernel launches per step become one graph launch, which removes the host
    launch latency that otherwise leaves the GPU idle between the short kernels of the backward passes.  HV_GRAPH=0 or an active kernel timer
    keeps the eager path.  The three phases are captured as ONE graph (7.81 -> 7.70 ms over four same-box pairs: two graph-launch boundaries
    less) -- except under the cut data-parallel schedule, which issues its collectives between the graphs.

    Data-parallel step schedule (one process per GPU); every collective of the step goes to one communicator on one stream in the order D_1, D_2, D_3, G:
      'captured' (RCCL only): the step as ONE hipGraph with the two collectives inside it, both on the main branch (ncclAllReduce, ncclAvg, ddp.RcclComm): the
          three discriminators' gradients -- one arena -- where their streams join, the generator's between its backward and its Adam step.  No graph
          cut, no host in the loop, no edge between branches, the order D, G on every rank by construction.
      'graphs': the step cut into its three graphs where the exchanges belong, the same collectives issued eagerly between them on the exchange stream
          (the main stream waits for each).  The fallback for runtimes that refuse to capture RCCL kernels, and the only schedule for gloo.
      'overlapped' (RCCL only): 'captured' with one collective per discriminator, issued the moment D_k's gradients are final and chained D_1 -> D_2 ->
          D_3 -> G by events (ddp.GradSync.reduce_branch): D_k's mean runs beside the other discriminators' passes, at the price of edges between the
          graph's branches (this runtime executes branch-crossing edges poorly: +0.3 ms in a one-rank group where 'captured' costs nothing).
      'auto' (default): gloo -> 'graphs'; RCCL -> dp_preflight() runs ALL on the job's first batch, checks that every rank ends with the same
          weights, keeps the fastest correct one and puts the weights back (the preflight steps are not training steps)."""
    GRAPH_WARMUP = 2     # eager steps before capture (lazy allocations, stream creation, weight tables)

    def __init__(self, phases, pairs, grad_sync, device, extra_state=()):
        self.phase_a, self.phase_b, self.phase_c = phases
        (self.nets, self.optimizers), self.grad_sync, self.device = zip(*pairs), grad_sync, device
        self.extra_state = list(extra_state)      # what a step writes besides networks and optimisers (the loss slots): dp_preflight() puts it back too
        self.use_graph, self.strict_graph = os.environ.get('HV_GRAPH', '1') != '0', False
        self.dp_schedule = os.environ.get('HV_DP_SCHEDULE', 'auto')
        if self.dp_schedule == 'phases':      # (the twelve-phase schedule of rounds 1-3 is gone; old launch scripts keep working)
            warnings.warn("HV_DP_SCHEDULE=phases is deprecated: taking 'graphs'", DeprecationWarning)
            self.dp_schedule = 'graphs'
        if self.dp_schedule not in ('auto', 'captured', 'overlapped', 'graphs'):
            raise ValueError("HV_DP_SCHEDULE must be 'auto', 'captured', 'overlapped' or 'graphs'")
        self.dp_preflight_record = self.dp_capture_error = self.d_streams = self._capture_stream = None
        self.inline = None          # the last step's StepMode.inline
        self._d_grad_arena = None      # when set, the three discriminators' flat gradients are its three slices (_home_d_grads)

    def sides(self, main):
        """The streams of D_1, D_2, D_3: their updates are independent of each other (kernels of different discriminators overlap on the 256 CUs)."""
        if self.d_streams is None:
            self.d_streams = [engine.named_stream('discriminator-%d' % k, self.device) for k in (1, 2, 3)]
            engine.NO_FORK_STREAMS.update(st.cuda_stream for st in self.d_streams)
        return [main] * 3 if engine.SERIAL else self.d_streams

    def join(self, main):
        if not engine.SERIAL:
            for side in self.d_streams:
                main.wait_stream(side)

    def _a(self, mode):
        if mode.inline:
            self.grad_sync.chain_reset()      # the step's collectives form one chain D_1 -> D_2 -> D_3 -> G (ddp.GradSync.reduce_branch)
        self.phase_a(mode)                    # ('overlapped': D_k's collective is issued inside, on D_k's stream)
        if mode.inline == 'captured':         # the three discriminators' gradients as ONE collective where their streams join
            for f in self._d_flats():
                self.grad_sync.reduce_branch(f)

    def _b(self, mode):
        self.phase_b(mode)
        if mode.inline:
            self.grad_sync.reduce_branch(self.nets[0].paramset().flat_grad)

    def step(self, state, strict=False):
        """One train step on the batch in `state`.  strict: a refused capture of the step with its collectives is raised (the preflight records
        it) instead of falling back to 'graphs'."""
        if self.dp_schedule == 'auto':      # -> a schedule, once, at the first step
            if not self.grad_sync.active():      # (single process: nothing to choose)
                self.dp_schedule = 'graphs'
            elif os.environ.get('HV_DP_PREFLIGHT', '1') == '0':
                self.dp_schedule = 'captured' if self.grad_sync.capturable() else 'graphs'
            else:      # (gloo cannot be captured: 'graphs' only -- the preflight then still proves that every rank ends with the same weights and records the time)
                self.dp_preflight(state, schedules=('graphs', 'captured', 'overlapped') if self.grad_sync.capturable() else ('graphs',))
        # after the first eager step for this batch shape every convolution of the four networks has been dispatched once: from then on the weight
        # layout passes write only the tables those kernels read (engine.lean_tables)
        with engine.lean_tables(state.eager_steps >= 1):
            for o in self.optimizers:
                o.sync_lr()
            graphable = self.use_graph and ops.timer() is None
            dp = self.grad_sync.active()
            self.inline = self.dp_schedule if dp and self.dp_schedule in ('captured', 'overlapped') and self.grad_sync.capturable() else None
            mode = StepMode(self.inline, False)
            cut = dp and not self.inline            # the means sit BETWEEN the step's graphs (exchange stream, issued eagerly)
            parts = ((self._a,), (self._b,), (self.phase_c,)) if cut else ((self._a, self._b, self.phase_c),)
            if dp and state.eager_steps == 0 and state.graphs is None:
                self._home_d_grads()      # (both schedules: a preflight runs them over the same gradient storage, and captured graphs keep its addresses)
            if graphable and state.graphs is None and state.eager_steps >= self.GRAPH_WARMUP:
                try:
                    # in one graph D_k goes from its backward straight on to its Adam step and its pass for the generator on its own stream -- no join of the
                    # three discriminator streams between the phases (that join only exists for the exchange that follows phase A): a discriminator that is
                    # done early (D_3 reads the 128 x 128 crop) does not wait for the others
                    state.graphs = self._capture(parts, mode._replace(through=not cut and not engine.SERIAL and self.inline != 'captured'))
                except RuntimeError as e:
                    if self.inline and strict:
                        raise
                    if self.inline:
                        # a runtime that refuses to capture the collectives: keep the step, cut it at the exchanges instead (they are then issued eagerly)
                        warnings.warn('hipGraph capture of the step with its RCCL collectives failed (%s); falling back to HV_DP_SCHEDULE=graphs' % str(e).splitlines()[0])
                        torch.cuda.synchronize(self.device)
                        self.dp_schedule = 'graphs'
                        state.reset()
                        self.dp_capture_error = str(e).splitlines()[0]
                        return self.step(state)
                    # capture refused by the runtime: keep launching eagerly and say so once -- unless the caller asked for a hard failure (bench.py: a
                    # number labelled 'hipGraph replay' must never come from eager launches)
                    if self.strict_graph:
                        raise RuntimeError('hipGraph capture of the train step failed: %s' % str(e).splitlines()[0]) from e
                    warnings.warn('hipGraph capture of the train step failed (%s); continuing with eager launches' % str(e).splitlines()[0])
                    torch.cuda.synchronize(self.device)
                    self.use_graph = graphable = False
            replay = graphable and state.graphs is not None
            for i, part in enumerate(parts):
                if replay:
                    state.graphs[i].replay()
                else:
                    for phase in part:
                        phase(mode)
                if cut and i < 2:      # D's means after phase A, G's after phase B
                    self._exchange([self.nets[0].paramset().flat_grad] if i else self._d_flats())
            if not replay:
                state.eager_steps += 1

    def _capture(self, parts, mode):
        if self._capture_stream is None:
            self._capture_stream = engine.named_stream('capture', self.device)
        torch.cuda.synchronize(self.device)
        if self.grad_sync.active() and self.grad_sync.capturable():
            # torch's ProcessGroupNCCL retires finished collectives from its watchdog thread (a poll every 100 ms) by querying their events.  On this stack a
            # query that lands while ANY stream of the process is capturing can fail with hipErrorCapturedEvent ("operation not permitted on an event last
            # recorded in a capturing stream" -- torch draws its collective stream from the same pool of 32 streams per device as the step's streams), and
            # the watchdog then aborts the process: seen once in ~20 runs of the one-rank RCCL test, a few ms after the warm-up steps' collectives (weight
            # broadcast, the communicator's id exchange, the cut schedule's means).  The device is idle here: give the watchdog time for three polls so
            # that nothing is left for it to query during the capture.  Once per batch shape.
            import time
            time.sleep(float(os.environ.get('HV_DP_CAPTURE_SETTLE_MS', '350')) * 1e-3)
        graphs, pool = [], None
        for part in parts:
            g = torch.cuda.CUDAGraph()
            # thread_local: a process-group watchdog thread polling its events must not invalidate the capture
            with torch.cuda.graph(g, pool=pool, stream=self._capture_stream, capture_error_mode='thread_local'):
                for phase in part:
                    phase(mode)
            pool = g.pool()
            graphs.append(g)
        return tuple(graphs)

    def _home_d_grads(self):
        """The three discriminators' flat gradient buffers as three consecutive slices of ONE buffer (ParamSet.grad_home, taken up when a set next lays
        out its tables: the discriminator passes of the step that follows), so that their means are one collective."""
        if self._d_grad_arena is not None:
            return
        sets = [net.paramset() for net in self.nets[1:]]
        sizes = [sum(p.numel() for p in ps.trainable()) for ps in sets]
        rup = lambda n: (n + 63) // 64 * 64          # every slice starts on a 256-byte boundary (the guarded Adam's vector loads); the gaps stay zero
        self._d_grad_arena = torch.zeros(sum(rup(n) for n in sizes), dtype=torch.float32, device=self.device)
        off = 0
        for ps, n in zip(sets, sizes):
            ps.grad_home = self._d_grad_arena[off:off + n]
            ps._key = None          # lay the tables out again over the new gradient storage at the next prep
            for t in list(ps.t_prep.values()) + list(ps.t_bwd.values()):
                t.key = None        # (their rows hold pointers into the gradient storage)
            off += rup(n)

    def _d_flats(self):      # what a mean over the discriminators' gradients covers: the arena (the three buffers and the zero gaps between them) as ONE collective
        return [self._d_grad_arena] if self._d_grad_arena is not None else [net.paramset().flat_grad for net in self.nets[1:]]

    def _exchange(self, flats):
        """Cut schedule: mean over the ranks of flat gradients (one all-reduce each, issued back to back on the exchange stream); the current
        stream continues when all of them are done.  Nothing blocks the host."""
        main = torch.cuda.current_stream(self.device)
        for ev in [self.grad_sync.reduce(f, after=main) for f in flats]:
            if ev is not None:
                main.wait_event(ev)

    def _dp_state(self):
        """Every tensor a train step changes besides the activations: the four networks' parameters and buffers (BatchNorm running statistics,
        spectral-norm vectors), the optimisers' moments / step counts / overflow counters, the loss slots."""
        ts = []
        for net in self.nets:
            ts += [p.data for p in net.parameters()] + list(net.buffers())
        for o in self.optimizers:
            o._ensure_state()
            ts += [o._m, o._v, o._step]
        return ts + self.extra_state

    def _dp_weight_checksum(self):
        """Order-independent, exact checksum of all four networks' weights: the int64 sum of their fp32 bit patterns."""
        tot = torch.zeros((), dtype=torch.int64, device=self.device)
        for net in self.nets:
            for p in net.parameters():
                tot += p.data.view(torch.int32).to(torch.int64).sum()
        return tot

    def dp_preflight(self, state, timed_steps=5, schedules=('graphs', 'captured', 'overlapped')):
        """Pick the data-parallel schedule on THIS job, on the batch the model's set_input() just delivered into `state`, before the first training step.

        Each schedule is run from the same weights: the eager warm-up, the capture, two replays, then `timed_steps` replays between barriers.  After each the ranks compare
        (a) that the schedule ran on every rank, (b) an exact checksum of all weights (MIN == MAX over the ranks: the collectives delivered the same
        mean to every rank, in the same order), (c) the slowest rank's time.  The faster schedule that passed is kept -- with its captured graphs --
        and every tensor the steps touched (weights, running statistics, Adam state) is put back: preflight steps are not training steps.
        A schedule that raises, diverges across the ranks or is refused by the runtime is recorded and dropped; if none is left the job stops with
        the recorded text.  A rank that never comes back from a collective cannot be recovered in-process: a timer (HV_DP_PREFLIGHT_TIMEOUT_S,
        default 300 s) then ends THIS process with the text on stderr and exit code 3 instead of hanging the launcher (never a re-exec: the
        process has touched the GPU; a retry is a fresh job)."""
        import sys
        import threading
        import time
        import torch.distributed as dist
        world = dist.get_world_size()
        rec = {'world_size': world, 'timed_steps': timed_steps, 'schedules': {}, 'chosen': None}
        self.dp_preflight_record = rec
        limit = float(os.environ.get('HV_DP_PREFLIGHT_TIMEOUT_S', '300'))
        where = {'at': 'start'}

        def expired():
            sys.stderr.write('healthivert-gan_amd: data-parallel preflight did not finish within %.0f s (rank %d, in %s): a rank is stuck in a collective; '
                             'giving up (exit 3).  Record so far: %r\n' % (limit, dist.get_rank(), where['at'], rec))
            sys.stderr.flush()
            os._exit(3)
        timer = threading.Timer(limit, expired)
        timer.daemon = True
        timer.start()
        self._home_d_grads()
        for net in self.nets:      # (gradient storage and tables in place before the snapshot)
            net.paramset()._ensure(self.device)
        tensors = self._dp_state()
        snap = [t.clone() for t in tensors]
        try:
            for sched in schedules:      # (the plain one first: its captured graphs are kept whatever the later trials do)
                where['at'] = sched
                r = {'ok': False, 'error': None, 'ms_per_step': None, 'weights_identical_across_ranks': None}
                rec['schedules'][sched] = r
                self.dp_schedule = sched
                state.reset()
                self.dp_capture_error = None
                ok, dt = 1.0, float('inf')
                try:
                    for _ in range(1 + self.GRAPH_WARMUP + 2):      # (step() takes the first one after a reset with full weight tables, the rest with lean ones)
                        self.step(state, strict=True)
                    if self.use_graph and state.graphs is None:
                        raise RuntimeError('the step was not captured')
                    torch.cuda.synchronize(self.device)
                    dist.barrier()
                    torch.cuda.synchronize(self.device)
                    t0 = time.perf_counter()
                    for _ in range(timed_steps):
                        self.step(state, strict=True)
                    torch.cuda.synchronize(self.device)
                    dt = (time.perf_counter() - t0) / timed_steps
                except Exception as e:      # noqa: BLE001 -- recorded; the other schedule may still serve
                    ok, r['error'] = 0.0, '%s: %s' % (type(e).__name__, (str(e).splitlines() or ['?'])[0])
                    torch.cuda.synchronize(self.device)
                # ---- what the other ranks saw (these small collectives run in every case, so that a failure on one rank cannot strand the others)
                agg = torch.tensor([ok, -dt if ok else 0.0], dtype=torch.float64, device=self.device)
                dist.all_reduce(agg, op=dist.ReduceOp.MIN)
                ck = self._dp_weight_checksum()
                ck2 = torch.stack([ck, -ck])
                dist.all_reduce(ck2, op=dist.ReduceOp.MIN)
                torch.cuda.synchronize(self.device)
                all_ok = float(agg[0].item()) == 1.0
                same = int(ck2[0].item()) == -int(ck2[1].item())
                r['weights_identical_across_ranks'] = same
                if all_ok:
                    r['ms_per_step'] = round(-float(agg[1].item()) * 1e3, 3)
                elif r['error'] is None:
                    r['error'] = 'failed on another rank'
                r['ok'] = bool(all_ok and same)
                if r['ok']:
                    state.keep(sched)
                for t, c in zip(tensors, snap):      # the same starting point for the next schedule, and for training
                    t.copy_(c)
                for net in self.nets[1:]:      # the discriminators' prepared tables belong to the weights just overwritten, and the captured steps (rightly) no longer lay
                    ps = net.paramset()            # them out before the discriminator update: once, here, from the restored weights
                    ps.weights_changed()
                    ps.prep(self.device, False)
                torch.cuda.synchronize(self.device)
        finally:
            timer.cancel()
        good = [k for k in schedules if rec['schedules'][k]['ok']]
        if not good:
            raise RuntimeError('data-parallel preflight: no schedule ran correctly on %d rank(s): %r' % (world, rec['schedules']))
        best = min(good, key=lambda k: rec['schedules'][k]['ms_per_step'])
        for pref in ('captured', 'overlapped'):      # (within a percent of the fastest: no graph cut / the collectives beside compute)
            if pref in good and rec['schedules'][pref]['ms_per_step'] <= 1.01 * rec['schedules'][best]['ms_per_step']:
                best = pref
        rec['chosen'] = best
        self.dp_schedule = best
        state.take(best)
        self.dp_capture_error = next((rec['schedules'][k]['error'] for k in ('captured', 'overlapped') if k in rec['schedules'] and rec['schedules'][k]['error']), None)
        if dist.get_rank() == 0:
            print('data-parallel preflight (%d rank(s)): %s -> %s' % (world, {k: (v['ms_per_step'], v['error']) for k, v in rec['schedules'].items()}, best), flush=True)
