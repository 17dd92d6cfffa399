"""The weight path of csrc/prep.hip against the fp64 references of tests/weight_ref.py (pinned by tests/test_weight_ref_cpu.py, which also measures that the
bounds used here catch subtly wrong kernels): hv_weight_prep2 / hv_weight_prep (spectral norm, the six kernel-layout tables and w_fwd_t2),
hv_weight_prep_backward, hv_adam_step and hv_adam_step_guarded.

The C entries are called through lib.get().call with ops.LayerTable descriptor arrays on hvtest.Guarded buffers: NaN around every buffer, NaN in every
output before the call (the padding rows of a fragment-ordered table hold the zeros the caller owes), intact() asserted after every call.  No element
is left out of a comparison.  u = 2^-24; every bound is computed from fp64 reference quantities, never from the kernel's output:

  exact outputs (bit for bit)   the W / sigma tables: fp32 division is correctly rounded and both sides divide the stored W by the STORED sigma read back
                                from the device; their fp16 roundings, the zero padding and the fragment order; dw_orig of a layer without spectral norm,
                                with and without accumulate (one fp32 add of stored values); the unscaled gradient (the multiplier is a power of two; 1
                                leaves every bit, -0 and denormals included); the guard's state words; p / m / v of a skipped step; u and v without
                                power iteration; a layer inside a mixed table against the same layer alone;
  dots and norms                the order-independent (n + 2) u sum |term_i| of a length-n fp32 dot, carried to first order (in double) through
                                v' = t / |t|, s = W v', u' = s / |s| and sigma = u' . s (weight_ref.spectral_norm_bounds); the second of two chained
                                power iterations also carries the bounds of the first one's u;
  exact-arithmetic inputs       multiples of 1/8 up to 1/2: every product and partial sum of sigma = u . (W v) (grid 1/512) and of the backward's
                                dot (grid 1/64) is exactly representable (the precondition sum |terms| x grid < 2^24 is asserted on the reference), so
                                the kernel must return the fp64 value's bits whatever its summation order;
  element-wise values           4 x (largest error of a plain fp32 CPU evaluation of the same formula) + 4u |ref|; the spectral-norm g adds the dot's
                                bound times |u v| / sigma on random inputs and nothing on the exact ones; Adam's p adds the device powf's share of
                                bc1 = 1 - beta1^step and bc2: P u beta^step / bc relative (half of it for sqrt(bc2)) times the update, P = 4 ASSUMED
                                (the ROCm install carries no math-accuracy table to read it from); chained Adam steps carry the previous step's
                                bounds of m, v and p through the update to first order.
The worst error / bound ratio of every family is printed at the end (pytest -s); the exact families report 0."""
import ctypes

import pytest
import torch

import weight_ref as WR
from test_norm_act_gpu import RATIOS, Check, print_ratios, same_bits

pytestmark = pytest.mark.gpu

NAN = float('nan')
T = lib = ops = L = None
TABLES = ('w_fwd', 'w_bwd', 'w_fwd_h', 'w_bwd_h', 'w_fwd_t', 'w_bwd_t', 'w_fwd_t2')


@pytest.fixture(scope='module', autouse=True)
def _env():
    global T, lib, ops, L
    import hvgan  # noqa: F401
    from hvgan import lib as _lib, ops as _ops
    import hvtest as _T
    T, lib, ops = _T, _lib, _ops
    L = _lib.get()
    yield
    print_ratios('weight.')


class Pool:
    """The guarded buffers of one call."""

    def __init__(self):
        self.all = []

    def put(self, data, dtype=None, offset=0):
        g = T.Guarded(tuple(data.shape), dtype or data.dtype, data=data, offset=offset)
        self.all.append(g)
        return g

    def out(self, shape, dtype=torch.float32):
        g = T.Guarded(shape, dtype)
        self.all.append(g)
        return g

    def intact(self):
        torch.cuda.synchronize()
        return all(g.intact() for g in self.all)


def table(struct, rows):
    t = ops.LayerTable(struct)
    t.update([{k: (v.t if isinstance(v, T.Guarded) else v) for k, v in r.items()} for r in rows], 1, T.dev())
    return t


def exact_le(ck, family, got, want, what):
    """Bit-exact family: records 0 or inf."""
    exact_flag(ck, family, same_bits(got, want), what)


def exact_flag(ck, family, ok, what):
    RATIOS.setdefault(family, 0.0)
    ck.le(family, torch.tensor(0.0 if ok else 1.0), torch.tensor(0.0), what)


def err(got, ref):
    return (got.double() - ref).abs()


# ---------------------------------------------------------------------------------------------------------------- hv_weight_prep2 / hv_weight_prep
class PrepLayer:
    """One hv_wprep_layer on guarded buffers.  keep: the tables handed to the kernel (the others are allocated all the same and must stay untouched)."""

    def __init__(self, pool, W, u, v, cout, cin, k, sn, pi, transposed=False, K2=0, keep=TABLES, sigma0=NAN):
        self.cout, self.cin, self.taps, self.sn, self.pi, self.transposed, self.K2, self.keep = cout, cin, k * k, sn, pi, transposed, K2, keep
        self.CinP = self.CinB = WR.rup(cin, 4)
        self.CoutF, self.CoutP = cout, WR.rup(cout, 4)
        self.W, self.u0, self.v0 = W.reshape(-1), u, v
        self.b = b = {'w_orig': pool.put(self.W), 'sigma': pool.put(torch.tensor([sigma0, 5.0, 5.0, 5.0]))}
        if sn:
            b['u'], b['v'] = pool.put(u), pool.put(v)
        shape = WR.weight_tables_ref(self.W, 1.0, cout, cin, self.taps, self.CinP, self.CoutF, self.CoutP, self.CinB, transposed, K2)
        for n in TABLES:
            if shape[n] is None:
                continue
            if n + '_real' in shape:      # fragment order: NaN where a real row lives, the caller's zeros in the padding rows
                b[n] = pool.put(torch.where(shape[n + '_real'], torch.tensor(NAN), torch.tensor(0.0)).half())
            else:
                b[n] = pool.out(shape[n].shape, shape[n].dtype)
        self.prefill = {n: b[n].cpu() for n in TABLES if n in b}

    def row(self):
        b = self.b
        r = dict(w_orig=b['w_orig'], u=b.get('u'), v=b.get('v'), sigma=b['sigma'], Cout=self.cout, Cin=self.cin, taps=self.taps, CinP=self.CinP, CoutF=self.CoutF,
                 CoutP=self.CoutP, CinB=self.CinB, sn=int(self.sn), power_iter=int(self.pi), transposed_src=int(self.transposed), K2=self.K2)
        r.update({n: (b[n] if n in self.keep else None) for n in TABLES if n in b})
        return r

    def check(self, ck, what, legacy=False):
        """sigma, u, v against the reference and its bounds; every table against weight_tables_ref of the stored sigma, bit for bit."""
        b = self.b
        ck.true(same_bits(b['w_orig'].cpu(), self.W), 'w_orig changed: ' + what)
        sg = b['sigma'].cpu()
        ck.true(same_bits(sg[1:], torch.tensor([5.0, 5.0, 5.0])), 'sigma[1..3] touched: ' + what)
        if self.sn:
            Wm = self.W.reshape(self.cout, -1)
            ref = WR.spectral_norm_ref(Wm, self.u0, self.v0, self.pi)
            bs, bu, bv = WR.spectral_norm_bounds(Wm, self.u0, self.v0, self.pi)
            ck.le('weight.sigma', err(sg[0], ref[0]), bs, what)
            if self.pi:
                ck.le('weight.sn_u', err(b['u'].cpu(), ref[1]), bu, what)
                ck.le('weight.sn_v', err(b['v'].cpu(), ref[2]), bv, what)
            else:
                ck.true(same_bits(b['u'].cpu(), self.u0) and same_bits(b['v'].cpu(), self.v0), 'u / v written without power_iter: ' + what)
        else:
            ck.true(sg[0].item() == 1.0, 'sigma of a plain layer is not 1.0: ' + what)
        want = WR.weight_tables_ref(self.W, sg[0].item(), self.cout, self.cin, self.taps, self.CinP, self.CoutF, self.CoutP, self.CinB, self.transposed, self.K2)
        for n in TABLES:
            if n not in b:
                continue
            got = b[n].cpu()
            if n not in self.keep or (legacy and n == 'w_fwd_t2'):
                ck.true(same_bits(got, self.prefill[n]), '%s not handed over but written: %s' % (n, what))
            else:
                exact_le(ck, 'weight.table_' + ('f32' if got.dtype == torch.float32 else 'f16_t' if n[-2:] in ('_t', 't2') else 'f16'), got.reshape(-1),
                         want[n].reshape(-1), n + ': ' + what)


def run_prep(layers, pool, any_sn, any_legacy, legacy_entry=False):
    tab = table('hv_wprep_layer', [l.row() for l in layers])
    mx = max(l.CoutF * l.taps * l.CinP + l.CinB * l.taps * l.CoutP for l in layers)
    if legacy_entry:
        L.call('hv_weight_prep', ctypes.cast(tab.ptr(), ctypes.POINTER(L.hv_wprep_layer)), tab.n, ctypes.c_longlong(mx), lib.stream())
    else:
        ops.weight_prep(tab, mx, any_sn=any_sn, any_legacy=any_legacy)
    return pool.intact()


def k2_of(cin):
    return 64 if WR.rup(cin, 4) >= 64 and cin > 64 else 32 if WR.rup(cin, 4) >= 32 and cin > 32 else 0


PREP_SHAPES = WR.SN_SHAPES + [s for s in WR.LAYOUT_SHAPES if s not in WR.SN_SHAPES]


@pytest.mark.parametrize('power_iter', [0, 1])
@pytest.mark.parametrize('shape', PREP_SHAPES, ids=['%dx%dx%d' % s for s in PREP_SHAPES])
def test_weight_prep_sigma_and_tables(shape, power_iter):
    """One layer through hv_weight_prep2 (any_sn = 1, any_legacy = 0) and through the element-wise hv_weight_prep: sigma, u', v' and all tables.  Spectral norm
    wherever the sigma kernel takes the shape (K <= 4608, Cout <= 1024); 1x512x4 (K = 8192) is a plain layer.  Without power iteration the spectral-norm case
    shapes also run on the exact-arithmetic inputs: sigma bit for bit."""
    cout, cin, k = shape
    sn = cin * k * k <= WR.SN_MAXK and cout <= WR.SN_MAXCO
    ck = Check()
    W, u, v = WR.sn_inputs(cout, cin, k)
    what = '%dx%dx%d pi=%d' % (cout, cin, k, power_iter)
    sig = {}
    for legacy in (False, True):
        pool = Pool()
        lay = PrepLayer(pool, W, u, v, cout, cin, k, sn, power_iter and sn, K2=k2_of(cin))
        ck.true(run_prep([lay], pool, 1, 0, legacy_entry=legacy), 'guards: ' + what)
        lay.check(ck, what + (' (hv_weight_prep)' if legacy else ''), legacy=legacy)
        sig[legacy] = lay.b['sigma'].cpu()
    ck.true(same_bits(sig[False], sig[True]), 'sigma differs between the two entries: ' + what)
    if shape in WR.SN_SHAPES and not power_iter:
        We, ue, ve = WR.sn_inputs(cout, cin, k, exact=True)
        assert WR.exact_ok(ue.double().abs() @ We.double().abs() @ ve.double().abs(), 512), 'test inputs: sigma is not exact in fp32'
        pool = Pool()
        lay = PrepLayer(pool, We, ue, ve, cout, cin, k, 1, 0)
        ck.true(run_prep([lay], pool, 1, 0), 'guards: exact ' + what)
        exact_le(ck, 'weight.sigma_exact', lay.b['sigma'].cpu()[:1], WR.spectral_norm_ref(We, ue, ve, 0)[0].float().reshape(1), 'exact inputs: ' + what)
        lay.check(ck, 'exact inputs: ' + what)
    ck.done()


@pytest.mark.parametrize('shape', WR.TRANSPOSED_SHAPES, ids=['%dx%dx%d' % s for s in WR.TRANSPOSED_SHAPES])
def test_weight_prep_conv_transpose_sources(shape):
    """transposed_src layers ([Cin][Cout][taps], no spectral norm) through the element-wise kernels: hv_weight_prep2 with any_legacy = 1 (beside a plain conv
    layer that the fused kernel takes) and hv_weight_prep."""
    cout, cin, k = shape
    ck = Check()
    W = torch.randn(cin * cout * k * k, generator=torch.Generator().manual_seed(cout))
    W2 = WR.sn_inputs(16, 4, 5)[0]
    for legacy in (False, True):
        pool = Pool()
        keep = TABLES[:6]
        lays = [PrepLayer(pool, W, None, None, cout, cin, k, 0, 0, transposed=True, sigma0=1.0, keep=keep), PrepLayer(pool, W2, None, None, 16, 4, 5, 0, 0, sigma0=1.0)]
        ck.true(run_prep(lays, pool, 0, 1, legacy_entry=legacy), 'guards')
        for i, lay in enumerate(lays):
            lay.check(ck, 'transposed %dx%dx%d layer %d legacy=%d' % (cout, cin, k, i, legacy), legacy=legacy)
    ck.done()


def test_weight_prep_lean_descriptor_leaves_the_other_tables_alone():
    ck = Check()
    for shape, keep in (((64, 128, 3), ('w_fwd_t', 'w_bwd_h')), ((32, 33, 3), ('w_fwd', 'w_bwd_t', 'w_fwd_t2')), ((40, 24, 3), ('w_bwd',)), ((128, 64, 4), ('w_fwd', 'w_fwd_t'))):
        cout, cin, k = shape
        W, u, v = WR.sn_inputs(cout, cin, k)
        pool = Pool()
        lay = PrepLayer(pool, W, u, v, cout, cin, k, 1, 0, K2=k2_of(cin), keep=keep)
        ck.true(run_prep([lay], pool, 1, 0), 'guards')
        lay.check(ck, 'lean %dx%dx%d %s' % (cout, cin, k, '+'.join(keep)))
    ck.done()


def test_weight_prep_mixed_table_and_two_power_iterations():
    """Spectral-norm and plain layers interleaved in one table: every layer's outputs equal those of the layer alone, bit for bit, and a plain layer's sigma
    slot is 1.0.  Then the same table once more: the second power iteration starts from the first one's u, v -- against two reference iterations."""
    ck = Check()
    specs = [(7, 7, 3, 1), (16, 4, 5, 0), (100, 57, 3, 1), (64, 1, 4, 0), (33, 65, 1, 1), (32, 33, 3, 1)]
    pool = Pool()
    lays = [PrepLayer(pool, *WR.sn_inputs(co, ci, k), co, ci, k, sn, sn, K2=k2_of(ci)) for co, ci, k, sn in specs]
    tab = table('hv_wprep_layer', [l.row() for l in lays])
    mx = max(l.CoutF * l.taps * l.CinP + l.CinB * l.taps * l.CoutP for l in lays)
    ops.weight_prep(tab, mx, any_sn=True, any_legacy=False)
    ck.true(pool.intact(), 'guards: mixed')
    for lay, (co, ci, k, sn) in zip(lays, specs):
        what = 'mixed %dx%dx%d' % (co, ci, k)
        lay.check(ck, what)
        p1 = Pool()
        one = PrepLayer(p1, *WR.sn_inputs(co, ci, k), co, ci, k, sn, sn, K2=k2_of(ci))
        ck.true(run_prep([one], p1, 1, 0), 'guards: alone ' + what)
        for n in one.b:
            ck.true(same_bits(one.b[n].cpu(), lay.b[n].cpu()), '%s differs from the layer alone: %s' % (n, what))
    ops.weight_prep(tab, mx, any_sn=True, any_legacy=False)
    ck.true(pool.intact(), 'guards: second call')
    for lay, (co, ci, k, sn) in zip(lays, specs):
        if not sn:
            continue
        what = 'second iteration %dx%dx%d' % (co, ci, k)
        Wm = lay.W.reshape(co, -1)
        _, u1, v1 = WR.spectral_norm_ref(Wm, lay.u0, lay.v0, 1)
        _, bu1, bv1 = WR.spectral_norm_bounds(Wm, lay.u0, lay.v0, 1)
        ref = WR.spectral_norm_ref(Wm, u1, v1, 1)
        bs, bu, bv = WR.spectral_norm_bounds(Wm, u1, v1, 1, du=bu1, dv=bv1)
        sg = lay.b['sigma'].cpu()[0]
        ck.le('weight.sigma', err(sg, ref[0]), bs, what)
        ck.le('weight.sn_u', err(lay.b['u'].cpu(), ref[1]), bu, what)
        ck.le('weight.sn_v', err(lay.b['v'].cpu(), ref[2]), bv, what)
        want = WR.weight_tables_ref(lay.W, sg.item(), co, ci, lay.taps, lay.CinP, lay.CoutF, lay.CoutP, lay.CinB)
        exact_le(ck, 'weight.table_f32', lay.b['w_fwd'].cpu().reshape(-1), want['w_fwd'].reshape(-1), what)
    ck.done()


# ---------------------------------------------------------------------------------------------------------------- hv_weight_prep_backward
class BwdLayer:
    def __init__(self, pool, cout, cin, taps, sn, accumulate, transposed=False, exact=False, offset=0):
        self.cout, self.cin, self.taps, self.sn, self.acc, self.transposed, self.exact = cout, cin, taps, sn, accumulate, transposed, exact
        self.I = I = WR.bwd_inputs(cout, cin, taps, transposed_src=transposed, exact=exact)
        self.sig0 = torch.tensor([I['sigma'].item(), 6.0, 5.0, 5.0])
        self.b = {k: pool.put(I[k], offset=offset if k == 'dw_ohwi' else 0) for k in ('dw_ohwi', 'w_fwd', 'u', 'v')}
        self.b['sigma'] = pool.put(self.sig0)
        self.b['dw_orig'] = pool.put(I['before']) if accumulate else pool.out(cout * cin * taps)

    def row(self):
        b = self.b
        return dict(dw_ohwi=b['dw_ohwi'], w_fwd=b['w_fwd'], u=b['u'] if self.sn else None, v=b['v'] if self.sn else None, sigma=b['sigma'], dw_orig=b['dw_orig'],
                    Cout=self.cout, Cin=self.cin, taps=self.taps, CinP=self.I['CinP'], sn=int(self.sn), transposed_src=int(self.transposed), accumulate=int(self.acc))

    def check(self, ck, what):
        I, b = self.I, self.b
        for k in ('dw_ohwi', 'w_fwd', 'u', 'v'):
            ck.true(same_bits(b[k].cpu(), I[k]), 'input %s changed: %s' % (k, what))
        sg, got = b['sigma'].cpu(), b['dw_orig'].cpu()
        keep = [0, 2, 3] if self.sn else [0, 1, 2, 3]
        ck.true(same_bits(sg[keep], self.sig0[keep]), 'sigma words touched: ' + what)
        if self.transposed:
            _, ref = WR.weight_prep_backward_ref(I['dw_ohwi'], I['w_fwd'], None, None, None, self.cout, self.cin, self.taps, I['CinP'], 0, True, I['before'], self.acc)
            exact_le(ck, 'weight.bwd_plain', got, ref.float(), what)
            return
        ref_dot, ref, bdot, bout = WR.bwd_bounds(I, self.cout, self.cin, self.taps, self.sn, self.acc, self.exact)
        if not self.sn:
            exact_le(ck, 'weight.bwd_plain', got, ref.float(), what)
            return
        if self.exact:
            exact_le(ck, 'weight.bwd_dot_exact', sg[1:2], ref_dot.float().reshape(1), what)
        else:
            ck.le('weight.bwd_dot', err(sg[1], ref_dot), bdot, what)
        ck.le('weight.bwd_g_exact' if self.exact else 'weight.bwd_g', err(got, ref), bout, what)


def run_bwd(lays, pool, any_sn):
    tab = table('hv_wprep_bwd_layer', [l.row() for l in lays])
    ops.weight_prep_backward(tab, max(l.cout * l.cin * l.taps for l in lays), any_sn)
    return pool.intact()


@pytest.mark.parametrize('name', sorted(WR.BWD_CASES))
def test_weight_prep_backward(name):
    """Spectral norm on and off, accumulate 0 and 1, random and exact-arithmetic inputs, dw_ohwi 16-byte aligned and at a 4-byte offset (the scalar dot).  A
    layer without spectral norm also with any_sn = 0; either way its sigma[1] stays."""
    cout, cin, taps = WR.BWD_CASES[name]
    ck = Check()
    for sn, acc, exact, off in ((1, 0, 0, 0), (1, 1, 0, 0), (1, 0, 1, 0), (1, 1, 1, 1), (1, 0, 0, 1), (0, 0, 0, 0), (0, 1, 0, 1), (0, 1, 0, 0)):
        what = '%s sn=%d acc=%d exact=%d offset=%d' % (name, sn, acc, exact, off)
        pool = Pool()
        lay = BwdLayer(pool, cout, cin, taps, sn, acc, exact=bool(exact), offset=off)
        ck.true(run_bwd([lay], pool, 1 if sn else acc), 'guards: ' + what)
        lay.check(ck, what)
    ck.done()


@pytest.mark.parametrize('name', sorted(WR.BWD_TRANSPOSED))
def test_weight_prep_backward_conv_transpose(name):
    cout, cin, taps = WR.BWD_TRANSPOSED[name]
    ck = Check()
    for acc in (0, 1):
        pool = Pool()
        lay = BwdLayer(pool, cout, cin, taps, 0, acc, transposed=True)
        ck.true(run_bwd([lay], pool, 0), 'guards')
        lay.check(ck, '%s acc=%d' % (name, acc))
    ck.done()


def test_weight_prep_backward_table_of_very_different_layers():
    """max_numel comes from the largest layer: the small ones see workgroups beyond their extent."""
    ck = Check()
    pool = Pool()
    specs = [('no36', 1, 0, False), ('n20736', 1, 1, False), ('tr5', 0, 0, True), ('no1025', 0, 1, False), ('no9225', 1, 0, False), ('no36', 0, 0, False)]
    lays = [BwdLayer(pool, *(WR.BWD_TRANSPOSED if tr else WR.BWD_CASES)[n], sn, acc, transposed=tr) for n, sn, acc, tr in specs]
    ck.true(run_bwd(lays, pool, 1), 'guards')
    for lay, s in zip(lays, specs):
        lay.check(ck, 'table %s sn=%d acc=%d' % s[:3])
    ck.done()


# ---------------------------------------------------------------------------------------------------------------- Adam
def adam_table(p, g, m, v, sizes):
    rows, off = [], 0
    for n in sizes:
        rows.append(dict(p=p.t[off:off + n], g=g.t[off:off + n], m=m.t[off:off + n], v=v.t[off:off + n], n=n))
        off += n
    return table('hv_adam_tensor', rows)


def call_adam(tab, max_numel, lr, h, step):
    L.call('hv_adam_step', ctypes.cast(tab.ptr(), ctypes.POINTER(L.hv_adam_tensor)), tab.n, ctypes.c_longlong(max_numel), lib.ptr(lr.t), ctypes.c_float(h['beta1']),
           ctypes.c_float(h['beta2']), ctypes.c_float(h['eps']), lib.ptr(step.t), lib.stream())


@pytest.mark.parametrize('step', WR.ADAM_STEPS)
def test_adam_step(step):
    """One call over tensors of 1 .. 4099 elements back to back in one flat buffer (most start off 16-byte alignment; max_numel = 4099 gives the short ones
    workgroups beyond their end), the step counter preset so that the kernel sees `step`.  Then g = 0 on m = v = 0: nothing moves."""
    ck = Check()
    h = WR.adam_hyper32()
    N = sum(WR.ADAM_SIZES)
    p, g, m, v = WR.adam_inputs(N, step)
    ref, bounds = WR.adam_bounds(p, g, m, v, step, h)
    pool = Pool()
    P, G, M, V = (pool.put(x) for x in (p, g, m, v))
    lr, cnt = pool.put(torch.tensor([h['lr']])), pool.put(torch.tensor([float(step - 1)]))
    call_adam(adam_table(P, G, M, V, WR.ADAM_SIZES), 4099, lr, h, cnt)
    ck.true(pool.intact(), 'guards')
    ck.true(cnt.cpu().item() == float(step), 'step counter %r' % cnt.cpu().item())
    ck.true(same_bits(G.cpu(), g), 'gradient changed')
    for fam, buf, r, b in (('weight.adam_p', P, ref[0], bounds[0]), ('weight.adam_m', M, ref[1], bounds[1]), ('weight.adam_v', V, ref[2], bounds[2])):
        ck.le(fam, err(buf.cpu(), r), b, 'step %d' % step)
    pool = Pool()
    P, G, M, V = pool.put(p), pool.put(torch.zeros(N)), pool.put(torch.zeros(N)), pool.put(torch.zeros(N))
    lr, cnt = pool.put(torch.tensor([h['lr']])), pool.put(torch.tensor([float(step - 1)]))
    call_adam(adam_table(P, G, M, V, WR.ADAM_SIZES), 4099, lr, h, cnt)
    ck.true(pool.intact(), 'guards: zero gradient')
    ck.true(same_bits(P.cpu(), p) and same_bits(M.cpu(), torch.zeros(N)) and same_bits(V.cpu(), torch.zeros(N)), 'zero gradient on zero moments moved something')
    ck.done()


def test_adam_three_chained_steps_follow_the_device_lr():
    """Three calls, the device lr scalar changed between them, against three reference steps; the counter advances by exactly 1 per call.  Bounds: each step's
    own (on the reference state), plus the previous bounds of m, v, p carried through the update to first order."""
    ck = Check()
    h = WR.adam_hyper32()
    N = sum(WR.ADAM_SIZES)
    p, g0, m, v = WR.adam_inputs(N, 1)
    pool = Pool()
    P, G, M, V = (pool.put(x) for x in (p, g0, m, v))
    lr, cnt = pool.put(torch.tensor([h['lr']])), pool.put(torch.tensor([0.0]))
    tab = adam_table(P, G, M, V, WR.ADAM_SIZES)
    rp, rm, rv = p.double(), m.double(), v.double()
    bp = bm = bv = torch.zeros(N, dtype=torch.float64)
    for step, lr_k in ((1, 2e-4), (2, 1e-4), (3, 3e-4)):
        hk = dict(h, lr=WR.f32(lr_k))
        g = WR.adam_inputs(N, step, seed=step)[1]
        G.t.copy_(g)
        lr.t.fill_(hk['lr'])
        call_adam(tab, 4099, lr, hk, cnt)
        ck.true(pool.intact(), 'guards: step %d' % step)
        ck.true(cnt.cpu().item() == float(step), 'step counter after call %d: %r' % (step, cnt.cpu().item()))
        # this step's own bounds, measured on the fp32 roundings of the reference state; the previous bounds through d(update) / d(m, v)
        ref, own = WR.adam_bounds(rp.float(), g, rm.float(), rv.float(), step, hk)
        exact = WR.adam_ref(rp, g, rm, rv, step, hk['lr'], hk['beta1'], hk['beta2'], hk['eps'])
        bc1, bc2 = 1 - hk['beta1'] ** step, 1 - hk['beta2'] ** step
        bm = own[1] + hk['beta1'] * bm
        bv = own[2] + hk['beta2'] * bv
        denom = exact[2].sqrt() / bc2 ** 0.5 + hk['eps']
        dden = bv / (2 * exact[2].sqrt().clamp_min(1e-30) * bc2 ** 0.5)
        bp = own[0] + bp + hk['lr'] / bc1 * (bm / denom + exact[1].abs() * dden / denom ** 2)
        rp, rm, rv = exact[:3]
        for fam, buf, r, b in (('weight.adam_chain_p', P, rp, bp), ('weight.adam_chain_m', M, rm, bm), ('weight.adam_chain_v', V, rv, bv)):
            ck.le(fam, err(buf.cpu(), r), b, 'chained step %d' % step)
    ck.done()


def guard_positions(n):
    """Where a bad value goes: index 0, the last index, inside the scalar tail of the float4 pass, inside the last workgroup's range (its last pass)."""
    pos = {'first': 0, 'last': n - 1}
    if n % 4:
        pos['tail'] = n - n % 4
    blocks = min(n // 4096 + 1, 256)
    i = (blocks - 1) * 1024 + 517
    if i < n:
        pos['last_wg'] = i + (n - 1 - i) // (blocks * 1024) * (blocks * 1024)
    return pos


def guard_gradient(n, seed):
    g = torch.randn(n, generator=torch.Generator().manual_seed(n + seed)) * 3.0
    return g


def call_guarded(tab, max_numel, lr, h, state, flat, n, mul):
    L.call('hv_adam_step_guarded', ctypes.cast(tab.ptr(), ctypes.POINTER(L.hv_adam_tensor)), tab.n, ctypes.c_longlong(max_numel), lib.ptr(lr.t),
           ctypes.c_float(h['beta1']), ctypes.c_float(h['beta2']), ctypes.c_float(h['eps']), lib.ptr(state.t), lib.ptr(flat.t), ctypes.c_longlong(n),
           ctypes.c_float(mul), lib.stream())


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize('n', WR.GUARD_SIZES)
def test_adam_step_guarded(n):
    """A clean gradient, 3.0e38 (finite by the contract), then one bad value (+inf, -inf, nan) at each position, grad_mul cycling through 1, 2^-7, 2^-16.  After
    every call: the state words, the gradient unscaled on good and bad steps alike, p / m / v untouched by a skipped step, a good step bit-identical to
    hv_adam_step on the unscaled gradient."""
    ck = Check()
    h = WR.adam_hyper32()
    k = min(n, 4099)
    sizes = [k] if k < 4 else [k - k // 3, k // 3]
    p0, _, m0, v0 = WR.adam_inputs(k, 10)
    pool = Pool()
    P, M, V, flat = pool.put(p0), pool.put(m0), pool.put(v0), pool.out(n)
    tab = adam_table(P, flat, M, V, sizes)
    P2, M2, V2, G2 = pool.put(p0), pool.put(m0), pool.put(v0), pool.out(k)
    tab2 = adam_table(P2, G2, M2, V2, sizes)
    cnt2 = pool.put(torch.tensor([0.0]))
    lr = pool.put(torch.tensor([h['lr']]))
    state = pool.put(torch.tensor([9.0, 0, 3.0, 0, 0, 0, 0, 0]))
    good, skipped = 9, 3
    cases = [('clean', None, None), ('3.0e38', n - 1, 3.0e38), ('-3.0e38', 0, -3.0e38)]
    cases += [(w, i, x) for w, i in guard_positions(n).items() for x in (float('inf'), -float('inf'), NAN)]
    muls = (1.0, 2.0 ** -7, 2.0 ** -16)
    for c, (where, idx, x) in enumerate(cases):
        mul = 1.0 if where.endswith('e38') else muls[c % 3]
        what = 'n=%d %s %r mul=%g' % (n, where, x, mul)
        for b_, x0 in zip((P, M, V), (p0, m0, v0)):      # every case from the same state (3.0e38 squared leaves v = inf)
            b_.t.copy_(x0)
        g = guard_gradient(n, c)
        if n >= 5 and mul == 1.0:
            g[1], g[2] = -0.0, 1e-40
        if idx is not None:
            g[idx] = x
        want, bad = WR.unscale_check_ref(g, mul)
        ck.true(bad == (where not in ('clean', '3.0e38', '-3.0e38')), 'reference flag: ' + what)
        flat.t.copy_(g)
        before = [bits(b.t).clone() for b in (P, M, V)]
        call_guarded(tab, k, lr, h, state, flat, n, mul)
        ck.true(pool.intact(), 'guards: ' + what)
        good, skipped = good + (not bad), skipped + bad
        st = state.cpu()
        ck.true(st.tolist() == [float(good), 0.0, float(skipped), float(bad), 0.0, 0.0, 0.0, 0.0] and int(bits(st)[4]) == 0, 'state %r: %s' % (st.tolist(), what))
        got, want32 = flat.t, want.float().to(T.dev())
        if bad:      # the bad element stays bad (inf keeps its sign); every other element is compared below
            gb = got[idx].item()
            ck.true(gb != gb if x != x else gb == x, 'bad element became %r: %s' % (gb, what))
            want32[idx] = got[idx]
        exact_le(ck, 'weight.unscale', got, want32, what)
        if bad:
            ck.true(all(torch.equal(bits(b.t), a) for b, a in zip((P, M, V), before)), 'a skipped step moved p / m / v: ' + what)
        else:
            for b, a in zip((P2, M2, V2), before):
                bits(b.t).copy_(a)
            G2.t.copy_(want32[:k])
            cnt2.t.fill_(float(good - 1))
            call_adam(tab2, k, lr, h, cnt2)
            ck.true(pool.intact(), 'guards: hv_adam_step of ' + what)
            same = all(torch.equal(bits(b.t), bits(b2.t)) for b, b2 in zip((P, M, V), (P2, M2, V2)))
            exact_flag(ck, 'weight.guarded_vs_plain', same, what)
            ck.true(not all(torch.equal(bits(b.t), a) for b, a in zip((P, M, V), before)), 'a good step moved nothing: ' + what)
    ck.done()


def test_adam_step_guarded_four_launches_without_a_host_sync():
    """good, bad, bad, good back to back on one stream (the gradients are staged by device copies): the ticket and the flag are back at zero for the next
    launch without the host's help, two steps are taken, two skipped, and the weights are those of the two good steps alone."""
    ck = Check()
    h = WR.adam_hyper32()
    n, sizes = 3 * 4096 + 7, [4099, 1025, 255]
    k = sum(sizes)
    p0, _, m0, v0 = WR.adam_inputs(k, 1)
    grads = [guard_gradient(n, s) * 1e-2 for s in range(4)]
    grads[1][n - 2] = float('inf')
    grads[2][4096 + 5] = NAN
    dev = [g.to(T.dev()) for g in grads]
    pool = Pool()
    P, M, V, flat = pool.put(p0), pool.put(m0), pool.put(v0), pool.out(n)
    lr, state = pool.put(torch.tensor([h['lr']])), pool.put(torch.zeros(8))
    tab = adam_table(P, flat, M, V, sizes)
    for d in dev:
        flat.t.copy_(d)
        call_guarded(tab, 4099, lr, h, state, flat, n, 2.0 ** -7)
    ck.true(pool.intact(), 'guards')
    st = state.cpu()
    ck.true(st.tolist() == [2.0, 0.0, 2.0, 0.0, 0.0, 0.0, 0.0, 0.0] and int(bits(st)[4]) == 0, 'state %r' % st.tolist())
    exact_le(ck, 'weight.unscale', flat.cpu(), (grads[3].double() * 2.0 ** -7).float(), 'fourth gradient')
    P2, M2, V2, G2 = pool.put(p0), pool.put(m0), pool.put(v0), pool.out(k)
    cnt = pool.put(torch.tensor([0.0]))
    tab2 = adam_table(P2, G2, M2, V2, sizes)
    for s in (0, 3):
        G2.t.copy_((grads[s][:k].double() * 2.0 ** -7).float())
        call_adam(tab2, 4099, lr, h, cnt)
    ck.true(pool.intact(), 'guards: plain')
    same = all(same_bits(a.cpu(), b.cpu()) for a, b in zip((P, M, V), (P2, M2, V2)))
    exact_flag(ck, 'weight.guarded_vs_plain', same, 'good, bad, bad, good')
    ck.done()
