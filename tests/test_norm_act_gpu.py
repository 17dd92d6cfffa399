"""The kernels between the convolutions against the fp64 references of tests/pointwise_ref.py (pinned by tests/test_pointwise_ref_cpu.py):
csrc/norm.hip (reduce mode 0 / 1, apply, backward apply; vector / scalar; fp32 / fp16 storage; the chunk planner and the workspace query),
the activation-gradient / head-seed section of csrc/prep.hip and the GAN-loss section of csrc/pointwise.hip.

Every bound is computed here from fp64 reference quantities (u = 2^-24), never from the kernel's output:
  element-wise outputs  4 x (the largest error of a plain fp32 torch evaluation of the same formula on the CPU) + 4u |ref| per element,
                        + max(2^-11 |ref|, 2^-25) for a value stored as fp16;
  statistics            |mean - ref| <= 2u |ref| + 1e-12, |rstd - ref| <= 8u ref; the running statistics 2u |ref| more for the blend;
  fp32 reductions       16u sum |g| (|xhat| + |mean| rstd) + u |ref| (dgamma), 16u sum |g| + u |ref| (plain sums), and (ceil(log2 npix) + 16) u sum |g|
                        more where the accumulation itself is fp32 (act_backward, the heads);
  loss scalars          64u (lw / n) sum |l_i|.
Both sides of a backward read the same stored y and the same stored fp32 statistics, so thresholds are decided alike and no element is left out.
The worst error / bound ratio of every family is printed at the end of the module (pytest -s)."""
import ctypes
import functools
import math

import pytest
import torch

import pointwise_ref as PR

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SENT = 7.5                     # sentinel of the channels around a view (exact in fp16)
EPS = float(torch.tensor(1e-5, dtype=torch.float32))
MOM = float(torch.tensor(0.1, dtype=torch.float32))
RATIOS = {}
ops = T = lib = None


@pytest.fixture(scope='module', autouse=True)
def _env():
    global ops, T, lib
    import hvgan  # noqa: F401
    from hvgan import lib as _lib, ops as _ops
    import hvtest as _T
    ops, T, lib = _ops, _T, _lib
    yield
    print_ratios()


def print_ratios(prefix=''):
    print('\nworst error / bound per family')
    for k in sorted(RATIOS):
        if k.startswith(prefix):
            print('  %-22s %.3e' % (k, RATIOS[k]))


class Check:
    """Collects error <= bound comparisons of one test; every failure is reported, the worst ratio per family is recorded."""

    def __init__(self):
        self.fails = []

    def le(self, family, err, bound, what=''):
        err, bound = torch.as_tensor(err, dtype=torch.float64), torch.as_tensor(bound, dtype=torch.float64)
        bound = bound.expand_as(err) if bound.dim() <= err.dim() else bound
        ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
        r = float('nan') if bool(torch.isnan(ratio).any()) else (ratio.max().item() if ratio.numel() else 0.0)
        if not (RATIOS.get(family, 0.0) >= r):
            RATIOS[family] = r
        if not r <= 1.0:
            self.fails.append((family, what, r))

    def true(self, cond, what):
        if not bool(cond):
            self.fails.append(what)

    def done(self):
        assert not self.fails, self.fails


def tol_elem(ref, floor, f16):
    t = 4 * floor + 4 * U * ref.abs()
    return t + torch.clamp(2.0 ** -11 * ref.abs(), min=2.0 ** -25) if f16 else t


def dtype_of(f16):
    return torch.float16 if f16 else torch.float32


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool((a.view(torch.uint8) == b.view(torch.uint8)).all())


class ExactWs:
    """ops._ws replaced by one that hands out EXACTLY the queried bytes, a 16-byte aligned view into a sentinel-filled buffer."""

    def __init__(self, monkeypatch):
        self.big, self.n = None, 0
        monkeypatch.setattr(ops, '_ws', self.ws)
        self.mp = monkeypatch

    def ws(self, nbytes, device, slot=0):
        self.n = int(nbytes)
        self.big = torch.full((512 + self.n,), 0xA5, dtype=torch.uint8, device=device)
        v = self.big[256:256 + self.n]
        assert v.data_ptr() % 16 == 0
        return v, ctypes.c_size_t(self.n)

    def close(self):
        self.mp.undo()
        torch.cuda.synchronize()
        assert self.big is not None, 'no workspace was asked for'
        assert bool((self.big[:256] == 0xA5).all()) and bool((self.big[256 + self.n:] == 0xA5).all()), 'wrote outside the queried workspace'


def others_untouched(act_view):
    t = act_view.t.cpu()
    keep = torch.ones(t.shape[-1], dtype=torch.bool)
    keep[act_view.coff:act_view.coff + act_view.C] = False
    return bool((t[..., keep] == SENT).all())


# ---------------------------------------------------------------------------------------------------------------- normalisation
# name: (norm, training, groups, B, H, W, C, views {tensor: (ld, coff)})
UNAL = {k: (24, 2) for k in ('x', 'y', 'dy', 'dx')}
VIEWS = {'x': (48, 8), 'y': (56, 8), 'dy': (64, 8), 'dx': (40, 8)}
ROWS = {
    'quad_ragged': ('batch', True, 1, 3, 7, 9, 16, {}),
    'cb4': ('batch', True, 1, 2, 5, 5, 4, {}),
    'slices4_r2': ('batch', True, 1, 2, 1, 1, 512, {}),
    'slices2_r8': ('batch', True, 1, 2, 2, 2, 256, {}),
    'widest': ('batch', True, 1, 2, 3, 3, 1024, {}),
    'halves': ('batch', True, 2, 4, 9, 7, 128, {}),
    'six_g2': ('batch', True, 2, 6, 5, 5, 64, {}),
    'six_g3': ('batch', True, 3, 6, 5, 5, 64, {}),
    'inst32': ('instance', True, 1, 3, 7, 9, 32, {}),
    'inst256': ('instance', True, 1, 4, 10, 10, 256, {}),
    'c1_batch': ('batch', True, 1, 2, 6, 5, 1, {}),
    'c2_batch': ('batch', True, 1, 2, 6, 5, 2, {}),
    'c1_inst': ('instance', True, 1, 2, 6, 5, 1, {}),
    'c2_inst': ('instance', True, 1, 2, 6, 5, 2, {}),
    'unaligned': ('batch', True, 1, 2, 6, 5, 16, UNAL),
    'slice_views': ('batch', True, 1, 2, 6, 5, 32, VIEWS),
    'cap': ('batch', True, 1, 2, 129, 129, 128, {}),
    'cap_groups': ('instance', True, 1, 16, 91, 91, 128, {}),
    'eval': ('batch', False, 1, 2, 7, 9, 32, {}),
}
BASE_ACTS = [('lrelu', False), ('relu', False), ('none', False)]
MORE_ACTS = [('elu', False), ('lrelu', True)]
MORE_ROWS = ('quad_ragged', 'halves', 'six_g2', 'six_g3', 'inst32', 'inst256')
NORM_CASES = [(r, f16, a, ps) for r in ROWS for f16 in (False, True) for a, ps in BASE_ACTS + (MORE_ACTS if r in MORE_ROWS else [])]


@functools.lru_cache(maxsize=2)
def norm_inputs(row, f16):
    """Stored inputs of a row (drawn in fp32, rounded once to the storage type).  Channel 0: |mu| / s = 1e3 (1e2 in fp16 storage); the last channel (C > 1)
    is constant at 0.3; gamma has a negative and, from four channels on, a zero entry.  s in [2, 4] keeps gamma * rstd * dy inside fp16 at the fp16 gradient
    scale."""
    norm, training, groups, B, H, W, C, _ = ROWS[row]
    dt = dtype_of(f16)
    gen = torch.Generator().manual_seed(1000 + sorted(ROWS).index(row))
    r = lambda *s: torch.randn(*s, generator=gen)
    s = 2 + 2 * torch.rand(C, generator=gen)
    # |mu| >= 16: the mean of every group, down to two rows of s <= 4, keeps the sign of mu and of the running mean 0.25 mu, so the blend never cancels (its
    # bound is relative to the blended value)
    mu = (16 + 4 * r(C).abs()) * torch.where(r(C) > 0, 1.0, -1.0)
    mu[0] = (1e2 if f16 else 1e3) * s[0]
    x = r(B, C, H, W) * s.view(1, C, 1, 1) + mu.view(1, C, 1, 1)
    cc = C - 1 if C > 1 else None
    if cc is not None:
        x[:, cc] = 0.3
        mu[cc] = 0.3
    gamma, beta = 1 + 0.25 * r(C), r(C)
    gamma[0] = -gamma[0].abs()
    if C >= 4:
        gamma[2] = 0.0
    rm0, rv0 = 0.25 * mu, (0.5 + torch.rand(C, generator=gen)) * s * s
    dy = r(B, C, H, W) * (ops.grad_scale('fp16') if f16 else 1.0)
    x = x.to(dt)
    if f16:      # rstd > 1/2 in some group (the constant channel; two rows that round to nearly the same fp16 value): dy * 2^-10 there, so that dx stays in fp16
        for sl in PR.group_slices(B, norm, groups):
            dy[sl] *= torch.where(x[sl].double().var(dim=(0, 2, 3), unbiased=False) < 4, 2.0 ** -10, 1.0).float().view(1, C, 1, 1)
    return dict(x=x, dy=dy.to(dt), gamma=gamma, beta=beta, rm0=rm0, rv0=rv0, cc=cc)


def view(row, name, data, fill=SENT):
    ld, coff = ROWS[row][7].get(name, (data.shape[1], 0))
    return T.to_act_view(data, ld, coff, fill)


def run_forward(row, inp, act, ps, stats_only=False):
    norm, training, groups, B, H, W, C, _ = ROWS[row]
    dev = T.dev()
    xa = view(row, 'x', inp['x'])
    ya = None if stats_only else view(row, 'y', torch.zeros_like(inp['x']))
    G = B if norm == 'instance' else groups
    stats = torch.full((G, 2, C), float('nan'), device=dev)
    kw = {}
    if norm == 'batch':
        kw = dict(gamma=inp['gamma'].to(dev), beta=inp['beta'].to(dev), running_mean=inp['rm0'].to(dev), running_var=inp['rv0'].to(dev),
                  nbt=torch.tensor([5], dtype=torch.int64, device=dev))
    ops.norm_act_forward(xa, ya, norm, training, stats, act=act, post_sigmoid=ps, eps=EPS, momentum=MOM, groups=groups, **kw)
    torch.cuda.synchronize()
    return ya, stats, kw


def run_backward(row, inp, y_st, stats32, act, ps, accumulate=None):
    norm, training, groups, B, H, W, C, _ = ROWS[row]
    dev = T.dev()
    xa, dya, ya = view(row, 'x', inp['x']), view(row, 'dy', inp['dy']), view(row, 'y', y_st)
    dxa = view(row, 'dx', torch.zeros_like(inp['x']))
    if accumulate is None:
        dg, db = torch.full((C,), float('nan'), device=dev), torch.full((C,), float('nan'), device=dev)
    else:
        dg, db = accumulate[0].to(dev), accumulate[1].to(dev)
    ops.norm_act_backward(dya, ya, xa, dxa, norm, training, stats32.to(dev), gamma=inp['gamma'].to(dev) if norm == 'batch' else None, act=act,
                          post_sigmoid=ps, dgamma=dg, dbeta=db, param_accumulate=accumulate is not None, groups=groups)
    torch.cuda.synchronize()
    return dxa, dg, db


@pytest.mark.parametrize('row,f16,act,ps', NORM_CASES, ids=['%s-%s-%s%s' % (r, 'f16' if h else 'f32', a, '+sig' if p else '') for r, h, a, p in NORM_CASES])
def test_norm_act_forward_backward(row, f16, act, ps, monkeypatch):
    norm, training, groups, B, H, W, C, views = ROWS[row]
    ck = Check()
    inp = norm_inputs(row, f16)
    dt = dtype_of(f16)
    affine = norm == 'batch'
    x64, dy64 = inp['x'].double(), inp['dy'].double()
    g64, b64 = (inp['gamma'].double(), inp['beta'].double()) if affine else (None, None)
    sl = PR.group_slices(B, norm, groups)
    yr, sr, rmr, rvr, nbt = PR.norm_act_forward_ref(x64, norm, training, g64, b64, inp['rm0'].double() if affine else None,
                                                    inp['rv0'].double() if affine else None, EPS, MOM, groups, act, ps)
    x32 = x64.float()
    y32 = torch.empty_like(x32)
    for k, s in enumerate(sl):
        y32[s] = PR.norm_apply_formula(x32[s], sr[k, 0].float(), sr[k, 1].float(), inp['gamma'] if affine else None, inp['beta'] if affine else None, act, ps)
    floor = (y32.double() - yr).abs().max().item()
    del y32

    # ---- forward
    ya, stats, kw = run_forward(row, inp, act, ps)
    ck.le('norm.y', (T.from_act(ya).double() - yr).abs(), tol_elem(yr, floor, f16), 'y')
    sd = stats.cpu().double()
    ck.le('norm.mean', (sd[:, 0] - sr[:, 0]).abs(), 2 * U * sr[:, 0].abs() + 1e-12, 'mean')
    ck.le('norm.rstd', (sd[:, 1] - sr[:, 1]).abs(), 8 * U * sr[:, 1], 'rstd')
    if inp['cc'] is not None and training:
        ck.le('norm.rstd', (sd[:, 1, inp['cc']] - EPS ** -0.5).abs(), 8 * U * EPS ** -0.5, 'rstd of the constant channel')
    if views:
        ck.true(others_untouched(ya), 'channels around y changed')
    if affine:
        if training:
            ck.le('norm.running', (kw['running_mean'].cpu().double() - rmr).abs(), 4 * U * rmr.abs() + 1e-12, 'running_mean')
            ck.le('norm.running', (kw['running_var'].cpu().double() - rvr).abs(), 10 * U * rvr.abs(), 'running_var')
        else:
            ck.true(torch.equal(kw['running_mean'].cpu(), inp['rm0']) and torch.equal(kw['running_var'].cpu(), inp['rv0']), 'eval changed the running statistics')
        ck.true(kw['nbt'].item() == 5 + nbt, 'num_batches_tracked %d' % kw['nbt'].item())
    _, stats2, kw2 = run_forward(row, inp, act, ps, stats_only=True)
    ck.true(same_bits(stats2, stats), 'statistics-only call: other stats bits')
    if affine:
        ck.true(same_bits(kw2['running_mean'], kw['running_mean']) and same_bits(kw2['running_var'], kw['running_var']), 'statistics-only call: other running bits')
    ex = ExactWs(monkeypatch)
    ya3, stats3, _ = run_forward(row, inp, act, ps)
    ex.close()
    ck.true(same_bits(ya3.t, ya.t) and same_bits(stats3, stats), 'exact workspace: other forward bits')
    del ya, ya3

    # ---- backward: both sides read the stored y and the stored fp32 statistics
    need_y = act != 'none' or ps
    y_st = yr.to(dt)
    stats32 = sr.float()
    st64 = stats32.double()
    dxr, dgr, dbr = PR.norm_act_backward_ref(dy64, y_st.double(), x64, st64, g64, norm, training, groups, act, ps)
    g, xhat = PR.norm_backward_terms(dy64, y_st.double(), x64, st64, norm, groups, act, ps)
    batch_stats = norm == 'instance' or training
    g32 = dy64.float() * PR.act_grad_from_out_formula(y_st.float(), act, ps) if need_y else dy64.float()
    dx32 = torch.empty_like(x32)
    bg, bb = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    for k, s in enumerate(sl):
        R = (s.stop - s.start) * H * W
        sg, sgx = g[s].sum(dim=(0, 2, 3)).float(), (g[s] * xhat[s]).sum(dim=(0, 2, 3)).float()
        dx32[s] = PR.norm_bwd_apply_formula(g32[s], x32[s], stats32[k, 0], stats32[k, 1], inp['gamma'] if affine else None, sg, sgx, R, batch_stats)
        bg += (g[s].abs() * (xhat[s].abs() + (st64[k, 0].abs() * st64[k, 1]).view(1, C, 1, 1))).sum(dim=(0, 2, 3))
        bb += g[s].abs().sum(dim=(0, 2, 3))
    bfloor = (dx32.double() - dxr).abs().max().item()
    del dx32, g32, g, xhat
    bg, bb = 16 * U * bg + U * dgr.abs(), 16 * U * bb + U * dbr.abs()
    if f16:
        assert dxr.abs().max().item() < 6.0e4, 'test inputs: dx leaves fp16'
    y_in = y_st if need_y else torch.full_like(y_st, float('nan'))          # act none: y must not be read
    dxa, dg, db = run_backward(row, inp, y_in, stats32, act, ps)
    ck.le('norm.dx', (T.from_act(dxa).double() - dxr).abs(), tol_elem(dxr, bfloor, f16), 'dx')
    ck.le('norm.dgamma', (dg.cpu().double() - dgr).abs(), bg, 'dgamma')
    ck.le('norm.dbeta', (db.cpu().double() - dbr).abs(), bb, 'dbeta')
    if views:
        ck.true(others_untouched(dxa), 'channels around dx changed')
    pre = (torch.linspace(-3, 3, C), torch.linspace(5, -5, C))
    _, dg2, db2 = run_backward(row, inp, y_in, stats32, act, ps, accumulate=pre)
    ck.le('norm.dgamma', (dg2.cpu().double() - (pre[0].double() + dgr)).abs(), bg + U * (pre[0].double() + dgr).abs(), 'dgamma accumulated')
    ck.le('norm.dbeta', (db2.cpu().double() - (pre[1].double() + dbr)).abs(), bb + U * (pre[1].double() + dbr).abs(), 'dbeta accumulated')
    ex = ExactWs(monkeypatch)
    dxa3, dg3, db3 = run_backward(row, inp, y_in, stats32, act, ps)
    ex.close()
    ck.true(same_bits(dxa3.t, dxa.t) and same_bits(dg3, dg) and same_bits(db3, db), 'exact workspace: other backward bits')
    ck.done()


def test_norm_workspace_query_covers_every_group_count(monkeypatch):
    """hv_norm_workspace_bytes has no `groups` argument: it has to cover every split of the batch.  B = 12, 209 x 209, C = 8 in four groups on the scalar
    path (an unaligned view) plans 4 x 512 chunks, more than the one-group plan (512) and the per-image plan (12 x 152)."""
    B, H, W, C, groups = 12, 209, 209, 8, 4
    ck = Check()
    gen = torch.Generator().manual_seed(77)
    x = (torch.randn(B, C, H, W, generator=gen) * 2 + torch.randn(1, C, 1, 1, generator=gen)).half()
    xa = T.to_act_view(x, 12, 2, SENT)
    dev = T.dev()
    z = torch.zeros(C, dtype=torch.float64)
    _, sr, _, _, _ = PR.norm_act_forward_ref(x.double(), 'batch', True, z + 1, z, None, None, EPS, MOM, groups, 'none', False)
    out = []
    for exact in (False, True):
        ex = ExactWs(monkeypatch) if exact else None
        stats = torch.full((groups, 2, C), float('nan'), device=dev)
        ops.norm_act_forward(xa, None, 'batch', True, stats, gamma=torch.ones(C, device=dev), beta=torch.zeros(C, device=dev), act='none', eps=EPS,
                             momentum=MOM, groups=groups)
        torch.cuda.synchronize()
        if ex:
            ex.close()
        out.append(stats)
    sd = out[0].cpu().double()
    ck.le('norm.mean', (sd[:, 0] - sr[:, 0]).abs(), 2 * U * sr[:, 0].abs() + 1e-12, 'mean')
    ck.le('norm.rstd', (sd[:, 1] - sr[:, 1]).abs(), 8 * U * sr[:, 1], 'rstd')
    ck.true(same_bits(out[0], out[1]), 'exact workspace: other bits')
    ck.done()


@pytest.mark.parametrize('f16', [False, True], ids=['f32', 'f16'])
@pytest.mark.parametrize('groups,per_image', [(1, 1), (2, 1), (2, 2), (1, 2)])
def test_norm_with_handed_over_partials(groups, per_image, f16):
    """Sums handed over as [n][C][2] fp32 partials (per image or per half image) instead of the reduction passes.  The partials are the fp64 sums rounded to
    fp32, so next to the statistics' own bounds stands the rounding of the inputs: u sum_k |partial_k|.  Derived bound of the variance: the partials of
    x^2 carry u E[x^2], the mean's error enters through 2 |mean| d(mean); rstd = (var + eps)^-1/2 turns d(var) into rstd^3 d(var) / 2."""
    B, H, W, C = 4, 6, 8, 16
    ck = Check()
    dev, dt = T.dev(), dtype_of(f16)
    gen = torch.Generator().manual_seed(31 + groups * 2 + per_image)
    r = lambda *s: torch.randn(*s, generator=gen)
    x = (r(B, C, H, W) * (2 + torch.rand(1, C, 1, 1, generator=gen)) + r(1, C, 1, 1)).to(dt)
    dy = (r(B, C, H, W) * (ops.grad_scale('fp16') if f16 else 1.0)).to(dt)
    gamma, beta = 1 + 0.25 * r(C), r(C)
    gamma[0], gamma[2] = -1.25, 0.0
    x64, dy64, g64, b64 = x.double(), dy.double(), gamma.double(), beta.double()
    n = B * per_image
    hh = H // per_image

    def partials(a, b):      # [n][C][2] of (sum a, sum b) over whole images or half images, image-major
        pa = a.view(B, C, per_image, hh * W).sum(dim=3).permute(0, 2, 1).reshape(n, C)
        pb = b.view(B, C, per_image, hh * W).sum(dim=3).permute(0, 2, 1).reshape(n, C)
        return torch.stack([pa, pb], dim=2).float().contiguous()

    rm0, rv0 = 0.25 * x64.mean(dim=(0, 2, 3)).float(), torch.ones(C) * 4
    yr, sr, rmr, rvr, nbt = PR.norm_act_forward_ref(x64, 'batch', True, g64, b64, rm0.double(), rv0.double(), EPS, MOM, groups, 'lrelu', False)
    fp = partials(x64, x64 * x64)
    xa, ya = T.to_act_view(x), T.to_act_view(torch.zeros_like(x))
    stats = torch.full((groups, 2, C), float('nan'), device=dev)
    rm, rv, nb = rm0.to(dev), rv0.to(dev), torch.zeros(1, dtype=torch.int64, device=dev)
    ops.norm_act_forward(xa, ya, 'batch', True, stats, gamma=gamma.to(dev), beta=beta.to(dev), running_mean=rm, running_var=rv, nbt=nb, act='lrelu',
                         eps=EPS, momentum=MOM, groups=groups, partials=fp.to(dev), n_partials=n)
    torch.cuda.synchronize()
    sd = stats.cpu().double()
    sl = PR.group_slices(B, 'batch', groups)
    y32, yextra = torch.empty_like(x64, dtype=torch.float32), torch.empty_like(x64)
    for k, s in enumerate(sl):
        R = (s.stop - s.start) * H * W
        ex, ex2 = x64[s].abs().sum(dim=(0, 2, 3)) / R, (x64[s] ** 2).sum(dim=(0, 2, 3)) / R
        dmean = 16 * U * ex + U * sr[k, 0].abs()
        dvar = 16 * U * ex2 + 2 * sr[k, 0].abs() * dmean
        drstd = 0.5 * sr[k, 1] ** 3 * dvar + 8 * U * sr[k, 1]
        ck.le('partials.mean', (sd[k, 0] - sr[k, 0]).abs(), dmean, 'mean')
        ck.le('partials.rstd', (sd[k, 1] - sr[k, 1]).abs(), drstd, 'rstd')
        # y at the reference statistics; the statistics' own allowance reaches y through |gamma| (rstd d(mean) + |x - mean| d(rstd)): lrelu has slope <= 1
        y32[s] = PR.norm_apply_formula(x64[s].float(), sr[k, 0].float(), sr[k, 1].float(), gamma, beta, 'lrelu', False)
        yextra[s] = g64.abs().view(1, C, 1, 1) * ((sr[k, 1] * dmean).view(1, C, 1, 1) + (x64[s] - sr[k, 0].view(1, C, 1, 1)).abs() * drstd.view(1, C, 1, 1))
    ck.true(nb.item() == nbt, 'num_batches_tracked')
    ck.le('partials.y', (T.from_act(ya).double() - yr).abs(), tol_elem(yr, (y32.double() - yr).abs().max().item(), f16) + yextra, 'y')

    # backward, act none: (sum g, sum g xhat) handed over
    stats32 = sr.float()
    st64 = stats32.double()
    dxr, dgr, dbr = PR.norm_act_backward_ref(dy64, yr, x64, st64, g64, 'batch', True, groups, 'none', False)
    g, xhat = PR.norm_backward_terms(dy64, yr, x64, st64, 'batch', groups, 'none', False)
    bp = partials(g, g * xhat)
    dxa = T.to_act_view(torch.zeros_like(x))
    dg, db = torch.full((C,), float('nan'), device=dev), torch.full((C,), float('nan'), device=dev)
    nan_y = T.to_act_view(torch.full_like(x, float('nan')))
    ops.norm_act_backward(T.to_act_view(dy), nan_y, xa, dxa, 'batch', True, stats32.to(dev), gamma=gamma.to(dev), act='none', dgamma=dg, dbeta=db,
                          groups=groups, partials=bp.to(dev), n_partials=n)
    torch.cuda.synchronize()
    dx32 = torch.empty_like(y32)
    extra = torch.empty_like(x64)
    for k, s in enumerate(sl):
        R = (s.stop - s.start) * H * W
        sg, sgx = g[s].sum(dim=(0, 2, 3)), (g[s] * xhat[s]).sum(dim=(0, 2, 3))
        dx32[s] = PR.norm_bwd_apply_formula(dy64[s].float(), x64[s].float(), stats32[k, 0], stats32[k, 1], gamma, sg.float(), sgx.float(), R, True)
        pk = bp.double().view(B, per_image, C, 2)[s].abs().sum(dim=(0, 1))      # [C][2]: sum_k |partial_k| of the group
        extra[s] = (g64 * st64[k, 1]).abs().view(1, C, 1, 1) * U * (pk[:, 0].view(1, C, 1, 1) + xhat[s].abs() * pk[:, 1].view(1, C, 1, 1)) / R
    ck.le('partials.dx', (T.from_act(dxa).double() - dxr).abs(), tol_elem(dxr, (dx32.double() - dxr).abs().max().item(), f16) + extra, 'dx')
    bgam = torch.zeros(C, dtype=torch.float64)
    for k, s in enumerate(sl):
        bgam += (g[s].abs() * (xhat[s].abs() + (st64[k, 0].abs() * st64[k, 1]).view(1, C, 1, 1))).sum(dim=(0, 2, 3))
    ck.le('partials.dgamma', (dg.cpu().double() - dgr).abs(), 16 * U * bgam + U * dgr.abs(), 'dgamma')
    ck.le('partials.dbeta', (db.cpu().double() - dbr).abs(), 16 * U * g.abs().sum(dim=(0, 2, 3)) + U * dbr.abs(), 'dbeta')
    ck.done()


def test_norm_partials_refusals():
    """Refused by the host code before anything is launched."""
    B, H, W, C = 4, 4, 4, 16
    dev = T.dev()
    x = torch.randn(B, C, H, W)
    xa, ya = T.to_act_view(x), T.to_act_view(torch.zeros_like(x))
    one, stats = torch.ones(C, device=dev), torch.zeros(2, 2, C, device=dev)
    part = torch.zeros(8, C, 2, device=dev)
    with pytest.raises(RuntimeError, match='HV_ERR_ARG'):      # three partials do not divide into two groups
        ops.norm_act_forward(xa, ya, 'batch', True, stats, gamma=one, beta=one, groups=2, partials=part, n_partials=3)
    with pytest.raises(RuntimeError, match='HV_ERR_ARG'):      # six divide into the groups, but not into whole images per group
        ops.norm_act_forward(xa, ya, 'batch', True, stats, gamma=one, beta=one, groups=2, partials=part, n_partials=6)
    bw = dict(gamma=one, dgamma=torch.zeros(C, device=dev), dbeta=torch.zeros(C, device=dev), groups=2, partials=part)
    with pytest.raises(RuntimeError, match='HV_ERR_ARG'):      # backward partials with an activation
        ops.norm_act_backward(ya, ya, xa, T.to_act_view(torch.zeros_like(x)), 'batch', True, stats, act='relu', n_partials=4, **bw)
    with pytest.raises(RuntimeError, match='HV_ERR_ARG'):      # ... in eval mode
        ops.norm_act_backward(ya, ya, xa, T.to_act_view(torch.zeros_like(x)), 'batch', False, stats, act='none', n_partials=4, **bw)
    with pytest.raises(RuntimeError, match='HV_ERR_ARG'):      # ... not divisible into the groups
        ops.norm_act_backward(ya, ya, xa, T.to_act_view(torch.zeros_like(x)), 'batch', True, stats, act='none', n_partials=3, **bw)
    torch.cuda.synchronize()


def test_norm_refuses_24_channels():
    """Channels 8 .. 32 of a buffer are 24 channels: neither quad-shaped (C / 4 a power of two) nor a power of two.  Both entries refuse that before any
    launch; the slice-view row above therefore runs 32 channels at offset 8."""
    dev = T.dev()
    x = torch.randn(2, 24, 6, 5)
    xa, ya, dxa = T.to_act_view(x, 48, 8), T.to_act_view(torch.zeros_like(x), 56, 8), T.to_act_view(torch.zeros_like(x), 40, 8)
    one, stats = torch.ones(24, device=dev), torch.zeros(1, 2, 24, device=dev)
    with pytest.raises(RuntimeError, match='HV_ERR_UNSUPPORTED'):
        ops.norm_act_forward(xa, ya, 'batch', True, stats, gamma=one, beta=one)
    with pytest.raises(RuntimeError, match='HV_ERR_UNSUPPORTED'):
        ops.norm_act_backward(T.to_act_view(x, 64, 8), ya, xa, dxa, 'batch', True, stats, gamma=one)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- activation gradient
def act_outputs(v, act, dt):
    """A plausible stored y: act(v) evaluated in fp32 and rounded to the storage type."""
    return PR.act_formula(v, act).to(dt)


def reduce_bound(gabs_sum, ref, npix):
    depth = math.ceil(math.log2(npix)) + 16 if npix > 1 else 16
    return (16 + depth) * U * gabs_sum + U * ref.abs()


ACT_ACTS = ('elu', 'relu', 'lrelu', 'sigmoid', 'clamp')
ACT_BIG = {1: 2 * 1024 * 1024 + 3, 2: 1024 * 1024 + 5, 4: 2 * 1024 * 1024 + 3, 64: 140003, 1024: 8195}


def act_case(ck, monkeypatch, C, npix, act, dy16, y16, accumulate, views=False, exact=False, seed=0):
    dev = T.dev()
    gen = torch.Generator().manual_seed(seed)
    dy = (torch.randn(1, C, 1, npix, generator=gen) * (ops.grad_scale('fp16') if dy16 else 1.0)).to(dtype_of(dy16))
    y = act_outputs(torch.randn(1, C, 1, npix, generator=gen) * 1.5, act, dtype_of(y16))
    gr, dbr = PR.act_backward_ref(dy.double(), y.double(), act)
    floor = ((dy.float() * PR.act_grad_from_out_formula(y.float(), act)).double() - gr).abs().max().item()
    pre = torch.linspace(-2, 2, C) if accumulate else torch.full((C,), float('nan'))
    want = dbr + pre.double() if accumulate else dbr
    outs = []
    for ws_exact in ((False, True) if exact else (False,)):
        dya = T.to_act_view(dy, C + 16, 8, SENT) if views else T.to_act_view(dy)
        ya = T.to_act_view(y, C + 8, 4, SENT) if views else T.to_act_view(y)
        y_before = ya.t.clone()
        dbias = pre.to(dev)
        ex = ExactWs(monkeypatch) if ws_exact else None
        ops.act_backward(dya, ya, act, dbias=dbias, dbias_accumulate=accumulate)
        torch.cuda.synchronize()
        if ex:
            ex.close()
        outs.append((dya.t, dbias))
        if not ws_exact:
            what = 'C=%d npix=%d %s dy16=%d y16=%d' % (C, npix, act, dy16, y16)
            ck.le('act.g', (T.from_act(dya).double() - gr).abs(), tol_elem(gr, floor, dy16), what)
            ck.le('act.dbias', (dbias.cpu().double() - want).abs(), reduce_bound(gr.abs().sum(dim=(0, 2, 3)), dbr, npix) + (U * want.abs() if accumulate else 0), what)
            ck.true(same_bits(ya.t, y_before), 'y changed: ' + what)
            if views:
                ck.true(others_untouched(dya), 'channels around dy changed: ' + what)
    if exact:
        ck.true(same_bits(outs[0][0], outs[1][0]) and same_bits(outs[0][1], outs[1][1]), 'exact workspace: other bits (C=%d npix=%d)' % (C, npix))


@pytest.mark.parametrize('dy16,y16', [(False, False), (True, True), (True, False), (False, True)], ids=['f32-f32', 'f16-f16', 'f16-f32', 'f32-f16'])
@pytest.mark.parametrize('C', [1, 2, 4, 64, 1024])
def test_act_backward(C, dy16, y16, monkeypatch):
    ck = Check()
    rstep = 256 // (C // 4) if C % 4 == 0 else 256 // C
    k = 0
    for npix in (1, 5, 4 * rstep - 1, 4 * rstep + 1):
        for act in ACT_ACTS:
            act_case(ck, monkeypatch, C, npix, act, dy16, y16, accumulate=bool(k & 1), exact=(act == ACT_ACTS[k // 5 % 5]), seed=k)
            k += 1
    if C % 4 == 0 and C <= 64:
        act_case(ck, monkeypatch, C, 4 * rstep + 1, 'elu', dy16, y16, accumulate=False, views=True, exact=True, seed=99)
    if dy16 != y16:      # the 2048-block cap re-sizes rows_per_block
        act_case(ck, monkeypatch, C, ACT_BIG[C], ACT_ACTS[[1, 2, 4, 64, 1024].index(C)], dy16, y16, accumulate=False, exact=True, seed=123)
    ck.done()


def test_act_backward_refuses_quad_channels_on_an_unaligned_view():
    dy, y = torch.randn(1, 4, 1, 9), torch.randn(1, 4, 1, 9)
    with pytest.raises(RuntimeError, match='HV_ERR_UNSUPPORTED'):
        ops.act_backward(T.to_act_view(dy, 8, 2), T.to_act_view(y, 8, 2), 'relu')
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- head seed
@pytest.mark.parametrize('y_ld', [1, 4])
@pytest.mark.parametrize('y16', [False, True], ids=['y32', 'y16'])
def test_head_seed_backward(y16, y_ld, monkeypatch):
    ck = Check()
    dev = T.dev()
    k = 0
    for npix in (1, 3, 4, 1023, 1024, 1025, 4099):
        for act in ('none', 'sigmoid', 'clamp'):
            gen = torch.Generator().manual_seed(500 + k)
            seed = torch.randn(npix, generator=gen) * ops.grad_scale('fp16')
            y = act_outputs(torch.randn(1, 1, 1, npix, generator=gen) * 1.5, act, dtype_of(y16))
            gr = PR.head_seed_ref(seed.double(), y.double().view(-1), act)
            floor = ((seed * PR.act_grad_from_out_formula(y.float().view(-1), act)).double() - gr).abs().max().item()
            accumulate = bool(k & 1)
            pre = torch.tensor([1.5]) if accumulate else torch.tensor([float('nan')])
            outs = []
            for ws_exact in (False, True):
                ya = T.to_act_view(y, y_ld, y_ld - 1, SENT)
                carrier = ops.Act(torch.full((1, 1, npix, 4), SENT, dtype=torch.float16, device=dev), 4, 0)
                dbias = pre.to(dev)
                ex = ExactWs(monkeypatch) if ws_exact else None
                ops.head_seed_backward(seed.to(dev), ya, carrier, act, dbias=dbias, dbias_accumulate=accumulate)
                torch.cuda.synchronize()
                if ex:
                    ex.close()
                outs.append((carrier.t, dbias))
            what = 'npix=%d %s' % (npix, act)
            c = outs[0][0].cpu().view(npix, 4)
            ck.true(bool((c[:, 1:] == 0).all()), 'carrier channels 1-3 not zero: ' + what)
            held = c[:, 0].double()
            ck.le('seed.g', (held - gr).abs(), tol_elem(gr, floor, True), what)
            want = held.sum() + (pre.double()[0] if accumulate else 0.0)      # the bias gradient sums what the carrier holds
            mag = (gr.abs() + tol_elem(gr, floor, True)).sum()      # |stored value| <= |ref| + its tolerance: the bound takes no magnitude from the device
            ck.le('seed.dbias', (outs[0][1].cpu().double()[0] - want).abs(), reduce_bound(mag, mag, npix) + (U * (mag + abs(float(pre[0]))) if accumulate else 0), what)
            ck.true(same_bits(outs[0][0], outs[1][0]) and same_bits(outs[0][1], outs[1][1]), 'exact workspace: other bits: ' + what)
            k += 1
    ck.done()


# ---------------------------------------------------------------------------------------------------------------- GAN loss heads
PLANTED = [0.0, 1e-4, -1e-4, 30.0, -30.0, 90.0, -90.0]
MODE_ID = {'vanilla': 0, 'lsgan': 1}


def logits(n, seed, small=False):
    gen = torch.Generator().manual_seed(seed)
    z = torch.randn(n, generator=gen) * (0.5 if small else 3.0)
    if n > 2 * len(PLANTED) and not small:
        z[torch.randperm(n, generator=gen)[:len(PLANTED)]] = torch.tensor(PLANTED)
    return z


def loss_refs(z, real, mode, lw, gw):
    """-> lw * loss, its bound 64u (lw / n) sum |l_i|, gw * dz, and the floor of gw * dz in fp32."""
    n = z.numel()
    loss, dz = PR.gan_loss_ref(z.double(), real, mode)
    l, _ = PR.gan_loss_terms_formula(z.double(), real, mode)
    _, g32 = PR.gan_loss_terms_formula(z, real, mode)
    dz32 = torch.tensor(gw, dtype=torch.float32) * g32 / torch.tensor(float(n), dtype=torch.float32)
    return lw * loss, 64 * U * (lw / n) * l.abs().sum(), gw * dz, (dz32.double() - gw * dz).abs().max().item()


def call_gan(entry, z, real, mode, lw, loss, acc, gw, dz, monkeypatch=None):
    L, ptr, stream = lib.get(), lib.ptr, lib.stream
    n = z.numel()
    if entry == 'ops':
        return ops.gan_loss(z, real, mode, loss=loss, loss_weight=lw, loss_accumulate=acc, dz=dz, grad_weight=gw)
    head = (ptr(z), ctypes.c_longlong(n), int(real), MODE_ID[mode], ctypes.c_float(lw), ptr(loss), int(acc), ctypes.c_float(gw), ptr(dz))
    if entry == 'hv_gan_loss':
        return L.call('hv_gan_loss', *head, stream())
    need = L.size('hv_gan_loss_workspace_bytes', ctypes.c_longlong(n))
    ex = ExactWs(monkeypatch)
    b, nb = ops._ws(need, z.device)
    L.call('hv_gan_loss_ws', *head, ptr(b), nb, stream())
    ex.close()


@pytest.mark.parametrize('real', [True, False], ids=['real', 'fake'])
@pytest.mark.parametrize('mode', ['vanilla', 'lsgan'])
def test_gan_loss(mode, real, monkeypatch):
    ck = Check()
    dev = T.dev()
    lw, gw = 0.75, 1.5
    runs = [('ops', n) for n in (1, 255, 256, 257, 4095, 4096, 14400)] + [('hv_gan_loss', 16385), ('hv_gan_loss', 14400), ('hv_gan_loss_ws', 255),
                                                                           ('hv_gan_loss_ws', 16385)]
    for k, (entry, n) in enumerate(runs):
        z = logits(n, 700 + k)
        lr, lb, dzr, floor = loss_refs(z, real, mode, lw, gw)
        zd = z.to(dev)
        what = '%s n=%d' % (entry, n)
        loss, dz = torch.full((1,), float('nan'), device=dev), torch.full((n,), float('nan'), device=dev)
        call_gan(entry, zd, real, mode, lw, loss, False, gw, dz, monkeypatch)
        torch.cuda.synchronize()
        ck.le('gan.loss', (loss.cpu().double()[0] - lr).abs(), lb, what)
        ck.le('gan.dz', (dz.cpu().double() - dzr).abs(), tol_elem(dzr, floor, False), what)
        acc = torch.full((1,), 2.25, device=dev)
        call_gan(entry, zd, real, mode, lw, acc, True, gw, None, monkeypatch)      # accumulate, no dz
        torch.cuda.synchronize()
        ck.le('gan.loss', (acc.cpu().double()[0] - (2.25 + lr)).abs(), lb + U * abs(2.25 + lr), what + ' accumulated')
        only = torch.full((1,), float('nan'), device=dev)
        call_gan(entry, zd, real, mode, lw, only, False, gw, None, monkeypatch)
        torch.cuda.synchronize()
        ck.true(same_bits(only, loss), 'dz=None: other loss bits: ' + what)
    ck.done()


@pytest.mark.parametrize('real', [True, False], ids=['real', 'fake'])
@pytest.mark.parametrize('mode', ['vanilla', 'lsgan'])
def test_gan_loss_head(mode, real, monkeypatch):
    """hv_gan_loss_head, the unpaired head: loss, optional fp32 dz, d loss / d logit in the fp16 carrier and the bias gradient = the sum of what the carrier
    holds, with a workspace of exactly hv_gan_loss_head_workspace_bytes(n) inside a sentinel buffer."""
    ck = Check()
    dev = T.dev()
    L, ptr, stream = lib.get(), lib.ptr, lib.stream
    lw, gw = 0.75, ops.grad_scale('fp16')
    k = 0
    for n in (1, 200, 256, 257, 1800):
        z = logits(n, 800 + n, small=n < 16)
        lr, lb, dzr, floor = loss_refs(z, real, mode, lw, gw)
        zd = z.to(dev)
        for give_dz, accumulate in ((True, False), (False, True)):
            what = '%s n=%d dz=%d acc=%d' % (mode, n, give_dz, accumulate)
            pre_l, pre_b = (2.25, 3.0) if accumulate else (float('nan'), float('nan'))
            loss, dbias = torch.full((1,), pre_l, device=dev), torch.full((1,), pre_b, device=dev)
            dz = torch.full((n,), float('nan'), device=dev) if give_dz else None
            carrier = torch.full((n, 4), SENT, dtype=torch.float16, device=dev)
            ex = ExactWs(monkeypatch)
            b, nb = ops._ws(L.size('hv_gan_loss_head_workspace_bytes', ctypes.c_longlong(n)), dev)
            L.call('hv_gan_loss_head', ptr(zd), ctypes.c_longlong(n), int(real), MODE_ID[mode], ctypes.c_float(lw), ptr(loss), int(accumulate),
                   ctypes.c_float(gw), ptr(dz), ptr(carrier), ptr(dbias), int(accumulate), ptr(b), nb, stream())
            ex.close()
            c = carrier.cpu()
            ck.true(bool((c[:, 1:] == 0).all()), 'carrier channels 1-3 not zero: ' + what)
            held = c[:, 0].double()
            ck.le('head.carrier', (held - dzr).abs(), tol_elem(dzr, floor, True), what)
            if give_dz:
                ck.le('head.dz', (dz.cpu().double() - dzr).abs(), tol_elem(dzr, floor, False), what)
            want_l = lr + (pre_l if accumulate else 0.0)
            ck.le('head.loss', (loss.cpu().double()[0] - want_l).abs(), lb + (U * abs(want_l) if accumulate else 0), what)
            mag = (dzr.abs() + tol_elem(dzr, floor, True)).sum()      # |stored value| <= |ref| + its tolerance
            want_b = held.sum() + (pre_b if accumulate else 0.0)      # the bias gradient sums what the carrier holds
            ck.le('head.dbias', (dbias.cpu().double()[0] - want_b).abs(), reduce_bound(mag, mag, n) + (U * (mag + abs(pre_b)) if accumulate else 0), what)
            k += 1
    # loss and dbias both absent: only the carrier is written
    carrier = torch.full((n, 4), SENT, dtype=torch.float16, device=dev)
    ex = ExactWs(monkeypatch)
    b, nb = ops._ws(L.size('hv_gan_loss_head_workspace_bytes', ctypes.c_longlong(n)), dev)
    L.call('hv_gan_loss_head', ptr(zd), ctypes.c_longlong(n), int(real), MODE_ID[mode], ctypes.c_float(lw), None, 0, ctypes.c_float(gw), None, ptr(carrier),
           None, 0, ptr(b), nb, stream())
    ex.close()
    ck.true(same_bits(carrier.cpu(), c), 'no loss, no dbias: other carrier bits')
    ck.done()


@pytest.mark.parametrize('real0,real1', [(True, False), (False, True)], ids=['real-fake', 'fake-real'])
@pytest.mark.parametrize('mode', ['vanilla', 'lsgan'])
def test_gan_loss_pair(mode, real0, real1):
    ck = Check()
    dev = T.dev()
    lw, gw = 0.75, ops.grad_scale('fp16')
    k = 0
    for n0, n1 in ((1800, 1800), (257, 0), (1, 255), (14400, 14400)):
        for give_loss1, accumulate in ((True, False), (False, True)):
            zs = [logits(n, 900 + 2 * k + i, small=n < 16) for i, n in enumerate((n0, n1)) if n]
            reals = (real0, real1)
            refs = [loss_refs(z, reals[i], mode, lw, gw) for i, z in enumerate(zs)]
            zd = [z.to(dev) for z in zs]
            pre = 3.0 if accumulate else float('nan')
            outs = []
            for rep in range(3):      # three launches in a row on one stream: the ticket has to come back to zero each time
                car = [ops.Act(torch.full((1, 1, z.numel(), 4), SENT, dtype=torch.float16, device=dev), 4, 0) for z in zs]
                losses = [torch.full((1,), float('nan'), device=dev) for _ in zs]
                dbias = torch.full((1,), pre, device=dev)
                two = len(zs) == 2
                ops.gan_loss_pair(zd[0], real0, losses[0], car[0], z1=zd[1] if two else None, real1=real1, loss1=losses[1] if (two and give_loss1) else None,
                                  carrier1=car[1] if two else None, mode=mode, loss_weight=lw, grad_weight=gw, dbias=dbias, dbias_accumulate=accumulate)
                outs.append((car, losses, dbias))
            torch.cuda.synchronize()
            what = '%s n=(%d,%d) loss1=%d acc=%d' % (mode, n0, n1, give_loss1, accumulate)
            ck.true(bool((ops._ticket(dev) == 0).all()), 'ticket not back at zero: ' + what)
            for rep in (1, 2):
                same = all(same_bits(a.t, b.t) for a, b in zip(outs[0][0], outs[rep][0])) and same_bits(outs[0][2], outs[rep][2]) and \
                    all(same_bits(a, b) for a, b in zip(outs[0][1], outs[rep][1]))
                ck.true(same, 'launch %d: other bits: %s' % (rep, what))
            car, losses, dbias = outs[0]
            held_sum, mag = 0.0, 0.0
            for i, (lr, lb, dzr, floor) in enumerate(refs):
                c = car[i].t.cpu().view(-1, 4)
                ck.true(bool((c[:, 1:] == 0).all()), 'carrier channels 1-3 not zero: ' + what)
                held = c[:, 0].double()
                ck.le('pair.carrier', (held - dzr).abs(), tol_elem(dzr, floor, True), what)
                held_sum, mag = held_sum + held.sum(), mag + (dzr.abs() + tol_elem(dzr, floor, True)).sum()      # |stored| <= |ref| + its tolerance
                if i == 0 or give_loss1:
                    ck.le('pair.loss', (losses[i].cpu().double()[0] - lr).abs(), lb, what)
                else:
                    ck.true(bool(torch.isnan(losses[i]).all()), 'loss1=None, yet a loss slot was written: ' + what)
            want = held_sum + (pre if accumulate else 0.0)
            ck.le('pair.dbias', (dbias.cpu().double()[0] - want).abs(),
                  reduce_bound(mag, mag, n0 + n1) + (U * (mag + abs(pre)) if accumulate else 0), what)
            k += 1
    ck.done()
