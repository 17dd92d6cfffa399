"""The contextual-attention glue kernels of csrc/attention.hip, called through the C entries, against the fp64 references of tests/attention_ref.py (pinned by
tests/test_attention_ref_cpu.py), at the shapes where the entries switch kernels.  The library records no kernel path for these entries
(hv_last_kernel_path is set by the convolution launchers only), so every test names the branch its shapes reach; the rules are those of the entry points.

Every output lies in a sentinel-filled buffer with guards on both sides (hvtest.Guarded); the guards, and the channels beside a view, must stay intact.
Every bound is computed from fp64 reference quantities and u = 2^-24, never from the kernel's output:
  copies (patch tables, mask, transpose)   bit for bit
  norm, rnorm                              (9C + 2) u ref: an fp32 sum of 9C non-negative terms in any order, the square root and the reciprocal
  fuse                                     9u sum |terms|
  soft-max A                               4 x (largest error of a plain fp32 torch evaluation on the CPU) + 4u |ref|, + max(2^-11 |ref|, 2^-25) stored as fp16
  soft-max dS                              scale mm |A| (16u sum |dA A| + 4u (|dA| + |dot|)) + the element rule above
  Gs                                       3u (|dS[j][i] r_i| + |dS[i][j] r_j|)
  coef                                     (16u sum |dS S0| + 4u |sum|) / norm^2
  col2im                                   18u sum |terms| (the prior content counts as a term when accumulating)
The worst error / bound ratio of every family is printed at the end of the module (pytest -s)."""
import ctypes

import numpy as np
import pytest
import torch

import attention_ref as AR

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
F64 = torch.float64
FLOOR32 = float(np.float32(1e-4))      # the norm's floor as the kernels hold it
RATIOS = {}
T = lib = None


@pytest.fixture(scope='module', autouse=True)
def _env():
    global T, lib
    import hvgan  # noqa: F401
    from hvgan import lib as _lib
    import hvtest as _T
    T, lib = _T, _lib
    yield
    print('\nworst error / bound per family')
    for k in sorted(RATIOS):
        print('  %-22s %.3e' % (k, RATIOS[k]))


class Check:
    """Collects the comparisons of one test; every failure is reported, the worst error / bound ratio per family is recorded."""

    def __init__(self):
        self.fails = []

    def le(self, family, err, bound, what=''):
        err, bound = torch.as_tensor(err, dtype=F64), torch.as_tensor(bound, dtype=F64)
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


def same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    return a.dtype == b.dtype and a.shape == b.shape and bool((a.view(torch.uint8) == b.view(torch.uint8)).all())


def call(name, *args):
    lib.get().call(name, *args, lib.stream())
    torch.cuda.synchronize()


def rc_of(name, *args):
    return getattr(lib.get().cdll, name)(*args, lib.stream())


def P(x):
    return lib.ptr(x.t if hasattr(x, 'intact') else x)


def f32c(v):
    return ctypes.c_float(v)


def ll(v):
    return ctypes.c_longlong(int(v))


HV_ERR_ARG, HV_ERR_UNSUPPORTED = -1, -2


# ---------------------------------------------------------------------------------------------------------------- patch tables
# name: (B, H, W, C, f_ld, source stored as fp16, base offset of every fp32 output in floats, kernel of the fp32 tables)
PATCH_ROWS = {
    'tile_one_partial_tile': (2, 12, 8, 8, 8, False, 0, 'tile'),       # L = 24 < 64 rows, C = 8 < 64 channels
    'tile_two_by_two': (1, 20, 16, 68, 68, False, 0, 'tile'),          # L = 80: 64 + 16 rows; 64 + 4 channels
    'elem_c6': (2, 12, 8, 6, 6, False, 0, 'element'),                  # C % 4 != 0
    'elem_ld10': (2, 12, 8, 8, 10, False, 0, 'element (raw); tile (wp: fd is dense)'),      # f_ld % 4 != 0
    'elem_offset': (2, 12, 8, 8, 8, False, 1, 'element'),              # outputs one float off 16 bytes
    'f16_source': (2, 12, 8, 8, 16, True, 0, 'tile'),
}


def patch_source(name):
    """The stored map [B][H][W][f_ld] (channels beyond C hold 7.5) with one 3x3 block of down-sampled pixels zero, and its fp32 value over the C channels."""
    B, H, W, C, ld, f16, off, _ = PATCH_ROWS[name]
    gen = torch.Generator().manual_seed(100 + sorted(PATCH_ROWS).index(name))
    f = torch.randn(B, H, W, C, generator=gen) * (1 + torch.rand(C, generator=gen))
    f[:, 2:8:2, 2:8:2, :] = 0                        # down-sampled pixels (1..3, 1..3): the patch at (2, 2) is all zero
    f = f.to(torch.float16 if f16 else torch.float32)
    st = torch.full((B, H, W, ld), 7.5, dtype=f.dtype)
    st[..., :C] = f
    return st, f.float()


@pytest.mark.parametrize('name', sorted(PATCH_ROWS))
def test_patch_tables_are_copies_and_norms_are_bounded(name):
    """hv_ca_patches (with and without wpT), hv_ca_patches_h, hv_ca_raw_patches (raw, rawT, both) and hv_ca_raw_patches_f16.  C % 4, f_ld % 4 and 16-byte bases
    choose ca_patch_tile_kernel or ca_wp_kernel / ca_raw_kernel (PATCH_ROWS names the side)."""
    B, H, W, C, ld, f16, off, _ = PATCH_ROWS[name]
    h, w = H // 2, W // 2
    L = h * w
    ck = Check()
    st, f = patch_source(name)
    fdev = T.Guarded(st.shape, st.dtype, data=st)
    fd_r = AR.down(f)
    wp_r, wpT_r = AR.patches3(fd_r)
    raw_r, rawT_r = AR.raw_patches4(f)
    n_r, rn_r = AR.norms(wp_r.double(), FLOOR32)
    zero_row = w * 2 + 2
    assert bool((wp_r[:, zero_row] == 0).all()) and float(n_r[0, zero_row]) == FLOOR32

    def outs(with_T=True):
        o = dict(fd=T.Guarded((B, h, w, C), offset=off), wp=T.Guarded((B, L, 9, C), offset=off), norm=T.Guarded((B, L), offset=off), rnorm=T.Guarded((B, L), offset=off))
        if with_T:
            o['wpT'] = T.Guarded((B, 9 * C, L), offset=off)
        return o

    def check_patches(o, what):
        ck.true(same_bits(o['fd'].cpu(), fd_r), what + ': fd')
        ck.true(same_bits(o['wp'].cpu(), wp_r), what + ': wp')
        if 'wpT' in o:
            ck.true(same_bits(o['wpT'].cpu(), wpT_r), what + ': wpT')
        bound = (9 * C + 2) * U
        ck.le('patches.norm', (o['norm'].cpu().double() - n_r).abs(), bound * n_r, what + ': norm')
        ck.le('patches.norm', (o['rnorm'].cpu().double() - rn_r).abs(), bound * rn_r, what + ': rnorm')
        one, floor = torch.tensor(1.0), torch.tensor(1e-4, dtype=torch.float32)
        ck.true(bool((o['norm'].cpu()[:, zero_row] == floor).all()) and bool((o['rnorm'].cpu()[:, zero_row] == one / floor).all()), what + ': floor of the all-zero patch')
        ck.true(all(g.intact() for g in o.values()), what + ': guards')

    a = outs()
    call('hv_ca_patches', P(fdev), int(f16), B, H, W, C, ld, P(a['fd']), P(a['wp']), P(a['wpT']), P(a['norm']), P(a['rnorm']))
    check_patches(a, 'hv_ca_patches')
    b = outs(with_T=False)
    call('hv_ca_patches', P(fdev), int(f16), B, H, W, C, ld, P(b['fd']), P(b['wp']), None, P(b['norm']), P(b['rnorm']))
    check_patches(b, 'hv_ca_patches without wpT')
    ck.true(all(same_bits(a[k].t, b[k].t) for k in b), 'wpT = NULL: other bits')

    c = outs(with_T=False)
    wp_h = T.Guarded((B, L, 9, C), torch.float16)
    args = (P(fdev), int(f16), B, H, W, C, ld, P(c['fd']), P(c['wp']), P(wp_h), P(c['norm']), P(c['rnorm']))
    if C % 4 or off:
        ck.true(rc_of('hv_ca_patches_h', *args) == HV_ERR_UNSUPPORTED, 'hv_ca_patches_h: not refused')
    else:
        call('hv_ca_patches_h', *args)
        check_patches(c, 'hv_ca_patches_h')
        ck.true(same_bits(wp_h.cpu(), wp_r.half()) and wp_h.intact(), 'wp_h')

    if not f16:      # hv_ca_raw_patches reads an fp32 map
        got = {}
        for want_raw, want_T in ((True, False), (False, True), (True, True)):
            raw, rawT = T.Guarded((B, L, 16, C), offset=off), T.Guarded((B, C, 16, L), offset=off)
            call('hv_ca_raw_patches', P(fdev), B, H, W, C, ld, P(raw) if want_raw else None, P(rawT) if want_T else None)
            what = 'hv_ca_raw_patches raw=%d rawT=%d' % (want_raw, want_T)
            ck.true(same_bits(raw.cpu(), raw_r) if want_raw else bool(torch.isnan(raw.cpu()).all()), what + ': raw')
            ck.true(same_bits(rawT.cpu(), rawT_r) if want_T else bool(torch.isnan(rawT.cpu()).all()), what + ': rawT')
            ck.true(raw.intact() and rawT.intact(), what + ': guards')
        rc = rc_of('hv_ca_raw_patches', P(fdev), B, H, W, C, ld, None, None)
        ck.true(rc == HV_ERR_ARG, 'hv_ca_raw_patches without an output: %d' % rc)

    raw_h, rawT_h = T.Guarded((B, L, 16, C), torch.float16), T.Guarded((B, C, 16, L), torch.float16)
    args = (P(fdev), int(f16), B, H, W, C, ld, P(raw_h), P(rawT_h))
    if C % 4 or ld % 4:
        ck.true(rc_of('hv_ca_raw_patches_f16', *args) == HV_ERR_UNSUPPORTED, 'hv_ca_raw_patches_f16: not refused')
    else:
        call('hv_ca_raw_patches_f16', *args)
        ck.true(same_bits(raw_h.cpu(), raw_r.half()) and same_bits(rawT_h.cpu(), rawT_r.half()), 'hv_ca_raw_patches_f16')
        ck.true(raw_h.intact() and rawT_h.intact(), 'hv_ca_raw_patches_f16: guards')
    ck.true(same_bits(fdev.cpu(), st) and fdev.intact(), 'the source changed')
    ck.done()


def test_patch_entries_refuse_what_they_do_not_serve():
    """C = 6 has no fp16 tables (HV_ERR_UNSUPPORTED, nothing launched); an odd H is an argument error in every entry."""
    B, H, W, C = 1, 12, 8, 6
    L = (H // 2) * (W // 2)
    f = T.Guarded((B, H + 1, W, 8), data=torch.zeros(B, H + 1, W, 8))
    o = [T.Guarded((B, L, 16, 8)) for _ in range(6)]
    h16 = [T.Guarded((B, L, 16, 8), torch.float16) for _ in range(2)]
    assert rc_of('hv_ca_patches_h', P(f), 0, B, H, W, C, C, P(o[0]), P(o[1]), P(h16[0]), P(o[2]), P(o[3])) == HV_ERR_UNSUPPORTED
    assert rc_of('hv_ca_raw_patches_f16', P(f), 0, B, H, W, C, C, P(h16[0]), P(h16[1])) == HV_ERR_UNSUPPORTED
    for CC in (6, 8):
        assert rc_of('hv_ca_patches', P(f), 0, B, H + 1, W, CC, CC, P(o[0]), P(o[1]), P(o[4]), P(o[2]), P(o[3])) == HV_ERR_ARG
        assert rc_of('hv_ca_patches_h', P(f), 0, B, H + 1, W, CC, CC, P(o[0]), P(o[1]), P(h16[0]), P(o[2]), P(o[3])) == HV_ERR_ARG
        assert rc_of('hv_ca_raw_patches', P(f), B, H + 1, W, CC, CC, P(o[0]), P(o[1])) == HV_ERR_ARG
        assert rc_of('hv_ca_raw_patches_f16', P(f), 0, B, H + 1, W, CC, CC, P(h16[0]), P(h16[1])) == HV_ERR_ARG
        assert rc_of('hv_ca_patches_backward', P(o[0]), P(o[1]), P(o[2]), P(o[3]), B, H + 1, W, CC, CC, 1) == HV_ERR_ARG
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(g.cpu()).all()) and g.intact() for g in o + h16)


# ---------------------------------------------------------------------------------------------------------------- mask
@pytest.mark.parametrize('Himg,Wimg,h,w', [(64, 64, 8, 8), (48, 64, 6, 8)])
def test_patch_mask_single_and_batched(Himg, Wimg, h, w):
    """hv_ca_mask / hv_ca_mask_batched (ca_mask_kernel): ones on a sampled pixel (8y, 8x), on unsampled neighbours (ignored), in a corner and on an edge;
    B = 3 masks that differ, a batch stride larger than an image; the one-sample form = sample 0 of the batched one."""
    B, L = 3, h * w
    stride = Himg * Wimg + 24
    mask = torch.zeros(B, stride)
    img = mask[:, :Himg * Wimg].view(B, Himg, Wimg)
    img[0, 24, 32] = 1                                  # sampled: (3, 4)
    img[0, 9, 9] = img[0, 8, 9] = img[0, 7, 8] = 1      # neighbours of the sampled (8, 8): never read
    img[1, 0, 0] = 1                                    # corner
    img[1, Himg - 8, Wimg - 8] = 1                      # the last sampled pixel: the opposite corner
    img[2, 16, 0] = img[2, 0, 40] = 1                   # left and top edge
    img[2, Himg - 1, :] = 1                             # last row: not sampled
    mask[:, Himg * Wimg:] = 1                           # between the images: not part of any
    want = AR.patch_mask(img.double(), h, w).float()
    assert [int(L - want[b].sum()) for b in range(B)] == [9, 8, 12]
    md = T.Guarded(mask.shape, data=mask)
    one, many = T.Guarded((L,)), T.Guarded((B, L))
    call('hv_ca_mask', P(md), Himg, Wimg, h, w, P(one))
    call('hv_ca_mask_batched', P(md), B, ll(stride), Himg, Wimg, h, w, P(many))
    assert same_bits(many.cpu(), want) and same_bits(one.cpu(), want[0])
    assert one.intact() and many.intact()


# ---------------------------------------------------------------------------------------------------------------- score fusion
@pytest.mark.parametrize('adjoint', [0, 1])
@pytest.mark.parametrize('h,w', [(8, 8), (16, 16), (6, 6), (4, 8), (6, 10)], ids=lambda v: str(v))
def test_score_fusion_outside_the_32x32_map(h, w, adjoint):
    """hv_ca_fuse: ca_fuse_p2_kernel for power-of-two h and w (8x8, 16x16, 4x8), ca_fuse_kernel otherwise (6x6, 6x10); square or not."""
    B, L = 2, h * w
    ck = Check()
    S = torch.randn(B, L, L, generator=torch.Generator().manual_seed(300 + 40 * h + 2 * w + adjoint))
    ref = AR.fuse(S.double(), h, w, adjoint)
    terms = AR.fuse(S.double().abs(), h, w, adjoint)
    Sd, out = T.Guarded(S.shape, data=S), T.Guarded(S.shape)
    call('hv_ca_fuse', P(Sd), P(out), B, h, w, adjoint)
    ck.le('fuse', (out.cpu().double() - ref).abs(), 9 * U * terms, '%dx%d adjoint=%d' % (h, w, adjoint))
    ck.true(out.intact() and same_bits(Sd.cpu(), S), 'guards / source')
    ck.done()


# ---------------------------------------------------------------------------------------------------------------- soft-max forward
SOFTMAX_ENTRY = {'plain': 'hv_ca_softmax', 'batched': 'hv_ca_softmax_batched', 'f16': 'hv_ca_softmax_f16'}


def run_softmax(entry, S, mm, B, L, s_off, stride, want_argmax):
    """S [B][L][L], mm [B][L] (CPU) -> A (CPU, as stored), arg-max (CPU or None), guards intact."""
    step = {0: 0, 'L': L, 'L+1': L + 1}[stride]
    Sd = T.Guarded(S.shape, offset=s_off, data=S)
    held = torch.full((B, max(step, L)), 3.0)
    held[:, :L] = mm
    mmd = T.Guarded(held.shape, data=held) if step else T.Guarded((L,), data=mm[0])
    A = T.Guarded(S.shape, torch.float16 if entry == 'f16' else torch.float32)
    arg = T.Guarded((B * L,), torch.int32) if want_argmax else None
    tail = (P(A), B, L, f32c(AR.SOFTMAX_SCALE), P(arg) if want_argmax else None)
    if entry == 'plain':
        assert step == 0
        call('hv_ca_softmax', P(Sd), P(mmd), *tail)
    else:
        call(SOFTMAX_ENTRY[entry], P(Sd), P(mmd), ll(step), *tail)
    ok = A.intact() and (arg is None or arg.intact()) and same_bits(Sd.cpu(), S)
    return A.cpu(), (arg.cpu().view(B, L).long() if want_argmax else None), ok


@pytest.mark.parametrize('name', sorted(AR.SOFTMAX_ROWS))
def test_softmax_forward(name):
    """hv_ca_softmax / _batched / _f16.  L in {256, 1024, 4096} with 16-byte bases and a mask stride that is a multiple of 4: ca_softmax_wave_kernel (wave*);
    the same L with S one float off, or a mask stride of L + 1, and L = 512, 2048: the register path of ca_softmax_kernel (reg*); L = 16, 100, 300, 2304: its
    three-pass path (gen*).  A against fp64, masked columns exactly 0, the arg-max equal to the reference's on every decided row (attention_ref.softmax_expectation),
    within the margin of the maximum elsewhere; the same A bits with and without an arg-max output."""
    L, B, entry, s_off, stride = AR.SOFTMAX_ROWS[name]
    ck = Check()
    e = AR.softmax_expectation(name)
    A, arg, ok = run_softmax(entry, e['S'], e['mm'], B, L, s_off, stride, True)
    ck.true(ok, 'guards / source')
    ck.le('softmax.A16' if entry == 'f16' else 'softmax.A', (A.double() - e['A']).abs(), e['tol'], name)
    masked = (e['mm'] == 0).unsqueeze(1).expand(B, L, L)
    ck.true(bool((A[masked] == 0).all()), 'masked columns not exactly 0')
    ck.true(bool(((arg >= 0) & (arg < L)).all()), 'arg-max out of range')
    arg = arg.clamp(0, L - 1)
    dec = e['decided']
    ck.true((~dec).float().mean().item() <= 0.01, 'more than 1 % of the rows undecided')
    ck.true(bool((arg[dec] == e['idx'][dec]).all()), 'arg-max of %d decided rows differs' % int((arg[dec] != e['idx'][dec]).sum()))
    at = e['A'].gather(2, arg.unsqueeze(2)).squeeze(2)
    ck.true(bool((at[~dec] >= (e['top'] - e['margin'])[~dec]).all()), 'arg-max of an undecided row outside the margin')
    A2, _, ok2 = run_softmax(entry, e['S'], e['mm'], B, L, s_off, stride, False)
    ck.true(ok2 and same_bits(A, A2), 'argmax = NULL: other A bits')
    ck.done()


@pytest.mark.parametrize('entry', ['batched', 'f16'])
@pytest.mark.parametrize('L', [256, 512, 300])
def test_softmax_of_a_row_without_valid_patches(L, entry):
    """A sample whose mask is all zero (per-sample masks; wave kernel, register path, three-pass path): A all 0, arg-max 0; the other sample is as without it."""
    B = 2
    ck = Check()
    gen = torch.Generator().manual_seed(600 + L)
    S = torch.randn(B, L, L, generator=gen)
    mm = (torch.rand(B, L, generator=gen) >= 1 / 3).float()
    mm[1] = 0
    ref, _ = AR.softmax(S.double(), mm.double(), AR.SOFTMAX_SCALE)
    A32 = torch.softmax(S * mm.unsqueeze(1) * torch.tensor(AR.SOFTMAX_SCALE), dim=2) * mm.unsqueeze(1)
    tol = AR.tol_elem(ref, (A32.double() - ref).abs().max().item(), entry == 'f16')
    A, arg, ok = run_softmax(entry, S, mm, B, L, 0, 'L', True)
    ck.true(ok, 'guards / source')
    ck.true(bool((A[1] == 0).all()) and bool((arg[1] == 0).all()), 'all-zero mask: A or arg-max not 0')
    ck.le('softmax.A16' if entry == 'f16' else 'softmax.A', (A.double() - ref).abs(), tol, 'L=%d' % L)
    ck.done()


TIE_ROUTES = [(256, 'wave'), (256, 'block'), (1024, 'wave'), (1024, 'block'), (512, 'block'), (300, 'block')]


@pytest.mark.parametrize('entry', ['plain', 'f16'])
@pytest.mark.parametrize('L,route', TIE_ROUTES, ids=['%d-%s' % r for r in TIE_ROUTES])
def test_softmax_argmax_takes_the_first_of_exact_ties(L, route, entry):
    """Two equal S values at unmasked columns l < l2, every other column strictly smaller: the tied entries go through the same arithmetic, so A ties exactly and
    the arg-max must be l.  l2 - l = 1 (one lane's float4 in the wave kernel), 4 (two lanes), 64 (two waves of the block kernel; lanes 16 apart in the wave
    kernel), 256 (two 256-chunks: the same lane / thread, a later register).  Every fourth row also has a MASKED column before l that holds a larger S (its
    logit is 0, its A is 0: it never wins).  'block': S one float off 16 bytes, which sends L = 256 / 1024 to ca_softmax_kernel."""
    B = 1
    seps = [s for s in (1, 4, 64, 256) if s < L - 8]
    S = -1.0 - torch.rand(B, L, L, generator=torch.Generator().manual_seed(700 + L))
    mm = torch.ones(L)
    mm[5] = 0
    S[:, :, 5] = -3.0
    want = torch.empty(L, dtype=torch.long)
    for r in range(L):
        sep = seps[r % len(seps)]
        l = 6 + (r * 7) % (L - sep - 6)
        S[0, r, l] = S[0, r, l + sep] = 1.0 + (r % 5) * 0.125
        if r % 4 == 3:
            S[0, r, 5] = 2.5
        want[r] = l
    A, arg, ok = run_softmax(entry, S, mm.view(1, L), B, L, 1 if route == 'block' else 0, 0, True)
    assert ok
    rows = torch.arange(L)
    assert bool((A[0, rows, want] == A[0, rows, want + torch.tensor([seps[r % len(seps)] for r in range(L)])]).all()), 'the tied entries differ'
    assert bool((A[0, :, 5] == 0).all())
    bad = (arg[0] != want).nonzero().flatten().tolist()
    assert not bad, ('rows', bad[:8], 'got', arg[0][bad[:8]].tolist(), 'want', want[bad[:8]].tolist())


# ---------------------------------------------------------------------------------------------------------------- soft-max backward
# (L, dS base offset, A holds mass on masked columns)
BWD_ROWS = [(256, 0, False), (1024, 0, False), (64, 0, False), (300, 0, False), (512, 0, False), (256, 1, False), (256, 0, True), (300, 0, True)]


@pytest.mark.parametrize('f16', [False, True], ids=['A32', 'A16'])
@pytest.mark.parametrize('L,off,unmasked', BWD_ROWS, ids=['L%d%s%s' % (r[0], '-offset' if r[1] else '', '-unmaskedA' if r[2] else '') for r in BWD_ROWS])
def test_softmax_backward(L, off, unmasked, f16):
    """hv_ca_softmax_backward(_f16), B = 2, one mask for both samples.  L = 256, 1024 with 16-byte bases: ca_softmax_bwd_wave_kernel; L = 64, 300, 512, and L = 256
    with dS one float off: ca_softmax_bwd_kernel.  Both sides read the same stored A (fp32 or fp16).  'unmaskedA': the stored A keeps its mass on the masked
    columns, so the factor mm of the formula is seen (dS exactly 0 there)."""
    B, scale = 2, 10.0
    ck = Check()
    gen = torch.Generator().manual_seed(800 + L + off + 2 * unmasked)
    S = torch.randn(B, L, L, generator=gen) * 0.3
    mm = (torch.rand(L, generator=gen) >= 1 / 3).float()
    A = torch.softmax(S.double() * mm.double() * scale, dim=2) * (1.0 if unmasked else mm.double())
    A = A.to(torch.float16 if f16 else torch.float32)
    dA = torch.randn(B, L, L, generator=gen)
    A64, dA64, m64 = A.double(), dA.double(), mm.double()
    ref = AR.softmax_backward(dA64, A64, m64, scale)
    dot = (dA64 * A64).sum(dim=2, keepdim=True)
    A32 = A.float()
    dot32 = (dA * A32).sum(dim=2, keepdim=True)
    plain = torch.tensor(scale) * mm * A32 * (dA - dot32)
    floor = (plain.double() - ref).abs().max().item()
    bound = scale * m64 * A64.abs() * (16 * U * (dA64 * A64).abs().sum(dim=2, keepdim=True) + 4 * U * (dA64.abs() + dot.abs())) + AR.tol_elem(ref, floor, False)
    dS = T.Guarded((B, L, L), offset=off)
    Ad, dAd, md = T.Guarded(A.shape, A.dtype, data=A), T.Guarded(dA.shape, data=dA), T.Guarded((L,), data=mm)
    call('hv_ca_softmax_backward_f16' if f16 else 'hv_ca_softmax_backward', P(dAd), P(Ad), P(md), P(dS), B, L, f32c(scale))
    got = dS.cpu()
    ck.le('softmax.dS', (got.double() - ref).abs(), bound, 'L=%d' % L)
    ck.true(bool((got[:, :, mm == 0] == 0).all()), 'dS of a masked column not exactly 0')
    ck.true(dS.intact() and same_bits(Ad.cpu(), A) and same_bits(dAd.cpu(), dA), 'guards / sources')
    ck.done()


# ---------------------------------------------------------------------------------------------------------------- backward prep
@pytest.mark.parametrize('L,B', [(256, 2), (512, 1), (64, 2), (96, 2), (160, 2)])
def test_score_backward_prep(L, B):
    """hv_ca_score_backward_prep.  (L / 32) % 8 == 0 (L = 256: 8 tiles a side, 512: 16): the XCD-ordered grid of ca_gs_kernel; L = 64, 96, 160: the plain grid --
    in the last two L is no multiple of the 64 columns of a ca_coef_part_kernel block.  One norm per sample at or below the floor: coef exactly 0 there."""
    ck = Check()
    gen = torch.Generator().manual_seed(900 + L)
    dS, S0 = torch.randn(B, L, L, generator=gen), torch.randn(B, L, L, generator=gen)
    norm = 0.5 + torch.rand(B, L, generator=gen)
    at = [(0, 17), (1, L - 3)][:B]
    norm[0, 17] = 1e-4                      # exactly the floor
    if B > 1:
        norm[1, L - 3] = 5e-5
    rnorm = 1.0 / norm.clamp_min(1e-4)
    Gs_r, coef_r = AR.score_backward_prep(dS.double(), S0.double(), norm.double(), rnorm.double(), FLOOR32)
    r64, d64 = rnorm.double(), dS.double()
    gb = 3 * U * ((d64.transpose(1, 2) * r64.unsqueeze(2)).abs() + (d64 * r64.unsqueeze(1)).abs())
    prod = d64 * S0.double()
    cb = (16 * U * prod.abs().sum(dim=1) + 4 * U * prod.sum(dim=1).abs()) / norm.double() ** 2
    Gs, coef = T.Guarded((B, L, L)), T.Guarded((17 * B * L,))
    src = [T.Guarded(t.shape, data=t) for t in (dS, S0, norm, rnorm)]
    call('hv_ca_score_backward_prep', *[P(t) for t in src], P(Gs), P(coef), B, L)
    ck.le('prep.Gs', (Gs.cpu().double() - Gs_r).abs(), gb, 'Gs')
    c = coef.cpu()[:B * L].view(B, L)
    ck.le('prep.coef', (c.double() - coef_r).abs(), cb, 'coef')
    ck.true(all(float(c[b, l]) == 0.0 for b, l in at), 'coef of a clamped norm not exactly 0')
    ck.true(Gs.intact() and coef.intact(), 'guards')
    ck.done()


def test_score_backward_prep_refuses_a_map_that_is_no_multiple_of_32():
    L = 48
    t = [T.Guarded((L, L)) for _ in range(3)] + [T.Guarded((L,)) for _ in range(2)] + [T.Guarded((17 * L,))]
    assert rc_of('hv_ca_score_backward_prep', P(t[0]), P(t[1]), P(t[3]), P(t[4]), P(t[2]), P(t[5]), 1, L) == HV_ERR_ARG
    torch.cuda.synchronize()
    assert bool(torch.isnan(t[2].cpu()).all()) and bool(torch.isnan(t[5].cpu()).all())


# ---------------------------------------------------------------------------------------------------------------- col2im
# name: (C, df_ld, accumulate, kernel)
COL2IM_ROWS = {
    'vector': (8, 8, 1, 'ca_patches_bwd_vec_kernel'),
    'assign': (8, 8, 0, 'ca_patches_bwd_kernel'),
    'c6': (6, 6, 1, 'ca_patches_bwd_kernel'),
    'vector_ld12': (8, 12, 1, 'ca_patches_bwd_vec_kernel'),
    'scalar_ld10': (8, 10, 1, 'ca_patches_bwd_kernel'),
}


def col2im_inputs(C):
    B, H, W = 2, 12, 8
    L = (H // 2) * (W // 2)
    gen = torch.Generator().manual_seed(1000 + C)
    dwp, wp = torch.randn(B, L, 9, C, generator=gen), torch.randn(B, L, 9, C, generator=gen)
    coef = torch.randn(B, L, generator=gen)
    prior = torch.randn(B, H, W, 16, generator=gen) + 3.0      # non-zero everywhere
    return B, H, W, L, dwp, wp, coef, prior


def run_col2im(C, ld, accumulate):
    B, H, W, L, dwp, wp, coef, prior = col2im_inputs(C)
    df = T.Guarded((B, H, W, ld), data=prior[..., :ld])
    src = [T.Guarded(t.shape, data=t) for t in (dwp, wp, coef)]
    call('hv_ca_patches_backward', *[P(t) for t in src], P(df), B, H, W, C, ld, accumulate)
    return df.cpu(), df.intact()


@pytest.mark.parametrize('name', sorted(COL2IM_ROWS))
def test_col2im_of_the_patch_gradient(name):
    """hv_ca_patches_backward, B = 2, 12 x 8: accumulate with C % 4 == 0, df_ld % 4 == 0 and 16-byte bases: ca_patches_bwd_vec_kernel; otherwise
    ca_patches_bwd_kernel (COL2IM_ROWS).  Assign mode writes exact zeros at the odd pixels, accumulate mode leaves them bit for bit; channels beyond C are not touched."""
    C, ld, accumulate, _ = COL2IM_ROWS[name]
    ck = Check()
    B, H, W, L, dwp, wp, coef, prior = col2im_inputs(C)
    prior = prior[..., :ld]
    ref = AR.patches_backward(dwp.double(), wp.double(), coef.double(), H, W)
    terms = AR.patches_backward(dwp.double().abs(), (wp.double() * coef.double().view(B, L, 1, 1)).abs(), torch.ones(B, L, dtype=F64), H, W)
    if accumulate:
        ref, terms = ref + prior[..., :C].double(), terms + prior[..., :C].double().abs()
    got, ok = run_col2im(C, ld, accumulate)
    ck.true(ok, 'guards')
    ck.le('col2im', (got[..., :C].double() - ref).abs(), 18 * U * terms, name)
    ck.true(same_bits(got[..., C:], prior[..., C:]), 'channels beyond C changed')
    odd = torch.ones(H, W, dtype=torch.bool)
    odd[::2, ::2] = False
    if accumulate:
        ck.true(same_bits(got[:, odd][..., :C], prior[:, odd][..., :C]), 'accumulate: an odd pixel changed')
    else:
        ck.true(same_bits(got[:, odd][..., :C], torch.zeros(B, int(odd.sum()), C)), 'assign: an odd pixel is not +0')
    ck.done()


def test_col2im_vector_and_scalar_kernels_give_the_same_bits():
    """The accumulate routes on the same inputs and the same prior content: df_ld = 8 (vector kernel) against df_ld = 10 (scalar kernel)."""
    a, ok_a = run_col2im(8, 8, 1)
    b, ok_b = run_col2im(8, 10, 1)
    assert ok_a and ok_b and same_bits(a, b[..., :8])


# ---------------------------------------------------------------------------------------------------------------- plain transpose
@pytest.mark.parametrize('B,R,C', [(2, 33, 50), (1, 64, 8), (3, 72, 40)])
def test_plain_transpose(B, R, C):
    """hv_transpose_batched (transpose_kernel, 32 x 32 tiles with ragged edges)."""
    src = torch.randn(B, R, C, generator=torch.Generator().manual_seed(R))
    s, d = T.Guarded(src.shape, data=src), T.Guarded((B, C, R))
    call('hv_transpose_batched', P(s), P(d), B, R, C)
    assert same_bits(d.cpu(), AR.transpose(src)) and d.intact()


# ---------------------------------------------------------------------------------------------------------------- offset flow
@pytest.mark.parametrize('up', [2, 8])
@pytest.mark.parametrize('h,w', [(8, 8), (6, 10)], ids=lambda v: str(v))
def test_offset_flow(h, w, up):
    """hv_ca_flow against inpaint_tools.flow_to_image and the nearest x`up`, as offsets_to_flow builds it.  B = 3: sample 0 is the identity arg-max (all offsets
    zero, radius 0), sample 1 random, sample 2 points every position at the far corner: the radius is normalised by the running maximum over samples 0..b."""
    from hvgan.models.inpaint_tools import flow_to_image
    B, L = 3, h * w
    arg = torch.empty(B, L, dtype=torch.int32)
    arg[0] = torch.arange(L)
    arg[1] = torch.randint(0, L, (L,), generator=torch.Generator().manual_seed(h * w + up))
    arg[2] = L - 1
    pos = torch.arange(L)
    off = torch.stack([arg.long() // w - pos // w, arg.long() % w - pos % w], dim=2).view(B, h, w, 2)
    img = torch.from_numpy(flow_to_image(off.numpy())) / 255.
    ref = img.permute(0, 3, 1, 2).repeat_interleave(up, dim=2).repeat_interleave(up, dim=3).contiguous()
    flow, argd = T.Guarded((B, 3, h * up, w * up)), T.Guarded(arg.shape, torch.int32, data=arg)
    call('hv_ca_flow', P(argd), B, h, w, up, P(flow))
    assert flow.intact() and not bool(torch.isnan(flow.cpu()).any())
    T._flow_close(flow.cpu(), ref, 'flow %dx%d up %d' % (h, w, up))
    assert float(flow.cpu()[1:].min()) < 1.0      # samples 1 and 2 are coloured
