"""The attention block's batched NT GEMM and fold (csrc/bgemm.hip) and its Gram-route kernels (csrc/attention_gram.hip), called through the C entries,
against the fp64 references of tests/attention_ref.py (pinned by tests/test_attention_ref_cpu.py) at the shapes where the entries switch kernels or row
groups.  Each test names the branch its shapes reach; the rules are those of the entry points (AR.gemm_takes_dma, AR.gram_lg restate them).

Every output lies in a hvtest.Guarded buffer; every padding column, padding row and gap between batches of an output holds NaN before the call and must hold
the same bits afterwards; the padding of every input holds NaN as well, so a kernel that reads it poisons its result.  Operands are drawn in fp16 (magnitude
0.5 .. 1.5, random sign), so the device and the reference see the same values.  Bounds, per element, from fp64 reference quantities and u = 2^-24 only:
  fp32 result of a K-term sum     (K + 2) u S, S = the sum of the |terms| (the worst case of any fp32 summation order)
  the same stored as fp16         + 2^-11 |ref| + 2^-25
  q                               (C + 2) u q
  norm, rnorm                     (9 + C + 6) u, relative
  copies (fd_h, fdT_h)            bit for bit
Each test asserts that its bound is below 1/20 of the mean |term| wherever the sum has terms: one dropped or doubled term fails.
The worst error / bound ratio of every family is printed at the end of the module (pytest -s)."""
import ctypes

import pytest
import torch

import attention_ref as AR

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
F64 = torch.float64
NAN = float('nan')
ERR_ARG, ERR_UNSUPPORTED = -1, -2
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
    rc = getattr(lib.get().cdll, name)(*args, lib.stream())
    torch.cuda.synchronize()
    return rc


def P(x):
    return lib.ptr(x.t if hasattr(x, 'intact') else x)


def f32c(v):
    return ctypes.c_float(v)


def ll(v):
    return ctypes.c_longlong(v)


def dt(f16):
    return torch.float16 if f16 else torch.float32


def lay(data, ld, stride, dtype, fill=NAN):
    """data [batch][rows][cols] placed with leading dimension ld and batch stride `stride` into a flat buffer of exactly the extent it spans, every other
    element `fill` -> (flat CPU tensor of dtype, index tensor [batch][rows][cols] into it)."""
    batch, rows, cols = data.shape
    idx = torch.arange(batch).view(-1, 1, 1) * stride + torch.arange(rows).view(1, -1, 1) * ld + torch.arange(cols).view(1, 1, -1)
    flat = torch.full(((batch - 1) * stride + (rows - 1) * ld + cols,), fill, dtype=dtype)
    flat[idx] = data.to(dtype)
    return flat, idx


def padding_kept(before, after, idx):
    """Every element outside idx has the bits it had."""
    pad = torch.ones(before.numel(), dtype=torch.bool)
    pad[idx.reshape(-1)] = False
    return same_bits(before[pad], after[pad])


# ================================================================================================================ hv_bgemm_nt / hv_bgemm_nt_h
def gemm_dims(name):
    M, N, K, batch, alpha, scaled, split, padded = AR.GEMM_ROWS[name]
    if padded:
        lda, ldb, ldc = K + 8, K + 16, N + 4
        return lda, ldb, ldc, M * lda + 8, N * ldb + 16, M * ldc + 4, N + 4
    return K, K, N, M * K, N * K, M * N, N


def gemm_run(name, a16, b16, c16, e):
    """-> (C values [batch][M][N] as stored, guards and padding intact)."""
    M, N, K, batch, alpha, scaled, split, padded = AR.GEMM_ROWS[name]
    lda, ldb, ldc, sA, sB, sC, sS = gemm_dims(name)
    Af, _ = lay(e['A'], lda, sA, dt(a16))
    Bf, _ = lay(e['B'], ldb, sB, dt(b16))
    csd = lay(e['cs'].unsqueeze(1), N, sS, torch.float32)[0].to(T.dev()) if scaled else None
    Cf, cidx = lay(torch.full((batch, M, N), NAN), ldc, sC, dt(c16))
    Ad, Bd, C = Af.to(T.dev()), Bf.to(T.dev()), T.Guarded(Cf.numel(), dt(c16), data=Cf)
    call('hv_bgemm_nt_h' if c16 else 'hv_bgemm_nt', P(Ad), a16, lda, ll(sA), P(Bd), b16, ldb, ll(sB), P(C), ldc, ll(sC), M, N, K, batch, f32c(alpha), P(csd) if scaled else None,
         ll(sS if scaled else 0), split)
    out = C.cpu()
    return out[cidx], C.intact() and padding_kept(Cf, out, cidx)


@pytest.mark.parametrize('c16', [0, 1])
@pytest.mark.parametrize('name', list(AR.GEMM_ROWS))
def test_bgemm_rows_against_fp64_with_padding_and_in_every_operand_form(name, c16):
    """hv_bgemm_nt (fp32 C) and hv_bgemm_nt_h (fp16 C, what AttentionPlan's paste and paste-gradient call) on AR.GEMM_ROWS.  Register-staged kernel:
    one k-step with a single lane quad of columns; ragged second tiles in both directions at BN = 64; the XCD swizzle (batch % 8 == 0); the plain map at
    BN = 128; alpha != 1, the column scale, b_split = 4 and N / 4, padded lda / ldb / ldc and batch strides.  LDS-DMA kernel (fp16 x fp16): exactly 128 tiles
    with two k-steps; one live row / column in the last tiles; one tile short and K % 64 != 0 (both fall back); b_split + column scale + padding with
    batch % 8 != 0.  The three operand forms (fp32 x fp32, fp32 x fp16, fp16 x fp16) must give equal bits: that holds the LDS-DMA kernel to the
    register-staged one."""
    M, N, K, batch, alpha, scaled, split, padded = AR.GEMM_ROWS[name]
    assert AR.gemm_takes_dma(M, N, K, batch) == (name in ('dma_128_tiles', 'dma_ragged', 'dma_split_scaled_padded'))
    e = AR.gemm_case(name)
    bound = AR.tol_sum(e['S'], K, e['ref'] if c16 else None)
    assert AR.one_term_shows(bound, e['S'], K)
    ck = Check()
    first = None
    for a16, b16 in ((0, 0), (0, 1), (1, 1)):
        got, kept = gemm_run(name, a16, b16, c16, e)
        ck.true(kept, ('guards / padding', a16, b16))
        if first is None:
            first = got
            ck.le('bgemm f16' if c16 else 'bgemm f32', (got.double() - e['ref']).abs(), bound, name)
        else:
            ck.true(same_bits(got, first), ('bits differ from fp32 x fp32', a16, b16))
    ck.done()


def test_bgemm_refusals():
    dev = T.dev()
    A, B, C = torch.zeros(4096, device=dev), torch.zeros(4096, device=dev), torch.zeros(4096, device=dev)

    def rc(M=16, N=8, K=32, lda=None, ldb=None, a16=0, b16=0, split=0, a_off=0):
        lda, ldb = K if lda is None else lda, K if ldb is None else ldb
        return rc_of('hv_bgemm_nt', P(A[a_off:]), a16, lda, ll(M * lda), P(B), b16, ldb, ll(N * ldb), P(C), N, ll(M * N), M, N, K, 1, f32c(1.0), None, ll(0), split)

    assert rc() == 0
    assert rc(K=48, lda=48, ldb=48) == ERR_UNSUPPORTED      # K % 32
    assert rc(N=6) == ERR_UNSUPPORTED                       # N % 4
    assert rc(K=64, lda=32, ldb=64) == ERR_UNSUPPORTED      # lda < K
    assert rc(a_off=1) == ERR_UNSUPPORTED                   # base off its 16 bytes
    assert rc(a16=1, b16=0) == ERR_UNSUPPORTED              # fp16 x fp32 is not instantiated
    assert rc(split=3) == ERR_ARG                           # N % b_split
    assert bool((C[128:] == 0).all())


# ================================================================================================================ hv_ca_fold / hv_ca_fold_h
def fold_run(e, shape, s16, d16, acc, ld, offset=0, expect=0):
    B, H, W, C = shape
    src = e['src'].to(dt(s16)).to(T.dev())
    before, idx = lay(e['old'].reshape(1, B * H * W, C), ld, 0, dt(d16))
    dst = T.Guarded(before.numel(), dt(d16), offset=offset, data=before)
    rc = rc_of('hv_ca_fold_h' if s16 else 'hv_ca_fold', P(src), P(dst), d16, B, H, W, C, ld, f32c(AR.FOLD_ALPHA), acc)
    assert rc == expect, (rc, expect)
    out = dst.cpu()
    return out[idx].reshape(B, H, W, C), dst.intact() and padding_kept(before, out, idx)


@pytest.mark.parametrize('d16', [0, 1])
@pytest.mark.parametrize('s16', [0, 1])
@pytest.mark.parametrize('shape', AR.FOLD_SHAPES)
def test_fold_against_fp64(shape, s16, d16):
    """fp32 / fp16 source (hv_ca_fold / hv_ca_fold_h: the plan calls the latter) x fp32 / fp16 destination, assign and accumulate onto a non-zero map,
    dst_ld = C and C + 8 with NaN in the padding channels, H != W.  C % 8 == 0: ca_fold_vec_kernel; C = 12: ca_fold_kernel, which hv_ca_fold_h refuses."""
    B, H, W, C = shape
    e = AR.fold_case(shape)
    ck = Check()
    for acc in (0, 1):
        ref, S, n = e['ref'][acc], e['S'][acc], e['nterms'][acc]
        bound = AR.tol_sum(S, n, ref if d16 else None)
        assert AR.one_term_shows(bound, S, n)
        for ld in (C, C + 8):
            if s16 and C % 8:
                got, kept = fold_run(e, shape, s16, d16, acc, ld, expect=ERR_UNSUPPORTED)
                ck.true(kept and same_bits(got, e['old'].to(dt(d16))), ('a refused call wrote', acc, ld))
                continue
            got, kept = fold_run(e, shape, s16, d16, acc, ld)
            ck.true(kept, ('guards / padding', acc, ld))
            ck.le('fold f16' if d16 else 'fold f32', (got.double() - ref).abs(), bound, (acc, ld))
    ck.done()


@pytest.mark.parametrize('d16', [0, 1])
def test_fold_scalar_kernel_gives_the_vector_kernels_bits(d16):
    """ca_fold_kernel reached by dst_ld % 8 != 0 and by a destination off its 16 bytes, fp32 source, on the data of the vector kernel: the same bits
    (same summation order per element), within the fp64 bound.  hv_ca_fold_h refuses both; odd H or W is an argument error."""
    shape = AR.FOLD_SHAPES[0]
    B, H, W, C = shape
    e = AR.fold_case(shape)
    ck = Check()
    for acc in (0, 1):
        ref, S, n = e['ref'][acc], e['S'][acc], e['nterms'][acc]
        bound = AR.tol_sum(S, n, ref if d16 else None)
        vec, kept = fold_run(e, shape, 0, d16, acc, C)
        ck.true(kept, 'vector')
        for what, ld, off in (('dst_ld = C + 4', C + 4, 0), ('base off by one element', C, 1)):
            got, kept = fold_run(e, shape, 0, d16, acc, ld, offset=off)
            ck.true(kept, ('guards / padding', what))
            ck.true(same_bits(got, vec), ('bits differ from the vector kernel', what, acc))
            ck.le('fold scalar', (got.double() - ref).abs(), bound, (what, acc))
            got, kept = fold_run(e, shape, 1, d16, acc, ld, offset=off, expect=ERR_UNSUPPORTED)
            ck.true(kept and same_bits(got, e['old'].to(dt(d16))), ('a refused call wrote', what))
    ck.done()
    src, dst = torch.zeros(4096, device=T.dev()), torch.zeros(4096, device=T.dev())
    for name in ('hv_ca_fold', 'hv_ca_fold_h'):
        assert rc_of(name, P(src), P(dst), 0, 1, 3, 4, 8, 8, f32c(1.0), 0) == ERR_ARG
        assert rc_of(name, P(src), P(dst), 0, 1, 4, 6 + 1, 8, 8, f32c(1.0), 0) == ERR_ARG
        assert rc_of(name, P(src), P(dst), 0, 1, 4, 4, 8, 4, f32c(1.0), 0) == ERR_ARG      # dst_ld < C


# ================================================================================================================ hv_ca_gram_down
@pytest.mark.parametrize('f_ld', [64, 72])
@pytest.mark.parametrize('B,H,W', [(2, 6, 16), (1, 4, 144), (3, 10, 64)])
def test_gram_down_against_fp64(B, H, W, f_ld):
    """w = 8, 72 (a second segment of 8 pixels behind the first 64) and 32; f_ld = C and C + 8 with NaN beside the channels; H != W."""
    C, h, w = 64, H // 2, W // 2
    L = h * w
    gen = torch.Generator().manual_seed(B * 1000 + H * 10 + W)
    f = AR.draw_f16((B, H, W, C), gen)
    fd, fdT, q = AR.gram_down(f.double())
    fdev = lay(f.reshape(1, B * H * W, C), f_ld, 0, torch.float16)[0].to(T.dev())
    fd_h, fdT_h, qd = T.Guarded((B, L, C), torch.float16), T.Guarded((B, C, L), torch.float16), T.Guarded((B, L))
    call('hv_ca_gram_down', P(fdev), 1, B, H, W, C, f_ld, P(fd_h), P(fdT_h), P(qd))
    ck = Check()
    ck.true(fd_h.intact() and fdT_h.intact() and qd.intact(), 'guards')
    ck.true(torch.equal(fd_h.cpu(), fd.reshape(B, L, C).half()), 'fd_h')
    ck.true(torch.equal(fdT_h.cpu(), fdT.half()), 'fdT_h')
    bound = (C + 2) * U * q
    assert AR.one_term_shows(bound, q, C)
    ck.le('gram q', (qd.cpu().double() - q).abs(), bound)
    ck.done()


def test_gram_down_refusals():
    dev = T.dev()
    f, a, b, q = torch.zeros(65536, dtype=torch.float16, device=dev), torch.zeros(65536, dtype=torch.float16, device=dev), \
        torch.zeros(65536, dtype=torch.float16, device=dev), torch.zeros(4096, device=dev)
    assert rc_of('hv_ca_gram_down', P(f), 1, 1, 4, 16, 64, 64, P(a), P(b), P(q)) == 0
    assert rc_of('hv_ca_gram_down', P(f), 0, 1, 4, 16, 64, 64, P(a), P(b), P(q)) == ERR_UNSUPPORTED      # fp32 input
    assert rc_of('hv_ca_gram_down', P(f), 1, 1, 4, 16, 32, 32, P(a), P(b), P(q)) == ERR_UNSUPPORTED      # C != 64
    assert rc_of('hv_ca_gram_down', P(f), 1, 1, 4, 20, 64, 64, P(a), P(b), P(q)) == ERR_UNSUPPORTED      # (W / 2) % 8
    assert rc_of('hv_ca_gram_down', P(f), 1, 1, 3, 16, 64, 64, P(a), P(b), P(q)) == ERR_ARG              # odd H


# ================================================================================================================ hv_ca_gram_scores
# (w, B, h, lg by the entry's rule, a 2 x 2 corner of zeros in the last sample: an all-zero 3x3 patch, the norm at its floor)
SCORE_CASES = [(32, 1, 1, 4, False), (32, 2, 5, 4, True), (32, 3, 12, 4, False), (32, 31, 17, 16, False), (32, 16, 32, 16, False),
               (64, 1, 3, 4, False), (64, 2, 9, 4, True), (64, 57, 9, 8, False), (64, 31, 17, 16, False)]


@pytest.mark.parametrize('w,B,h,lg,zeros', SCORE_CASES)
def test_gram_scores_against_fp64(w, B, h, lg, zeros):
    """hv_ca_gram_scores: S0, norm, rnorm of every sample against the patch definition (the box-filter form of the reference, pinned against it on the CPU,
    where B L^2 is large).  h != w throughout.  w = 32 (four grid rows of l per round, one per wave): lg = 4 with h = 1, 5 (ly1 clips the second group)
    and 12; lg = 16 -- four rounds per wave, the rotating row registers -- with a last group of one row (B, h = 31, 17) and at the benchmarked 16 x 32.
    w = 64 (one grid row per round): lg = 4 at h = 3, 9; lg = 8 at (57, 9), the smallest h whose B h reaches 1024 workgroups at lg = 8 but not at 16, with
    a last group of one row; lg = 16 with h % 16 != 0 at (31, 17), the smallest B h that gives 1024 workgroups at lg = 16 (S0: 147 MB)."""
    assert AR.gram_lg(B, h) == lg
    C, L, K = 64, h * w, 9 * 64
    gen = torch.Generator().manual_seed(w * 10000 + B * 100 + h)
    fd = AR.draw_f16((B, h, w, C), gen)
    if zeros:
        fd[B - 1, 0:2, 0:2] = 0
    q = fd.double().pow(2).sum(dim=3).reshape(B, L).float()
    fdev = fd.reshape(B, L, C).half().to(T.dev())
    S0, norm, rnorm = T.Guarded((B, L, L)), T.Guarded((B, L)), T.Guarded((B, L))
    call('hv_ca_gram_scores', P(fdev), P(q.to(T.dev())), B, h, w, C, P(S0), P(norm), P(rnorm))
    ck = Check()
    ck.true(S0.intact() and norm.intact() and rnorm.intact(), 'guards')
    ref_of = AR.gram_scores if B * L * L <= 2 ** 22 else AR.gram_scores_box
    gn, gr = norm.cpu().double(), rnorm.cpu().double()
    for b in range(B):
        r0, Sb, rn, rr = ref_of(fd[b:b + 1])
        bound = AR.tol_sum(Sb, K)
        assert AR.one_term_shows(bound, Sb, K)
        ck.le('gram S0', (S0.t[b:b + 1].cpu().double() - r0).abs(), bound, b)
        ck.le('gram norm', (gn[b:b + 1] - rn).abs(), (9 + C + 6) * U * rn, b)
        ck.le('gram rnorm', (gr[b:b + 1] - rr).abs(), (9 + C + 6) * U * rr, b)
        if zeros and b == B - 1:
            ck.true(rn[0, 0] == 1e-4 and bool((Sb[0, :, 0] == 0).all()) and bool((Sb[0, 0, :] == 0).all()), 'the zero patch')
    ck.done()


def test_gram_scores_and_backward_refusals():
    dev = T.dev()
    fd, fT = torch.zeros(65536, dtype=torch.float16, device=dev), torch.zeros(65536, dtype=torch.float16, device=dev)
    q, S0, n, r = torch.zeros(4096, device=dev), torch.zeros(32 * 32 + 64, device=dev), torch.zeros(4096, device=dev), torch.zeros(4096, device=dev)
    assert rc_of('hv_ca_gram_scores', P(fd), P(q), 1, 1, 32, 64, P(S0), P(n), P(r)) == 0
    assert rc_of('hv_ca_gram_scores', P(fd), P(q), 1, 1, 32, 32, P(S0), P(n), P(r)) == ERR_UNSUPPORTED      # C != 64
    assert rc_of('hv_ca_gram_scores', P(fd), P(q), 1, 1, 48, 64, P(S0), P(n), P(r)) == ERR_UNSUPPORTED      # w = 48
    Gs, coef, df = torch.zeros(48 * 48, device=dev), torch.zeros(4096, device=dev), torch.zeros(2 * 64 * 64, device=dev)
    assert rc_of('hv_ca_gram_backward', P(Gs), P(fd), P(fT), P(coef), 1, 1, 32, 64, P(df), 64) == 0
    assert rc_of('hv_ca_gram_backward', P(Gs), P(fd), P(fT), P(coef), 1, 1, 32, 32, P(df), 64) == ERR_UNSUPPORTED      # C != 64
    assert rc_of('hv_ca_gram_backward', P(Gs), P(fd), P(fT), P(coef), 1, 1, 48, 64, P(df), 64) == ERR_UNSUPPORTED      # w = 48
    assert rc_of('hv_ca_gram_backward', P(Gs), P(fd), P(fT), P(coef), 1, 1, 32, 64, P(df), 32) == ERR_ARG              # df_ld < C
    assert bool((df == 0).all())


# ================================================================================================================ hv_ca_gram_backward
@pytest.mark.parametrize('w,h', [(32, 1), (32, 2), (32, 5), (32, 6), (32, 8), (32, 16), (64, 3), (64, 8)])
def test_gram_backward_against_fp64(w, h):
    """hv_ca_gram_backward, B = 3: w = 32 with odd h (ca_gram_backward_kernel<32, 1>) and even h (<32, 2>), h % 8 == 0 (xcd_rows) and not; w = 64 (<64, 1>)
    with and without xcd_rows.  Gs is non-symmetric with entries k / 8, |k| <= 4, and so is coef: E = the box sum of nine entries and the coefficient sum are
    exact in fp32 and in the kernel's fp16 copy of E, so the fp64 reference (the K = 9C route written out) needs no rounding model; the bound is the fp32
    one of the Gram form's L + 1 terms plus the prior content.  df is fp32, pre-filled, df_ld = C and C + 8: the even positions receive old + reference,
    every odd position and every padding channel keeps its bits."""
    B, C, L, H, W = 3, 64, h * w, 2 * h, 2 * w
    gen = torch.Generator().manual_seed(w * 100 + h)
    fd = AR.draw_f16((B, h, w, C), gen)
    Gs, coef = AR.draw_eighths((B, L, L), gen), AR.draw_eighths((B, L), gen)
    assert (Gs - Gs.transpose(1, 2)).abs().max().item() > 0
    ref, S = AR.gram_backward(Gs, fd, coef), AR.gram_backward_bound(Gs, fd, coef)
    dev = T.dev()
    fd_h = fd.reshape(B, L, C).half().to(dev)
    fdT_h = fd_h.transpose(1, 2).contiguous()
    Gd, cd = Gs.to(dev), coef.to(dev)
    ck = Check()
    for df_ld in (C, C + 8):
        old = AR.draw_f16((B, H, W, df_ld), gen)
        df = T.Guarded((B, H, W, df_ld), data=old)
        call('hv_ca_gram_backward', P(Gd), P(fd_h), P(fdT_h), P(cd), B, h, w, C, P(df), df_ld)
        got = df.cpu()
        ck.true(df.intact(), 'guards')
        o = old[:, ::2, ::2, :C].double()
        St = S + o.abs()
        bound = AR.tol_sum(St, L + 1)
        assert AR.one_term_shows(bound, St, L + 2)
        ck.le('gram backward', (got[:, ::2, ::2, :C].double() - (o + ref)).abs(), bound, df_ld)
        keep = torch.ones(B, H, W, df_ld, dtype=torch.bool)
        keep[:, ::2, ::2, :C] = False
        ck.true(same_bits(got[keep], old[keep]), ('odd positions / padding channels', df_ld))
    ck.done()
