"""The fp64 references of tests/attention_ref.py against oracle/restate.py (the dense restatement of ContextualAttention) and torch autograd, in fp64 on the
CPU, on a small non-square map; the composed block against restate.contextual_attention and against fixture g2_attention; and the check that the
soft-max test rows leave at most 1 % of their arg-max undecided by the reference alone."""
import pytest
import torch
import torch.nn.functional as F

import attention_ref as AR
from conftest import load_golden
from oracle import restate as R

RTOL = 1e-12
B, H, W, C = 2, 12, 8, 5
h, w, L = H // 2, W // 2, (H // 2) * (W // 2)
F64 = torch.float64


def close(a, b, what):
    a, b = torch.as_tensor(a, dtype=F64), torch.as_tensor(b, dtype=F64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = (a - b).abs().max().item()
    assert err <= RTOL * max(b.abs().max().item(), 1e-300), (what, err, b.abs().max().item())


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def table(p):
    """restate._patches' [N][L][C][k][k] -> [N][L][k*k][C]."""
    n, l, c, k, _ = p.shape
    return p.permute(0, 1, 3, 4, 2).reshape(n, l, k * k, c)


def draw(seed=3):
    gen = torch.Generator().manual_seed(seed)
    f = torch.randn(B, H, W, C, generator=gen, dtype=F64)
    mask = torch.zeros(B, 8 * h, 8 * w, dtype=F64)
    mask[0, 16:30, 9:20] = 1      # sample 0: a hole; sample 1: another one
    mask[1, 0:10, 20:32] = 1
    return f, mask, gen


def restate_scores(fd_nchw):
    """The plain scores of restate.contextual_attention, [N][L_b][L_f] -> the device layout [N][p][l]."""
    n = fd_nchw.shape[0]
    wp = R._patches(fd_nchw, 3, 1)
    norm = torch.sqrt((wp ** 2).sum(dim=(2, 3, 4), keepdim=True))
    wn = wp / torch.max(norm, torch.tensor(1e-4, dtype=F64))
    xp = F.unfold(R._same_pad(fd_nchw, 3, 1), kernel_size=3, stride=1)
    return torch.bmm(wn.reshape(n, wp.shape[1], -1), xp).transpose(1, 2)


def restate_fuse(S, hh, ww):
    n, LL = S.shape[0], hh * ww
    S = R._diag_fuse(S)
    S = S.view(n, hh, ww, hh, ww).permute(0, 2, 1, 4, 3).reshape(n, LL, LL)
    S = R._diag_fuse(S)
    return S.view(n, ww, hh, ww, hh).permute(0, 2, 1, 4, 3).reshape(n, LL, LL)


def test_tables_mask_and_norms_match_the_restatement():
    f, mask, _ = draw()
    fd = AR.down(f)
    close(fd, nhwc(F.interpolate(nchw(f), scale_factor=0.5, mode='nearest', recompute_scale_factor=True)), 'down')
    wp, wpT = AR.patches3(fd)
    close(wp, table(R._patches(nchw(fd), 3, 1)), 'wp')
    close(wpT, wp.reshape(B, L, 9 * C).transpose(1, 2), 'wpT')
    assert wpT.shape == (B, 9 * C, L) and wpT.is_contiguous()
    raw, rawT = AR.raw_patches4(f)
    close(raw, table(R._patches(nchw(f), 4, 2)), 'raw')
    assert rawT.shape == (B, C, 16, L)
    close(rawT, raw.permute(0, 3, 2, 1), 'rawT')
    md = F.interpolate(mask.unsqueeze(1), scale_factor=1. / 8, mode='nearest', recompute_scale_factor=True)
    mm = (R._patches(md, 3, 1).mean(dim=(2, 3, 4)) == 0).to(F64)
    got = AR.patch_mask(mask, h, w)
    assert torch.equal(got, mm) and 0 < mm[0].sum() < L and not torch.equal(mm[0], mm[1])
    fz = f.clone()
    fz[:, 0:6, 0:6] = 0                         # patches (0,0), (0,1), (1,0), (1,1) all zero: the floor
    wz, _ = AR.patches3(AR.down(fz))
    norm, rnorm = AR.norms(wz)
    want = torch.sqrt((wz ** 2).sum(dim=(2, 3))).clamp_min(1e-4)
    close(norm, want, 'norm')
    close(rnorm, 1 / want, 'rnorm')
    assert norm[0, 0] == 1e-4 and norm[1, w + 1] == 1e-4 and rnorm[0, 0] == 1 / 1e-4


@pytest.mark.parametrize('hh,ww', [(6, 4), (4, 6), (5, 5), (2, 8)])
def test_fuse_matches_the_restatement_and_its_adjoint_autograd(hh, ww):
    LL = hh * ww
    gen = torch.Generator().manual_seed(hh * 16 + ww)
    S = torch.randn(B, LL, LL, generator=gen, dtype=F64)
    want = restate_fuse(S, hh, ww)
    close(AR.fuse(S, hh, ww, 0), want, 'fuse')
    # the restatement holds [l][p]; the device [p][l]: the operator treats both indices alike
    close(AR.fuse(S.transpose(1, 2).contiguous(), hh, ww, 0), want.transpose(1, 2), 'fuse of the transposed matrix')
    G = torch.randn(B, LL, LL, generator=gen, dtype=F64)
    Sa = S.clone().requires_grad_(True)
    (restate_fuse(Sa, hh, ww) * G).sum().backward()
    close(AR.fuse(G, hh, ww, 1), Sa.grad, 'fuse adjoint')
    if hh != ww:
        assert (AR.fuse(G, hh, ww, 1) - AR.fuse(G, hh, ww, 0)).abs().max() > 1e-3      # not its own adjoint: the two must not be swapped


def test_softmax_and_its_backward_match_autograd():
    gen = torch.Generator().manual_seed(11)
    S = torch.randn(B, L, L, generator=gen, dtype=F64)
    dA = torch.randn(B, L, L, generator=gen, dtype=F64)
    mm = (torch.rand(L, generator=gen) > 0.3).to(F64)
    Sa = S.clone().requires_grad_(True)
    want = F.softmax(Sa * mm.view(1, 1, L) * 10.0, dim=2) * mm.view(1, 1, L)
    (want * dA).sum().backward()
    A, top = AR.softmax(S, mm, 10.0)
    close(A, want.detach(), 'A')
    close(top, want.detach().sort(dim=2, descending=True).values[..., :2], 'top')
    assert bool((A[:, :, mm == 0] == 0).all())
    close(AR.softmax_backward(dA, A, mm, 10.0), Sa.grad, 'dS')
    mb = (torch.rand(B, L, generator=gen) > 0.3).to(F64)      # per-sample masks
    Ab, _ = AR.softmax(S, mb, 10.0)
    for b in range(B):
        close(Ab[b:b + 1], AR.softmax(S[b:b + 1], mb[b], 10.0)[0], 'per-sample mask')
    Az, _ = AR.softmax(S, torch.zeros(L, dtype=F64), 10.0)
    assert bool((Az == 0).all()) and bool((Az.argmax(dim=2) == 0).all())


def test_score_gradient_pieces_match_autograd_through_a_clamped_norm():
    """d fd of sum(dS0 * S0(fd)) from score_backward_prep + patches_backward against autograd of the restatement's scores.  A corner of the map is
    scaled to 1e-6, so that four patches have a norm below the floor 1e-4 with non-zero entries: the gradient through their norm is 0."""
    f, _, gen = draw(5)
    fd = AR.down(f)
    fd[:, 0:3, 0:3] *= 1e-6
    dS0 = torch.randn(B, L, L, generator=gen, dtype=F64)
    fa = nchw(fd).clone().requires_grad_(True)
    S0t = restate_scores(fa)
    (S0t * dS0).sum().backward()
    wp, _ = AR.patches3(fd)
    norm, rnorm = AR.norms(wp)
    assert int((norm == 1e-4).sum()) == 4 * B and bool((wp[:, w + 1].abs().sum(dim=(1, 2)) > 0).all())
    S0 = AR.scores(wp, rnorm)
    close(S0, S0t.detach(), 'S0')
    Gs, coef = AR.score_backward_prep(dS0, S0, norm, rnorm)
    assert bool((coef[norm == 1e-4] == 0).all()) and bool((coef[norm > 1e-4] != 0).all())
    dwp = torch.einsum('bij,bjk->bik', Gs, wp.flatten(2))
    df = AR.patches_backward(dwp, wp, coef, H, W)
    close(df[:, ::2, ::2], nhwc(fa.grad), 'd fd')
    odd = torch.ones(H, W, dtype=torch.bool)
    odd[::2, ::2] = False
    assert bool((df[:, odd] == 0).all())
    # without the clamp rule the result would differ: the test sees the rule
    _, coef_wrong = AR.score_backward_prep(dS0, S0, norm, rnorm, floor=0.0)
    assert (AR.patches_backward(dwp, wp, coef_wrong, H, W) - df).abs().max() > 1e-6 * df.abs().max()


def test_transpose():
    x = torch.randn(2, 5, 7, dtype=F64)
    t = AR.transpose(x)
    assert t.shape == (2, 7, 5) and t.is_contiguous() and torch.equal(t, x.permute(0, 2, 1))


def test_composed_block_matches_the_restatement_forward_and_backward():
    f, mask, gen = draw(7)
    dy = torch.randn(B, H, W, C, generator=gen, dtype=F64)
    fa = nchw(f).clone().requires_grad_(True)
    y, arg = R.contextual_attention(fa, fa, mask.unsqueeze(1), return_offsets=True)
    (y * nchw(dy)).sum().backward()
    fw = AR.attention_forward(f, mask)
    close(fw['y'], nhwc(y.detach()), 'y')
    assert torch.equal(fw['argmax'], arg.reshape(B, L))
    close(AR.attention_backward(fw, dy), nhwc(fa.grad), 'd f')
    # every sample under its own mask = that sample alone
    per = AR.attention_forward(f, mask, per_sample_mask=True)
    for b in range(B):
        yb = R.contextual_attention(nchw(f)[b:b + 1], nchw(f)[b:b + 1], mask[b:b + 1].unsqueeze(1))
        close(per['y'][b:b + 1], nhwc(yb), 'y under per-sample masks')


def test_composed_block_matches_fixture_g2():
    """The reference's own tensors (fp32): f, mask -> y, and coef as the output gradient -> grad_f, at the fixture's tolerance (tests/test_generator_gpu.py)."""
    g = load_golden('g2_attention')
    tol = 1e-3
    f = nhwc(g['f'].double())
    fw = AR.attention_forward(f, g['mask'].double()[:, 0])
    assert (nchw(fw['y']) - g['y'].double()).abs().max().item() <= tol
    df = AR.attention_backward(fw, nhwc(g['coef'].double()))
    assert (nchw(df) - g['grad_f'].double()).abs().max().item() <= tol * max(1.0, g['grad_f'].abs().max().item())


@pytest.mark.parametrize('name', sorted(AR.SOFTMAX_ROWS))
def test_softmax_rows_leave_at_most_one_percent_of_the_argmax_undecided(name):
    """By the reference alone: the seeds of tests/attention_ref.py's soft-max rows are chosen so that the device has to reproduce the arg-max of (nearly)
    every row exactly.  Also what the inputs promise: scale * S spans about +-30 and about a third of every mask is zero."""
    e = AR.softmax_expectation(name)
    Lr = AR.SOFTMAX_ROWS[name][0]
    assert (~e['decided']).float().mean().item() <= 0.01
    span = (AR.SOFTMAX_SCALE * e['S']).abs().amax(dim=2)
    assert 10 <= span.min().item() and span.max().item() <= 60, (span.min().item(), span.max().item())
    zeros = 1 - e['mm'].mean().item()
    assert (0.2 <= zeros <= 0.45) if Lr >= 100 else (0 < zeros < 0.7), zeros
    assert bool((e['A'][e['mm'].unsqueeze(1).expand_as(e['A']) == 0] == 0).all())


def test_flow_to_image_reproduces_the_flow_of_fixture_g2():
    """models/inpaint_tools.flow_to_image is the reference of hv_ca_flow in tests/test_attention_gpu.py: from the fp64 arg-max of the composed block it must give
    the reference's own recorded offset_flow, colour code for colour code (each wheel entry is divided by 255 BEFORE the blend: with the product first, a blend
    of two full entries falls to 254 where the reference has 255)."""
    from hvgan.models.inpaint_tools import flow_to_image
    g = load_golden('g2_attention')
    fw = AR.attention_forward(nhwc(g['f'].double()), g['mask'].double()[:, 0])
    n, hh, ww = g['f'].shape[0], fw['h'], fw['w']
    arg, pos = fw['argmax'], torch.arange(hh * ww)
    off = torch.stack([arg // ww - pos // ww, arg % ww - pos % ww], dim=2).view(n, hh, ww, 2)
    img = torch.from_numpy(flow_to_image(off.numpy())) / 255.
    up = g['flow'].shape[2] // hh
    flow = img.permute(0, 3, 1, 2).repeat_interleave(up, dim=2).repeat_interleave(up, dim=3)
    assert flow.shape == g['flow'].shape and float((flow - g['flow']).abs().max()) < 0.5 / 255


# ---------------------------------------------------------------------------------------------------------------- batched GEMM, fold, Gram route
@pytest.mark.parametrize('split', [0, 4, 3])
def test_bgemm_reference_matches_bmm_on_explicitly_permuted_rows(split):
    gen = torch.Generator().manual_seed(21 + split)
    bt, M, N, K = 3, 5, 12, 7
    A = torch.randn(bt, M, K, generator=gen, dtype=F64)
    Bm = torch.randn(bt, N, K, generator=gen, dtype=F64)
    cs = torch.randn(bt, N, generator=gen, dtype=F64)
    Bl = Bm
    if split:       # stored row c (N / split) + t is the logical row t split + c
        Bl = torch.empty_like(Bm)
        for c in range(split):
            for t in range(N // split):
                Bl[:, t * split + c] = Bm[:, c * (N // split) + t]
    for alpha, scale in ((1.0, None), (-0.25, cs)):
        Cr, S = AR.bgemm_nt(A, Bm, alpha, scale, split)
        want = alpha * torch.bmm(A, Bl.transpose(1, 2)) * (1 if scale is None else scale[:, None, :])
        close(Cr, want, 'C')
        close(S, abs(alpha) * torch.bmm(A.abs(), Bl.abs().transpose(1, 2)) * (1 if scale is None else scale.abs()[:, None, :]), 'S')
        assert bool((S >= Cr.abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize('HH,WW', [(4, 6), (6, 4), (2, 2), (8, 8)])
def test_fold_reference_is_F_fold_and_the_adjoint_of_the_raw_patches(HH, WW):
    gen = torch.Generator().manual_seed(HH * 16 + WW)
    LL = (HH // 2) * (WW // 2)
    src = torch.randn(B, LL, 16, C, generator=gen, dtype=F64)
    cols = src.permute(0, 3, 2, 1).reshape(B, C * 16, LL)                  # F.fold wants [b][c * 16 + tap][p]
    want = 0.25 * F.fold(cols, (HH, WW), kernel_size=4, stride=2, padding=1)
    close(AR.fold4(src, HH, WW, 0.25), nhwc(want), 'fold')
    f = torch.randn(B, HH, WW, C, generator=gen, dtype=F64)
    raw, _ = AR.raw_patches4(f)
    lhs, rhs = (AR.fold4(src, HH, WW) * f).sum().item(), (src * raw).sum().item()
    assert abs(lhs - rhs) <= 1e-12 * (src.abs() * raw.abs()).sum().item()


def test_gram_down_and_both_score_references_agree_on_a_non_square_map():
    f, _, _ = draw(13)
    f[:, 0:6, 0:6] = 0                                                    # four all-zero patches: the floor
    fd, fdT, q = AR.gram_down(f)
    close(fd, AR.down(f), 'fd')
    assert fdT.shape == (B, C, L) and fdT.is_contiguous()
    close(fdT, fd.reshape(B, L, C).transpose(1, 2), 'fdT')
    close(q, (fd.reshape(B, L, C) ** 2).sum(dim=2), 'q')
    S0, Sb, norm, rnorm = AR.gram_scores(fd)
    wp, _ = AR.patches3(fd)
    n2, r2 = AR.norms(wp)
    close(S0, AR.scores(wp, r2), 'S0 against scores()')
    close(S0, restate_scores(nchw(fd)), 'S0 against the restatement')
    close(norm, n2, 'norm')
    close(rnorm, r2, 'rnorm')
    assert norm[0, 0] == 1e-4 and bool((S0[:, :, 0] == 0).all()) and bool((Sb >= S0.abs() * (1 - 1e-12)).all())
    T0, Tb, n3, r3 = AR.gram_scores_box(fd)
    close(T0, S0, 'box-filter S0')
    close(Tb, Sb, 'box-filter bound')
    close(n3, norm, 'box-filter norm')
    close(r3, rnorm, 'box-filter rnorm')


def test_gram_backward_reference_matches_autograd_and_the_explicit_box_form():
    f, _, gen = draw(17)
    fd = AR.down(f)
    # symmetric Gs: autograd of sum 1/2 Gs[p][l] <wp[p], wp[l]>
    Gs = torch.randn(B, L, L, generator=gen, dtype=F64)
    Gs = Gs + Gs.transpose(1, 2)
    fa = fd.clone().requires_grad_(True)
    wpa = AR.patches3(fa)[0].flatten(2)
    (0.5 * Gs * torch.einsum('bpk,blk->bpl', wpa, wpa)).sum().backward()
    zero = torch.zeros(B, L, dtype=F64)
    close(AR.gram_backward(Gs, fd, zero), fa.grad, 'd fd, symmetric Gs')
    # non-symmetric Gs and a coefficient: E[a][b] = sum_t Gs[a + t][b + t], every term written out
    Gn = torch.randn(B, L, L, generator=gen, dtype=F64)
    coef = torch.randn(B, L, generator=gen, dtype=F64)
    E = torch.zeros(B, L, L, dtype=F64)
    cb = torch.zeros(B, h, w, dtype=F64)
    for ay in range(h):
        for ax in range(w):
            for ty in (-1, 0, 1):
                for tx in (-1, 0, 1):
                    if 0 <= ay - ty < h and 0 <= ax - tx < w:             # every patch a - t inside the grid holds pixel a
                        cb[:, ay, ax] += coef[:, (ay - ty) * w + ax - tx]
                    if not (0 <= ay + ty < h and 0 <= ax + tx < w):
                        continue
                    for by in range(h):
                        for bx in range(w):
                            if 0 <= by + ty < h and 0 <= bx + tx < w:
                                E[:, ay * w + ax, by * w + bx] += Gn[:, (ay + ty) * w + ax + tx, (by + ty) * w + bx + tx]
    close(AR.box_diag(Gn, h, w), E, 'E')
    close(AR.coef_box(coef, h, w)[..., 0], cb, 'coefficient sum')
    want = (E @ fd.reshape(B, L, C)).reshape(B, h, w, C) + cb.unsqueeze(3) * fd
    got = AR.gram_backward(Gn, fd, coef)
    close(got, want, 'd fd, non-symmetric Gs')
    # the same through the patch-table pieces that test_score_gradient_pieces... pins against autograd
    wp, _ = AR.patches3(fd)
    dwp = torch.einsum('bij,bjk->bik', Gn, wp.flatten(2))
    close(got, AR.patches_backward(dwp, wp, coef, H, W)[:, ::2, ::2], 'd fd against patches_backward')
    assert (got - AR.gram_backward(Gn.transpose(1, 2), fd, coef)).abs().max() > 1e-3      # the transposed Gs is another result
    bound = AR.gram_backward_bound(Gn, fd, coef)
    assert bool((bound >= got.abs() * (1 - 1e-12)).all())


def test_gram_lg_rule_and_the_exact_draws():
    assert [AR.gram_lg(*c) for c in ((1, 1), (2, 5), (3, 12), (2, 16), (2, 32), (2, 64))] == [4, 4, 4, 4, 4, 8]
    assert [AR.gram_lg(*c) for c in ((31, 17), (16, 32), (57, 9))] == [16, 16, 8]
    gen = torch.Generator().manual_seed(1)
    v = AR.draw_f16((1000,), gen)
    assert torch.equal(v, v.half().float()) and 0.5 <= v.abs().min().item() and v.abs().max().item() <= 1.5 and 0.3 < (v > 0).float().mean().item() < 0.7
    e = AR.draw_eighths((1000,), gen)
    assert torch.equal(e * 8, (e * 8).round()) and e.min().item() == -0.5 and e.max().item() == 0.5


@pytest.mark.parametrize('name', list(AR.GEMM_ROWS))
def test_gemm_rows_show_one_term_in_both_storage_types(name):
    """By the reference alone, for the seeds of tests/test_attention_gemm_gpu.py: the element bound (fp32 and fp16 result) lies below 1/20 of the mean
    |term| everywhere, and the results stay in fp16's normal range.  (The fp32 bound is (K + 2) u S against S / 20K: true whenever 20 K (K + 2) < 2^24,
    as for the Gram kernels' K = 576 and L + 1 <= 513; the fp16 share depends on the data.)"""
    M, N, K, batch = AR.GEMM_ROWS[name][:4]
    e = AR.gemm_case(name)
    assert e['ref'].shape == (batch, M, N) and bool((e['S'] > 0).all())
    assert AR.one_term_shows(AR.tol_sum(e['S'], K), e['S'], K) and AR.one_term_shows(AR.tol_sum(e['S'], K, e['ref']), e['S'], K)
    assert e['ref'].abs().max().item() < 6e4 and (e['ref'].abs() < 2.0 ** -14).double().mean().item() < 1e-3
    assert 20 * 576 * 578 < 2 ** 24 and 20 * 514 * 515 < 2 ** 24


@pytest.mark.parametrize('shape', AR.FOLD_SHAPES)
def test_fold_cases_show_one_term_in_both_storage_types(shape):
    e = AR.fold_case(shape)
    for acc in (0, 1):
        ref, S, n = e['ref'][acc], e['S'][acc], e['nterms'][acc]
        assert bool((S > 0).all()) and AR.one_term_shows(AR.tol_sum(S, n), S, n) and AR.one_term_shows(AR.tol_sum(S, n, ref), S, n)
    assert (e['ref'][1] - e['ref'][0]).abs().min().item() >= 0.5      # accumulate adds a non-zero map
