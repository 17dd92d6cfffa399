"""Plain float64 references of the contextual-attention glue stages (include/hvgan.h, "contextual attention pieces"), written from their definitions and
pinned against oracle/restate.py and torch autograd by tests/test_attention_ref_cpu.py.  Layouts are the device's: feature maps are [B][H][W][C], patch
tables [B][L][taps][C] with L = (H/2)(W/2) patch positions in row order, score matrices [B][p][l] (p: foreground position, l: background patch).

The batched NT GEMM, the fold and the Gram-route stages (csrc/bgemm.hip, csrc/attention_gram.hip) follow, with the rows and cases that
tests/test_attention_gemm_gpu.py runs them on.

The last part holds the soft-max test rows (inputs, fp64 expectation, element bound, decided rows): tests/test_attention_gpu.py compares the kernels
with them and tests/test_attention_ref_cpu.py checks, without a GPU, that the chosen seeds leave at most 1 % of the rows' arg-max undecided."""
import functools
import math

import torch
import torch.nn.functional as F

F64 = torch.float64
U = 2.0 ** -24
NORM_FLOOR = 1e-4


# ---------------------------------------------------------------------------------------------------------------- patch tables
def down(f):
    """Nearest x1/2: the even rows and columns of f [B][H][W][C]."""
    return f[:, ::2, ::2, :].contiguous()


def _windows(x, k, step):
    """Every k x k window of x [B][H][W][C] zero-padded by one pixel all round, taken every `step` pixels: [B][(H/step)(W/step)][k*k][C], taps in row order."""
    B, H, W, C = x.shape
    h, w = H // step, W // step
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    taps = [xp[:, ty:ty + step * h:step, tx:tx + step * w:step, :] for ty in range(k) for tx in range(k)]
    return torch.stack(taps, dim=3).reshape(B, h * w, k * k, C)


def _unwindows(t, k, step, H, W):
    """Adjoint of _windows: every tap of every window added back to the pixel it was read from -> [B][H][W][C]."""
    B, L, _, C = t.shape
    h, w = H // step, W // step
    acc = torch.zeros(B, H + 2, W + 2, C, dtype=t.dtype)
    t = t.reshape(B, h, w, k * k, C)
    for ty in range(k):
        for tx in range(k):
            acc[:, ty:ty + step * h:step, tx:tx + step * w:step, :] += t[:, :, :, ty * k + tx, :]
    return acc[:, 1:H + 1, 1:W + 1, :].contiguous()


def patches3(fd):
    """3x3 stride-1 patches of the down-sampled map: wp [B][L][9][C] and its transposed copy wpT [B][9C][L]."""
    wp = _windows(fd, 3, 1)
    return wp, wp.flatten(2).transpose(1, 2).contiguous()


def raw_patches4(f):
    """4x4 stride-2 'same' patches of the full map: raw [B][L][16][C] and rawT [B][C][16][L]."""
    raw = _windows(f, 4, 2)
    return raw, raw.permute(0, 3, 2, 1).contiguous()


def norms(wp, floor=NORM_FLOOR):
    """norm [B][L] = max(|patch|, floor) and its reciprocal."""
    n = wp.flatten(2).pow(2).sum(dim=2).sqrt().clamp_min(floor)
    return n, 1.0 / n


def patch_mask(mask, h, w):
    """mask [B][Himg][Wimg] -> mm [B][h*w]: 1 where the 3x3 patch of the nearest-down-sampled mask (every Himg/h-th row, Wimg/w-th column) is all zero."""
    md = mask[:, ::mask.shape[1] // h, ::mask.shape[2] // w][:, :h, :w].unsqueeze(3)
    return (_windows(md, 3, 1).sum(dim=(2, 3)) == 0).to(mask.dtype)


# ---------------------------------------------------------------------------------------------------------------- score fusion
def _shift(n):
    return torch.diag(torch.ones(n - 1, dtype=F64), 1)      # (D x)[i] = x[i + 1]


def _diag3(X, D):
    """X[i][j] + X[i+1][j+1] + X[i-1][j-1], out-of-range terms dropped: the 3-tap identity filter on the score matrix.  Its own adjoint."""
    return X + D @ X @ D.T + D.T @ X @ D


def fuse(S, h, w, adjoint=0):
    """Score fusion on S [B][p][l]: the diagonal 3-tap sum with both positions counted in row order, then the same with both counted in column order.
    adjoint=1 applies the transposed operator (each of the two sums is symmetric, so it is the two in the other order)."""
    L = h * w
    D = _shift(L)
    col = torch.arange(L).view(h, w).t().reshape(-1)      # col[k]: row-order index of the k-th position in column order
    P = torch.zeros(L, L, dtype=F64)
    P[torch.arange(L), col] = 1                            # (P x)[k] = x[col[k]]
    by_rows = lambda X: _diag3(X, D)
    by_cols = lambda X: P.T @ _diag3(P @ X @ P.T, D) @ P
    return by_rows(by_cols(S)) if adjoint else by_cols(by_rows(S))


# ---------------------------------------------------------------------------------------------------------------- soft-max
def _per_row(mm, S):
    """mm [L] (shared) or [B][L] (per sample) -> broadcastable against S [B][p][l]."""
    return mm.view(1, 1, -1) if mm.dim() == 1 else mm.unsqueeze(1)


def softmax(S, mm, scale):
    """A = softmax_l(S mm scale) mm: a masked column enters with logit 0, takes its share of the mass and is zeroed afterwards.
    -> A, top [B][p][2] (the two largest values of every row, largest first)."""
    m = _per_row(mm, S)
    A = torch.softmax(S * m * scale, dim=2) * m
    return A, torch.topk(A, min(2, A.shape[2]), dim=2).values


def softmax_backward(dA, A, mm, scale):
    """dS = scale mm A (dA - sum_l dA A), one mask [L] for every sample."""
    dot = (dA * A).sum(dim=2, keepdim=True)
    return scale * mm.view(1, 1, -1) * A * (dA - dot)


# ---------------------------------------------------------------------------------------------------------------- matching scores and their gradient
def scores(wp, rnorm):
    """S0[b][p][l] = <patch p, patch l> / norm[l]: the patches are both the filters (l, normalised) and the inputs (p)."""
    w = wp.flatten(2)
    return torch.einsum('bpk,blk->bpl', w, w) * rnorm.unsqueeze(1)


def score_backward_prep(dS, S0, norm, rnorm, floor=NORM_FLOOR):
    """Gs[b][i][j] = dS[b][j][i] rnorm[i] + dS[b][i][j] rnorm[j] (d wp = Gs wp: patch i as filter and as input);
    coef[b][l] = -(sum_p dS[p][l] S0[p][l]) / norm[l]^2, the gradient through the norm -- 0 where the norm sits at its floor."""
    Gs = dS.transpose(1, 2) * rnorm.unsqueeze(2) + dS * rnorm.unsqueeze(1)
    coef = torch.where(norm > floor, -(dS * S0).sum(dim=1) / (norm * norm), torch.zeros_like(norm))
    return Gs, coef


def patches_backward(dwp, wp, coef, H, W):
    """col2im of dwp + coef wp ([B][L][9][C]) to the down-sampled map, placed on the even positions of a zero [B][H][W][C] map."""
    B, L, _, C = wp.shape
    g = dwp.reshape(B, L, 9, C) + coef.view(B, L, 1, 1) * wp
    df = torch.zeros(B, H, W, C, dtype=wp.dtype)
    df[:, ::2, ::2, :] = _unwindows(g, 3, 1, H // 2, W // 2)
    return df


def transpose(x):
    return x.transpose(1, 2).contiguous()


# ---------------------------------------------------------------------------------------------------------------- batched GEMM, fold, Gram route
def bgemm_nt(A, B, alpha=1.0, colscale=None, b_split=0):
    """C[b][m][n] = alpha cs[b][n] sum_k A[b][m][k] B'[b][n][k] for A [batch][M][K], B [batch][N][K] as stored: with b_split the logical row
    n = t b_split + c of B' is the stored row c (N / b_split) + t.  -> C and S = |alpha cs| sum_k |A B'| (what the rounding error of any summation
    order is bounded by), both fp64."""
    A, B = A.double(), B.double()
    batch, N, K = B.shape
    if b_split:
        n = torch.arange(N)
        B = B[:, (n % b_split) * (N // b_split) + n // b_split, :]
    cs = torch.full((batch, N), float(alpha), dtype=F64)
    if colscale is not None:
        cs = cs * colscale.double()
    C = torch.einsum('bmk,bnk->bmn', A, B) * cs.unsqueeze(1)
    S = torch.einsum('bmk,bnk->bmn', A.abs(), B.abs()) * cs.abs().unsqueeze(1)
    return C, S


def fold4(src, H, W, alpha=1.0):
    """Overlap-add of 4x4 stride-2 pad-1 patches src [B][L][16][C] (L = (H/2)(W/2), taps in row order) -> alpha times the sum per pixel, [B][H][W][C]:
    the adjoint of raw_patches4."""
    return alpha * _unwindows(src.double(), 4, 2, H, W)


def gram_down(f):
    """f [B][H][W][C] -> fd [B][h][w][C] (nearest x1/2), fdT [B][C][L] and q [B][L] = |fd|^2 per pixel."""
    fd = down(f)
    flat = fd.flatten(1, 2)
    return fd, flat.transpose(1, 2).contiguous(), flat.pow(2).sum(dim=2)


def gram_scores(fd):
    """The matching scores from the patch definition, fd [B][h][w][C] -> S0 [B][p][l] = rnorm[l] <wp[p], wp[l]>, the element bound
    rnorm[l] <|wp[p]|, |wp[l]|>, norm, rnorm [B][L]."""
    wp, _ = patches3(fd.double())
    norm, rnorm = norms(wp)
    w = wp.flatten(2)
    S0 = torch.einsum('bpk,blk->bpl', w, w) * rnorm.unsqueeze(1)
    Sb = torch.einsum('bpk,blk->bpl', w.abs(), w.abs()) * rnorm.unsqueeze(1)
    return S0, Sb, norm, rnorm


def box_diag(G, h, w):
    """E[a][b] = sum over the 3x3 offsets t of G[a + t][b + t] for G [B][L][L] over an h x w grid; terms with a + t or b + t outside the grid dropped."""
    B = G.shape[0]
    Gp = F.pad(G.reshape(B, h, w, h, w), (1, 1, 1, 1, 1, 1, 1, 1))
    E = torch.zeros(B, h, w, h, w, dtype=G.dtype)
    for ty in range(3):
        for tx in range(3):
            E += Gp[:, ty:ty + h, tx:tx + w, ty:ty + h, tx:tx + w]
    return E.reshape(B, h * w, h * w)


def gram_scores_box(fd):
    """gram_scores by the box-filter identity <wp[p], wp[l]> = sum_t <fd[p + t], fd[l + t]> (K = C instead of 9C; for the large cases): the same four
    results.  The bound's identity holds with |fd| in place of fd."""
    fd = fd.double()
    B, h, w, C = fd.shape
    x = fd.flatten(1, 2)
    norm, rnorm = norms(patches3(fd)[0])
    S0 = box_diag(x @ x.transpose(1, 2), h, w) * rnorm.unsqueeze(1)
    Sb = box_diag(x.abs() @ x.abs().transpose(1, 2), h, w) * rnorm.unsqueeze(1)
    return S0, Sb, norm, rnorm


def coef_box(coef, h, w):
    """[B][L] -> [B][h][w][1]: sum_t coef[a - t], the coefficient of every patch that holds pixel a."""
    B, L = coef.shape
    return _unwindows(coef.reshape(B, L, 1, 1).expand(B, L, 9, 1), 3, 1, h, w)


def gram_backward(Gs, fd, coef):
    """d fd [B][h][w][C] = col2im(Gs wp) + (sum_t coef[a - t]) fd[a]: the K = 9C route written out (hv_ca_gram_backward takes it through E = box_diag(Gs))."""
    fd, Gs = fd.double(), Gs.double()
    B, h, w, C = fd.shape
    wp, _ = patches3(fd)
    dwp = torch.einsum('bij,bjk->bik', Gs, wp.flatten(2)).reshape(B, h * w, 9, C)
    return _unwindows(dwp, 3, 1, h, w) + coef_box(coef.double(), h, w) * fd


def gram_backward_bound(Gs, fd, coef):
    """sum_b |E[a][b] fd[b]| + |sum_t coef[a - t]| |fd[a]|: the L + 1 terms of the Gram form's sum per element, [B][h][w][C]."""
    fd = fd.double()
    B, h, w, C = fd.shape
    E = box_diag(Gs.double(), h, w)
    return (E.abs() @ fd.flatten(1, 2).abs()).reshape(B, h, w, C) + coef_box(coef.double(), h, w).abs() * fd.abs()


def gram_lg(B, h):
    """Grid rows of l per workgroup, by hv_ca_gram_scores' rule (csrc/attention_gram.hip): 16, halved down to 4 while fewer than 1024 workgroups result."""
    lg = 16
    while lg > 4 and B * h * ((h + lg - 1) // lg) < 1024:
        lg >>= 1
    return (lg + 3) // 4 * 4


def draw_f16(shape, gen):
    """Values of magnitude 0.5 .. 1.5 with random sign, rounded to fp16 (returned as fp32): no term of a sum is negligible beside the others."""
    v = (torch.rand(shape, generator=gen) + 0.5) * (torch.randint(0, 2, shape, generator=gen) * 2 - 1)
    return v.half().float()


def draw_eighths(shape, gen):
    """Multiples of 1/8 in [-1/2, 1/2]: sums of a few of them are exact in fp32 and fp16."""
    return torch.randint(-4, 5, shape, generator=gen).float() / 8


def tol_sum(S, nterms, ref=None):
    """(nterms + 2) u S: the worst case of an fp32 sum of nterms exact products in any order; 2^-11 |ref| + 2^-25 more for a result stored as fp16."""
    t = (nterms + 2) * U * S
    return t if ref is None else t + 2.0 ** -11 * ref.abs() + 2.0 ** -25


def one_term_shows(bound, S, nterms):
    """The bound lies below 1/20 of the mean |term| = S / nterms wherever the sum has a term at all: a dropped or doubled term cannot hide in it."""
    m = S > 0
    return bool((bound[m] < S[m] / (20.0 * nterms)).all())


# name: (M, N, K, batch, alpha, column scale, b_split, padded leading dimensions and batch strides)
GEMM_ROWS = {
    'one_kstep': (16, 4, 32, 1, 1.0, False, 0, False),
    'ragged_bn64': (129, 132, 96, 3, 0.25, True, 4, True),
    'swizzle': (128, 128, 64, 8, 1.0, False, 32, False),
    'plain_bn128': (130, 256, 64, 9, -0.5, True, 0, True),
    'dma_128_tiles': (256, 256, 64, 128, 1.0, False, 0, False),
    'dma_ragged': (257, 260, 128, 32, 0.5, False, 0, False),
    'dma_one_tile_short': (256, 256, 64, 127, 1.0, False, 0, False),
    'dma_k96': (256, 256, 96, 128, 1.0, False, 0, False),
    'dma_split_scaled_padded': (256, 512, 64, 65, 0.25, True, 4, True),
}


def gemm_takes_dma(M, N, K, batch):
    """bgemm_impl's rule for fp16 x fp16 operands (csrc/bgemm.hip)."""
    t256 = -(-M // 256) * -(-N // 256) * batch
    return K % 64 == 0 and M >= 256 and N >= 256 and t256 >= 128


@functools.lru_cache(maxsize=1)
def gemm_case(name):
    M, N, K, batch, alpha, scaled, split, padded = GEMM_ROWS[name]
    gen = torch.Generator().manual_seed(7000 + sorted(GEMM_ROWS).index(name))
    A, B = draw_f16((batch, M, K), gen), draw_f16((batch, N, K), gen)
    cs = (torch.rand(batch, N, generator=gen) + 0.5) if scaled else None
    ref, S = bgemm_nt(A, B, alpha, cs, split)
    return dict(A=A, B=B, cs=cs, ref=ref, S=S)


FOLD_SHAPES = [(2, 4, 6, 8), (1, 2, 2, 16), (3, 6, 4, 24), (2, 4, 6, 12)]
FOLD_ALPHA = 0.25


@functools.lru_cache(maxsize=4)
def fold_case(shape):
    """src [B][L][16][C], old [B][H][W][C] (fp16 values) -> for accumulate 0 / 1: the fp64 result, the sum of its |terms| and their number."""
    B, H, W, C = shape
    gen = torch.Generator().manual_seed(8000 + FOLD_SHAPES.index(shape))
    src, old = draw_f16((B, (H // 2) * (W // 2), 16, C), gen), draw_f16((B, H, W, C), gen)
    f, fa = fold4(src, H, W, FOLD_ALPHA), fold4(src.abs(), H, W, FOLD_ALPHA)
    return dict(src=src, old=old, ref=(f, old.double() + f), S=(fa, old.double().abs() + fa), nterms=(4, 5))


# ---------------------------------------------------------------------------------------------------------------- the block, composed
def attention_forward(f, mask, scale=10.0, per_sample_mask=False):
    """ContextualAttention(f, f, mask) from the pieces above.  f [B][H][W][C], mask [B][Himg][Wimg] -> dict of every intermediate; 'y' [B][H][W][C], 'argmax' [B][L]."""
    B, H, W, C = f.shape
    h, w = H // 2, W // 2
    fd = down(f)
    wp, _ = patches3(fd)
    raw, _ = raw_patches4(f)
    norm, rnorm = norms(wp)
    mm = patch_mask(mask, h, w)
    mm = mm if per_sample_mask else mm[0]
    S0 = scores(wp, rnorm)
    S1 = fuse(S0, h, w)
    A, _ = softmax(S1, mm, scale)
    O = torch.einsum('bpl,blk->bpk', A, raw.flatten(2)).reshape(B, h * w, 16, C)
    y = 0.25 * _unwindows(O, 4, 2, H, W)
    return dict(fd=fd, wp=wp, raw=raw, norm=norm, rnorm=rnorm, mm=mm, S0=S0, S1=S1, A=A, y=y, argmax=A.argmax(dim=2), h=h, w=w, scale=scale)


def attention_backward(fw, dy):
    """d f of attention_forward (shared mask) for the output gradient dy [B][H][W][C], through the backward pieces above."""
    B, H, W, C = dy.shape
    h, w, A, raw, wp = fw['h'], fw['w'], fw['A'], fw['raw'], fw['wp']
    dO = 0.25 * _windows(dy, 4, 2).flatten(2)                                     # [B][p][16 C]
    dA = torch.einsum('bpk,blk->bpl', dO, raw.flatten(2))
    df = _unwindows(torch.einsum('bpl,bpk->blk', A, dO).reshape(B, h * w, 16, C), 4, 2, H, W)      # through the pasted raw patches
    dS1 = softmax_backward(dA, A, fw['mm'], fw['scale'])
    dS0 = fuse(dS1, h, w, adjoint=1)
    Gs, coef = score_backward_prep(dS0, fw['S0'], fw['norm'], fw['rnorm'])
    dwp = torch.einsum('bij,bjk->bik', Gs, wp.flatten(2))
    return df + patches_backward(dwp, wp, coef, H, W)


# ================================================================================================================ soft-max test rows
def tol_elem(ref, floor, f16):
    """4 x (the largest error of a plain fp32 evaluation) + 4u |ref| per element; max(2^-11 |ref|, 2^-25) more for a value stored as fp16."""
    t = 4 * floor + 4 * U * ref.abs()
    return t + torch.clamp(2.0 ** -11 * ref.abs(), min=2.0 ** -25) if f16 else t


# name: (L, B, entry, S base offset in floats, mask stride: 0 shared / 'L' / 'L+1').  entry: plain = hv_ca_softmax, batched, f16.
SOFTMAX_ROWS = {
    'wave256': (256, 3, 'plain', 0, 0),
    'wave256_masks': (256, 3, 'batched', 0, 'L'),
    'wave1024': (1024, 2, 'plain', 0, 0),
    'wave1024_masks': (1024, 2, 'f16', 0, 'L'),
    'wave4096': (4096, 1, 'plain', 0, 0),
    'wave4096_f16': (4096, 1, 'f16', 0, 0),
    'reg256_offset': (256, 3, 'plain', 1, 0),
    'reg1024_offset': (1024, 2, 'plain', 1, 0),
    'reg256_stride': (256, 3, 'batched', 0, 'L+1'),
    'reg1024_stride': (1024, 2, 'batched', 0, 'L+1'),
    'reg512': (512, 2, 'batched', 0, 'L'),
    'reg512_f16': (512, 2, 'f16', 0, 0),
    'reg2048': (2048, 1, 'plain', 0, 0),
    'gen16': (16, 2, 'batched', 0, 'L'),
    'gen100': (100, 2, 'plain', 0, 0),
    'gen300': (300, 2, 'batched', 0, 'L'),
    'gen300_f16': (300, 2, 'f16', 0, 'L'),
    'gen2304': (2304, 1, 'plain', 0, 0),
}
SOFTMAX_SCALE = 10.0


def softmax_inputs(name):
    """S [B][L][L] fp32 with scale * S spanning about +-30 within a row (normal, 3 / sqrt(2 ln L) wide), masks [B][L] with about a third zeros
    (all rows alike for a shared mask)."""
    L, B, entry, s_off, stride = SOFTMAX_ROWS[name]
    gen = torch.Generator().manual_seed(4000 + sorted(SOFTMAX_ROWS).index(name))
    S = torch.randn(B, L, L, generator=gen) * (3.0 / math.sqrt(2 * math.log(L)))
    nm = B if stride else 1
    mm = (torch.rand(nm, L, generator=gen) >= 1 / 3).float()
    return S, mm.expand(B, L).contiguous()


@functools.lru_cache(maxsize=1)
def softmax_expectation(name):
    """-> dict: S, mm (fp32 inputs), A (fp64), tol (element bound of the stored A), idx (the reference's arg-max), decided [B][L] (bool), margin [B][L].
    A row is decided when its largest A exceeds the second largest by more than twice the element bound.  The kernels take the arg-max on the fp32
    values before they are stored, so the margin is the fp32 bound for the fp16-stored matrix as well."""
    L, B, entry, s_off, stride = SOFTMAX_ROWS[name]
    S, mm = softmax_inputs(name)
    A, top = softmax(S.double(), mm.double(), SOFTMAX_SCALE)
    A32 = torch.softmax(S * mm.unsqueeze(1) * torch.tensor(SOFTMAX_SCALE, dtype=torch.float32), dim=2) * mm.unsqueeze(1)
    floor = (A32.double() - A).abs().max().item()
    del A32
    margin = 2 * tol_elem(top[..., 0], floor, False)
    decided = (top[..., 0] - top[..., 1]) > margin
    return dict(S=S, mm=mm, A=A, tol=tol_elem(A, floor, entry == 'f16'), idx=A.argmax(dim=2), decided=decided, margin=margin, top=top[..., 0], floor=floor)
