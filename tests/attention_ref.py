"""Plain float64 references of the contextual-attention glue stages (include/hvgan.h, "contextual attention pieces"), written from their definitions and
pinned against oracle/restate.py and torch autograd by tests/test_attention_ref_cpu.py.  Layouts are the device's: feature maps are [B][H][W][C], patch
tables [B][L][taps][C] with L = (H/2)(W/2) patch positions in row order, score matrices [B][p][l] (p: foreground position, l: background patch).

The second half holds the soft-max test rows (inputs, fp64 expectation, element bound, decided rows): tests/test_attention_gpu.py compares the kernels
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
