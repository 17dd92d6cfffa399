"""Plain fp64 references of the weight path of csrc/prep.hip -- spectral norm, the kernel-layout weight tables, the spectral-norm backward, Adam and the
overflow guard's unscale / check -- with the a-priori error bounds and the case lists that tests/test_weight_path_gpu.py (device) and
tests/test_weight_ref_cpu.py (pins the references, measures that the bounds have teeth) share.  torch / numpy on the CPU, no device code.

The `*_ref` functions take the fp32 values the kernel is given and evaluate in double.  The `*_formula` functions evaluate one element-wise formula in
the dtype of their arguments: the references call them in fp64, the tests in fp32 to measure what a plain fp32 evaluation of the same formula loses
(the error floor of the element-wise rule).  u = 2^-24 throughout.

Bounds (all from fp64 reference quantities, first order in u):
  a length-n fp32 dot        (n + 2) u sum |term_i|, whatever the summation order (dot_bound);
  spectral norm              that bound on every dot of the iteration, carried through v' = t / |t|, s = W v', u' = s / |s| and sigma = u' . s by the
                             derivatives of those steps, absolute values throughout (spectral_norm_bounds); a norm of n squares adds ((n + 2) / 2 + 1) u
                             of itself, a quotient u of itself;
  element-wise values        4 x floor + 4u |ref| (tol_elem), the floor measured by the caller from the fp32 `*_formula`;
  Adam's shared scalars      bc = 1 - beta^step comes from the device powf: P_POWF u beta^step / bc relative, once for step_size = lr / bc1 and half of it
                             for sqrt(bc2), times the size of the update (adam_bc_term)."""
import functools
import math

import numpy as np
import torch

U = 2.0 ** -24
# ULP accuracy of the device powf.  The ROCm install carries no HIP math-accuracy table to read it from: 4 is ASSUMED, not measured.
P_POWF = 4
FINITE_MAX = float(np.float32(3.0e38))      # grad_unscale_check_kernel: |g| above this counts as an overflow, as inf and nan do
SN_MAXK, SN_MAXCO = 4608, 1024              # weight_prep_kernel's PREP_MAXK / PREP_MAXCO (LDS staging of v and u)

# Cout, Cin, k of the spectral-norm cases (weight_prep_kernel: 512 threads = 8 waves; rows in groups of 32; K walked 64 per wave, 512 per block)
SN_SHAPES = [(1, 1, 3), (7, 7, 3), (8, 4, 4), (33, 65, 1), (100, 57, 3), (32, 33, 3), (64, 128, 3), (8, 512, 3), (1024, 4, 2)]
SN_LIMIT = [(8, 512, 3), (1024, 4, 2)]      # K = 4608 and Cout = 1024: the limits; their dot bounds are too loose for single-element mutants
SN_SMALL = [s for s in SN_SHAPES if s not in SN_LIMIT]
# the existing layout test's list (tests/test_conv_gpu.py), as Cout, Cin, k
LAYOUT_SHAPES = [(64, 1, 4), (128, 64, 4), (512, 256, 4), (1, 512, 4), (32, 33, 3), (64, 64, 3), (1, 8, 3), (16, 4, 5), (40, 24, 3)]
TRANSPOSED_SHAPES = [(8, 16, 4), (20, 33, 4)]      # Cout, Cin, k of conv-transpose sources [Cin][Cout][taps]

# hv_weight_prep_backward: name -> (Cout, Cin, taps); no = Cout Cin taps in {36, 1023, 1024, 1025, 9225}, padded n = Cout taps CinP below 4 * 512, exactly 8192,
# 8192 + 4, one unrolled round + tail (12300) and two rounds + tail (20736)
BWD_CASES = {
    'no36': (4, 1, 9), 'no1023': (31, 33, 1), 'no1024': (16, 64, 1), 'no1025': (41, 1, 25), 'no9225': (123, 3, 25),
    'n8192': (32, 64, 4), 'n8196': (683, 3, 3), 'n20736': (64, 33, 9),
}
BWD_TRANSPOSED = {'tr33': (33, 20, 16), 'tr5': (5, 3, 4)}      # transposed_src, ragged Cout (the padded width of dw_ohwi)

ADAM_SIZES = [1, 255, 1023, 1024, 1025, 4099]
ADAM_STEPS = [1, 2, 10, 1000]
ADAM_HYPER = dict(lr=2e-4, beta1=0.5, beta2=0.999, eps=1e-8)
GUARD_SIZES = [1, 3, 4, 5, 4095, 4096, 4097, 256 * 4096 + 5]


def rup(a, b):
    return (a + b - 1) // b * b


def f32(x):
    """The fp32 rounding of a Python float, as a Python float (what a float argument of the C ABI carries)."""
    return float(np.float32(x))


def tol_elem(ref, floor):
    return 4 * floor + 4 * U * ref.abs()


def dot_bound(abs_term_sum, n):
    return (n + 2) * U * abs_term_sum


def exact_values(gen, *shape):
    """Non-zero multiples of 1/8 in [-1/2, 1/2]: products of two or three and all their partial sums are exact in fp32 (exact_ok)."""
    k = torch.randint(1, 5, shape, generator=gen).float()
    return k / 8 * (torch.randint(0, 2, shape, generator=gen).float() * 2 - 1)


def exact_ok(abs_term_sum, grid):
    """Every partial sum of terms that are multiples of 1/grid is an integer multiple of 1/grid below 2^24 / grid: exactly representable."""
    return float(abs_term_sum) * grid < 2 ** 24


# ---------------------------------------------------------------------------------------------------------------- spectral norm
def sn_inputs(cout, cin, k, exact=False):
    """W [Cout][K], u, v as fp32: random W of a conv initialisation's size, random u and v that are NOT unit vectors."""
    K = cin * k * k
    gen = torch.Generator().manual_seed(cout * 7919 + cin * 101 + k + (5000 if exact else 0))
    if exact:
        return exact_values(gen, cout, K), exact_values(gen, cout), exact_values(gen, K)
    return torch.randn(cout, K, generator=gen) / math.sqrt(K), torch.randn(cout, generator=gen) * 0.7, torch.randn(K, generator=gen) * 1.3


def normalize(x, eps=1e-12):
    return x / max(float(x.norm()), eps)


def spectral_norm_ref(W, u, v, power_iter, eps=1e-12):
    """torch.nn.utils.spectral_norm's forward pre-hook: one power iteration (train) or none (eval) -> (sigma, u', v') in double."""
    W, u, v = W.double(), u.double(), v.double()
    if power_iter:
        v = normalize(W.t() @ u, eps)
        u = normalize(W @ v, eps)
    return torch.dot(u, W @ v), u, v


def spectral_norm_bounds(W, u, v, power_iter, du=None, dv=None):
    """|error| bounds of (sigma, u', v') for a kernel that evaluates spectral_norm_ref with fp32 dots in any order; du, dv: bounds of errors its INPUT u, v
    already carry (the second of two chained calls)."""
    W, u, v = W.double(), u.double(), v.double()
    A = W.abs()
    co, K = W.shape
    du = torch.zeros_like(u) if du is None else du
    dv = torch.zeros_like(v) if dv is None else dv
    if not power_iter:
        s = W @ v
        bs = dot_bound(A @ v.abs(), K) + A @ dv
        return dot_bound((u * s).abs().sum(), co) + (u.abs() * bs).sum() + (du * s.abs()).sum(), du, dv
    t = W.t() @ u
    bt = dot_bound(A.t() @ u.abs(), co) + A.t() @ du
    nv = float(t.norm())
    dnv = float((t.abs() * bt).sum()) / nv + nv * ((K + 2) / 2 + 1) * U
    vn = t / nv
    bv = bt / nv + vn.abs() * (dnv / nv + U)
    s = W @ vn
    bs = dot_bound(A @ vn.abs(), K) + A @ bv
    nu = float(s.norm())
    dnu = float((s.abs() * bs).sum()) / nu + nu * ((co + 2) / 2 + 1) * U
    un = s / nu
    bu = bs / nu + un.abs() * (dnu / nu + U)
    bsig = dot_bound((un * s).abs().sum(), co) + (un.abs() * bs).sum() + (s.abs() * bu).sum()
    return bsig, bu, bv


# ---------------------------------------------------------------------------------------------------------------- weight tables
def tiled_index(row, tap, k, taps, K, T):
    """Half index of (row, tap, k) in the MFMA-fragment order documented at hv_weight_tile_f16 (include/hvgan.h)."""
    q = T // 4
    return (row // 16) * 16 * taps * K + ((tap * K + k) // T) * 16 * T + (((k % T) // q) * 16 + row % 16) * q + k % q


def tile_width(K):
    return 32 if K % 32 == 0 else 16 if K % 16 == 0 else 0


@functools.lru_cache(maxsize=64)
def _tiled_indices(rows, taps, K, T):
    r, t, k = np.meshgrid(np.arange(rows), np.arange(taps), np.arange(K), indexing='ij')
    return torch.from_numpy(tiled_index(r, t, k, taps, K, T).ravel())


def tile_table(plain_h, rows, taps, K):
    """fp16 [rows][taps][K] -> (its fragment-ordered form with zero padding rows, mask of the halfs that belong to real rows), or (None, None)."""
    T = tile_width(K)
    if not T:
        return None, None
    idx = _tiled_indices(rows, taps, K, T)
    out = torch.zeros(rup(rows, 16) * taps * K, dtype=torch.float16)
    out[idx] = plain_h.reshape(-1)
    real = torch.zeros(out.numel(), dtype=torch.bool)
    real[idx] = True
    return out, real


def source_weight(W, cout, cin, taps, transposed_src):
    """The flat fp32 source in its torch layout -> logical [Cout][Cin][taps]."""
    return W.reshape(cin, cout, taps).permute(1, 0, 2) if transposed_src else W.reshape(cout, cin, taps)


def weight_tables_ref(W, sigma32, cout, cin, taps, CinP, CoutF, CoutP, CinB, transposed_src=False, K2=0):
    """All tables hv_weight_prep / hv_weight_prep2 write, from the STORED fp32 sigma: w_fwd [CoutF][taps][CinP] and w_bwd [CinB][taps][CoutP] (fp32, zero
    beyond the real extents), their fp16 roundings (_h) and the fragment-ordered forms (_t, with `_real` masks; None where the width has none); w_fwd_t2:
    the first K2 channels of w_fwd_h as a fragment-ordered table of their own.  The quotient is taken in double and rounded once to fp32: for a
    division of two fp32 values that IS the correctly rounded fp32 quotient (53 >= 2 * 24 + 2 bits)."""
    q = (source_weight(W.double(), cout, cin, taps, transposed_src) / float(sigma32)).float()      # [Cout][Cin][taps]
    fwd = torch.zeros(CoutF, taps, CinP)
    ro, ri = min(cout, CoutF), min(cin, CinP)
    fwd[:ro, :, :ri] = q[:ro, :ri].permute(0, 2, 1)
    bwd = torch.zeros(CinB, taps, CoutP)
    ro, ri = min(cout, CoutF, CoutP), min(cin, CinP, CinB)
    bwd[:ri, :, :ro] = q[:ro, :ri].permute(1, 2, 0)
    out = {'w_fwd': fwd, 'w_bwd': bwd, 'w_fwd_h': fwd.half(), 'w_bwd_h': bwd.half()}
    out['w_fwd_t'], out['w_fwd_t_real'] = tile_table(out['w_fwd_h'], CoutF, taps, CinP)
    out['w_bwd_t'], out['w_bwd_t_real'] = tile_table(out['w_bwd_h'], CinB, taps, CoutP)
    out['w_fwd_t2'], out['w_fwd_t2_real'] = tile_table(out['w_fwd_h'][:, :, :K2].contiguous(), CoutF, taps, K2) if K2 else (None, None)
    return out


# ---------------------------------------------------------------------------------------------------------------- spectral-norm backward
def bwd_inputs(cout, cin, taps, transposed_src=False, exact=False, sentinel=7.5):
    """fp32 inputs of one hv_wprep_bwd_layer.  dw_ohwi is [rows][taps][CinP] with rows = Cout, CinP = rup(Cin, 4) (conv) or rows = Cin, CinP = rup(Cout, 4)
    (conv-transpose); its padding channels hold `sentinel`, w_fwd's hold zero (as prep leaves them)."""
    gen = torch.Generator().manual_seed(cout * 6007 + cin * 89 + taps + (3000 if exact else 0) + (77 if transposed_src else 0))
    rows, width = (cin, cout) if transposed_src else (cout, cin)
    CinP = rup(width, 4)
    draw = (lambda *s: exact_values(gen, *s)) if exact else (lambda *s: torch.randn(*s, generator=gen))
    dw = torch.full((rows, taps, CinP), sentinel)
    dw[:, :, :width] = draw(rows, taps, width)
    w = torch.zeros(rows, taps, CinP)
    w[:, :, :width] = draw(rows, taps, width) * (1.0 if exact else 1 / math.sqrt(cin * taps))
    u, v = draw(cout), draw(cin * taps)
    before = torch.randn(cout * cin * taps, generator=gen)
    sigma = torch.tensor(1.75 if exact else 0.8314)
    return dict(dw_ohwi=dw, w_fwd=w, u=u, v=v, sigma=sigma, before=before, CinP=CinP)


def bwd_gather(dw_ohwi, cout, cin, taps, transposed_src):
    """dw_ohwi -> G in the torch source layout ([Cout][Cin][taps], or [Cin][Cout][taps] with transposed_src), the padding dropped."""
    if transposed_src:
        return dw_ohwi[:cin, :, :cout].permute(0, 2, 1)
    return dw_ohwi[:cout, :, :cin].permute(0, 2, 1)


def bwd_g_formula(G, dot, u, v, sigma):
    return (G - dot * u * v) / sigma


def _uv_views(u, v, cout, cin, taps, transposed_src):
    return (u.view(1, cout, 1), v.view(cin, 1, taps)) if transposed_src else (u.view(cout, 1, 1), v.view(1, cin, taps))


def weight_prep_backward_ref(dw_ohwi, w_fwd, u, v, sigma, cout, cin, taps, CinP, sn, transposed_src, dw_orig_before, accumulate, dot=None):
    """-> (dot, dw_orig flat in the torch source layout), double.  dot = <dW, W_sn> over the real extent (None without spectral norm); `dot`: take this
    value (the kernel's stored one) instead, to separate the element-wise arithmetic from the reduction.  w_fwd is indexed like dw_ohwi (for
    transposed_src, where the device path has no spectral norm, that is [Cin][taps][CoutP])."""
    dw, w = dw_ohwi.double(), w_fwd.double()
    assert dw.shape[-1] == CinP and w.shape == dw.shape
    G = bwd_gather(dw, cout, cin, taps, transposed_src)
    d = None
    if sn:
        d = (G * bwd_gather(w, cout, cin, taps, transposed_src)).sum() if dot is None else torch.as_tensor(dot, dtype=torch.float64)
        G = bwd_g_formula(G, d, *_uv_views(u.double(), v.double(), cout, cin, taps, transposed_src), sigma.double())
    g = G.reshape(-1)
    return d, (dw_orig_before.double() + g if accumulate else g)


def bwd_bounds(I, cout, cin, taps, sn, accumulate, exact=False):
    """One conv layer (not transposed) of bwd_inputs -> (dot ref, dw_orig ref, dot bound, dw_orig bound).  Without spectral norm the output is a copy or one
    fp32 add of stored values: bound 0 against fp32(ref).  With it: the dot bound over the n = Cout taps CinP products the kernel sums (0 on the
    exact-arithmetic inputs, whose precondition is asserted), and the element-wise rule with the floor of an fp32 evaluation that is handed the
    fp32-rounded reference dot, plus the dot's bound carried through |u v| / sigma."""
    ref_dot, ref = weight_prep_backward_ref(I['dw_ohwi'], I['w_fwd'], I['u'], I['v'], I['sigma'], cout, cin, taps, I['CinP'], sn, False, I['before'], accumulate)
    if not sn:
        return None, ref, None, torch.zeros_like(ref)
    terms = (I['dw_ohwi'][:, :, :cin].double() * I['w_fwd'][:, :, :cin].double()).abs().sum()
    if exact:
        assert exact_ok(terms, 64), 'test inputs: the dot is not exact in fp32'
        bdot = torch.zeros((), dtype=torch.float64)
    else:
        bdot = dot_bound(terms, cout * taps * I['CinP'])
    G = bwd_gather(I['dw_ohwi'], cout, cin, taps, False)
    e32 = bwd_g_formula(G, ref_dot.float(), *_uv_views(I['u'], I['v'], cout, cin, taps, False), I['sigma']).reshape(-1)
    if accumulate:
        e32 = I['before'] + e32
    floor = (e32.double() - ref).abs().max().item()
    uv = (I['u'].double().view(cout, 1, 1) * I['v'].double().view(1, cin, taps)).abs().reshape(-1)
    return ref_dot, ref, bdot, tol_elem(ref, floor) + bdot * uv / float(I['sigma'])


# ---------------------------------------------------------------------------------------------------------------- Adam
def adam_hyper32():
    return {k: f32(x) for k, x in ADAM_HYPER.items()}


def adam_inputs(n, step, seed=0):
    """p, g, m, v (fp32) of one tensor before the update that the kernel sees as `step`.  Weights of an N(0, 0.02) initialisation; gradients and moments in
    three magnitude classes (1e-2, 1e-4, 1e-6 by index) with v ~ (magnitude)^2 (1 - beta2^step), so that sqrt(v / bc2) runs from 1e-2 down to
    the size of eps and every term of the denominator matters somewhere."""
    gen = torch.Generator().manual_seed(n * 31 + step + 1000 * seed)
    s = torch.tensor([1e-2, 1e-4, 1e-6])[torch.arange(n) % 3]
    bc2 = 1 - f32(ADAM_HYPER['beta2']) ** step
    p = torch.randn(n, generator=gen) * 0.02
    g = torch.randn(n, generator=gen) * s
    m = torch.randn(n, generator=gen) * s
    v = (torch.rand(n, generator=gen) * s) ** 2 * bc2
    return p, g, m, v


def adam_formula(p, g, m, v, bc1, bc2, lr, beta1, beta2, eps):
    """One Adam update in the dtype of the arguments, the kernel's (torch.optim.Adam's) expression order -> (p', m', v', update)."""
    m = m + (g - m) * (1 - beta1)
    v = v * beta2 + (1 - beta2) * g * g
    upd = (lr / bc1) * (m / (torch.sqrt(v) / torch.sqrt(bc2) + eps))
    return p - upd, m, v, upd


def adam_ref(p, g, m, v, step, lr32, beta1_32, beta2_32, eps32):
    """torch.optim.Adam (no weight decay, no amsgrad) in double on the fp32-ROUNDED hyper-parameters the kernel receives -> (p', m', v', update)."""
    d = lambda x: torch.as_tensor(x, dtype=torch.float64)
    bc1, bc2 = 1 - d(beta1_32) ** step, 1 - d(beta2_32) ** step
    return adam_formula(p.double(), g.double(), m.double(), v.double(), bc1, bc2, d(lr32), d(beta1_32), d(beta2_32), d(eps32))


def adam_bc_term(upd, step, beta1_32, beta2_32):
    """A-priori share of the device powf in p': relative P_POWF u beta^step / bc of bc1 (step_size = lr / bc1) and half that of bc2 (its root)."""
    b1, b2 = float(beta1_32) ** step, float(beta2_32) ** step
    return upd.abs() * P_POWF * U * (b1 / (1 - b1) + 0.5 * b2 / (1 - b2))


def adam_bounds(p, g, m, v, step, h):
    """-> (ref (p', m', v', upd), bounds (p', m', v')): the element-wise rule with the floor of a plain fp32 evaluation (bc1, bc2 handed over as the fp32
    roundings of their double values), taken per magnitude class of adam_inputs, + adam_bc_term on p'."""
    ref = adam_ref(p, g, m, v, step, h['lr'], h['beta1'], h['beta2'], h['eps'])
    t = lambda x: torch.tensor(x, dtype=torch.float32)
    bc1 = (1 - torch.tensor(h['beta1'], dtype=torch.float64) ** step).float()
    bc2 = (1 - torch.tensor(h['beta2'], dtype=torch.float64) ** step).float()
    e32 = adam_formula(p, g, m, v, bc1, bc2, t(h['lr']), t(h['beta1']), t(h['beta2']), t(h['eps']))
    cls = torch.arange(p.numel()) % 3      # adam_inputs' magnitude classes: a floor per class (one global floor would be vacuous for the small ones)
    tols = []
    for e, r in zip(e32[:3], ref[:3]):
        d = (e.double() - r).abs()
        floor = torch.stack([d[cls == c].max() if bool((cls == c).any()) else d.new_zeros(()) for c in range(3)])[cls]
        tols.append(tol_elem(r, floor))
    return ref, (tols[0] + adam_bc_term(ref[3], step, h['beta1'], h['beta2']), tols[1], tols[2])


# ---------------------------------------------------------------------------------------------------------------- overflow guard
def unscale_check_ref(g, mul):
    """-> (g * mul in double, overflow flag).  The flag is any(!(|g| <= 3.0e38)) on the values BEFORE the scaling: stricter than "not finite"."""
    g = g.double()
    return g * mul, bool((~(g.abs() <= FINITE_MAX)).any())
