"""Plain numpy references of the five in-training evaluation metrics of ONE sample (hv_eval_metrics, csrc/eval_metrics.hip; reference train.py:37-48,
:101-141), in two forms:

  metrics_f32   the float32 form oracle/restate.py states (eval_ssim / eval_psnr on scipy's uniform_filter, eval_dice_score / eval_iou_score on float32
                torch sums) -- imported, not copied; this is what the device is held to
  metrics_f64   the same definitions in float64, SSIM as direct 7x7 window sums over the cropped region (no uniform_filter): it shares no code with the
                float32 form and says how far float32 rounding moves each metric on a given input

Both take the operands the C entry takes: inp (the composited image), gt, mask, the four binary maps, pred_h (float32) and height (int).  The images the
metrics see are the float32 products gt * mask and inp * mask (that is the data skimage is handed); everything after that is float64 in metrics_f64.

edge_inputs / batch_case build the seeded inputs of tests/test_eval_edges_gpu.py: images in [-1, 1] with texture in every window (uniform noise, variance
~1/3, so no window's variance cancels to nothing in float32) -- tests/test_eval_ref_cpu.py checks that on each of them the float32 form lies within a
quarter of the device tolerance of the float64 form."""
import numpy as np
import torch

from oracle.restate import eval_dice_score, eval_iou_score, eval_psnr, eval_ssim

TOL = (1e-5, 1e-4, 1e-6, 1e-6, 1e-4)       # ssim, psnr, dice, iou, diff_h: the device tolerances of tests/test_eval_gpu.py
# (B, H, W): one SSIM pixel; SSIM region one pixel wide; ragged width; a second row tile of one row; HW no multiple of 1024 with a ragged last tile;
# the second workgroup of the final kernel
SHAPES = ((1, 7, 7), (1, 14, 7), (2, 8, 23), (3, 15, 14), (2, 40, 70), (65, 9, 9))


def metrics_f32(inp, gt, mask, cb, nv, fb, lab, pred_h, height):
    inp, gt, mask = (np.asarray(v, dtype=np.float32) for v in (inp, gt, mask))
    a, b = gt * mask, inp * mask
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))
    with np.errstate(divide='ignore'):
        psnr = eval_psnr(a, b, inp.max() - gt.min())
    h = np.float32(height)
    dh = np.abs(np.float32(pred_h) - h) / h * np.float32(100)
    return np.array([eval_ssim(a, b, inp.max() - inp.min()), psnr, float(eval_dice_score(t(cb), t(nv))), float(eval_iou_score(t(fb), t(lab))), float(dh)])


def _window_sums(x):
    """sums over every 7x7 window that lies inside the image: [H - 6][W - 6], entry (i, j) = the window centred on pixel (i + 3, j + 3)"""
    H, W = x.shape
    out = np.zeros((H - 6, W - 6))
    for di in range(7):
        for dj in range(7):
            out += x[di:di + H - 6, dj:dj + W - 6]
    return out


def ssim_f64(a, b, data_range):
    a, b, R = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), float(data_range)
    ux, uy = _window_sums(a) / 49.0, _window_sums(b) / 49.0
    uxx, uyy, uxy = _window_sums(a * a) / 49.0, _window_sums(b * b) / 49.0, _window_sums(a * b) / 49.0
    n = 49.0 / 48.0
    vx, vy, vxy = n * (uxx - ux * ux), n * (uyy - uy * uy), n * (uxy - ux * uy)
    C1, C2 = (0.01 * R) ** 2, (0.03 * R) ** 2
    return float((((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))).mean())


def metrics_f64(inp, gt, mask, cb, nv, fb, lab, pred_h, height):
    inp32, gt32, m32 = (np.asarray(v, dtype=np.float32) for v in (inp, gt, mask))
    a, b = (gt32 * m32).astype(np.float64), (inp32 * m32).astype(np.float64)
    mx, mn, mg = float(inp32.max()), float(inp32.min()), float(gt32.min())
    err = ((a - b) ** 2).mean()
    psnr = float('inf') if err == 0 else 10.0 * np.log10((mx - mg) ** 2 / err)
    cb, nv, fb, lab = (np.asarray(v, dtype=np.float64) for v in (cb, nv, fb, lab))
    s = 1e-5
    dice = (2.0 * (cb * nv).sum() + s) / (cb.sum() + nv.sum() + s)
    inter = (fb * lab).sum()
    iou = (inter + s) / (fb.sum() + lab.sum() - inter + s)
    dh = abs(float(np.float32(pred_h)) - float(height)) / float(height) * 100.0
    return np.array([ssim_f64(a, b, mx - mn), psnr, dice, iou, dh])


def edge_inputs(B, H, W, seed=0):
    """Seeded operands of hv_eval_metrics for B samples, float32 [B][H][W] (pred_h float32 [B], height int64 [B]).  inp: uniform noise in [-1, 1]; gt:
    0.3 inp + 0.7 noise of its own; mask: the rows of a band (every row for H < 10); the binary maps: independent coin flips.
    The weak correlation is on purpose.  Per window SSIM's second factor is (n a + C2) / (n b + C2), a = 2 cov, b = var + var, n the covariance
    normalisation: its derivative in n is C2 (a - b) / (n b + C2)^2, which vanishes for near-identical images.  Here a ~ 0.2, b ~ 0.53, C2 = 0.0036: a
    normalisation of 1 in place of 49/48 moves the mean SSIM by ~9e-5, nine device tolerances."""
    rng = np.random.RandomState(1000 * H + 10 * W + B + seed)
    inp = rng.uniform(-1, 1, (B, H, W)).astype(np.float32)
    gt = (0.3 * inp + 0.7 * rng.uniform(-1, 1, (B, H, W))).astype(np.float32)
    mask = np.ones((B, H, W), dtype=np.float32)
    if H >= 10:
        mask[:, :H // 5] = 0
        mask[:, H - H // 8:] = 0
    maps = [(rng.rand(B, H, W) < p).astype(np.float32) for p in (0.5, 0.4, 0.3, 0.6)]
    height = rng.randint(8, 40, B).astype(np.int64)
    pred_h = (height * rng.uniform(0.6, 1.5, B)).astype(np.float32)
    return dict(inp=inp, gt=gt, mask=mask, cb=maps[0], nv=maps[1], fb=maps[2], lab=maps[3], pred_h=pred_h, height=height)


def sample(d, i):
    """operands of sample i, in the argument order of metrics_f32 / metrics_f64"""
    return tuple(d[k][i] for k in ('inp', 'gt', 'mask', 'cb', 'nv', 'fb', 'lab', 'pred_h', 'height'))


def batch_case(B=2, H=40, W=70, seed=5):
    """Generator outputs and batch attributes for eval_metrics.batch_metrics ((B,1,H,W) float32 torch tensors): the predicted height stays below the
    vertebra's, so the composited image is stage2 on the rows [x1, x2) and real_B elsewhere (oracle.restate.shrm_composite states that for any rows)."""
    rng = np.random.RandomState(seed)
    img = lambda: torch.from_numpy(rng.uniform(-1, 1, (B, 1, H, W)).astype(np.float32))
    real_B = img()
    stage2 = 0.3 * real_B + 0.7 * img()
    x1 = torch.tensor([H // 4 + i for i in range(B)], dtype=torch.int64)
    height = torch.tensor([H // 3 + 2 * i for i in range(B)], dtype=torch.int64)
    mask = torch.zeros(B, 1, H, W)
    for i in range(B):
        mask[i, :, int(x1[i]) - 2:int(x1[i] + height[i]) + 3] = 1
    seg = lambda: torch.from_numpy(rng.rand(B, 1, H, W).astype(np.float32))
    binm = lambda p: torch.from_numpy((rng.rand(B, 1, H, W) < p).astype(np.float32))
    outs = dict(stage2=stage2, fine_seg=seg(), coarse_seg=seg(), pred2=torch.tensor([[0.21 + 0.02 * i] for i in range(B)], dtype=torch.float32))
    batch = dict(real_B=real_B, real_B_mask=binm(0.4), normal_vert=binm(0.5), mask=mask, height=height, x1=x1, x2=x1 + height,
                 maxheight=torch.full((B,), H, dtype=torch.int64))
    assert all(float(outs['pred2'][i, 0]) * H < int(height[i]) for i in range(B))
    return outs, batch
