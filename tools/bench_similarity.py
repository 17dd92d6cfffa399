"""Joint histograms of the project's usual crop, 256 x 256 x 64 int16, against itself moved a little, both resident in HBM: device time (events
around back-to-back launches, median of 10) of hv_joint_hist at K = 1 / 13 / 16 poses, orders 0 / 1 / 3 (order 3 on coefficients made once)
and G = 32 / 64 levels, each against three things measured in the same run:
  copy        a device copy of the two volumes (what the kernel must read once);
  two-launch  K x (hv_resample at the same order into an int16 volume + hv_glcm with the single offset (0, 0, 0) on the result): the route
              this replaces, one resampled volume formed and binned per pose (it gives the moving marginal only, so it is a floor);
  host        K x (the volumes fetched, scipy.ndimage.affine_transform and np.histogram2d), timed for one pose.
And the wall time of one register_rigid, synchronised.  One run on one box."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from scipy import ndimage
import hvgan  # noqa: F401
from hvgan import resample as RS
from hvgan import similarity as SM
from hvgan import texture as TX

SHAPE, SP = (256, 256, 64), (0.7, 0.7, 1.5)
dev = torch.device('cuda:0')


def median_us(fn, reps=10, inner=5):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / inner * 1e3)
    return statistics.median(ts)


print('device: %s' % torch.cuda.get_device_name(0), flush=True)
rs = np.random.RandomState(0)
g = np.meshgrid(*[np.linspace(-1.0, 1.0, n) for n in SHAPE], indexing='ij')
ct_h = (700.0 * np.exp(-(g[0] ** 2 + g[1] ** 2 + g[2] ** 2) * 3.0) - 300.0 + rs.randn(*SHAPE) * 40.0).astype(np.int16)
fixed = torch.from_numpy(ct_h).to(dev)
true = SM.rigid_pose((2.0, -1.5, 1.0, 2.0, -1.0, 1.5), SHAPE, SHAPE, SP, SP)
moving = RS.affine_transform(fixed, true[0], true[1], order=1, cval=-1024)
coef = RS.spline_filter(moving)
label = torch.ones(SHAPE, dtype=torch.uint8, device=dev)
out16 = torch.empty(SHAPE, dtype=torch.int16, device=dev)
a2, b2 = torch.empty_like(fixed), torch.empty_like(moving)
t_copy = median_us(lambda: (a2.copy_(fixed), b2.copy_(moving)))
print('device copy of the two volumes: %.1f us' % t_copy, flush=True)


def poses_of(K):
    step = np.array([1.0, 1.0, 1.0, 1.0, 1.0, 1.0])
    return SM._check_poses([SM.rigid_pose(q, SHAPE, SHAPE, SP, SP) for q in (SM._neighbours(np.zeros(6), step) * 2)[:K]])


t_host = {}
for order in (0, 1, 3):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fh, mh = fixed.cpu().numpy(), moving.cpu().numpy()
    y = ndimage.affine_transform(mh, true[0], true[1], order=order, output=np.float64, mode='constant', cval=np.nan)
    ok = np.isfinite(y)
    np.histogram2d(fh[ok], y[ok], bins=32, range=((-200.0, 600.0), (-200.0, 600.0)))
    t_host[order] = (time.perf_counter() - t0) * 1e3

for order in (0, 1, 3):
    src = coef if order == 3 else moving
    for G in (32, 64):
        width = 800.0 / G
        gb = TX._buffers(1, 1, 1, G, dev)
        t_two = median_us(lambda: (RS.affine_transform(src, true[0], true[1], output=out16, order=order, cval=-1024, prefilter=False),
                                   TX._launch(out16[None], label[None], None, [1], np.zeros((1, 3), dtype=np.int64), G, -200.0, width, False,
                                              gb[1], gb[2])))
        for K in (1, 13, 16):
            p = poses_of(K)
            buf = torch.empty((K * (G * G + SM.INFO),), dtype=torch.int64, device=dev)
            o, i = buf[:K * G * G].view(K, G, G), buf[K * G * G:].view(K, SM.INFO)
            t = median_us(lambda: SM._launch(fixed, src, None, p, order, -200.0, width, G, -200.0, width, G, o, i))
            print('joint_hist order %d, G %d, K %2d: %.0f us = %.1f x the copy = %.1f x the copy per pose; two-launch route %d x %.0f us = %.0f us '
                  '(%.2f x ours); host chain %d x %.0f ms (%.0f x ours)'
                  % (order, G, K, t, t / t_copy, t / t_copy / K, K, t_two, K * t_two, K * t_two / t, K, t_host[order],
                     K * t_host[order] * 1e3 / t), flush=True)

kw = dict(spacing_fixed=SP, spacing_moving=SP, steps_deg=(2.0, 1.0, 0.5), steps_mm=(2.0, 1.0, 0.5))
reg = SM.register_rigid(fixed, moving, **kw)
torch.cuda.synchronize()
ts = []
for _ in range(3):
    t0 = time.perf_counter()
    reg = SM.register_rigid(fixed, moving, **kw)
    torch.cuda.synchronize()
    ts.append((time.perf_counter() - t0) * 1e3)
print('register_rigid (order 1, 32 levels, nmi): wall %.1f ms (median of 3, synchronised), %d calls of 13 poses, params %s, score %.4f -> %.4f'
      % (statistics.median(ts), reg.calls, np.round(reg.params, 2).tolist(), reg.history[0][2], reg.score), flush=True)
