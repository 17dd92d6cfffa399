"""Separable Gaussian filtering of one 256 x 256 x 64 crop at spacing 0.7 x 0.7 x 1.5 mm, resident in HBM: device time (events around
back-to-back launches, median of 10) of gaussian_filter at sigma = 1 mm on a float64 and on an int16 volume -- all three axes, and each axis
alone --, of smooth_label at 1 mm on the uint8 label, and of clean_label with and without smooth_mm; a plain device copy of the same bytes as
the yardstick; wall time of scipy.ndimage.gaussian_filter on the host with its two transfers."""
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
from hvgan import components as C
from hvgan import filters as F

H, W, Z, LABEL = 256, 256, 64, 20
SP, SIGMA = (0.7, 0.7, 1.5), 1.0
dev = torch.device('cuda:0')
g = np.meshgrid(np.arange(H) - 128.0, np.arange(W) - 128.0, np.arange(Z) - 31.5, indexing='ij')


def label_crop(seed):
    v = np.zeros((H, W, Z), dtype=np.uint8)
    for k in range(Z):                                        # a vertebra-sized blob whose outline jumps from slice to slice
        o = (0, 2, -1, 1)[k % 4]
        v[..., k][((g[0][..., k] - o) / 40) ** 2 + (g[1][..., k] / 60) ** 2 + (g[2][..., k] / 27.6) ** 2 <= 1] = LABEL
    v[(g[0] + 90) ** 2 / 20 ** 2 + (g[1] / 60) ** 2 <= 1] = LABEL - 1
    r = np.random.RandomState(seed)
    v[r.randint(0, H, 300), r.randint(0, W, 300), r.randint(0, Z, 300)] = LABEL
    return v


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
ct64 = rs.randn(H, W, Z) * 300.0
out = torch.empty(H, W, Z, dtype=torch.float64, device=dev)
sig = tuple(SIGMA / s for s in SP)
for name, host in (('float64', ct64), ('int16', ct64.astype(np.int16))):
    d = torch.from_numpy(host).to(dev)
    t_all = median_us(lambda: F.gaussian_filter(d, SIGMA, spacing=SP, out=out))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    want = torch.from_numpy(ndimage.gaussian_filter(d.cpu().numpy().astype(np.float64), sig)).to(dev)
    torch.cuda.synchronize()
    host_ms = (time.perf_counter() - t0) * 1e3
    same = bool(torch.equal(out, want))
    per_axis = []
    for a in range(3):
        s = [0.0, 0.0, 0.0]
        s[a] = SIGMA
        per_axis.append(median_us(lambda: F.gaussian_filter(d, s, spacing=SP, out=out)))
    copy_in = torch.empty_like(d)
    t_copy_in, t_copy64 = median_us(lambda: copy_in.copy_(d)), median_us(lambda: out.copy_(want))
    print('gaussian_filter %s, sigma %.1f mm at %s (radii %s): %.0f us for the three axes; one axis alone (read %s, write float64) %s us; '
          'device copy of the input %.1f us, of a float64 volume %.1f us; scipy on the host with its two transfers %.0f ms (same bits: %s)'
          % (name, SIGMA, SP, [int(4.0 * x + 0.5) for x in sig], t_all, name, ' / '.join('%.0f' % t for t in per_axis), t_copy_in, t_copy64,
             host_ms, same), flush=True)

lab = label_crop(0)
d = torch.from_numpy(lab).to(dev)
res = torch.empty_like(d)
mask = torch.empty(H, W, Z, dtype=torch.uint8, device=dev)
t_mask = median_us(lambda: F.smooth_mask(d, LABEL, SIGMA, SP, out=mask))
t_smooth = median_us(lambda: F.smooth_label(d, LABEL, SIGMA, SP, out=res))
torch.cuda.synchronize()
t0 = time.perf_counter()
m = ndimage.gaussian_filter((d.cpu().numpy() == LABEL).astype(np.float64), sig) >= 0.5
want = torch.from_numpy(m.view(np.uint8)).to(dev)
torch.cuda.synchronize()
host_ms = (time.perf_counter() - t0) * 1e3
t_copy = median_us(lambda: res.copy_(d))
print('smooth_label uint8, sigma %.1f mm: mask %.0f us, with the write-back %.0f us; device copy of the label %.1f us; scipy mask on the host '
      'with its two transfers %.0f ms (same mask: %s)' % (SIGMA, t_mask, t_smooth, t_copy, host_ms, bool(torch.equal(mask, want))), flush=True)
t_plain = median_us(lambda: C.clean_label(d, LABEL, out=res))
t_sm = median_us(lambda: C.clean_label(d, LABEL, out=res, smooth_mm=SIGMA, spacing=SP))
print('clean_label (keep the largest component): %.0f us; with smooth_mm=%.1f %.0f us' % (t_plain, SIGMA, t_sm), flush=True)
