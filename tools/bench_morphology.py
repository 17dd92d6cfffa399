"""3-D binary morphology of one 256 x 256 x 64 uint8 label crop -- a vertebra-sized blob plus a few hundred speckle voxels -- resident in HBM:
device time (events around back-to-back launches, median of 10) of hv_morph_ball (dilation and closing by a ball of 1, 2 and 5 mm, at unit
spacing and at 0.7 x 0.7 x 1.5 mm), of the same masks by the route that existed before -- hv_edt, then a torch comparison of its doubles --,
of hv_morph_struct (connectivity 1, 1 and 3 iterations) and of clean_label with and without closing_mm; wall time of the scipy call on the
host with its two transfers."""
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
from hvgan import generation_eval as GE
from hvgan import morphology as M

H, W, Z, LABEL = 256, 256, 64, 20
dev = torch.device('cuda:0')
g = np.meshgrid(np.arange(H) - 128.0, np.arange(W) - 128.0, np.arange(Z) - 31.5, indexing='ij')


def crop(seed):
    v = np.zeros((H, W, Z), dtype=np.uint8)
    v[(g[0] / 40) ** 2 + (g[1] / 60) ** 2 + (g[2] / 27.6) ** 2 <= 1] = LABEL
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


host = crop(0)
d = torch.from_numpy(host).to(dev)
mask = torch.empty(H, W, Z, dtype=torch.uint8, device=dev)
mid = torch.empty(H, W, Z, dtype=torch.uint8, device=dev)
dist = torch.empty(H, W, Z, dtype=torch.float64, device=dev)
via = torch.empty(H, W, Z, dtype=torch.bool, device=dev)


def edt_dilation(r, sp):
    GE.distance_transform(d, LABEL, sp, out=dist)
    torch.le(dist, r, out=via)


def edt_closing(r, sp):
    """The dilation, then the erosion as the voxels further than r from the dilation's complement (the volume's faces are not modelled)."""
    GE.distance_transform(d, LABEL, sp, out=dist)
    torch.le(dist, r, out=via)
    mid.copy_(via)
    GE.distance_transform(mid, 0, sp, out=dist)
    torch.gt(dist, r, out=via)


def host_call(fn, r, sp):
    v = d.cpu().numpy()                                                                   # download
    out = fn(v == LABEL, structure=M.ball(r, sp))
    return torch.from_numpy(out.view(np.uint8)).to(dev)                                   # upload


for sp in ((1.0, 1.0, 1.0), (0.7, 0.7, 1.5)):
    for r in (1.0, 2.0, 5.0):
        t_dil = median_us(lambda: M.binary_dilation(d, LABEL, radius=r, spacing=sp, out=mask))
        same_d = bool(torch.equal(mask.bool(), (edt_dilation(r, sp), via)[1]))
        t_clo = median_us(lambda: M.binary_closing(d, LABEL, radius=r, spacing=sp, out=mask))
        t_edt_dil = median_us(lambda: edt_dilation(r, sp))
        t_edt_clo = median_us(lambda: edt_closing(r, sp))
        host_ms = float('nan')
        same_h = None
        if r <= 2.0:                                                                      # scipy needs tens of seconds for the 5 mm ball
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            want = host_call(ndimage.binary_closing, r, sp)
            torch.cuda.synchronize()
            host_ms = (time.perf_counter() - t0) * 1e3
            same_h = bool(torch.equal(mask, want))
        print('ball r = %.0f mm, spacing %s (%d offsets): hv_morph_ball dilation %.0f us, closing %.0f us; hv_edt + torch comparison: dilation '
              '%.0f us (same mask: %s), closing %.0f us; scipy binary_closing on the host with its two transfers %.0f ms (same mask: %s)'
              % (r, sp, int(M.ball(r, sp).sum()), t_dil, t_clo, t_edt_dil, same_d, t_edt_clo, host_ms, same_h), flush=True)

for it in (1, 3):
    t_dil = median_us(lambda: M.binary_dilation(d, LABEL, connectivity=1, iterations=it, out=mask))
    t_clo = median_us(lambda: M.binary_closing(d, LABEL, connectivity=1, iterations=it, out=mask))
    print('connectivity 1, %d iteration(s): hv_morph_struct dilation %.0f us, closing %.0f us' % (it, t_dil, t_clo), flush=True)

out = torch.empty_like(d)
t_copy = median_us(lambda: out.copy_(d))
t_plain = median_us(lambda: C.clean_label(d, LABEL, out=out))
t_close = median_us(lambda: C.clean_label(d, LABEL, out=out, closing_mm=1.0, spacing=(0.7, 0.7, 1.5)))
t_both = median_us(lambda: C.clean_label(d, LABEL, out=out, closing_mm=1.0, opening_mm=0.7, spacing=(0.7, 0.7, 1.5)))
print('clean_label (keep the largest component): %.0f us; with closing_mm=1.0 at 0.7 x 0.7 x 1.5 mm %.0f us; with opening_mm=0.7 as well %.0f us; '
      'device copy of the same bytes %.1f us' % (t_plain, t_close, t_both, t_copy), flush=True)
