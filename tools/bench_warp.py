"""Deformable resampling of the project's usual crop, 256 x 256 x 64 int16 at 0.7 x 0.7 x 1.5 mm with its uint8 label, resident in HBM: device
time (events around back-to-back launches, median of 10) of
  map_coordinates  orders 0 / 1 / 3 (order 3 on coefficients made once) with float64 and float32 [3, ...] coordinates, against a device copy
                   of what the kernel must read and write (the coordinate planes and the output) and scipy on the host with its transfers;
  warp_grid        the same orders through a 20 mm control grid, gorder 1 and 3, against hv_resample at the same order on the identity lattice
                   (the cost of the deformation itself) and a device copy of the output;
  elastic_pair     wall time of the CT at order 1 and the label at order 0 through one grid, synchronised.
One run on one box."""
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
from hvgan import warp as WP

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
ct_h = (rs.randn(*SHAPE) * 300.0).astype(np.int16)
lab_h = (rs.random_sample(SHAPE) * 4).astype(np.uint8)
ct, lab = torch.from_numpy(ct_h).to(dev), torch.from_numpy(lab_h).to(dev)
coef = RS.spline_filter(ct)
out = torch.empty(SHAPE, dtype=torch.int16, device=dev)
out2 = torch.empty_like(out)
t_out = median_us(lambda: out.copy_(out2))

grids = {g: WP.random_control_grid(SHAPE, SP, 20.0, 4.0, 1, gorder=g, device=dev) for g in (1, 3)}
print('control grid %s for %s' % (tuple(grids[3].values.shape), SHAPE), flush=True)
dense = WP.displacement_of(grids[3])
o = torch.stack(torch.meshgrid(*[torch.arange(n, dtype=torch.float64, device=dev) for n in SHAPE], indexing='ij'))
for cname, cdt in (('float64', torch.float64), ('float32', torch.float32)):
    u = (o + dense).to(cdt)
    u2 = torch.empty_like(u)
    t_copy = median_us(lambda: (u2.copy_(u), out.copy_(out2)))
    for order in (0, 1, 3):
        src = coef if order == 3 else ct
        fn = lambda: WP.map_coordinates(src, u, output=out, order=order, cval=-1024, prefilter=False)
        t = median_us(fn)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        want = torch.from_numpy(ndimage.map_coordinates(ct_h, u.cpu().numpy(), order=order, mode='constant', cval=-1024)).to(dev)
        torch.cuda.synchronize()
        host_ms = (time.perf_counter() - t0) * 1e3
        fn()
        diff = (out.double() - want.double()).abs()
        print('map_coordinates %s coordinates, order %d%s: %.0f us = %.1f x the device copy of coordinates + output (%.1f us); scipy on the '
              'host with its transfers %.0f ms = %.0f x (voxels that differ: %d, by at most %g)'
              % (cname, order, ' (sample only, resident coefficients)' if order == 3 else '', t, t / t_copy, t_copy, host_ms,
                 host_ms * 1e3 / t, int((diff != 0).sum()), float(diff.max())), flush=True)
    del u, u2
for order in (0, 1, 3):
    src = coef if order == 3 else ct
    t_rs = median_us(lambda: RS.affine_transform(src, np.ones(3), output=out, order=order, cval=-1024, prefilter=False))
    for g in (1, 3):
        t = median_us(lambda: WP.warp_grid(src, grids[g], output=out, order=order, cval=-1024, prefilter=False))
        print('warp_grid order %d, gorder %d: %.0f us = %.2f x hv_resample on the identity lattice (%.0f us) = %.1f x the device copy of the '
              'output (%.1f us)' % (order, g, t, t / t_rs, t_rs, t / t_out, t_out), flush=True)
for _ in range(3):
    WP.elastic_pair(ct, lab, grids[3])
torch.cuda.synchronize()
ts = []
for _ in range(10):
    t0 = time.perf_counter()
    WP.elastic_pair(ct, lab, grids[3])
    torch.cuda.synchronize()
    ts.append((time.perf_counter() - t0) * 1e3)
print('elastic_pair (int16 CT order 1 + uint8 label order 0, gorder 3): wall %.3f ms (median of 10, synchronised)' % statistics.median(ts), flush=True)
