"""Resampling of one 256 x 256 x 64 crop at spacing 0.7 x 0.7 x 1.5 mm, resident in HBM, to 1 mm isotropic (179 x 179 x 96), as int16 and as
float64: device time (events around back-to-back launches, median of 10) of resample_to_spacing at orders 0, 1 and 3 -- order 3 with its
prefilter and, on coefficients made once, without -- and of a full-matrix rigid transform of the same crop; a plain device copy of the OUTPUT
volume as the yardstick; wall time of scipy.ndimage on the host with its two transfers, and whether the two results have the same bytes (else
the largest difference).  Then a 512 x 512 x 400 int16 scan at the same spacing to 1 mm (358 x 358 x 600): orders 0 and 1 against scipy,
order 3 on the device alone (scipy needs the better part of a minute there)."""
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

SP, NEW = (0.7, 0.7, 1.5), (1.0, 1.0, 1.0)
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


def report(name, what, fn, ref, d, out, t_copy, inner=5):
    t = median_us(fn, inner=inner)
    line = '%s %s: %.0f us = %.1f x the device copy of the output (%.1f us)' % (name, what, t, t / t_copy, t_copy)
    if ref is not None:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        want = torch.from_numpy(ref(d.cpu().numpy())).to(dev)
        torch.cuda.synchronize()
        host_ms = (time.perf_counter() - t0) * 1e3
        fn()
        same = bool(torch.equal(out, want))
        line += '; scipy on the host with its two transfers %.0f ms = %.0f x (same bytes: %s' % (host_ms, host_ms * 1e3 / t, same)
        if not same:
            diff = (out.double() - want.double()).abs()
            line += ', %d voxels differ, by at most %.3g' % (int((diff != 0).sum()), float(diff.max()))
        line += ')'
    print(line, flush=True)


def rigid(shape):
    a, b = np.deg2rad(7.0), np.deg2rad(-4.0)
    rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    c = (np.array(shape) - 1) / 2.0
    return RS.rigid_matrix(rz @ ry, c, c)


print('device: %s' % torch.cuda.get_device_name(0), flush=True)
rs = np.random.RandomState(0)
ct64 = rs.randn(256, 256, 64) * 300.0
plan = RS.spacing_plan(ct64.shape, SP, NEW)
zm = tuple(o / a for o, a in zip(plan['new_shape'], plan['shape']))
assert RS.zoom_arguments(plan['shape'], zm)[0] == plan['new_shape']
M, OFF = rigid(ct64.shape)
for name, host in (('int16', ct64.astype(np.int16)), ('float64', ct64)):
    d = torch.from_numpy(host).to(dev)
    out = torch.empty(plan['new_shape'], dtype=d.dtype, device=dev)
    src = torch.empty_like(out)
    t_copy = median_us(lambda: out.copy_(src))
    for order in (0, 1, 3):
        report(name, 'to 1 mm, order %d%s' % (order, ' (prefilter + sample)' if order == 3 else ''),
               lambda: RS.resample_to_spacing(d, SP, NEW, order=order, output=out), lambda a: ndimage.zoom(a, zm, order=order, mode='constant'),
               d, out, t_copy)
    coef = RS.spline_filter(d)
    report(name, 'to 1 mm, order 3 on resident coefficients (sample only)',
           lambda: RS.zoom(coef, zm, order=3, output=out, prefilter=False), None, d, out, t_copy)
    rout, rsrc = torch.empty_like(d), torch.empty_like(d)
    t_copy_r = median_us(lambda: rout.copy_(rsrc))
    for order in (1, 3):
        report(name, 'rigid transform (full matrix), order %d' % order, lambda: RS.affine_transform(d, M, OFF, output=rout, order=order),
               lambda a: ndimage.affine_transform(a, M, OFF, order=order, mode='constant'), d, rout, t_copy_r)
    del coef

scan = (rs.randn(512, 512, 400) * 300.0).astype(np.int16)
plan = RS.spacing_plan(scan.shape, SP, NEW)
zm = tuple(o / a for o, a in zip(plan['new_shape'], plan['shape']))
assert RS.zoom_arguments(plan['shape'], zm)[0] == plan['new_shape']
d = torch.from_numpy(scan).to(dev)
out = torch.empty(plan['new_shape'], dtype=d.dtype, device=dev)
src = torch.empty_like(out)
t_copy = median_us(lambda: out.copy_(src), inner=2)
name = 'int16 scan 512x512x400 -> %dx%dx%d' % plan['new_shape']
for order in (0, 1):
    report(name, 'order %d' % order, lambda: RS.resample_to_spacing(d, SP, NEW, order=order, output=out),
           lambda a: ndimage.zoom(a, zm, order=order, mode='constant'), d, out, t_copy, inner=2)
report(name, 'order 3 (prefilter + sample)', lambda: RS.resample_to_spacing(d, SP, NEW, order=3, output=out), None, d, out, t_copy, inner=2)
