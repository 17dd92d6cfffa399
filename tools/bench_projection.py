"""Parallel-beam projections (hv_project) of a resident volume: the 256 x 256 x 64 int16 crop and a 512 x 512 x 400 int16 scan, lateral, AP and
one oblique view at orders 0 / 1, one pose and three poses per call.  Device time from events around back-to-back launches, median of 10,
resident inputs and outputs.  Beside each: a plain device copy of the volume as the memory-rate yardstick, and the two-step route this
operator replaces -- hv_resample onto the (P0, P1, T) float64 lattice plus torch.sum over t -- where that lattice fits (it is dropped, and
said so, where P0 * P1 * T * 8 bytes exceed LATTICE_LIMIT).  The named views use the volume's own pitches and extents (every voxel sampled
once); the oblique view covers the bounding sphere at a pitch of one voxel."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import hvgan  # noqa: F401
from hvgan import projection as P
from hvgan import resample as RS

dev = torch.device('cuda:0')
LATTICE_LIMIT = 4 << 30                      # bytes of float64 lattice the two-step route may allocate
OBLIQUE = (10.0, 25.0, 5.0)


def median_us(fn, reps=10, inner=3):
    for _ in range(2):
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


def volume(shape):
    """A smooth body with seeded noise, int16, like a windowed CT."""
    g = torch.Generator(device='cpu').manual_seed(3)
    z = torch.linspace(-1, 1, shape[0])[:, None, None] ** 2 + torch.linspace(-1, 1, shape[1])[None, :, None] ** 2 + torch.linspace(-1, 1, shape[2])[None, None, :] ** 2
    v = 900.0 * torch.exp(-2.0 * z) - 200.0 + 30.0 * torch.randn(shape, generator=g)
    return v.to(torch.int16).to(dev)


def native_view(shape, view):
    a0, a1, ar = P.VIEWS[view]
    return P.view_pose(shape, (1, 1, 1), view, det_spacing=1.0, step_mm=1.0, det_shape=(shape[a0], shape[a1]), steps=shape[ar])


def run(name, vol):
    shape = tuple(vol.shape)
    c = torch.empty_like(vol)
    t_copy = median_us(lambda: c.copy_(vol))
    del c
    print('%s (%.1f MB): device copy of the volume %.0f us' % (name, vol.numel() * 2 / 1e6, t_copy), flush=True)
    for view in ('lateral', 'ap', OBLIQUE):
        vp = native_view(shape, view) if isinstance(view, str) else P.view_pose(shape, (1, 1, 1), view)
        for K in (1, 3):
            poses = P._check_poses([(vp.matrix, vp.offset + 0.25 * k) for k in range(K)])
            acc, idx, info, _ = P._buffers(K, vp.det_shape, dev)
            for order in (0, 1):
                t = median_us(lambda: P._launch(vol, None, 0.0, poses, vp.det_shape, vp.steps, order, acc, idx, info))
                counted = int(info[:, P.COUNTED].sum())
                line = '  %-22s K=%d order %d: detector %s x %d steps, %d samples counted: hv_project %.0f us = %.2f x the copy' % (
                    view, K, order, vp.det_shape, vp.steps, counted, t, t / t_copy)
                lattice = vp.det_shape[0] * vp.det_shape[1] * vp.steps * 8
                if K == 1 and lattice <= LATTICE_LIMIT:
                    out = torch.empty((vp.det_shape[0], vp.det_shape[1], vp.steps), dtype=torch.float64, device=dev)
                    t2 = median_us(lambda: RS.affine_transform(vol, vp.matrix, vp.offset, out.shape, out, order, 'constant', 0.0).sum(dim=2))
                    two = RS.affine_transform(vol, vp.matrix, vp.offset, out.shape, out, order, 'constant', 0.0).sum(dim=2)
                    diff = float((two - acc[0, P.SUM]).abs().max())
                    line += '; two-step (hv_resample to a %.0f MB float64 lattice + torch.sum) %.0f us = %.2f x hv_project, max |difference| %.3g' % (
                        lattice / 1e6, t2, t2 / t, diff)
                    del out, two
                elif K == 1:
                    line += '; two-step route dropped: its float64 lattice would take %.1f GB' % (lattice / 1e9)
                print(line, flush=True)


run('256x256x64 int16 crop', volume((256, 256, 64)))
run('512x512x400 int16 scan', volume((512, 512, 400)))
