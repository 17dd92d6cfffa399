"""Rank filtering of one 256 x 256 x 64 crop at spacing 0.7 x 0.7 x 1.5 mm, resident in HBM, as int16 and as float64: device time (events around
back-to-back launches, median of 10) of the 3 x 3 x 3 median, median_ct over a 1.5 mm ball, deflicker along the slice axis, the separable
3 x 3 x 3 minimum_filter and the 3 x 3 x 3 grey_opening; a plain device copy of the same volume as the yardstick; wall time of scipy.ndimage on
the host with its two transfers, and whether the two results have the same bytes."""
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
from hvgan import rank_filters as RF

H, W, Z = 256, 256, 64
SP, RADIUS = (0.7, 0.7, 1.5), 1.5
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
ct64 = rs.randn(H, W, Z) * 300.0
ball = RF.ball(RADIUS, SP)
ball_fp = np.zeros(tuple(2 * np.abs(ball).max(axis=0) + 1), dtype=bool)
ball_fp[tuple((ball + np.abs(ball).max(axis=0)).T)] = True
for name, host in (('int16', ct64.astype(np.int16)), ('float64', ct64)):
    d = torch.from_numpy(host).to(dev)
    out = torch.empty_like(d)
    t_copy = median_us(lambda: out.copy_(d))
    cases = (
        ('median_filter 3x3x3 (27 taps)', lambda: RF.median_filter(d, size=3, out=out), lambda a: ndimage.median_filter(a, size=3)),
        ('median_ct %.1f mm ball (%d taps)' % (RADIUS, len(ball)), lambda: RF.median_ct(d, radius_mm=RADIUS, spacing=SP, out=out),
         lambda a: ndimage.median_filter(a, footprint=ball_fp, mode='nearest')),
        ('deflicker (3 taps along the slice axis)', lambda: RF.deflicker(d, out=out), lambda a: ndimage.median_filter(a, size=(1, 1, 3), mode='nearest')),
        ('minimum_filter 3x3x3 (separable, 3 launches)', lambda: RF.minimum_filter(d, size=3, out=out), lambda a: ndimage.minimum_filter(a, size=3)),
        ('grey_opening 3x3x3 (6 launches)', lambda: RF.grey_opening(d, size=3, out=out), lambda a: ndimage.grey_opening(a, size=3)),
    )
    for what, fn, ref in cases:
        t = median_us(fn)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        want = torch.from_numpy(ref(d.cpu().numpy())).to(dev)
        torch.cuda.synchronize()
        host_ms = (time.perf_counter() - t0) * 1e3
        fn()
        same = bool(torch.equal(out, want))
        print('%s %s: %.0f us = %.1f x the device copy of the volume (%.1f us); scipy on the host with its two transfers %.0f ms = %.0f x '
              '(same bytes: %s)' % (name, what, t, t / t_copy, t_copy, host_ms, host_ms * 1e3 / t, same), flush=True)
