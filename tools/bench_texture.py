"""Per-label grey-level co-occurrence matrices (hv_glcm) of a resident volume: one 256 x 256 x 64 crop with a vertebra-sized label, the 13
directions at distance 1, G = 32, symmetric; as int16 and as float64, once on smooth-plus-noise intensities and once on a constant (every pair in
one bin: the contention worst case).  Device time from events around back-to-back launches, median of 10; beside it a plain device copy of the
same bytes (volume + label) as the memory-rate yardstick, glcm's wall time with its one readback, and the numpy shifted-slice chain on the host
with its transfers (run once, and compared bin for bin)."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import hvgan  # noqa: F401
from hvgan import texture as T

dev = torch.device('cuda:0')
SHAPE, VERT, G, LO, WIDTH = (256, 256, 64), 20, 32, -200.0, 25.0


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


def vertebra_label(shape, vid):
    """One ellipsoid in the middle of the crop, vertebra-like: about a sixth of the crop's voxels."""
    g0, g1, g2 = np.meshgrid(*(np.arange(n) - n / 2.0 for n in shape), indexing='ij')
    lab = np.zeros(shape, dtype=np.uint8)
    lab[(g0 / (0.33 * shape[0])) ** 2 + (g1 / (0.33 * shape[1])) ** 2 + (g2 / (0.4 * shape[2])) ** 2 <= 1.0] = vid
    return lab


def host_chain(d_vol, d_lab, vid, offsets):
    """The numpy chain this operator replaces: 13 shifted full-volume passes, after the downloads."""
    vol, lab = d_vol.cpu().numpy(), d_lab.cpu().numpy()
    t = (vol.astype(np.float64) - LO) / WIDTH
    lev = np.clip(np.trunc(np.clip(t, -1.0, float(G))), 0, G - 1).astype(np.int64)
    inside = lab == vid
    out = np.zeros((len(offsets), G, G), dtype=np.int64)
    for n, d in enumerate(offsets):
        src = tuple(slice(max(0, -c), a - max(0, c)) for a, c in zip(vol.shape, d))
        dst = tuple(slice(max(0, c), a - max(0, -c)) for a, c in zip(vol.shape, d))
        both = inside[src] & inside[dst]
        m = np.bincount(lev[src][both] * G + lev[dst][both], minlength=G * G).reshape(G, G)
        out[n] = m + m.T
    return out


def run(name, vol, lab):
    d_vol, d_lab = torch.from_numpy(vol).to(dev), torch.from_numpy(lab).to(dev)
    off = T.directions(1)
    buf, out, info = T._buffers(1, 1, len(off), G, dev)
    t_dev = median_us(lambda: T._launch(d_vol[None], d_lab[None], None, [VERT], off, G, LO, WIDTH, True, out, info))
    c_vol, c_lab = torch.empty_like(d_vol), torch.empty_like(d_lab)
    t_copy = median_us(lambda: (c_vol.copy_(d_vol), c_lab.copy_(d_lab)))
    del c_vol, c_lab
    T.glcm(d_vol, d_lab, [VERT], off, G, LO, WIDTH)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = T.glcm(d_vol, d_lab, [VERT], off, G, LO, WIDTH)
    wall = (time.perf_counter() - t0) * 1e6
    t0 = time.perf_counter()
    ref = host_chain(d_vol, d_lab, VERT, off.tolist())
    chain = time.perf_counter() - t0
    nbytes = d_vol.numel() * d_vol.element_size() + d_lab.numel() * d_lab.element_size()
    pairs = int(res['matrices'].sum()) // 2
    print('%s (%.0f MB, %d voxels in the label, %d pairs, %d non-zero bins): hv_glcm %.0f us = %.1f x the device copy of the same bytes (%.0f us); '
          'glcm %.0f us wall with its readback; numpy shifted-slice chain on the host with its transfers %.0f ms; equal: %s'
          % (name, nbytes / 1e6, int(res['count'][0]), pairs, int((res['matrices'] != 0).sum()), t_dev, t_dev / t_copy, t_copy, wall, chain * 1e3,
             bool((res['matrices'][0] == ref).all())), flush=True)


r = np.random.RandomState(0)
lab = vertebra_label(SHAPE, VERT)
i, j, k = np.meshgrid(*(np.arange(n) for n in SHAPE), indexing='ij')
smooth = 200.0 + 120.0 * np.sin(i / 9.0) * np.cos(j / 11.0) + 60.0 * np.sin(k / 5.0) + r.standard_normal(SHAPE) * 40.0
for dtype in (np.int16, np.float64):
    run('256x256x64 %s crop, smooth + noise' % np.dtype(dtype).name, np.round(smooth).astype(dtype), lab)
    run('256x256x64 %s crop, constant' % np.dtype(dtype).name, np.full(SHAPE, 300, dtype=dtype), lab)
