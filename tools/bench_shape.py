"""Per-label shape records (hv_shape) of a resident label volume: one 256 x 256 x 64 uint8 crop with one vertebra-sized blob, and the same
crop with 13 labels in one call.  Device time from events around back-to-back launches, median of 10; beside it a plain device copy of the
label volume as the memory-rate yardstick, hv_label_stats' moments pass (Q = 0) on the same input (the label volume as its own intensity
volume: the nearest existing one-pass per-label kernel), shape_descriptors' wall time with its one readback, and the numpy restatement on the
host with its transfer (pad, eight shifted slices, bincount; moments and extents on the coordinates -- run once, and compared word for word)."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import hvgan  # noqa: F401
from hvgan import label_statistics as LS
from hvgan import shape as S

dev = torch.device('cuda:0')
SHAPE = (256, 256, 64)


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


def stacked_labels(shape, ids):
    """len(ids) ellipsoids stacked along axis 0, each about a fifth of its slab (tools/bench_labelstats.py's)."""
    lab = np.zeros(shape, dtype=np.uint8)
    g1, g2 = np.meshgrid(np.arange(shape[1]) - shape[1] / 2.0, np.arange(shape[2]) - shape[2] / 2.0, indexing='ij')
    inplane = (g1 / (0.3 * shape[1])) ** 2 + (g2 / (0.43 * shape[2])) ** 2
    h = shape[0] / len(ids)
    for s, l in enumerate(ids):
        for i in range(int(s * h), int((s + 1) * h)):
            lab[i][inplane + ((i - (s + 0.5) * h) / (0.45 * h)) ** 2 <= 1.0] = l
    return lab


def host_chain(d_lab, ids):
    """The numpy restatement this operator replaces, after the download -> int64 [S][REC]."""
    lab = d_lab.cpu().numpy()
    dirs = S.directions(1)
    out = np.zeros((len(ids), S.REC), dtype=np.int64)
    n = tuple(a + 1 for a in lab.shape)
    for s, l in enumerate(ids):
        x = np.pad(lab == l, 1)
        code = np.zeros(n, dtype=np.int64)
        for q in range(8):
            d0, d1, d2 = q >> 2 & 1, q >> 1 & 1, q & 1
            code += x[d0:d0 + n[0], d1:d1 + n[1], d2:d2 + n[2]].astype(np.int64) << q
        out[s, :256] = np.bincount(code.ravel(), minlength=256)
        p = np.argwhere(lab == l).astype(np.int64)
        out[s, S.COUNT] = len(p)
        out[s, S.SUM:S.SUM + 3] = p.sum(axis=0)
        for m, (a, b) in enumerate(S._PAIRS):
            out[s, S.SUM2 + m] = (p[:, a] * p[:, b]).sum()
        dot = p @ dirs.T
        out[s, S.EXTENT:S.STATUS:2], out[s, S.EXTENT + 1:S.STATUS:2] = dot.min(axis=0), dot.max(axis=0)
    return out


def run(name, lab, ids):
    d_lab = torch.from_numpy(lab).to(dev)
    ids = list(ids)
    out = torch.empty((1, len(ids), S.REC), dtype=torch.int64, device=dev)
    t_dev = median_us(lambda: S._launch(d_lab[None], None, ids, out))
    rec = out.cpu().numpy()[0]
    c_lab = torch.empty_like(d_lab)
    t_copy = median_us(lambda: c_lab.copy_(d_lab))
    del c_lab
    ls_out = torch.empty((1, len(ids), LS.REC), dtype=torch.float64, device=dev)
    t_ls = median_us(lambda: LS._launch(d_lab[None], d_lab[None], None, ids, [], ls_out))
    S.shape_descriptors(d_lab, ids)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = S.shape_descriptors(d_lab, ids)
    wall = (time.perf_counter() - t0) * 1e6
    t0 = time.perf_counter()
    ref = host_chain(d_lab, ids)
    chain = time.perf_counter() - t0
    print('%s (%.1f MB, %d labels, %d voxels in them, %d non-zero bins): hv_shape %.0f us = %.1f x the device copy of the label volume (%.0f us) '
          '= %.2f x the moments pass of hv_label_stats on the same input (%.0f us); shape_descriptors %.0f us wall with its readback; numpy '
          'restatement on the host with its transfer %.0f ms; equal: %s; sphericity of the first label %.4f, Euler numbers %d / %d'
          % (name, d_lab.numel() / 1e6, len(ids), int(rec[:, S.COUNT].sum()), int((rec[:, :256] != 0).sum()), t_dev, t_dev / t_copy, t_copy,
             t_dev / t_ls, t_ls, wall, chain * 1e3, bool((rec[:, :S.STATUS] == ref[:, :S.STATUS]).all()), res['sphericity'][0], res['euler_6'][0],
             res['euler_26'][0]), flush=True)


run('256x256x64 uint8 crop, one vertebra-sized blob', vertebra_label(SHAPE, 20), (20,))
ids13 = tuple(range(8, 21))
run('256x256x64 uint8 crop, 13 labels in one call', stacked_labels(SHAPE, ids13), ids13)
