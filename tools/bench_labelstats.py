"""Per-label intensity statistics (hv_label_stats) of resident volumes: one 256 x 256 x 64 float64 crop with three labels, a batch of 13 such
crops, and a 512 x 512 x 400 int16 scan with 24 labels, each without percentiles (Q = 0: the moments pass) and with three (Q = 3: 8 / 2 select
passes on top).  Device time from events around back-to-back launches, median of 10; beside it a plain device copy of the same bytes (volume
+ label), label_statistics' wall time with its one readback, and the scipy / numpy chain on the host with its transfers (run once).
Reported: the moments pass as a multiple of the copy, and the cost of one select pass ((t[Q = 3] - t[Q = 0]) / passes)."""
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
from hvgan import label_statistics as S

dev = torch.device('cuda:0')
QS = (5.0, 50.0, 95.0)


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


def crop_labels(shape, ids):
    """len(ids) ellipsoids stacked along axis 0, vertebra-like: each about a fifth of its slab."""
    lab = np.zeros(shape, dtype=np.uint8)
    n = len(ids)
    g1, g2 = np.meshgrid(np.arange(shape[1]) - shape[1] / 2.0, np.arange(shape[2]) - shape[2] / 2.0, indexing='ij')
    inplane = (g1 / (0.3 * shape[1])) ** 2 + (g2 / (0.43 * shape[2])) ** 2
    h = shape[0] / n
    for s, l in enumerate(ids):
        for i in range(int(s * h), int((s + 1) * h)):
            lab[i][inplane + ((i - (s + 0.5) * h) / (0.45 * h)) ** 2 <= 1.0] = l
    return lab


def host_chain(d_vol, d_lab, ids):
    vol, lab = d_vol.cpu().numpy(), d_lab.cpu().numpy()                                    # downloads
    out = []
    for v, l in zip(vol.reshape((-1,) + vol.shape[-3:]), lab.reshape((-1,) + lab.shape[-3:])):
        idx = list(ids)
        r = [ndimage.sum_labels(v, l, idx), ndimage.mean(v, l, idx), ndimage.variance(v, l, idx), ndimage.minimum(v, l, idx),
             ndimage.maximum(v, l, idx), ndimage.center_of_mass(np.ones_like(l), l, idx), ndimage.find_objects(l.astype(np.int32))]
        r.append([np.percentile(v[l == i].astype(np.float64), QS) for i in idx])
        out.append(r)
    return out


def run(name, vol, lab, ids, host=True):
    d_vol, d_lab = torch.from_numpy(vol).to(dev), torch.from_numpy(lab).to(dev)
    v4, l4 = (d_vol, d_lab) if d_vol.dim() == 4 else (d_vol[None], d_lab[None])
    V = v4.shape[0]
    passes = {torch.uint8: 2, torch.int16: 2, torch.float32: 4, torch.float64: 8}[d_vol.dtype]
    t = {}
    for q in ((), QS):
        out = torch.empty((V, len(ids), S.REC), dtype=torch.float64, device=dev)
        t[len(q)] = median_us(lambda: S._launch(v4, l4, None, list(ids), list(q), out))
    c_vol, c_lab = torch.empty_like(d_vol), torch.empty_like(d_lab)
    t_copy = median_us(lambda: (c_vol.copy_(d_vol), c_lab.copy_(d_lab)))
    del c_vol, c_lab
    S.label_statistics(d_vol, d_lab, ids, QS)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = S.label_statistics(d_vol, d_lab, ids, QS)
    wall = (time.perf_counter() - t0) * 1e6
    nbytes = d_vol.numel() * d_vol.element_size() + d_lab.numel() * d_lab.element_size()
    line = ('%s (%d labels, %.0f MB): moments (Q = 0) %.0f us = %.2f x the device copy of the same bytes (%.0f us; %.2f TB/s read); Q = 3 %.0f us: '
            '%.0f us per select pass (%d passes); label_statistics %.0f us wall with its readback'
            % (name, len(ids), nbytes / 1e6, t[0], t[0] / t_copy, t_copy, nbytes / t[0] / 1e6, t[3], (t[3] - t[0]) / passes, passes, wall))
    if host:
        t0 = time.perf_counter()
        ref = host_chain(d_vol, d_lab, ids)
        chain = time.perf_counter() - t0
        cnt = np.asarray(res['count']).reshape(V, -1)
        mean = np.asarray(res['mean']).reshape(V, -1)
        pct = np.asarray(res['percentiles']).reshape(V, len(ids), -1)
        dm = max(abs(mean[v, s] - ref[v][1][s]) / abs(ref[v][1][s]) for v in range(V) for s in range(len(ids)))
        same = all(pct[v, s, k] == ref[v][7][s][k] for v in range(V) for s in range(len(ids)) for k in range(3))
        line += '; scipy / numpy chain on the host with its transfers %.0f ms; largest relative mean difference %.2g, percentiles equal: %s' % (
            chain * 1e3, dm, same)
        assert cnt.min() > 0
    print(line, flush=True)


r = np.random.RandomState(0)
ids3 = (19, 20, 21)
lab = crop_labels((256, 256, 64), ids3)
vol = r.standard_normal((256, 256, 64)) * 150.0 + 300.0
run('256x256x64 float64 crop, C order', vol, lab, ids3)
run('batch of 13 256x256x64 float64 crops', np.stack([vol + s for s in range(13)]), np.stack([lab] * 13), ids3)
ids24 = tuple(range(1, 25))
lab = crop_labels((512, 512, 400), ids24)
vol = (r.standard_normal((64, 512, 400)) * 300.0 + 200.0).astype(np.int16)
run('512x512x400 int16 scan', np.ascontiguousarray(np.tile(vol, (8, 1, 1))), lab, ids24)
