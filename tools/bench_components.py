"""3-D connected components of one 256 x 256 x 64 uint8 label crop -- a vertebra-sized blob plus a few hundred speckle voxels -- resident in
HBM, z-fastest (as straighten_patient leaves a crop) and in C order, and of a batch of 13 such crops: device time of hv_label3d,
hv_clean_components (keep the largest component) and hv_fill_holes (events around back-to-back launches, median of 10), wall time of
clean_label with the table readback, the scipy chain on the host with its two transfers, and a plain device copy of the same bytes."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from scipy.ndimage import generate_binary_structure
from scipy.ndimage import label as nd_label
import hvgan  # noqa: F401
from hvgan import components as C

H, W, Z, LABEL, BATCH = 256, 256, 64, 20, 13
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


def host_chain(d):
    v = d.cpu().numpy()                                                                   # download
    lab, n = nd_label(v == LABEL, generate_binary_structure(3, 1))
    keep = np.argmax(np.bincount(lab.ravel())[1:]) + 1
    v[(lab > 0) & (lab != keep)] = 0
    return torch.from_numpy(v).to(dev)                                                    # upload


host = crop(0)
layouts = {'C order': torch.from_numpy(host).to(dev),
           'z-fastest': torch.from_numpy(np.ascontiguousarray(host.transpose(2, 0, 1))).to(dev).permute(1, 2, 0)}
for name, d in layouts.items():
    labels = torch.empty(H, W, Z, dtype=torch.int32, device=dev)
    out = torch.empty(H, W, Z, dtype=torch.uint8, device=dev)
    table = torch.empty(8, dtype=torch.int32, device=dev)
    t_label = median_us(lambda: C.label(d, LABEL, out=labels, max_components=512))
    t_clean = median_us(lambda: C._launch_clean(d, float(LABEL), 1, 0, True, 0.0, out, table[:4]))
    t_fill = median_us(lambda: C._launch_fill(d, float(LABEL), float(LABEL), out, table[4:]))
    t_copy = median_us(lambda: out.copy_(d))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got, tb = C.clean_label(d, LABEL, return_table=True)
    tb = tb.cpu().numpy()
    wall = (time.perf_counter() - t0) * 1e6
    host_chain(d)
    t0 = time.perf_counter()
    want = host_chain(d)
    torch.cuda.synchronize()
    chain = (time.perf_counter() - t0) * 1e6
    same = bool(torch.equal(got, want))
    print('%dx%dx%d uint8 crop, %s (%d components, the largest %d voxels): hv_label3d %.0f us, hv_clean_components %.0f us, hv_fill_holes '
          '%.0f us device; clean_label %.0f us wall with the table readback; scipy chain on the host with its two transfers %.0f ms; device '
          'copy of the same bytes %.1f us; equal to the host chain: %s' % (H, W, Z, name, tb[0], tb[2], t_label, t_clean, t_fill, wall,
                                                                           chain / 1e3, t_copy, same), flush=True)

batch = [torch.from_numpy(crop(s)).to(dev) for s in range(BATCH)]
for _ in range(2):
    C.clean_labels(batch, LABEL)
torch.cuda.synchronize()
walls = []
for _ in range(10):
    t0 = time.perf_counter()
    outs, tables = C.clean_labels(batch, LABEL)
    walls.append((time.perf_counter() - t0) * 1e6)
t0 = time.perf_counter()
for d in batch:
    host_chain(d)
torch.cuda.synchronize()
chain = (time.perf_counter() - t0) * 1e6
print('batch of %d crops: clean_labels %.0f us wall with one readback of the tables (median of 10; %.0f us per crop); scipy chain on the '
      'host %.0f ms' % (BATCH, statistics.median(walls), statistics.median(walls) / BATCH, chain / 1e3), flush=True)
