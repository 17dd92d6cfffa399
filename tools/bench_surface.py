"""Surface-distance metrics (HD, HD95, ASSD) of one 256 x 256 x 64 label pair with a vertebra-sized blob, at spacing (0.7, 0.7, 1.5) and at
unit spacing: the device call (hv_surface_distance, volumes resident in HBM) restricted to the sets' bounding box and over the whole volume,
against the scipy chain on the host -- two downloads, binary_erosion and distance_transform_edt twice each, np.percentile.  One line per
spacing: us per pair for each, and the largest relative difference of the three metrics."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from scipy.ndimage import binary_erosion, distance_transform_edt, generate_binary_structure
import hvgan  # noqa: F401
from hvgan import generation_eval as GE

H, W, Z, LABEL = 256, 256, 64, 20
g = np.meshgrid(np.arange(H) - 128.0, np.arange(W) - 128.0, np.arange(Z) - 31.5, indexing='ij')
ori = np.zeros((H, W, Z), dtype=np.uint8)
ori[(g[0] / 40) ** 2 + (g[1] / 60) ** 2 + (g[2] / 27.6) ** 2 <= 1] = LABEL
ori[(g[0] + 70) ** 2 / 30 ** 2 + (g[1] / 60) ** 2 <= 1] = LABEL - 1
fake = np.zeros((H, W, Z), dtype=np.uint8)
fake[((g[0] - 2) / 38) ** 2 + (g[1] / 62) ** 2 + (g[2] / 27.6) ** 2 <= 1] = LABEL
dev = torch.device('cuda:0')
d_ori, d_fake = torch.from_numpy(ori).to(dev), torch.from_numpy(fake).to(dev)
ST = generate_binary_structure(3, 1)


def host_chain(a_dev, b_dev, spacing):
    a, b = a_dev.cpu().numpy() == LABEL, b_dev.cpu().numpy() == LABEL                     # the two downloads
    sa, sb = a & ~binary_erosion(a, ST, border_value=0), b & ~binary_erosion(b, ST, border_value=0)
    ab = distance_transform_edt(~sb, sampling=spacing)[sa]
    ba = distance_transform_edt(~sa, sampling=spacing)[sb]
    return {'hd': max(ab.max(), ba.max()), 'hd95': np.percentile(np.concatenate([ab, ba]), 95), 'assd': (ab.mean() + ba.mean()) / 2}


def device_us(restrict, csp, reps=20):
    out = torch.empty(16, dtype=torch.float64, device=dev)
    for _ in range(3):
        GE._launch_surface(d_ori, d_fake, LABEL, csp, restrict, out)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        GE._launch_surface(d_ori, d_fake, LABEL, csp, restrict, out)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


for spacing in ((0.7, 0.7, 1.5), (1.0, 1.0, 1.0)):
    _, csp = GE._spacing3(spacing)
    boxed, whole = device_us(True, csp), device_us(False, csp)
    t0 = time.perf_counter()
    got = GE.surface_distances(d_ori, d_fake, label=LABEL, spacing=spacing)
    wall = (time.perf_counter() - t0) * 1e6
    host_chain(d_ori, d_fake, spacing)
    t0 = time.perf_counter()
    want = host_chain(d_ori, d_fake, spacing)
    host = (time.perf_counter() - t0) * 1e6
    rel = max(abs(got[k] - want[k]) / want[k] for k in ('hd', 'hd95', 'assd'))
    print('hv_surface_distance %dx%dx%d pair (surfaces of %d and %d voxels), spacing %s: box-restricted %.0f us device (%.0f us wall with the '
          'readback), whole volume %.0f us; scipy chain on the host %.0f ms; hd %.4f hd95 %.4f assd %.4f, max relative |d| %.2e'
          % (H, W, Z, got['n_a'], got['n_b'], spacing, boxed, wall, whole, host / 1e3, got['hd'], got['hd95'], got['assd'], rel), flush=True)
