"""Per-label run-length matrices (hv_glrlm, the 13 directions, nothing capped) and dependence / neighbourhood sums (hv_gldm) of a resident volume:
one 256 x 256 x 64 int16 crop with a vertebra-sized label, G = 32; once on noise (every level equally likely: almost every run has length 1, the
most runs to count) and once on a constant (the longest runs: one lane walks a whole line, and every count falls in one bin).  Device time from
events around back-to-back launches, median of 10.  Two yardsticks from the same run: a plain device copy of the inputs (volume + label), and
hv_glcm on the same crop with the 13 offsets."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import hvgan  # noqa: F401
from hvgan import texture as T
from hvgan import texture_runs as R

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


def run(name, vol, lab):
    d_vol, d_lab = torch.from_numpy(vol).to(dev), torch.from_numpy(lab).to(dev)
    off, Rmax = T.directions(1), max(SHAPE)
    b = R._Buffers(1, 1, G, dev, D=len(off), R=Rmax)
    t_rlm = median_us(lambda: R._launch_glrlm(d_vol[None], d_lab[None], None, [VERT], off, G, LO, WIDTH, Rmax, b.dev('out'), b.dev('info_r')))
    t_dm = median_us(lambda: R._launch_gldm(d_vol[None], d_lab[None], None, [VERT], G, LO, WIDTH, 0, b.dev('dep'), b.dev('ngt'), b.dev('info_d')))
    host = b.read()
    _, g_out, g_info = T._buffers(1, 1, len(off), G, dev)
    t_glcm = median_us(lambda: T._launch(d_vol[None], d_lab[None], None, [VERT], off, G, LO, WIDTH, True, g_out, g_info))
    c_vol, c_lab = torch.empty_like(d_vol), torch.empty_like(d_lab)
    t_copy = median_us(lambda: (c_vol.copy_(d_vol), c_lab.copy_(d_lab)))
    nbytes = d_vol.numel() * d_vol.element_size() + d_lab.numel() * d_lab.element_size()
    runs = host['out'][0, 0].sum(axis=(1, 2))
    print('%s (%.0f MB, %d voxels in the label, %d .. %d runs per direction): hv_glrlm %.0f us, hv_gldm %.0f us; hv_glcm with the 13 offsets %.0f us '
          '(glrlm %.2f x, gldm %.2f x); device copy of the inputs %.0f us (glrlm %.1f x, gldm %.1f x)'
          % (name, nbytes / 1e6, int(host['info_r'][0, 0, 1]), int(runs.min()), int(runs.max()), t_rlm, t_dm, t_glcm, t_rlm / t_glcm, t_dm / t_glcm,
             t_copy, t_rlm / t_copy, t_dm / t_copy), flush=True)


lab = vertebra_label(SHAPE, VERT)
noise = np.random.RandomState(0).randint(-200, 600, SHAPE).astype(np.int16)
run('256x256x64 int16 crop, noise', noise, lab)
run('256x256x64 int16 crop, constant', np.full(SHAPE, 300, dtype=np.int16), lab)
