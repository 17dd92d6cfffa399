"""Generation-quality evaluation of one 256 x 256 x 64 volume pair (float64 CT and labels, the vertebra spanning 55 slices): device
(hv_gen_eval, volumes resident in HBM) vs the float64 host restatement tests/gen_eval_ref.py.  One line per layout and view:
us per pair, GB/s on the 134 MB the call reads at least once, the restatement's time, max |d| over the seven values.

    --items N --experiments E    the set form instead: N originals x E synthesized volumes each, all resident.  Per layout and view: the
                                 device time of one hv_gen_eval_batch call, the wall time of process_images_batch (tables, launch, readback),
                                 and N * E hv_gen_eval calls queued back to back in the same process on the same volumes."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch
import hvgan  # noqa: F401
from hvgan import generation_eval as GE
import gen_eval_ref as ref

ap = argparse.ArgumentParser()
ap.add_argument('--items', type=int, default=0)
ap.add_argument('--experiments', type=int, default=0)
args = ap.parse_args()
H, W, Z, LABEL = 256, 256, 64, 20
rng = np.random.default_rng(0)
g = np.meshgrid(np.arange(H) - 128.0, np.arange(W) - 128.0, np.arange(Z) - 31.5, indexing='ij')
ori = np.zeros((H, W, Z))
ori[(g[0] / 40) ** 2 + (g[1] / 60) ** 2 + (g[2] / 27.6) ** 2 <= 1] = LABEL
ori[(g[0] + 70) ** 2 / 30 ** 2 + (g[1] / 60) ** 2 <= 1] = LABEL - 1
fake = np.zeros((H, W, Z))
fake[((g[0] - 2) / 38) ** 2 + (g[1] / 62) ** 2 + (g[2] / 27.6) ** 2 <= 1] = LABEL
ct = np.round(rng.uniform(0, 255, size=(H, W, Z)))
fct = ct + np.round(rng.normal(0, 12, size=(H, W, Z))) * (fake == LABEL)
zs = np.flatnonzero((ori == LABEL).any(axis=(0, 1)))
dev = torch.device('cuda:0')
N = 50


def timed(fn, reps):
    """(device us, wall us) per call of fn, medians over `reps` calls, after warm-up."""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    d, w = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        w.append((time.perf_counter() - t0) * 1e6)
        d.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(d)), float(np.median(w))


def bench_set(n_items, n_exp, vols, layout, view):
    # distinct storage for every volume, as a resident validation set has
    originals = [(vols[0].clone(), vols[2].clone(), LABEL) for _ in range(n_items)]
    fakes = [[(vols[1].clone(), vols[3].clone()) for _ in range(n_exp)] for _ in range(n_items)]
    E, groups = GE.group_items(originals, fakes)
    (sig, idx), = groups
    out = torch.zeros(n_items, n_exp, 16, dtype=torch.float64, device=dev)
    outs = torch.zeros(n_items * n_exp, 16, dtype=torch.float64, device=dev)
    keep = []

    def batch():
        keep[:] = GE._launch_batch(sig, originals, fakes, idx, E, view, out, None, dev)

    def loop():
        for i in range(n_items):
            for e in range(n_exp):
                GE._launch(originals[i][0], fakes[i][e][0], originals[i][1], fakes[i][e][1], LABEL, view, outs[i * n_exp + e])
    b_dev, _ = timed(batch, 7)
    _, b_wall = timed(lambda: GE.process_images_batch(originals, fakes, view=view, chunk=n_items), 5)
    l_dev, l_wall = timed(loop, 5)
    same = bool((out.view(torch.int64).reshape(-1, 16) == outs.view(torch.int64)).all())
    P = n_items * n_exp
    print('hv_gen_eval_batch %dx%dx%d, %d items x %d experiments, %s-order, %s: batch call %.0f us device (%.1f us per pair), '
          'process_images_batch %.0f us wall; %d hv_gen_eval calls back to back %.0f us device / %.0f us wall (%.1f us per pair): '
          'x%.2f; bits equal: %s' % (H, W, Z, n_items, n_exp, layout, view, b_dev, b_dev / P, b_wall, P, l_dev, l_wall, l_dev / P,
                                     l_dev / b_dev, same), flush=True)


for layout in ('C', 'F'):
    vols = [torch.from_numpy(np.ascontiguousarray(a) if layout == 'C' else np.asfortranarray(a)).to(dev) for a in (ct, fct, ori, fake)]
    for view in ('sagittal', 'coronal'):
        if args.items and args.experiments:
            bench_set(args.items, args.experiments, vols, layout, view)
            continue
        out = torch.empty(16, dtype=torch.float64, device=dev)
        for _ in range(3):
            GE._launch(*vols, LABEL, view, out)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(N):
            GE._launch(*vols, LABEL, view, out)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) / N * 1e3
        t0 = time.perf_counter()
        want = ref.process_images(ct, fct, ori, fake, LABEL, view=view)
        cpu_ms = (time.perf_counter() - t0) * 1e3
        got = GE.process_images(*vols, LABEL, view=view)
        byt = 4 * ct.size * 8
        d = max(abs(a - b) for a, b in zip(got, want))
        print('hv_gen_eval %dx%dx%d pair (vertebra over %d slices), %s-order, %s: %.1f us per pair (%.0f GB/s of the %.0f MB read once), '
              'CPU restatement %.0f ms; max |d| %.2e' % (H, W, Z, len(zs), layout, view, us, byt / us / 1e3, byt / 1e6, cpu_ms, d), flush=True)
