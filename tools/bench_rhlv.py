"""RHLV quantification of 256 x 256 x 64 label-volume pairs resident in HBM:
  * one pair, sagittal view: device (hv_rhlv) vs the CPU oracle;
  * one pair, both views (the 2.5D grade's six features): rhlv_volume_25d (one pass over the volumes, one readback) vs two rhlv_volume
    calls, the second on the permuted view -- the only way to both views before hv_rhlv_views (its coronal numbers follow the sagittal
    script's arithmetic, so it is a timing yardstick only);
  * one pair, both views, the per-column height-loss maps and profiles: height_loss_map (rhlv_volume_25d's launches plus two, the maps left in
    HBM) vs the host alternative -- download both volumes and run the numpy restatement (tests/height_map_ref.py) on them;
  * a dataset of 64 pairs: rhlv_dataset (one launch sequence, one readback) vs 64 rhlv_volume_25d calls.
Device-only times are hipEvent brackets around back-to-back launches; the end-to-end times (`wall`) include the readbacks and are
medians of repeated wall-clock measurements.

    python tools/bench_rhlv.py --sweep [--pairs N] [--divisors D] [--thresholds T] [--parent-lib PATH]
times instead one rhlv_sweep over N pairs and a D x T grid (device and wall) against the same grid as D * T rhlv_dataset calls in the same
process, per (pair, grid point), and -- with the parent commit's libhvgan.so given -- hv_rhlv_views through that library and through this one,
loaded side by side, in alternating rounds."""
import argparse, ctypes, os, sys, time
_ap = argparse.ArgumentParser()
_ap.add_argument('--sweep', action='store_true')
_ap.add_argument('--pairs', type=int, default=64)
_ap.add_argument('--divisors', type=int, default=5)
_ap.add_argument('--thresholds', type=int, default=8)
_ap.add_argument('--parent-lib', default=None)
ARGS = _ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import hvgan
from hvgan import evaluation, synth
from oracle import restate as R

fake, label = synth.make_rhlv_pair(seed=7, H=256, W=256, Z=64, empty_ends=6)
f, l = torch.from_numpy(fake).float().cuda(), torch.from_numpy(label).float().cuda()


def device_us(fn, n=50, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def wall_us(fn, n=20, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(ts))


def sweep_bench():
    from hvgan import lib as _lib, ops
    L = _lib.get()
    N, D, T = ARGS.pairs, ARGS.divisors, ARGS.thresholds
    divs = [1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 20, 24, 32, 48, 64, 1000][:D]
    thrs = [round(0.3 + 0.7 * i / max(1, T - 1), 4) for i in range(T)]
    fakes, labels = [], []
    for i in range(N):
        a, b = synth.make_rhlv_pair(seed=100 + i, H=256, W=256, Z=64, empty_ends=6, collapse=0.05 * (i % 8))
        fakes.append(torch.from_numpy(a).float().cuda())
        labels.append(torch.from_numpy(b).float().cuda())
    ids = [20] * N
    sweep = evaluation.rhlv_sweep(fakes, labels, ids, divs, thrs)
    rec = sweep['records']
    for d in (0, D - 1):
        for t in (0, T - 1):
            one, _ = evaluation.rhlv_dataset(fakes, labels, ids, divs[d], thrs[t])
            assert np.array_equal(rec[:, d, t].view(np.int64), one.view(np.int64)), (d, t)
    # device time: the C entries back to back on prepared buffers, no readback
    dev = fakes[0].device
    geo = evaluation._geometry(fakes[0])
    table = torch.tensor([p for a, b in zip(fakes, labels) for p in (a.data_ptr(), b.data_ptr())], dtype=torch.int64).to(dev)
    idt = torch.tensor([20.0] * N, dtype=torch.float32).to(dev)
    both = evaluation.SAGITTAL | evaluation.CORONAL
    ws = torch.empty(L.size('hv_rhlv_sweep_workspace_bytes', 256, 64, both, N, D, T) + 64, dtype=torch.uint8, device=dev)
    out = torch.empty(N, D, T, 2, 16, dtype=torch.float64, device=dev)
    grid = L.hv_rhlv_grid(D, (ctypes.c_int * 16)(*divs), T, (ctypes.c_double * 32)(*thrs))

    def sweep_dev():
        L.call('hv_rhlv_sweep', _lib.ptr(table), _lib.ptr(idt), N, *geo, both, ctypes.byref(grid), _lib.ptr(out), _lib.ptr(ws),
               ctypes.c_size_t(ws.numel()), _lib.stream())

    def calls_dev():
        for dv in divs:
            for th in thrs:
                sag, cor = evaluation._view_args(L, both, dv, evaluation.INT_MIN, 0, th)
                L.call('hv_rhlv_views_batch', _lib.ptr(table), _lib.ptr(idt), N, *geo, both, sag, cor, _lib.ptr(out), _lib.ptr(ws),
                       ctypes.c_size_t(ws.numel()), _lib.stream())

    s_dev, c_dev = device_us(sweep_dev, n=20), device_us(calls_dev, n=5, warm=1)
    s_wall = wall_us(lambda: evaluation.rhlv_sweep(fakes, labels, ids, divs, thrs), n=10)
    c_wall = wall_us(lambda: [evaluation.rhlv_dataset(fakes, labels, ids, dv, th) for dv in divs for th in thrs], n=5, warm=1)
    one_dev = c_dev / (D * T)
    print('RHLV sweep, %d float32 256x256x64 pairs, %d divisors x %d thresholds, both views: rhlv_sweep %.1f us device / %.1f us wall = '
          '%.3f / %.3f us per (pair, grid point); %d rhlv_dataset calls %.1f us device / %.1f us wall = %.3f / %.3f us per (pair, grid point); '
          'one rhlv_dataset call %.1f us device; sampled grid points bit-identical'
          % (N, D, T, s_dev, s_wall, s_dev / (N * D * T), s_wall / (N * D * T), D * T, c_dev, c_wall, c_dev / (N * D * T), c_wall / (N * D * T),
             one_dev))
    if ARGS.parent_lib:
        # hv_rhlv_views through the parent commit's library and through this one, side by side
        P = ctypes.CDLL(os.path.abspath(ARGS.parent_lib))
        fn_old, fn_new = P.hv_rhlv_views, L.cdll.hv_rhlv_views
        fn_old.restype, fn_old.argtypes = fn_new.restype, fn_new.argtypes
        f0, l0 = fakes[0], labels[0]
        sag, cor = evaluation._view_args(L, both, 5, evaluation.INT_MIN, 0, 0.64)
        outs = [torch.zeros(2, 16, dtype=torch.float64, device=dev) for _ in range(2)]

        def run(fn, o):
            rc = fn(_lib.ptr(f0), _lib.ptr(l0), *geo, ctypes.c_float(20.0), both, sag, cor, _lib.ptr(o), _lib.ptr(ws), ctypes.c_size_t(ws.numel()),
                    _lib.stream())
            assert rc == 0, rc

        rounds = [(device_us(lambda: run(fn_old, outs[0]), n=200), device_us(lambda: run(fn_new, outs[1]), n=200)) for _ in range(9)]
        assert torch.equal(outs[0], outs[1])
        old, new = (float(np.median([r[i] for r in rounds])) for i in (0, 1))
        print('hv_rhlv_views, one 256x256x64 float32 pair, both views, 9 alternating rounds of 200 calls: parent library %.1f us (spread %.1f), '
              'this library %.1f us (spread %.1f); records bit-identical'
              % (old, max(r[0] for r in rounds) - min(r[0] for r in rounds), new, max(r[1] for r in rounds) - min(r[1] for r in rounds)))


if ARGS.sweep:
    sweep_bench()
    sys.exit(0)

us = device_us(lambda: evaluation._run(f, l, 20.0, 5, evaluation.INT_MIN, 0, 0.64))
t0 = time.perf_counter()
ref, _ = R.rhlv_volume(fake, label, 20)
cpu_ms = (time.perf_counter() - t0) * 1e3
got = evaluation.rhlv_volume(f, l, 20)
byt = 2 * fake.size * 4
print('hv_rhlv 256x256x64 pair: %.1f us per pair (%.1f GB/s of the %.1f MB read once), CPU oracle %.1f ms; max |d| %.2e'
      % (us, byt / us / 1e3, byt / 1e6, cpu_ms, max(abs(a - b) for a, b in zip(got, ref))))

# (a) both views of one pair
fp, lp = f.permute(0, 2, 1), l.permute(0, 2, 1)
both = evaluation.SAGITTAL | evaluation.CORONAL


def two_calls_device():
    evaluation._run(f, l, 20.0, 5, evaluation.INT_MIN, 0, 0.64)
    evaluation._run(fp, lp, 20.0, 5, evaluation.INT_MIN, 0, 0.64)


def two_calls():
    return evaluation.rhlv_volume(f, l, 20), evaluation.rhlv_volume(fp, lp, 20)


one_dev = device_us(lambda: evaluation._run_views(f, l, 20.0, both, 5, evaluation.INT_MIN, 0, 0.64))
two_dev = device_us(two_calls_device)
one_wall = wall_us(lambda: evaluation.rhlv_volume_25d(f, l, 20))
two_wall = wall_us(two_calls)
print('2.5D, one 256x256x64 pair: rhlv_volume_25d %.1f us device / %.1f us wall; two rhlv_volume calls (second on the permuted view) '
      '%.1f us device / %.1f us wall' % (one_dev, one_wall, two_dev, two_wall))

# (a') the per-column maps and profiles of the same pair
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
import height_map_ref


def host_maps():
    hf, hl = f.cpu().numpy(), l.cpu().numpy()
    return [height_map_ref.view_maps(hf, hl, 20, 5, 0.64, view) for view in ('sagittal', 'coronal')]


bufs = evaluation._run_maps(f, l, 20.0, both, 5, evaluation.INT_MIN, 0, 0.64)      # allocated once: the bracket holds launches only
map_dev = device_us(lambda: evaluation._run_maps(f, l, 20.0, both, 5, evaluation.INT_MIN, 0, 0.64, buffers=bufs))
map_wall = wall_us(lambda: evaluation.height_loss_map(f, l, 20))
host_wall = wall_us(host_maps, n=5, warm=1)
maps, ref = evaluation.height_loss_map(f, l, 20), host_maps()
worst = max(float(np.nanmax(np.abs(maps[view]['loss'].cpu().numpy() - r['loss']))) for view, r in zip(('sagittal', 'coronal'), ref))
print('height-loss maps, one 256x256x64 pair, both views: height_loss_map %.1f us device / %.1f us wall (rhlv_volume_25d: %.1f / %.1f); '
      'download + numpy restatement %.1f ms wall; max |d loss| %.2e' % (map_dev, map_wall, one_dev, one_wall, host_wall / 1e3, worst))

# (b) a dataset of 64 resident pairs
N = 64
fakes, labels = [], []
for i in range(N):
    a, b = synth.make_rhlv_pair(seed=100 + i, H=256, W=256, Z=64, empty_ends=6, collapse=0.05 * (i % 8))
    fakes.append(torch.from_numpy(a).float().cuda())
    labels.append(torch.from_numpy(b).float().cuda())
ids = [20] * N
rec, present = evaluation.rhlv_dataset(fakes, labels, ids)
single = evaluation.rhlv_volume_25d(fakes[5], labels[5], 20)
assert present.all() and tuple(rec[5, 0, :5]) == single['sagittal'] and tuple(rec[5, 1, :5]) == single['coronal']
batch_wall = wall_us(lambda: evaluation.rhlv_dataset(fakes, labels, ids), n=10)
loop_wall = wall_us(lambda: [evaluation.rhlv_volume_25d(a, b, 20) for a, b in zip(fakes, labels)], n=10)
print('2.5D dataset of %d 256x256x64 pairs: rhlv_dataset %.1f us per pair wall (one readback); %d rhlv_volume_25d calls %.1f us per pair wall'
      % (N, batch_wall / N, N, loop_wall / N))
