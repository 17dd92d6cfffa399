"""The volume intake / output kernels of the inference driver, entry by entry, for both slice axes: hv_volume_scan_view / hv_volume_slices_view /
hv_volume_merge_view on one 256 x 256 x 64 volume (axis 2, the sagittal view) and on its swap 256 x 64 x 256 (axis 1, the coronal view) -- the same
voxels, the same 51 of 64 slices cut and merged.  Prints the time per launch (device events around `--iters` back-to-back launches: an upper bound that includes the launch gaps) and the bytes per second
of what the algorithm has to move; run under `rocprofv3 --kernel-trace --stats -- python tools/prof_volume_views.py` for the per-kernel times.
--baseline-lib PATH times the hv_volume_scan / slices / merge entries of another build of the library (the parent commit's) on the same buffers.
Compare the rates with tools/hbm_rw_probe.py's copy rate on the same box."""
import argparse, ctypes, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import hvgan  # noqa: F401
from hvgan import lib, synth

ap = argparse.ArgumentParser()
ap.add_argument('--iters', type=int, default=200)
ap.add_argument('--dtype', default='float64', choices=['float64', 'float32', 'uint8'])
ap.add_argument('--baseline-lib', default=None)
args = ap.parse_args()
L = lib.get()
dev = torch.device('cuda:0')
tdt = getattr(torch, args.dtype)
DT = {torch.uint8: 0, torch.float32: 4, torch.float64: 5}[tdt]
esz = torch.empty(0, dtype=tdt).element_size()
ct, label, cam = synth.make_volume(nz=64, size=256, seed=2)
K0, S = 6, 51
ROT = 8                     # rotating buffers: 8 x 33.5 MB of float64 exceed what the L2 holds


def timeit(f):
    for i in range(4):
        f(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(args.iters):
        f(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.iters * 1e3


def report(name, us, nbytes):
    print('%-44s %8.1f us  %6.2f TB/s (%.1f MB moved)' % (name, us, nbytes / us / 1e6, nbytes / 1e6), flush=True)


for axis in (2, 1):
    swap = (lambda v: v) if axis == 2 else (lambda v: np.ascontiguousarray(np.swapaxes(v, 1, 2)))
    lab = [torch.from_numpy(swap(label)).to(dev).to(tdt) for _ in range(ROT)]
    vol = [torch.from_numpy(swap(ct)).to(dev).to(tdt) for _ in range(ROT)]
    A0, A1, A2 = shape = tuple(lab[0].shape)
    n, N = A0 * A1 * A2, shape[axis]
    counts = torch.empty(3 * N, dtype=torch.int32, device=dev)
    sl = [torch.empty(S, 256, 256, dtype=torch.float32, device=dev) for _ in range(ROT)]
    flag = torch.ones(S, dtype=torch.int32, device=dev)
    p, st = lib.ptr, lib.stream
    tag = 'axis %d %s %s' % (axis, 'x'.join(map(str, shape)), args.dtype)
    report('hv_volume_scan_view   ' + tag, timeit(lambda i: L.call('hv_volume_scan_view', p(lab[i % ROT]), DT, A0, A1, A2, axis, 20.0, 19.0, 21.0, p(counts), st())), n * esz)
    report('hv_volume_slices_view ' + tag, timeit(lambda i: L.call('hv_volume_slices_view', p(vol[i % ROT]), DT, A0, A1, A2, axis, K0, S, p(sl[i % ROT]), st())),
           S * 65536 * (esz + 4))
    for odt, oname in ((5, 'float64'), (4, 'float32')):
        out = [torch.empty(shape, dtype=getattr(torch, oname), device=dev) for _ in range(ROT)]
        report('hv_volume_merge_view  axis %d -> %s' % (axis, oname),
               timeit(lambda i: L.call('hv_volume_merge_view', p(sl[i % ROT]), p(flag), A0, A1, A2, axis, K0, S, odt, p(out[i % ROT]), st())),
               S * 65536 * 4 + n * out[0].element_size())
        del out
    if axis == 2 and args.baseline_lib and args.dtype == 'float64':
        B = ctypes.CDLL(os.path.abspath(args.baseline_lib))
        for name in ('hv_volume_scan', 'hv_volume_slices', 'hv_volume_merge'):
            getattr(B, name).argtypes = L.protos[name][1]
        HW = A0 * A1
        out = [torch.empty(shape, dtype=torch.float64, device=dev) for _ in range(ROT)]
        print('baseline %s (hv_version %d)' % (args.baseline_lib, B.hv_version()))
        report('  hv_volume_scan   (baseline)', timeit(lambda i: B.hv_volume_scan(p(lab[i % ROT]), HW, A2, 20.0, 19.0, 21.0, p(counts), st())), n * 8)
        report('  hv_volume_slices (baseline)', timeit(lambda i: B.hv_volume_slices(p(vol[i % ROT]), HW, A2, K0, S, p(sl[i % ROT]), st())), S * 65536 * 12)
        report('  hv_volume_merge  (baseline)', timeit(lambda i: B.hv_volume_merge(p(sl[i % ROT]), p(flag), HW, A2, K0, S, p(out[i % ROT]), st())), S * 65536 * 4 + n * 8)
        del out
