"""Restore of one vertebra's straightened crop to patient space: device (hvgan.straighten.restore_patient,
csrc/restore.hip) vs the numpy restatement tests/restore_ref.py on the host.  Synthetic 512 x 512 x 400 int16 CT with a 15-vertebra uint8
label, the reference's parameters (plane 128 x 128, out_size (256, 256, 64)), one vertebra in the middle of the spine.  Prints one JSON line:
  knots / box / box_voxels / covered      the curve's knot count, the patient-space box, its voxels and how many of them the crop covers
  restore_ms                              the restore kernel alone: one hv_restore_volume_sp launch with the curve already on the device, events around it, median
  voxels_per_s                            box voxels / that
  patient_ms                              restore_patient end to end with zero bases handed in (host box arithmetic, three small blocking uploads, the launch), median
  copy_ms                                 a plain device copy of the box's bytes (fp64 CT + uint8 label + uint8 covered written per voxel)
  cpu_ref_s_extrapolated                  restore_ref on the host for a sub-box of --cpu-voxels voxels, scaled to the whole box
                                          (EXTRAPOLATED: the per-point Python loop takes minutes per vertebra)

  --order 3 adds: prefilter_ms (hv_spline_prefilter of the crop's filled sub-box), restore3_ms (hv_restore_volume_spline alone),
                  patient3_ms (restore_patient(order=3) end to end: the prefilter and the launch)
  --baseline-lib PATH adds: restore_ms_baseline, hv_restore_volume_sp of another build of the library (the parent commit's) loaded beside this
                  one, timed in the same process, and restore_ms_spread / restore_ms_baseline_spread (max - min over the repeats)

    timeout -k 10 600 python tools/bench_restore.py [--reps 10] [--cpu-voxels 4000] [--no-cpu] [--spacing a,b,c] [--order 3] [--baseline-lib PATH]
--spacing: millimetres per voxel of the same 512 x 512 x 400 voxel patient (default 1,1,1).
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import hvgan  # noqa: E402,F401
from hvgan import lib as _lib, straighten as S, synth  # noqa: E402


def _times(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


def _timed(fn, reps):
    return float(np.median(_times(fn, reps)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--cpu-voxels', type=int, default=4000)
    ap.add_argument('--no-cpu', action='store_true')
    ap.add_argument('--spacing', default='1,1,1')
    ap.add_argument('--order', type=int, default=1, choices=(1, 3))
    ap.add_argument('--baseline-lib', default=None)
    args = ap.parse_args()
    spacing = S.check_spacing([float(v) for v in args.spacing.split(',')])
    shape = (512, 512, 400)
    ct, label = synth.make_spine_patient(seed=11, shape=shape, n_vert=15, radius=(40, 30, 9), end_radius=(14, 12, 5), margin=16, curve=(20.0, 40.0))
    tct, tlab = torch.from_numpy(ct).cuda(), torch.from_numpy(label).cuda()
    vid = [e['label'] for e in S.vertebra_centroids(tlab)][6]
    crops, plan = S.straighten_patient(tct, tlab, [vid], return_plan=True, spacing=spacing)
    box = plan['boxes'][0]
    region = S.restore_box(plan['knots'], plan['basis'], box, shape, spacing=spacing)
    nvox = int(np.prod(region[3:]))
    out = (torch.zeros(shape, dtype=torch.float64, device='cuda'), torch.zeros(shape, dtype=torch.uint8, device='cuda'))

    def run():
        return S.restore_patient(plan, crops, label=tlab, where='crop', return_covered=True, out=out)

    covered = int(run()[2].sum())
    torch.cuda.synchronize()
    patient_ms = _timed(run, args.reps)
    # the kernel alone: the curve uploaded once, hv_restore_volume_sp launched directly, events around each launch
    cvol, lvol = crops[vid]
    d_knots = torch.from_numpy(np.ascontiguousarray(plan['knots'])).cuda()
    d_basis = torch.from_numpy(np.ascontiguousarray(plan['basis'])).cuda()
    d_cum = torch.from_numpy(np.ascontiguousarray(S.cumulative_length(plan['knots']))).cuda()
    cov = torch.zeros(shape, dtype=torch.uint8, device='cuda')
    L = _lib.get()
    c_box, c_region = (ctypes.c_int * 9)(*box), (ctypes.c_int * 6)(*region)
    st = lambda t: [ctypes.c_longlong(v) for v in t.stride()]      # noqa: E731

    def tail():
        return (_lib.ptr(lvol), *st(lvol), *cvol.shape, c_box, _lib.ptr(d_knots), _lib.ptr(d_basis), _lib.ptr(d_cum), len(plan['knots']),
                ctypes.c_double(S.PLANE[0] / 2), ctypes.c_double(S.PLANE[1] / 2), _lib.ptr(tlab), S._DT[tlab.dtype], *st(tlab), *shape, c_region,
                S.RESTORE['crop'], int(vid), _lib.ptr(out[0]), *st(out[0]), _lib.ptr(out[1]), *st(out[1]), _lib.ptr(cov), *st(cov), None,
                (ctypes.c_double * 3)(*spacing), _lib.stream())

    def launch(cdll=None):
        args_ = (_lib.ptr(cvol), S._DT[cvol.dtype], *st(cvol)) + tail()
        if cdll is None:
            L.call('hv_restore_volume_sp', *args_)
        else:
            assert cdll.hv_restore_volume_sp(*args_) == 0

    launch()
    torch.cuda.synchronize()
    assert int(cov.sum()) == covered
    restore_ms = _timed(launch, args.reps)
    src_ct = torch.zeros(region[3], region[4], region[5], dtype=torch.float64, device='cuda')
    src_u8 = torch.zeros(2, region[3], region[4], region[5], dtype=torch.uint8, device='cuda')
    dst_ct, dst_u8 = torch.empty_like(src_ct), torch.empty_like(src_u8)

    def copy():
        dst_ct.copy_(src_ct)
        dst_u8.copy_(src_u8)

    copy()
    copy_ms = _timed(copy, args.reps)
    res = {'spacing': list(spacing), 'knots': len(plan['knots']), 'box': region, 'box_voxels': nvox, 'covered': covered, 'restore_ms': round(restore_ms, 4),
           'voxels_per_s': round(nvox / (restore_ms * 1e-3), 1), 'patient_ms': round(patient_ms, 4), 'copy_ms': round(copy_ms, 4)}
    if args.baseline_lib:
        B = ctypes.CDLL(args.baseline_lib)
        B.hv_restore_volume_sp.restype = ctypes.c_int
        B.hv_restore_volume_sp.argtypes = L.protos['hv_restore_volume_sp'][1]
        launch()
        ref_ct = out[0].clone()
        launch(B)
        torch.cuda.synchronize()
        assert torch.equal(out[0], ref_ct)
        for _ in range(2):                  # interleaved: this build, the baseline, this build, the baseline
            t_new, t_old = _times(launch, args.reps), _times(lambda: launch(B), args.reps)
        res.update(restore_ms=round(float(np.median(t_new)), 4), restore_ms_spread=round(max(t_new) - min(t_new), 4),
                   restore_ms_baseline=round(float(np.median(t_old)), 4), restore_ms_baseline_spread=round(max(t_old) - min(t_old), 4))
    if args.order == 3:
        sub = cvol[box[6]:box[6] + box[3], box[7]:box[7] + box[4], box[8]:box[8] + box[5]]
        coef = torch.empty(box[3], box[4], box[5], dtype=torch.float64, device='cuda')
        pre = lambda: L.call('hv_spline_prefilter', _lib.ptr(sub), S._DT[sub.dtype], *st(sub), box[3], box[4], box[5], 0, ctypes.c_double(0.0),  # noqa: E731
                             ctypes.c_double(1.0), _lib.ptr(coef), _lib.stream())
        res['sub_box'] = [int(v) for v in box[3:6]]
        res['prefilter_ms'] = round(_timed(pre, args.reps), 4)
        res['restore3_ms'] = round(_timed(lambda: L.call('hv_restore_volume_spline', _lib.ptr(coef), *tail()), args.reps), 4)
        res['patient3_ms'] = round(_timed(lambda: S.restore_patient(plan, crops, label=tlab, where='crop', return_covered=True, out=out, order=3),
                                          args.reps), 4)
    if not args.no_cpu:
        import restore_ref as R
        import spacing_ref as SR
        side = max(2, int(round(args.cpu_voxels ** (1 / 3))))
        sub = [region[i] + (region[3 + i] - side) // 2 for i in range(3)] + [min(side, region[3 + i]) for i in range(3)]
        t0 = time.perf_counter()
        loc = SR.local_coords(plan['knots'], plan['basis'], sub, spacing)
        c, cov = R.crop_coords(loc, box)
        from scipy.ndimage import map_coordinates
        cc, cl = crops[vid][0].cpu().numpy(), crops[vid][1].cpu().numpy()
        map_coordinates(cc, c[cov].T, order=1)
        map_coordinates(cl, c[cov].T, order=0)
        dt = time.perf_counter() - t0
        n_sub = int(np.prod(sub[3:]))
        res['cpu_ref_sub_voxels'] = n_sub
        res['cpu_ref_s_extrapolated'] = round(dt * nvox / n_sub, 1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
