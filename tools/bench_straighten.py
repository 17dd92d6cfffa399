"""Straightening of one full-size patient: device (hvgan.straighten, volumes resident in HBM) vs the host
mirror of the reference's numpy / scipy path.  Synthetic 512 x 512 x 400 int16 CT with a 15-vertebra uint8 label, the reference's
parameters (plane 128 x 128, out_size (256, 256, 64), every kept vertebra requested).  Prints one JSON line:
  stats_ms / stats_GBps / stats_of_copy   the stats pass (both volumes read once) against the 5.1 TB/s copy rate of tools/hbm_rw_probe.py
  sample_ms / samples_per_s               the sampler (N x 128 x 128 straight samples, CT and label)
  crop_ms                                 the crop launch (all vertebrae)
  patient_ms                              straighten_patient end to end (stats, read back, host curve math, sample, crop), median
  h2d_ct_ms / h2d_label_ms                upload of the two volumes from pageable host memory
  cpu_mirror_s                            the same patient on the host: centroids per label (np.where), window, map_coordinates x 2,
                                          split cleanup, crops

  --order 3 adds: prefilter_ms (hv_spline_prefilter of the whole scan, window fused, its up to three launches together; per axis:
                  rocprofv3 --kernel-trace --stats lists spline_axis_kernel<true> (axis 0), <false> (axis 1) and spline_axis2_kernel),
                  coef_MB / coef_copy_ms (a plain device copy of the coefficient volume's bytes), sample3_ms (hv_straighten_sample_spline),
                  patient3_ms (straighten_patient(order=3) end to end)
  --baseline-lib PATH adds: sample_ms_baseline, the order-1 sampler of another build of the library (the parent commit's) loaded beside
                  this one, timed in the same process, and sample_ms_spread / sample_ms_baseline_spread (max - min over the repeats)

    timeout -k 10 600 python tools/bench_straighten.py [--reps 10] [--no-cpu] [--spacing a,b,c] [--order 3] [--baseline-lib libhvgan_parent.so]
--spacing: millimetres per voxel of the same 512 x 512 x 400 voxel patient (default 1,1,1); the host mirror is skipped at other spacings.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hvgan  # noqa: E402,F401
from hvgan import lib as _lib, straighten as S, synth  # noqa: E402

COPY_TBPS = 5.1


def _ev():
    return torch.cuda.Event(enable_timing=True)


def _times(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = _ev(), _ev()
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


def _timed(fn, reps):
    return float(np.median(_times(fn, reps)))


def cpu_mirror(ct, label, ids, out_size=(256, 256, 64)):
    from scipy.ndimage import map_coordinates
    t0 = time.perf_counter()
    lab8 = label.astype(np.uint8)
    labels = [l for l in np.unique(lab8) if l != 0]
    cents = []
    for l in labels:                       # location_json_local.py:37-45
        n = np.sum(lab8 == l)
        if (n < 8000 and l == max(labels)) or (n < 6000 and l == min(labels)):
            continue
        c = np.mean(np.where(lab8 == l), axis=1)
        cents.append({'label': int(l), 'X': c[0], 'Y': c[1], 'Z': c[2]})
    knots, basis, local, boxes = S.plan(cents, ct.shape, ids, out_size)
    ctw = ct.astype(np.float64)
    if not (ctw.max() < 800 and ctw.min() > -300):
        ctw = np.clip(255.0 * (ctw + 300) / 1100, 0, 255)
    a, b = np.meshgrid(np.arange(128) - 64.0, np.arange(128) - 64.0, indexing='ij')
    grid = np.stack([(basis[:, i, 1, None, None] * b + basis[:, i, 2, None, None] * a) + knots[:, i, None, None] for i in range(3)])
    sct = map_coordinates(ctw, grid, order=1, cval=0)
    slab = map_coordinates(label.astype(np.float64), grid, order=0, cval=0)
    for l in np.unique(slab[slab != 0]):
        for h in range(64, 128):
            if l not in slab[:, h, 64]:
                sub = slab[:, h:, :]
                sub[sub == l] = 0
                break
    for bx in boxes:
        lo, ln, st = bx[0:3], bx[3:6], bx[6:9]
        o = np.zeros(out_size)
        o[st[0]:st[0] + ln[0], st[1]:st[1] + ln[1], st[2]:st[2] + ln[2]] = sct[lo[0]:lo[0] + ln[0], lo[1]:lo[1] + ln[1], lo[2]:lo[2] + ln[2]]
        ol = np.zeros(out_size)
        ol[st[0]:st[0] + ln[0], st[1]:st[1] + ln[1], st[2]:st[2] + ln[2]] = slab[lo[0]:lo[0] + ln[0], lo[1]:lo[1] + ln[1], lo[2]:lo[2] + ln[2]]
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--no-cpu', action='store_true')
    ap.add_argument('--spacing', default='1,1,1')
    ap.add_argument('--order', type=int, default=1, choices=(1, 3))
    ap.add_argument('--baseline-lib', default=None)
    args = ap.parse_args()
    spacing = S.check_spacing([float(v) for v in args.spacing.split(',')])
    c_spacing = (ctypes.c_double * 3)(*spacing)
    shape = (512, 512, 400)
    ct, label = synth.make_spine_patient(seed=5, shape=shape, n_vert=15, radius=(40, 30, 10), end_radius=(14, 12, 6), margin=16,
                                         curve=(20.0, 40.0))
    dev = torch.device('cuda:0')
    torch.zeros(1, device=dev)
    h2d_ct = _timed(lambda: torch.from_numpy(ct).to(dev), 3)
    h2d_lab = _timed(lambda: torch.from_numpy(label).to(dev), 3)
    tct, tlab = torch.from_numpy(ct).to(dev), torch.from_numpy(label).to(dev)
    L = _lib.get()
    st = lambda t: [ctypes.c_longlong(s) for s in t.stride()]     # noqa: E731
    X, Y, Z = shape
    nbytes = L.size('hv_straighten_stats_bytes', Y)
    rec = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
    stats = lambda: L.call('hv_straighten_stats', _lib.ptr(tct), 1, *st(tct), _lib.ptr(tlab), 0, *st(tlab), X, Y, Z, _lib.ptr(rec),  # noqa: E731
                           ctypes.c_size_t(nbytes), _lib.stream())
    stats_ms = _timed(stats, args.reps)
    cents = S.vertebra_centroids(tlab)
    ids = [e['label'] for e in cents]
    out, plan = S.straighten_patient(tct, tlab, ids, return_plan=True, spacing=spacing)
    knots, basis, boxes = plan['knots'], plan['basis'], plan['boxes']
    N = len(knots)
    d_knots, d_basis = torch.from_numpy(knots).to(dev), torch.from_numpy(basis).to(dev)
    sct = torch.empty(N, 128, 128, dtype=torch.float64, device=dev)
    slab = torch.empty(N, 128, 128, dtype=torch.uint8, device=dev)
    pbytes = L.size('hv_straighten_presence_bytes', 128)
    pres = torch.empty(pbytes // 8, dtype=torch.int64, device=dev)
    wmin, wmax = ctypes.c_double(-300.0), ctypes.c_double(800.0)
    sample = lambda: L.call('hv_straighten_sample_sp', _lib.ptr(tct), 1, *st(tct), _lib.ptr(tlab), 0, *st(tlab), X, Y, Z, _lib.ptr(d_knots),  # noqa: E731
                            _lib.ptr(d_basis), N, 128, 128, int(plan['window']), wmin, wmax, _lib.ptr(sct), _lib.ptr(slab), _lib.ptr(pres),
                            ctypes.c_size_t(pbytes), c_spacing, _lib.stream())
    sample_ms = _timed(sample, args.reps)
    V = len(ids)
    d_boxes = torch.tensor(boxes, dtype=torch.int32).to(dev)
    ct_out = torch.empty(V, 256, 256, 64, dtype=torch.float64, device=dev)
    lab_out = torch.empty(V, 256, 256, 64, dtype=torch.uint8, device=dev)
    crop = lambda: L.call('hv_straighten_crop', _lib.ptr(sct), 5, *st(sct), _lib.ptr(slab), 0, *st(slab), 128, 0, wmin, wmax,  # noqa: E731
                          _lib.ptr(pres), _lib.ptr(d_boxes), V, 256, 256, 64, _lib.ptr(ct_out), _lib.ptr(lab_out), _lib.stream())
    crop_ms = _timed(crop, args.reps)
    assert torch.equal(ct_out, torch.stack([out[v][0] for v in ids])) and torch.equal(lab_out, torch.stack([out[v][1] for v in ids]))
    patient_ms = _timed(lambda: S.straighten_patient(tct, tlab, ids, spacing=spacing), args.reps)
    read = ct.nbytes + label.nbytes
    res = {'shape': list(shape), 'spacing': list(spacing), 'vertebrae': V, 'planes': N, 'stats_ms': round(stats_ms, 4),
           'stats_GBps': round(read / stats_ms / 1e6, 1), 'stats_of_copy': round(read / stats_ms / 1e9 / COPY_TBPS, 3),
           'sample_ms': round(sample_ms, 4), 'samples_per_s': float('%.4g' % (N * 128 * 128 / sample_ms * 1e3)), 'crop_ms': round(crop_ms, 4),
           'crop_out_MB': round(V * 256 * 256 * 64 * 9 / 1e6, 1), 'patient_ms': round(patient_ms, 3), 'h2d_ct_ms': round(h2d_ct, 3),
           'h2d_label_ms': round(h2d_lab, 3)}
    if args.baseline_lib:
        B = ctypes.CDLL(args.baseline_lib)
        B.hv_straighten_sample_sp.restype = ctypes.c_int
        B.hv_straighten_sample_sp.argtypes = L.protos['hv_straighten_sample_sp'][1]
        sct_b = torch.empty_like(sct)
        base = lambda: B.hv_straighten_sample_sp(_lib.ptr(tct), 1, *st(tct), _lib.ptr(tlab), 0, *st(tlab), X, Y, Z, _lib.ptr(d_knots),  # noqa: E731
                                                 _lib.ptr(d_basis), N, 128, 128, int(plan['window']), wmin, wmax, _lib.ptr(sct_b), _lib.ptr(slab),
                                                 _lib.ptr(pres), ctypes.c_size_t(pbytes), c_spacing, _lib.stream())
        assert base() == 0
        sample()
        torch.cuda.synchronize()
        assert torch.equal(sct, sct_b)
        for _ in range(2):                  # interleaved: this build, the baseline, this build, the baseline
            t_new, t_old = _times(sample, args.reps), _times(base, args.reps)
        res.update(sample_ms=round(float(np.median(t_new)), 4), sample_ms_spread=round(max(t_new) - min(t_new), 4),
                   sample_ms_baseline=round(float(np.median(t_old)), 4), sample_ms_baseline_spread=round(max(t_old) - min(t_old), 4))
    if args.order == 3:
        win = int(plan['window'])
        coef = torch.empty(X, Y, Z, dtype=torch.float64, device=dev)
        pre = lambda: L.call('hv_spline_prefilter', _lib.ptr(tct), 1, *st(tct), X, Y, Z, win, wmin, wmax, _lib.ptr(coef), _lib.stream())  # noqa: E731
        res['prefilter_ms'] = round(_timed(pre, args.reps), 4)
        res['coef_MB'] = round(coef.numel() * 8 / 1e6, 1)
        dst = torch.empty_like(coef)
        res['coef_copy_ms'] = round(_timed(lambda: dst.copy_(coef), args.reps), 4)
        del dst
        smp3 = lambda: L.call('hv_straighten_sample_spline', _lib.ptr(coef), _lib.ptr(tlab), 0, *st(tlab), X, Y, Z, _lib.ptr(d_knots),  # noqa: E731
                              _lib.ptr(d_basis), N, 128, 128, _lib.ptr(sct), _lib.ptr(slab), _lib.ptr(pres), ctypes.c_size_t(pbytes), c_spacing,
                              _lib.stream())
        res['sample3_ms'] = round(_timed(smp3, args.reps), 4)
        del coef
        res['patient3_ms'] = round(_timed(lambda: S.straighten_patient(tct, tlab, ids, spacing=spacing, order=3), args.reps), 3)
    if not args.no_cpu and spacing == (1.0, 1.0, 1.0):
        res['cpu_mirror_s'] = round(cpu_mirror(ct, label, ids), 3)
    res['device'] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
