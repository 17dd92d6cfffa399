"""De-pedicling of label crops: device (hvgan.straighten.depedicle, csrc/depedicle.hip) against the scipy path of
the reference's process_3d_array on the host and against a plain device copy of the same bytes.  One [256, 256, 64] uint8 crop and a batch of
13 (the crops of the patient of row f5), z-fastest as straighten_patient leaves them: a synthetic vertebra body per slice with a posterior
blob, bridged in every other slice, and two neighbouring vertebrae.  Launches back to back, timed with events.  Prints one JSON line:
  depedicle_us_1 / _13        hv_depedicle per call (out of place), one crop / the batch of 13
  counts_us_1 / _13           the counts-only form
  copy_us_1 / _13             torch's device copy of the same bytes (read once, written once)
  of_copy_1 / _13             copy time / de-pedicle time
  host_s_1                    transfer to the host, process_3d_array restated with scipy.ndimage.label, transfer back (one crop)

    timeout -k 10 300 python tools/bench_depedicle.py [--reps 20] [--no-cpu]
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
from hvgan import lib as _lib, straighten as S  # noqa: E402


def make_crop(seed):
    rng = np.random.default_rng(seed)
    vol = np.zeros((256, 256, 64), np.uint8)
    i0, i1 = np.mgrid[0:256, 0:256]
    for z in range(4, 60):
        r = 1.0 - ((z - 32) / 34.0) ** 2
        for k, lab in enumerate((17, 18, 19)):
            c0 = 48 + 80 * k + rng.integers(-2, 3)
            vol[:, :, z][((i0 - c0) / (30 * r)) ** 2 + ((i1 - 100) / (44 * r)) ** 2 <= 1.0] = lab
            vol[c0 - 8:c0 + 8, 160:200, z] = lab                     # the arch
            if z % 2 == 0:
                vol[c0 - 2:c0 + 2, 100:160, z] = lab                 # a pedicle joining it to the body
    return vol


def host_path(t):
    from scipy import ndimage
    t0 = time.perf_counter()
    arr = t.cpu().numpy()
    out = np.zeros_like(arr)
    for z in range(arr.shape[2]):                                    # process_layer (straighten_mask_3d.py:189-213)
        layer = arr[:, :, z]
        res = out[:, :, z]
        for lab in np.unique(layer):
            if lab == 0:
                continue
            labeled, n = ndimage.label(layer == lab)
            if n == 0:
                continue
            left = sorted((np.argwhere(labeled == f)[:, 1].min(), f) for f in range(1, n + 1))
            res[labeled == left[0][1]] = lab
    back = torch.from_numpy(out).to(t.device)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, back


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--no-cpu', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    L = _lib.get()
    res = {}
    crops = np.stack([make_crop(s) for s in range(13)])
    for V in (1, 13):
        vol = torch.from_numpy(crops[:V]).to(dev)
        out = torch.empty_like(vol)
        counts = torch.empty(V, 64, 256, dtype=torch.int32, device=dev)
        status = torch.empty(V, dtype=torch.int32, device=dev)
        sv, s0, s1, s2 = (ctypes.c_longlong(s) for s in vol.stride())

        def run(o):
            L.call('hv_depedicle', _lib.ptr(vol), 0, s0, s1, s2, sv, 256, 256, 64, V, _lib.ptr(o), s0, s1, s2, sv, _lib.ptr(counts),
                   _lib.ptr(status), _lib.stream())
        res['depedicle_us_%d' % V] = round(timed(lambda: run(out), args.reps), 1)
        res['counts_us_%d' % V] = round(timed(lambda: run(None), args.reps), 1)
        dst = torch.empty_like(vol)
        res['copy_us_%d' % V] = round(timed(lambda: dst.copy_(vol), args.reps), 1)
        res['of_copy_%d' % V] = round(res['copy_us_%d' % V] / res['depedicle_us_%d' % V], 4)
        assert int(status.abs().sum()) == 0
        assert torch.equal(S.depedicle(vol), out)
        if V == 1 and not args.no_cpu:
            secs, back = host_path(vol[0])
            assert torch.equal(back, out[0])
            res['host_s_1'] = round(secs, 3)
            res['changed_voxels_1'] = int((out[0] != vol[0]).sum())
    res['device'] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
