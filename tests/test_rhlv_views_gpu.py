"""Coronal and 2.5D RHLV on the device (hv_rhlv_views / hv_rhlv_views_batch through hvgan.evaluation) against the reference's coronal
outputs (fixture G15) and the float64 restatement tests/rhlv_coronal_ref.py.  Integer steps (column counts, thirds, centre columns,
selections) are exact; the final means differ from numpy's only in the summation grouping of doubles: tolerance 1e-12 relative with a
floor of 1, as in tests/test_rhlv_gpu.py.  The one-pass and batched forms run the kernels of the single-view calls: bit for bit equal."""
import functools
import inspect

import numpy as np
import pytest
import torch

from conftest import load_golden
import rhlv_coronal_ref as C

pytestmark = pytest.mark.gpu
TOL = 1e-12


def _close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.all(np.abs(a - b) <= TOL * np.maximum(1.0, np.abs(b)))


@functools.lru_cache(maxsize=None)
def _golden():
    g = {k: np.asarray(v) for k, v in load_golden('g15_rhlv_coronal').items()}
    return g, sorted({k.split('/')[0] for k in g} - {'narrow'})


def _random_kw(seed):
    return dict(seed=300 + seed, H=40 + 8 * (seed % 3), W=48 + 16 * (seed // 2 % 2), Z=16 + seed, collapse=0.1 * (seed % 5), fake_shorter=seed % 4 == 3)


@functools.lru_cache(maxsize=None)
def _random_case(seed):
    """-> (generated, original, length_divisor, height_threshold, the restatement's (results, means) or 'raises')."""
    from hvgan import synth
    fake, label = synth.make_rhlv_pair(**_random_kw(seed))
    div, thr = 3 + seed % 3, 0.5 + 0.05 * seed
    try:
        ref = C.rhlv_volume(fake, label, 20, div, thr)
    except ValueError:
        ref = 'raises'
    return fake, label, div, thr, ref


def _zslowest(t):
    """The same [H, W, Z] values stored as [Z, H, W]."""
    return t.permute(2, 0, 1).contiguous().permute(1, 2, 0)


def test_coronal_matches_reference_golden():
    import hvgan  # noqa: F401
    from hvgan import evaluation
    g, names = _golden()
    for n in names:
        idx, div, thr, center, length = (float(v) for v in g[n + '/params'])
        fake, label = torch.from_numpy(g[n + '/fake']).cuda(), torch.from_numpy(g[n + '/label']).cuda()      # uint8 id volumes, [H, W, Z]
        binary = [((fake == idx).float(), (label == idx).float())]                                         # z fastest
        binary.append(tuple(_zslowest(t) for t in binary[0]))
        assert binary[0][0].stride(2) == 1 and binary[1][0].stride(2) > binary[1][0].stride(0)
        if g[n + '/raises']:
            with pytest.raises(ValueError):
                evaluation.rhlv_volume(fake, label, idx, int(div), thr, view='coronal')
            for sf, sl in binary:
                with pytest.raises(ValueError):
                    evaluation.calculate_rhlv(sf, sl, int(center), int(length), 'v', thr, view='coronal')
            continue
        res, means = evaluation.rhlv_volume(fake, label, idx, int(div), thr, return_means=True, view='coronal')
        assert _close(res, g[n + '/out']), (n, res, g[n + '/out'])
        assert _close(means, g[n + '/means']), (n, means, g[n + '/means'])
        assert (res, means) == evaluation.rhlv_volume(_zslowest(fake), _zslowest(label), idx, int(div), thr, return_means=True, view='coronal')
        for sf, sl in binary:
            res2 = evaluation.calculate_rhlv(sf, sl, int(center), int(length), 'v', thr, view='coronal')
            assert _close(res2, g[n + '/out']), (n, sf.stride(), res2)
            res3, means3 = evaluation.rhlv_volume(sf * idx, sl * idx, idx, int(div), thr, return_means=True, view='coronal')
            assert _close(res3, g[n + '/out']) and _close(means3, g[n + '/means']), (n, sf.stride(), res3)


def test_coronal_random_pairs_match_restatement():
    import hvgan  # noqa: F401
    from hvgan import evaluation
    shapes = {(_random_kw(s)['W'], _random_kw(s)['Z']) for s in range(8)}
    assert any(w % 64 and z % 2 for w, z in shapes)
    compared = 0
    for seed in range(8):
        fake, label, div, thr, ref = _random_case(seed)
        f, l = torch.from_numpy(fake).float().cuda(), torch.from_numpy(label).float().cuda()
        if ref == 'raises':
            with pytest.raises(ValueError):
                evaluation.rhlv_volume(f, l, 20, div, thr, view='coronal')
            continue
        got, gm = evaluation.rhlv_volume(f, l, 20, div, thr, return_means=True, view='coronal')
        assert _close(got, ref[0]) and _close(gm, ref[1]), (seed, got, ref)
        compared += 1
    assert compared >= 6
    # the original volume does not contain the vertebra: the reference skips it
    assert evaluation.rhlv_volume(f, l, 33, view='coronal') is None and C.rhlv_volume(fake, label, 33) is None
    # generated volume empty: every slice is skipped, all means are zero
    res = evaluation.rhlv_volume(torch.zeros_like(f), l, 20, view='coronal')
    assert _close(res, C.rhlv_volume(np.zeros_like(fake), label, 20)[0])


def test_coronal_raises_where_the_reference_raises():
    import hvgan  # noqa: F401
    from hvgan import evaluation
    g, _ = _golden()
    # one-slice volumes, the generated vertebra on columns [y_min, y_min + y_range]: the reference's own table of which extents it refuses
    for (y_min, y_range, raised), fake, label in zip(g['narrow/table'], g['narrow/fake'], g['narrow/label']):
        f, l = torch.from_numpy(fake).cuda(), torch.from_numpy(label).cuda()
        if raised:
            with pytest.raises(ValueError):
                evaluation.calculate_rhlv(f, l, 1, 1, 'v', 0.64, view='coronal')
        else:
            got = evaluation.calculate_rhlv(f, l, 1, 1, 'v', 0.64, view='coronal')
            assert _close(got, C.rhlv(fake.astype(np.float64), label.astype(np.float64), 1, 1, 0.64)[0]), (y_min, y_range, got)
        # the sagittal script guards its thirds with .size > 0: the same table walked by the sagittal arithmetic never raises
        evaluation.calculate_rhlv(f.permute(0, 2, 1), l.permute(0, 2, 1), 1, 1, 'v', 0.64)
    # a whole vertebra: the 2.5D call raises for its coronal half, the dataset call records the flag instead
    fake, label = torch.from_numpy(g['two_columns/fake']).cuda(), torch.from_numpy(g['two_columns/label']).cuda()
    with pytest.raises(ValueError):
        evaluation.rhlv_volume_25d(fake, label, 20)
    rec, present = evaluation.rhlv_dataset([fake], [label], [20])
    assert present[0] and rec[0, 1, 14] == 1.0 and rec[0, 0, 14] == 0.0


class _CountedCpu:
    """Counts Tensor.cpu() calls: every readback of these entry points is one."""
    def __enter__(self):
        self.n, self.orig = 0, torch.Tensor.cpu

        def cpu(t, *a, **kw):
            self.n += 1
            return self.orig(t, *a, **kw)
        torch.Tensor.cpu = cpu
        return self

    def __exit__(self, *exc):
        torch.Tensor.cpu = self.orig


def test_one_pass_and_batched_forms_are_bit_identical_with_one_readback():
    import hvgan  # noqa: F401
    from hvgan import evaluation, synth
    pairs = [synth.make_rhlv_pair(seed=400 + i, H=48, W=48, Z=17, collapse=0.15 * i, fake_shorter=i == 1) for i in range(5)]
    fakes = [torch.from_numpy(f.astype(np.uint8)).cuda() for f, _ in pairs]
    labels = [torch.from_numpy(l.astype(np.uint8)).cuda() for _, l in pairs]
    ids = [20, 20, 33, 20, 20]                  # pair 2: the original lacks vertebra 33
    fakes[3] = torch.zeros_like(fakes[3])       # pair 3: empty generated volume
    thr = (0.64, 0.7)
    singles = []
    for f, l, i in zip(fakes, labels, ids):
        with _CountedCpu() as c:
            both = evaluation.rhlv_volume_25d(f, l, i, 4, thr, return_means=True)
        assert c.n == 1
        singles.append(both)
        if i == 33:
            assert both is None and evaluation.rhlv_volume(f, l, i, 4, thr[0]) is None
            continue
        assert both['sagittal'] == evaluation.rhlv_volume(f, l, i, 4, thr[0], return_means=True)
        assert both['coronal'] == evaluation.rhlv_volume(f, l, i, 4, thr[1], return_means=True, view='coronal')
    assert singles[0]['sagittal'] != singles[0]['coronal']
    with _CountedCpu() as c:
        rec, present = evaluation.rhlv_dataset(fakes, labels, ids, 4, thr)
    assert c.n == 1
    assert rec.shape == (5, 2, 16) and rec.dtype == np.float64 and list(present) == [True, True, False, True, True]
    for k, both in enumerate(singles):
        if both is None:
            continue
        for v, view in enumerate(('sagittal', 'coronal')):
            assert tuple(rec[k, v, :5]) == both[view][0] and list(rec[k, v, 5:13]) == both[view][1], (k, view)
            assert rec[k, v, 14] == 0.0 and rec[k, v, 15] == 0.0
    assert np.all(rec[3, :, 5:13:2] == 0.0)     # nothing generated: no generated height selected
    # chunked launches write the same records
    rec2, _ = evaluation.rhlv_dataset(fakes, labels, ids, 4, thr, chunk=2)
    assert np.array_equal(rec, rec2)
    # the six SVM features: file1's Pre / Mid / Post, then the other view's
    feats = evaluation.svm_features(rec)
    assert feats.shape == (5, 6) and np.array_equal(feats[:, :3], rec[:, 0, 1:4]) and np.array_equal(feats[:, 3:], rec[:, 1, 1:4])
    assert np.array_equal(evaluation.svm_features(rec, file1='coronal'), feats[:, [3, 4, 5, 0, 1, 2]])


def test_default_view_is_the_sagittal_entry_unchanged():
    import hvgan  # noqa: F401
    from hvgan import evaluation, synth
    from oracle import restate as R
    assert inspect.signature(evaluation.rhlv_volume).parameters['view'].default == 'sagittal'
    assert inspect.signature(evaluation.calculate_rhlv).parameters['view'].default == 'sagittal'
    fake, label = synth.make_rhlv_pair(seed=9, H=48, W=80, Z=18, fake_shorter=True)
    f, l = torch.from_numpy(fake).float().cuda(), torch.from_numpy(label).float().cuda()
    raw = evaluation._run(f, l, 20.0, 5, evaluation.INT_MIN, 0, 0.64).cpu()          # hv_rhlv itself
    assert raw.shape == (14,)
    res, means = evaluation.rhlv_volume(f, l, 20, return_means=True)
    assert res == tuple(float(v) for v in raw[:5]) and means == [float(v) for v in raw[5:13]]
    assert res == evaluation.rhlv_volume(f, l, 20, view='sagittal')
    ref, ref_means = R.rhlv_volume(fake, label, 20)
    assert _close(res, ref) and _close(means, ref_means)
    sf, sl = (f == 20).float(), (l == 20).float()
    raw = evaluation._run(sf, sl, -1.0, 1, 5, 13, 0.64).cpu()
    assert evaluation.calculate_rhlv(sf, sl, 9, 4, 'v', 0.64) == tuple(float(v) for v in raw[:5])
    assert _close(raw[:5], R.rhlv(sf.cpu().numpy().astype(np.float64), sl.cpu().numpy().astype(np.float64), 9, 4, 0.64)[0])
