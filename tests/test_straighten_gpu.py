"""Device straightening (hvgan.straighten: csrc/straighten.hip) against the reference's own results on the synthetic patients of
fixture G13 (tools/make_golden_straighten.py), and a full-size patient against a host mirror (scipy's map_coordinates on the product's
fixture-pinned knots and frame).  Centroids are integer sums: bit-identical.  The straight CT differs from the reference's at most in the
summation order of doubles (1e-9 absolute); the uint8-truncated CT and the labels may differ only where a nearest sample is a tie."""
import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
CT_TOL = 1e-9
MISMATCH = 1e-5


def _g():
    g = load_golden('g13_straighten')
    cases = {}
    for k, v in g.items():
        a, b = k.split('/')
        cases.setdefault(a, {})[b] = v.numpy()
    return cases


def _centroid_list(arr):
    return [{'label': int(r[0]), 'X': float(r[1]), 'Y': float(r[2]), 'Z': float(r[3])} for r in arr]


def _check_crops(name, out, ids, ref_ct, ref_lab):
    for k, v in enumerate(ids):
        ct, lab = out[v]
        assert ct.dtype == torch.float64 and lab.dtype == torch.uint8 and ct.is_cuda
        ct, lab = ct.cpu().numpy(), lab.cpu().numpy()
        assert ct.shape == ref_ct[k].shape, (name, v, ct.shape)
        err = np.abs(ct - ref_ct[k]).max()
        assert err <= CT_TOL, (name, v, err)
        n = ct.size
        bad_ct = int((ct.astype(np.uint8) != ref_ct[k].astype(np.uint8)).sum())
        bad_lab = int((lab != ref_lab[k]).sum())
        assert bad_ct <= MISMATCH * n and bad_lab <= MISMATCH * n, (name, v, bad_ct, bad_lab)


def _run_case(c, ct, label, centroids=None):
    from hvgan import straighten as S
    ids = [int(v) for v in c['ids']]
    out = S.straighten_patient(ct, label, ids, centroids=centroids, out_size=tuple(int(s) for s in c['out_size']))
    torch.cuda.synchronize()
    return ids, out


def test_centroids_bit_identical_to_reference():
    import hvgan  # noqa: F401
    from hvgan import straighten as S
    for name, c in _g().items():
        got = S.vertebra_centroids(torch.from_numpy(c['label']).cuda())
        assert got == _centroid_list(c['centroids']), (name, got)
        got = S.vertebra_centroids(torch.from_numpy(np.asfortranarray(c['label']).astype(np.float64)).cuda())   # float64, Fortran order
        assert got == _centroid_list(c['centroids']), (name, 'f64 fortran')


def test_every_fixture_case_matches_reference():
    import hvgan  # noqa: F401
    for name, c in _g().items():
        ct, label = torch.from_numpy(c['ct']).cuda(), torch.from_numpy(c['label']).cuda()
        ids, out = _run_case(c, ct, label)
        _check_crops(name, out, ids, c['crop_ct'], c['crop_label'])
        # the same with the centroid list handed in (the JSON the reference reads)
        ids, out = _run_case(c, ct, label, centroids=_centroid_list(c['centroids']))
        _check_crops(name, out, ids, c['crop_ct'], c['crop_label'])


@pytest.mark.parametrize('variant', ['fortran', 'float32', 'float64', 'label_f64', 'fortran_f64_both'])
def test_input_layouts_and_dtypes(variant):
    import hvgan  # noqa: F401
    for name, c in _g().items():
        ct, label = c['ct'], c['label']
        if variant == 'fortran':
            ct, label = np.asfortranarray(ct), np.asfortranarray(label)
        elif variant == 'float32':
            ct = ct.astype(np.float32)
        elif variant == 'float64':
            ct = ct.astype(np.float64)
        elif variant == 'label_f64':
            label = label.astype(np.float64)
        else:
            ct, label = np.asfortranarray(ct.astype(np.float64)), np.asfortranarray(label.astype(np.float64))
        tct, tlab = torch.from_numpy(ct).cuda(), torch.from_numpy(label).cuda()
        if variant.startswith('fortran'):
            assert tct.stride()[0] == 1 and tlab.stride()[0] == 1
        ids, out = _run_case(c, tct, tlab)
        _check_crops(name + '/' + variant, out, ids, c['crop_ct'], c['crop_label'])


def test_bad_inputs_raise_and_a_following_call_succeeds():
    import hvgan  # noqa: F401
    from hvgan import straighten as S
    c = _g()['curved']
    ct, label = torch.from_numpy(c['ct']).cuda(), torch.from_numpy(c['label']).cuda()
    for bad in (label.to(torch.float64) + 0.5 * (label == 17).to(torch.float64), label.to(torch.int16) * 20, label.to(torch.int32) - 1):
        with pytest.raises(ValueError):
            S.straighten_patient(ct, bad, [17])
        with pytest.raises(ValueError):
            S.vertebra_centroids(bad)
    with pytest.raises(ValueError):
        S.straighten_patient(ct, label, [17, 42])                       # 42 has no centroid
    cents = _centroid_list(c['centroids'])
    with pytest.raises(ValueError):
        S.straighten_patient(ct, label, [17], centroids=cents[:1] + cents[:1] + cents[1:])   # two equal consecutive points
    ids, out = _run_case(c, ct, label)
    _check_crops('after errors', out, ids, c['crop_ct'], c['crop_label'])


def test_output_feeds_vertebra_volume():
    import hvgan  # noqa: F401
    from hvgan import batch_assembly
    c = _g()['curved']
    ids, out = _run_case(c, torch.from_numpy(c['ct']).cuda(), torch.from_numpy(c['label']).cuda())
    ct, lab = (t.cpu().numpy() for t in out[ids[0]])
    vv = batch_assembly.VertebraVolume(ct, lab, np.zeros(ct.shape), ids[0], [ids[1]])
    assert (vv.H, vv.W, vv.Z) == ct.shape
    assert np.array_equal(vv.ct, np.ascontiguousarray(np.moveaxis(ct.astype(np.uint8), 2, 0)))


def _mirror(ct, label, plan, out_size):
    """Host mirror of the device path from the product's plan (knots, frame, boxes -- pinned against the reference by
    tests/test_straighten_cpu.py): window, scipy map_coordinates, the split cleanup as the reference loops it, the crops."""
    from scipy.ndimage import map_coordinates
    knots, basis, boxes = plan['knots'], plan['basis'], plan['boxes']
    ctw = ct.astype(np.float64)
    if plan['window']:
        ctw = np.clip(255.0 * (ctw + 300.0) / 1100.0, 0, 255)
    a, b = np.meshgrid(np.arange(128) - 64.0, np.arange(128) - 64.0, indexing='ij')
    grid = np.stack([(basis[:, i, 1, None, None] * b + basis[:, i, 2, None, None] * a) + knots[:, i, None, None] for i in range(3)])
    sct = map_coordinates(ctw, grid, order=1, cval=0)
    slab = map_coordinates(label, grid, order=0, cval=0).astype(np.uint8)
    for l in np.unique(slab[slab != 0]):
        for h in range(64, 128):
            if l not in slab[:, h, 64]:
                sub = slab[:, h:, :]
                sub[sub == l] = 0
                break
    res = []
    for bx in boxes:
        lo, ln, st = bx[0:3], bx[3:6], bx[6:9]
        o, ol = np.zeros(out_size), np.zeros(out_size, np.uint8)
        o[st[0]:st[0] + ln[0], st[1]:st[1] + ln[1], st[2]:st[2] + ln[2]] = sct[lo[0]:lo[0] + ln[0], lo[1]:lo[1] + ln[1], lo[2]:lo[2] + ln[2]]
        ol[st[0]:st[0] + ln[0], st[1]:st[1] + ln[1], st[2]:st[2] + ln[2]] = slab[lo[0]:lo[0] + ln[0], lo[1]:lo[1] + ln[1], lo[2]:lo[2] + ln[2]]
        res.append((o, ol))
    return res


def test_full_size_patient_against_host_mirror():
    import hvgan  # noqa: F401
    from hvgan import straighten as S, synth
    ct, label = synth.make_spine_patient(seed=11, shape=(512, 512, 300), n_vert=10, radius=(40, 30, 11), end_radius=(14, 12, 6), margin=20,
                                         curve=(20.0, 40.0))
    nz = np.nonzero(label)
    ids_all = np.unique(label[nz])
    sums = {int(l): [int(ax[label[nz] == l].sum()) for ax in nz] for l in ids_all}
    counts = {int(l): int((label[nz] == l).sum()) for l in ids_all}
    tct, tlab = torch.from_numpy(ct).cuda(), torch.from_numpy(label).cuda()
    cents = S.vertebra_centroids(tlab)
    kept = [e['label'] for e in cents]
    assert kept == [int(l) for l in ids_all[1:-1]]                     # both small end vertebrae dropped
    for e in cents:
        assert [e['X'], e['Y'], e['Z']] == [np.float64(s) / np.float64(counts[e['label']]) for s in sums[e['label']]]
    ids = kept[::3]
    out, plan = S.straighten_patient(tct, tlab, ids, out_size=(256, 256, 64), return_plan=True)
    torch.cuda.synchronize()
    assert plan['window'] and plan['centroids'] == cents
    ref = _mirror(ct, label, plan, (256, 256, 64))
    _check_crops('full', out, ids, [r[0] for r in ref], [r[1] for r in ref])
