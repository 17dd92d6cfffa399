"""The float64 restatement tests/gen_eval_ref.py reproduces what fixture G14 recorded from the reference's own process_images
(tools/make_golden_gen_eval.py): which cases raise, the evaluated slices, crop rows and data ranges in call order, and the seven outputs."""
import math

import numpy as np
import pytest

from conftest import load_golden
import gen_eval_ref as ref


def _cases():
    g = load_golden('g14_gen_eval')
    cases = {}
    for k, v in g.items():
        name, rest = k.split('/', 1)
        cases.setdefault(name, {})[rest] = v.numpy()
    return cases


CASES = _cases()


@pytest.mark.parametrize('view', ['sagittal', 'coronal'])
@pytest.mark.parametrize('name', sorted(CASES))
def test_restatement_reproduces_g14(name, view):
    c = CASES[name]
    args = (c['ori_ct'], c['fake_ct'], c['ori_seg'], c['fake_seg'], int(c['label']))
    calls = c[view + '/calls']
    rec = []
    if c[view + '/raises']:
        with pytest.raises(ValueError):
            ref.process_images(*args, view=view, record=rec)
        return
    out = ref.process_images(*args, view=view, record=rec)
    want = c[view + '/out']
    for a, b in zip(out, want):
        assert (math.isnan(a) and math.isnan(b)) or a == b, (out, want)
    n = len(rec)
    assert calls.shape == (4 * n, 8)
    patch, glob = calls[calls[:, 0] == 0], calls[calls[:, 0] == 1]
    for i, r in enumerate(rec):
        for rows, x1, R in ((patch, r['x1'], r['R_patch']), (glob, 0, r['R_global'])):
            for k in (0, 1):        # psnr then ssim
                row = rows[2 * i + k]
                assert row[1] == k and row[2] == r['z'] and row[3] == x1 and row[6] == R
        assert patch[2 * i, 4] == r['x2'] - r['x1'] + 1
    np.testing.assert_array_equal(c[view + '/overlap'], np.array(out)[[4, 6, 5]])


def test_g14_covers_the_edge_cases():
    """The fixture holds the cases the issue lists: an absent vertebra, a short patch, slices at exactly 400 voxels, flat crops."""
    assert CASES['absent']['sagittal/raises'] and CASES['absent']['coronal/raises']
    assert CASES['thin']['sagittal/raises'] and not CASES['thin']['coronal/raises']
    ori = CASES['exact400']['ori_seg'] == 20
    per_z = ori.sum(axis=(0, 1))
    assert (per_z == 400).sum() >= 4 and (per_z > 400).sum() >= 4
    assert set(CASES['exact400']['sagittal/calls'][:, 2].astype(int)) == set(np.flatnonzero(per_z > 400))
    assert np.isinf(CASES['identical']['sagittal/out'][0]) and CASES['flatall']['sagittal/out'][2] == 0
    assert (CASES['flat']['sagittal/calls'][:, 6] == 0).any()
