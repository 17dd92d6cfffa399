"""Host curve math of the straightening stage (hvgan.straighten: curve extension, knots and frame, global_to_local, crop boxes, the
centroid drop rules) against the reference's own results on the synthetic patients of fixture G13 (tools/make_golden_straighten.py).
No device: these run everywhere."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12


def _g():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'g13_straighten.npz'))


def _cases(g):
    return sorted({k.split('/')[0] for k in g.files})


def _centroid_list(arr):
    return [{'label': int(r[0]), 'X': float(r[1]), 'Y': float(r[2]), 'Z': float(r[3])} for r in arr]


def _close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return np.all(np.abs(a - b) <= TOL * np.maximum(1.0, np.abs(b)))


def test_fixture_covers_the_reference_branches():
    g = _g()
    names = _cases(g)
    assert {'curved', 'bypass', 'single', 'edge'} <= set(names)
    assert not bool(g['bypass/window']) and bool(g['curved/window'])
    assert len(g['single/centroids']) == 1 and 'single/knots' not in g.files
    c = g['edge/curve']
    shape = g['edge/ct'].shape
    assert c[0][2] == 0.0 and c[-1][2] == shape[2]          # both extensions clamped, the upper one to shape_i itself


def test_curve_extension_knots_and_frame_match_reference():
    import hvgan  # noqa: F401
    from hvgan import straighten as S
    g = _g()
    for n in _cases(g):
        if n + '/knots' not in g.files:
            continue
        cents = _centroid_list(g[n + '/centroids'])
        coords = np.array([[e['X'], e['Y'], e['Z']] for e in cents])
        curve = S.extend_curve(coords, 20, (0, 0, 0), g[n + '/ct'].shape)
        assert _close(curve, g[n + '/curve']), n
        knots, basis = S.curve_frame(curve, 1)
        assert _close(knots, g[n + '/knots']), n
        assert _close(basis, g[n + '/basis']), n


def test_global_to_local_and_crop_boxes_match_reference():
    import hvgan  # noqa: F401
    from hvgan import straighten as S
    g = _g()
    for n in _cases(g):
        cents = _centroid_list(g[n + '/centroids'])
        ids = [int(v) for v in g[n + '/ids']]
        out_size = tuple(int(v) for v in g[n + '/out_size'])
        knots, basis, local, boxes = S.plan(cents, g[n + '/ct'].shape, ids, out_size)
        if n + '/local' in g.files:
            assert _close(np.stack([local[v] for v in ids]), g[n + '/local']), n
            src = (len(knots), 128, 128)
        else:
            assert knots is None
            src = g[n + '/ct'].shape
        # the boxes reproduce where the reference put the source in its zero volume: a crop voxel outside every box is 0 there
        for v, box, crop in zip(ids, boxes, g[n + '/crop_label']):
            lo, ln, st = box[0:3], box[3:6], box[6:9]
            assert all(0 <= lo[i] and lo[i] + ln[i] <= src[i] for i in range(3)), (n, v, box)
            inside = np.zeros(out_size, dtype=bool)
            inside[st[0]:st[0] + ln[0], st[1]:st[1] + ln[1], st[2]:st[2] + ln[2]] = True
            assert not crop[~inside].any(), (n, v)


def test_crop_box_is_extract_3d_volume_index_arithmetic():
    import hvgan  # noqa: F401
    from hvgan import straighten as S
    # int() truncation toward zero at c - d // 2 = -0.5, the clip at the volume's upper end, and an empty range
    assert S.crop_box((31.5, 100.2, 3.7), (64, 110, 40), (64, 32, 8)) == [0, 84, 0, 63, 26, 7, 0, 3, 0]
    lo0, lo1, lo2, n0, n1, n2, s0, s1, s2 = S.crop_box((200.0, 10.0, 5.0), (64, 64, 64), (16, 16, 4))
    assert n0 == 0 and (n1, n2) == (16, 4) and (s1, s2) == (0, 0)


def test_centroid_drop_rules():
    import hvgan  # noqa: F401
    from hvgan import straighten as S
    counts = np.zeros(256, np.int64)
    sums = np.zeros((256, 3), np.int64)
    for l, c in ((3, 5999), (4, 100), (7, 7999)):
        counts[l] = c
        sums[l] = (c * 2, c * 3 + 1, c * 5 + 2)
    assert [e['label'] for e in S.centroids_from_counts(counts, sums)] == [4]
    counts[3], counts[7] = 6000, 8000
    got = S.centroids_from_counts(counts, sums)
    assert [e['label'] for e in got] == [3, 4, 7]
    assert got[0]['Y'] == float(np.float64(3 * 5999 + 1) / np.float64(6000))
    lone = np.zeros(256, np.int64)
    lone[9] = 7999
    assert S.centroids_from_counts(lone, sums) == []            # a lone label is both the largest and the smallest


def test_plan_rejects_missing_ids_and_degenerate_curves():
    import hvgan  # noqa: F401
    from hvgan import straighten as S
    cents = [{'label': 1, 'X': 10.0, 'Y': 10.0, 'Z': 10.0}, {'label': 2, 'X': 10.0, 'Y': 12.0, 'Z': 30.0}]
    with pytest.raises(ValueError):
        S.plan(cents, (40, 40, 60), [5])
    with pytest.raises(ValueError):
        S.plan(cents + [dict(cents[1], label=3)], (40, 40, 60), [1])
    S.plan(cents, (40, 40, 60), [1, 2])
