"""Pins tests/straighten_ref.py, the restatement the device tests of csrc/straighten.hip compare with (tests/test_straighten_kernels_gpu.py):
its sampler against scipy.ndimage.map_coordinates (order 1 and order 0, mode 'constant'), sampler + crop against the host mirror of
tests/test_straighten_gpu.py (window, scipy, the split cleanup as the reference loops it, the crops) on a small patient and a 24 x 20 plane,
and its stats against plain numpy and fixture G13's centroid list.  No device: these run everywhere."""
import os

import numpy as np

import spline_ref as P
import straighten_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# The one place where the kernel's trilinear weights are not scipy's bits: scipy takes the upper weight as 1 - (1 - t), the kernel as t
# (t = c - floor(c)).  For c >= 1 the two are equal (t is a multiple of 2^-52, so 1 - t is exact); for a coordinate inside the first cell,
# 0 < c < 1, they differ by at most 2^-53.  Three axes, windowed values of at most 255 and the roundings of the 8-term sum: 255 * 2^-50
# (2.3e-13) bounds the difference there; everywhere else the samples are equal.  Measured on the patient below: 4 of 24960 samples, 2.8e-14.
CT_FIRST_CELL = 255.0 * 2.0 ** -50


def _labels(shape, seed, top=6):
    return np.random.RandomState(seed).randint(0, top, size=shape).astype(np.uint8)


def _coords(shape, seed=3, n=4000):
    """[3, M]: random points reaching past every face, then per axis the hand-picked values 0, D - 1, D - 1 + 1e-7, -1e-9 and two half-integers
    beside an inside point on the other axes."""
    rng = np.random.RandomState(seed)
    pts = [rng.uniform(-1.5, shape[a] + 0.5, size=n) for a in range(3)]
    special = []
    for a in range(3):
        for x in (0.0, shape[a] - 1.0, shape[a] - 1.0 + 1e-7, -1e-9, 0.5, shape[a] - 1.5):
            for other in ((2.25, 3.5, 4.75), (0.0, 0.0, 0.0), (shape[0] - 1.0, shape[1] - 1.0, shape[2] - 1.0)):
                p = list(other)
                p[a] = x
                special.append(p)
    return np.concatenate([np.array(pts), np.array(special).T], axis=1)


def test_sample_points_is_map_coordinates_order_1_and_order_0():
    from scipy.ndimage import map_coordinates
    shape = (9, 11, 13)
    v, lab = P.case_volume(shape, 70), _labels(shape, 71)
    c = _coords(shape)
    for a in range(3):
        assert c[a].min() < 0.0 and c[a].max() > shape[a] - 1 and (c[a] == shape[a] - 1.0).any() and (c[a] == 0.0).any()
    tie = np.zeros(c.shape[1], dtype=bool)
    for a in range(3):
        tie |= (c[a] + 0.5) == np.floor(c[a] + 0.5)
    want_lab = map_coordinates(lab, c, order=0, mode='constant', cval=0)
    for win in (0, 1):
        got, got_lab = R.sample_points(v, lab, c, win, *P.WINDOW)
        want = map_coordinates(P.window(v) if win else v, c, order=1, mode='constant', cval=0.0)
        print('window', win, 'points', c.shape[1], 'max |restatement - scipy| %.3g' % np.abs(got - want).max(), 'label mismatches',
              int((got_lab != want_lab)[~tie].sum()), 'exact ties', int(tie.sum()), 'of which differ', int((got_lab != want_lab)[tie].sum()))
        assert (got == want).all()
        assert np.array_equal(got_lab[~tie], want_lab[~tie]) and tie.sum() > 0
    outside = (c < 0.0).any(0) | (c > np.array(shape, dtype=np.float64)[:, None] - 1.0).any(0)
    assert outside.sum() > 100 and (got[outside] == 0.0).all() and (got_lab[outside] == 0).all()
    # other CT dtypes are widened to double first: the same values give the same samples
    assert np.array_equal(R.sample_points(v.astype(np.int16), lab.astype(np.float32), c, 1, *P.WINDOW)[0], got)


def _mirror(ct, label, knots, basis, boxes, win, PA, PB, out_size):
    """_mirror of tests/test_straighten_gpu.py for a PA x PB plane."""
    from scipy.ndimage import map_coordinates
    ctw = ct.astype(np.float64)
    if win:
        ctw = np.clip(255.0 * (ctw + 300.0) / 1100.0, 0, 255)
    a, b = np.meshgrid(np.arange(PA) - PA / 2.0, np.arange(PB) - PB / 2.0, indexing='ij')
    grid = np.stack([(basis[:, i, 1, None, None] * b + basis[:, i, 2, None, None] * a) + knots[:, i, None, None] for i in range(3)])
    sct = map_coordinates(ctw, grid, order=1, cval=0)
    slab = map_coordinates(label, grid, order=0, cval=0).astype(np.uint8)
    before = slab.copy()
    for l in np.unique(slab[slab != 0]):
        for h in range(PA // 2, PA):
            if l not in slab[:, h, PB // 2]:
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
    return res, before, slab, sct


def test_sampler_and_crop_reproduce_the_host_mirror_with_its_split_cleanup():
    import hvgan  # noqa: F401
    from hvgan import straighten as S, synth
    ct, label = synth.make_spine_patient(seed=5, shape=(24, 30, 48), n_vert=4, first_id=16, radius=(5, 4, 4), end_radius=(4, 4, 3), margin=7,
                                         curve=(2.0, 3.0))
    st = R.stats_ref(ct, label)
    ids = [l for l in range(1, 256) if st['counts'][l]]
    cents = [{'label': l, 'X': float(st['sums'][l][0] / st['counts'][l]), 'Y': float(st['sums'][l][1] / st['counts'][l]),
              'Z': float(st['sums'][l][2] / st['counts'][l])} for l in ids]
    PA, PB, out_size = 24, 20, (12, 22, 18)
    knots, basis, _, boxes = S.plan(cents, ct.shape, ids, out_size, plane=(PB, PA))
    win = int(not (st['max'] < P.WINDOW[1] and st['min'] > P.WINDOW[0]))
    assert ids == [16, 17, 18, 19] and win == 1 and len(knots) > 20
    ref, before, after, ref_sct = _mirror(ct, label, knots, basis, boxes, win, PA, PB, out_size)
    sct, slab, pres = R.sample_ref(ct, label, knots, basis, PA, PB, (1.0, 1.0, 1.0), win, *P.WINDOW)
    assert np.array_equal(slab, before)
    grid = P.straight_grid(knots, basis, (1.0, 1.0, 1.0), plane=(PB, PA))
    low = ((grid > 0.0) & (grid < 1.0)).any(0)
    differ = sct != ref_sct
    print('straight CT: samples', sct.size, 'with a coordinate in (0, 1)', int(low.sum()), 'differing from scipy', int(differ.sum()),
          'max |diff| %.3g' % np.abs(sct - ref_sct).max())
    assert not differ[~low].any() and np.abs(sct - ref_sct).max() <= CT_FIRST_CELL
    got_ct, got_lab = R.crop_ref(sct, slab, PA, 0, *P.WINDOW, pres, boxes, out_size)
    cut = R.cutoffs(PA, pres)
    removed = int((before != after).sum())
    print('cutoffs', {l: int(cut[l]) for l in ids}, 'voxels the split cleanup removed', removed)
    assert removed > 0 and any(PA // 2 < cut[l] < PA for l in ids)       # the cleanup does something here, past the first row
    for k in range(len(ids)):
        assert np.abs(got_ct[k] - ref[k][0]).max() <= CT_FIRST_CELL and np.array_equal(got_lab[k], ref[k][1]), ids[k]
        assert got_lab[k].any()
    # the whole straight label volume under the cutoffs, not only the crops
    whole = [[0, 0, 0, len(knots), PA, PB, 0, 0, 0]]
    assert np.array_equal(R.crop_ref(sct, slab, PA, 0, *P.WINDOW, pres, whole, slab.shape)[1][0], after)


def test_cutoffs_at_the_word_edges():
    full = np.uint64(0xFFFFFFFFFFFFFFFF)
    pres = np.zeros((256, 2), dtype=np.uint64)
    pres[1] = (full, 1)                       # R = 65 bits set
    pres[2] = (full, 0)                       # first clear bit at h = 64
    pres[3] = (full >> np.uint64(1), full)    # first clear bit at h = 63, set bits after it
    pres[4] = (full << np.uint64(1), full)    # first clear bit at h = 0
    pres[5] = (full, full)                    # set bits at and past R
    cut = R.cutoffs(130, pres)
    assert [int(cut[l]) for l in range(6)] == [65, 130, 129, 128, 65, 130]
    assert int(R.cutoffs(128, pres[:, :1])[1]) == 128 and int(R.cutoffs(7, pres[:, :1])[4]) == 3 and int(R.cutoffs(7, pres[:, :1])[1]) == 7
    assert [R.rows_words(d) for d in (1, 2, 7, 128, 129, 131)] == [1, 1, 1, 1, 2, 2]
    # crop: the label at or past its cutoff goes, the CT stays, rows below D1 // 2 stay
    lab = np.full((2, 130, 3), 3, dtype=np.uint8)
    lab[:, :, 1] = 2
    ctv = np.arange(lab.size, dtype=np.float64).reshape(lab.shape)
    oc, ol = R.crop_ref(ctv, lab, 130, 0, 0.0, 1.0, pres, [[0, 0, 0, 2, 130, 3, 0, 0, 0]], lab.shape)
    assert np.array_equal(oc[0], ctv)
    want = lab.copy()
    want[:, 128:, 0] = want[:, 128:, 2] = 0
    want[:, 129:, 1] = 0
    assert np.array_equal(ol[0], want)


def test_stats_ref_is_plain_numpy_and_gives_the_fixture_centroids():
    import hvgan  # noqa: F401
    from hvgan import straighten as S
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'g13_straighten.npz'))
    label, ct = g['curved/label'], g['curved/ct']
    st = R.stats_ref(ct, label)
    want = [{'label': int(r[0]), 'X': float(r[1]), 'Y': float(r[2]), 'Z': float(r[3])} for r in g['curved/centroids']]
    assert S.centroids_from_counts(st['counts'], st['sums']) == want
    counts = np.bincount(label.ravel().astype(np.int64), minlength=256)
    counts[0] = 0
    assert np.array_equal(st['counts'], counts) and not st['bad'] and st['min'] == ct.min() and st['max'] == ct.max()
    for l in np.unique(label[label != 0]):
        nz = np.nonzero(label == l)
        assert [int(a.sum()) for a in nz] == [int(s) for s in st['sums'][l]]
    D0, D1, D2 = label.shape
    assert st['presence'].shape == (256, R.rows_words(D1)) and st['presence'].any()
    for l in range(256):
        for h in range(D1 - D1 // 2):
            bit = (int(st['presence'][l][h // 64]) >> (h % 64)) & 1
            assert bit == int(l != 0 and (label[:, D1 // 2 + h, D2 // 2] == l).any()), (l, h)
    # bad values count as 0 and raise the flag: floats that are no integers in [0, 255], NaN and inf among them
    small = _labels((4, 5, 6), 72).astype(np.float64)
    clean = R.stats_ref(None, small)
    assert clean['min'] is None and clean['max'] is None and not clean['bad']
    for bad in (256.0, -1.0, 0.5, np.nan, np.inf):
        v = small.copy()
        was = int(v[3, 4, 5])
        v[3, 4, 5] = bad
        got = R.stats_ref(None, v)
        counts = clean['counts'].copy()
        if was:
            counts[was] -= 1
        assert got['bad'] and np.array_equal(got['counts'], counts)


def test_decode_stats_reads_the_record_layout():
    import hvgan  # noqa: F401
    from hvgan import straighten as S
    assert (R.HDR, R.CNT, R.SUM, R.PRES) == (S._HDR, S._CNT, S._SUM, S._PRES)
    D1 = 129
    w = np.zeros(R.PRES + 256 * 2, dtype=np.uint64)
    bits = lambda x: int(np.array([x], dtype=np.float64).view(np.uint64)[0])   # noqa: E731
    w[0] = np.uint64(bits(-2.5))                          # ~key(min): the key of a negative value is all its bits flipped
    w[1] = np.uint64(bits(7.25) | (1 << 63))              # key(max): a non-negative value gets its sign bit set
    w[2], w[3] = 1, 0
    w[R.CNT + 9], w[R.SUM + 27:R.SUM + 30] = 4, (1, 2, 3)
    w[R.PRES + 2 * 9 + 1] = 5
    d = R.decode_stats(w, D1)
    assert (d['min'], d['max'], d['bad'], d['word3']) == (-2.5, 7.25, True, 0)
    assert d['counts'][9] == 4 and list(d['sums'][9]) == [1, 2, 3] and d['presence'][9][1] == 5 and d['presence'].sum() == 5
