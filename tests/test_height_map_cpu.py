"""The height-loss map restatement (tests/height_map_ref.py) against the reference's own per-slice arrays (fixture G16, written by
tools/make_golden_height_map.py from the two RHLV scripts called on one-slice sub-volumes) and, reduced the scripts' way, against their
whole-volume outputs in G16, G8 (sagittal) and G15 (coronal), on the CPU.  Column counts and every original-vertebra height are integers:
exact.  The generated heights are one float64 product each, the means one numpy mean: 1e-12 relative, as everywhere for RHLV."""
import numpy as np

from conftest import load_golden
import height_map_ref as M

TOL = 1e-12
VIEWS = ('sagittal', 'coronal')


def _close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.all(np.abs(a - b) <= TOL * np.maximum(1.0, np.abs(b)))


def g16():
    g = {k: np.asarray(v) for k, v in load_golden('g16_height_map').items()}
    return g, sorted({k.split('/')[0] for k in g})


def g16_case(g, n, view):
    idx, div, thr = (float(v) for v in g[n + '/params'])
    return M.view_maps(g[n + '/fake'], g[n + '/label'], idx, int(div), thr, view)


def test_restatement_matches_the_reference_slice_by_slice():
    g, names = g16()
    assert len(names) >= 6
    rescaled = unscaled = skipped = raised = 0
    for n in names:
        for view in VIEWS:
            key = '%s/%s/' % (n, view)
            m = g16_case(g, n, view)
            lo, hi = (int(v) for v in g[key + 'range'][2:])
            assert m['range'] == (lo, hi), key
            values, offsets = g[key + 'values'], g[key + 'offsets']
            assert offsets.size == 8 * max(0, hi - lo) + 1
            for i, s in enumerate(range(lo, hi)):
                ref = [values[offsets[8 * i + k]:offsets[8 * i + k + 1]] for k in range(8)]
                visited = bool(m['flags'][s, 0] & M.VISITED)
                assert visited == (s in m['selected']) and np.all((m['flags'][s] & M.VISITED != 0) == visited)
                if g[key + 'raised'][i]:
                    raised += 1
                    assert visited and view == 'coronal' and m['raises'], (key, s)
                    continue
                if not visited:
                    skipped += 1
                    assert all(r.size == 0 for r in ref) and np.all(np.isnan(m['loss'][s])) and not m['flags'][s].any(), (key, s)
                    assert not m['height_fake'][s].any() and not m['height_label'][s].any()
                    continue
                got = m['selected'][s]
                for k in range(8):
                    if k % 2:
                        assert np.array_equal(got[k], ref[k]), (key, s, k)            # heights of the original: integers
                    else:
                        assert _close(got[k], ref[k]), (key, s, k, got[k], ref[k])
                # the map row is the whole-slice pair of arrays, spread over the columns they were selected from
                f = m['flags'][s]
                sel_f, sel_l = f & M.SEL_FAKE != 0, f & M.SEL_LABEL != 0
                assert _close(m['height_fake'][s][sel_f], ref[0]) and np.array_equal(m['height_label'][s][sel_l], ref[1]), (key, s)
                for region in range(3):
                    inside = f & M.REGION == region
                    assert (inside & sel_l).sum() == ref[3 + 2 * region].size, (key, s, region)
                    assert np.array_equal(m['height_label'][s][inside & sel_l], ref[3 + 2 * region]), (key, s, region)
                assert np.all(np.diff((f & M.REGION).astype(int)) >= 0)
                exact = np.array_equal(m['height_fake'][s], np.round(m['height_fake'][s]))
                rescaled += not exact
                unscaled += exact
                hf, hl = m['height_fake'][s], m['height_label'][s]
                assert np.array_equal(np.isnan(m['loss'][s]), ~sel_f)
                assert _close(m['loss'][s][sel_f], (hf[sel_f] - hl[sel_f]) / (hf[sel_f] + 1e-6))
            assert m['raises'] == bool(g[key + 'raises']), key
    assert rescaled and unscaled and skipped and raised, (rescaled, unscaled, skipped, raised)


def _check_reduction(m, out, means, what):
    res, mm = M.reduce_selected(m['selected'])
    assert _close(res, out), (what, res, out)
    assert _close(mm, means), (what, mm, means)
    # the identity that ties the map to the pinned numbers: its selected heights average to all_height_fake / all_height_label
    assert _close(M.selected_means(m), means[:2]), (what, M.selected_means(m), means[:2])


def test_reduced_the_scripts_way_the_restatement_gives_the_pinned_numbers():
    g, names = g16()
    checked = 0
    for n in names:
        for view in VIEWS:
            key = '%s/%s/' % (n, view)
            if g[key + 'raises']:
                continue
            _check_reduction(g16_case(g, n, view), g[key + 'out'], g[key + 'means'], key)
            checked += 1
    assert checked >= 11
    for fixture, view in (('g8_rhlv', 'sagittal'), ('g15_rhlv_coronal', 'coronal')):
        g = {k: np.asarray(v) for k, v in load_golden(fixture).items()}
        names = sorted({k.split('/')[0] for k in g} - {'narrow'})
        assert len(names) >= 6
        for n in names:
            idx, div, thr, centre, length = (float(v) for v in g[n + '/params'])
            m = M.view_maps(g[n + '/fake'], g[n + '/label'], idx, int(div), thr, view)
            assert m['range'] == slice(int(centre - length), int(centre + length)).indices(m['flags'].shape[0])[:2], (fixture, n)
            if n + '/raises' in g and g[n + '/raises']:
                assert m['raises'], (fixture, n)
                continue
            assert not m['raises']
            _check_reduction(m, g[n + '/out'], g[n + '/means'], (fixture, n))
            # the explicit centre / half-length form walks the same slices
            m2 = M.view_maps(g[n + '/fake'], g[n + '/label'], idx, 99, thr, view, centre_length=(int(centre), int(length)))
            assert np.array_equal(m2['flags'], m['flags']) and np.array_equal(m2['loss'], m['loss'], equal_nan=True)


def test_profiles_are_the_selected_heights_averaged_along_one_axis():
    g, names = g16()
    for n in names:
        for view in VIEWS:
            m = g16_case(g, n, view)
            sel_f, sel_l = m['flags'] & M.SEL_FAKE != 0, m['flags'] & M.SEL_LABEL != 0
            for axis, pre in ((0, ''), (1, 'slice_')):
                pf, pl, curve = m[pre + 'profile_fake'], m[pre + 'profile_label'], m[pre + 'curve']
                assert np.array_equal(np.isnan(pf), sel_f.sum(axis=axis) == 0) and np.array_equal(np.isnan(pl), sel_l.sum(axis=axis) == 0)
                assert np.array_equal(np.isnan(curve), np.isnan(pf) | np.isnan(pl))
                with np.errstate(invalid='ignore', divide='ignore'):
                    ref_f = np.where(sel_f, m['height_fake'], 0).sum(axis=axis) / sel_f.sum(axis=axis)
                    ref_l = np.where(sel_l, m['height_label'], 0).sum(axis=axis) / sel_l.sum(axis=axis)
                ok = ~np.isnan(pf)
                assert _close(pf[ok], ref_f[ok]) and _close(pl[~np.isnan(pl)], ref_l[~np.isnan(pl)])
                ok = ~np.isnan(curve)
                assert _close(curve[ok], (pf[ok] - pl[ok]) / (pf[ok] + 1e-6))
            # a slice nothing is selected from is not visited or has no selected column; the visited ones all have a slice profile of the original
            visited = m['flags'][:, 0] & M.VISITED != 0
            assert not np.any(~visited & ~np.isnan(m['slice_profile_label']))


def test_absent_vertebra_gives_none():
    g, names = g16()
    assert M.view_maps(g['plain/fake'], g['plain/label'], 33, 5, 0.64, 'sagittal') is None
    assert M.view_maps(g['plain/fake'], g['plain/label'], 33, 5, 0.64, 'coronal') is None
