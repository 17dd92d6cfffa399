"""float64 numpy restatement of the per-column height-loss maps and profiles (include/hvgan.h, hv_rhlv_maps), from
the lines of the reference's evaluation/RHLV_quantification.py and evaluation/RHLV_quantification_coronal.py (:41-147 and the per-vertebra body of
process_datasets_to_excel): the CPU side of tests/test_height_map_gpu.py, itself checked against the reference's own per-slice arrays and
whole-volume outputs (fixtures G16, G8, G15) by tests/test_height_map_cpu.py.

A view walks slices s with columns c: 'sagittal' = slices along axis 2 with columns along axis 1 and the sagittal script's ratio
label.max() / (fake.max() + 1e-6) behind .size > 0 guards; 'coronal' = slices along axis 1 with columns along axis 2 and the coronal script's
label.max() / fake.max(), which raises ValueError (max() of an empty array) where a third of columns is empty.  A raising slice still has a
map row -- the whole-slice quantities are defined -- and is reported by `raises`.
"""
import numpy as np

REGION, SEL_FAKE, SEL_LABEL, VISITED = 3, 4, 8, 16       # bits of a flags element


def column_table(vol, label_index, view):
    """Id volume [H, W, Z] -> int64 cnt[s][c], the vertebra's voxels per column of every slice of the view."""
    cnt = (np.asarray(vol) == label_index).sum(axis=0).astype(np.int64)          # [W][Z]
    return cnt.T.copy() if view == 'sagittal' else cnt


def _centre_height(cols):
    """Height at the column int(mean of the column index over the voxels)."""
    return int(cols[int((cols * np.arange(cols.size)).sum() / cols.sum())])


def slice_state(cf, cl, height_threshold, view):
    """Column counts of a visited slice -> (t1, t2, the four ratios all / pre / mid / post, the two selection thresholds, raises)."""
    idx = np.flatnonzero(cf)
    y_min, y_range = int(idx[0]), int(idx[-1]) - int(idx[0])
    t1, t2 = int(y_min + y_range / 3), int(y_min + 2 * y_range / 3)
    ratios, raises = [], False
    for p in (slice(None), slice(None, t1), slice(t1, t2), slice(t2, None)):
        if cf[p].size == 0:                      # sagittal: guarded, ratio 1; coronal: max() of an empty array
            raises = raises or view == 'coronal'
            ratios.append(np.float64(1.0))
            continue
        mf, ml = np.float64(cf[p].max()), np.float64(cl[p].max())
        with np.errstate(divide='ignore'):
            ratios.append((ml / mf if view == 'coronal' else ml / (mf + 1e-6)) if ml > mf else np.float64(1.0))
    thr_f = (_centre_height(cf) * ratios[0]) * height_threshold
    thr_l = _centre_height(cl) * height_threshold
    return t1, t2, ratios, thr_f, thr_l, raises


def selected_heights(cf, cl, state):
    """The eight arrays calculate_heights appends for one slice: all / pre / mid / post x generated / original, in column order."""
    t1, t2, ratios, thr_f, thr_l, _ = state
    out = []
    for r, p in zip(ratios, (slice(None), slice(None, t1), slice(t1, t2), slice(t2, None))):
        with np.errstate(invalid='ignore'):
            hf = cf[p].astype(np.float64) * r
        hl = cl[p].astype(np.float64)
        out += [hf[hf > thr_f], hl[hl > thr_l]]
    return out


def slice_range(tot_label, length_divisor):
    """Voxels of the original vertebra per slice -> (centre, half-length) by the lines of process_datasets_to_excel, or None where it has no voxel."""
    idx = np.flatnonzero(tot_label)
    if idx.size == 0:
        return None
    centre = int((tot_label * np.arange(tot_label.size)).sum() / tot_label.sum())
    return centre, (int(idx[-1]) - int(idx[0])) // length_divisor


def _profile(hf, hl, sel_f, sel_l, axis):
    """Selected heights averaged along `axis`, summed in ascending index order -> (profile_fake, profile_label, curve)."""
    nf, nl = sel_f.sum(axis=axis), sel_l.sum(axis=axis)
    sf, sl = np.zeros(nf.shape), np.zeros(nl.shape)
    for i in range(hf.shape[axis]):
        a, b, m, n = (np.take(v, i, axis=axis) for v in (hf, hl, sel_f, sel_l))
        sf = np.where(m, sf + a, sf)
        sl = np.where(n, sl + b, sl)
    with np.errstate(invalid='ignore', divide='ignore'):
        pf = np.where(nf > 0, sf / nf, np.nan)
        pl = np.where(nl > 0, sl / nl, np.nan)
        return pf, pl, (pf - pl) / (pf + 1e-6)


def view_maps(vol_fake, vol_label, label_index, length_divisor=5, height_threshold=0.64, view='sagittal', centre_length=None):
    """-> dict of loss / height_fake / height_label [S, C] float64, flags [S, C] uint8, the column profiles (profile_fake, profile_label, curve: [C])
    and slice profiles (slice_profile_fake, slice_profile_label, slice_curve: [S]), range (lo, hi), raises, and `selected`: {s: the eight arrays of
    selected_heights} for every visited slice -- or None where the original lacks the vertebra.  centre_length: explicit (centre, half-length)."""
    tf, tl = column_table(vol_fake, label_index, view), column_table(vol_label, label_index, view)
    S, C = tf.shape
    cl_ = centre_length or slice_range(tl.sum(axis=1), length_divisor)
    if cl_ is None:
        return None
    lo, hi, _ = slice(cl_[0] - cl_[1], cl_[0] + cl_[1]).indices(S)           # numpy slice normalisation
    hf, hl = np.zeros((S, C)), np.zeros((S, C))
    loss = np.full((S, C), np.nan)
    flags = np.zeros((S, C), np.uint8)
    selected, raises = {}, False
    for s in range(lo, hi):
        if tf[s].sum() == 0 or tl[s].sum() == 0:
            continue
        state = slice_state(tf[s], tl[s], height_threshold, view)
        t1, t2, ratios, thr_f, thr_l, r = state
        raises = raises or r
        selected[s] = selected_heights(tf[s], tl[s], state)
        hf[s], hl[s] = tf[s].astype(np.float64) * ratios[0], tl[s].astype(np.float64)
        sel_f, sel_l = hf[s] > thr_f, hl[s] > thr_l
        c = np.arange(C)
        flags[s] = np.where(c < t1, 0, np.where(c < t2, 1, 2)) | sel_f * SEL_FAKE | sel_l * SEL_LABEL | VISITED
        loss[s, sel_f] = (hf[s, sel_f] - hl[s, sel_f]) / (hf[s, sel_f] + 1e-6)
    sel_f, sel_l = (flags & SEL_FAKE) != 0, (flags & SEL_LABEL) != 0
    res = {'loss': loss, 'height_fake': hf, 'height_label': hl, 'flags': flags, 'range': (lo, hi), 'raises': raises, 'selected': selected}
    res['profile_fake'], res['profile_label'], res['curve'] = _profile(hf, hl, sel_f, sel_l, 0)
    res['slice_profile_fake'], res['slice_profile_label'], res['slice_curve'] = _profile(hf, hl, sel_f, sel_l, 1)
    return res


def reduce_selected(selected):
    """The script's own reduction (calculate_rhlv :130-147) of the per-slice arrays -> ((all, pre, mid, post RHLV, relative_height_label), the eight means)."""
    m = []
    for k in range(8):
        h = np.concatenate([selected[s][k] for s in sorted(selected)]) if selected else np.zeros(0)
        m.append(float(np.mean(h)) if h.size > 0 else 0.0)
    res = [(m[2 * c] - m[2 * c + 1]) / (m[2 * c] + 1e-6) for c in range(4)]
    lab = [m[3], m[5], m[7]]
    return tuple(res) + (min(lab) / (max(lab) + 1e-6),), m


def selected_means(maps):
    """(mean selected height_fake, mean selected height_label) of a whole map: the all_height_fake / all_height_label the script reports."""
    sel_f, sel_l = (maps['flags'] & SEL_FAKE) != 0, (maps['flags'] & SEL_LABEL) != 0
    return (float(maps['height_fake'][sel_f].mean()) if sel_f.any() else 0.0, float(maps['height_label'][sel_l].mean()) if sel_l.any() else 0.0)
