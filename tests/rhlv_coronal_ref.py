"""float64 numpy restatement of the reference's coronal RHLV script (evaluation/RHLV_quantification_coronal.py:41-147 and the per-vertebra
body of process_datasets_to_excel :159-181), in this project's words: the CPU side of tests/test_rhlv_views_gpu.py, itself checked against
the reference's own outputs (fixture G15) by tests/test_rhlv_views_cpu.py.

The coronal script is not the sagittal one (oracle.restate.rhlv_*) on a permuted volume:
  * slices run along axis 1 (`[:, s, :]`), their columns along axis 2;
  * a third's rescale ratio is label.max() / fake.max() -- no + 1e-6, so a third the generated vertebra leaves empty under a non-empty original
    one gives inf, its columns become 0 * inf = nan and select nothing;
  * the thirds are not guarded by .size > 0: a participating slice whose pre or mid third of columns is empty raises ValueError (numpy's max()
    of an empty array).  With t1 = int(y_min + y_range / 3) and t2 = int(y_min + 2 * y_range / 3) of the generated vertebra's column extent
    that is: pre `[:t1]` empty iff t1 == 0 (y_min == 0 and y_range < 3), mid `[t1:t2]` empty iff y_range < 2; post `[t2:]` never is.
"""
import numpy as np


def third_bounds(cols_fake):
    """Column counts of the generated vertebra in one slice -> (t1, t2): pre = [:t1], mid = [t1:t2], post = [t2:]."""
    idx = np.flatnonzero(cols_fake)
    y_min, y_max = int(idx[0]), int(idx[-1])
    y_range = y_max - y_min
    return int(y_min + y_range / 3), int(y_min + 2 * y_range / 3)


def _centre_height(cols):
    """Height at the column int(mean of the column index over the voxels)."""
    return int(cols[int((cols * np.arange(cols.size)).sum() / cols.sum())])


def heights(seg_fake, seg_label, height_threshold):
    """Binary [H, S, C] volumes (already cut to the slice range along axis 1) -> the eight arrays of selected column heights
    (all / pre / mid / post x generated / original).  ValueError where the reference raises."""
    out = [[] for _ in range(8)]
    for s in range(seg_label.shape[1]):
        cols_f = np.count_nonzero(seg_fake[:, s, :], axis=0)
        cols_l = np.count_nonzero(seg_label[:, s, :], axis=0)
        if cols_f.sum() == 0 or cols_l.sum() == 0:
            continue
        t1, t2 = third_bounds(cols_f)
        parts = [slice(None), slice(None, t1), slice(t1, t2), slice(t2, None)]
        ratios = []
        for p in parts:
            if cols_f[p].size == 0:
                raise ValueError('zero-size array to reduction operation maximum which has no identity')
            mf, ml = np.float64(cols_f[p].max()), np.float64(cols_l[p].max())
            with np.errstate(divide='ignore'):
                ratios.append(ml / mf if ml > mf else np.float64(1.0))
        centre_f = _centre_height(cols_f) * ratios[0]
        centre_l = _centre_height(cols_l)
        for c, p in enumerate(parts):
            with np.errstate(invalid='ignore'):
                hf = cols_f[p].astype(np.float64) * ratios[c]
            out[2 * c].extend(hf[hf > centre_f * height_threshold])
            hl = cols_l[p].astype(np.float64)
            out[2 * c + 1].extend(hl[hl > centre_l * height_threshold])
    return [np.array(o, dtype=np.float64) for o in out]


def rhlv(seg_fake, seg_label, center, length, height_threshold):
    """calculate_rhlv -> ((all, pre, mid, post RHLV, relative_height_label), the eight mean heights)."""
    cut = slice(center - length, center + length)          # numpy slice rules: a negative start wraps around
    hs = heights(seg_fake[:, cut, :], seg_label[:, cut, :], height_threshold)
    m = [float(np.mean(h)) if h.size > 0 else 0.0 for h in hs]
    res = [(m[2 * c] - m[2 * c + 1]) / (m[2 * c] + 1e-6) for c in range(4)]
    lab = [m[3], m[5], m[7]]
    return tuple(res) + (min(lab) / (max(lab) + 1e-6),), m


def center_length(seg_label, length_divisor):
    """Centre slice and half-length from the original vertebra's extent along axis 1, or None where it has no voxel."""
    loc = np.where(seg_label)[1]
    if loc.size == 0:
        return None
    return int(np.mean(loc)), (int(np.max(loc)) - int(np.min(loc))) // length_divisor


def rhlv_volume(vol_fake, vol_label, label_index, length_divisor=5, height_threshold=0.64):
    """Per-vertebra body of process_datasets_to_excel on id volumes -> rhlv(), or None where the original lacks the vertebra."""
    sl = (np.asarray(vol_label) == label_index).astype(np.float64)
    sf = (np.asarray(vol_fake) == label_index).astype(np.float64)
    cl = center_length(sl, length_divisor)
    if cl is None:
        return None
    return rhlv(sf, sl, cl[0], cl[1], height_threshold)
