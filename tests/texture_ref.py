"""numpy restatement of hv_glcm (csrc/texture.hip): boolean shifted slices plus np.add.at, the quantisation t = (x - lo) / width in float64.
tests/test_texture_ref_cpu.py pins it against a triple-loop brute force and Haralick's 4 x 4 example; the GPU tests compare the device's out and
info with it bit for bit (everything is an integer count)."""
import numpy as np

from labelstats_ref import BAD_LABEL, EMPTY, NONFINITE, valid_labels

INFO = 4
MAX_REACH = 4
HARALICK_IMAGE = np.array([[0, 0, 1, 1], [0, 0, 1, 1], [0, 2, 2, 2], [2, 2, 3, 3]], dtype=np.uint8)
HARALICK_GLCM = np.array([[4, 2, 1, 0], [2, 4, 0, 0], [1, 0, 6, 1], [0, 0, 1, 2]], dtype=np.int64)      # offset along the row, symmetric


def directions13():
    """The 13 offsets whose first non-zero component is positive, in lexicographic order."""
    return [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) > (0, 0, 0)]


def levels_of(vol, lo, width, G):
    """-> (level per voxel (0 where not finite), finite, t < 0, t >= G): the two float64 operations, then the clamp and the truncation."""
    x = np.asarray(vol).astype(np.float64)
    finite = np.isfinite(x)
    with np.errstate(invalid='ignore', over='ignore'):
        t = (np.where(finite, x, np.float64(lo)) - np.float64(lo)) / np.float64(width)
    low, high = t < 0, t >= G
    lev = np.where(low, 0, np.where(high, G - 1, np.trunc(np.where(low | high, 0.0, t)))).astype(np.int64)
    return lev, finite, low & finite, high & finite


def slots_of(label, labels, mask=None):
    """-> (slot per voxel, -1 for none; whether the volume holds a value that is no label).  A masked-out voxel's label is not looked at."""
    label = np.asarray(label)
    if mask is not None:
        keep = np.asarray(mask) != 0
        lab, _ = valid_labels(np.where(keep, label, 0))
        _, bad = valid_labels(label[keep]) if keep.any() else (None, False)
        lab = np.where(keep, lab, -1)
    else:
        lab, bad = valid_labels(label)
    slot = np.full(lab.shape, -1, dtype=np.int64)
    for s, l in enumerate(labels):
        slot[lab == l] = s
    return slot, bad


def _shifted(A, d):
    """The slices of p and of p + d over every p with both inside an extent-A axis."""
    return slice(max(0, -d), A - max(0, d)), slice(max(0, d), A - max(0, -d))


def glcm_ref(vol, label, labels, offsets, lo, width, G, symmetric=True, mask=None):
    """One 3-D volume -> (out [S][D][G][G] int64, info [S][INFO] int64) as the device writes them."""
    vol = np.asarray(vol)
    S, D = len(labels), len(offsets)
    lev, finite, low, high = levels_of(vol, lo, width, G)
    slot, bad = slots_of(label, labels, mask)
    pair_slot = np.where(finite, slot, -1)
    out = np.zeros((S, D, G, G), dtype=np.int64)
    info = np.zeros((S, INFO), dtype=np.int64)
    for s in range(S):
        mine = slot == s
        info[s, 1], info[s, 2], info[s, 3] = (mine & finite).sum(), (mine & low).sum(), (mine & high).sum()
        info[s, 0] = (BAD_LABEL if bad else 0) | (NONFINITE if (mine & ~finite).any() else 0) | (0 if info[s, 1] else EMPTY)
    for n, d in enumerate(offsets):
        if any(abs(int(c)) >= a for c, a in zip(d, vol.shape)):
            continue                                # no pair at all along an axis shorter than the step
        src, dst = zip(*(_shifted(a, int(c)) for a, c in zip(vol.shape, d)))
        sp, sq = pair_slot[src], pair_slot[dst]
        both = (sp == sq) & (sp >= 0)
        s_idx, a, b = sp[both], lev[src][both], lev[dst][both]
        np.add.at(out, (s_idx, n, a, b), 1)
        if symmetric:
            np.add.at(out, (s_idx, n, b, a), 1)
    return out, info


def glcm_brute(vol, label, labels, offsets, lo, width, G, symmetric=True, mask=None):
    """The definition as three loops over the voxels (tiny cases only)."""
    vol, label = np.asarray(vol), np.asarray(label)
    A = vol.shape
    out = np.zeros((len(labels), len(offsets), G, G), dtype=np.int64)

    def slot(p):
        if mask is not None and not mask[p]:
            return -1
        return list(labels).index(int(label[p])) if int(label[p]) in labels else -1

    def level(p):
        t = (np.float64(vol[p]) - np.float64(lo)) / np.float64(width)
        return 0 if t < 0 else (G - 1 if t >= G else int(t))

    for n, d in enumerate(offsets):
        for i in range(A[0]):
            for j in range(A[1]):
                for k in range(A[2]):
                    p, q = (i, j, k), (i + d[0], j + d[1], k + d[2])
                    if not all(0 <= c < a for c, a in zip(q, A)):
                        continue
                    s = slot(p)
                    if s < 0 or slot(q) != s:
                        continue
                    out[s, n, level(p), level(q)] += 1
                    if symmetric:
                        out[s, n, level(q), level(p)] += 1
    return out
