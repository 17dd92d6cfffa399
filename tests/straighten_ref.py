"""Numpy float64 / Python-int restatement of the four kernels of csrc/straighten.hip -- the stats pass (hv_straighten_stats), the order-1
sampler (hv_straighten_sample_sp) and the crop with its split cleanup (hv_straighten_crop) -- and decoders of the stats record.  No device
and no torch here; tests/test_straighten_ref_cpu.py pins it against scipy, plain numpy and the host mirror of tests/test_straighten_gpu.py.

Volumes are [D0][D1][D2].  Presence words: presence[l][h // 64] bit h % 64 says that label l occurs in row rows // 2 + h of the centre
column (all of axis 0, the last axis at its centre), for h in [0, rows - rows // 2); `rows` is D1 of a raw scan, PA of a straight volume.
"""
import numpy as np

import spline_ref as P

HDR, CNT, SUM, PRES = 4, 4, 260, 1028          # word offsets of the stats record (include/hvgan.h)


def rows_words(rows):
    """64-bit words per label of the presence record of a volume with `rows` rows."""
    return (rows - rows // 2 + 63) // 64


def label_values(label):
    """-> (int64 labels with every bad value replaced by 0, bad flag).  A value is bad unless it is an integer in [0, 255]."""
    d = np.asarray(label).astype(np.float64)
    with np.errstate(invalid='ignore'):
        ok = (d >= 0.0) & (d <= 255.0) & (d == np.floor(d))
    return np.where(ok, d, 0.0).astype(np.int64), bool((~ok).any())


def presence_ref(lab):
    """Presence words [256][Rw] uint64 of an integer label volume [D0][rows][cols]."""
    rows, cols = lab.shape[1], lab.shape[2]
    row0, Rw = rows // 2, rows_words(rows)
    words = [[0] * Rw for _ in range(256)]
    for h in range(rows - row0):
        for l in set(int(x) for x in lab[:, row0 + h, cols // 2]):
            if l != 0:
                words[l][h // 64] |= 1 << (h % 64)
    return np.array(words, dtype=np.uint64).reshape(256, Rw)


def stats_ref(ct, label):
    """hv_straighten_stats.  ct: a volume or None.  -> dict: 'min', 'max' (floats; None without a CT), 'bad' (bool), 'counts' int64 [256],
    'sums' int64 [256][3] (label 0 is not counted), 'presence' uint64 [256][Rw] with Rw = (D1 - D1 // 2 + 63) // 64."""
    lab, bad = label_values(label)
    counts = np.zeros(256, dtype=np.int64)
    sums = np.zeros((256, 3), dtype=np.int64)
    idx = np.indices(lab.shape, dtype=np.int64)
    keep = lab != 0
    np.add.at(counts, lab[keep], 1)
    for a in range(3):
        np.add.at(sums[:, a], lab[keep], idx[a][keep])
    mn = mx = None
    if ct is not None:
        c = np.asarray(ct).astype(np.float64)
        mn, mx = float(c.min()), float(c.max())
    return {'min': mn, 'max': mx, 'bad': bad, 'counts': counts, 'sums': sums, 'presence': presence_ref(lab)}


def decode_stats(words, D1):
    """The stats record (uint64 or int64 words, hv_straighten_stats_bytes(D1) / 8 of them) -> the dict of stats_ref, plus 'raw' (words 0, 1:
    ~key(min), key(max)) and 'word3'.  The two keys are decoded by hvgan.straighten._Stats."""
    from hvgan import straighten as S
    w = np.ascontiguousarray(words).view(np.uint64)
    Rw = rows_words(D1)
    assert w.size == PRES + 256 * Rw, (w.size, D1)
    st = S._Stats(w[:PRES].copy())
    return {'min': st.ct_min, 'max': st.ct_max, 'bad': bool(w[2] != 0), 'counts': st.counts, 'sums': st.sums.astype(np.int64),
            'presence': w[PRES:].reshape(256, Rw).copy(), 'raw': (int(w[0]), int(w[1])), 'word3': int(w[3])}


def sample_points(ct, label, coords, win, wmin, wmax):
    """The sampler's value rule at coords [3, M] (voxel indices): -> (ct float64 [M], label uint8 [M]).  Inside iff 0 <= c <= D - 1 on every
    axis, else both are 0.  CT: i0 = floor(c), t = c - i0, i1 = min(i0 + 1, D - 1), the sum over the 8 corners with axis 0 outermost and axis
    2 innermost of ((u * wx) * wy) * wz, u the corner value (windowed first when `win`).  Label: the voxel at floor(c + 0.5)."""
    ct, label = np.asarray(ct), np.asarray(label)
    c = np.asarray(coords, dtype=np.float64)
    D = ct.shape
    inside = np.ones(c.shape[1], dtype=bool)
    for a in range(3):
        inside &= (c[a] >= 0.0) & (c[a] <= float(D[a] - 1))
    u = c[:, inside]
    i0, i1, w0, w1 = [], [], [], []
    for a in range(3):
        f = np.floor(u[a])
        t = u[a] - f
        lo = f.astype(np.int64)
        i0.append(lo)
        i1.append(np.minimum(lo + 1, D[a] - 1))
        w0.append(1.0 - t)
        w1.append(t)
    acc = np.zeros(u.shape[1])
    for hx in range(2):
        for hy in range(2):
            for hz in range(2):
                val = ct[(i1 if hx else i0)[0], (i1 if hy else i0)[1], (i1 if hz else i0)[2]].astype(np.float64)
                if win:
                    val = P.window(val, wmin, wmax)
                acc = acc + ((val * (w1 if hx else w0)[0]) * (w1 if hy else w0)[1]) * (w1 if hz else w0)[2]
    n = [np.floor(u[a] + 0.5).astype(np.int64) for a in range(3)]
    d = label[n[0], n[1], n[2]].astype(np.float64)
    with np.errstate(invalid='ignore'):
        lab = np.where((d >= 0.0) & (d <= 255.0), d, 0.0).astype(np.uint8)
    out_ct, out_lab = np.zeros(c.shape[1]), np.zeros(c.shape[1], dtype=np.uint8)
    out_ct[inside], out_lab[inside] = acc, lab
    return out_ct, out_lab


def sample_ref(ct, label, knots, basis, PA, PB, spacing, win, wmin, wmax):
    """hv_straighten_sample_sp (order 1): -> (sct float64 [N][PA][PB], slab uint8 [N][PA][PB], presence uint64 [256][Rw] of slab)."""
    knots, basis = np.asarray(knots, dtype=np.float64), np.asarray(basis, dtype=np.float64)
    grid = P.straight_grid(knots, basis, spacing, plane=(PB, PA))
    v, l = sample_points(ct, label, grid.reshape(3, -1), win, wmin, wmax)
    sct, slab = v.reshape(grid.shape[1:]), l.reshape(grid.shape[1:])
    return sct, slab, presence_ref(slab)


def cutoffs(D1, presence):
    """Row cutoff per label [256]: D1 // 2 plus the first h in [0, D1 - D1 // 2) whose presence bit is clear, D1 if none is."""
    row0 = D1 // 2
    cut = np.full(256, D1, dtype=np.int64)
    for l in range(256):
        for h in range(D1 - row0):
            if not (int(presence[l][h // 64]) >> (h % 64)) & 1:
                cut[l] = row0 + h
                break
    return cut


def crop_ref(ct, label, D1, win, wmin, wmax, presence, boxes, out_size):
    """hv_straighten_crop: per box {lo0, lo1, lo2, len0, len1, len2, start0, start1, start2} the source range [lo, lo + len) placed at
    `start` in a zero volume of out_size; the CT windowed when `win` and never cut, the label zeroed where its source row (axis 1) is at or
    past its label's cutoff.  -> (ct float64 [V][*out_size], label uint8 [V][*out_size])."""
    ct, label = np.asarray(ct), np.asarray(label)
    cut = cutoffs(D1, presence)
    V = len(boxes)
    out_ct = np.zeros((V,) + tuple(out_size))
    out_lab = np.zeros((V,) + tuple(out_size), dtype=np.uint8)
    for v, bx in enumerate(boxes):
        lo, ln, st = [int(x) for x in bx[0:3]], [int(x) for x in bx[3:6]], [int(x) for x in bx[6:9]]
        ln = [max(0, min(ln[i], out_size[i] - st[i])) for i in range(3)]        # what of the box falls into the output
        if min(ln) == 0:
            continue
        src = tuple(slice(lo[i], lo[i] + ln[i]) for i in range(3))
        dst = (v,) + tuple(slice(st[i], st[i] + ln[i]) for i in range(3))
        c = ct[src].astype(np.float64)
        out_ct[dst] = P.window(c, wmin, wmax) if win else c
        d = label[src].astype(np.float64)
        with np.errstate(invalid='ignore'):
            l = np.where((d >= 0.0) & (d <= 255.0), d, 0.0).astype(np.int64)
        y = np.arange(lo[1], lo[1] + ln[1], dtype=np.int64)[None, :, None]
        out_lab[dst] = np.where(y >= cut[l], 0, l).astype(np.uint8)
    return out_ct, out_lab
