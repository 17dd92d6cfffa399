"""numpy restatement, float64, of every field hv_label_stats (csrc/labelstats.hip) writes, in the device's record layout, and the cases the CPU
and GPU tests share.  tests/test_labelstats_ref_cpu.py pins it against scipy.ndimage and np.percentile.  Float sums are math.fsum-exact (the
correctly rounded sum of the doubles, and of the float64 products v * v); integer sums are Python integers."""
import math
from fractions import Fraction

import numpy as np

REC = 32
COUNT, SUM, SUMSQ, MIN, MAX, COORD, LO, HI, STATUS, ORDER = 0, 1, 2, 3, 4, 5, 8, 11, 14, 16
BAD_LABEL, NONFINITE, EMPTY = 1, 2, 4
SENTINEL = -12345.678                          # what a record's unwritten fields hold in these tests
QS = (0.0, 100.0, 50.0, 5.0, 95.0, 25.0)       # 25 % of a 65-voxel label is position 16 exactly, 50 % position 32
LABELS = (1, 2, 3, 4, 5, 6, 7, 9)              # 9 is absent
SHAPE = (33, 40, 70)


def sort_key(x):
    """The order-preserving unsigned key of the values (float: -0.0 below +0.0, NaNs at the two ends by their sign bit)."""
    x = np.asarray(x)
    if x.dtype == np.float32:
        u = x.view(np.uint32)
        return np.where(u >> 31 != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint64)
    if x.dtype == np.float64:
        u = x.view(np.uint64)
        return np.where(u >> np.uint64(63) != 0, ~u, u | np.uint64(1 << 63))
    return (x.astype(np.int64) + 32768).astype(np.uint64)


def valid_labels(label):
    """-> (int labels with -1 where the value is no integer in [0, 255], whether any such value exists)."""
    d = np.asarray(label).astype(np.float64)
    with np.errstate(invalid='ignore'):
        ok = (d >= 0) & (d <= 255) & (d == np.floor(d))
    return np.where(ok, np.nan_to_num(d, nan=0.0, posinf=0.0, neginf=0.0), -1).astype(np.int64), bool((~ok).any())


def order_ranks(n, q):
    """numpy's linear rule: vi = (n - 1) * (q / 100); -> (lo, hi, vi)."""
    vi = np.float64(n - 1) * np.true_divide(np.float64(q), np.float64(100))
    if vi >= n - 1:
        return n - 1, n - 1, vi
    lo = int(np.floor(vi))
    return lo, lo + 1, vi


def label_stats_ref(vol, label, labels, q=(), mask=None, fill=SENTINEL):
    """One 3-D volume -> records [S][REC] as the device writes them (fields it leaves alone hold `fill`).  Integer dtypes: [SUM], [SUMSQ] hold the
    int64 bit patterns of the exact sums."""
    vol, label = np.asarray(vol), np.asarray(label)
    integer = vol.dtype.kind in 'iu'
    lab, bad = valid_labels(label)
    if mask is not None:
        lab = np.where(np.asarray(mask) != 0, lab, -1)
    rec = np.full((len(labels), REC), fill, dtype=np.float64)
    raw = rec.view(np.int64)
    idx = np.indices(vol.shape)
    for s, l in enumerate(labels):
        sel = lab == l
        x = vol[sel]
        n = int(x.size)
        r = rec[s]
        r[COUNT] = n
        st = (BAD_LABEL if bad else 0) | (0 if n else EMPTY)
        xd = x.astype(np.float64)
        if integer:
            xi = [int(t) for t in x]
            raw[s, SUM], raw[s, SUMSQ] = sum(xi), sum(t * t for t in xi)
        else:
            if not np.isfinite(xd).all():
                st |= NONFINITE
            with np.errstate(all='ignore'):
                r[SUM], r[SUMSQ] = (math.fsum(xd), math.fsum(xd * xd)) if not st & NONFINITE else (np.nan, np.nan)
        order = np.argsort(sort_key(x), kind='stable')
        xs = xd[order]
        r[MIN], r[MAX] = (xs[0], xs[-1]) if n else (np.inf, -np.inf)
        for a in range(3):
            c = idx[a][sel]
            r[COORD + a] = int(c.sum())
            r[LO + a], r[HI + a] = (int(c.min()), int(c.max())) if n else (vol.shape[a], -1)
        r[STATUS], r[STATUS + 1] = st, 0.0
        for t, p in enumerate(q):
            if n:
                lo, hi, _ = order_ranks(n, p)
                r[ORDER + 2 * t], r[ORDER + 2 * t + 1] = xs[lo], xs[hi]
            else:
                r[ORDER + 2 * t] = r[ORDER + 2 * t + 1] = np.nan
    return rec


def mean_variance(rec, integer):
    """Mean and population variance of every slot from a record array, exactly rounded from the sums (rational arithmetic)."""
    raw = rec.view(np.int64)
    out = np.full((rec.shape[0], 2), np.nan)
    for s in range(rec.shape[0]):
        n = int(rec[s, COUNT])
        if n == 0 or int(rec[s, STATUS]) & NONFINITE:
            continue
        sv, svv = (Fraction(int(raw[s, SUM])), Fraction(int(raw[s, SUMSQ]))) if integer else (Fraction(float(rec[s, SUM])), Fraction(float(rec[s, SUMSQ])))
        out[s] = float(sv / n), max(float(svv / n - (sv / n) ** 2), 0.0)
    return out


def same_value(a, b):
    """Bit for bit, except that two zeros compare equal whatever their signs (the select may return either)."""
    a, b = np.float64(a), np.float64(b)
    return a.tobytes() == b.tobytes() or (a == 0.0 and b == 0.0)


# ------------------------------------------------------------------------------------------------ the shared cases
def base_label():
    """Label sizes 1, 2, 63, 64, 65, one label over many tiles and workgroups, one of a single value; everything else 0."""
    lab = np.zeros(SHAPE, dtype=np.uint8)
    lab[2:30, 3:37, 5:60] = 1                  # 28 x 34 x 55 voxels, across 2 x 3 x 4 tiles
    lab[31, 0, 0] = 2
    lab[31, 2, 15:17] = 3                      # two voxels on both sides of a tile edge
    lab[31, 4, 0:63] = 4
    lab[31, 6, 3:67] = 5
    lab[32, 8, 2:67] = 6
    lab[30:33, 20:30, 30:50] = 7
    return lab


def intensities(dtype, seed=0):
    """Intensities for base_label(): both ends of the dtype's range, negative values, denormals, a pair that differs in the last bit (label 3:
    its median's two order statistics), a constant label (7), +0.0 and -0.0."""
    g = np.random.default_rng(seed)
    dtype = np.dtype(dtype)
    if dtype == np.uint8:
        v = g.integers(0, 256, SHAPE).astype(np.uint8)
        v[5, 5, 10], v[5, 5, 11] = 0, 255
    elif dtype == np.int16:
        v = g.integers(-1000, 3000, SHAPE).astype(np.int16)
        v[5, 5, 10], v[5, 5, 11] = -32768, 32767
    else:
        v = (g.standard_normal(SHAPE) * 300.0 + 400.0).astype(dtype)
        tiny = np.finfo(dtype).smallest_subnormal
        v[5, 5, 10], v[5, 5, 11], v[5, 5, 12], v[5, 5, 13] = tiny, -tiny * 3, 0.0, -0.0
        v[31, 6, 10], v[31, 6, 11] = tiny * 7, -1234.5
        x = dtype.type(517.3)
        v[31, 2, 15], v[31, 2, 16] = np.nextafter(x, dtype.type(np.inf)), x
    v[30:33, 20:30, 30:50] = dtype.type(77)
    return v


def scipy_chain(vol, label, labels, q=(), mask=None):
    """The host chain this operator replaces: -> dict of per-label lists from scipy.ndimage and np.percentile, on the float64 copy of the
    volume (exact for every dtype; scipy would sum a float32 volume in float32)."""
    from scipy import ndimage
    vol = np.asarray(vol).astype(np.float64)
    lab = np.asarray(label).astype(np.int64)
    if mask is not None:
        lab = np.where(np.asarray(mask) != 0, lab, -1)
    lab1 = lab + 1                              # find_objects wants positive labels; label 0 may be listed
    objs = ndimage.find_objects(lab1, max_label=257)
    out = {k: [] for k in ('count', 'sum', 'mean', 'variance', 'min', 'max', 'centroid', 'box', 'percentiles')}
    for l in labels:
        sel = lab == l
        n = int(sel.sum())
        out['count'].append(n)
        if n == 0:
            for k in ('sum', 'mean', 'variance', 'min', 'max', 'centroid', 'percentiles'):
                out[k].append(None)
            out['box'].append(objs[l])
            continue
        out['sum'].append(ndimage.sum_labels(vol, lab, l))
        out['mean'].append(ndimage.mean(vol, lab, l))
        out['variance'].append(ndimage.variance(vol, lab, l))
        out['min'].append(ndimage.minimum(vol, lab, l))
        out['max'].append(ndimage.maximum(vol, lab, l))
        out['centroid'].append(ndimage.center_of_mass(np.ones(vol.shape), lab, l))
        out['box'].append(objs[l])
        out['percentiles'].append([np.percentile(vol[sel], p) for p in q])
    return out
