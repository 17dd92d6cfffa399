"""numpy restatement of hv_glrlm and hv_gldm (csrc/texture_runs.hip): shifted boolean chains for the runs, shifted slices for the neighbourhood,
the quantisation and the slots of tests/texture_ref.py.  tests/test_texture_runs_ref_cpu.py pins it against loop-form brute forces and the worked
examples of the pyradiomics documentation; the GPU tests compare the device's out, dep, ngt and info with it bit for bit (everything is an integer
count).  The loop forms of the host features at the end are written independently of healthivert-gan_amd/texture_runs.py's vectorised ones."""
import itertools
import math

import numpy as np

from labelstats_ref import BAD_LABEL, EMPTY, NONFINITE
from texture_ref import INFO, directions13, levels_of, slots_of  # noqa: F401

RLM_INFO = 4 + 13
NB = 27
NEIGHBOURS = [d for d in itertools.product((-1, 0, 1), repeat=3) if d != (0, 0, 0)]

# the worked examples of the pyradiomics documentation, levels 1 .. 5 as printed
RUN_IMAGE = np.array([[5, 2, 5, 4, 4], [3, 3, 3, 1, 3], [2, 1, 1, 1, 3], [4, 2, 2, 2, 3], [3, 5, 3, 3, 2]], dtype=np.uint8)
RUN_GLRLM = np.array([[1, 0, 1, 0, 0], [3, 0, 1, 0, 0], [4, 1, 1, 0, 0], [1, 1, 0, 0, 0], [3, 0, 0, 0, 0]], dtype=np.int64)     # along the row
RUN_GLDM = np.array([[0, 1, 2, 1], [1, 2, 3, 0], [1, 4, 4, 0], [1, 2, 0, 0], [3, 0, 0, 0]], dtype=np.int64)                     # alpha = 0, k = 0 .. 3
NGTDM_IMAGE = np.array([[1, 2, 5, 2], [3, 5, 1, 3], [1, 3, 5, 5], [3, 1, 1, 1]], dtype=np.uint8)
NGTDM_N = np.array([6, 2, 4, 0, 4], dtype=np.int64)
NGTDM_S = np.array([13.35, 2.0, 91.0 / 30.0, 0.0, 10.075])


def _codes(vol, label, labels, lo, width, G, mask):
    """-> (code per voxel: slot * 64 + level, -1 for a voxel with no slot or not finite; info [S][INFO] as the device writes it)."""
    lev, finite, low, high = levels_of(vol, lo, width, G)
    slot, bad = slots_of(label, labels, mask)
    info = np.zeros((len(labels), INFO), dtype=np.int64)
    for s in range(len(labels)):
        mine = slot == s
        info[s, 1], info[s, 2], info[s, 3] = (mine & finite).sum(), (mine & low).sum(), (mine & high).sum()
        info[s, 0] = (BAD_LABEL if bad else 0) | (NONFINITE if (mine & ~finite).any() else 0) | (0 if info[s, 1] else EMPTY)
    return np.where(finite & (slot >= 0), slot * 64 + lev, -1), info


def _at(a, d, t, fill):
    """b with b[p] = a[p + t d] where p + t d lies inside, else fill."""
    out = np.full(a.shape, fill, dtype=a.dtype)
    src, dst = [], []
    for n, c in zip(a.shape, d):
        s = t * int(c)
        if abs(s) >= n:
            return out
        src.append(slice(max(0, s), n - max(0, -s)))
        dst.append(slice(max(0, -s), n - max(0, s)))
    out[tuple(dst)] = a[tuple(src)]
    return out


def glrlm_ref(vol, label, labels, offsets, lo, width, G, R, mask=None):
    """One 3-D volume -> (out [S][D][G][R] int64, info [S][RLM_INFO] int64) as the device writes them."""
    vol = np.asarray(vol)
    S, D = len(labels), len(offsets)
    code, info4 = _codes(vol, label, labels, lo, width, G, mask)
    out = np.zeros((S, D, G, R), dtype=np.int64)
    info = np.zeros((S, RLM_INFO), dtype=np.int64)
    info[:, :INFO] = info4
    has = code >= 0
    for n, d in enumerate(offsets):
        start = has & (_at(code, d, -1, -1) != code)
        length = np.zeros(vol.shape, dtype=np.int64)
        chain = start.copy()                                        # the run that starts at p reaches p + (t - 1) d
        t = 1
        while chain.any():
            length[chain] = t
            chain = chain & (_at(code, d, t, -1) == code)
            t += 1
        c, L = code[start], length[start]
        np.add.at(out, (c // 64, n, c % 64, np.minimum(L, R) - 1), 1)
        np.add.at(info, (c[L > R] // 64, INFO + n), 1)
    return out, info


def gldm_ref(vol, label, labels, lo, width, G, alpha, mask=None):
    """One 3-D volume -> (dep [S][G][27], ngt [S][G][27][2], info [S][INFO]) int64 as the device writes them."""
    vol = np.asarray(vol)
    S = len(labels)
    code, info = _codes(vol, label, labels, lo, width, G, mask)
    has = code >= 0
    n = np.zeros(vol.shape, dtype=np.int64)
    total, close = n.copy(), n.copy()
    for d in NEIGHBOURS:
        q = _at(code, d, 1, -1)
        same = has & (q >= 0) & (q // 64 == code // 64)
        n += same
        total += np.where(same, q % 64, 0)
        close += same & (np.abs(q % 64 - code % 64) <= alpha)
    dep = np.zeros((S, G, NB), dtype=np.int64)
    ngt = np.zeros((S, G, NB, 2), dtype=np.int64)
    s, lev = code[has] // 64, code[has] % 64
    np.add.at(dep, (s, lev, close[has]), 1)
    np.add.at(ngt, (s, lev, n[has], 0), 1)
    np.add.at(ngt, (s, lev, n[has], 1), np.abs(lev * n[has] - total[has]))
    return dep, ngt, info


# ------------------------------------------------------------------------------------------------ the definitions as loops (tiny cases only)
def _voxel(vol, label, labels, lo, width, G, mask, p):
    """-> (slot, level) of voxel p, None if it has no slot or is not finite."""
    if mask is not None and not mask[p]:
        return None
    if int(label[p]) not in labels or not math.isfinite(float(vol[p])):
        return None
    t = (np.float64(vol[p]) - np.float64(lo)) / np.float64(width)
    return list(labels).index(int(label[p])), 0 if t < 0 else (G - 1 if t >= G else int(t))


def glrlm_brute(vol, label, labels, offsets, lo, width, G, R, mask=None):
    """-> (out [S][D][G][R], capped [S][D]): every voxel asked whether a run starts at it, the run walked to its end."""
    A = vol.shape
    cell = lambda p: _voxel(vol, label, labels, lo, width, G, mask, p) if all(0 <= c < a for c, a in zip(p, A)) else None
    out = np.zeros((len(labels), len(offsets), G, R), dtype=np.int64)
    capped = np.zeros((len(labels), len(offsets)), dtype=np.int64)
    for n, d in enumerate(offsets):
        for p in itertools.product(*(range(a) for a in A)):
            me = cell(p)
            if me is None or cell(tuple(x - c for x, c in zip(p, d))) == me:
                continue
            L, q = 0, p
            while cell(q) == me:
                L, q = L + 1, tuple(x + c for x, c in zip(q, d))
            out[me[0], n, me[1], min(L, R) - 1] += 1
            capped[me[0], n] += L > R
    return out, capped


def gldm_brute(vol, label, labels, lo, width, G, alpha, mask=None):
    A = vol.shape
    dep = np.zeros((len(labels), G, NB), dtype=np.int64)
    ngt = np.zeros((len(labels), G, NB, 2), dtype=np.int64)
    for p in itertools.product(*(range(a) for a in A)):
        me = _voxel(vol, label, labels, lo, width, G, mask, p)
        if me is None:
            continue
        n = total = k = 0
        for d in NEIGHBOURS:
            q = tuple(x + c for x, c in zip(p, d))
            if not all(0 <= c < a for c, a in zip(q, A)):
                continue
            other = _voxel(vol, label, labels, lo, width, G, mask, q)
            if other is None or other[0] != me[0]:
                continue
            n, total, k = n + 1, total + other[1], k + (abs(other[1] - me[1]) <= alpha)
        dep[me[0], me[1], k] += 1
        ngt[me[0], me[1], n, 0] += 1
        ngt[me[0], me[1], n, 1] += abs(me[1] * n - total)
    return dep, ngt


# ------------------------------------------------------------------------------------------------ the host features as loops
def _matrix_loop(P, names):
    """One matrix P [G][J] (level i = row + 1, j = column + 1) -> the fourteen features the run-length and the dependence class share."""
    G, J = P.shape
    N = float(P.sum())
    if N == 0:
        return {k: float('nan') for k in names}
    f = dict.fromkeys(names, 0.0)
    short, long_, gln, ln, lnn, glv, lv, ent, low, high, sl, sh, ll, lh = names
    mu_i = sum((i + 1) * float(P[i, j]) / N for i in range(G) for j in range(J))
    mu_j = sum((j + 1) * float(P[i, j]) / N for i in range(G) for j in range(J))
    for i in range(G):
        f[gln] += float(P[i].sum()) ** 2 / N
    for j in range(J):
        f[ln] += float(P[:, j].sum()) ** 2 / N
    f[lnn] = f[ln] / N
    for i in range(G):
        for j in range(J):
            c, a, b = float(P[i, j]), float(i + 1), float(j + 1)
            if c == 0:
                continue
            p = c / N
            f[short] += c / (b * b) / N
            f[long_] += c * b * b / N
            f[glv] += p * (a - mu_i) ** 2
            f[lv] += p * (b - mu_j) ** 2
            f[ent] -= p * math.log2(p)
            f[low] += c / (a * a) / N
            f[high] += c * a * a / N
            f[sl] += c / (a * a * b * b) / N
            f[sh] += c * a * a / (b * b) / N
            f[ll] += c * b * b / (a * a) / N
            f[lh] += c * a * a * b * b / N
    return f


def glrlm_features_loop(P):
    """One run-length matrix [G][R] -> the sixteen features and 'mean_run'."""
    f = _matrix_loop(P, ('SRE', 'LRE', 'GLN', 'RLN', 'RLNN', 'GLV', 'RV', 'RE', 'LGLRE', 'HGLRE', 'SRLGLE', 'SRHGLE', 'LRLGLE', 'LRHGLE'))
    Nr = float(P.sum())
    Np = float(sum((j + 1) * int(P[i, j]) for i in range(P.shape[0]) for j in range(P.shape[1])))
    f['GLNN'] = f['GLN'] / Nr if Nr else float('nan')
    f['RP'] = Nr / Np if Nr else float('nan')
    f['mean_run'] = Np / Nr if Nr else float('nan')
    return f


def gldm_features_loop(P):
    return _matrix_loop(P, ('SDE', 'LDE', 'GLN', 'DN', 'DNN', 'GLV', 'DV', 'DE', 'LGLE', 'HGLE', 'SDLGLE', 'SDHGLE', 'LDLGLE', 'LDHGLE'))


def ngtdm_table_loop(T):
    """One ngt [G][27][2] -> (n_i, s_i) as lists."""
    G = T.shape[0]
    return ([sum(int(T[i, n, 0]) for n in range(1, NB)) for i in range(G)], [sum(int(T[i, n, 1]) / n for n in range(1, NB)) for i in range(G)])


def ngtdm_features_loop(T):
    n, s = ngtdm_table_loop(T)
    G, Nvp = len(n), float(sum(n))
    names = ('coarseness', 'contrast', 'busyness', 'complexity', 'strength')
    if Nvp == 0:
        return {k: float('nan') for k in names}
    p = [x / Nvp for x in n]
    on = [i for i in range(G) if n[i] > 0]
    ps, ssum, Ngp = sum(p[i] * s[i] for i in on), sum(s), len(on)
    pairs = [(i, j) for i in on for j in on]
    f = {'coarseness': 1e6 if ps == 0 else 1.0 / ps}
    f['contrast'] = 0.0 if Ngp == 1 else sum(p[i] * p[j] * (i - j) ** 2 for i, j in pairs) / (Ngp * (Ngp - 1)) * ssum / Nvp
    den = sum(abs((i + 1) * p[i] - (j + 1) * p[j]) for i, j in pairs)
    f['busyness'] = 0.0 if den == 0 else ps / den
    f['complexity'] = sum(abs(i - j) * (p[i] * s[i] + p[j] * s[j]) / (p[i] + p[j]) for i, j in pairs) / Nvp
    f['strength'] = 0.0 if ssum == 0 else sum((p[i] + p[j]) * (i - j) ** 2 for i, j in pairs) / ssum
    return f
