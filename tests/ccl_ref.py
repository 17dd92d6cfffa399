"""The reference of the 3-D connected-component tests (csrc/ccl3d.hip: hv_label3d, hv_clean_components, hv_fill_holes; DESIGN.md section 8
row f10): scipy.ndimage.label with generate_binary_structure(3, c), np.bincount, binary_fill_holes, the filter rules in numpy -- all integers,
so every comparison is exact -- and a small numpy restatement of the device's scheme (tile-local unions, seam unions, smallest-index roots,
rank numbering) for an arbitrary tile shape, with the cases the CPU and GPU tests share."""
import itertools

import numpy as np
from scipy.ndimage import binary_fill_holes, generate_binary_structure
from scipy.ndimage import label as nd_label


def label(mask, connectivity=1):
    """-> (labels int32, n): scipy's labelling of a boolean volume."""
    lab, n = nd_label(np.asarray(mask, dtype=bool), generate_binary_structure(3, connectivity))
    return lab.astype(np.int32), int(n)


def sizes(lab, n):
    return np.bincount(lab.ravel(), minlength=n + 1)[1:].astype(np.int64)


def table(mask, connectivity=1, cap=0):
    """What hv_label3d leaves in its table: [n, largest label, its size, status] + `cap` sizes."""
    lab, n = label(mask, connectivity)
    s = sizes(lab, n)
    t = np.zeros(4 + cap, dtype=np.int32)
    t[0] = n
    if n:
        t[1] = int(np.argmax(s)) + 1                       # ties: the lowest label
        t[2] = s[t[1] - 1]
    t[3] = 0 if n else 1
    m = min(n, cap)
    t[4:4 + m] = s[:m]
    return lab, t


def clean(vol, value, connectivity=1, min_size=0, keep_largest=True, fill=0):
    """The filter of hv_clean_components: components of vol == value with fewer than min_size voxels (the reference's
    `np.sum(labeled == i) < min_size`) and, with keep_largest, all but the largest become `fill`."""
    vol = np.asarray(vol)
    lab, t = table(vol == value, connectivity)
    n = int(t[0])
    drop = np.zeros(n + 1, dtype=bool)
    if min_size > 1:
        drop[1:] |= sizes(lab, n) < min_size
    if keep_largest:
        drop[1:] |= np.arange(1, n + 1) != t[1]
    out = vol.copy()
    out[drop[lab]] = fill
    return out, t


def fill_holes(vol, value):
    """-> (vol with the holes of vol == value set to value, number of holes, voxels filled)."""
    vol = np.asarray(vol)
    m = vol == value
    filled = binary_fill_holes(m)
    holes = filled & ~m
    out = vol.copy()
    out[holes] = value
    return out, label(holes, 1)[1], int(holes.sum())


def clean_label(vol, value, connectivity=1, min_size=0, keep_largest=True, holes=False, fill=0):
    out, t = clean(vol, value, connectivity, min_size, keep_largest, fill)
    if holes:
        out = fill_holes(out, value)[0]
    return out, t


def backward_offsets(connectivity):
    """The neighbour offsets that precede (0, 0, 0) in raster order: 3, 9 or 13 of them."""
    return [d for d in itertools.product((-1, 0, 1), repeat=3) if d < (0, 0, 0) and sum(x != 0 for x in d) <= connectivity]


def restate(mask, connectivity, tile):
    """The device's scheme in numpy: union-find whose links always point to the smaller raster index; first the pairs of backward neighbours
    inside one tile, then the pairs that cross a tile's face, edge or corner; the root of a set is its smallest index; the roots are numbered
    in raster order.  -> (labels int32, n)."""
    mask = np.asarray(mask, dtype=bool)
    A = mask.shape
    parent = np.where(mask.ravel(), np.arange(mask.size), -1)

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    def union(a, b):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)

    idx = np.argwhere(mask)
    offs = backward_offsets(connectivity)
    for seam in (False, True):
        for p in idx:
            for d in offs:
                q = p + d
                if (q < 0).any() or (q >= A).any() or not mask[tuple(q)]:
                    continue
                if ((p // tile != q // tile).any()) == seam:
                    union(int(np.ravel_multi_index(tuple(p), A)), int(np.ravel_multi_index(tuple(q), A)))
    roots = np.array([find(x) if parent[x] >= 0 else -1 for x in range(mask.size)])
    is_root = roots == np.arange(mask.size)
    rank = np.cumsum(is_root)                                   # 1-based rank at each root
    lab = np.where(roots >= 0, rank[np.maximum(roots, 0)], 0).astype(np.int32)
    return lab.reshape(A), int(is_root.sum())


def random_mask(shape, density, seed):
    return np.random.RandomState(seed).rand(*shape) < density


def checkerboard(shape):
    i, j, k = np.ogrid[:shape[0], :shape[1], :shape[2]]
    return (i + j + k) % 2 == 0


def serpentine(shape):
    """One 1-voxel-wide 6-connected path: along axis 2 on every second row of every second slice, the rows joined alternately at their two
    ends, the slices where the last row stops, the rows of every second slice taken in descending order.  It starts at raster index 0, its
    smallest.  -> (mask, number of voxels)."""
    A0, A1, A2 = shape
    m = np.zeros(shape, dtype=bool)
    rows, slices = list(range(0, A1, 2)), list(range(0, A0, 2))
    k_at = 0                                                    # where the path stands along axis 2
    for si, i in enumerate(slices):
        order = rows if si % 2 == 0 else rows[::-1]
        for ri, j in enumerate(order):
            m[i, j, :] = True                                   # the row, walked from k_at to its other end
            k_at = A2 - 1 - k_at
            if ri + 1 < len(order):
                j2 = order[ri + 1]
                m[i, min(j, j2):max(j, j2) + 1, k_at] = True
        if si + 1 < len(slices):
            m[i:i + 3, order[-1], k_at] = True
    return m, int(m.sum())


def ellipsoid(shape, centre, radii):
    g = np.ogrid[:shape[0], :shape[1], :shape[2]]
    return sum(((g[a] - centre[a]) / radii[a]) ** 2 for a in range(3)) <= 1.0


def full_size_case(seed=3):
    """256 x 256 x 64 uint8: an ellipsoid body of label 20, 300 random speckle voxels and two detached fragments of the same label, a second
    label beside them."""
    shape = (256, 256, 64)
    v = np.zeros(shape, dtype=np.uint8)
    v[ellipsoid(shape, (150.0, 128.0, 31.5), (40.0, 60.0, 27.0))] = 20
    v[ellipsoid(shape, (60.0, 128.0, 31.5), (25.0, 50.0, 20.0))] = 19
    v[ellipsoid(shape, (220.0, 40.0, 12.0), (6.0, 5.0, 4.0))] = 20
    v[ellipsoid(shape, (210.0, 220.0, 50.0), (3.0, 7.0, 5.0))] = 20
    r = np.random.RandomState(seed)
    v[r.randint(0, 256, 300), r.randint(0, 256, 300), r.randint(0, 64, 300)] = 20
    return v
