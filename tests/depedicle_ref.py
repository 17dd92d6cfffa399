"""Plain-numpy restatement of the de-pedicling rule (csrc/depedicle.hip; include/hvgan.h hv_depedicle), pinned against the reference's own
process_3d_array / find_single_component_layers by fixture G17 (tools/make_golden_depedicle.py).  No scipy: a flood fill per component.

Per slice [:, :, z] with the raster index p = i0 * A1 + i1: pixels are joined iff they are 4-neighbours holding the same non-zero value; a
component's identity is its smallest raster index (the flood fills start in raster order, so the first pixel met is the identity); per value
the component with the smallest (min i1, identity) stays, every other pixel of that value becomes 0."""
import numpy as np


def components(layer):
    """-> [(value, root, min_i1, [raster indices])] of one 2-D layer, in raster order of the roots."""
    layer = np.asarray(layer)
    A0, A1 = layer.shape
    flat = layer.reshape(-1)
    seen = np.zeros(A0 * A1, dtype=bool)
    out = []
    for p in np.flatnonzero(flat):
        if seen[p]:
            continue
        v = flat[p]
        seen[p] = True
        stack, pix = [int(p)], []
        while stack:
            q = stack.pop()
            pix.append(q)
            i0, i1 = divmod(q, A1)
            for ok, n in ((i1 > 0, q - 1), (i1 + 1 < A1, q + 1), (i0 > 0, q - A1), (i0 + 1 < A0, q + A1)):
                if ok and not seen[n] and flat[n] == v:
                    seen[n] = True
                    stack.append(n)
        out.append((int(v), int(p), min(q % A1 for q in pix), pix))
    return out


def depedicle_layer(layer):
    """-> (processed layer uint8, counts int32 [256])"""
    layer = np.asarray(layer)
    res = np.zeros(layer.shape, dtype=np.uint8)
    counts = np.zeros(256, dtype=np.int32)
    best = {}
    for v, root, lo, pix in components(layer):
        counts[v] += 1
        if v not in best or (lo, root) < best[v][:2]:
            best[v] = (lo, root, pix)
    flat = res.reshape(-1)
    for v, (_, _, pix) in best.items():
        flat[pix] = v
    return res, counts


def depedicle(vol):
    """-> (uint8 volume, counts [Z, 256]) of a [A0, A1, Z] volume."""
    vol = np.asarray(vol)
    out = np.zeros(vol.shape, dtype=np.uint8)
    counts = np.zeros((vol.shape[2], 256), dtype=np.int32)
    for z in range(vol.shape[2]):
        out[:, :, z], counts[z] = depedicle_layer(vol[:, :, z])
    return out, counts


def single_component_range(counts, label, offset=10):
    """find_single_component_layers from the counts [Z, 256]: the walk from mid -+ offset outwards (start indices clamped), defaults 1 / 128."""
    col = counts[:, int(label)] if 1 <= int(label) <= 255 else np.zeros(len(counts), dtype=np.int32)
    Z = len(col)
    mid = Z // 2
    z0, z1 = 1, 128
    for i in range(max(0, mid - offset), -1, -1):
        if col[i] == 1:
            z0 = i
            break
    for i in range(min(Z - 1, mid + offset), Z):
        if col[i] == 1:
            z1 = i
            break
    return z0, z1


# ------------------------------------------------------------------------------------------------ worst-case shapes for the labelling
def spiral(n):
    """A one-pixel-wide square spiral filling n x n, from the corner (0, 0) inwards: one 4-connected component whose arms lie one pixel
    apart.  A turtle walks ahead while the next cell is free and the one after it is not part of an earlier arm, else it turns right."""
    a = np.zeros((n, n), dtype=np.uint8)
    r, c, dr, dc = 0, 0, 0, 1
    a[0, 0] = 1

    def free(dr, dc):
        r1, c1, r2, c2 = r + dr, c + dc, r + 2 * dr, c + 2 * dc
        if not (0 <= r1 < n and 0 <= c1 < n) or a[r1, c1]:
            return False
        return not (0 <= r2 < n and 0 <= c2 < n and a[r2, c2])
    while True:
        if not free(dr, dc):
            dr, dc = dc, -dr
            if not free(dr, dc):
                return a
        r, c = r + dr, c + dc
        a[r, c] = 1


def comb(n, teeth):
    """A comb in n x n: a spine along row 0 and `teeth` one-pixel-wide teeth hanging from it on every second column."""
    a = np.zeros((n, n), dtype=np.uint8)
    a[0, :2 * teeth - 1] = 1
    a[:, 0:2 * teeth:2] = 1
    return a
