"""A numpy restatement of scipy.ndimage.rank_filter on a 3-D array for a footprint given as integer offsets from the window's centre: what
csrc/rankfilt.hip computes.  Extend by the index map (filter_ref.index_map), gather the footprint's cells, sort, take the rank.
tests/test_rank_filters_ref_cpu.py pins it against scipy by np.array_equal and equal dtype on inputs without NaN or -0.0;
tests/test_rank_filters_gpu.py compares the device against it."""
import numpy as np

from filter_ref import MODES, index_map  # noqa: F401

DTYPES = (np.uint8, np.int16, np.float32, np.float64)
SHAPES = ((5, 6, 7), (1, 3, 2), (2, 1, 9))
CVAL = 7


def windows(a, offsets, mode='reflect', cval=0):
    """a [A0][A1][A2] -> [A0][A1][A2][n]: for every voxel p the extended volume at p + o, o running over the offsets in their order.
    cval must be a value of a's dtype."""
    a = np.asarray(a)
    off = np.asarray(offsets, dtype=np.int64).reshape(-1, 3)
    lo = np.maximum(0, -off.min(axis=0))
    hi = np.maximum(0, off.max(axis=0))
    ext = a
    for ax in range(3):
        n = a.shape[ax]
        idx = index_map(np.arange(-lo[ax], n + hi[ax]), n, mode)
        ext = np.take(ext, np.maximum(idx, 0), axis=ax)
        if mode == 'constant':
            sel = [slice(None)] * 3
            sel[ax] = idx < 0
            ext[tuple(sel)] = np.asarray(cval).astype(a.dtype)
    A = a.shape
    return np.stack([ext[lo[0] + o[0]:lo[0] + o[0] + A[0], lo[1] + o[1]:lo[1] + o[1] + A[1], lo[2] + o[2]:lo[2] + o[2] + A[2]] for o in off],
                    axis=-1)


def rank_filter(a, offsets, rank, mode='reflect', cval=0):
    """The rank-th smallest (0-based; negative: from the end) of every window -> an array of a's shape and dtype."""
    w = np.sort(windows(a, offsets, mode, cval), axis=-1)
    return np.ascontiguousarray(w[..., rank])


def box_offsets(shape, origin=(0, 0, 0), footprint=None):
    """The offsets of the cells of a box (or of the True cells of `footprint`) from the centre shape // 2 + origin, in C order."""
    fp = np.ones(shape, dtype=bool) if footprint is None else np.asarray(footprint, dtype=bool)
    return np.argwhere(fp) - (np.array(fp.shape) // 2 + np.array(origin))


def volume(shape, dtype, seed=0):
    """Few distinct values, so that windows hold ties."""
    r = np.random.RandomState(seed + 7 * sum(shape))
    if np.dtype(dtype).kind == 'f':
        return (r.randint(-40, 40, shape) * 0.37).astype(dtype)
    if np.dtype(dtype) == np.uint8:
        return r.randint(0, 60, shape).astype(np.uint8)
    return r.randint(-300, 300, shape).astype(np.int16)


def same_bytes(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()
