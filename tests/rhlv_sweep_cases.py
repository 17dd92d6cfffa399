"""Shared inputs and CPU references of the RHLV parameter-sweep tests (tests/test_rhlv_sweep_cpu.py, tests/test_rhlv_sweep_gpu.py): fixture
G18 (the reference's two scripts at every grid point, tools/make_golden_rhlv_sweep.py), small random pairs at the shapes where the sweep kernels
change path, and each grid point's record by the float64 restatement tests/height_map_ref.py -- computed once per process and left unchanged."""
import functools

import numpy as np

from conftest import load_golden
import height_map_ref as M

VIEWS = ('sagittal', 'coronal')
IDX = 7
# the grid of the bit-identity tests
THRESHOLDS = (0.3, 0.64, 0.7, 0.95, 1.0)
DIVISORS = (1, 2, 5, 8, 1000)
# (H, W, Z), z fastest in memory: one block per slice; W > 256 lanes (the strided column loops of the sagittal view); the same for the coronal
# view; the z-fastest counts kernel (the other shapes are stored z slowest)
SHAPES = (((9, 37, 21), False), ((5, 300, 7), False), ((5, 7, 300), False), ((12, 64, 64), True))
PAIRS = 3


@functools.lru_cache(maxsize=None)
def g18():
    g = {k: np.asarray(v) for k, v in load_golden('g18_rhlv_sweep').items()}
    return g, sorted({k.split('/')[0] for k in g if '/' in k})


def reference_record(fake, label, idx, divisor, threshold, view):
    """-> (hv_rhlv_views' record [:14] by the restatement, raised) at one setting; the record of an absent original is zeros."""
    m = M.view_maps(fake, label, idx, divisor, threshold, view)
    rec = np.zeros(14)
    if m is None:
        return rec, False
    res, means = M.reduce_selected(m['selected'])
    rec[:5], rec[5:13], rec[13] = res, means, 1.0
    return rec, bool(m['raises'])


def random_pair(seed, H, W, Z):
    """uint8 id volumes [H, W, Z]: a vertebra (id IDX) of random column heights over nearly the whole [W, Z] footprint, the original wedge-
    compressed along w and partly taller than the generated one, a neighbour id above it."""
    rng = np.random.default_rng(seed)
    inside = np.zeros((W, Z), dtype=bool)
    mw, mz = int(W >= 16), int(Z >= 16)                 # a short axis is filled: its few slices must give the divisors different ranges
    inside[mw * (1 + seed % 2):W - mw, mz:Z - mz * (1 + seed % 2)] = True
    hf = rng.integers(1, H + 1, size=(W, Z)) * inside
    wedge = 1.0 - 0.6 * (seed % 3) / 2 * np.linspace(1.0, 0.0, W)[:, None]
    hl = np.clip(np.round(hf * wedge + rng.integers(-1, 2, size=(W, Z))), 0, H).astype(np.int64) * inside
    hl[W // 2, Z // 2] = max(1, hl[W // 2, Z // 2])
    rows = np.arange(H)[:, None, None]
    fake = np.where(rows < hf[None], IDX, np.where(rows == H - 1, IDX + 1, 0)).astype(np.uint8)
    label = np.where(rows < hl[None], IDX, np.where(rows == H - 1, IDX + 1, 0)).astype(np.uint8)
    return fake, label


@functools.lru_cache(maxsize=None)
def random_case(shape_no):
    """-> (fakes, labels: PAIRS uint8 volumes each, reference records [PAIRS, D, T, 2, 14], raised [PAIRS, D], wraps [PAIRS, 2]: divisor 1 drives
    centre - length negative in that view)."""
    (H, W, Z), _ = SHAPES[shape_no]
    fakes, labels = zip(*(random_pair(40 + 10 * shape_no + k, H, W, Z) for k in range(PAIRS)))
    rec = np.zeros((PAIRS, len(DIVISORS), len(THRESHOLDS), 2, 14))
    raised = np.zeros((PAIRS, len(DIVISORS)), dtype=bool)
    wraps = np.zeros((PAIRS, 2), dtype=bool)
    for k in range(PAIRS):
        for v, view in enumerate(VIEWS):
            centre, length = M.slice_range(M.column_table(labels[k], IDX, view).sum(axis=1), DIVISORS[0])
            wraps[k, v] = centre - length < 0
            for d, div in enumerate(DIVISORS):
                for t, thr in enumerate(THRESHOLDS):
                    rec[k, d, t, v], r = reference_record(fakes[k], labels[k], IDX, div, thr, view)
                    raised[k, d] |= r and view == 'coronal'
    return fakes, labels, rec, raised, wraps


def distinct(records):
    """Number of distinct records among [..., n] rows."""
    return len({np.ascontiguousarray(r).tobytes() for r in records.reshape(-1, records.shape[-1])})
