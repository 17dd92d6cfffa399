"""Slice preparation of the inference driver (csrc/infer_prep.hip) at its edges, through the C entries.

hv_slice_components / hv_slice_components_u8 against scipy.ndimage.label with the 3x3 structure (oracle.restate.remove_small_components): the four stats
integers exact, the u8 entry's filtered plane exact.  Every float slice carries distractors in its background (NaN, value + 0.5, value + 1) and every byte
plane carries value - 1, value + 1 and 255 there: none of them may match.  hv_infer_prepare against oracle.restate.infer_prepare on label slices that
produce the hand-placed rows; hv_select_slices, hv_slice_count and hv_volume_scan against numpy.

Every buffer a kernel writes is a hvtest.Guarded buffer, every workspace exactly the queried bytes inside guards; after every call the guards are intact."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T = lib = None
VALUE, V8 = 20.0, 200


@pytest.fixture(scope='module', autouse=True)
def _env():
    global T, lib
    import hvgan  # noqa: F401
    from hvgan import lib as _lib
    import hvtest as _T
    T, lib = _T, _lib
    yield


@pytest.fixture(autouse=True)
def _no_launch_after_a_device_error():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:      # a faulted context fails every later call: end the session instead of launching on
        pytest.exit('device error, nothing more is launched: %s' % e, returncode=3)


_ALIVE = []


@pytest.fixture(autouse=True)
def _release_inputs():
    yield
    del _ALIVE[:]


def dv(a):
    """numpy -> device tensor that lives until the test ends (its pointer is handed to the C entry, often from a temporary)"""
    _ALIVE.append(torch.from_numpy(np.ascontiguousarray(a)).to(T.dev()))
    return _ALIVE[-1]


def bytes_guarded(shape, data=None):
    """a uint8 buffer inside 0xA5 guards (held as int8: the byte sentinel is a signed value); .u8 is the uint8 view"""
    g = T.Guarded(shape, torch.int8, guard=64)
    g.u8 = g.t.view(torch.uint8)
    if data is not None:
        g.u8.copy_(dv(data.astype(np.uint8)))
    return g


# ------------------------------------------------------------------------------------------------------------------------- connected components
def ref_components(mask, min_size):
    """-> ([count, first row, last row, row sum], kept mask) of what remove_small_components leaves"""
    from scipy.ndimage import label as cc_label
    cl, n = cc_label(mask.astype(np.int32), np.ones((3, 3), dtype=np.int32))
    keep = np.bincount(cl.ravel(), minlength=n + 1) >= min_size
    keep[0] = False
    kept = keep[cl]
    rows = np.nonzero(kept)[0].astype(np.int64)
    return ([len(rows), int(rows.min()), int(rows.max()), int(rows.sum())] if len(rows) else [0, -1, -1, 0]), kept


def float_labels(masks):
    S, H, W = masks.shape
    r, c = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    bg = np.array([0.0, VALUE + 1, VALUE + 0.5, np.nan], dtype=np.float32)[(r + 2 * c) % 4]
    return np.where(masks, np.float32(VALUE), bg[None]).astype(np.float32)


def byte_planes(masks):
    S, H, W = masks.shape
    r, c = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    bg = np.array([0, V8 + 1, V8 - 1, 255], dtype=np.uint8)[(r + 2 * c) % 4]
    return np.where(masks, np.uint8(V8), bg[None]).astype(np.uint8)


def run_f32(lab, min_size, value=VALUE):
    L = lib.get()
    S, H, W = lab.shape
    need = L.size('hv_slice_components_workspace_bytes', S, H, W)
    assert need == 2 * S * H * W * 4
    ws, stats = T.Guarded((need,), torch.int8), T.Guarded((S, 4), torch.int32)
    rc = L.cdll.hv_slice_components(lib.ptr(dv(lab)), S, H, W, ctypes.c_float(value), min_size, lib.ptr(stats.t), lib.ptr(ws.t), ctypes.c_size_t(need),
                                    lib.stream())
    torch.cuda.synchronize()
    assert ws.intact() and stats.intact()
    return rc, stats


def run_u8(plane, min_size, value=V8, in_place=False):
    L = lib.get()
    S, H, W = plane.shape
    need = L.size('hv_slice_components_workspace_bytes', S, H, W)
    ws, stats = T.Guarded((need,), torch.int8), T.Guarded((S, 4), torch.int32)
    out = bytes_guarded((S, H, W), data=plane if in_place else None)
    src = out.u8 if in_place else dv(plane)
    rc = L.cdll.hv_slice_components_u8(lib.ptr(src), S, H, W, value, min_size, lib.ptr(stats.t), lib.ptr(out.u8), lib.ptr(ws.t), ctypes.c_size_t(need),
                                       lib.stream())
    torch.cuda.synchronize()
    assert ws.intact() and stats.intact() and out.intact()
    return rc, stats, out


def check(masks, min_size):
    """both entries on the slices `masks` (bool [S][H][W]); -> the expected stats rows"""
    masks = np.ascontiguousarray(masks, dtype=bool)
    ref = [ref_components(m, min_size) for m in masks]
    want = np.array([r[0] for r in ref], dtype=np.int64)
    rc, stats = run_f32(float_labels(masks), min_size)
    assert rc == 0 and np.array_equal(stats.cpu().numpy(), want), ('float', min_size, stats.cpu().numpy(), want)
    filtered = np.stack([r[1] for r in ref]).astype(np.uint8) * np.uint8(V8)
    planes = byte_planes(masks)
    rc, stats, out = run_u8(planes, min_size)
    assert rc == 0 and np.array_equal(stats.cpu().numpy(), want), ('u8', min_size, stats.cpu().numpy(), want)
    assert np.array_equal(out.u8.cpu().numpy(), filtered), ('u8 plane', min_size)
    rc, stats2, out2 = run_u8(planes, min_size, in_place=True)
    assert rc == 0 and torch.equal(stats2.t, stats.t) and torch.equal(out2.u8, out.u8), ('u8 in place', min_size)
    return want


def mirrors(a):
    return np.stack([a, a[::-1], a[:, ::-1], a[::-1, ::-1]])


def serpentine(H, W):
    """a one-pixel path that fills the slice: every other row, joined alternately at the right and the left end"""
    a = np.zeros((H, W), dtype=bool)
    a[0::2] = True
    for k, r in enumerate(range(1, H, 2)):
        a[r, W - 1 if k % 2 == 0 else 0] = True
    return a


def spiral(H, W):
    """a one-pixel path from the corner inwards, one background pixel between its arms"""
    a = np.zeros((H, W), dtype=bool)
    r = c = 0
    dr, dc = 0, 1
    a[0, 0] = True
    while True:
        for _ in range(2):
            nr, nc, fr, fc = r + dr, c + dc, r + 2 * dr, c + 2 * dc
            if 0 <= nr < H and 0 <= nc < W and not a[nr, nc] and not (0 <= fr < H and 0 <= fc < W and a[fr, fc]):
                r, c = nr, nc
                a[r, c] = True
                break
            dr, dc = dc, -dr
        else:
            return a


def comb(H, W):
    a = np.zeros((H, W), dtype=bool)
    a[0] = True
    a[:, ::2] = True
    return a


def staircase(H, W):
    """one pixel per step of the longer axis, bouncing along the shorter: neighbours touch only at corners"""
    a = np.zeros((H, W), dtype=bool)
    n, m = max(H, W), min(H, W)
    for i in range(n):
        j = i % (2 * m - 2) if m > 1 else 0
        j = j if j < m else 2 * m - 2 - j
        a[(i, j) if H >= W else (j, i)] = True
    return a


PATTERNS = {'serpentine': serpentine, 'spiral': spiral, 'comb': comb, 'staircase': staircase}


@pytest.mark.parametrize('shape', [(33, 70), (64, 64), (128, 128)], ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('name', sorted(PATTERNS))
def test_shapes_that_need_many_relabelling_passes(name, shape):
    """One component whose smallest label has to travel the whole path, in its four mirror images (the root at either end of the path).  These are the
    many-pass cases; none of them needs anywhere near the kernel's 4096-pass bound, which stays untested."""
    a = PATTERNS[name](*shape)
    want = check(mirrors(a), 50)
    assert (want[:, 0] == a.sum()).all() and a.sum() >= (max(shape) if name == 'staircase' else shape[0] * shape[1] // 4), (name, want, a.sum())


def test_connectivity_is_eight_and_a_gap_separates():
    m = np.zeros((2, 16, 20), dtype=bool)
    m[0, 2:7, 3:9], m[0, 7:12, 9:15] = True, True           # two 30-pixel blobs that touch only at a corner: one component of 60
    m[1, 2:7, 3:9], m[1, 8:13, 3:9] = True, True            # one background row apart: two components of 30, both below 50
    want = check(m, 50)
    assert list(want[0]) == [60, 2, 11, 30 * 4 + 30 * 9] and list(want[1]) == [0, -1, -1, 0]
    m[1, 2:7, 3:9], m[1, 2:7, 10:16] = True, True           # ... and one background column apart
    assert list(check(m, 31)[1]) == [0, -1, -1, 0]


def test_min_size_boundary():
    m = np.zeros((1, 40, 40), dtype=bool)
    m[0, 1:8, 1:8] = True           # 49
    m[0, 10:15, 1:11] = True        # 50
    m[0, 20:23, 1:18] = True        # 51
    m[0, 30, 30] = True             # 1
    for min_size, count in ((50, 101), (49, 150), (51, 51), (52, 0), (2, 150), (1, 151), (0, 151)):
        assert check(m, min_size)[0, 0] == count, min_size


def test_small_and_degenerate_sizes():
    rng = np.random.RandomState(7)
    for H, W in ((5, 7), (25, 41), (300, 1), (1, 300), (1, 1)):       # fewer pixels than threads; HW = 1025; one column; one row; one pixel
        m = rng.rand(3, H, W) < 0.7
        m[1] = False                                                   # an empty slice between the others
        m[2] = True                                                    # a full slice
        for min_size in (0, 3):
            want = check(m, min_size)
            assert list(want[1]) == [0, -1, -1, 0]
            assert list(want[2]) == ([H * W, 0, H - 1, W * H * (H - 1) // 2] if H * W >= min_size else [0, -1, -1, 0])


def test_float_labels_match_exactly_or_not_at_all():
    m = np.zeros((1, 12, 12), dtype=bool)
    m[0, 3:9, 3:9] = True
    lab = np.where(m, np.float32(VALUE), np.float32(np.nan))          # NaN everywhere else
    rc, stats = run_f32(lab, 1)
    assert rc == 0 and stats.cpu().tolist() == [[36, 3, 8, 6 * (3 + 4 + 5 + 6 + 7 + 8)]]
    rc, stats = run_f32(np.where(m, np.float32(VALUE + 0.5), np.float32(np.nan)), 0)      # value + 0.5 and NaN only
    assert rc == 0 and stats.cpu().tolist() == [[0, -1, -1, 0]]
    rc, stats = run_f32(lab, 0, value=float('nan'))                   # a NaN value matches nothing, NaN pixels included
    assert rc == 0 and stats.cpu().tolist() == [[0, -1, -1, 0]]


def test_u8_value_range():
    plane = byte_planes(np.ones((1, 8, 8), dtype=bool))
    for value in (0, 256, -1):
        rc, stats, out = run_u8(plane, 1, value=value)
        assert rc == -1 and bool((stats.t == stats.sentinel).all()) and bool((out.t == out.sentinel).all()), value
    rc, stats, out = run_u8(np.full((1, 8, 8), 255, np.uint8), 1, value=255)
    assert rc == 0 and stats.cpu().tolist() == [[64, 0, 7, 8 * 28]] and bool((out.u8 == 255).all())


def test_row_sum_bound_the_tallest_column():
    """stats[3], the shared sum and the per-thread sums are ints: a full H x 1 column sums to H (H - 1) / 2, which is 2 147 450 880 <= INT_MAX at
    H = 65536 and 2 147 516 416 > INT_MAX at H = 65537.  The first is the tallest column accepted and its sum is exact."""
    m = np.ones((1, 65536, 1), dtype=bool)
    rc, stats = run_f32(float_labels(m), 50)
    assert rc == 0 and stats.cpu().tolist() == [[65536, 0, 65535, 2147450880]]
    rc, stats, out = run_u8(byte_planes(m), 50)
    assert rc == 0 and stats.cpu().tolist() == [[65536, 0, 65535, 2147450880]] and bool((out.u8 == V8).all())


def test_row_sum_bound_refuses_what_would_wrap():
    m = np.ones((1, 65537, 1), dtype=bool)
    rc, stats = run_f32(float_labels(m), 50)
    assert rc == -2 and bool((stats.t == stats.sentinel).all()), (rc, stats.cpu().tolist())
    rc, stats, out = run_u8(byte_planes(m), 50)
    assert rc == -2 and bool((stats.t == stats.sentinel).all()) and bool((out.t == out.sentinel).all()), (rc, stats.cpu().tolist())


# ---------------------------------------------------------------------------------------------------------------------------- hv_infer_prepare
PH, PW = 64, 13


def block(r0, r1, narrow_from=None):
    """label slice: rows r0..r1 (inclusive) over the full width, from row narrow_from on only three columns wide (moves the mean row up)"""
    lab = np.zeros((PH, PW), dtype=np.float32)
    lab[r0:r1 + 1] = VALUE
    if narrow_from is not None:
        lab[narrow_from:r1 + 1] = 0
        lab[narrow_from:r1 + 1, 5:8] = VALUE
    return lab


def stats_of(lab):
    rows = np.nonzero(lab == VALUE)[0]
    assert len(rows) >= 50
    return [len(rows), int(rows.min()), int(rows.max()), int(rows.sum())]


def slices(seed, S):
    rng = np.random.RandomState(seed)
    ct, cam = rng.uniform(0, 255.99, (S, PH, PW)), rng.uniform(0, 255.99, (S, PH, PW))
    for k, v in enumerate((0.0, 0.99, 254.999, 255.99)):      # quantisation: truncation to 0, 0, 254, 255 -- in a restacked row and in a band row
        for r in (1, 30, PH - 2):
            ct[:, r, 2 * k], cam[:, r, 2 * k + 1] = v, v
    return ct.astype(np.float32), cam.astype(np.float32)


def run_prepare(ct, cam, stats, maxheight, selected=None):
    L = lib.get()
    S, H, W = ct.shape
    planes = T.Guarded((4, S, 1, H, W))
    rows = [T.Guarded((S,), torch.int64) for _ in range(3)]
    valid = T.Guarded((S,), torch.int32)
    rc = L.cdll.hv_infer_prepare(lib.ptr(dv(ct)), lib.ptr(dv(cam)), lib.ptr(dv(np.asarray(stats, dtype=np.int32))),
                                 None if selected is None else lib.ptr(dv(np.asarray(selected, dtype=np.int32))), S, H, W, maxheight,
                                 *[lib.ptr(planes.t[k]) for k in range(4)], *[lib.ptr(g.t) for g in rows], lib.ptr(valid.t), lib.stream())
    torch.cuda.synchronize()
    assert planes.intact() and valid.intact() and all(g.intact() for g in rows), 'wrote outside the planes / row tables'
    return rc, planes, [g.cpu().tolist() for g in rows], valid.cpu().tolist()


def compare_with_oracle(labs, ct, cam, maxheight, selected=None):
    from oracle import restate as R
    S = len(labs)
    rc, planes, (x1, x2, height), valid = run_prepare(ct, cam, [stats_of(l) for l in labs], maxheight, selected)
    assert rc == 0
    pl = planes.cpu()
    bands = []
    for s in range(S):
        q = R.infer_prepare(cam[s].astype(np.float64), labs[s].astype(np.float64), ct[s].astype(np.float64), VALUE, maxheight)
        assert torch.equal(pl[1, s], q['ori_ct']), s
        if selected is not None and not selected[s]:
            assert valid[s] == 0 and (x1[s], x2[s], height[s]) == (0, 0, PH), s
            assert bool((pl[0, s] == -1).all()) and bool((pl[2, s] == 0).all()) and bool((pl[3, s] == 0).all()), s
            bands.append(None)
            continue
        assert valid[s] == 1 and (x1[s], x2[s], height[s]) == (q['x1'], q['x2'], q['height']), (s, x1[s], x2[s], height[s], q['x1'], q['x2'], q['height'])
        assert torch.equal(pl[0, s], q['ct_batch']) and torch.equal(pl[2, s], q['mask_batch']) and torch.equal(pl[3, s], q['cam']), s
        band = np.flatnonzero(q['mask_batch'][0, :, 0].numpy())
        bands.append((int(band.min()), int(band.max())))
    return bands


def test_prepare_at_the_clamps_and_the_window_switch():
    """maxheight 40 on 64 x 13 slices (HW = 832, no multiple of 256).  Band rows [min_x, max_x] as the mask plane shows them."""
    ct, cam = slices(3, 4)
    # centre row (x1 + x2) // 2 = 20 = maxheight / 2: the top clamp holds; one row lower it does not
    # centre row 44, 2 * (64 - 44) = 40: the bottom clamp holds; one row higher (43) it does not
    labs = [block(10, 30), block(11, 31), block(34, 54), block(33, 53)]
    assert compare_with_oracle(labs, ct, cam, 40) == [(0, 40), (1, 41), (24, 63), (23, 63)]
    # a vertebra against the last row, and one against the first: deep inside either clamp
    # height == 40: the rows as they are; height == 41: the 40-row window around the mean row 23 (x1 = 3, x2 = 43, height stays 41)
    labs = [block(50, 63), block(0, 9), block(10, 50, narrow_from=26), block(10, 51, narrow_from=26)]
    assert compare_with_oracle(labs, ct, cam, 40) == [(24, 63), (0, 40), (10, 50), (3, 43)]
    # maxheight == H: the band is the whole slice, nothing is restacked
    assert compare_with_oracle(labs, ct, cam, PH) == [(0, 63)] * 4
    # slices the stage does not run on
    bands = compare_with_oracle(labs, ct, cam, 40, selected=[1, 0, 0, 1])
    assert bands == [(24, 63), None, None, (3, 43)]


def test_prepare_with_a_mean_row_below_twenty():
    """A vertebra taller than maxheight whose mean row is 14: the window starts at x1 = -6.  With maxheight 40 the centre row stays inside the top clamp, every
    restacked row has its source inside the image and oracle.restate.infer_prepare states the result.  With maxheight 20 the band [4, 24] leaves rows whose
    source lies above the first or below the last image row; the oracle raises on the shape mismatch there, the device writes the zero byte (-1 after
    Normalize for the CT plane, 0 for the CAM plane) -- and in both cases nothing outside the planes is touched (the guards, checked in run_prepare)."""
    from oracle import restate as R
    ct, cam = slices(4, 1)
    lab = block(0, 45, narrow_from=10)
    assert stats_of(lab) == [238, 0, 45, 3555]
    assert compare_with_oracle([lab], ct, cam, 40) == [(0, 40)]
    with pytest.raises(ValueError):
        R.infer_prepare(cam[0].astype(np.float64), lab.astype(np.float64), ct[0].astype(np.float64), VALUE, 20)
    rc, planes, (x1, x2, height), valid = run_prepare(ct, cam, [stats_of(lab)], 20)
    assert rc == 0 and valid == [1] and (x1, x2, height) == ([-6], [34], [45])
    min_x, max_x = R.dataset_band(-6, 34, PH, 20)
    assert (min_x, max_x) == (4, 24)
    u8 = lambda a: a.astype(np.uint8)
    ect, ecam = np.zeros((PH, PW), np.uint8), np.zeros((PH, PW), np.uint8)      # rows 0..3 come from rows -10..-7: outside
    ect[24:54], ecam[24:54] = u8(ct[0, 34:64]), u8(cam[0, 34:64])             # rows 24..53 from rows 34..63; rows 54..63 from rows 64..73: outside
    emask = np.zeros((PH, PW), np.uint8)
    emask[4:25] = 255
    pl = planes.cpu()
    assert torch.equal(pl[0, 0], R.to_tensor_u8(ect, True)) and torch.equal(pl[3, 0], R.to_tensor_u8(ecam, False))
    assert torch.equal(pl[2, 0], R.to_tensor_u8(emask, False)) and torch.equal(pl[1, 0], R.to_tensor_u8(u8(ct[0]), True))


def test_prepare_refusals():
    ct, cam = slices(5, 1)
    st = [stats_of(block(10, 30))]
    for maxheight in (39, PH + 2, 0):
        rc, planes, _, _ = run_prepare(ct, cam, st, maxheight)
        assert rc == -1 and bool(torch.isnan(planes.t).all()), maxheight
    L = lib.get()
    planes, rows, valid = T.Guarded((4, 1, 1, PH, PW)), T.Guarded((3, 1), torch.int64), T.Guarded((1,), torch.int32)
    rc = L.cdll.hv_infer_prepare(lib.ptr(dv(ct)), lib.ptr(dv(cam)), lib.ptr(dv(np.asarray(st, dtype=np.int32))), None, 65536, PH, PW, 40,
                                 *[lib.ptr(planes.t[k]) for k in range(4)], *[lib.ptr(rows.t[k]) for k in range(3)], lib.ptr(valid.t), lib.stream())
    torch.cuda.synchronize()
    assert rc == -1 and bool(torch.isnan(planes.t).all()) and planes.intact() and rows.intact() and valid.intact()
    assert bool((rows.t == rows.sentinel).all()) and bool((valid.t == valid.sentinel).all())


# ------------------------------------------------------------------------------------------------------------------------- the small neighbours
@pytest.mark.parametrize('per', [1, 255, 256, 257])
def test_select_and_count_around_one_workgroup_pass(per):
    L = lib.get()
    S = 3
    rng = np.random.RandomState(per)
    src = rng.rand(S, per).astype(np.float32)
    old = rng.rand(S, per).astype(np.float32)
    flag = np.array([1, 0, 5], dtype=np.int32)
    for keep in (1, 0):
        dst = T.Guarded((S, per), data=torch.from_numpy(old))
        L.call('hv_select_slices', lib.ptr(dv(flag)), lib.ptr(dv(src)), lib.ptr(dst.t), S, ctypes.c_longlong(per), keep, lib.stream())
        torch.cuda.synchronize()
        want = src.copy()
        want[1] = old[1] if keep else 0
        assert dst.intact() and np.array_equal(dst.cpu().numpy(), want), (per, keep)
    lab = rng.choice(np.array([8, 9, 9.5, np.nan], dtype=np.float32), size=(S, per))
    lab[0] = np.nan                                                    # a slice of NaN labels
    lab[2] = 9
    for value, want in ((9.0, (lab == 9).sum(axis=1)), (float('nan'), np.zeros(S))):
        cnt = T.Guarded((S,), torch.int32)
        L.call('hv_slice_count', lib.ptr(dv(lab)), S, ctypes.c_longlong(per), ctypes.c_float(value), lib.ptr(cnt.t), lib.stream())
        torch.cuda.synchronize()
        assert cnt.intact() and np.array_equal(cnt.cpu().numpy(), want.astype(np.int32)), (per, value)
    assert list((lab == 9).sum(axis=1))[::2] == [0, per]


def test_volume_scan_at_the_histogram_limit():
    L = lib.get()
    rng = np.random.RandomState(11)
    HW, Z = 5, 2048
    label = rng.choice([0.0, 7.0, 8.0, 9.0, 20.0], size=(HW, Z))
    label[:, Z - 1] = 8.0                                             # the last bin of each histogram row
    counts = T.Guarded((3 * Z,), torch.int32)
    L.call('hv_volume_scan', lib.ptr(dv(label)), ctypes.c_longlong(HW), Z, ctypes.c_double(8.0), ctypes.c_double(7.0), ctypes.c_double(20.0),
           lib.ptr(counts.t), lib.stream())
    torch.cuda.synchronize()
    want = np.stack([(label == v).sum(axis=0) for v in (8.0, 7.0, 20.0)]).astype(np.int32)
    assert counts.intact() and np.array_equal(counts.cpu().numpy().reshape(3, Z), want) and want[0, Z - 1] == HW
    Z = 2049                                                          # one slice more than the histogram in LDS holds: refused, counts untouched
    counts = T.Guarded((3 * Z,), torch.int32)
    rc = L.cdll.hv_volume_scan(lib.ptr(dv(np.ones((HW, Z)))), ctypes.c_longlong(HW), Z, ctypes.c_double(8.0), ctypes.c_double(7.0),
                               ctypes.c_double(20.0), lib.ptr(counts.t), lib.stream())
    torch.cuda.synchronize()
    assert rc == -1 and counts.intact() and bool((counts.t == counts.sentinel).all())
