"""View-general volume inference (infer.VolumePipeline(view=...), device-resident inputs and outputs) and its three C entries
hv_volume_scan_view / hv_volume_slices_view / hv_volume_merge_view.

The kernels move and count values: every check is exact (integer counts, C casts, copies).  The coronal view of a volume equals the sagittal view of
the volume with axes 1 and 2 swapped -- the same planes, the same batch, the same kernels after the intake -- so the pipeline checks are exact too."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F64, F32, U8 = 5, 4, 0              # HV_DT_* of include/hvgan.h
NP = {F64: np.float64, F32: np.float32, U8: np.uint8}
CHAIN_NZ = 12            # slices of the RHLV chain's volume: rhlv_volume on the synthesized 12-slice volume returns numbers in both views (asserted there)


def _lib():
    import hvgan  # noqa: F401
    from hvgan import lib
    return lib, lib.get(), torch.device('cuda:0')


def _upload(a, dev, offset=0):
    """Device copy of a numpy array, `offset` elements into its allocation (offset 1: rows that no vector access may touch)."""
    buf = torch.empty(a.size + offset, dtype=torch.from_numpy(a[:0].ravel()).dtype, device=dev)
    t = buf[offset:].view(a.shape)
    t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return t


def _slice_range(n):
    """k0, S: a range inside the axis that leaves both ends out and, where the axis is long enough, crosses the 32-slice tile of the axis-2 kernels."""
    return (5, 33) if n >= 40 else (2, n - 4)


def _take(vol, axis, k0, S):
    """The slices k0 .. k0 + S - 1 as [S][A0][C] float32, in numpy's words."""
    if axis == 1:
        return np.ascontiguousarray(vol[:, k0:k0 + S, :].astype(np.float32).transpose(1, 0, 2))
    return np.ascontiguousarray(vol[:, :, k0:k0 + S].astype(np.float32).transpose(2, 0, 1))


# [37, 45, 29]: odd rows, no axis a multiple of any tile (scalar rows); [16, 9, 64]: aligned rows of 64 (the 4-wide path); the same one element into its
# allocation: A2 % 4 == 0 but no row start is aligned (scalar path again)
@pytest.mark.parametrize('dtype', [F64, F32, U8])
@pytest.mark.parametrize('shape,offset', [((37, 45, 29), 0), ((16, 9, 64), 0), ((16, 9, 64), 1)])
def test_view_kernels_match_numpy(shape, offset, dtype):
    lib, L, dev = _lib()
    ptr, stream = lib.ptr, lib.stream
    rng = np.random.RandomState(3)
    A0, A1, A2 = shape
    label = rng.choice([0, 0, 0, 7, 8, 9, 20], size=shape).astype(NP[dtype])
    ct = rng.uniform(0, 255.99, size=shape).astype(NP[dtype])
    dl, dc = _upload(label, dev, offset), _upload(ct, dev, offset)
    for axis in (2, 1):
        N = shape[axis]
        other = tuple(a for a in range(3) if a != axis)
        counts = torch.full((3 * N,), -1, dtype=torch.int32, device=dev)
        L.call('hv_volume_scan_view', ptr(dl), dtype, A0, A1, A2, axis, 8.0, 7.0, -1.0, ptr(counts), stream())
        got = counts.cpu().numpy().reshape(3, N)
        assert np.array_equal(got[0], (label == 8).sum(axis=other)) and np.array_equal(got[1], (label == 7).sum(axis=other)), (axis, 'counts')
        assert not got[2].any()                                                           # the third id is unused
        k0, S = _slice_range(N)
        C = shape[3 - axis]
        out = torch.full((S * A0 * C + offset,), -3.0, dtype=torch.float32, device=dev)[offset:].view(S, A0, C)
        L.call('hv_volume_slices_view', ptr(dc), dtype, A0, A1, A2, axis, k0, S, ptr(out), stream())
        want = _take(ct, axis, k0, S)
        assert np.array_equal(out.cpu().numpy(), want), (axis, 'slices')
        f = (rng.rand(S) > 0.3).astype(np.int32)
        f[1] = 0
        flag = torch.from_numpy(f).to(dev)
        merged = {}
        for odt, tdt in ((F64, torch.float64), (F32, torch.float32)):
            vol = torch.full((A0 * A1 * A2 + offset,), 7.0, dtype=tdt, device=dev)[offset:].view(shape)     # 7.0: an unwritten element shows
            L.call('hv_volume_merge_view', ptr(out), ptr(flag), A0, A1, A2, axis, k0, S, odt, ptr(vol), stream())
            ref = np.zeros(shape, dtype=NP[odt])
            for s in range(S):
                if f[s]:
                    if axis == 1:
                        ref[:, k0 + s, :] = want[s]
                    else:
                        ref[:, :, k0 + s] = want[s]
            merged[odt] = vol.cpu().numpy()
            assert merged[odt].dtype == NP[odt] and np.array_equal(merged[odt], ref), (axis, 'merge', odt)
        if axis == 2 and dtype == F64:
            # the entries the sagittal host path used so far, on the same buffers: bit for bit
            HW = ctypes.c_longlong(A0 * A1)
            c_old = torch.full((3 * N,), -1, dtype=torch.int32, device=dev)
            L.call('hv_volume_scan', ptr(dl), HW, A2, 8.0, 7.0, -1.0, ptr(c_old), stream())
            o_old = torch.full((S, A0, C), -3.0, dtype=torch.float32, device=dev)
            L.call('hv_volume_slices', ptr(dc), HW, A2, k0, S, ptr(o_old), stream())
            v_old = torch.full(shape, 7.0, dtype=torch.float64, device=dev)
            L.call('hv_volume_merge', ptr(o_old), ptr(flag), HW, A2, k0, S, ptr(v_old), stream())
            assert torch.equal(c_old, counts) and torch.equal(o_old.view(torch.int32), out.contiguous().view(torch.int32))
            assert np.array_equal(v_old.cpu().numpy().view(np.int64), merged[F64].view(np.int64))


def test_view_kernels_reject_bad_arguments():
    """Every refusal happens before a launch (negative status, nothing thrown across the ABI) and leaves the output buffers as they were."""
    lib, L, dev = _lib()
    ptr, stream = lib.ptr, lib.stream
    A0, A1, A2 = 8, 6, 12
    vol = torch.zeros(A0, A1, A2, dtype=torch.float64, device=dev)
    counts = torch.full((3 * 12,), -1, dtype=torch.int32, device=dev)
    out = torch.full((4, A0, 12), -3.0, dtype=torch.float32, device=dev)
    flag = torch.ones(4, dtype=torch.int32, device=dev)
    big = torch.full((A0, A1, A2), 7.0, dtype=torch.float64, device=dev)
    ARG, UNSUPPORTED = -1, -2
    scan = lambda v=vol, dt=F64, s=(A0, A1, A2), axis=1, ids=(8.0, 7.0, -1.0), c=counts: L.cdll.hv_volume_scan_view(
        ptr(v), dt, s[0], s[1], s[2], axis, ids[0], ids[1], ids[2], ptr(c), stream())
    slices = lambda v=vol, dt=F64, s=(A0, A1, A2), axis=1, k0=1, S=4, o=out: L.cdll.hv_volume_slices_view(
        ptr(v), dt, s[0], s[1], s[2], axis, k0, S, ptr(o), stream())
    merge = lambda src=out, f=flag, s=(A0, A1, A2), axis=1, k0=1, S=4, odt=F64, o=big: L.cdll.hv_volume_merge_view(
        ptr(src), ptr(f), s[0], s[1], s[2], axis, k0, S, odt, ptr(o), stream())
    for axis in (0, 3, -1):                                               # an axis other than 1 or 2
        assert scan(axis=axis) == ARG and slices(axis=axis) == ARG and merge(axis=axis) == ARG
    for dt in (1, 2, 3, 6, -1):                                           # int16 / int32 / int64 volumes and unknown codes
        assert scan(dt=dt) == ARG and slices(dt=dt) == ARG
    for odt in (U8, 1, 6):
        assert merge(odt=odt) == ARG
    for axis, n in ((1, A1), (2, A2)):                                    # the slice range leaves the axis
        for k0, S in ((n - 3, 4), (-1, 4), (0, 0), (0, n + 1), (n, 1), (2147483647, 4)):
            assert slices(axis=axis, k0=k0, S=S) == ARG and merge(axis=axis, k0=k0, S=S) == ARG, (axis, k0, S)
    assert scan(v=None) == ARG and scan(c=None) == ARG                    # null pointers
    assert slices(v=None) == ARG and slices(o=None) == ARG
    assert merge(src=None) == ARG and merge(f=None) == ARG and merge(o=None) == ARG
    for ids in ((0.0, 7.0, -1.0), (8.0, 0.0, -1.0), (8.0, 7.0, 0.0)):     # an id of 0 (background is skipped; unused ids are negative)
        assert scan(ids=ids) == ARG and scan(ids=ids, axis=2) == ARG
    for s in ((0, A1, A2), (A0, -1, A2), (A0, A1, 0)):                    # non-positive sizes
        assert scan(s=s) == ARG and slices(s=s) == ARG and merge(s=s) == ARG
    # sizes beyond the index ranges of the kernels (refused before any launch: the buffers need not be that large)
    for s in ((65536, 65536, 1), (65536, 1, 65536)):
        for axis in (1, 2):
            assert scan(s=s, axis=axis) == UNSUPPORTED and slices(s=s, axis=axis, k0=0, S=1) == UNSUPPORTED
            assert merge(s=s, axis=axis, k0=0, S=1) == UNSUPPORTED
    assert scan(s=(1, 1, 2049), axis=2) == UNSUPPORTED                   # the axis-2 scan's histogram
    assert slices(s=(1, 70000, 1), axis=1, k0=0, S=65536) == UNSUPPORTED and merge(s=(1, 65536, 1), axis=1, k0=0, S=1) == UNSUPPORTED
    assert merge(s=(1, 1, 32 * 65535 + 1), axis=2, k0=0, S=1) == UNSUPPORTED
    with pytest.raises(RuntimeError, match='HV_ERR_ARG'):
        L.call('hv_volume_scan_view', ptr(vol), F64, A0, A1, A2, 0, 8.0, 7.0, -1.0, ptr(counts), stream())
    torch.cuda.synchronize()
    assert bool((counts == -1).all()) and bool((out == -3.0).all()) and bool((big == 7.0).all())
    # and the same calls with good arguments do write
    assert scan() == 0 and slices() == 0 and merge() == 0
    torch.cuda.synchronize()
    assert bool((counts[:3 * A1] == 0).all()) and bool((out == 0).all()) and bool((big == 0).all())


@pytest.fixture(scope='module')
def net():
    """The generator of test_infer_gpu.test_pipelined_volumes_equal_single_volume_calls."""
    import hvgan  # noqa: F401
    from hvgan.models.inpaint_networks import Generator
    torch.manual_seed(5)
    g = Generator({'input_dim': 1, 'ngf': 16}, True)
    g.fine_generator.fc_height.bias.data.fill_(0.41)
    g.fine_generator.fc_height.weight.data.mul_(1e-2)
    return g.cuda().eval()


def _swap(v):
    return np.ascontiguousarray(np.swapaxes(v, 1, 2))


def _volume(nz, seed, view, absent=False):
    """(ct, label, cam * 255) of synth.make_volume, [256, 256, nz] for the sagittal view and its swap [256, nz, 256] for the coronal view."""
    from hvgan import synth
    ct, label, cam = synth.make_volume(nz=nz, size=256, seed=seed)
    if absent:
        label = np.where(label == 20, 0.0, label)
    vol = (ct, label, cam * 255)
    return tuple(_swap(v) for v in vol) if view == 'coronal' else vol


def test_coronal_equals_sagittal_on_the_swapped_volume(net):
    from hvgan import infer
    dev = torch.device('cuda:0')
    vol = _volume(12, 2, 'sagittal')
    cor = tuple(_swap(v) for v in vol)
    assert cor[0].shape == (256, 12, 256)
    for vid in (20, 21):
        s_ct, s_seg = infer.process_volume(net, *vol, vid, dev)
        c_ct, c_seg = infer.process_volume(net, *cor, vid, dev, view='coronal')
        assert s_ct.any() and s_seg.any() and c_ct.any() and c_seg.any()
        assert c_ct.shape == (256, 12, 256) and c_ct.dtype == np.float64 and c_seg.dtype == np.float64
        assert np.array_equal(c_ct, np.swapaxes(s_ct, 1, 2)), vid
        assert np.array_equal(c_seg, np.swapaxes(s_seg, 1, 2)), vid


@pytest.mark.parametrize('view', ['sagittal', 'coronal'])
def test_resident_inputs_and_outputs(net, view):
    from hvgan import infer
    dev = torch.device('cuda:0')
    ct, label, cam = _volume(12, 2, view)
    h_ct, h_seg = infer.process_volume(net, ct, label, cam, 20, dev, view=view)
    assert h_ct.any() and h_seg.any()
    d = [torch.from_numpy(v).to(dev) for v in (ct, label, cam)]
    keep = [t.clone() for t in d]
    o_ct, o_seg = infer.process_volume(net, *d, 20, dev, view=view)                         # device float64 in, host out
    assert isinstance(o_ct, np.ndarray) and np.array_equal(o_ct, h_ct) and np.array_equal(o_seg, h_seg)
    lab8 = d[1].to(torch.uint8)
    assert torch.equal(lab8.double(), d[1])
    keep8 = lab8.clone()
    r_ct, r_seg = next(infer.process_volumes(net, [(d[0], lab8, d[2], 20)], dev, view=view, output='device'))     # uint8 label, device out
    for r in (r_ct, r_seg):
        assert isinstance(r, torch.Tensor) and r.device == dev and r.dtype == torch.float64 and tuple(r.shape) == ct.shape and r.is_contiguous()
    assert r_ct.data_ptr() != r_seg.data_ptr()
    assert np.array_equal(r_ct.cpu().numpy(), h_ct) and np.array_equal(r_seg.cpu().numpy(), h_seg)
    # float32 device volumes are cast as they are: the result of the host path on the values they hold
    f = [t.float() for t in d]
    f_ct, f_seg = infer.process_volume(net, *f, 20, dev, view=view, output='device')
    g_ct, g_seg = infer.process_volume(net, *(t.cpu().numpy().astype(np.float64) for t in f), 20, dev, view=view)
    assert np.array_equal(f_ct.cpu().numpy(), g_ct) and np.array_equal(f_seg.cpu().numpy(), g_seg)
    # a second resident volume does not touch the tensors handed out for the first
    r2 = infer.process_volume(net, *d, 21, dev, view=view, output='device')
    assert np.array_equal(r_ct.cpu().numpy(), h_ct) and np.array_equal(r_seg.cpu().numpy(), h_seg) and r2[0].data_ptr() != r_ct.data_ptr()
    # the inputs are as they were
    assert all(torch.equal(a, b) for a, b in zip(d, keep)) and torch.equal(lab8, keep8)
    assert all(torch.equal(a, b.float()) for a, b in zip(f, keep))


def test_pipelined_coronal_stream_equals_single_calls(net):
    """Three coronal volumes (another slice count last: the slots are rebuilt), the middle one without the vertebra: fresh arrays, pinned views, a
    stream that mixes host and device inputs, and the same stream left on the device."""
    from hvgan import infer
    dev = torch.device('cuda:0')
    vols = [_volume(12, 2, 'coronal') + (20,), _volume(12, 6, 'coronal', absent=True) + (20,), _volume(16, 3, 'coronal') + (21,)]
    single = [infer.process_volume(net, *v[:3], v[3], dev, view='coronal') for v in vols]
    assert not single[1][0].any() and not single[1][1].any()
    assert single[0][1].any() and single[2][1].any()
    for copy in (True, False):
        n = 0
        for i, (oc, os_) in enumerate(infer.process_volumes(net, vols, dev, copy=copy, view='coronal')):
            assert oc.dtype == np.float64 and oc.shape == vols[i][0].shape
            assert np.array_equal(oc, single[i][0]) and np.array_equal(os_, single[i][1]), (copy, i)
            n += 1
        assert n == 3
    up = lambda a: torch.from_numpy(a).to(dev)
    mixed = [vols[0],
             (up(vols[1][0]), up(vols[1][1]), up(vols[1][2]), 20),                          # all resident (and empty)
             (vols[2][0], up(vols[2][1]).to(torch.uint8), up(vols[2][2]), 21)]              # host CT, resident uint8 label and CAM
    for output in ('host', 'device'):
        res = list(infer.process_volumes(net, mixed, dev, view='coronal', output=output))
        assert len(res) == 3
        for i, (oc, os_) in enumerate(res):
            if output == 'device':
                oc, os_ = oc.cpu().numpy(), os_.cpu().numpy()
            assert np.array_equal(oc, single[i][0]) and np.array_equal(os_, single[i][1]), (output, i)


@pytest.mark.parametrize('view', ['sagittal', 'coronal'])
def test_resident_chain_into_rhlv(net, view):
    """synthesize -> RHLV without leaving the device: rhlv_volume on the output='device' label volume and the device input label, both read through the
    view's own strides, equals the same call on the downloaded arrays."""
    from hvgan import infer, evaluation
    dev = torch.device('cuda:0')
    ct, label, cam = _volume(CHAIN_NZ, 2, view)
    h_ct, h_seg = infer.process_volume(net, ct, label, cam, 20, dev, view=view)
    host = evaluation.rhlv_volume(h_seg, label, 20, view=view)
    assert host is not None and len(host) == 5 and all(np.isfinite(v) for v in host), host       # numbers, not None (and nothing raised)
    d = [torch.from_numpy(v).to(dev) for v in (ct, label, cam)]
    r_ct, r_seg = infer.process_volume(net, *d, 20, dev, view=view, output='device')
    got = evaluation.rhlv_volume(r_seg, d[1], 20, view=view)
    assert got == host, (got, host)
    got8 = evaluation.rhlv_volume(r_seg, d[1].to(torch.uint8), 20, view=view)                  # the label as straighten_patient leaves it
    assert got8 == host, (got8, host)

