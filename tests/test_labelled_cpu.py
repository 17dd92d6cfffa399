"""The pure logic of healthivert-gan_amd/labelled.py, the one owner of the per-label input protocol: the argument checks, how a pair of volumes
is addressed (one [2] batch or two launches) and the Strided view.  None of it needs a device."""
import numpy as np
import pytest
import torch


def _L():
    import hvgan  # noqa: F401
    from hvgan import labelled
    return labelled


def test_check_labels():
    L = _L()
    assert L.check_labels([3]) == [3] and L.check_labels((0, 255, 7)) == [0, 255, 7]
    assert L.check_labels(np.asarray([21.0, 22.0])) == [21, 22] and L.check_labels(range(64)) == list(range(64))
    for bad in ([], list(range(65)), [1, 1], [-1], [256], [1.5], ['a'], 3, None):
        with pytest.raises(ValueError):
            L.check_labels(bad)


def test_check_spacing():
    L = _L()
    assert L.check_spacing((0.7, 0.7, 1.5)) == (0.7, 0.7, 1.5) and L.check_spacing(2) == (2.0, 2.0, 2.0)
    assert L.check_spacing(np.float32(0.5)) == (0.5, 0.5, 0.5) and L.check_spacing([1, 2, 3]) == (1.0, 2.0, 3.0)
    for bad in ((1, 1), (1, 1, 1, 1), (1, 0, 1), (1, -1, 1), (1, float('nan'), 1), (1, float('inf'), 1), 'abc', None, True, 0):
        with pytest.raises(ValueError):
            L.check_spacing(bad)


def test_check_erode():
    L = _L()
    assert L.check_erode(0) == 0.0 and L.check_erode(1.5) == 1.5 and L.check_erode(np.float64(2)) == 2.0
    for bad in (-0.5, float('nan'), float('inf'), True, '1', None, (1,)):
        with pytest.raises(ValueError):
            L.check_erode(bad)


def test_tensor_checks_refuse_the_host():
    L = _L()
    t = torch.zeros((2, 3, 4), dtype=torch.int16)
    with pytest.raises(TypeError):
        L.check_tensor(t.numpy(), 'vol', L.VOL_DT)                     # not a tensor
    with pytest.raises(ValueError):
        L.check_tensor(t, 'vol', L.VOL_DT)                             # a CPU tensor: there is no CPU path
    with pytest.raises(ValueError):
        L.check_3d(t, 'ct', L.VOL_DT)
    with pytest.raises(ValueError):
        L.resolve_labels(None, lambda: [])
    with pytest.raises(ValueError):
        L.resolve_labels(None, lambda: list(range(1, 66)))
    assert L.resolve_labels(None, lambda: [4, 9]) == [4, 9] and L.resolve_labels((5,), None) == [5]
    assert L.squeeze({'labels': [1], 'count': np.zeros((1, 1))})['count'].shape == (1,)


def _plan(L, cts, labels):
    return [(None if v is None else tuple(v.shape), tuple(l.shape), sel) for v, l, sel in L.pair_plan(cts, labels)]


def test_pair_addressing():
    L = _L()
    both = torch.zeros((2, 5, 6, 7), dtype=torch.int16)
    labs = torch.zeros((2, 5, 6, 7), dtype=torch.uint8)
    assert L.batch_stride(both[0], both[1]) == 5 * 6 * 7 and L.batch_stride(both[1], both[0]) == -5 * 6 * 7
    one, two = (2, 5, 6, 7), (1, 5, 6, 7)
    assert _plan(L, (both[0], both[1]), (labs[0], labs[1])) == [(one, one, slice(None))]
    assert _plan(L, None, (labs[0], labs[1])) == [(None, one, slice(None))]
    split = [(two, two, slice(0, 1)), (two, two, slice(1, 2))]
    # a permuted second member: the same shape, other strides
    perm = torch.zeros((7, 5, 6), dtype=torch.int16).permute(1, 2, 0)
    assert perm.shape == both[0].shape and L.batch_stride(both[0], perm) is None
    assert _plan(L, (both[0], perm), (labs[0], labs[1])) == split
    assert _plan(L, (both[0], both[1]), (labs[0], torch.zeros((7, 5, 6), dtype=torch.uint8).permute(1, 2, 0))) == split
    assert _plan(L, None, (labs[0], torch.zeros((7, 5, 6), dtype=torch.uint8).permute(1, 2, 0))) == [(None,) + s[1:] for s in split]
    # members of different dtype
    assert L.batch_stride(both[0], both[1].to(torch.float32)) is None
    assert _plan(L, (both[0], both[1]), (labs[0], labs[1].to(torch.int16))) == split
    # a distance that is no multiple of the element size: two int16 views one byte apart in one buffer
    raw = np.zeros(2 * 5 * 6 * 7 + 1, dtype=np.uint8)
    a, b = (torch.from_numpy(np.ndarray((5, 6, 7), np.int16, raw, o)) for o in (0, 1))
    assert b.data_ptr() - a.data_ptr() == 1 and a.stride() == b.stride() and L.batch_stride(a, b) is None
    assert _plan(L, (a, b), (labs[0], labs[1])) == split
    # the two-launch plan hands out the members themselves, in order
    (v0, l0, _), (v1, l1, _) = L.pair_plan((both[0], perm), (labs[0], labs[1]))
    assert v0.data_ptr() == both[0].data_ptr() and v1.data_ptr() == perm.data_ptr() and v1.stride()[1:] == perm.stride()
    assert l0.data_ptr() == labs[0].data_ptr() and l1.data_ptr() == labs[1].data_ptr()


def test_strided_view():
    L = _L()
    both = torch.zeros((2, 5, 6, 7), dtype=torch.float32)
    s = L.Strided(both[0], L.batch_stride(both[0], both[1]))
    assert s.shape == (2, 5, 6, 7) and s.stride() == both.stride() == (210, 42, 7, 1) and s.data_ptr() == both.data_ptr()
    assert s.dtype == torch.float32 and s.device == both.device
    far = torch.zeros((5, 6, 7), dtype=torch.float32)
    d = (far.data_ptr() - both[0].data_ptr()) // 4
    t = L.Strided(both[0], d)
    assert t.stride() == (d, 42, 7, 1) and t.data_ptr() + 4 * t.stride()[0] == far.data_ptr()
    # the one batch of a plan is this view: the members' rows of a [2][...] result are all of it
    (v, l, sel), = L.pair_plan((both[0], both[1]), (both[0], both[1]))
    assert isinstance(v, L.Strided) and v.stride() == both.stride() and sel == slice(None)


def test_pair_launch_follows_the_plan():
    """Pair.launch hands the masks' rows that sel names to the callable; built without the constructor's device checks."""
    L = _L()
    both = torch.zeros((2, 5, 6, 7), dtype=torch.int16)
    labs = torch.zeros((2, 5, 6, 7), dtype=torch.uint8)
    for synth, want in ((both[1], [2]), (torch.zeros((7, 5, 6), dtype=torch.int16).permute(1, 2, 0), [1, 1])):
        for masks in (None, torch.ones((2, 5, 6, 7), dtype=torch.uint8)):
            p = object.__new__(L.Pair)
            p.cts, p.labels, p.masks = (both[0], synth), (labs[0], labs[1]), masks
            calls = []
            p.launch(lambda vol, label, mask, sel: calls.append((int(vol.shape[0]), None if mask is None else tuple(mask.shape), sel)))
            assert [c[0] for c in calls] == want
            assert all(c[1] == (None if masks is None else (c[0], 5, 6, 7)) for c in calls)
            assert [c[2] for c in calls] == ([slice(None)] if want == [2] else [slice(0, 1), slice(1, 2)])
