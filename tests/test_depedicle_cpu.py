"""De-pedicling without a GPU: the plain-numpy restatement of the rule (tests/depedicle_ref.py) against the reference's own results in fixture
G17 (tools/make_golden_depedicle.py) and against scipy where it is installed, the host walk of single_component_range, and the C ABI."""
import os

import numpy as np
import pytest

import depedicle_ref as R
from conftest import ROOT, load_golden


def _g():
    cases = {}
    for k, v in load_golden('g17_depedicle').items():
        a, b = k.split('/')
        cases.setdefault(a, {})[b] = v.numpy()
    return cases


def test_restatement_reproduces_every_array_and_range_of_g17():
    cases = _g()
    assert len(cases) >= 7
    changed = 0
    for name, c in cases.items():
        out, counts = R.depedicle(c['in'])
        assert out.dtype == np.uint8 and np.array_equal(out, c['out']), name
        assert np.array_equal(counts, c['counts']), name
        changed += int((out != c['in']).any())
        for l, z0, z1 in c['ranges']:
            assert R.single_component_range(counts, l) == (z0, z1), (name, l)
    assert changed >= 6                                     # the fixture is not a no-op


def test_wrapper_walk_equals_restatement_walk():
    import hvgan  # noqa: F401
    from hvgan import straighten as S
    rng = np.random.default_rng(3)
    for Z in (1, 2, 7, 16, 24, 64):
        for _ in range(20):
            counts = np.zeros((Z, 256), np.int32)
            counts[:, 5] = rng.integers(0, 3, Z)
            for off in (0, 3, 10, 40):
                assert S.single_component_walk(counts[:, 5], off) == R.single_component_range(counts, 5, off), (Z, off)
    for name, c in _g().items():
        for l, z0, z1 in c['ranges']:
            col = c['counts'][:, l] if l <= 255 else np.zeros(len(c['counts']))
            assert S.single_component_walk(col) == (z0, z1), (name, l)


def test_restatement_counts_equal_scipy_on_random_layers():
    ndimage = pytest.importorskip('scipy.ndimage')
    rng = np.random.default_rng(17)
    for t in range(60):
        shape = (int(rng.integers(1, 14)), int(rng.integers(1, 14)))
        layer = rng.integers(0, 4, shape).astype(np.uint8) * np.uint8(85)      # values 0, 85, 170, 255
        out, counts = R.depedicle_layer(layer)
        for v in range(1, 256):
            lab, n = ndimage.label(layer == v)
            assert counts[v] == n, (t, v)
            if n:                                           # the kept component: smallest (min column, feature number)
                keep = min((np.nonzero(lab == f)[1].min(), f) for f in range(1, n + 1))[1]
                assert np.array_equal(out == v, lab == keep), (t, v)
        assert counts[0] == 0


def test_worst_case_shapes_are_what_they_claim():
    s = R.spiral(63)
    assert len(R.components(s)) == 1 and s.sum() == 2047
    assert not (s[:-1, :-1] & s[1:, :-1] & s[:-1, 1:] & s[1:, 1:]).any()       # one pixel wide
    c = R.comb(64, 31)
    assert len(R.components(c)) == 1 and c[1:, :61].sum(axis=0).tolist() == [63, 0] * 30 + [63]


def test_header_declares_and_library_exports_the_entry_point():
    import __graft_entry__ as g
    g.build()
    import ctypes
    import hvgan  # noqa: F401
    from hvgan import lib as L, straighten as S
    _, protos = L.parse_header()
    res, args = protos['hv_depedicle']
    assert res is ctypes.c_int and len(args) == 18
    assert args[:6] == [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_longlong] * 4 and args[-3:] == [ctypes.c_void_p] * 3
    cdll = ctypes.CDLL(L.LIB_PATH)
    assert hasattr(cdll, 'hv_depedicle')
    for name in ('depedicle', 'component_counts', 'single_component_range'):
        assert callable(getattr(S, name))
    src = open(os.path.join(ROOT, 'healthivert-gan_amd', 'csrc', 'build.py')).read()
    assert "'depedicle.hip'" in src


def test_cpu_tensor_and_wrong_rank_are_refused():
    import torch
    import hvgan  # noqa: F401
    from hvgan import straighten as S
    vol = torch.zeros(4, 4, 2, dtype=torch.uint8)
    for fn in (S.depedicle, S.component_counts, lambda t: S.single_component_range(t, 1)):
        with pytest.raises(RuntimeError):
            fn(vol)
