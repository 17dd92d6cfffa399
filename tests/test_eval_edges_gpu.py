"""hv_eval_metrics (csrc/eval_metrics.hip) at its edges, through the C entry, against tests/eval_ref.py (pinned by tests/test_eval_ref_cpu.py, which also
checks that on every input used here the float32 reference lies within a quarter tolerance of the float64 definition).

Shapes (eval_ref.SHAPES): one SSIM pixel with HW = 49, far below one 1024-thread pass; an SSIM region one pixel wide; a ragged width; H - 6 = 9, a second
8-row SSIM tile that holds one row; HW no multiple of 1024 with a ragged last tile, non-square; B = 65, the second workgroup of the final kernel.
`out` and the workspace are hvtest.Guarded buffers, the workspace exactly the queried bytes; after every call the guards must be intact.  Tolerances are
those of tests/test_eval_gpu.py (eval_ref.TOL); the closed cases are asserted bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import eval_ref as ER

pytestmark = pytest.mark.gpu

T = lib = None
KEYS = ('inp', 'gt', 'mask', 'cb', 'nv', 'fb', 'lab', 'pred_h', 'height')


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


def workspace(nbytes, offset=0):
    """exactly nbytes inside 0xA5 guards (int8: the byte sentinel is a signed value), the base `offset` bytes off the buffer's 64-byte alignment"""
    return T.Guarded((nbytes,), torch.int8, guard=64, offset=offset)


def call(d, B, H, W, ws=None, ws_bytes=None):
    """-> (status, Guarded out [B][5] that held NaN before the call); guards of out and workspace checked"""
    L = lib.get()
    dev = T.dev()
    t = [torch.from_numpy(np.ascontiguousarray(d[k])).to(dev) for k in KEYS]
    need = L.size('hv_eval_metrics_workspace_bytes', B, H, W)
    ws = workspace(need) if ws is None else ws
    out = T.Guarded((B, 5))
    rc = L.cdll.hv_eval_metrics(*[lib.ptr(v) for v in t], B, H, W, lib.ptr(out.t), lib.ptr(ws.t), ctypes.c_size_t(need if ws_bytes is None else ws_bytes),
                                lib.stream())
    torch.cuda.synchronize()
    assert out.intact() and ws.intact(), 'wrote outside out / the queried workspace'
    return rc, out


def f32_counts(x, y, kind):
    """train.py's dice_score / iou_score in float32 on the exact integer counts of two 0/1 maps"""
    f = np.float32
    i, p, t, s = f((x * y).sum(dtype=np.float64)), f(x.sum(dtype=np.float64)), f(y.sum(dtype=np.float64)), f(1e-5)
    return (f(2) * i + s) / (p + t + s) if kind == 'dice' else (i + s) / (p + t - i + s)


@pytest.mark.parametrize('shape', ER.SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_edge_shapes_match_the_float32_reference(shape):
    B, H, W = shape
    d = ER.edge_inputs(B, H, W)
    rc, out = call(d, B, H, W)
    assert rc == 0
    got = out.cpu().double().numpy()
    ref = np.stack([ER.metrics_f32(*ER.sample(d, i)) for i in range(B)])
    err = np.abs(got - ref).max(axis=0)
    print('eval edges', shape, 'max error / tolerance', err / np.array(ER.TOL))
    for k, (name, tol) in enumerate(zip(('ssim', 'psnr', 'dice', 'iou', 'diff_h'), ER.TOL)):
        assert err[k] <= tol, (shape, name, got[:, k], ref[:, k])
    # random 0/1 maps: the overlap counts are exact integers in any order, so Dice and IoU are the float32 expression on them, bit for bit
    g32 = out.cpu().numpy()
    for i in range(B):
        assert g32[i, 2] == f32_counts(d['cb'][i], d['nv'][i], 'dice') and g32[i, 3] == f32_counts(d['fb'][i], d['lab'][i], 'iou'), (shape, i)
    # the reductions have a fixed order: a second run gives the same bytes
    rc2, out2 = call(d, B, H, W)
    assert rc2 == 0 and torch.equal(out.t.view(torch.int32), out2.t.view(torch.int32))


@pytest.mark.parametrize('shape', [(1, 7, 7), (3, 15, 14), (2, 40, 70), (65, 9, 9)], ids=lambda s: 'x'.join(map(str, s)))
def test_closed_cases_are_exact(shape):
    B, H, W = shape
    d = ER.edge_inputs(B, H, W)
    same = dict(d, gt=d['inp'].copy())                                  # identical images
    rc, out = call(same, B, H, W)
    m = out.cpu().numpy()
    assert rc == 0 and (m[:, 0] == 1.0).all() and (m[:, 1] == np.inf).all(), m[:, :2]
    assert (d['inp'].reshape(B, -1).max(1) > d['inp'].reshape(B, -1).min(1)).all()          # R > 0
    rc, out = call(dict(d, mask=np.zeros_like(d['mask'])), B, H, W)    # all-zero mask: every window is (C1 C2) / (C1 C2)
    m = out.cpu().numpy()
    assert rc == 0 and (m[:, 0] == 1.0).all(), m[:, 0]
    z = np.zeros_like(d['cb'])
    rc, out = call(dict(d, cb=z, nv=z, fb=z, lab=z), B, H, W)           # empty maps: smooth / smooth
    m = out.cpu().numpy()
    assert rc == 0 and (m[:, 2] == 1.0).all() and (m[:, 3] == 1.0).all(), m[:, 2:4]


def test_refusals_leave_out_untouched():
    L = lib.get()
    B, H, W = 2, 8, 23
    d = ER.edge_inputs(B, H, W)
    need = L.size('hv_eval_metrics_workspace_bytes', B, H, W)
    assert need > 0 and need % 8 == 0

    def refused(rc_out, status):
        rc, out = rc_out
        assert rc == status and bool(torch.isnan(out.t).all()), (rc, status)
    refused(call(d, B, H, W, ws=workspace(need + 4, offset=4), ws_bytes=need + 4), -3)      # base + 4 bytes: not 8-byte aligned
    refused(call(d, B, H, W, ws=workspace(need), ws_bytes=need - 1), -3)                    # one byte short
    rc, out = call(d, B, H, W, ws=workspace(need), ws_bytes=need)                           # control: the same buffers are accepted
    assert rc == 0 and bool(torch.isfinite(out.t).all())
    for h, w in ((6, 23), (8, 6), (6, 6)):
        small = {k: (v[:, :h, :w] if v.ndim == 3 else v) for k, v in d.items()}
        assert L.size('hv_eval_metrics_workspace_bytes', B, h, w) == 0
        refused(call(small, B, h, w, ws=workspace(4096), ws_bytes=4096), -2)


def test_batch_metrics_under_an_exact_workspace(monkeypatch):
    """eval_metrics.batch_metrics (composite, thresholds, metrics) on a 40 x 70 batch with ops._ws handing out exactly the queried bytes"""
    from hvgan import eval_metrics as EM
    from oracle import restate as R
    outs, b = ER.batch_case()
    ref, inp_ref = R.eval_sample_metrics(outs['stage2'], outs['fine_seg'], outs['coarse_seg'], outs['pred2'], b)
    dv = lambda t: t.to(T.dev())
    ws = T.ExactWs(monkeypatch, required=True)
    m, inp, cb, fb = EM.batch_metrics(dv(outs['stage2']), dv(outs['fine_seg']), dv(outs['coarse_seg']), dv(outs['pred2']), dv(b['real_B']),
                                      dv(b['real_B_mask']), dv(b['normal_vert']), dv(b['mask']), dv(b['height']), dv(b['x1']), dv(b['x2']),
                                      dv(b['maxheight']))
    ws.close()
    assert torch.equal(inp.cpu(), inp_ref) and torch.equal(cb.cpu(), (outs['coarse_seg'] > 0.5).float())
    got = m.cpu().double().numpy()
    for k, tol in enumerate(ER.TOL):
        assert np.abs(got[:, k] - ref[:, k]).max() <= tol, (k, got[:, k], ref[:, k])
