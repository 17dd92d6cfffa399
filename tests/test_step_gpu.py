"""Full Pix2PixModel train step on the HIP path against (a) the golden vectors of the reference's own
optimize_parameters (G5: B=2, 256^2, seed 1234, two steps) and (b) the CPU oracle run live on the same weights.
fp32 mode; tolerance 1e-3 on continuous tensors, mismatch fraction on thresholded ones."""
from argparse import Namespace

import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu


def make_opt(**kw):
    o = Namespace(gpu_ids=[0], isTrain=True, checkpoints_dir='/tmp/hv_ckpt', name='t', preprocess='none', input_nc=1, output_nc=1,
                  ngf=64, ndf=64, netD='basic', netG='unet_256', n_layers_D=3, norm='batch', init_type='normal', init_gain=0.02,
                  no_dropout=True, gan_mode='vanilla', lr=2e-4, beta1=0.5, lambda_L1=200.0, direction='BtoA', lr_policy='linear',
                  epoch_count=1, n_epochs=100, n_epochs_decay=100, continue_train=False, load_iter=0, epoch='latest', verbose=False)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _sparse(t, step=8):
    return t.detach()[..., ::step, ::step].cpu()


# max-abs <= 1e-3 on CONTINUOUS tensors; a mismatch fraction only for tensors behind a threshold (fine_seg > 0.5 and
# what is computed from it) or behind the ceil() of the SHRM row bounds (composited images: a height that lands on the other side of an
# integer moves one row of the paste)
CONTINUOUS = ('x_stage1', 'fake_B_raw', 'coarse_seg_sigmoid', 'fake_B_mask_sigmoid', 'real_edges')


def check_activation(name, got, ref, tol=1e-3, frac_tol=1e-4, ctx=()):
    d = (got.detach().cpu().float() - ref.detach().cpu().float()).abs()
    if name in CONTINUOUS:
        assert d.max().item() <= tol, ctx + (name, 'max-abs', d.max().item())
    else:
        frac = (d > tol).float().mean().item()
        assert frac <= frac_tol, ctx + (name, 'mismatch fraction', frac, d.max().item())


@pytest.mark.parametrize('batch_d', ['1', '0'])      # discriminators' fake | real passes as one 2B launch sequence (default) / split, real first
@pytest.mark.parametrize('precision,loss_tol,norm_tol', [('fp32', 2e-3, 1e-3), ('fp16', 6e-3, 4e-3)])
def test_g5_two_train_steps_match_reference_golden(precision, loss_tol, norm_tol, batch_d, monkeypatch):
    """fp32 = exact-fp32 MFMA parity mode.  fp16 = the benchmarked mode (fp16 MFMA operands, fp32 accumulate/storage): it
    meets the SAME |d| <= 1e-3 gate on every sampled activation of both steps (observed max 3e-4); only the loss scalars that
    sit behind a >0.5 threshold (edge, D_2) and the post-Adam parameter norms get the wider stated tolerances."""
    monkeypatch.setenv('HV_PRECISION', precision)
    monkeypatch.setenv('HV_BATCH_D', batch_d)
    import hvgan
    from hvgan import synth
    from hvgan.models.pix2pix_model import Pix2PixModel
    g = load_golden('g5_full_step')
    torch.manual_seed(1234)
    model = Pix2PixModel(make_opt())
    for n in ('G', 'D_1', 'D_2', 'D_3'):
        sd = getattr(model, 'net' + n).state_dict()
        chk = torch.tensor([float(v.double().sum()) for v in sd.values()] + [float(sum(v.double().abs().sum() for v in sd.values()))], dtype=torch.float64)
        assert torch.allclose(chk, g['init'][n].double(), rtol=1e-6, atol=1e-5), "seeded initial weights differ from the reference for net" + n
    report = {}
    for step in range(2):
        model.set_input(synth.make_batch(2, 256, seed=1234 + step))
        model.optimize_parameters()
        torch.cuda.synchronize()
        losses = model.get_current_losses()
        for k, v in g['losses%d' % step].items():
            ref = float(v)
            report['loss%d/%s' % (step, k)] = (losses[k], ref)
            # (fp16 mode: the losses behind the fine_seg > 0.5 threshold -- edge, D_2's -- move with the pixels that fp16 rounding flips: 2 %)
            tol = (2e-2 if (precision != 'fp32' and k in ('edge', 'D_real_2', 'D_fake_2')) else loss_tol) * max(1.0, abs(ref))
            assert abs(losses[k] - ref) <= tol, (step, k, losses[k], ref)
        for k, ref in g['samples%d' % step].items():
            # fp16 operands can move fine_seg across 0.5 at a pixel or two of the 2048 sampled ones (edges follow the thresholded mask)
            check_activation(k, _sparse(getattr(model, k)), ref, frac_tol=1e-4 if precision == 'fp32' else 2e-3, ctx=(precision, step))
        ph = torch.cat([model.pred1_h, model.pred2_h]).cpu()
        assert (ph - g['pred_h%d' % step]).abs().max().item() <= 1e-2
        for key, ref in g['norms%d' % step].items():
            n, k = key.split('/', 1)
            v = getattr(model, 'net' + n).state_dict()[k]
            got = float(v.double().norm())
            assert abs(got - float(ref)) <= norm_tol * max(1.0, float(ref)), (step, key, got, float(ref))
        # sampled ELEMENTS of every tensor after the step (every 97th).  Adam's first updates are +-lr = 2e-4 per element whatever the gradient's
        # size (m / sqrt(v) = sign(g)), so a missing, doubled or mis-scaled update of a tensor moves ALL its elements by ~2e-4 and hides inside the
        # norm tolerance above; here it does not.  The same property makes an element whose gradient is at rounding-noise level land on the other
        # side (2 lr away) now and then: the gate is the FRACTION of sampled elements beyond a tenth of lr, plus a hard bound of a few lr.
        lr, bad, tot, worst = 2e-4, 0, 0, 0.0
        for key, ref in g['elems%d' % step].items():
            n, k = key.split('/', 1)
            if n == 'D_2' and precision != 'fp32':
                continue      # D_2 is fed the thresholded mask (fine_seg > 0.5): with fp16 operands a few flipped pixels change its INPUT
            v = getattr(model, 'net' + n).state_dict()[k].detach().flatten()[::97].cpu().float()
            e = (v - ref.float()).abs()
            if 'running' in k or 'num_batches' in k or k.endswith('weight_u') or k.endswith('weight_v'):
                # buffers (BatchNorm statistics, spectral-norm power-iteration vectors): not Adam-updated; they follow the weights
                assert e.max().item() <= (1e-4 if precision == 'fp32' else 5e-3) * max(1.0, ref.abs().max().item()), (precision, step, key, e.max().item())
                continue
            frac = (e > 0.1 * lr).float().mean().item()
            if precision == 'fp32' or e.numel() >= 64:      # (fp16 operands flip the sign of noise-level gradient elements more often: small samples are noisy)
                assert frac <= (0.02 if precision == 'fp32' else 0.25), (precision, step, key, 'fraction of sampled weights off by > lr/10', frac)
            bad += int((e > 0.1 * lr).sum()); tot += e.numel(); worst = max(worst, e.max().item())
        assert worst <= 2.5 * lr * (step + 1), (precision, step, worst)
        assert bad <= (0.002 if precision == 'fp32' else 0.05) * tot, (precision, step, bad, tot)


def test_g7_eval_forward_bs1_matches_reference_golden():
    import hvgan
    from hvgan import synth
    from hvgan.models.inpaint_networks import Generator
    g = load_golden('g7_inference')
    torch.manual_seed(77)
    net = Generator({'input_dim': 1, 'ngf': 16}, True).eval()
    chk = torch.tensor([float(v.double().sum()) for v in net.state_dict().values()], dtype=torch.float64)
    assert torch.allclose(chk, g['init'].double(), rtol=1e-6, atol=1e-5)
    net.cuda()
    b = synth.to_model_inputs(synth.make_batch(1, 256, seed=77))
    dev = torch.device('cuda:0')
    with torch.no_grad():
        o = net(b['real_A'].to(dev), b['mask'].to(dev), (1 - b['CAM']).to(dev), b['slice_ratio'].to(dev))
    for name, idx in (('coarse_seg', 0), ('fine_seg', 1), ('x_stage1', 2), ('x_stage2', 3)):
        assert (_sparse(o[idx], 4) - g[name]).abs().max().item() <= 1e-3, name
    assert (o[5].cpu() - g['pred1_h']).abs().max().item() <= 1e-3 and (o[6].cpu() - g['pred2_h']).abs().max().item() <= 1e-3


def test_graph_replay_matches_eager_launches(monkeypatch):
    """The captured hipGraph step (one graph per step in a single process; three, cut where the gradient exchanges go, under data parallelism) leaves the same weights, BatchNorm statistics, Adam state and
    losses as launching the ~650 kernels eagerly: 5 steps on changing inputs from one seed, compared bit for bit."""
    monkeypatch.setenv('HV_PRECISION', 'fp16')
    import hvgan
    from hvgan import synth
    from hvgan.models.pix2pix_model import Pix2PixModel

    def run(use_graph):
        torch.manual_seed(99)
        model = Pix2PixModel(make_opt())
        model.use_graph = use_graph
        losses = []
        for step in range(5):
            model.set_input(synth.make_batch(2, 256, seed=500 + step))
            model.optimize_parameters()
            losses.append(model.get_current_losses())
        torch.cuda.synchronize()
        assert (model._graphs is not None) == use_graph
        state = {n + '/' + k: v.detach().clone() for n in ('G', 'D_1', 'D_2', 'D_3') for k, v in getattr(model, 'net' + n).state_dict().items()}
        state['adam_m'] = model.optimizer_G._m.clone()
        state['fake_B'] = model.fake_B.clone()
        return losses, state

    le, se = run(False)
    lg, sg = run(True)
    for a, b in zip(le, lg):
        for k in a:
            assert a[k] == b[k], (k, a[k], b[k])
    for k in se:
        assert torch.equal(se[k], sg[k]), k


@pytest.mark.parametrize('precision,loss_tol,act_tol', [('fp32', 2e-3, 1e-3), ('fp16', 6e-3, 1e-3)])
def test_benchmark_configuration_bs16_matches_live_oracle(precision, loss_tol, act_tol, monkeypatch):
    """The benchmarked configuration itself (bs=16, 256x256: 8x32-pixel tiles, wide weight-gradient tiles, many split-K slabs --
    kernel instantiations the B=2 golden run never reaches): one full train step from seeded weights against the CPU oracle run
    live on the same weights and batch.  12 losses, sampled activations, and every parameter after Adam."""
    monkeypatch.setenv('HV_PRECISION', precision)
    import hvgan
    from hvgan import synth
    from hvgan.models.pix2pix_model import Pix2PixModel
    from oracle import restate as R
    torch.manual_seed(4321)
    model = Pix2PixModel(make_opt())
    sd_g = {k: v.detach().cpu().clone() for k, v in model.netG.state_dict().items()}
    sd_d = [{k: v.detach().cpu().clone() for k, v in getattr(model, 'netD_%d' % k).state_dict().items()} for k in (1, 2, 3)]
    raw = synth.make_batch(16, 256, seed=777)
    model.set_input(raw)
    model.optimize_parameters()
    torch.cuda.synchronize()
    st = R.StepState(sd_g, sd_d, lr=2e-4, beta1=0.5, norm='batch', gan_mode='vanilla', lambda_l1=200.0)
    losses, outs = R.pix2pix_step(st, synth.to_model_inputs(raw))
    got = model.get_current_losses()
    for k, ref in losses.items():
        assert abs(got[k] - ref) <= loss_tol * max(1.0, abs(ref)), (k, got[k], ref)
    for name in ('fake_B', 'fake_B_coarse', 'x_stage1', 'fake_B_raw', 'coarse_seg_sigmoid', 'fake_B_mask_sigmoid', 'fake_B_local'):
        ref = outs[{'coarse_seg_sigmoid': 'coarse_seg', 'fake_B_mask_sigmoid': 'fine_seg'}.get(name, name)]
        check_activation(name, getattr(model, name), ref, tol=act_tol, ctx=(precision,))
    # parameter gradients (relative L2 error per tensor) and, in the exact-fp32 mode, the parameters after the Adam step (Adam's first
    # step moves every weight by ~lr*sign(g): a sign flip of a round-off-level gradient shows as 2*lr, so only a small fraction may differ)
    # fp16 operands: observed <= 5 % on matrices (the layers behind the attention soft-max; the rest < 1 %) and <= 14 % on vectors
    gtol, vtol = (2e-3, 2e-3) if precision == 'fp32' else (6e-2, 1.6e-1)
    d2_own = None
    if precision != 'fp32':
        # D_2 is fed the thresholded mask (fine_seg > 0.5): with fp16 operands a few pixels flip, which changes its INPUT, not its arithmetic.
        # Its gradients are therefore held against the oracle's D pass on the DEVICE's own binary mask (exactly representable), from the
        # same initial D_2 weights: fake pass, real pass, (loss_fake + loss_real) / 2 -- models/pix2pix_model.py:267-300
        sd2 = {k: (v.detach().clone().requires_grad_(True) if v.is_floating_point() and k in st.d_params[1] else v.detach().clone()) for k, v in sd_d[1].items()}
        dev_fake = model.fake_B_mask_raw.detach().cpu().float()
        assert set(dev_fake.unique().tolist()) <= {0.0, 1.0}
        pf, _ = R.disc_forward(sd2, dev_fake, 'batch', True)
        pr, _ = R.disc_forward(sd2, synth.to_model_inputs(raw)['real_B_mask'], 'batch', True)
        ((R.gan_loss(pf, False, 'vanilla') + R.gan_loss(pr, True, 'vanilla')) * 0.5).backward()
        d2_own = sd2
    for n, sd in (('G', st.g), ('D_1', st.d[0]), ('D_2', st.d[1] if d2_own is None else d2_own), ('D_3', st.d[2])):
        net = getattr(model, 'net' + n)
        msd, params = net.state_dict(), dict(net.named_parameters())
        for k, v in sd.items():
            if not (k.endswith('weight_orig') or k.endswith('.weight') or k.endswith('.bias')) or v.dtype != torch.float32 or v.grad is None:
                continue
            g_ref, g = v.grad.detach(), params[k].grad.detach().cpu()
            rel = (g - g_ref).norm().item() / max(g_ref.norm().item(), 1e-12)
            # 1-D tensors (biases, BatchNorm affine) are sums over all pixels with heavy cancellation: fp16 operand rounding upstream shows
            # up as a larger RELATIVE error there (observed up to 14 %), while the fp32 mode stays below 2e-3 everywhere
            assert rel <= (gtol if g.dim() > 1 else vtol), (n, k, rel)
            if precision == 'fp32':
                d = (msd[k].detach().cpu() - v.detach()).abs()
                assert (d > 1e-4).float().mean().item() <= 2e-3, (n, k, d.max().item())


def test_graph_recapture_when_the_batch_shape_changes(monkeypatch):
    """A last, smaller batch of an epoch: the new shape warms up eagerly and gets its own captured graphs; when the full batch size comes
    back its graphs (and input buffers) are still there -- every shape is captured once.  Results stay those of eager launches."""
    monkeypatch.setenv('HV_PRECISION', 'fp16')
    import hvgan
    from hvgan import synth
    from hvgan.models.pix2pix_model import Pix2PixModel

    def run(use_graph):
        torch.manual_seed(7)
        model = Pix2PixModel(make_opt())
        model.use_graph = use_graph
        seen = []
        for step, B in enumerate((2, 2, 2, 2, 1, 1, 1, 2, 2, 2)):
            model.set_input(synth.make_batch(B, 256, seed=900 + step))
            model.optimize_parameters()
            seen.append(model._graphs is not None)
            assert model.fake_B.shape[0] == B and model.get_current_visuals()['fake_B_raw'].shape[0] == B   # names follow the active shape
        torch.cuda.synchronize()
        return seen, {k: v.detach().clone() for k, v in model.netG.state_dict().items()}, model.get_current_losses()

    se, we, le = run(False)
    sg, wg, lg = run(True)
    assert sg == [False, False, True, True, False, False, True, True, True, True] and not any(se)
    bad = [(k, (we[k].float() - wg[k].float()).abs().max().item()) for k in we if not torch.equal(we[k], wg[k])]
    assert not bad, ('%d of %d tensors differ' % (len(bad), len(we)), bad[:8])
    assert le == lg


# what forward() / the phases bound per batch shape before ShapeState recorded it (the hand-kept list it replaces): none may drop out
STEP_BOUND = ('fake_B', 'fake_B_coarse', 'fake_B_local', 'real_B_local', 'fake_B_mask_raw', 'coarse_seg_binary', 'coarse_seg_sigmoid', 'fake_B_mask_sigmoid',
              'x_stage1', 'fake_B_raw', 'pred1_h', 'pred2_h', 'real_edges', 'fake_edges', '_gplan', '_rows', '_dxs')
SHAPE_SEQUENCE = (2, 2, 2, 2, 1, 1, 1, 2, 2)


def _shape_sequence_run(use_graph, after_step):
    from hvgan import synth
    from hvgan.models.pix2pix_model import Pix2PixModel
    torch.manual_seed(7)
    model = Pix2PixModel(make_opt())
    model.use_graph = use_graph
    for step, B in enumerate(SHAPE_SEQUENCE):
        model.set_input(synth.make_batch(B, 256, seed=900 + step))
        model.optimize_parameters()
        after_step(model, step, B)
    torch.cuda.synchronize()


def test_every_bound_tensor_follows_the_active_batch_shape(monkeypatch):
    """Batch sizes 2, 2, 2, 2, 1, 1, 1, 2, 2 with graphs on (fp16 mode): after every step each name the active ShapeState recorded is, on the model,
    that very tensor, with the current batch size in front; when batch size 2 comes back its tensors are the buffers of its first visit."""
    monkeypatch.setenv('HV_PRECISION', 'fp16')
    import hvgan  # noqa: F401
    first = {}

    def check(model, step, B):
        bound = model._cur.bound
        assert set(STEP_BOUND) <= set(bound), sorted(set(STEP_BOUND) - set(bound))
        tensors = {n: t for n, t in bound.items() if isinstance(t, torch.Tensor)}
        assert len(tensors) >= len(STEP_BOUND) - 2      # (_gplan is the generator's plan, _dxs a dict of tensors)
        for n, t in tensors.items():
            assert getattr(model, n) is t, (step, B, n)
            if t.dim() == 4 or n == '_rows':      # (B, ...); pred1_h / pred2_h are (1, B)
                assert t.shape[0] == B, (step, B, n, tuple(t.shape))
        assert model.pred1_h.shape == model.pred2_h.shape == (1, B)
        ptrs = {n: t.data_ptr() for n, t in tensors.items()}
        if B == 2:
            assert first.setdefault(2, ptrs) == ptrs, (step, [n for n in ptrs if first[2].get(n) != ptrs[n]])
        else:
            assert not set(ptrs.values()) & set(first[2].values()), (step, B)

    _shape_sequence_run(True, check)


def test_replay_after_a_shape_comes_back_shows_that_shape_s_visuals(monkeypatch):
    """The same sequence: the first step after batch size 2 returns is a pure graph replay (no Python rebinds anything), and get_current_visuals()
    must show THAT step's batch-size-2 images: bit for bit those of a run that launches every step eagerly."""
    monkeypatch.setenv('HV_PRECISION', 'fp16')
    import hvgan  # noqa: F401
    back = SHAPE_SEQUENCE.index(2, SHAPE_SEQUENCE.index(1))
    seen = {}

    def grab(use_graph):
        def after(model, step, B):
            if step == back:
                assert (model._graphs is not None) == use_graph
                assert list(model.get_current_visuals()) == model.visual_names
                seen[use_graph] = {n: v.detach().clone() for n, v in model.get_current_visuals().items()}
        return after

    _shape_sequence_run(False, grab(False))
    _shape_sequence_run(True, grab(True))
    for n, v in seen[True].items():
        assert v.shape[0] == 2, (n, tuple(v.shape))
        assert torch.equal(v, seen[False][n]), (n, (v.float() - seen[False][n].float()).abs().max().item())


def test_step_at_512_matches_live_oracle(monkeypatch):
    """BASELINE config #5's slice size: one full train step at 512 x 512 (attention over 128 x 128 patches, L = 4096; 62 x 62 PatchGAN logits)
    from seeded weights against the CPU oracle on the same weights and batch -- nothing in the kernels or the host mirror is tied to 256."""
    monkeypatch.setenv('HV_PRECISION', 'fp32')
    import hvgan
    from hvgan import synth
    from hvgan.models.pix2pix_model import Pix2PixModel
    from oracle import restate as R
    torch.manual_seed(99)
    model = Pix2PixModel(make_opt())
    sd_g = {k: v.detach().cpu().clone() for k, v in model.netG.state_dict().items()}
    sd_d = [{k: v.detach().cpu().clone() for k, v in getattr(model, 'netD_%d' % k).state_dict().items()} for k in (1, 2, 3)]
    raw = synth.make_batch(2, 512, seed=31)
    model.set_input(raw)
    model.optimize_parameters()
    torch.cuda.synchronize()
    st = R.StepState(sd_g, sd_d, lr=2e-4, beta1=0.5, norm='batch', gan_mode='vanilla', lambda_l1=200.0)
    losses, outs = R.pix2pix_step(st, synth.to_model_inputs(raw))
    got = model.get_current_losses()
    for k, ref in losses.items():
        assert abs(got[k] - ref) <= 2e-3 * max(1.0, abs(ref)), (k, got[k], ref)
    for name in ('fake_B', 'fake_B_coarse', 'x_stage1', 'fake_B_raw', 'coarse_seg_sigmoid', 'fake_B_mask_sigmoid'):
        ref = outs[{'coarse_seg_sigmoid': 'coarse_seg', 'fake_B_mask_sigmoid': 'fine_seg'}.get(name, name)]
        assert getattr(model, name).shape == ref.shape == (2, 1, 512, 512)
        check_activation(name, getattr(model, name), ref, ctx=(512,))


@pytest.mark.parametrize('norm,gan_mode', [('instance', 'vanilla'), ('batch', 'lsgan'), ('instance', 'lsgan')])
def test_train_step_instance_norm_and_lsgan_match_live_oracle(norm, gan_mode, monkeypatch):
    """The north-star's InstanceNorm+LeakyReLU discriminators (--norm instance) and the least-squares GAN loss (--gan_mode lsgan) through a
    FULL train step (reference pix2pix_model.py:67 `opt.norm`, networks.py:212-278), fp32 mode, against the CPU oracle on the same weights
    and batch: 12 losses, activations, every parameter gradient, and the losses of a second step taken from the updated weights."""
    monkeypatch.setenv('HV_PRECISION', 'fp32')
    import hvgan
    from hvgan import synth
    from hvgan.models.pix2pix_model import Pix2PixModel
    from oracle import restate as R
    torch.manual_seed(2024)
    model = Pix2PixModel(make_opt(norm=norm, gan_mode=gan_mode))
    sd_g = {k: v.detach().cpu().clone() for k, v in model.netG.state_dict().items()}
    sd_d = [{k: v.detach().cpu().clone() for k, v in getattr(model, 'netD_%d' % k).state_dict().items()} for k in (1, 2, 3)]
    st = R.StepState(sd_g, sd_d, lr=2e-4, beta1=0.5, norm=norm, gan_mode=gan_mode, lambda_l1=200.0)
    for step in range(2):
        raw = synth.make_batch(2, 256, seed=60 + step)
        model.set_input(raw)
        model.optimize_parameters()
        torch.cuda.synchronize()
        losses, outs = R.pix2pix_step(st, synth.to_model_inputs(raw))
        got = model.get_current_losses()
        for k, ref in losses.items():
            assert abs(got[k] - ref) <= (2e-3 if step == 0 else 1e-2) * max(1.0, abs(ref)), (step, k, got[k], ref)
        if step:
            break
        for name in ('fake_B', 'x_stage1', 'fake_B_raw', 'coarse_seg_sigmoid', 'fake_B_mask_sigmoid'):
            ref = outs[{'coarse_seg_sigmoid': 'coarse_seg', 'fake_B_mask_sigmoid': 'fine_seg'}.get(name, name)]
            check_activation(name, getattr(model, name), ref, ctx=(norm, gan_mode))
        for n, sd in (('G', st.g), ('D_1', st.d[0]), ('D_2', st.d[1]), ('D_3', st.d[2])):
            params = dict(getattr(model, 'net' + n).named_parameters())
            for k, v in sd.items():
                if v.dtype != torch.float32 or getattr(v, 'grad', None) is None:
                    continue
                if norm == 'instance' and n != 'G' and k in ('model.2.bias', 'model.5.bias', 'model.8.bias'):
                    # a conv bias in front of an InstanceNorm (no affine) has an exactly-zero true gradient -- the norm removes the
                    # per-channel mean: both sides hold uncorrelated round-off noise of the sums there, nothing to compare
                    continue
                g_ref, g = v.grad.detach(), params[k].grad.detach().cpu()
                err = (g - g_ref).norm().item()
                assert err <= 2e-3 * g_ref.norm().item(), (norm, gan_mode, n, k, err, g_ref.norm().item())


def test_unet_ct_mask_full_size_config1_matches_live_oracle(monkeypatch):
    """BASELINE config #1 at its real size: UnetG_CT_mask.define_G(3, 1, 64, ...) -- ngf=64, so the 512/1024-channel
    conv-transpose layers the mini fixture (G6, ngf=4 at 64^2) never reaches -- one 256x256 slice, pix2pix L1 loss, forward + backward +
    BatchNorm running statistics against the CPU oracle (oracle.restate.unet_forward, pinned by G6) on the same seeded weights."""
    monkeypatch.setenv('HV_PRECISION', 'fp32')
    import hvgan  # noqa: F401
    from hvgan.models.UnetG_CT_mask import define_G
    from oracle import restate as R
    torch.manual_seed(64)
    net = define_G(3, 1, 64, 'unet_256', 'batch', False, 'normal', 0.02, [])
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(5)
    x = torch.rand(1, 3, 256, 256, generator=g) * 2 - 1
    tgt = torch.rand(1, 1, 256, 256, generator=g) * 2 - 1
    dev = torch.device('cuda:0')
    net.cuda().train()
    net.precision = 'fp32'
    ct, mk = net(x.to(dev))
    loss = (ct - tgt.to(dev)).abs().mean()          # criterionL1 of the reference (pix2pix_model.py:125)
    loss.backward()
    torch.cuda.synchronize()
    params = [k for k in sd if (k.endswith('.weight') or k.endswith('.bias'))]
    for k in params:
        sd[k].requires_grad_(True)
    (rct, rmk), upd = R.unet_forward(sd, x, 5, True)
    rloss = (rct - tgt).abs().mean()
    rloss.backward()
    assert (ct.detach().cpu() - rct.detach()).abs().max().item() <= 1e-3
    assert (mk.detach().cpu() - rmk.detach()).abs().max().item() <= 1e-3
    assert abs(loss.item() - rloss.item()) <= 1e-4
    got = dict(net.named_parameters())
    for k in params:
        ref = sd[k].grad
        if ref is None:          # the mask decoder gets no gradient from an L1 loss on the CT output
            continue
        rel = (got[k].grad.detach().cpu() - ref).norm().item() / max(ref.norm().item(), 1e-12)
        assert rel <= 2e-3, (k, rel)
    now = net.state_dict()
    for k, v in upd.items():
        assert (now[k].detach().cpu().double() - v.double()).abs().max().item() <= 1e-4, k
    net.eval()
    with torch.no_grad():
        cte, mke = net(x.to(dev))
        for k, v in upd.items():
            sd[k] = v
        (rcte, rmke), _ = R.unet_forward({k: v.detach() for k, v in sd.items()}, x, 5, False)
    assert (cte.cpu() - rcte).abs().max().item() <= 1e-3 and (mke.cpu() - rmke).abs().max().item() <= 1e-3


@pytest.mark.parametrize('policy', ['linear', 'step'])
def test_learning_rate_schedule_reaches_the_captured_graphs(policy, monkeypatch):
    """get_scheduler / update_learning_rate (models/networks.py:39-65, base_model.py:124-134) with the learning rate living on
    the DEVICE and consumed inside captured hipGraphs.  train.py calls update_learning_rate() at the start of every epoch; here every "epoch"
    is one step, the decay window starts at once (`linear`: n_epochs 1, n_epochs_decay 3 -> factors 0.75, 0.5, 0.25, 0; `step`: gamma 0.1 every
    2 epochs), steps 3 and 4 replay the graphs captured after step 2.  The oracle takes the same scheduler on its own torch.optim.Adam.  Checked per
    step: the host lr sequence, the device scalar, the mean |dW| of every network against the oracle's (Adam's update is ~lr per element: a
    stale lr in a replayed graph is off by the decay factor), and with lr == 0 the weights must not move at all."""
    monkeypatch.setenv('HV_PRECISION', 'fp32')
    import hvgan
    from hvgan import synth
    from hvgan.models.pix2pix_model import Pix2PixModel
    from hvgan.models import networks as N
    from oracle import restate as R
    torch.manual_seed(2468)
    opt = make_opt(lr_policy=policy, n_epochs=1, n_epochs_decay=3, epoch_count=1, lr_decay_iters=2)
    model = Pix2PixModel(opt)
    model.setup(opt)
    sd_g = {k: v.detach().cpu().clone() for k, v in model.netG.state_dict().items()}
    sd_d = [{k: v.detach().cpu().clone() for k, v in getattr(model, 'netD_%d' % k).state_dict().items()} for k in (1, 2, 3)]
    st = R.StepState(sd_g, sd_d, lr=2e-4, beta1=0.5, norm='batch', gan_mode='vanilla', lambda_l1=200.0)
    o_opts = [st.opt_g] + list(st.opt_d)
    o_scheds = [N.get_scheduler(o, opt) for o in o_opts]

    def snapshot_model():
        return {n: torch.cat([p.detach().flatten().cpu() for p in getattr(model, 'net' + n).parameters()]) for n in ('G', 'D_1', 'D_2', 'D_3')}

    def snapshot_oracle():
        out = {'G': torch.cat([st.g[k].detach().flatten() for k in st.g_params])}
        for i in range(3):
            out['D_%d' % (i + 1)] = torch.cat([st.d[i][k].detach().flatten() for k in st.d_params[i]])
        return out

    want_lr = {'linear': [1.5e-4, 1.0e-4, 0.5e-4, 0.0], 'step': [2e-4, 2e-5, 2e-5, 2e-6]}[policy]
    for it in range(4):
        model.update_learning_rate()
        for s in o_scheds:
            s.step()
        lr = model.optimizers[0].param_groups[0]['lr']
        assert abs(lr - want_lr[it]) <= 1e-12 and abs(o_opts[0].param_groups[0]['lr'] - lr) <= 1e-12, (it, lr, want_lr[it])
        raw = synth.make_batch(2, 256, seed=900 + it)
        before_m, before_o = snapshot_model(), snapshot_oracle()
        model.set_input(raw)
        model.optimize_parameters()
        torch.cuda.synchronize()
        R.pix2pix_step(st, synth.to_model_inputs(raw))
        for o in model.optimizers:
            assert abs(o._lr.item() - lr) <= 1e-12 * max(1.0, lr) + 1e-10, (it, o._lr.item(), lr)      # the device scalar the Adam kernel reads
        after_m, after_o = snapshot_model(), snapshot_oracle()
        if it >= 2:
            assert model._graphs is not None, 'the step was not replayed from the captured graphs'
        for n in ('G', 'D_1', 'D_2', 'D_3'):
            dm, do = (after_m[n] - before_m[n]).abs().mean().item(), (after_o[n] - before_o[n]).abs().mean().item()
            if lr == 0.0:
                assert dm == 0.0 and do == 0.0, (policy, it, n, dm, do)
            else:
                assert abs(dm - do) <= 0.03 * do, (policy, it, n, dm, do, lr)
    # and the weights themselves still follow the oracle after four scheduled steps
    fin_m, fin_o = snapshot_model(), snapshot_oracle()
    for n in ('G', 'D_1', 'D_3'):
        d = (fin_m[n] - fin_o[n]).abs()
        assert (d > 5e-5).float().mean().item() <= 0.02, (policy, n, d.max().item())


def test_fp16_overflow_guard_skips_the_step_and_counts_it(monkeypatch):
    """fp16 storage mode: the gradient seeds carry a power-of-two scale; if a scaled activation gradient overflows an fp16 buffer, inf / nan reach
    the network's parameter gradients.  The Adam step then must not happen at all (weights, moments, step count), on the device, and be counted.
    Forced here with an absurd scale (2^40) for one step; with the normal scale the next step updates every network and the count stays."""
    monkeypatch.setenv('HV_PRECISION', 'fp16')
    import hvgan
    from hvgan import synth
    from hvgan.models.pix2pix_model import Pix2PixModel
    torch.manual_seed(31)
    model = Pix2PixModel(make_opt())
    nets = ('G', 'D_1', 'D_2', 'D_3')
    snap = lambda: {n: torch.cat([p.detach().flatten().clone() for p in getattr(model, 'net' + n).parameters()]) for n in nets}
    w0 = snap()
    assert model.grad_scale == 8192.0
    model.grad_scale = float(2 ** 40)
    model.set_input(synth.make_batch(2, 256, seed=5))
    model.optimize_parameters()
    torch.cuda.synchronize()
    assert model.overflow_steps() == {n: 1 for n in nets}, model.overflow_steps()
    w1 = snap()
    for n in nets:
        assert torch.equal(w0[n], w1[n]), n
        o = getattr(model, 'optimizer_' + n)
        assert float(o._step[0].item()) == 0.0 and float(o._m.abs().max().item()) == 0.0 and float(o._v.abs().max().item()) == 0.0, n
    model.grad_scale = 8192.0
    model.set_input(synth.make_batch(2, 256, seed=6))
    model.optimize_parameters()
    torch.cuda.synchronize()
    w2 = snap()
    assert model.overflow_steps() == {n: 1 for n in nets}
    for n in nets:
        assert torch.isfinite(w2[n]).all() and (w2[n] - w1[n]).abs().max().item() > 1e-5, n
        assert float(getattr(model, 'optimizer_' + n)._step[0].item()) == 1.0


def test_guarded_adam_equals_torch_adam_and_ignores_a_poisoned_gradient():
    import hvgan
    from hvgan.optim import FusedAdam
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(3)
    flat_p = torch.randn(5000, generator=g).to(dev)
    flat_g = torch.zeros(5000, device=dev)
    ps = [torch.nn.Parameter(flat_p[:3000].view(30, 100)), torch.nn.Parameter(flat_p[3000:])]
    ps[0].grad, ps[1].grad = flat_g[:3000].view(30, 100), flat_g[3000:]
    ref = [torch.nn.Parameter(p.detach().cpu().clone()) for p in ps]
    opt, ropt = FusedAdam(ps, lr=2e-4, betas=(0.5, 0.999)), torch.optim.Adam(ref, lr=2e-4, betas=(0.5, 0.999))
    for it in range(4):
        gr = torch.randn(5000, generator=g)
        if it == 1:
            gr[4321] = float('inf') if True else 0.0
        if it == 2:
            gr[17] = float('nan')
        flat_g.copy_(gr)
        opt.step(guard_flat=flat_g)
        if it in (0, 3):
            ref[0].grad, ref[1].grad = gr[:3000].view(30, 100).clone(), gr[3000:].clone()
            ropt.step()
        torch.cuda.synchronize()
        for p, r in zip(ps, ref):
            assert (p.detach().cpu() - r.detach()).abs().max().item() <= 1e-6, it
    assert opt.skipped_steps() == 2 and float(opt._step[0].item()) == 2.0


@pytest.mark.parametrize('precision', ['fp32', 'fp16'])
def test_weight_writes_between_public_discriminator_passes_refresh_the_tables(precision, monkeypatch):
    """backward_D_k lays its weight tables out only when they are stale (prep='if_stale').  An optimiser step and a load_state_dict between two
    backward_D_1 calls must make the second one lay them out again: losses and flat gradients bit-identical to a run that never skips."""
    monkeypatch.setenv('HV_PRECISION', precision)
    monkeypatch.setenv('HV_GRAPH', '0')
    import hvgan
    from hvgan import engine, synth
    from hvgan.models.pix2pix_model import Pix2PixModel

    def run(skip):
        monkeypatch.setattr(engine, 'PREP_SKIP', skip)
        torch.manual_seed(41)
        model = Pix2PixModel(make_opt())
        other = {k: v.clone() for k, v in model.netD_2.state_dict().items()}
        model.set_input(synth.make_batch(2, 256, seed=41))
        model.forward()
        out = []

        def d1():
            model.backward_D_1()
            out.extend([torch.stack([model.loss_D_fake_1, model.loss_D_real_1]).clone(), model.netD_1.paramset().flat_grad.clone()])
        d1()
        model.optimizer_D_1.step()
        d1()
        model.netD_1.load_state_dict(other)
        d1()
        torch.cuda.synchronize()
        return out

    got, ref = run(True), run(False)
    for i, (a, b) in enumerate(zip(got, ref)):
        assert torch.equal(a, b), (precision, i, (a - b).abs().max().item())


def test_public_per_method_order_equals_optimize_parameters_in_fp16(monkeypatch):
    """The reference's public train-step API -- forward(), backward_D_k() + optimizer_D_k.step() for k = 1..3, backward_G() + optimizer_G.step() --
    in the fp16 mode (scaled gradients in .grad until the bound optimisers step): two steps leave the same weights, BatchNorm statistics and Adam
    state, bit for bit, as optimize_parameters() from the same seed (the same kernels per network, in the same order)."""
    monkeypatch.setenv('HV_PRECISION', 'fp16')
    monkeypatch.setenv('HV_GRAPH', '0')
    import hvgan
    from hvgan import synth
    from hvgan.models.pix2pix_model import Pix2PixModel
    nets = ('G', 'D_1', 'D_2', 'D_3')

    def run(public):
        torch.manual_seed(77)
        model = Pix2PixModel(make_opt())
        for step in range(2):
            model.set_input(synth.make_batch(2, 256, seed=70 + step))
            if not public:
                model.optimize_parameters()
                continue
            model.forward()
            for k in (1, 2, 3):
                model.set_requires_grad(getattr(model, 'netD_%d' % k), True)
                getattr(model, 'optimizer_D_%d' % k).zero_grad()
                getattr(model, 'backward_D_%d' % k)()
                getattr(model, 'optimizer_D_%d' % k).step()
            model.set_requires_grad([model.netD_1, model.netD_2, model.netD_3], False)
            model.optimizer_G.zero_grad()
            model.backward_G()
            model.optimizer_G.step()
        torch.cuda.synchronize()
        state = {n + '/' + k: v.detach().clone() for n in nets for k, v in getattr(model, 'net' + n).state_dict().items()}
        for n in nets:
            o = getattr(model, 'optimizer_' + n)
            state.update({n + '/adam_m': o._m.clone(), n + '/adam_v': o._v.clone(), n + '/adam_step': o._step[:3].clone()})
        return state

    a, b = run(True), run(False)
    bad = [(k, (a[k].double() - b[k].double()).abs().max().item()) for k in a if not torch.equal(a[k], b[k])]
    assert not bad, ('%d of %d tensors differ' % (len(bad), len(a)), bad[:8])


def test_bridge_backward_then_bound_step_in_fp16(monkeypatch):
    """fp16 mode, netD_1 after the model's explicit backward (its .grad scaled by S): an nn.Module-bridge loss.backward() that accumulates onto
    those gradients adds true gradients to true gradients; after a fresh bridge backward the bound optimiser's step sees true gradients (no second
    unscale) and equals torch.optim.Adam on them."""
    monkeypatch.setenv('HV_PRECISION', 'fp16')
    monkeypatch.setenv('HV_GRAPH', '0')
    import hvgan
    from hvgan import synth
    from hvgan.models import networks
    from hvgan.models.pix2pix_model import Pix2PixModel
    torch.manual_seed(19)
    model = Pix2PixModel(make_opt())
    net, opt = model.netD_1, model.optimizer_D_1
    ps = net.paramset()
    crit = networks.GANLoss('vanilla').to(torch.device('cuda:0'))
    model.set_input(synth.make_batch(2, 256, seed=19))
    model.forward()
    model.backward_D_1()
    S = model.grad_scale
    assert S == 8192.0 and ps.grad_factor == S
    g1 = ps.flat_grad / S
    crit(net(model.fake_B.detach()), False).backward()          # accumulates (no zero_grad since the explicit backward)
    acc = ps.flat_grad.clone()
    assert ps.grad_factor == 1.0
    opt.zero_grad()
    crit(net(model.fake_B.detach()), False).backward()          # the same pass alone, assigned
    g2 = ps.flat_grad.clone()
    tol = 1e-5 * (g1.abs().max() + g2.abs().max()).item()
    assert (acc - (g1 + g2)).abs().max().item() <= tol, ((acc - (g1 + g2)).abs().max().item(), tol)
    ps_list = list(net.parameters())
    ref = [torch.nn.Parameter(p.detach().cpu().clone()) for p in ps_list]
    for r, p in zip(ref, ps_list):
        r.grad = p.grad.detach().cpu().clone()
    ropt = torch.optim.Adam(ref, lr=2e-4, betas=(0.5, 0.999))
    opt.step()
    ropt.step()
    torch.cuda.synchronize()
    assert ps.grad_factor == 1.0 and opt.skipped_steps() == 0
    for p, r in zip(ps_list, ref):
        assert (p.detach().cpu() - r.detach()).abs().max().item() <= 1e-6


def test_step_at_512_fp16_mode_matches_live_oracle(monkeypatch):
    """BASELINE config #5's slice size in the benchmarked fp16 mode (the fp32-mode 512^2 test is above): one full train step, B = 2, against the
    CPU oracle on the same weights -- continuous activations within |d| <= 1e-3, the 12 losses within the fp16-mode tolerances."""
    monkeypatch.setenv('HV_PRECISION', 'fp16')
    import hvgan
    from hvgan import synth
    from hvgan.models.pix2pix_model import Pix2PixModel
    from oracle import restate as R
    torch.manual_seed(512)
    model = Pix2PixModel(make_opt())
    sd_g = {k: v.detach().cpu().clone() for k, v in model.netG.state_dict().items()}
    sd_d = [{k: v.detach().cpu().clone() for k, v in getattr(model, 'netD_%d' % k).state_dict().items()} for k in (1, 2, 3)]
    raw = synth.make_batch(2, 512, seed=99)
    model.set_input(raw)
    model.optimize_parameters()
    torch.cuda.synchronize()
    st = R.StepState(sd_g, sd_d, lr=2e-4, beta1=0.5, norm='batch', gan_mode='vanilla', lambda_l1=200.0)
    losses, outs = R.pix2pix_step(st, synth.to_model_inputs(raw))
    got = model.get_current_losses()
    for k, ref in losses.items():
        tol = 3e-2 if k in ('edge', 'D_real_2', 'D_fake_2', 'G_GAN') else 6e-3        # behind the fine_seg > 0.5 threshold: a few flipped pixels
        assert abs(got[k] - ref) <= tol * max(1.0, abs(ref)), (k, got[k], ref)
    for name in ('x_stage1', 'fake_B_raw', 'coarse_seg_sigmoid', 'fake_B_mask_sigmoid'):
        ref = outs[{'coarse_seg_sigmoid': 'coarse_seg', 'fake_B_mask_sigmoid': 'fine_seg'}.get(name, name)]
        check_activation(name, getattr(model, name), ref, tol=1e-3, ctx=('fp16', 512))
    assert model.overflow_steps() == {n: 0 for n in ('G', 'D_1', 'D_2', 'D_3')}


def test_fp16_mode_tracks_fp32_mode_over_a_short_training_run(monkeypatch):
    """The fp16 storage mode (static gradient scale 8192 + overflow guard) against the exact-fp32 parity mode over 30 graph-replayed train steps from
    the same initialisation on the same eight batches: the supervised losses stay within 1 %, the discriminator losses within 0.03, and the guard
    skips no step.  (GAN dynamics amplify rounding differences: by step ~40 the two runs drift apart while staying in the same regime --
    tools/fp16_vs_fp32_run.py prints both trajectories.)"""
    import math
    from hvgan import synth
    from hvgan.models.pix2pix_model import Pix2PixModel
    hist = {}
    for prec in ('fp32', 'fp16'):
        monkeypatch.setenv('HV_PRECISION', prec)
        torch.manual_seed(0)
        opt = make_opt()
        m = Pix2PixModel(opt)
        m.setup(opt)
        rows = []
        for step in range(30):
            m.set_input(synth.make_batch(4, 128, seed=10_000 + step % 8))
            m.optimize_parameters()
            if step % 10 == 9:
                rows.append(m.get_current_losses())
        assert m._graphs is not None, 'the run must have gone through graph replay'
        assert m.overflow_steps() == {'G': 0, 'D_1': 0, 'D_2': 0, 'D_3': 0}
        hist[prec] = rows
        del m
    for a, b in zip(hist['fp32'], hist['fp16']):
        assert all(math.isfinite(v) for v in b.values()), b
        for k in ('G_maskL1', 'G_Dice', 'coarse_Dice', 'h'):
            assert abs(a[k] - b[k]) <= 0.01 * max(1.0, abs(a[k])), (k, a[k], b[k])
        for k in ('G_GAN', 'D_real_1', 'D_fake_1', 'D_real_2', 'D_fake_2', 'D_real_3', 'D_fake_3'):
            assert abs(a[k] - b[k]) <= 0.03, (k, a[k], b[k])
