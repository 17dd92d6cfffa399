"""CPU-only checks: the C ABI library builds, loads and exports every symbol include/hvgan.h declares; host-side
logic (state-dict keys, seeded initialisation, synthetic batch schema, loud failure without a GPU); the oracle's
full train step against the reference's golden losses; 2-rank gloo gradient averaging."""
import os
import subprocess
import sys

import pytest
import torch

from conftest import load_golden, ROOT


def test_library_builds_loads_and_exports_every_declared_symbol():
    import __graft_entry__ as g
    g.build()
    import hvgan
    from hvgan import lib
    L = lib.get()
    structs, protos = lib.parse_header()
    assert len(protos) >= 35
    for name in protos:
        assert hasattr(L.cdll, name), name
    assert L.cdll.hv_version() >= 100
    L.cdll.hv_arch.restype = __import__('ctypes').c_char_p
    assert L.cdll.hv_arch() == b'gfx950'


def test_state_dict_keys_match_reference_fixtures():
    import hvgan
    from hvgan.models.inpaint_networks import Generator
    from hvgan.models import networks
    from hvgan.models.UnetG_CT_mask import define_G
    g = load_golden('g1_generator_mini')
    net = Generator({'input_dim': 1, 'ngf': 4}, False)
    assert list(net.state_dict().keys()) == list(g['sd'].keys())
    net.load_state_dict(g['sd'])
    for norm in ('batch', 'instance'):
        gd = load_golden('g3_disc_%s' % norm)
        d = networks.define_D(1, 8, 'basic', 3, norm, 'normal', 0.02, [])
        assert list(d.state_dict().keys()) == list(gd['sd'].keys())
        d.load_state_dict(gd['sd'])
    gu = load_golden('g6_unet_mini')
    u = define_G(3, 1, 4, 'unet_256', 'batch', False, 'normal', 0.02, [])
    assert list(u.state_dict().keys()) == list(gu['sd'].keys())
    u.load_state_dict(gu['sd'])


def test_seeded_initialisation_equals_reference():
    import hvgan
    from hvgan.models.inpaint_networks import Generator
    g = load_golden('g7_inference')
    torch.manual_seed(77)
    net = Generator({'input_dim': 1, 'ngf': 16}, True)
    chk = torch.tensor([float(v.double().sum()) for v in net.state_dict().values()], dtype=torch.float64)
    assert torch.allclose(chk, g['init'].double(), rtol=1e-6, atol=1e-5)
    assert sum(p.numel() for p in net.parameters()) == 986888


def test_synthetic_batch_schema_and_geometry():
    from hvgan import synth
    b = synth.make_batch(3, 256, seed=5)
    for k in ('A', 'B', 'A_mask', 'mask', 'normal_vert', 'CAM'):
        assert b[k].shape == (3, 1, 256, 256) and b[k].dtype == torch.float32
    for k in ('height', 'x1', 'x2', 'h2'):
        assert b[k].shape == (3,) and b[k].dtype == torch.int64
    assert b['slice_ratio'].dtype == torch.float64 and len(b['A_paths']) == 3
    assert b['A'].min() >= -1 and b['A'].max() <= 1 and set(b['mask'].unique().tolist()) <= {0.0, 1.0}
    assert (b['mask'].sum(dim=(1, 2, 3)) == 40 * 256).all() and (b['x2'] - b['x1'] == b['height']).all()
    assert (b['height'] <= 40).all()
    b2 = synth.make_batch(3, 256, seed=5)
    assert torch.equal(b['A'], b2['A'])


def test_no_cpu_fallback_operators_fail_loudly():
    import hvgan
    from hvgan.models.inpaint_networks import Generator
    from hvgan.models.edge_operator import Sobel
    net = Generator({'input_dim': 1, 'ngf': 4}, False)
    x = torch.zeros(1, 1, 64, 64)
    with pytest.raises(RuntimeError):
        net(x, x, x, torch.zeros(1, dtype=torch.float64))
    with pytest.raises(RuntimeError):
        Sobel()(x)


def test_oracle_full_step_matches_reference_losses():
    """Oracle pix2pix_step on seed-constructed weights vs the reference's own optimize_parameters (G5)."""
    import hvgan
    from hvgan import synth
    from hvgan.models.inpaint_networks import Generator
    from hvgan.models.edge_operator import Sobel
    from hvgan.models import networks
    from oracle import restate as R
    g = load_golden('g5_full_step')
    torch.manual_seed(1234)
    G = Generator({'input_dim': 1, 'ngf': 16}, True)
    Sobel()
    Ds = [networks.define_D(1, 64, 'basic', 3, 'batch', 'normal', 0.02, []) for _ in range(3)]
    st = R.StepState(G.state_dict(), [d.state_dict() for d in Ds])
    torch.set_num_threads(8)
    losses, _ = R.pix2pix_step(st, synth.to_model_inputs(synth.make_batch(2, 256, seed=1234)))
    for k, v in g['losses0'].items():
        assert abs(losses[k] - float(v)) <= 1e-3 * max(1.0, abs(float(v))), (k, losses[k], float(v))


_DDP = r'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, %r)
import hvgan
from hvgan import ddp
rank, world = int(sys.argv[1]), 2
os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=sys.argv[2])
dist.init_process_group('gloo', rank=rank, world_size=world)
flat = torch.full((1000,), float(rank + 1))
gs = ddp.GradSync()
assert gs.reduce(flat) is None      # CPU tensors: reduced synchronously, no event
assert torch.allclose(flat, torch.full((1000,), 1.5)), flat[:3]
lin = torch.nn.Linear(4, 4)
ddp.broadcast_parameters([lin])
w = lin.weight.detach().clone()
dist.all_reduce(w)
assert torch.allclose(w, 2 * lin.weight.detach())
dist.destroy_process_group()
print('ok', rank)
'''


def test_gradient_averaging_two_ranks_gloo():
    port = str(29500 + os.getpid() % 2000)
    procs = [subprocess.Popen([sys.executable, '-c', _DDP % ROOT, str(r), port], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(2)]
    for p in procs:
        out, _ = p.communicate(timeout=300)
        assert p.returncode == 0 and b'ok' in out, out.decode()[-2000:]


def test_integration_doc_struct_matches_header():
    """The ctypes structs INTEGRATION.md shows a maintainer are generated from include/hvgan.h (tools/gen_integration_stub.py): the
    documented `_fields_` must equal what the product's own header parse yields, field for field -- a short struct would make the
    library read pointers from garbage."""
    import ctypes
    import re
    import hvgan  # noqa: F401
    from hvgan import lib
    text = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    blocks = re.findall(r'# >>> generated: (\w+)\n(.*?)# <<< generated', text, flags=re.S)
    assert blocks, 'INTEGRATION.md has no generated struct block'
    structs, _ = lib.parse_header()
    for name, src in blocks:
        assert src == lib.ctypes_source(name), 'INTEGRATION.md block for %s is stale: run python tools/gen_integration_stub.py' % name
        ns = {'ctypes': ctypes}
        exec(src, ns)
        doc = ns[name]
        assert [(n, t) for n, t in doc._fields_] == [(n, t) for n, t in structs[name]._fields_], name
        assert ctypes.sizeof(doc) == ctypes.sizeof(structs[name])
    # the example call in the same file names only fields the struct has, and all of them
    call = re.search(r'd = hv_conv_desc\((.*?)\)\n    rc', text, flags=re.S).group(1)
    used = set(re.findall(r'(\w+)=', call))
    assert used == {n for n, _ in structs['hv_conv_desc']._fields_}, used ^ {n for n, _ in structs['hv_conv_desc']._fields_}


def test_bench_starts_its_own_ranks_dry_run():
    """`python bench.py --gpus 2` from a plain shell (WORLD_SIZE unset) must start two ranks itself and report n_gpus == 2; the
    --dry-run form rehearses exactly that plumbing over gloo on the CPU: launcher, rendezvous on 127.0.0.1, the flat-gradient mean of
    the real networks' sizes through ddp.GradSync, barrier and MAX-over-ranks clock, one JSON line from rank 0."""
    import json
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--dry-run', '--steps', '2', '--warmup', '1'],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, env=env)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    lines = [l for l in p.stdout.decode().splitlines() if l.startswith('{')]
    assert len(lines) == 1, p.stdout.decode()[-2000:]
    rec = json.loads(lines[0])
    assert rec['n_gpus'] == 2 and rec['dry_run'] is True and rec['config']['bytes_per_round'] > 30e6
    # a rank count that differs from --gpus is an error, not a silently smaller run
    env2 = dict(env, WORLD_SIZE='1', RANK='0')
    q = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--dry-run'], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300, env=env2)
    assert q.returncode != 0 and b'--gpus 2' in q.stderr



def test_bench_dump_outputs_is_a_fixed_sample_within_64_mb(tmp_path):
    """bench.py --dump-outputs on a host stand-in for the trained model: computed visuals, heights and flattened parameters as float32, losses as
    float64, set_input's tensors left out; an array larger than DUMP_MAX_ELEMS is written as the SAME seeded sample in every run, and the whole
    dump stays within 64 MB even at 512 x 512."""
    import numpy as np
    import bench

    class Net(torch.nn.Module):
        def __init__(self, n):
            super().__init__()
            self.w = torch.nn.Parameter(torch.arange(n, dtype=torch.float32))
            self.b = torch.nn.Parameter(torch.ones(3))

    class Model:
        model_names = ['G', 'D_1']
        netG, netD_1 = Net(10), Net(3 << 20)
        pred1_h, pred2_h = torch.full((1, 16), 0.25), torch.full((1, 16), 0.5)

        def get_current_visuals(self):
            g = torch.Generator().manual_seed(3)
            return {n: torch.rand(16, 1, 512, 512, generator=g).half() for n in bench.INPUT_VISUALS + ('fake_B', 'fake_B_raw', 'real_edges')}

        def get_current_losses(self):
            return {'G_GAN': 0.75, 'h': 1.0 / 3.0}

    files = []
    for run in ('a', 'b'):
        total = bench.dump_outputs(Model(), str(tmp_path / run))
        assert total <= bench.DUMP_MAX_BYTES and total == sum(f.stat().st_size - 128 for f in (tmp_path / run).iterdir())
        files.append({f.name: np.load(str(f)) for f in (tmp_path / run).iterdir()})
    a, b = files
    assert sorted(a) == sorted(['visual_fake_B.npy', 'visual_fake_B_raw.npy', 'visual_real_edges.npy', 'pred1_h.npy', 'pred2_h.npy', 'params_G.npy',
                                'params_D_1.npy', 'loss_G_GAN.npy', 'loss_h.npy'])
    for n in a:
        assert np.array_equal(a[n], b[n]), n
        assert a[n].dtype == (np.float64 if n.startswith('loss_') else np.float32), n
    assert float(a['loss_h.npy']) == 1.0 / 3.0 and a['pred2_h.npy'].shape == (1, 16)
    assert np.array_equal(a['params_G.npy'], np.r_[np.arange(10), np.ones(3)].astype(np.float32))
    big = a['params_D_1.npy']            # w = arange(3 << 20), then the 3-element bias: a sorted sample without repeats, in w's part increasing
    assert big.shape == (bench.DUMP_MAX_ELEMS,) and np.all(np.diff(big[:-3]) > 0) and big.max() < (3 << 20)
    assert a['visual_fake_B.npy'].shape == (bench.DUMP_MAX_ELEMS,) and not np.array_equal(a['visual_fake_B.npy'], a['visual_fake_B_raw.npy'])


def test_oracle_data_parallel_step_is_the_mean_of_rank_gradients():
    """oracle.restate.pix2pix_step_data_parallel (the spec the GPU ranks are compared with): with the SAME batch on
    both ranks it must reproduce the single-process step bit for bit (the mean of two equal gradients); with different batches both
    ranks end with identical weights that differ from either single-rank result."""
    import torch
    import hvgan  # noqa: F401
    from hvgan import synth
    from hvgan.models.inpaint_networks import Generator
    from hvgan.models import networks
    from oracle import restate as R
    torch.manual_seed(5)
    G = Generator({'input_dim': 1, 'ngf': 4}, True)
    Ds = [networks.define_D(1, 8, 'basic', 3, 'batch', 'normal', 0.02, []) for _ in range(3)]
    mk = lambda: R.StepState(G.state_dict(), [d.state_dict() for d in Ds])
    b0 = synth.to_model_inputs(synth.make_batch(2, 64, seed=1))
    b1 = synth.to_model_inputs(synth.make_batch(2, 64, seed=2))
    single = mk()
    R.pix2pix_step(single, b0)
    a, b = mk(), mk()
    R.pix2pix_step_data_parallel([a, b], [b0, b0])
    for k in single.g_params:
        assert torch.equal(single.g[k], a.g[k]) and torch.equal(a.g[k], b.g[k]), k
    a, b = mk(), mk()
    R.pix2pix_step_data_parallel([a, b], [b0, b1])
    diff = 0
    for k in single.g_params:
        assert torch.equal(a.g[k], b.g[k]) and torch.equal(a.g[k].grad, b.g[k].grad), k
        diff += int(not torch.equal(a.g[k], single.g[k]))
    assert diff > 0
    for d in range(3):
        for k in a.d_params[d]:
            assert torch.equal(a.d[d][k], b.d[d][k]), (d, k)


def test_infer_prepare_slice_matches_reference_network_inputs():
    """infer.prepare_slice (the host-side slice preparation of the stage-batched inference driver) produces exactly the tensors the
    reference's run_model hands to the network (fixture G10, recorded by a stand-in network) and the same rows / height."""
    import numpy as np
    import torch
    import hvgan  # noqa: F401
    from hvgan import infer
    from oracle import restate as R
    from test_oracle_golden import g10_cases
    for name, ct, label, cam, vert_id, ratio, model, exp in g10_cases():
        p = infer.prepare_slice(cam, label, ct, vert_id)
        if exp is None:
            assert p is None, name
            continue
        q = R.infer_prepare(cam, label, ct, vert_id)
        assert (p['x1'], p['x2'], p['height']) == (q['x1'], q['x2'], q['height']) and p['height'] == int(exp['height'][0]), name
        assert torch.equal(torch.from_numpy(p['ct_masked'])[None], R.to_tensor_u8(exp['in_ct'], True)), name
        assert torch.equal(torch.from_numpy(p['mask'])[None], R.to_tensor_u8(exp['in_mask'], False)), name
        assert torch.equal(torch.from_numpy(p['cam'])[None], R.to_tensor_u8(exp['in_cam'], False)), name
        assert torch.equal(torch.from_numpy(p['ori_ct'])[None], q['ori_ct']), name


def test_no_kernel_spills_to_scratch():
    """The build records every kernel's registers / scratch bytes / occupancy from the compiler's resource-usage remarks
    (healthivert-gan_amd/csrc/build/*.resources.json).  A kernel that spills to scratch memory still computes the right numbers, only several
    times slower (a two-bodied activation epilogue once put the accumulators of every conv kernel in scratch and doubled the step time
    with all parity tests green), so spills are a test failure.  Allowed: instantiations no dispatch path takes."""
    import glob
    import json
    not_dispatched = (
        '_Z16conv_halo_kernelILi8ELi32ELi128ELi2ELi2ELi2ELi16ELi11ELb1EEv5HaloK',     # 8x32 tiles x 128 channels: the dispatch takes 8x16 tiles there
        '_Z16conv_halo_kernelILi8ELi32ELi128ELi2ELi2ELi2ELi32ELi11ELb1EEv5HaloK',
        '_Z15wgrad_tr_kernelILi4ELi2ELi64ELi32EEv4WTrK',                               # stride 2 with 64-channel blocks is planned with BC = 16
    )
    files = glob.glob(os.path.join(ROOT, 'healthivert-gan_amd', 'csrc', 'build', '*.resources.json'))
    if not files:
        pytest.skip('no resource records: the library was not built here by healthivert-gan_amd/csrc/build.py')
    seen = 0
    for f in files:
        for name, r in json.load(open(f)).items():
            seen += 1
            assert not r.get('scratch') or name in not_dispatched, (os.path.basename(f), name, r)
    assert seen > 200


def test_environment_variables_are_the_kept_list():
    """Every environment variable the library reads (getenv in csrc, os.environ in the package) is one of these.  The A/B switches of the tuning rounds
    were retired (their measurements stay in DESIGN.md section 4.5 and the commit log): a new one has to be added here on purpose."""
    import glob
    import re
    kept = {
        # operational settings
        'HV_PRECISION', 'HV_GRAD_SCALE', 'HV_GRAPH', 'HV_BATCH_D', 'HV_DDP_BACKEND', 'HV_DDP_FORCE', 'HV_DP_SCHEDULE', 'HV_DP_PREFLIGHT',
        'HV_DP_PREFLIGHT_TIMEOUT_S', 'HV_DP_CAPTURE_SETTLE_MS', 'HVGAN_LIB', 'HV_EXTRA_FLAGS', 'HIPCC',
        'WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT',      # torchrun
        # in-tree references of bit-identity tests (tests/test_generator_gpu.py), and of the ParamSet staleness check
        'HV_CONV_LF', 'HV_LF_PERSIST', 'HV_PREP_SKIP',
        # read only in the G4_STAMPS / WT_STAMPS diagnostic builds
        'HV_G4_DBG', 'HV_WTR_DBG',
    }
    pkg = os.path.join(ROOT, 'healthivert-gan_amd')
    seen = set()
    for f in glob.glob(os.path.join(pkg, 'csrc', '*.hip')) + glob.glob(os.path.join(pkg, 'csrc', '*.h')):
        seen |= set(re.findall(r'getenv\("([^"]+)"\)', open(f).read()))
    for f in glob.glob(os.path.join(pkg, '**', '*.py'), recursive=True):
        seen |= set(re.findall(r'environ(?:\.get\(|\.setdefault\(|\[)\s*[\'"]([^\'"]+)[\'"]', open(f).read()))
        seen |= set(re.findall(r'[\'"]([A-Z_]+)[\'"] not in os\.environ', open(f).read()))
    assert seen == kept, (sorted(seen - kept), sorted(kept - seen))


def test_tiled_filter_table_size_is_host_arithmetic():
    """hv_weight_tiled_elems (include/hvgan.h: rows padded to 16, a tiled form only when K % 16 == 0) is plain host code: callable without a GPU."""
    import hvgan  # noqa: F401
    from hvgan import lib
    if not lib.available():
        pytest.skip('libhvgan.so not built')
    L = lib.get()
    for rows, taps, K, want in ((512, 16, 256, 512 * 16 * 256), (20, 9, 48, 32 * 9 * 48), (4, 25, 16, 16 * 25 * 16), (64, 9, 36, 0), (1, 16, 512, 16 * 16 * 512),
                                (0, 9, 32, 0), (8, 0, 32, 0)):
        assert L.size('hv_weight_tiled_elems', rows, taps, K) == want, (rows, taps, K)


def test_attention_scores_are_a_box_filter_on_the_pixel_gram_matrix():
    """the 3x3 patches of contextual attention are both filters and inputs, so the reference's score matrix
    (models/inpaint_networks.py:327-344: conv2d of the padded map with its own normalised patches) equals rnorm[l] * sum over the 3x3 offsets t of
    G[l+t][p+t] with G the Gram matrix of the PIXELS (K = C instead of 9C), and the patch norms are the same sums on G's diagonal.  Held against
    the oracle's own tensors: the identity is what a blocked attention kernel would start from."""
    import torch.nn.functional as F
    from oracle import restate as R
    torch.manual_seed(0)
    c, h, w = 8, 6, 10
    L = h * w
    fd = torch.randn(1, c, h, w)
    wp = R._patches(fd, 3, 1)
    norm = torch.sqrt((wp ** 2).sum(dim=(2, 3, 4))).reshape(L)
    xp = F.unfold(R._same_pad(fd, 3, 1), kernel_size=3, stride=1)
    S = torch.bmm((wp / torch.clamp(norm, min=1e-4).view(1, L, 1, 1, 1)).reshape(1, L, -1), xp)[0]
    px = fd[0].reshape(c, L).t()
    G = (px @ px.t()).view(h, w, h, w)
    T = torch.zeros(h, w, h, w)
    for ty in (-1, 0, 1):
        for tx in (-1, 0, 1):
            ys = slice(max(0, -ty), h - max(0, ty)); xs = slice(max(0, -tx), w - max(0, tx))
            yd = slice(max(0, ty), h + min(0, ty)); xd = slice(max(0, tx), w + min(0, tx))
            T[ys, xs, ys, xs] += G[yd, xd, yd, xd]
    T = T.view(L, L)
    assert (S - T / torch.clamp(norm, min=1e-4).view(L, 1)).abs().max().item() <= 1e-4
    assert (T.diagonal().sqrt() - norm).abs().max().item() <= 1e-4


def test_conv_params_refuses_spectral_norm_on_a_conv_transpose_source():
    """weight_prep_kernel reads a spectral-norm layer's weight as [cout][cin * taps]; a transposed_src weight is [cin][cout][taps].  No model builds the
    combination, and ConvParams refuses it where it used to yield a wrong sigma silently."""
    import hvgan  # noqa: F401
    from hvgan import engine
    w = torch.zeros(8, 4, 3, 3)
    engine.ConvParams('plain_t', w, None, 8, 4, 3, transposed_src=True)
    engine.ConvParams('sn', torch.zeros(4, 8, 3, 3), None, 8, 4, 3, u=torch.zeros(4), v=torch.zeros(72))
    with pytest.raises(ValueError, match='transposed_src'):
        engine.ConvParams('sn_t', w, None, 8, 4, 3, u=torch.zeros(4), v=torch.zeros(72), transposed_src=True)


def test_conv_params_refuses_a_spectral_norm_layer_beyond_the_sigma_kernels_lds_arrays():
    """cin * k * k <= 4608 and cout <= 1024 (PREP_MAXK / PREP_MAXCO of csrc/prep.hip): the limits themselves pass, one more is a ValueError; layers without
    spectral norm have no such limit."""
    import re
    import hvgan  # noqa: F401
    from hvgan import engine
    src = open(os.path.join(ROOT, 'healthivert-gan_amd', 'csrc', 'prep.hip')).read()
    assert int(re.search(r'#define PREP_MAXK (\d+)', src).group(1)) == engine.SN_MAX_K == 4608
    assert int(re.search(r'#define PREP_MAXCO (\d+)', src).group(1)) == engine.SN_MAX_COUT == 1024
    sn = lambda cin, cout, k: engine.ConvParams('c', None, None, cin, cout, k, u=torch.zeros(cout), v=torch.zeros(cin * k * k))
    sn(512, 8, 3)
    sn(4, 1024, 2)
    for cin, cout, k in ((513, 8, 3), (4609, 1, 1), (4, 1025, 2), (289, 8, 4)):
        with pytest.raises(ValueError, match='4608'):
            sn(cin, cout, k)
    engine.ConvParams('plain', None, None, 1024, 2048, 3)


def test_weight_path_entries_refuse_bad_arguments_before_any_launch():
    """hv_adam_step(_guarded), hv_weight_prep(2) and hv_weight_prep_backward return HV_ERR_ARG / HV_ERR_UNSUPPORTED for these arguments before they touch
    the device: callable without a GPU, on pointers that are never followed."""
    import ctypes
    import hvgan  # noqa: F401
    from hvgan import lib
    L = lib.get()
    P = ctypes.c_void_p(0x10000)
    tab = lambda s, v=0x10000: ctypes.cast(ctypes.c_void_p(v), ctypes.POINTER(getattr(L, s)))
    ll, fl = ctypes.c_longlong, ctypes.c_float

    def guarded(t=tab('hv_adam_tensor'), nt=1, mx=8, lr=P, st=P, g=P, n=8, mul=1.0):
        L.call('hv_adam_step_guarded', t, nt, ll(mx), lr, fl(0.5), fl(0.999), fl(1e-8), st, g, ll(n), fl(mul), None)

    bad = [dict(g=ctypes.c_void_p(0x10004)), dict(g=ctypes.c_void_p(0x10008)), dict(mul=0.0), dict(mul=-1.0), dict(mul=float('nan')), dict(n=0), dict(n=-4),
           dict(nt=0), dict(mx=0), dict(t=tab('hv_adam_tensor', None)), dict(lr=None), dict(st=None), dict(g=None)]
    for kw in bad:
        with pytest.raises(RuntimeError, match='HV_ERR_ARG'):
            guarded(**kw)
    for t, nt, mx, lr, st in ((tab('hv_adam_tensor', None), 1, 8, P, P), (tab('hv_adam_tensor'), 0, 8, P, P), (tab('hv_adam_tensor'), 1, 0, P, P),
                              (tab('hv_adam_tensor'), 1, 8, None, P), (tab('hv_adam_tensor'), 1, 8, P, None)):
        with pytest.raises(RuntimeError, match='HV_ERR_ARG'):
            L.call('hv_adam_step', t, nt, ll(mx), lr, fl(0.5), fl(0.999), fl(1e-8), st, None)
    for t, n, mx in ((tab('hv_wprep_layer', None), 1, 8), (tab('hv_wprep_layer'), 0, 8), (tab('hv_wprep_layer'), 1, 0)):
        with pytest.raises(RuntimeError, match='HV_ERR_ARG'):
            L.call('hv_weight_prep', t, n, ll(mx), None)
        with pytest.raises(RuntimeError, match='HV_ERR_ARG'):
            L.call('hv_weight_prep2', t, n, ll(mx), 1, 1, None)
    for t, n, mx in ((tab('hv_wprep_bwd_layer', None), 1, 8), (tab('hv_wprep_bwd_layer'), 0, 8), (tab('hv_wprep_bwd_layer'), 1, 0), (tab('hv_wprep_bwd_layer'), -1, 8)):
        with pytest.raises(RuntimeError, match='HV_ERR_ARG'):
            L.call('hv_weight_prep_backward', t, n, ll(mx), 1, None)
    for mx in (1 << 31, (1 << 31) + 5, 1 << 40):
        with pytest.raises(RuntimeError, match='HV_ERR_UNSUPPORTED'):
            L.call('hv_weight_prep_backward', tab('hv_wprep_bwd_layer'), 1, ll(mx), 1, None)
