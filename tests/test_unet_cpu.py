"""The UNet autoencoder without a GPU: the C ABI's declarations, refusals and launch geometry, the model's state_dict against the
reference's, the float64 restatement (tests/tools/unet_ref.py) against the goldens of the real reference classes, its upsample
against torch's, the command line and the checkpoint reader."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'tools'))

import unet_ref as R                                                                 # noqa: E402
from oracle.weights import digest                                                    # noqa: E402

P = 4096            # a dummy non-null device address; never dereferenced
DA_EINVAL = -1
NEW = ('da_unet_plan', 'da_unet_bias_relu', 'da_unet_bias_relu_pool2_fwd', 'da_unet_relu_upsample2_fwd', 'da_unet_relu_upsample2_bwd',
       'da_unet_pool2_skip_bwd', 'da_unet_relu_bwd', 'da_unet_out_fwd', 'da_unet_out_bwd')


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from deepards_amd import _lib
    return _lib.lib()


def test_library_declares_binds_and_builds_the_new_source(lib):
    from deepards_amd import _lib
    assert 'unet.hip' in _lib.SOURCES and os.path.exists(os.path.join(_lib.CSRC, 'unet.hip'))
    declared = _lib.header_symbols()
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and getattr(lib, name) is not None, name
    assert sorted(n for n in declared if n.startswith('da_unet_')) == sorted(NEW)
    from deepards_amd import hip_ops as H
    for name in ('unet_plan', 'unet_bias_relu', 'unet_bias_relu_pool2_fwd', 'unet_relu_upsample2_fwd', 'unet_relu_upsample2_bwd',
                 'unet_pool2_skip_bwd', 'unet_relu_bwd', 'unet_out_fwd', 'unet_out_bwd'):
        assert callable(getattr(H, name))


def _plan(lib, op, rows, l, c, ld):
    b, ws = ctypes.c_int(-7), ctypes.c_size_t(77)
    rc = lib.da_unet_plan(op, rows, l, c, ld, ctypes.byref(b), ctypes.byref(ws))
    return rc, b.value, ws.value


@pytest.mark.parametrize('rows,l,c,ld', [(3, 2, 32, 160), (3, 6, 96, 160), (5, 26, 64, 64), (320, 224, 64, 192), (1280, 28, 512, 512),
                                         (1280, 224, 64, 192)])
def test_plans_of_the_elementwise_entries(lib, rows, l, c, ld):
    """One thread per 4 channels of a position (bias_relu, relu_bwd, the upsamples: of a LOW-resolution position) or of a pair
    (the pools), 256 to a block, at most 16384 blocks (grid-stride beyond); no workspace."""
    from deepards_amd import hip_ops as H, unet_ops
    for op, name in enumerate(unet_ops.OPS[:6]):
        pairs = 'pool2' in name
        rc, b, ws = _plan(lib, op, rows, l, c, ld)
        assert rc == 0 and ws == 0
        threads = rows * (l // 2 if pairs else l) * (c // 4)
        assert b == min(-(-threads // 256), 16384), name
        assert H.unet_plan(name, rows, l, c, ld) == (b, 0)


@pytest.mark.parametrize('rows,l', [(3, 8), (5, 40), (320, 224), (1280, 224)])
def test_plans_of_the_output_stage(lib, rows, l):
    """16 positions per block pass, at most 512 blocks; one float per block (forward), a record of 68 (backward)."""
    blocks = min(-(-rows * l // 16), 512)
    assert _plan(lib, 6, rows, l, 64, 64) == (0, blocks, 4 * blocks)
    assert _plan(lib, 7, rows, l, 64, 64) == (0, blocks, 4 * 68 * blocks)
    assert _plan(lib, 6, rows, l, 32, 32)[0] == DA_EINVAL and _plan(lib, 7, rows, l, 64, 96)[0] == DA_EINVAL


def test_plan_and_entries_refuse_before_a_launch(lib):
    bad = [(3, 6, 48, 48), (3, 6, 32, 34), (3, 6, 64, 32), (0, 6, 32, 32), (3, 0, 32, 32), (1 << 16, 1 << 10, 64, 64)]
    for op in range(6):
        for rows, l, c, ld in bad:
            assert _plan(lib, op, rows, l, c, ld)[0] == DA_EINVAL, (op, rows, l, c, ld)
    for op in (1, 4):                                                                   # the pools: an even length
        assert _plan(lib, op, 3, 7, 32, 32)[0] == DA_EINVAL and _plan(lib, op, 3, 1, 32, 32)[0] == DA_EINVAL
    for op in (2, 3):                                                                   # the upsamples: L = 1 is a shape; 2 L must fit
        assert _plan(lib, op, 3, 1, 32, 32)[0] == 0 and _plan(lib, op, 1 << 15, 1 << 10, 64, 64)[0] == DA_EINVAL
    assert _plan(lib, 8, 3, 6, 32, 32)[0] == DA_EINVAL and _plan(lib, -1, 3, 6, 32, 32)[0] == DA_EINVAL
    assert lib.da_unet_plan(0, 3, 6, 32, 32, None, None) == DA_EINVAL
    # the entry points: a NULL operand, or a refused shape, before anything is launched (the addresses are never read)
    assert lib.da_unet_bias_relu(None, 32, P, 3, 6, 32, None) == DA_EINVAL
    assert lib.da_unet_bias_relu(P, 34, P, 3, 6, 32, None) == DA_EINVAL
    assert lib.da_unet_bias_relu_pool2_fwd(P, 32, P, None, 3, 6, 32, None) == DA_EINVAL
    assert lib.da_unet_bias_relu_pool2_fwd(P, 32, P, P, 3, 7, 32, None) == DA_EINVAL
    assert lib.da_unet_relu_upsample2_fwd(P, None, P, 32, 3, 6, 32, None) == DA_EINVAL
    assert lib.da_unet_relu_upsample2_fwd(P, P, P, 16, 3, 6, 32, None) == DA_EINVAL
    assert lib.da_unet_relu_upsample2_bwd(P, 32, P, P, None, 3, 6, 32, None) == DA_EINVAL
    assert lib.da_unet_relu_upsample2_bwd(P, 32, P, P, P, 3, 6, 40, None) == DA_EINVAL
    assert lib.da_unet_pool2_skip_bwd(P, P, 32, None, 32, P, 3, 6, 32, None) == DA_EINVAL
    assert lib.da_unet_pool2_skip_bwd(P, P, 32, P, 30, P, 3, 6, 32, None) == DA_EINVAL
    assert lib.da_unet_pool2_skip_bwd(P, P, 16, P, 32, P, 3, 6, 32, None) == DA_EINVAL
    assert lib.da_unet_relu_bwd(P, None, 32, P, 3, 6, 32, None) == DA_EINVAL
    assert lib.da_unet_relu_bwd(P, P, 32, P, -1, 6, 32, None) == DA_EINVAL
    assert lib.da_unet_out_fwd(P, P, P, P, P, P, P, None, 3, 8, None) == DA_EINVAL
    assert lib.da_unet_out_fwd(P, P, P, P, P, P, P, P, 0, 8, None) == DA_EINVAL
    assert lib.da_unet_out_bwd(P, P, P, P, P, None, P, 3, 8, 0, None) == DA_EINVAL
    assert lib.da_unet_out_bwd(P, P, P, P, P, P, P, 3, 0, 0, None) == DA_EINVAL


# ---- the model ------------------------------------------------------------------------------------------------------------------
def _golden_keys():
    return [str(k) for k in R.load_golden(4, 16)['keys']]


def test_state_dicts_have_the_golden_keys_and_shared_tensors():
    import deepards_amd.models as M
    unet = M.UNet(1)
    assert list(unet.state_dict().keys()) == R.state_dict_keys() and len(R.state_dict_keys()) == 46
    net = M.AutoencoderNetwork(M.UNet(1))
    sd = net.state_dict()
    assert list(sd.keys()) == _golden_keys() == R.network_keys() and len(sd) == 62
    u = net.base_network
    assert u.n_out_filters == 512 and net.breath_block is u.encoder and net.breath_block.n_out_filters == 512
    for k in range(1, 5):
        for leaf in ('0.weight', '0.bias', '2.weight', '2.bias'):
            a = sd['base_network.dconv_down%d.%s' % (k, leaf)]
            assert a.data_ptr() == sd['base_network.encoder.%d.%s' % (2 * (k - 1), leaf)].data_ptr() == \
                sd['breath_block.%d.%s' % (2 * (k - 1), leaf)].data_ptr()
    assert len(list(net.parameters())) == 30                                        # shared, not copied
    assert [n for n, _ in u.named_parameters()] == [n for n, _ in R.param_names()]
    assert [tuple(p.shape) for p in u.parameters()] == [s for _, s in R.param_names()]
    assert 'unet' not in M.BACKBONES and 'unet' not in M.base_networks and not isinstance(u, M.Backbone)
    assert isinstance(u.maxpool, torch.nn.MaxPool1d) and isinstance(u.upsample, torch.nn.Upsample) and u.precise_convs in (False, True)
    assert [tuple(getattr(u, 'dconv_up%d' % k)[0].weight.shape) for k in (3, 2, 1)] == [(256, 768, 3), (128, 384, 3), (64, 192, 3)]


def _reference_state_dict(seed=0):
    params = R.seeded_params(seed)
    return params, {k: torch.tensor(v, dtype=torch.float32) for k, v in R.network_state_dict(params).items()}


def test_reference_state_dict_loads_strictly():
    import deepards_amd.models as M
    params, sd = _reference_state_dict()
    net = M.AutoencoderNetwork(M.UNet(1))
    net.load_state_dict(sd, strict=True)
    for name, v in params.items():
        assert np.array_equal(dict(net.base_network.named_parameters())[name].detach().numpy(), v.astype(np.float32)), name
    unet = M.UNet(1)
    unet.load_state_dict({k[len('base_network.'):]: v for k, v in sd.items() if k.startswith('base_network.')}, strict=True)
    assert torch.equal(unet.encoder[6][2].bias, sd['base_network.dconv_down4.2.bias'])


def test_model_refuses_what_it_does_not_run(monkeypatch):
    import deepards_amd.models as M
    from deepards_amd import functional as F_, hip_ops as H
    with pytest.raises(NotImplementedError, match='n_class = 1'):
        M.UNet(2)
    net = M.AutoencoderNetwork(M.UNet(1))
    with pytest.raises(Exception, match='4 dimensional'):
        net(torch.zeros(4, 1, 32), None)
    with pytest.raises(NotImplementedError, match='multiple of 8'):
        net(torch.zeros(2, 2, 1, 36), None)
    with pytest.raises(NotImplementedError, match='multiple of 8'):
        net.base_network(torch.zeros(2, 1, 4))
    with pytest.raises(NotImplementedError, match='one channel'):
        net(torch.zeros(2, 2, 2, 32), None)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        net(torch.zeros(2, 2, 1, 32), None)
    with pytest.raises(NotImplementedError, match='no decisions'):
        net(torch.zeros(2, 2, 1, 32), None, sels=[None] * 3)
    with pytest.raises(NotImplementedError, match='second stage'):
        net.breath_block(torch.zeros(2, 1, 224))
    with torch.no_grad(), pytest.raises(RuntimeError, match='no CPU fallback'):
        net.breath_block(torch.zeros(2, 1, 224))
    monkeypatch.setattr(H, 'CONV_DTYPE', 'f32x3p')
    with pytest.raises(NotImplementedError, match='fp32 conv arithmetic and float activation storage only'):
        F_._unet_f32_only()
    monkeypatch.setattr(H, 'CONV_DTYPE', 'f32')
    monkeypatch.setattr(H, 'ACT', torch.bfloat16)
    with pytest.raises(NotImplementedError, match='fp32 conv arithmetic and float activation storage only'):
        F_.unet_forward(torch.zeros(2, 16), [], (), False)


def test_trainer_takes_the_unet_and_words_its_refusals_truthfully():
    import deepards_amd.models as M
    from deepards_amd.autoencoder import AutoencoderTrainer
    net = M.AutoencoderNetwork(M.UNet(1))
    with pytest.raises(NotImplementedError, match='one GPU.*not built') as e:
        AutoencoderTrainer(net, world_size=2)
    assert 'BatchNorm' not in str(e.value)
    with pytest.raises(NotImplementedError, match='folds in flight.*not built') as e:
        AutoencoderTrainer(M.UNet(1), folds_in_flight=2)
    assert 'BatchNorm' not in str(e.value)
    with pytest.raises(NotImplementedError, match='BatchNorm'):                          # (the CNN autoencoder's reason is unchanged)
        AutoencoderTrainer(M.AutoencoderNetwork(M.AutoencoderCNN()), world_size=2)


# ---- the restatement against the real reference ---------------------------------------------------------------------------------
@pytest.mark.parametrize('n,l', R.MODEL_SHAPES)
def test_restatement_reproduces_the_reference_goldens(n, l):
    g = R.load_golden(n, l)
    seed = int(g['seed'][0])
    res = R.forward_backward(R.seeded_rows(n, l, seed), R.seeded_params(seed))
    assert R.rel_l2(res['recon'], g['full/recon']) <= 1e-10 and R.rel_l2(res['loss'], g['loss']) <= 1e-10
    for name, _ in R.param_names():
        for key in ('grad/' + name, ):
            want = g['dig/' + key] if 'dig/' + key in g.files else g[key]
            got = digest(res[key]) if 'dig/' + key in g.files else res[key]
            assert R.rel_l2(got, want) <= 1e-10, key
    enc = digest(res['encoded']) if 'dig/encoded' in g.files else res['encoded']
    assert R.rel_l2(enc, g['dig/encoded'] if 'dig/encoded' in g.files else g['encoded']) <= 1e-10
    assert R.decisions_differ((res['relu'], res['pool']), R.golden_decisions(g)) == 0
    assert R.near_count(res) == int(g['near'][0])
    # forced with its own decisions it is the same function; forced with others it is another
    again = R.forward_backward(R.seeded_rows(n, l, seed), R.seeded_params(seed), decisions=(res['relu'], res['pool']))
    assert all(np.array_equal(again[k], res[k]) for k in res if k.startswith('grad/'))
    flipped = ([~m for m in res['relu'][:1]] + res['relu'][1:], res['pool'])
    assert not np.array_equal(R.forward_backward(R.seeded_rows(n, l, seed), R.seeded_params(seed), decisions=flipped)['recon'], res['recon'])


@pytest.mark.parametrize('l', [1, 2, 3, 7, 28, 56, 112])
def test_closed_form_upsample_is_torchs_and_its_adjoint_is_the_transpose(l):
    r = np.random.RandomState(l)
    x, d = r.standard_normal((3, 5, l)), r.standard_normal((3, 5, 2 * l))
    up = torch.nn.Upsample(scale_factor=2, mode='linear', align_corners=True)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    yt = up(xt)
    assert np.abs(R.upsample2(x) - yt.detach().numpy()).max() <= 1e-12
    yt.backward(torch.tensor(d, dtype=torch.float64))
    assert np.abs(R.upsample2_t(d) - xt.grad.numpy()).max() <= 1e-12
    lhs, rhs = float((R.upsample2(x) * d).sum()), float((x * R.upsample2_t(d)).sum())
    assert abs(lhs - rhs) <= 1e-12 * (np.abs(R.upsample2(x)) * np.abs(d)).sum()
    assert np.allclose(R.upsample2(np.ones((1, 1, l))), 1.0, rtol=0, atol=1e-15)       # every row of weights sums to 1


# ---- the command line, the driver class and the checkpoint reader -----------------------------------------------------------------
def test_module_parser_accepts_the_unet_and_the_main_parser_does_not():
    import deepards_amd.autoencoder as A
    import deepards_amd.train_ards_detector as T
    ns = A.build_parser().parse_args(['-n', 'autoencoder', '--base-network', 'unet', '-p', 'x.pkl'])
    assert (ns.network, ns.base_network) == ('autoencoder', 'unet')
    assert A.build_parser().parse_args(['-n', 'autoencoder', '--base-network', 'basic_cnn_ae']).base_network == 'basic_cnn_ae'
    with pytest.raises(SystemExit):
        T.build_parser().parse_args(['--base-network', 'unet'])
    import deepards_amd.models as M
    model = T.AutoencoderModel.__new__(T.AutoencoderModel)
    for name, cls in (('unet', M.UNet), ('basic_cnn_ae', M.AutoencoderCNN), ('resnet18', M.AutoencoderCNN), (None, M.AutoencoderCNN)):
        model.args = types.SimpleNamespace(base_network=name)
        assert type(model.get_base_network()) is cls, name
    with pytest.raises(NotImplementedError, match='folds-in-flight.*not built'):
        T.AutoencoderModel(T.make_args(network='autoencoder', base_network='unet', folds_in_flight=2, cuda_no_dp=True))


def _as_reference_pickle(net, path):
    """torch.save(net) with the classes claiming the reference's paths (deepards.models.unet.UNet, deepards.models.
    autoencoder_network.AutoencoderNetwork), as a file the reference pickled names them -- without the reference being importable."""
    import deepards_amd.models.autoencoder as A
    import deepards_amd.models.unet as U
    moved, fakes = [], {'deepards': types.ModuleType('deepards'), 'deepards.models': types.ModuleType('deepards.models')}
    for mod, refname in ((U, 'deepards.models.unet'), (A, 'deepards.models.autoencoder_network')):
        fake = fakes.setdefault(refname, types.ModuleType(refname))
        for name, obj in list(vars(mod).items()):
            if isinstance(obj, type) and obj.__module__ == mod.__name__:
                moved.append((obj, obj.__module__))
                obj.__module__ = refname
                setattr(fake, name, obj)
    saved = {k: sys.modules.get(k) for k in fakes}
    sys.modules.update(fakes)
    try:
        torch.save(net, path)
    finally:
        for obj, m in moved:
            obj.__module__ = m
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def test_load_autoencoder_round_trips_the_three_file_forms_and_load_base_network_refuses_them(tmp_path):
    import deepards_amd.models as M
    import deepards_amd.train_ards_detector as T
    from deepards_amd import checkpoint
    params, sd = _reference_state_dict(1)
    net = M.AutoencoderNetwork(M.UNet(1))
    net.load_state_dict(sd, strict=True)
    files = {'state_dict': str(tmp_path / 'unet_state.pth'), 'dataparallel': str(tmp_path / 'unet_dp.pth'),
             'own': str(tmp_path / 'unet_module.pth'), 'foreign': str(tmp_path / 'unet_reference.pth')}
    torch.save(sd, files['state_dict'])
    torch.save({'module.' + k: v for k, v in sd.items()}, files['dataparallel'])
    torch.save(net, files['own'])
    _as_reference_pickle(net, files['foreign'])
    assert checkpoint.checkpoint_kind(files['own']) == 'own' and checkpoint.checkpoint_kind(files['foreign']) == 'foreign'
    for form, path in files.items():
        back = checkpoint.load_autoencoder(path)
        assert isinstance(back, M.AutoencoderNetwork) and isinstance(back.base_network, M.UNet), form
        assert list(back.state_dict().keys()) == _golden_keys() and back.breath_block is back.base_network.encoder
        for name, v in params.items():
            assert np.array_equal(dict(back.base_network.named_parameters())[name].detach().numpy(), v.astype(np.float32)), (form, name)
        with pytest.raises(ValueError, match='not built in this package'):
            checkpoint.load_base_network(path, T.base_networks, {})
    # a UNet file with a key missing is not read as one; the CNN autoencoder's files still load as before
    short = dict(sd)
    del short['base_network.conv_last.bias']
    torch.save(short, files['state_dict'])
    with pytest.raises(ValueError, match='not an autoencoder checkpoint'):
        checkpoint.load_autoencoder(files['state_dict'])
    torch.save(M.AutoencoderNetwork(M.AutoencoderCNN()).state_dict(), files['state_dict'])
    assert isinstance(checkpoint.load_autoencoder(files['state_dict']).base_network, M.AutoencoderCNN)
