"""The se_resnet50 / 101 / 152 backbones without a GPU: the float64 oracle (tests/tools/sebn_ref.py) against the goldens written
from the reference's own classes, the model surface (names, order, refusals, parser), the gate-family rule and reference
checkpoints."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'tools'))

from oracle.weights import digest  # noqa: E402
import sebn_ref as R  # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
TOL = 1e-10
BLOCK_TAGS = ['id_4x2x56x256', 'id_6x3x5x1024', 'id_5x5x7x2048', 'e1_4x2x56x256', 's2_6x3x28x512', 's2_6x3x14x1024', 's2_5x5x7x2048']
NETS = {'se_resnet50': 18485232, 'se_resnet101': 33039408, 'se_resnet152': 45029360}        # backbone parameters


def _gold(name):
    z = np.load(os.path.join(GOLD, name), allow_pickle=False)
    return {k: z[k] for k in z.files}


def _against(g, key, value, tol=TOL):
    """value (float64 array) against the golden's entry: the tensor itself, or its digest."""
    value = np.asarray(value, np.float64)
    if key in g:
        ref, got = g[key], value.reshape(g[key].shape)
    else:
        ref, got = g['dig/' + key], digest(value)
    e = R.rel_l2(got, ref)
    assert e <= tol, (key, e)


@pytest.mark.parametrize('tag', BLOCK_TAGS)
def test_oracle_reproduces_the_block_goldens(tag):
    g = _gold('sebn_block_%s.npz' % tag)
    rows, R_, l_out, cin, planes, stride, ds, seed = (int(v) for v in g['cfg'])
    x0, params, dout = R.block_draws(rows, R_, l_out, cin, planes, stride, bool(ds), seed)
    x = g['x']
    assert x.shape == x0.shape and x.dtype == np.float32 and int(g['steps']) <= 2000
    assert R.rel_l2(x, x0) < 0.05                                      # the stored input is the draw, nudged
    m = R.block_margins(x, params, stride, R_)
    assert set(m) == {'h1', 'h2', 'hid', 'out'} and min(m.values()) >= R.MARGIN, (tag, m)
    r = R.block_case(x, params, stride, R_, dout)
    assert tuple(r['out'].shape) == (rows, l_out, 4 * planes)
    _against(g, 'out', r['out'].numpy())
    _against(g, 'dx', r['dx'].numpy())
    assert set(params) == {k[5:] for k in r if k.startswith('grad/')}
    for n in params:
        _against(g, 'grad/' + n, r['grad/' + n].numpy())
    assert max(float(g[k]) for k in g if k.startswith('err32/')) < 2e-6   # the reference's own fp32 run: the GPU tests' yardstick


def test_block_generator_is_deterministic_where_it_is_cheap():
    """The smallest case from scratch: sebn_ref.block_inputs finds the golden's input again."""
    g = _gold('sebn_block_e1_4x2x56x256.npz')
    rows, R_, l_out, cin, planes, stride, ds, seed = (int(v) for v in g['cfg'])
    x, _, _, steps = R.block_inputs(rows, R_, l_out, cin, planes, stride, bool(ds), seed)
    assert np.array_equal(x, g['x']) and steps == int(g['steps'])


@pytest.mark.parametrize('name,net', [('sebn_model_se_resnet50_nb20.npz', 'se_resnet50'), ('sebn_model_se_resnet50_nb20_shifted.npz', 'se_resnet50'),
                                      ('sebn_model_se_resnet101_nb2_shifted.npz', 'se_resnet101'),
                                      ('sebn_model_se_resnet152_nb2_shifted.npz', 'se_resnet152'),
                                      ('sebn_model_se_resnet50_b2_grads.npz', 'se_resnet50')])
def test_oracle_reproduces_the_model_goldens(name, net):
    g = _gold(name)
    nb, shift = int(g['nb']), float(g['bn_bias_shift'])
    assert shift == float(g['fc1_bias_shift']) == (2.0 if 'shifted' in name or 'grads' in name else 0.0)
    params = R.seeded_params(net, int(g['seed']), nb, bn_bias_shift=shift, fc1_bias_shift=shift)
    grads = 'grads' in name
    r = R.model_case(net, g['x'], g['target'], params, want_grads=grads)
    _against(g, 'logits', r['logits'].numpy())
    assert abs(float(r['loss']) - float(g['loss'])) <= 1e-12
    if grads:
        names = [n for n, _, _ in R.param_spec(net, nb)]
        assert len(names) == 225
        assert {'grad/' + n for n in names} == {k[4:] for k in g if k.startswith('dig/grad/')} | {k for k in g if k.startswith('grad/')}
        for n in names:
            _against(g, 'grad/' + n, r['grad/' + n].numpy(), 1e-9)
        unpinned = [str(n) for n in g['unpinned']]
        assert len(unpinned) <= 4 and all(float(g['err32/' + n]) > 2.5e-5 for n in unpinned)
        assert all(float(g[k]) <= 2.5e-5 for k in g if k.startswith('err32/grad/') and k[6:] not in unpinned)
    else:
        assert not any('grad/' in k for k in g)


@pytest.mark.parametrize('net', sorted(NETS))
def test_model_surface(net):
    import deepards_amd.models as M
    from deepards_amd import train_ards_detector as T
    assert M.base_networks[net] is getattr(M, net) and net in T.base_networks
    bb = M.base_networks[net]()
    assert bb.network_name == net and bb.n_out_filters == 2048 and bb.dropout is None and bb.inplanes == 2048
    assert sum(p.numel() for p in bb.parameters()) == NETS[net]
    assert [len(getattr(bb, 'layer%d' % i)) for i in (1, 2, 3, 4)] == list(R.LAYERS[net])
    nb = 2
    model = M.CNNLinearNetwork(bb, nb, 0)
    assert [n for n, _ in model.named_parameters()] == [n for n, _, _ in R.param_spec(net, nb)]
    assert [tuple(p.shape) for _, p in model.named_parameters()] == [sh for _, sh, _ in R.param_spec(net, nb)]
    gname = {'se_resnet50': 'sebn_model_se_resnet50_b2_grads.npz'}.get(net, 'sebn_model_%s_nb2_shifted.npz' % net)
    g = _gold(gname)
    sd = model.state_dict()
    assert list(sd.keys()) == [str(n) for n in g['names']]
    assert ['x'.join(map(str, v.shape)) for v in sd.values()] == [str(s) for s in g['shapes']]
    b0 = bb.layer1[0]
    assert isinstance(b0, M.SEResNetBottleneck) and b0.expansion == 4 and b0.precise_convs
    assert [n for n, _ in b0.named_children()] == ['conv1', 'bn1', 'conv2', 'bn2', 'conv3', 'bn3', 'relu', 'se_module', 'downsample']
    assert list(bb.layer1[1]._modules) == ['conv1', 'bn1', 'conv2', 'bn2', 'conv3', 'bn3', 'relu', 'se_module']     # (identity: None)
    assert bb.layer1[1].downsample is None and b0.downsample[0].stride == (1,) and b0.conv1.stride == (1,)
    assert bb.layer2[0].conv1.stride == (2,) and bb.layer2[0].conv2.stride == (1,) and bb.layer2[0].downsample[0].stride == (2,)
    assert [n for n, _ in b0.se_module.named_children()] == ['avg_pool', 'fc1', 'relu', 'fc2', 'sigmoid']
    assert tuple(bb.layer4[0].se_module.fc1.weight.shape) == (128, 2048, 1) and bb.layer4[0].se_module.fc1.bias is not None
    assert [n for n, _ in bb.named_children()] == ['layer0', 'layer1', 'layer2', 'layer3', 'layer4', 'avg_pool']
    args = T.build_parser().parse_args(['--base-network', net, '--train-from-pickle', 'x.pkl'])
    assert args.base_network == net


def test_network_map_is_unchanged():
    from deepards_amd import train_ards_detector as T
    assert sorted(T.network_map) == ['cnn_double_linear', 'cnn_linear', 'cnn_linear_compr_to_rf', 'cnn_linear_to_mean', 'cnn_lstm',
                                     'cnn_single_breath_linear']


def test_refused_constructions():
    import deepards_amd.models as M
    S, B = M.SENet, M.SEResNetBottleneck
    ok = dict(groups=1, reduction=16, dropout_p=None, inplanes=64, input_3x3=False, downsample_kernel_size=1, downsample_padding=0)
    S(B, [1, 1, 1, 1], **ok)
    for change in (dict(groups=64), dict(input_3x3=True), dict(dropout_p=0.2), dict(downsample_kernel_size=3, downsample_padding=1),
                   dict(groups=32), dict(reduction=4), dict(reduction=64), dict(inplanes=128)):
        with pytest.raises(NotImplementedError):
            S(B, [3, 4, 6, 3], **dict(ok, **change))            # (reduction 4: a hidden width of 512 at layer4; 64: of 4 at layer1)
    with pytest.raises(NotImplementedError):
        B(256, 64, 32, 16)                                      # groups != 1
    assert not hasattr(M, 'SEBottleneck') and not hasattr(M, 'SEResNeXtBottleneck')
    import deepards_amd.models.senet as senet
    assert not hasattr(senet, 'SEBottleneck') and not hasattr(senet, 'SEResNeXtBottleneck') and not hasattr(senet, 'senet154')

    class SEBottleneck(torch.nn.Module):                        # a block class by the reference's other names is not taken
        expansion = 4
    with pytest.raises(NotImplementedError):
        S(SEBottleneck, [3, 8, 36, 3], **ok)
    # conv arithmetic / storage the SE tail does not have: refused when forward_windows is entered, before any launch
    from deepards_amd import functional as F_
    net = M.se_resnet50()
    prev = F_.conv_dtype()
    try:
        for name in ('bf16', 'f32x3p'):
            F_.H.CONV_DTYPE = name
            with pytest.raises(NotImplementedError, match='f32'):
                net.forward_windows(torch.zeros(2, 1, 224), 2)
    finally:
        F_.H.CONV_DTYPE = prev
    with pytest.raises(RuntimeError, match='MI355X'):
        net.forward_windows(torch.zeros(2, 1, 224), 2)          # fp32: the usual no-CPU-path error


def test_eval_test_and_cnn_lstm_refuse_the_bottleneck_nets_like_the_resnets():
    import deepards_amd.models as M
    from deepards_amd import train_ards_detector as T
    from deepards_amd.train import HotPathTrainer
    with pytest.raises(NotImplementedError, match='running statistics'):
        HotPathTrainer(M.CNNLinearNetwork(M.se_resnet50(), 2, 0), eval_test=True)
    for net in sorted(NETS):
        with pytest.raises(NotImplementedError, match='running statistics'):
            T.network_map['cnn_lstm'](T.make_args(network='cnn_lstm', base_network=net))


def test_gate_family_rule():
    """se_ops.se_gate_family: a pure function of (C, Cr)."""
    from deepards_amd import se_ops as S
    assert S.se_gate_family(1024, 64) == S.WIDE == S.se_gate_family(2048, 128)            # above 512 channels: mandatory
    assert S.se_gate_family(768, 48) == S.WIDE and S.se_gate_family(320, 16) == S.WIDE    # shapes only the wide family takes
    for c in (64, 128, 256, 512):                               # se_resnet18's shapes (reduction 4) keep their kernels
        assert S.se_gate_family(c, c // 4) == S.NARROW
    assert S.se_gate_family(512, 256) == S.NARROW and S.se_gate_family(64, 64) == S.NARROW   # only the narrow family takes them
    for shape in ((256, 16), (512, 32)):                        # both take them: the timed choice, written down in one place
        assert S.se_narrow_ok(*shape) and S.se_wide_ok(*shape)
        assert S.se_gate_family(*shape) == (S.WIDE if shape in S.WIDE_SHARED else S.NARROW)
    assert S.WIDE_SHARED <= {(256, 16), (512, 32)}
    assert S.se_gate_family(512, 16) == S.NARROW and S.se_gate_family(256, 64) == S.NARROW   # shared, not timed: narrow
    for shape in ((96, 16), (4096, 128), (384, 24), (2048, 256), (1024, 8), (0, 16)):
        assert not S.se_wide_ok(*shape)
        with pytest.raises(NotImplementedError):
            S.se_gate_family(*shape)
    # the four stages of the bottleneck nets
    assert [S.se_wide_ok(256 << i, 16 << i) for i in range(4)] == [True] * 4


def test_header_declares_the_wide_family():
    from deepards_amd import _lib
    names = [n for n in _lib.SIGNATURES if n.startswith('da_se_wide_')]
    assert sorted(names) == ['da_se_wide_bwd_reduce', 'da_se_wide_bwd_scale', 'da_se_wide_chunk_rows', 'da_se_wide_gate_bwd',
                             'da_se_wide_gate_bwd_workspace', 'da_se_wide_gate_fwd', 'da_se_wide_scale_fwd', 'da_se_wide_shape_ok',
                             'da_se_wide_stats']
    assert set(names) <= set(_lib.header_symbols()) and 'se_wide.hip' in _lib.SOURCES
    from deepards_amd import hip_ops as H, se_ops
    for n in ('se_wide_stats', 'se_wide_gate_fwd', 'se_wide_scale_fwd', 'se_wide_bwd_reduce', 'se_wide_gate_bwd', 'se_wide_bwd_scale'):
        assert getattr(H, n) is getattr(se_ops, n) and getattr(H, n).__module__ == se_ops.__name__


def test_reference_checkpoint_lands_in_a_fresh_se_resnet50(tmp_path):
    """A whole module pickled under the reference's class paths (deepards.models.senet.*) is read without unpickling;
    --load-base-network builds a fresh se_resnet50 for it (no keyword arguments) and loads the breath_block.* weights."""
    from se_ref_paths import as_reference_classes
    from deepards_amd import checkpoint as C
    import deepards_amd.models as M
    path = str(tmp_path / 'ref_sebn.pth')

    def save(M_):
        torch.manual_seed(5)
        m = M_.CNNLinearNetwork(M_.se_resnet50(), 2, 0)
        torch.save(m, path, _use_new_zipfile_serialization=False)
        return m
    m = as_reference_classes(save)
    assert M.SEResNetBottleneck.__module__ == 'deepards_amd.models.senet'
    assert C.checkpoint_kind(path) == 'foreign'
    info = C.read_module_checkpoint(path)
    assert info['breath_block_class'] == 'deepards.models.senet.SENet' and info['network_name'] == 'se_resnet50'
    assert list(info['state_dict']) == list(m.state_dict())
    kw = dict(base_network='densenet18', resnet_kwargs=dict(initial_planes=64), densenet_kwargs=dict(with_fft=False))
    bb = C.load_base_network(path, M.base_networks, kw)
    assert isinstance(bb, M.SENet) and bb is not m.breath_block and bb.network_name == 'se_resnet50'
    assert isinstance(bb.layer3[5], M.SEResNetBottleneck)
    for (k, a), (_, b) in zip(bb.state_dict().items(), m.breath_block.state_dict().items()):
        assert torch.equal(a, b), k
    own = str(tmp_path / 'own_sebn.pth')                        # an own whole-module file round-trips through the restricted unpickler
    torch.save(m, own)
    back = C.load_own_module(own)
    assert isinstance(back.breath_block.layer1[0], M.SEResNetBottleneck)
    from deepards_amd import train_ards_detector as T
    cls = object.__new__(T.network_map['cnn_linear'])           # (the constructor needs a device; get_base_network does not)
    cls.args = T.make_args(base_network='se_resnet101', with_fft=True)
    assert cls.get_base_network().network_name == 'se_resnet101'
    cls.args = T.make_args(base_network='resnet18', load_base_network=path)
    assert cls.get_base_network().network_name == 'se_resnet50'  # the file's backbone, not --base-network
