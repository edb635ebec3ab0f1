"""The se_resnext50_32x4d / se_resnext101_32x4d backbones without a GPU: the grouped-conv symbols and shape predicate, the
launch-free plan of the three kernels, the model surface, the float64 oracle (tests/tools/resnext_ref.py) against the goldens
written from the reference's own classes, and the refusals."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'tools'))

from oracle.weights import digest  # noqa: E402
import resnext_ref as R  # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
FLOOR = 16 * 2.0 ** -23
BLOCK_TAGS = ['e1_4x2x56x64', 'id_4x2x56x256', 's2_6x3x28x256', 's2_6x3x14x512', 's2_5x5x7x1024', 'id_5x5x7x2048']
NETS = {'se_resnext50_32x4d': ('resnext_model_se_resnext50_32x4d_nb20.npz', 382),
        'se_resnext101_32x4d': ('resnext_model_se_resnext101_32x4d_nb2_shifted.npz', 756)}
SYMBOLS = ('da_gconv3_shape_ok', 'da_gconv3_plan', 'da_gconv3_fwd', 'da_gconv3_dgrad', 'da_gconv3_wgrad')
# conv2 of the four stages at L = 224: (L of its input, C, stride)
STAGE_SHAPES = [(56, 128, 1), (56, 256, 2), (28, 256, 1), (28, 512, 2), (14, 512, 1), (14, 1024, 2), (7, 1024, 1), (1, 128, 1),
                (1, 1024, 2)]
HIP_MAX_GRID_X, HIP_MAX_GRID_YZ, HIP_MAX_BLOCK = 2 ** 31 - 1, 65535, 1024


def _gold(name):
    z = np.load(os.path.join(GOLD, name), allow_pickle=False)
    return {k: z[k] for k in z.files}


def _against(g, key, value):
    """value (float64 array) against the golden's fp64 entry -- the tensor itself, or its digest -- within 8 err32."""
    value = np.asarray(value, np.float64)
    if key in g:
        ref, got = g[key], value.reshape(g[key].shape)
    else:
        ref, got = g['dig/' + key], digest(value)
    e, tol = R.rel_l2(got, ref), 8 * float(g['err32/' + key])
    assert e <= tol, (key, e, tol)
    return e


# ---- symbols and predicates ----------------------------------------------------------------------------------------------
def test_header_and_signatures_hold_the_grouped_family():
    from deepards_amd import _lib
    assert set(SYMBOLS) <= set(_lib.header_symbols()) and set(SYMBOLS) <= set(_lib.SIGNATURES)
    assert 'conv_grouped.hip' in _lib.SOURCES
    assert sorted(_lib.header_symbols()) == sorted(_lib.SIGNATURES)
    from deepards_amd import hip_ops as H, gconv_ops
    for n in ('gconv3_fwd', 'gconv3_dgrad', 'gconv3_wgrad', 'gconv3_ok', 'gconv3_plan'):
        assert getattr(H, n) is getattr(gconv_ops, n)


def test_shape_predicate():
    from deepards_amd import hip_ops as H, _lib
    L = _lib.lib()
    for c in (32, 64, 96, 128, 192, 256, 384, 512, 768, 1024, 2048):
        for groups in (1, 16, 32, 64):
            for stride in (0, 1, 2, 3):
                want = groups == 32 and c in (128, 256, 512, 1024) and stride in (1, 2)
                assert H.gconv3_ok(c, groups, stride) == want == bool(L.da_gconv3_shape_ok(c, groups, stride)), (c, groups, stride)
    for c in (64, 96, 2048):
        assert not H.gconv3_ok(c, 32, 1)
    assert not H.gconv3_ok(128, 1, 1) and not H.gconv3_ok(128, 64, 1) and not H.gconv3_ok(128, 32, 3)


# ---- the launch-free plan ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows', [4, 1280, 5120])
def test_plan_of_every_kernel_at_the_stage_shapes(rows):
    from deepards_amd import hip_ops as H, gconv_ops as G
    for which in (G.FWD, G.DGRAD, G.WGRAD):
        for l, c, stride in STAGE_SHAPES:
            p = H.gconv3_plan(which, rows, l, c, stride)
            assert 1 <= p.grid[0] <= HIP_MAX_GRID_X and 1 <= p.grid[1] <= HIP_MAX_GRID_YZ and p.grid[2] == 1, (which, l, c, stride, p)
            assert p.block[0] * p.block[1] * p.block[2] <= HIP_MAX_BLOCK and p.block[0] % 64 == 0
            assert p.lds <= 64 * 1024                                     # the kernels keep to static LDS: no opt-in to more
            lo = G.gconv3_out_len(l, stride)
            ldst = l if which == G.DGRAD else lo
            assert p.tiles == rows * -(-ldst // p.tile_positions) and p.grid[0] == -(-p.tiles // p.tiles_per_block)
            assert p.grid[1] * 128 == c
            if which == G.WGRAD:
                # one partial of the weight's size per block column: what gconv3_wgrad allocates
                assert p.workspace == p.grid[0] * c * (c // 32) * 3 * 4 and G.gconv3_workspace_floats(p) * 4 == p.workspace
                assert p.workspace <= 32 << 20
            else:
                assert p.workspace == 0


def test_plan_refuses_what_cannot_be_launched():
    from deepards_amd import hip_ops as H, gconv_ops as G
    for which in (G.FWD, G.DGRAD, G.WGRAD):
        H.gconv3_plan(which, 2 ** 17 - 1, 128, 128, 1)                    # just below 2^31 elements
        for shape in ((2 ** 17, 128, 128, 1), (2 ** 21, 1, 1024, 1), (1, 2 ** 24, 128, 2), (0, 7, 128, 1), (4, 0, 128, 1),
                      (4, 7, 96, 1), (4, 7, 128, 3), (2 ** 31, 1, 128, 1)):
            with pytest.raises(H.HipError, match='no launch'):
                H.gconv3_plan(which, *shape)
    with pytest.raises(H.HipError):
        H.gconv3_plan(3, 4, 7, 128, 1)


# ---- model surface -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('net', sorted(NETS))
def test_model_surface(net):
    import deepards_amd.models as M
    import deepards_amd.models.seresnext as X
    from deepards_amd import train_ards_detector as T
    gname, nkeys = NETS[net]
    g = _gold(gname)
    bb = getattr(M, net)()
    assert isinstance(bb, M.SENet) and M.SENet.running_stats and bb.network_name == net
    assert bb.n_out_filters == 2048 and bb.final_length(224) == 7 and bb.dropout is None
    assert [len(getattr(bb, 'layer%d' % i)) for i in (1, 2, 3, 4)] == list(R.LAYERS[net])
    nb = int(g['nb'])
    model = M.CNNLinearNetwork(bb, nb, 0)
    sd = model.state_dict()
    assert len(bb.state_dict()) == nkeys == len([n for n in g['names'] if str(n).startswith('breath_block.')])
    assert list(sd.keys()) == [str(n) for n in g['names']] and len(sd) == nkeys + 2      # + linear_final.{weight, bias}
    assert ['x'.join(map(str, v.shape)) for v in sd.values()] == [str(s) for s in g['shapes']]
    assert [n for n, _ in model.named_parameters()] == [n for n, _, _ in R.param_spec(net, nb)]
    assert [tuple(p.shape) for _, p in model.named_parameters()] == [sh for _, sh, _ in R.param_spec(net, nb)]
    b0 = bb.layer1[0]
    assert isinstance(b0, X.SEResNeXtBottleneck) and b0.expansion == 4
    assert [n for n, _ in b0.named_children()] == ['conv1', 'bn1', 'conv2', 'bn2', 'conv3', 'bn3', 'relu', 'se_module', 'downsample']
    assert b0.conv2.groups == 32 and tuple(b0.conv2.weight.shape) == (128, 4, 3) and b0.downsample[0].stride == (1,)
    e = bb.layer2[0]                                                   # the stride sits on conv2; conv1 is stride 1
    assert e.conv1.stride == (1,) and e.conv2.stride == (2,) and e.downsample[0].stride == (2,) and e.stride == 2
    assert tuple(bb.layer4[2].conv2.weight.shape) == (1024, 32, 3)
    # registration: the pinned tables stay as they were, the second table carries the two names
    assert net not in M.base_networks and net not in M.BACKBONES and net in M.UNLISTED_BACKBONES
    assert M.backbone_class(net) is M.SENet and M.UNLISTED_BACKBONES[net][0] is getattr(M, net)
    assert isinstance(M.build_base_network(net, {'resnet_kwargs': {'initial_planes': 64}}), M.SENet)
    args = T.build_parser().parse_args(['--base-network', net, '--train-from-pickle', 'x.pkl'])
    assert args.base_network == net
    drv = object.__new__(T.network_map['cnn_linear'])              # (the constructor needs a device; get_base_network does not)
    drv.args = T.make_args(base_network=net)
    assert drv.get_base_network().network_name == net


def test_reference_checkpoint_lands_in_a_fresh_se_resnext50(tmp_path):
    from deepards_amd import checkpoint as C
    import deepards_amd.models as M
    torch.manual_seed(3)
    m = M.CNNLinearNetwork(M.se_resnext50_32x4d(), 2, 0)
    path = str(tmp_path / 'sd.pth')
    torch.save(m.state_dict(), path)
    bb = C.load_base_network(path, M.base_networks, {'base_network': 'se_resnext50_32x4d'})
    assert isinstance(bb, M.SENet) and bb.network_name == 'se_resnext50_32x4d'
    for (k, a), (_, b) in zip(bb.state_dict().items(), m.breath_block.state_dict().items()):
        assert torch.equal(a, b), k
    with pytest.raises(ValueError, match='not built'):
        C.load_base_network(path, M.base_networks, {'base_network': 'senet154'})


# ---- the oracle against the goldens ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', BLOCK_TAGS)
def test_oracle_reproduces_the_block_goldens(tag):
    g = _gold('resnext_block_%s.npz' % tag)
    rows, R_, l_out, cin, planes, stride, ds, seed = (int(v) for v in g['cfg'])
    x0, params, dout = R.block_draws(rows, R_, l_out, cin, planes, stride, bool(ds), seed)
    x = g['x']
    assert x.shape == x0.shape and x.dtype == np.float32
    assert R.rel_l2(x, x0) < 0.05                                      # the stored input is the draw, nudged
    m = R.block_margins(x, params, stride, R_)
    assert set(m) == {'h1', 'h2', 'hid', 'out'} and min(m.values()) >= R.MARGIN, (tag, m)
    r = R.block_case(x, params, stride, R_, dout)
    assert tuple(r['out'].shape) == (rows, l_out, 4 * planes)
    worst = max([_against(g, 'out', r['out'].numpy()), _against(g, 'dx', r['dx'].numpy())] +
                [_against(g, 'grad/' + n, r['grad/' + n].numpy()) for n in params])
    assert set(params) == {k[5:] for k in r if k.startswith('grad/')}
    assert worst <= 1e-9                                               # float64 against float64: far inside 8 err32
    assert max(float(g[k]) for k in g if k.startswith('err32/')) < 2e-6   # the reference's own fp32 run: the GPU tests' yardstick


@pytest.mark.parametrize('name,net', [('resnext_model_se_resnext50_32x4d_nb20.npz', 'se_resnext50_32x4d'),
                                      ('resnext_model_se_resnext101_32x4d_nb2_shifted.npz', 'se_resnext101_32x4d'),
                                      ('resnext_model_se_resnext50_32x4d_b2_grads.npz', 'se_resnext50_32x4d')])
def test_oracle_reproduces_the_model_goldens(name, net):
    g = _gold(name)
    nb, shift = int(g['nb']), float(g['bn_bias_shift'])
    assert shift == float(g['fc1_bias_shift']) == 2.0
    assert float(g['err32/logits']) <= 2.5e-5                           # the 1e-4 ceiling of the GPU bound never binds
    params = R.seeded_params(net, int(g['seed']), nb, bn_bias_shift=shift, fc1_bias_shift=shift)
    grads = 'grads' in name
    r = R.model_case(net, g['x'], g['target'], params, want_grads=grads)
    _against(g, 'logits', r['logits'].numpy())
    assert abs(float(r['loss']) - float(g['loss'])) <= 8 * float(g['err32/loss']) * abs(float(g['loss']))
    if grads:
        names = [n for n, _, _ in R.param_spec(net, nb)]
        assert len(names) == 225
        assert {'grad/' + n for n in names} == {k[4:] for k in g if k.startswith('dig/grad/')} | {k for k in g if k.startswith('grad/')}
        for n in names:
            _against(g, 'grad/' + n, r['grad/' + n].numpy())
        unpinned = [str(n) for n in g['unpinned']]
        assert len(unpinned) <= 4 and all(float(g['err32/' + n]) > 2.5e-5 for n in unpinned)
        assert all(float(g[k]) <= 2.5e-5 for k in g if k.startswith('err32/grad/') and k[6:] not in unpinned)
    else:
        assert not any('grad/' in k for k in g)


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refused_constructions():
    import deepards_amd.models as M
    import deepards_amd.models.seresnext as X
    S, B = M.SENet, X.SEResNeXtBottleneck
    B(256, 64, 32, 16)
    for args, kw, why in (((256, 64, 64, 16), {}, 'groups'), ((256, 64, 32, 16), dict(base_width=8), 'base_width'),
                          ((256, 96, 32, 16), {}, 'planes'), ((256, 1024, 32, 16), {}, 'planes'), ((256, 64, 32, 4), {}, 'reduction'),
                          ((256, 64, 1, 16), {}, 'groups')):
        with pytest.raises(NotImplementedError, match=why):
            B(*args, **kw)
    ok = dict(groups=32, reduction=16, dropout_p=None, inplanes=64, input_3x3=False, downsample_kernel_size=1, downsample_padding=0)
    S(B, [1, 1, 1, 1], **ok)
    for change in (dict(groups=1), dict(groups=64), dict(input_3x3=True), dict(dropout_p=0.2),
                   dict(downsample_kernel_size=3, downsample_padding=1), dict(inplanes=128), dict(reduction=4)):
        with pytest.raises(NotImplementedError):
            S(B, [1, 1, 1, 1], **dict(ok, **change))
    for blk in (M.SEBasicBlock, M.SEResNetBottleneck):                  # the plain blocks stay ungrouped
        with pytest.raises(NotImplementedError, match='grouped'):
            S(blk, [1, 1, 1, 1], **dict(ok, reduction=4 if blk is M.SEBasicBlock else 16))
    # conv arithmetic / storage the SE tail and the grouped kernels do not have: refused before any launch
    from deepards_amd import functional as F_
    net = M.se_resnext50_32x4d()
    prev = F_.conv_dtype()
    try:
        for name in ('bf16', 'f32x3p'):
            F_.H.CONV_DTYPE = name
            with pytest.raises(NotImplementedError, match='f32'):
                net.forward_windows(torch.zeros(2, 1, 224), 2)
    finally:
        F_.H.CONV_DTYPE = prev
    with pytest.raises(RuntimeError, match='MI355X'):
        net.forward_windows(torch.zeros(2, 1, 224), 2)                  # fp32: the usual no-CPU-path error


def test_eval_test_and_cnn_lstm_refuse_the_nets_like_every_net_with_running_statistics():
    import deepards_amd.models as M
    from deepards_amd import train_ards_detector as T
    from deepards_amd.train import HotPathTrainer
    with pytest.raises(NotImplementedError, match='running statistics'):
        HotPathTrainer(M.CNNLinearNetwork(M.se_resnext50_32x4d(), 2, 0), eval_test=True)
    for net in sorted(NETS):
        with pytest.raises(NotImplementedError, match='running statistics'):
            T.network_map['cnn_lstm'](T.make_args(network='cnn_lstm', base_network=net))
