"""The se_resnet18 backbone without a GPU: the float64 oracle (tests/tools/se_ref.py) against the goldens written from the
reference's own classes, the model surface (names, order, refusals, parser), the ceil-mode length rule of the host code and
reference checkpoints."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'tools'))

from oracle.weights import digest  # noqa: E402
import se_ref as R  # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
F64 = 1e-11          # float64 rounding of two different summation orders through 17 convolutions (rel-l2)


def _gold(name):
    z = np.load(os.path.join(GOLD, name), allow_pickle=False)
    return {k: z[k] for k in z.files}


def _against(g, key, value, tol=F64):
    """value (float64 array) against the golden's entry: the tensor itself, or its digest."""
    value = np.asarray(value, np.float64)
    if key in g:
        ref, got = g[key], value.reshape(g[key].shape)
    else:
        ref, got = g['dig/' + key], digest(value)
    e = R.rel_l2(got, ref)
    assert e <= tol, (key, e)


@pytest.fixture(scope='module')
def blocks():
    return _gold('se_block_cases.npz')


@pytest.mark.parametrize('shifted', [True, False])
def test_oracle_reproduces_the_model_goldens(shifted):
    g = _gold('se_model_b2.npz' if shifted else 'se_model_b2_unshifted.npz')
    params = R.seeded_se_params(int(g['seed']), 20, bn_bias_shift=float(g['bn_bias_shift']), fc1_bias_shift=float(g['fc1_bias_shift']))
    r = R.model_case(g['x'], g['target'], params, want_grads=shifted)
    _against(g, 'logits', r['logits'].numpy())
    assert abs(float(r['loss']) - float(g['loss'])) <= 1e-12
    assert (float(g['bn_bias_shift']), float(g['fc1_bias_shift'])) == ((2.0, 2.0) if shifted else (0.0, 0.0))
    if shifted:
        names = [n for n, _, _ in R.se_param_spec(20)]
        assert {'grad/' + n for n in names} == {k[4:] for k in g if k.startswith('dig/grad/')} | {k for k in g if k.startswith('grad/')}
        for n in names:
            _against(g, 'grad/' + n, r['grad/' + n].numpy(), 1e-9)
    else:
        assert not any('grad/' in k for k in g)


def test_oracle_reproduces_the_block_goldens(blocks):
    g = blocks
    for tag in [str(t) for t in g['blocks']]:
        rows, R_, l_out, planes, stride, seed = (int(v) for v in g[tag + '/cfg'])
        x, params, dout = R.block_inputs(rows, R_, l_out, planes, stride, seed)
        assert np.array_equal(x, g[tag + '/x']), tag                    # the generator is deterministic
        m = R.block_margins(x, params, stride, R_)
        assert min(m.values()) >= R.MARGIN, (tag, m)
        r = R.block_case(x, params, stride, R_, dout)
        _against(g, tag + '/out', r['out'].numpy())
        _against(g, tag + '/dx', r['dx'].numpy(), 1e-10)
        for n in params:
            _against(g, tag + '/grad/' + n, r['grad/' + n].numpy(), 1e-10)


def test_oracle_reproduces_the_stem_goldens(blocks):
    g = blocks
    for tag in [str(t) for t in g['stems']]:
        rows, R_, lin, c, seed = (int(v) for v in g[tag + '/cfg'])
        x, w, gamma, beta, dout = R.stem_inputs(rows, R_, lin, c, seed)
        r = R.stem_case(x, w, gamma, beta, R_, dout)
        assert r['out'].shape[1] == R.pool_len_ceil(lin // 2)
        for k in ('out', 'dw', 'dgamma', 'dbeta'):
            _against(g, tag + '/' + k, r[k].numpy(), 1e-10)
        # the routing written out as a loop is the pool's backward: dout through it, the ReLU and the BatchNorm is dw
        a = torch.relu(R.window_bn(r['y'], R_, torch.from_numpy(gamma).double(), torch.from_numpy(beta).double()))
        assert torch.equal(R.ceil_pool(a), r['out'])
        a.requires_grad_(True)
        (da,) = torch.autograd.grad(R.ceil_pool(a), a, torch.from_numpy(dout).double())
        assert torch.equal(da, r['routed']), tag


def test_tail_closed_form_is_the_autograd_of_the_block_tail():
    """se_tail's backward (what the five kernels compute, by name) against autograd through the plain forward."""
    for shape in ((6, 3, 7, 64), (4, 2, 5, 512)):
        rows, R_, l, c = shape
        case = R.tail_case(*shape)
        h, o = R.tail_margins(case, R_)
        assert h >= R.MARGIN and o >= R.MARGIN, (shape, h, o)
        r = R.se_tail(R=R_, **case)
        t = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in case.items() if k != 'dout'}
        z = R.window_bn(t['y2'], R_, t['gamma'], t['beta'])
        cr = c // 4
        s = torch.sigmoid(torch.relu(z.mean(1) @ t['w1'].reshape(cr, c).t() + t['b1']) @ t['w2'].reshape(c, cr).t() + t['b2'])
        out = torch.relu(z * s[:, None, :] + t['res'])
        names = ('y2', 'gamma', 'beta', 'w1', 'b1', 'w2', 'b2', 'res')
        grads = torch.autograd.grad(out, [t[k] for k in names], torch.tensor(case['dout'], dtype=torch.float64))
        for k, got, ref in zip(names, (r['dy2'], r['dgamma'], r['dbeta'], r['dw1'], r['db1'], r['dw2'], r['db2'], r['g']), grads):
            assert R.rel_l2(got.numpy().reshape(ref.shape), ref.numpy()) <= 1e-12, (shape, k)


def test_model_surface():
    import deepards_amd.models as M
    from deepards_amd import train_ards_detector as T
    g = _gold('se_model_b2.npz')
    assert M.base_networks['se_resnet18'] is M.se_resnet18
    bb = M.base_networks['se_resnet18']()
    assert bb.network_name == 'se_resnet18' and bb.n_out_filters == 512 and bb.dropout is None and bb.inplanes == 512
    model = M.CNNLinearNetwork(bb, 20, 0)
    sd = model.state_dict()
    assert list(sd.keys()) == [str(n) for n in g['names']]
    assert ['x'.join(map(str, v.shape)) for v in sd.values()] == [str(s) for s in g['shapes']]
    assert [n for n, _ in model.named_parameters()] == [n for n, _, _ in R.se_param_spec(20)]
    assert [n for n, _ in bb.layer1[0].named_children()] == ['conv1', 'bn1', 'relu', 'conv2', 'se_module', 'bn2']
    assert bb.layer1[0].downsample is None and list(bb.layer2[0]._modules) == ['conv1', 'bn1', 'relu', 'conv2', 'se_module', 'bn2',
                                                                               'downsample']
    assert [n for n, _ in bb.layer0.named_children()] == ['conv1', 'bn1', 'relu1', 'pool']
    assert [n for n, _ in bb.layer1[0].se_module.named_children()] == ['avg_pool', 'fc1', 'relu', 'fc2', 'sigmoid']
    assert bb.layer0.pool.ceil_mode and bb.layer0.pool.padding == 0 and bb.layer3[1].se_module.fc1.bias is not None
    assert [n for n, _ in bb.named_children()] == ['layer0', 'layer1', 'layer2', 'layer3', 'layer4', 'avg_pool']
    for m in ('features', 'logits', 'forward', 'forward_windows'):
        assert callable(getattr(bb, m))
    # torch's default initialisation: BatchNorm 1 / 0, no init loop over the convs
    assert float(bb.layer4[1].bn2.weight.detach().min()) == 1.0 and float(bb.layer4[1].bn2.bias.detach().abs().max()) == 0.0
    # the parser and the driver's table
    assert 'se_resnet18' in T.base_networks
    args = T.build_parser().parse_args(['--base-network', 'se_resnet18', '--train-from-pickle', 'x.pkl'])
    assert args.base_network == 'se_resnet18'


def test_network_map_is_unchanged():
    from deepards_amd import train_ards_detector as T
    assert sorted(T.network_map) == ['cnn_double_linear', 'cnn_linear', 'cnn_linear_compr_to_rf', 'cnn_linear_to_mean', 'cnn_lstm',
                                     'cnn_single_breath_linear']


def test_refused_constructions():
    import deepards_amd.models as M
    S, B = M.SENet, M.SEBasicBlock
    ok = dict(groups=1, reduction=4, dropout_p=None, inplanes=64, input_3x3=False, downsample_kernel_size=1, downsample_padding=0)
    S(B, [1, 1, 1, 1], **ok)
    for change in (dict(groups=64), dict(input_3x3=True), dict(dropout_p=0.2), dict(downsample_kernel_size=3, downsample_padding=1),
                   dict(groups=32)):
        with pytest.raises(NotImplementedError):
            S(B, [2, 2, 2, 2], **dict(ok, **change))
    with pytest.raises(NotImplementedError):
        S(M.BasicBlock, [2, 2, 2, 2], **ok)                     # a non-SE block (the Bottlenecks are not built at all)
    with pytest.raises(NotImplementedError):
        S(B, [2, 2, 2, 2], 64, 4)                               # senet18's defaults: groups 64, dropout, 3x3 stem
    with pytest.raises(NotImplementedError):
        B(64, 64, 64, 4)
    # conv arithmetic / storage the SE tail does not have: refused when forward_windows is entered, before any launch
    from deepards_amd import functional as F_
    net = M.se_resnet18()
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


def test_eval_test_and_cnn_lstm_refuse_the_se_resnet_like_the_resnets():
    import deepards_amd.models as M
    from deepards_amd import train_ards_detector as T
    from deepards_amd.train import HotPathTrainer
    with pytest.raises(NotImplementedError, match='running statistics'):
        HotPathTrainer(M.CNNLinearNetwork(M.se_resnet18(), 20, 0), eval_test=True)
    with pytest.raises(NotImplementedError, match='running statistics'):
        T.network_map['cnn_lstm'](T.make_args(network='cnn_lstm', base_network='se_resnet18'))


def test_se_block_convs_keep_off_the_f43_kernels():
    """The SE block asks for F(2,3) where the shape alone would take F(4,3): forward / data gradient, weight gradient and the
    step's pack form; every other conv keeps the project's choice."""
    import deepards_amd.models as M
    from deepards_amd import hip_ops as H
    assert M.SEBasicBlock.precise_convs and not getattr(M.BasicBlock, 'precise_convs', False)
    if H.WINOGRAD_WGRAD and H.CONV_DTYPE == 'f32':
        assert H.conv_kernel_wanted(512, 512, 3, 1, 1) == H.WINO4 == H.wgrad_kernel(512, 512, 3, 1, 1, 7) == H.step_pack_form(512, 512, 3, 1, 1)
        assert H.conv_kernel_wanted(512, 512, 3, 1, 1, True) == H.WINO2 == H.conv_kernel(512, 512, 3, 1, 1, False, 7, True)
        assert H.wgrad_kernel(512, 512, 3, 1, 1, 7, precise=True) == H.WINO2 == H.step_pack_form(512, 512, 3, 1, 1, True)
        assert H.conv_kernel_wanted(256, 256, 3, 1, 1, True) == H.WINO2 == H.conv_kernel_wanted(256, 256, 3, 1, 1)
    assert H.conv_kernel_wanted(512, 256, 3, 2, 1, True) == H.DIRECT


def test_ceil_mode_length_rule_of_the_host_code():
    from deepards_amd import hip_ops as H
    from deepards_amd import functional as F_
    assert (F_.POOL_MAX, F_.POOL_AVG, F_.POOL_MAX_CEIL) == (0, 1, 2)
    pool = torch.nn.MaxPool1d(3, 2, ceil_mode=True)
    for lc in range(1, 131):
        try:
            want = pool(torch.zeros(1, 1, lc)).shape[-1]
        except RuntimeError:
            want = 0                                            # torch refuses an empty output: a one-element row has no window
        assert H.pool_out_len(lc, F_.POOL_MAX_CEIL) == want == R.pool_len_ceil(lc), lc
        assert H.pool_out_len(lc, F_.POOL_MAX) == H.pool_out_len(lc, F_.POOL_AVG) == (lc - 1) // 2 + 1
    assert H.pool_out_len(112, 2) == 56
    with pytest.raises(ValueError):
        H.pool_out_len(112, 3)


def test_reference_checkpoint_lands_in_a_fresh_se_resnet18(tmp_path):
    """A whole module pickled under the reference's class paths (deepards.models.senet.*) is read without unpickling;
    --load-base-network builds a fresh se_resnet18 for it (no keyword arguments) and loads the breath_block.* weights."""
    from se_ref_paths import as_reference_classes
    from deepards_amd import checkpoint as C
    import deepards_amd.models as M
    path = str(tmp_path / 'ref_se.pth')

    def save(M_):
        torch.manual_seed(5)
        m = M_.CNNLinearNetwork(M_.se_resnet18(), 20, 0)
        torch.save(m, path, _use_new_zipfile_serialization=False)
        return m
    m = as_reference_classes(save)
    assert M.SENet.__module__ == 'deepards_amd.models.senet'
    assert C.checkpoint_kind(path) == 'foreign'
    info = C.read_module_checkpoint(path)
    assert info['breath_block_class'] == 'deepards.models.senet.SENet' and info['network_name'] == 'se_resnet18'
    assert list(info['state_dict']) == list(m.state_dict())
    kw = dict(base_network='densenet18', resnet_kwargs=dict(initial_planes=64), densenet_kwargs=dict(with_fft=False))
    bb = C.load_base_network(path, M.base_networks, kw)
    assert isinstance(bb, M.SENet) and bb is not m.breath_block and bb.network_name == 'se_resnet18'
    for (k, a), (_, b) in zip(bb.state_dict().items(), m.breath_block.state_dict().items()):
        assert torch.equal(a, b), k
    # an own whole-module file round-trips through the restricted unpickler
    own = str(tmp_path / 'own_se.pth')
    torch.save(m, own)
    back = C.load_own_module(own)
    assert isinstance(back.breath_block, M.SENet) and isinstance(back.breath_block.layer1[0].se_module, M.SEModule)
    # the driver builds the network its name asks for, without the DenseNet keywords
    from deepards_amd import train_ards_detector as T
    cls = object.__new__(T.network_map['cnn_linear'])           # (the constructor needs a device; get_base_network does not)
    cls.args = T.make_args(base_network='se_resnet18', with_fft=True)
    assert isinstance(cls.get_base_network(), M.SENet)
    cls.args = T.make_args(base_network='resnet18', load_base_network=path)
    assert isinstance(cls.get_base_network(), M.SENet)          # the file's backbone, not --base-network
