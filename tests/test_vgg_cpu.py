"""The vgg11 / vgg13 backbones without a GPU: the float64 formulas (tests/tools/vgg_ref.py) against torch.nn and against the
goldens written from the reference's own classes, the model surface (names, order, shapes, parser, refusals)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'tools'))

from oracle.weights import digest  # noqa: E402
import vgg_ref as R  # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
F64 = 1e-10          # float64 rounding of two different summation orders (rel-l2)


def _gold(name):
    z = np.load(os.path.join(GOLD, name), allow_pickle=False)
    return {k: z[k] for k in z.files}


def _against(g, key, value, tol=F64):
    value = np.asarray(value, np.float64)
    if key in g:
        ref, got = g[key], value.reshape(g[key].shape)
    else:
        ref, got = g['dig/' + key], digest(value)
    e = R.rel_l2(got, ref)
    assert e <= tol, (key, e)


def stage_x(g, tag):
    return g[tag + '/x'] if tag + '/x' in g else _gold('vgg_stage_x700.npz')[tag + '/x']


@pytest.mark.parametrize('arch', ['vgg11', 'vgg13'])
def test_model_surface(arch):
    import deepards_amd.models as M
    g = _gold('vgg_model_%s_nb20.npz' % arch)
    fn = {'vgg11': M.vgg11_bn, 'vgg13': M.vgg13_bn}[arch]
    assert M.base_networks[arch] is fn
    bb = fn()
    assert bb.n_out_filters == 3584 and bb.network_name == arch
    assert isinstance(bb.features, torch.nn.Sequential) and isinstance(bb.avgpool, torch.nn.AdaptiveAvgPool1d)
    model = M.CNNLinearNetwork(bb, 20, 0)
    sd = model.state_dict()
    assert len(sd) == {'vgg11': 58, 'vgg13': 72}[arch]
    assert list(sd.keys()) == [str(n) for n in g['names']] == [k for k, _ in R.state_dict_spec(arch)]
    assert ['x'.join(map(str, v.shape)) for v in sd.values()] == [str(s) for s in g['shapes']]
    assert tuple(model.linear_final.weight.shape) == (2, 71680)
    assert [n for n, _ in model.named_parameters()] == [n for n, _, _ in R.vgg_param_spec(arch)]
    assert sum(q.numel() for q in bb.parameters()) == int(g['n_params'])
    # the reference's initialisation: conv bias 0, BN weight 1 / bias 0, conv weights N(0, 2 / (k C_out))
    for m in bb.features:
        if isinstance(m, torch.nn.Conv1d):
            assert m.bias is not None and float(m.bias.detach().abs().max()) == 0
            if m.in_channels >= 256:
                assert abs(float(m.weight.detach().std()) / np.sqrt(2.0 / (3 * m.out_channels)) - 1) < 0.02
        elif isinstance(m, torch.nn.BatchNorm1d):
            assert bool((m.weight == 1).all()) and bool((m.bias == 0).all()) and m.track_running_stats
    # the stage table and the reference's flat list build the same tree
    assert [type(m).__name__ for m in M.make_layers(R.CFGS[arch], batch_norm=True)] == [type(m).__name__ for m in bb.features]
    assert [(i, p) for i, _, _, p in R.stage_list(arch)] == [(list(bb.features).index(c), p) for c, _, p in bb.stages()]


def test_parser_and_refusals():
    import deepards_amd.models as M
    from deepards_amd import functional as F_
    from deepards_amd import train_ards_detector as T
    from deepards_amd.train import HotPathTrainer
    assert T.build_parser().parse_args(['--base-network', 'vgg11']).base_network == 'vgg11'
    assert T.build_parser().parse_args(['--base-network', 'vgg13']).base_network == 'vgg13'
    with pytest.raises(SystemExit):
        T.build_parser().parse_args(['--base-network', 'vgg16'])
    with pytest.raises(NotImplementedError):
        M.make_layers(R.CFGS['vgg11'], batch_norm=False)
    with pytest.raises(NotImplementedError):
        M.make_layers(['M', 64], batch_norm=True)
    bb = M.vgg11_bn()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        bb(torch.zeros(4, 1, 224))
    with pytest.raises(TypeError):
        bb.forward_windows(torch.zeros(4, 1, 224), 4, pooled=False)
    with pytest.raises(NotImplementedError, match='running statistics'):
        HotPathTrainer(M.CNNLinearNetwork(bb, 20, 0), eval_test=True)
    with pytest.raises(NotImplementedError, match='running statistics'):
        T.network_map['cnn_lstm'](T.make_args(base_network='vgg11', network='cnn_lstm', cuda=False, cuda_no_dp=True))
    prev = (F_.conv_dtype(), F_.storage_dtype())
    try:
        for name in ('bf16', 'f32x3p'):
            F_.set_conv_dtype(name)
            with pytest.raises(NotImplementedError, match='f32'):
                bb(torch.zeros(4, 1, 224))
    finally:
        F_.set_conv_dtype(prev[0])
        F_.set_storage_dtype(prev[1])


def test_stage_formula_is_torch_nn():
    """vgg_ref.stage_case (conv with bias, BatchNorm per window, ReLU, MaxPool1d(2, 2), running statistics) against torch.nn
    modules fed window by window, float64; an odd length drops its last position."""
    for rows, R_, lin, cin, c, pool in ((4, 2, 7, 8, 16, True), (6, 3, 6, 4, 8, False), (4, 2, 2, 4, 8, True), (6, 2, 9, 1, 8, True)):
        rng = np.random.default_rng([rows, lin, c])
        p = {k: v.astype(np.float64) for k, v in R.stage_params(cin, c, 5).items()}
        x, dout = rng.standard_normal((rows, lin, cin)), rng.standard_normal((rows, lin // 2 if pool else lin, c))
        r = R.stage_case(x, p, R_, pool, dout)
        conv, bn = torch.nn.Conv1d(cin, c, 3, padding=1).double(), torch.nn.BatchNorm1d(c).double()
        mods = [conv, bn, torch.nn.ReLU()] + ([torch.nn.MaxPool1d(2, 2)] if pool else [])
        with torch.no_grad():
            conv.weight.copy_(torch.from_numpy(p['w']))
            conv.bias.copy_(torch.from_numpy(p['b']))
            bn.weight.copy_(torch.from_numpy(p['gamma']))
            bn.bias.copy_(torch.from_numpy(p['beta']))
        seq = torch.nn.Sequential(*mods).train()
        xt = torch.from_numpy(x).permute(0, 2, 1).contiguous().requires_grad_(True)
        out = torch.cat([seq(xt[w * R_:(w + 1) * R_]) for w in range(rows // R_)], 0)
        out.backward(torch.from_numpy(dout).permute(0, 2, 1))
        ref = dict(out=out.permute(0, 2, 1), dx=xt.grad.permute(0, 2, 1), dw=conv.weight.grad, db=conv.bias.grad, dgamma=bn.weight.grad,
                   dbeta=bn.bias.grad, running_mean=bn.running_mean, running_var=bn.running_var)
        for k, v in ref.items():
            assert R.rel_l2(r[k].numpy(), v.detach().numpy()) <= 1e-12, (lin, k)
        assert float(r['db'].abs().max()) < 1e-12 and float(r['running_mean'].abs().max()) > 0.01


def test_adaptive_pool_formula_is_torch_nn():
    for rows, lin, c, lout in ((3, 7, 8, 7), (3, 16, 8, 7), (2, 3, 4, 7), (2, 8, 4, 7), (2, 14, 4, 7), (2, 5, 4, 3)):
        rng = np.random.default_rng([rows, lin, c])
        x, dfeat = rng.standard_normal((rows, lin, c)), rng.standard_normal((rows, c * lout))
        r = R.adaptive_pool_case(x, lout, dfeat)
        xt = torch.from_numpy(x).permute(0, 2, 1).contiguous().requires_grad_(True)
        feat = torch.nn.AdaptiveAvgPool1d(lout)(xt).reshape(rows, -1)
        feat.backward(torch.from_numpy(dfeat))
        assert R.rel_l2(r['feat'].numpy(), feat.detach().numpy()) <= 1e-14
        assert R.rel_l2(r['dx'].numpy(), xt.grad.permute(0, 2, 1).numpy()) <= 1e-14


def test_oracle_reproduces_the_stage_goldens():
    """The goldens hold the REFERENCE's results on these inputs; what the GPU tests compare against element by element is
    vgg_ref's float64 evaluation -- shown here to be the same thing.  Margins of every ReLU and pool decision: >= 1e-3."""
    g = _gold('vgg_stage_cases.npz')
    shapes = set()
    for tag in [str(t) for t in g['stages']]:
        rows, R_, lin, cin, c, pool, seed = (int(v) for v in g[tag + '/cfg'])
        shapes.add((rows, R_, lin, cin, c))
        x = stage_x(g, tag)
        p, dout = R.stage_params(cin, c, seed), R.stage_dout(rows, lin, c, pool, seed)
        assert float(np.abs(p['b']).min()) > 0 and float(np.abs(p['b']).max()) > 0.4          # a conv bias that matters
        r = R.stage_case(x, p, R_, pool, dout)
        mz, mg = R.decision_margins(r['z'], bool(pool))
        assert mz >= R.MARGIN and mg >= R.MARGIN, (tag, mz, mg)
        for k in ('out', 'dx', 'dw', 'db', 'dgamma', 'dbeta', 'running_mean', 'running_var'):
            _against(g, tag + '/' + k, r[k].numpy())
        assert float(np.abs(g[tag + '/db']).max()) < 1e-12
    assert shapes == {(4, 2, 2, 64, 64), (6, 3, 3, 64, 128), (4, 2, 7, 256, 256), (6, 3, 15, 128, 256), (4, 2, 14, 512, 512),
                      (4, 2, 700, 64, 128), (8, 4, 224, 1, 64), (6, 3, 30, 1, 64)}


@pytest.mark.parametrize('name', ['vgg_model_vgg11_nb1.npz', 'vgg_model_vgg11_nb4.npz', 'vgg_model_vgg11_nb20.npz', 'vgg_model_vgg13_nb20.npz'])
def test_oracle_reproduces_the_model_goldens(name):
    g = _gold(name)
    arch, nb = name.split('_')[2], int(name.split('nb')[1].split('.')[0])
    params = R.seeded_vgg_params(arch, int(g['seed']), nb, bn_bias_shift=float(g['bn_bias_shift']))
    logits, loss = R.model_forward(g['x'], g['target'], params, arch)
    _against(g, 'logits', logits.numpy())
    assert abs(float(loss) - float(g['loss'])) <= 1e-11
    if nb in (1, 4):                                     # the decision margins the generator searched a seed for
        # nb1 (200 704 decisions): the smallest |pre-activation| and the smallest pool gap are 8 x the reference's fp32 error
        # of their tensors, as asked.  nb4 (802 816 decisions): none of the 64 seeds walked reaches that; the file records what
        # its seed has -- every decision of the reference's fp32 run is the float64 run's, at margin_ratio x the fp32 error
        assert float(g['bn_bias_shift']) == 2.0 and float(g['margin_wanted']) == 8.0
        assert int(g['decisions']) == 200704 * nb and int(g['seeds_walked']) >= int(g['seeds_agreeing']) >= 1
        assert bool(g['margin_met']) == (float(g['margin_ratio'].min()) >= 8.0) == (nb == 1)
        assert float(g['margin_ratio'].min()) > 2.5
        assert {'grad/' + n for n, _, _ in R.vgg_param_spec(arch, nb)} == \
            {k[4:] for k in g if k.startswith('dig/grad/')} | {k for k in g if k.startswith('grad/')}
    else:
        assert not any('grad/' in k for k in g)


def test_oracle_reproduces_the_seq_len_512_features():
    g = _gold('vgg_backbone_512.npz')
    params = {k: torch.from_numpy(v).double() for k, v in R.seeded_vgg_params('vgg11', int(g['seed']), 20).items()}
    feat = R.backbone_forward(torch.from_numpy(g['x']).double(), params, 'vgg11', 20)
    assert tuple(feat.shape) == (20, 3584)
    _against(g, 'feat', feat.numpy())
