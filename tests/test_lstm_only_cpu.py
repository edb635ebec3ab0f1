"""CPU tests of the lstm_only networks (deepards_amd/models/lstm_only.py, csrc/lstm_seq.hip): a stock-torch float64
restatement of both networks -- written here, length rule included -- against the goldens recorded from the reference's own
classes (tests/tools/make_golden_lstm_only.py), and the host surface: keys, constants, refusals, driver classes, header."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, 'tests', 'golden')

CASES = {'2x3x8': False, '2x20x16': False, 'packing_2x4x8': True}


def load_golden(name):
    z = dict(np.load(os.path.join(GOLD, 'lstm_only_%s.npz' % name)))
    extra = os.path.join(GOLD, 'lstm_only_%s_gradw.npz' % name)
    if os.path.exists(extra):
        z.update(np.load(extra))
    return z


def packed_lengths(rows):
    """len = index of the first exact zero + 1; a row that starts with a zero, or holds none, runs whole.  rows (N, T)."""
    t = rows.shape[1]
    lens = torch.full((rows.shape[0],), t, dtype=torch.int64)
    for n in range(rows.shape[0]):
        zero = (rows[n] == 0).nonzero()
        if zero.numel() and int(zero[0]) > 0:
            lens[n] = int(zero[0]) + 1
    return lens


def restated(params, x, r, packed, dtype=torch.float64):
    """Both networks from stock torch cells, step by step: -> logits, {parameter: gradient of sum(logits * r)}."""
    p = {k: torch.from_numpy(v).to(dtype).requires_grad_(True) for k, v in params.items()}
    xt = torch.from_numpy(x).to(dtype)
    b, nb, _, t = xt.shape
    rows = xt.reshape(b * nb, t)
    w_ih, w_hh = p['lstm_breath_block.weight_ih_l0'], p['lstm_breath_block.weight_hh_l0']
    bias = p['lstm_breath_block.bias_ih_l0'] + p['lstm_breath_block.bias_hh_l0']
    hd = w_hh.shape[1]
    lens = packed_lengths(rows) if packed else torch.full((rows.shape[0],), t, dtype=torch.int64)
    h = torch.zeros(rows.shape[0], hd, dtype=dtype)
    c = torch.zeros_like(h)
    outs = []
    for s in range(t):
        z = rows[:, s:s + 1] @ w_ih.t() + h @ w_hh.t() + bias
        i, f, g, o = z[:, :hd].sigmoid(), z[:, hd:2 * hd].sigmoid(), z[:, 2 * hd:3 * hd].tanh(), z[:, 3 * hd:].sigmoid()
        c = f * c + i * g
        h = o * c.tanh()
        outs.append(h * (s < lens).to(dtype).unsqueeze(1))        # behind a row's length: zeros, no gradient
    hs = torch.stack(outs, dim=1)                                 # (N, T, H), flattened t-major
    feat = hs.reshape(b, nb, -1) @ p['linear_breath_inst.weight'].t() + p['linear_breath_inst.bias']
    logits = feat.reshape(b, -1) @ p['linear_final.weight'].t() + p['linear_final.bias']
    (logits * torch.from_numpy(r).to(dtype)).sum().backward()
    return logits.detach().numpy(), {k: v.grad.numpy() for k, v in p.items()}, lens.numpy()


def golden_params(z):
    return {k[len('param/'):]: v for k, v in z.items() if k.startswith('param/')}


@pytest.mark.parametrize('name', sorted(CASES))
def test_restatement_reproduces_the_goldens(name):
    """Pins the semantics independently of the kernels: float64 against float64, agreement to rounding."""
    z = load_golden(name)
    logits, grads, lens = restated(golden_params(z), z['x'], z['r'], CASES[name])
    assert np.abs(logits - z['logits']).max() <= 1e-12 * max(1.0, np.abs(z['logits']).max())
    for k, g in grads.items():
        ref = z['grad/' + k]
        assert ref.dtype == np.float64 and ref.shape == g.shape
        assert np.abs(g - ref).max() <= 1e-11 * max(1e-3, np.abs(ref).max()), k
    if CASES[name]:
        assert lens.tolist() == z['lens'].tolist() == [101, 224, 2, 224, 224, 224, 151, 58]
        rows = z['x'].reshape(-1, 224)
        assert np.signbit(rows[6, 150]) and rows[6, 150] == 0 and not (rows[6, :150] == 0).any()       # the -0.0 row
        assert not (rows[4] == 0).any() and (rows[5] == 0).all()


def test_length_rule_rows():
    """The four rows the reference was measured on: zeros from 100 on, at 0, from 1 on, at 223 only."""
    rows = torch.ones(4, 224)
    rows[0, 100:] = 0
    rows[1, 0] = 0
    rows[2, 1:] = 0
    rows[3, 223] = 0
    assert packed_lengths(rows).tolist() == [101, 224, 2, 224]


def test_classes_mirror_the_reference():
    import deepards_amd.models as M
    from deepards_amd.models import lstm_only
    for cls, feat, h, nb in ((M.LSTMOnlyNetwork, 16, 16, 20), (M.LSTMOnlyWithPacking, 64, 8, 4)):
        assert cls is getattr(lstm_only, cls.__name__)
        assert cls.seq_len == 224 and cls.intermediate_features == feat
        m = cls(h, nb)
        assert [n for n, _ in m.named_children()] == ['lstm_breath_block', 'linear_breath_inst', 'linear_final']
        assert isinstance(m.lstm_breath_block, torch.nn.LSTM) and m.lstm_breath_block.batch_first
        assert m.lstm_breath_block.input_size == 1 and m.lstm_breath_block.hidden_size == h
        assert isinstance(m.linear_breath_inst, torch.nn.Linear) and isinstance(m.linear_final, torch.nn.Linear)
        shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
        assert shapes == {'lstm_breath_block.weight_ih_l0': (4 * h, 1), 'lstm_breath_block.weight_hh_l0': (4 * h, h),
                          'lstm_breath_block.bias_ih_l0': (4 * h,), 'lstm_breath_block.bias_hh_l0': (4 * h,),
                          'linear_breath_inst.weight': (feat, 224 * h), 'linear_breath_inst.bias': (feat,),
                          'linear_final.weight': (2, feat * nb), 'linear_final.bias': (2,)}
    z = load_golden('2x3x8')
    M.LSTMOnlyNetwork(8, 3).load_state_dict({k: torch.from_numpy(v) for k, v in golden_params(z).items()}, strict=True)
    assert not hasattr(M, 'DoubleLSTMNetwork')


def test_refusals():
    import deepards_amd.models as M
    for h in (4, 12, 72, 0):
        with pytest.raises(ValueError, match='lstm_hidden_units'):
            M.LSTMOnlyNetwork(h, 20)
        with pytest.raises(ValueError, match='lstm_hidden_units'):
            M.LSTMOnlyWithPacking(h, 20)
    m = M.LSTMOnlyNetwork(8, 3)
    with pytest.raises(ValueError, match='last dimension must be 224'):
        m(torch.zeros(2, 3, 1, 112), None)
    with pytest.raises(ValueError, match='ONE channel'):
        m(torch.zeros(2, 3, 2, 224), None)
    with pytest.raises(ValueError, match='breaths per window'):
        m(torch.zeros(2, 4, 1, 224), None)


def test_driver_classes():
    from deepards_amd import train_ards_detector as T
    import deepards_amd.models as M
    assert set(T.network_map) == {'cnn_lstm', 'cnn_linear', 'cnn_double_linear', 'cnn_single_breath_linear',
                                  'cnn_linear_compr_to_rf', 'cnn_linear_to_mean'}
    for cls, net in ((T.LSTMOnlyModel, M.LSTMOnlyNetwork), (T.LSTMOnlyWithPackingModel, M.LSTMOnlyWithPacking)):
        assert cls not in T.network_map.values()
        assert cls.clip_odd_batches is True and cls.per_breath_outputs is False and cls.eval_in_test_epoch is False
        assert issubclass(cls, T.BaseTraining) and issubclass(cls, T.PatientClassifierMixin)
        for name in ('calc_loss', '_process_test_batch_results', 'get_network', 'get_model', 'train_and_test'):
            assert callable(getattr(cls, name)), name
        drv = object.__new__(cls)                           # (the constructor needs a device; get_network does not)
        drv.args = T.make_args(time_series_hidden_units=8, n_sub_batches=5, base_network='no_such_network')
        m = drv.get_network(None)                           # ignores the base network
        assert type(m) is net and m.linear_final.in_features == net.intermediate_features * 5
        with pytest.raises(RuntimeError, match='no base network'):
            drv.get_base_network()
        for flag, val in (('load_base_network', 'some.pth'), ('freeze_base_network', True)):
            with pytest.raises(ValueError, match=flag.replace('_', '-')):
                cls(T.make_args(cuda=True, **{flag: val}))
    assert not hasattr(T, 'DoubleLSTMModel')


def test_header_and_bindings():
    from deepards_amd import _lib
    names = ['da_lstm_seq_block_seqs', 'da_lstm_seq_fwd', 'da_lstm_seq_bwd_workspace', 'da_lstm_seq_bwd', 'da_lstm_seq_proj_fwd',
             'da_lstm_seq_proj_bwd_workspace', 'da_lstm_seq_proj_bwd']
    assert 'lstm_seq.hip' in _lib.SOURCES
    assert set(_lib.header_symbols()) == set(_lib.SIGNATURES)
    for n in names:
        assert n in _lib.SIGNATURES and n in _lib.header_symbols(), n
