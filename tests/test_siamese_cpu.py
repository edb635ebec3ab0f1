"""Host-side tests of the siamese pretraining stage (no GPU): the C ABI's declarations, the model surface, the float64 oracle of
the GPU tests against stock torch autograd, the triplet draw's rule, the store's host logic, checkpoints and the command line."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import siamese_ref as R                                                             # noqa: E402
from deepards_amd import _lib, models as M                                          # noqa: E402
from deepards_amd import train_ards_detector as T                                   # noqa: E402
from deepards_amd.siamese import SiameseTileStore, SiameseTrainer, build_parser     # noqa: E402

NEW_SYMBOLS = ('da_siamese_draw', 'da_siamese_head_rows_per_block', 'da_siamese_head_fwd', 'da_siamese_head_bwd_workspace',
               'da_siamese_head_bwd')


def test_header_declares_and_binds_the_new_symbols():
    declared = set(_lib.header_symbols())
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES
    assert set(_lib.SIGNATURES) == declared
    assert 'siamese.hip' in _lib.SOURCES and os.path.exists(os.path.join(_lib.CSRC, 'siamese.hip'))


# ---- the model surface -------------------------------------------------------------------------------------------------------
def _block_keys(d, h):
    keys = []
    for i in (0, 1):
        p = 'transformer.blocks.%d.' % i
        keys += [(p + 'attention.q_linear.weight', (h, d)), (p + 'attention.q_linear.bias', (h,)),
                 (p + 'attention.k_linear.weight', (h, d)), (p + 'attention.k_linear.bias', (h,)),
                 (p + 'attention.v_linear.weight', (h, d)), (p + 'attention.v_linear.bias', (h,)),
                 (p + 'attention.joint_linear.weight', (d, h)), (p + 'attention.joint_linear.bias', (d,)),
                 (p + 'attention_norm.weight', (d,)), (p + 'attention_norm.bias', (d,)),
                 (p + 'ff.0.weight', (h, d)), (p + 'ff.0.bias', (h,)), (p + 'ff.2.weight', (d, h)), (p + 'ff.2.bias', (d,)),
                 (p + 'ff_norm.weight', (d,)), (p + 'ff_norm.bias', (d,))]
    return keys


@pytest.mark.parametrize('base,d', [('resnet18', 512), ('densenet18', 128)])
def test_constructors_children_attributes_and_state_dict_keys(base, d):
    nb, h = 20, 16
    head = lambda width: [('linear_intermediate.weight', (2, width)), ('linear_intermediate.bias', (2,)),
                          ('linear_final.weight', (2, 2 * nb)), ('linear_final.bias', (2,))]
    lstm = [('lstm.weight_ih_l0', (4 * h, d)), ('lstm.weight_hh_l0', (4 * h, h)), ('lstm.bias_ih_l0', (4 * h,)),
            ('lstm.bias_hh_l0', (4 * h,))]
    cases = [(M.SiameseCNNLinearNetwork, (nb,), ['breath_block', 'linear_intermediate', 'linear_final'], head(d)),
             (M.SiameseCNNLSTMNetwork, (h, nb), ['breath_block', 'lstm', 'linear_intermediate', 'linear_final'], lstm + head(h)),
             (M.SiameseCNNTransformerNetwork, (32, nb), ['breath_block', 'transformer', 'linear_intermediate', 'linear_final'],
              _block_keys(d, 32) + head(d))]
    for cls, extra, children, tail in cases:
        bb = M.base_networks[base]()
        model = cls(bb, *extra)
        assert [n for n, _ in model.named_children()] == children
        assert model.seq_size == 224 and model.breath_block is bb
        want = [('breath_block.' + k, tuple(v.shape)) for k, v in bb.state_dict().items()] + tail
        assert [(k, tuple(v.shape)) for k, v in model.state_dict().items()] == want
    lstm_model = M.SiameseCNNLSTMNetwork(M.base_networks[base](), h, nb)
    assert lstm_model.time_layer_hidden_units == h and lstm_model.lstm_layers == 1 and lstm_model.lstm.batch_first
    tfm = M.SiameseCNNTransformerNetwork(M.base_networks[base](), 32, nb)
    assert tfm.time_layer_hidden_units == 32 and len(tfm.transformer.blocks) == 2
    assert not hasattr(M.SiameseCNNLinearNetwork(M.base_networks[base](), nb), 'time_layer_hidden_units')
    x = torch.zeros(3)
    assert M.Identity()(x) is x and list(M.Identity().state_dict()) == []


def test_cpu_input_wrong_length_and_refused_sizes():
    model = M.SiameseCNNLinearNetwork(M.resnet18(), 2)
    x = torch.zeros(1, 2, 1, 224)
    with pytest.raises(RuntimeError, match='MI355X only'):
        model(x, x)
    with pytest.raises(RuntimeError, match='MI355X only'):
        model.forward_triplet(torch.zeros(3, 2, 1, 224), literal=False)
    bad = torch.zeros(1, 2, 1, 223)
    for call in (lambda: model(bad, bad), lambda: model.forward_triplet(torch.zeros(4, 2, 1, 223))):
        with pytest.raises(Exception, match='input breaths must have sequence length of 224'):
            call()
    with pytest.raises(ValueError):
        model.forward_triplet(torch.zeros(5, 2, 1, 224), literal=True)            # not a multiple of 4
    for hidden in (4, 12, 72):
        with pytest.raises(NotImplementedError):
            M.SiameseCNNLSTMNetwork(M.resnet18(), hidden, 2)
    with pytest.raises(TypeError):
        SiameseTrainer(M.CNNLinearNetwork(M.resnet18(), 2, 0))
    with pytest.raises(NotImplementedError, match='one GPU'):
        SiameseTrainer(model, world_size=2)
    with pytest.raises(NotImplementedError, match='folds in flight'):
        SiameseTrainer(model, folds_in_flight=2)


# ---- the oracle of the GPU tests against stock torch ---------------------------------------------------------------------------
@pytest.mark.parametrize('shared', [False, True])
@pytest.mark.parametrize('b,nb,d', [(1, 1, 1), (2, 3, 5), (3, 2, 17)])
def test_oracle_equals_stock_torch_autograd(b, nb, d, shared):
    rng = np.random.RandomState(b * 100 + nb * 10 + d)
    rows = b * nb
    f = lambda *s: rng.randn(*s)
    fa_pos, fc_pos, fc_neg = f(rows, d), f(rows, d), f(rows, d)
    fc_pos[0, 0] = fa_pos[0, 0]                                                      # one exactly equal element: sign(0) = 0
    W1, b1, W2, b2 = f(2, d), f(2), f(2, 2 * nb), f(2)
    t = lambda a: torch.tensor(a, dtype=torch.float64, requires_grad=True)
    ta, tcp, tcn, tW1, tb1, tW2, tb2 = t(fa_pos), t(fc_pos), t(fc_neg), t(W1), t(b1), t(W2), t(b2)
    tan = ta if shared else t(f(rows, d))
    fa_neg = tan.detach().numpy()

    def logits(a, c):
        inter = torch.nn.functional.linear(torch.abs(c - a), tW1, tb1)
        return torch.nn.functional.linear(inter.view(b, -1), tW2, tb2), inter
    zp, up = logits(ta, tcp)
    zn, un = logits(tan, tcn)
    crit = torch.nn.BCEWithLogitsLoss()
    loss = crit(zp, torch.tensor([[0.0, 1.0]], dtype=torch.float64).repeat(b, 1)) + \
        crit(zn, torch.tensor([[1.0, 0.0]], dtype=torch.float64).repeat(b, 1))
    gscale = 0.5
    (gscale * loss).backward()
    fwd = R.head_forward(fa_pos, fc_pos, fa_neg, fc_neg, W1, b1, W2, b2, b, nb)
    close = lambda x, y: np.allclose(x, y, rtol=1e-12, atol=1e-13)
    assert close(fwd['u'], torch.stack([up, un]).detach().numpy()) and close(fwd['z'], torch.stack([zp, zn]).detach().numpy())
    assert close(fwd['loss'], loss.item())
    assert (fwd['S_u'] >= np.abs(fwd['u'])).all() and (fwd['S_z'] >= np.abs(fwd['z']) - 1e-12).all() and fwd['S_loss'] >= fwd['loss']
    bwd = R.head_backward(fa_pos, fc_pos, fa_neg, fc_neg, W1, W2, fwd['u'], fwd['z'], b, nb, shared, gscale=gscale)
    assert close(bwd['dfc_pos'], tcp.grad.numpy()) and close(bwd['dfc_neg'], tcn.grad.numpy())
    assert close(bwd['dfa_pos'], ta.grad.numpy()) and bwd['dfc_pos'][0, 0] == 0.0
    if shared:
        assert bwd['dfa_neg'] is None
    else:
        assert close(bwd['dfa_neg'], tan.grad.numpy())
    for name, p in (('dW1', tW1), ('db1', tb1), ('dW2', tW2), ('db2', tb2)):
        assert close(bwd[name], p.grad.numpy()), name
        assert (bwd['S_' + name] >= np.abs(bwd[name]) - 1e-15).all()


def test_make_case_holds_the_hard_spots():
    for shared in (False, True):
        c = R.make_case(3, 2, 65, shared)
        assert (c['fa_neg'] is c['fa_pos']) == shared and c['fa_pos'].dtype == np.float32
        diff = c['fc_pos'].astype(np.float64) - c['fa_pos']
        assert (diff[0] == 0).all() and (diff[:, 0::3] == 0).all()
        tiny = np.abs(diff[-1, 1::3])
        assert (tiny > 0).all() and (tiny < 2.0 ** -126).all()                      # denormal-scale differences
        z = R.head_forward(c['fa_pos'], c['fc_pos'], c['fa_neg'], c['fc_neg'], c['W1'], c['b1'], c['W2'], c['b2'], 3, 2)['z']
        assert np.abs(z[c['big']]).min() > 40 and np.isfinite(z).all()


# ---- the draw ----------------------------------------------------------------------------------------------------------------
def test_mix32_matches_known_values():
    # common.h's mix32 evaluated by hand in Python integers
    def scalar(a, b):
        m = 0xffffffff
        h = ((a * 0x9E3779B1) & m) ^ ((b + 0x7F4A7C15) & m)
        h ^= h >> 16
        h = (h * 0x85EBCA6B) & m
        h ^= h >> 13
        h = (h * 0xC2B2AE35) & m
        return h ^ (h >> 16)
    for a, b in ((0, 0), (1234, 0), (0xffffffff, 0xffffffff), (7, 2 ** 31)):
        assert int(R.mix32(a, b)) == scalar(a, b)
    assert [int(v) for v in R.mix32(5, np.arange(3))] == [scalar(5, i) for i in range(3)]


def test_draw_rule_on_the_fixture():
    counts = [2, 3, 2, 5, 4]
    ps, pc, pat = R.patient_tables(counts)
    n = 16
    assert len(ps) == n
    anchors = np.arange(n)
    seen = np.zeros((n, n), dtype=int)
    for step in range(256):
        out = R.draw(anchors, ps, pc, 1234, step, literal=True)
        a, pos, a2, neg = out.reshape(4, n)
        assert (a == anchors).all() and (a2 == anchors).all()
        assert (pat[neg] != pat[anchors]).all()                                      # never the anchor's own patient
        last = anchors + 1 == ps + pc
        assert (pos == np.where(last, anchors - 1, anchors + 1)).all() and (pat[pos] == pat[anchors]).all()
        short = R.draw(anchors, ps, pc, 1234, step, literal=False)
        assert (short == np.concatenate([a, pos, neg])).all()
        seen[anchors, neg] += 1
    other = pat[:, None] != pat[None, :]
    assert seen[~other].sum() == 0
    assert seen[other].min() == 7 and seen[other].max() == 37                        # every other-patient window is drawn
    assert not (R.draw(anchors, ps, pc, 1235, 0, True) == R.draw(anchors, ps, pc, 1234, 0, True)).all()


# ---- the store's host logic --------------------------------------------------------------------------------------------------
def _windows(n, nb=2, seed=0):
    return np.random.RandomState(seed).randn(n, nb, 1, 224)


def test_store_drops_sorts_and_tables():
    pats = np.array(['b', 'a', 'b', 'c', 'a', 'd', 'c', 'c'])
    w = _windows(8)
    s = SiameseTileStore(w, pats, device='cpu')
    assert s.dropped == 1 and len(s) == 7                                            # 'd' has a single window
    assert s.original_index.tolist() == [0, 2, 1, 4, 3, 6, 7]                        # stable: first appearance, original order
    assert s.patients.tolist() == ['b', 'b', 'a', 'a', 'c', 'c', 'c']
    assert s.pat_start.tolist() == [0, 0, 2, 2, 4, 4, 4] and s.pat_count.tolist() == [2, 2, 2, 2, 3, 3, 3]
    assert s.pat_start.dtype == torch.int32 and s.pat_count.dtype == torch.int32
    assert np.array_equal(s.tiles.numpy(), w[s.original_index])
    from deepards_amd.tiles import scaling_factors_for_indices
    mu, std = scaling_factors_for_indices(w[s.original_index])                       # the whole (kept) set
    assert s.mu == float(mu[0]) and s.std == float(std[0]) and s.n_sub_batches == 2 and not s.padded
    test = SiameseTileStore(_windows(4, seed=1), np.array([1, 1, 2, 2]), device='cpu', scaling_from=s)
    assert test.mu == s.mu and test.std == s.std
    given = SiameseTileStore(w, pats, mu=[0.25], std=[2.0], device='cpu')
    assert given.mu == 0.25 and given.std == 2.0
    with pytest.raises(IndexError):
        s.anchors_on_device([7])


def test_store_refusals():
    w = _windows(5)
    with pytest.raises(ValueError, match='at least two patients'):
        SiameseTileStore(w, np.array(['a', 'a', 'a', 'b', 'c']), device='cpu')       # one patient left after the drop
    with pytest.raises(ValueError, match='at least two patients'):
        SiameseTileStore(w, np.array(['a', 'b', 'c', 'd', 'e']), device='cpu')
    with pytest.raises(ValueError):
        SiameseTileStore(w, np.array(['a', 'a']), device='cpu')                      # one id per window
    s = SiameseTileStore(w[:4], np.array(['a', 'a', 'b', 'b']), device='cpu')
    with pytest.raises(ValueError, match='k-fold'):
        s.enable_kfolds(np.arange(4), 2)
    from deepards_amd.ingest import IngestedDataset
    ds = IngestedDataset(w[:4], np.tile([[1.0, 0.0]], (4, 1)), ['a', 'a', 'b', 'b'], np.zeros((4, 2)), {}, 2,
                         'unpadded_centered_sequences', total_kfolds=5)
    with pytest.raises(ValueError, match='k-fold'):
        SiameseTileStore.from_dataset(ds, device='cpu')
    ds.total_kfolds = None
    ok = SiameseTileStore.from_dataset(ds, device='cpu')
    assert len(ok) == 4 and ok.pat_count.tolist() == [2, 2, 2, 2]
    ds.dataset_type = 'padded_breath_by_breath'
    assert SiameseTileStore.from_dataset(ds, device='cpu').padded


class SiameseNetworkDataset(object):
    """The attributes of the reference's class that a pickle of it carries (plain lists and ndarrays)."""


def test_from_pickle_reads_patient_array_pairs(tmp_path):
    w = _windows(6, nb=3, seed=3)
    pats = ['p1', 'p2', 'p1', 'p3', 'p2', 'p2']
    ds = SiameseNetworkDataset()
    ds.all_sequences = [[p, w[i]] for i, p in enumerate(pats)]
    ds.total_kfolds = None
    ds.n_sub_batches = 3
    ds.dataset_type = 'unpadded_centered_sequences'
    ds.scaling_factors = {None: (np.full((3, 1, 224), 0.5), np.full((3, 1, 224), 1.5))}
    path = tmp_path / 'siamese.pkl'
    with open(path, 'wb') as f:
        pickle.dump(ds, f, protocol=2)
    s = SiameseTileStore.from_pickle(str(path), device='cpu')
    assert len(s) == 5 and s.dropped == 1 and s.original_index.tolist() == [0, 2, 1, 4, 5]
    assert s.patients.tolist() == ['p1', 'p1', 'p2', 'p2', 'p2'] and s.mu == 0.5 and s.std == 1.5
    assert np.array_equal(s.tiles.numpy(), w[[0, 2, 1, 4, 5]])
    del ds.scaling_factors
    with open(path, 'wb') as f:
        pickle.dump(ds, f, protocol=2)
    derived = SiameseTileStore.from_pickle(str(path), device='cpu')
    assert abs(derived.mu - w[[0, 2, 1, 4, 5]].mean()) < 1e-12
    ds.total_kfolds = 5
    with open(path, 'wb') as f:
        pickle.dump(ds, f, protocol=2)
    with pytest.raises(ValueError, match='k-fold'):
        SiameseTileStore.from_pickle(str(path), device='cpu')


# ---- checkpoints and the command line ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cls_name,base', [('SiameseCNNLinearModel', 'resnet18'), ('SiameseCNNLSTMModel', 'densenet18'),
                                           ('SiameseCNNTransformerModel', 'densenet18')])
def test_saved_siamese_model_seeds_a_base_network(tmp_path, cls_name, base):
    from deepards_amd.checkpoint import load_base_network, checkpoint_kind
    drv = object.__new__(getattr(T, cls_name))                                     # (the constructor needs a device; _save does not)
    drv.args = T.make_args(time_series_hidden_units=16)
    drv.n_sub_batches = 4
    torch.manual_seed(3)
    model = drv.get_network(M.base_networks[base]())
    for p in model.parameters():
        p._da_grad = torch.zeros(1)                                                  # what a trainer hangs on them: not saved
    path = str(tmp_path / 'pretrained.pth')
    drv._save(model, path)
    assert checkpoint_kind(path) == 'own'
    bb = load_base_network(path, T.base_networks, {})
    assert type(bb) is type(model.breath_block) and bb.network_name == base
    want, got = model.breath_block.state_dict(), bb.state_dict()
    assert list(want) == list(got) and all(torch.equal(want[k], got[k]) for k in want)
    assert not any('_da_grad' in q.__dict__ for q in bb.parameters())


def test_command_line_and_maps():
    p = build_parser()
    a = p.parse_args(['-n', 'siamese_cnn_lstm', '--share-anchor', '-b', '8'])
    assert a.network == 'siamese_cnn_lstm' and a.share_anchor is True and a.batch_size == 8
    assert p.parse_args(['-n', 'siamese_cnn_linear']).share_anchor is None
    with pytest.raises(SystemExit):
        p.parse_args(['-n', 'cnn_linear'])
    assert sorted(T.network_map) == ['cnn_double_linear', 'cnn_linear', 'cnn_linear_compr_to_rf', 'cnn_linear_to_mean',
                                     'cnn_lstm', 'cnn_single_breath_linear']
    assert sorted(T.siamese_network_map) == ['siamese_cnn_linear', 'siamese_cnn_lstm', 'siamese_cnn_transformer']
    assert not set(T.siamese_network_map.values()) & set(T.network_map.values())
    assert 'cnn_linear' in T.build_parser().parse_args(['-n', 'cnn_linear']).network  # the driver's own parser is as it was
    from deepards_amd.siamese import main
    with pytest.raises(SystemExit, match='--load-siamese'):
        main(['--load-siamese', 'x.pth'])
    with pytest.raises(ValueError, match='k-folds'):
        T.SiameseCNNLinearModel(T.make_args(kfolds=5))
    with pytest.raises(NotImplementedError, match='folds-in-flight'):
        T.SiameseCNNLinearModel(T.make_args(folds_in_flight=2))


def test_module_help_parses():
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, '-m', 'deepards_amd.siamese', '-h'], cwd=ROOT, env=env, capture_output=True, text=True)
    assert out.returncode == 0 and 'siamese_cnn_transformer' in out.stdout and '--share-anchor' in out.stdout
    bad = subprocess.run([sys.executable, '-m', 'deepards_amd.siamese', '-n', 'cnn_linear'], cwd=ROOT, env=env,
                         capture_output=True, text=True)
    assert bad.returncode == 2 and 'invalid choice' in bad.stderr
