"""CPU tests of the nested networks (deepards_amd/models/nested.py, csrc/seq_wide.hip's host side): the stock-torch
restatement tests/tools/nested_ref.py is pinned to the real reference through the goldens of tests/tools/make_golden_nested.py,
the model classes keep the reference's state_dict, the ABI carries the new symbols and every refusal names its reason."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from tools import nested_ref as NR                                       # noqa: E402
from tools.nested_ref import load_golden, W, NB                          # noqa: E402

KINDS = ('rnn', 'lstm')
_GOLD = {}


def golden(kind):
    """The merged golden record of ``kind``, read once and shared (never written to)."""
    if kind not in _GOLD:
        _GOLD[kind] = load_golden(kind)
    return _GOLD[kind]


def golden_params(z):
    return {str(k): z['param/' + str(k)] for k in z['keys']}


def head_weights(z, kind):
    return [z['param/%s.%s' % (kind, n)] for n in NR.PARAMS]


def build(kind):
    import deepards_amd.models as M
    cls = M.CNNToNestedLSTMNetwork if kind == 'lstm' else M.CNNToNestedRNNNetwork
    return cls(M.densenet18(drop_rate=0), NB, True)


# ---- the restatement is the reference ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
def test_restatement_reproduces_the_reference_head(kind):
    """From the golden's own breath-block features: logits, the medians' breaths and the six head gradients of the float64
    reference run, to float64 rounding (1e-12 relative to each tensor's largest magnitude)."""
    z = golden(kind)
    out = NR.head(kind, z['feat'], head_weights(z, kind), z['param/linear_final.weight'], z['param/linear_final.bias'], z['r'])
    assert out['logits'].shape == (1, W, 2)
    assert np.array_equal(out['idx'], z['idx'])
    pairs = [('logits', out['logits'], z['logits'])]
    pairs += [(n, out['grad/' + n], z['grad/%s.%s' % (kind, n)]) for n in NR.PARAMS]
    pairs += [(n, out['grad/' + n], z['grad/' + n]) for n in ('linear_final.weight', 'linear_final.bias')]
    for name, got, want in pairs:
        err, mag = np.abs(got - want).max(), np.abs(want).max()
        print('%s %-22s err %.3e  max |ref| %.3e' % (kind, name, err, mag))
        assert err <= 1e-12 * mag, name


def test_goldens_select_the_same_breaths_in_both_precisions():
    for kind in KINDS:
        z = golden(kind)
        live = np.take_along_axis(z['feat'], z['idx'][:, None, :].astype(np.int64), 1)[:, 0, :] != 0
        assert live.any() and (z['idx'] == z['idx32'])[live].all()
        assert not any(str(k).startswith('grad/window_linear') for k in z)


# ---- model classes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
def test_state_dict_matches_the_reference(kind):
    z = golden(kind)
    m = build(kind)
    assert list(m.state_dict().keys()) == [str(k) for k in z['keys']]
    assert [n for n, _ in m.named_children()] == ['breath_block', 'window_linear', kind, 'linear_final']
    assert m.is_cuda is True
    m.load_state_dict({k: torch.from_numpy(v) for k, v in golden_params(z).items()}, strict=True)
    assert torch.equal(m.window_linear.weight.detach(), torch.from_numpy(z['param/window_linear.weight']))
    assert tuple(m.window_linear.weight.shape) == (128, 128 * NB)


def test_abi_carries_the_new_symbols():
    from deepards_amd import _lib
    names = {'da_seqw_shape_ok', 'da_seqw_rnn_fwd', 'da_seqw_rnn_bwd', 'da_seqw_lstm_fwd', 'da_seqw_lstm_bwd'}
    assert names <= set(_lib.header_symbols()) and names <= set(_lib.SIGNATURES)
    assert 'seq_wide.hip' in _lib.SOURCES and os.path.exists(os.path.join(_lib.CSRC, 'seq_wide.hip'))


def test_shape_ok_answers_without_a_launch():
    from deepards_amd import _lib, seq_wide_ops as SW
    lib = _lib.lib()
    for kind in (0, 1):
        assert lib.da_seqw_shape_ok(kind, 128, 1) == 1 and lib.da_seqw_shape_ok(kind, 128, 4096) == 1
        assert lib.da_seqw_shape_ok(kind, 128, 0) == 0
        assert lib.da_seqw_shape_ok(kind, 64, 1) == 0 and lib.da_seqw_shape_ok(kind, 130, 1) == 0
    assert lib.da_seqw_shape_ok(2, 128, 1) == 0
    assert SW.shape_ok('lstm', 128, 1) and not SW.shape_ok('rnn', 64, 1)


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_reasons():
    import deepards_amd.models as M
    from deepards_amd import functional as F_
    from deepards_amd.train import HotPathTrainer
    m = build('rnn')
    x = torch.zeros(1, 2, NB, 1, 224)
    with pytest.raises(Exception, match='patient batch sizes of 1'):
        m(torch.zeros(2, 2, NB, 1, 224), None)
    with pytest.raises(NotImplementedError, match='metadata'):
        m(x, torch.zeros(1, 3))
    with pytest.raises(NotImplementedError, match='GPU only'):
        m(x, torch.full((1, 3), float('nan')))
    with pytest.raises(NotImplementedError, match='GPU only'):
        m(x[0], None)
    with pytest.raises(Exception, match='sequence length of 224'):
        m(torch.zeros(1, 2, NB, 1, 200), None)
    for cls in (M.CNNToNestedRNNNetwork, M.CNNToNestedLSTMNetwork):
        with pytest.raises(NotImplementedError, match='n_out_filters = 512.*densenet18'):
            cls(M.resnet18(), NB, True)
        with pytest.raises(TypeError, match='Backbone'):
            cls(torch.nn.Linear(2, 2), NB, True)
    with pytest.raises(NotImplementedError, match='long-sequence kernel; the block kernels stop at T = 64'):
        M.CNNToNestedTransformerNetwork(M.densenet18(), NB, True, 2)
    for dtype in ('bf16', 'f32x3p'):
        F_.set_conv_dtype(dtype)
        try:
            with pytest.raises(NotImplementedError, match="conv arithmetic 'f32' and float storage only"):
                m(x, None)
        finally:
            F_.set_conv_dtype('f32')
    for loss in ('vacillating', 'confidence'):
        with pytest.raises(ValueError, match='BCEWithLogitsLoss only'):
            HotPathTrainer(m, loss=loss)
    with pytest.raises(ValueError, match='not built, not run'):
        HotPathTrainer(m, world_size=2)
    HotPathTrainer(m, loss_calc='last_breath', use_graph=False)


# ---- whole-patient data -----------------------------------------------------------------------------------------------------------
SLOTS = [0, 1, 2, 2, 3, 3, 4, 5, 5, 6, 7, 8, 8, 8, 9, 9, 9, 9, 10, 11]


def test_patient_store_groups_the_fixture_in_dataset_order():
    from deepards_amd import ingest
    from deepards_amd.nested import PatientSequenceStore, group_by_patient
    ds = ingest.load_dataset(os.path.join(ROOT, 'tests', 'golden', 'test_dataset.npz'))
    assert ds.patient_slot.tolist() == SLOTS
    ps = PatientSequenceStore.from_windows(ds, device='cpu')
    assert len(ps) == 12 and [ps.windows(p) for p in range(12)] == [1, 1, 2, 2, 1, 2, 1, 1, 3, 4, 1, 1]
    assert [ps.indices(p).tolist() for p in (2, 8, 9)] == [[2, 3], [11, 12, 13], [14, 15, 16, 17]]
    assert ps.hours(9).shape == (4, 20) and np.array_equal(ps.hours(9), ds.hours[14:18], equal_nan=True)    # every window's own
    assert [g.tolist() for g in group_by_patient([7, 3, 7, 3, 5])] == [[0, 2], [1, 3], [4]]                     # interleaved patients
    ps.select([9, 2])
    assert len(ps) == 2 and [ps.windows(p) for p in range(2)] == [2, 4]
    with pytest.raises(NotImplementedError, match='oversampling with whole patient super batch'):
        PatientSequenceStore.from_windows(ds, device='cpu', oversample_minority=True)
    ds.dataset_type = 'unpadded_centered_with_bm'
    with pytest.raises(NotImplementedError, match='with_bm'):
        PatientSequenceStore.from_windows(ds, device='cpu')
    ds.dataset_type = 'unpadded_centered_sequences'
    ds.windows = np.concatenate([ds.windows, ds.windows], axis=2)
    with pytest.raises(NotImplementedError, match='one input channel'):
        PatientSequenceStore.from_windows(ds, device='cpu')


def _whole_patient_pickle(protocol):
    """A pickle as the reference writes it WITH whole_patient_super_batch=True: class path deepards.dataset.ARDSRawDataset,
    one [patient, (W, NB, 1, L), target, hours of the last window] per patient, W varying."""
    import pickle
    import types
    mod, pkg = types.ModuleType('deepards.dataset'), types.ModuleType('deepards')

    class ARDSRawDataset(object):
        pass
    ARDSRawDataset.__module__, ARDSRawDataset.__qualname__ = 'deepards.dataset', 'ARDSRawDataset'
    mod.ARDSRawDataset = ARDSRawDataset
    rng = np.random.RandomState(11)
    seqs = []
    for i, w in enumerate((3, 1, 4)):
        seqs.append(['%04dRPI%02d' % (i, i), rng.randn(w, 5, 1, 32), np.array([0., 1.]) if i % 2 else np.array([1., 0.]),
                     [float(i) + 0.25 * k for k in range(5)]])
    d = ARDSRawDataset()
    d.all_sequences, d.whole_patient_super_batch = seqs, True
    d.n_sub_batches, d.dataset_type, d.train, d.total_kfolds = 5, 'unpadded_centered_sequences', True, None
    d.scaling_factors = {None: (np.full((5, 1, 32), 0.5), np.full((5, 1, 32), 2.0))}
    saved = {k: sys.modules.get(k) for k in ('deepards', 'deepards.dataset')}
    sys.modules['deepards'], sys.modules['deepards.dataset'] = pkg, mod
    try:
        return pickle.dumps(d, protocol=protocol), seqs
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


@pytest.mark.parametrize('protocol', [2, 4])
def test_whole_patient_pickle_round_trips_without_unpickling(protocol, tmp_path):
    from deepards_amd import ingest
    from deepards_amd.nested import PatientSequenceStore
    blob, seqs = _whole_patient_pickle(protocol)
    assert 'deepards' not in sys.modules
    path = tmp_path / 'whole.pkl'
    path.write_bytes(blob)
    ds = ingest.load_dataset(str(path))
    assert ds.whole_patient and ds.windows.shape == (8, 5, 1, 32) and ds.patient_slot.tolist() == [0, 0, 0, 1, 2, 2, 2, 2]
    assert np.array_equal(ds.windows, np.concatenate([s[1] for s in seqs]))
    assert np.array_equal(ds.targets, np.repeat(np.stack([s[2] for s in seqs]), [3, 1, 4], axis=0).astype(np.float32))
    last = [2, 3, 7]                                                    # the reference kept the last window's hours only
    assert np.allclose(ds.hours[last], np.array([s[3] for s in seqs]))
    assert np.isnan(np.delete(ds.hours, last, axis=0)).all()
    assert {k: (float(m[0]), float(s[0])) for k, (m, s) in ds.scaling_factors.items()} == {None: (0.5, 2.0)}
    ps = PatientSequenceStore.from_windows(ds, device='cpu')
    assert [ps.windows(p) for p in range(len(ps))] == [3, 1, 4]
    back = ingest.load_dataset(ds.save_npz(str(tmp_path / 'whole.npz')))
    assert np.array_equal(back.windows, ds.windows) and back.patient_slot.tolist() == ds.patient_slot.tolist()


def test_nested_network_map_has_the_two_names_and_network_map_is_unchanged():
    from deepards_amd import train_ards_detector as T, nested
    assert T.nested_network_map == {'cnn_to_nested_rnn': T.CNNToNestedRNNModel, 'cnn_to_nested_lstm': T.CNNToNestedLSTMModel}
    assert not any('nested' in k for k in T.network_map)
    assert tuple(nested.NESTED_NETWORKS) == tuple(T.nested_network_map)
    assert issubclass(T.CNNToNestedLSTMModel, T.NestedMixin) and issubclass(T.CNNToNestedRNNModel, T.BaseTraining)


def test_driver_refusals_name_their_reasons():
    """Raised before anything touches the device; the batch size is forced to 1 first, as the reference's constructors do."""
    from deepards_amd import train_ards_detector as T, nested
    data = os.path.join(ROOT, 'tests', 'golden', 'test_dataset.npz')
    for loss in ('vacillating', 'confidence'):
        args = T.make_args(train_from_pickle=data, loss_func=loss, batch_size=16, cuda=False, cuda_no_dp=True)
        with pytest.raises(ValueError, match='BCEWithLogitsLoss only'):
            T.CNNToNestedLSTMModel(args)
        assert args.batch_size == 1
    with pytest.raises(NotImplementedError, match='oversampling with whole patient super batch'):
        T.CNNToNestedRNNModel(T.make_args(train_from_pickle=data, oversample_minority=True, cuda=False, cuda_no_dp=True))
    with pytest.raises(NotImplementedError, match='not built, not run'):
        T.CNNToNestedRNNModel(T.make_args(train_from_pickle=data, folds_in_flight=2, cuda=False, cuda_no_dp=True))
    with pytest.raises(SystemExit, match='long-sequence kernel; the block kernels stop at T = 64'):
        nested.main(['-n', 'cnn_to_nested_transformer', '-p', data, '--cuda-no-dp'])
    with pytest.raises(SystemExit):
        nested.main(['-n', 'cnn_linear', '-p', data, '--cuda-no-dp'])


def test_the_cap_on_w_names_the_patient_and_w():
    from deepards_amd.models.nested import check_windows
    check_windows(14979, 20)
    with pytest.raises(ValueError, match=r'patient slot 7 has W = 14980 windows .* the cap is W < 14980'):
        check_windows(14980, 20, 'patient slot 7')


def test_trainer_runs_the_nested_networks_eagerly_by_default():
    import deepards_amd.models as M
    from deepards_amd.train import HotPathTrainer
    assert HotPathTrainer(build('lstm')).use_graph is False and HotPathTrainer(build('rnn'), use_graph=True).use_graph is True
    assert HotPathTrainer(M.CNNLinearToMean(M.densenet18())).use_graph is True
