"""Host-side tests of the breath-metadata pretraining stage (no GPU): the C ABI's declarations and its shape / workspace rules,
the float64 oracle of the GPU tests against stock torch autograd, the model surface, checkpoints, the breath-level ingest, the
store's host logic and the command line with its refusals."""
import ctypes
import os
import pickle
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'tools'))

import regress_ref as R                                                             # noqa: E402
from deepards_amd import _lib, hip_ops as H, ingest, models as M, regress_ops as RO  # noqa: E402
from deepards_amd import train_ards_detector as T                                   # noqa: E402
from deepards_amd.regressor import (BM_TARGET_TYPES, BreathMetaStore, RegressorTrainer, build_parser, epoch_index_batches,   # noqa: E402
                                    main)

NEW_SYMBOLS = ('da_regress_rows_per_block', 'da_regress_shape_ok', 'da_regress_workspace', 'da_regress_fwd', 'da_regress_bwd')
PINNED_NETWORK_MAP = ['cnn_double_linear', 'cnn_linear', 'cnn_linear_compr_to_rf', 'cnn_linear_to_mean', 'cnn_lstm',
                      'cnn_single_breath_linear']


def test_header_declares_and_binds_the_new_symbols():
    declared = set(_lib.header_symbols())
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES
    assert set(_lib.SIGNATURES) == declared
    assert 'regress.hip' in _lib.SOURCES and os.path.exists(os.path.join(_lib.CSRC, 'regress.hip'))
    for name in ('regress_rows_per_block', 'regress_shape_ok', 'regress_workspace', 'regress_fwd', 'regress_bwd',
                 'regress_head_loss'):
        assert getattr(H, name) is getattr(RO, name)


# (R, F, M, form) -- legal ones and every way to be refused
SHAPES = [(1, 32, 1, 0), (1, 32, 1, 1), (7, 256, 3, 1), (8, 288, 9, 0), (9, 3584, 16, 0), (19, 512, 9, 1), (128, 512, 9, 1),
          (5, 30, 2, 1), (1 << 24, 4, 1, 0),
          (0, 32, 1, 0), (-1, 32, 1, 1), (4, 0, 3, 0), (4, 32, 0, 1), (4, 32, 17, 0), (4, 32, 3, 2), (4, 32, 3, -1),
          ((1 << 24) + 1, 4, 1, 0), (4, (1 << 20) + 4, 1, 0), (1 << 24, 1 << 20, 1, 1)]


def test_shape_and_workspace_rules_match_their_python_twins():
    lib = _lib.lib()
    assert lib.da_regress_rows_per_block() == RO.ROWS_PER_BLOCK == RO.regress_rows_per_block()
    refused = 0
    for r, f, m, form in SHAPES:
        ok = RO.regress_shape_ok(r, f, m, form)
        assert bool(lib.da_regress_shape_ok(r, f, m, form)) == ok, (r, f, m, form)
        assert lib.da_regress_workspace(r, f, m) == RO.regress_workspace(r, f, m), (r, f, m)
        if ok:
            assert RO.regress_workspace(r, f, m) == -(-r // RO.ROWS_PER_BLOCK) * m * f * 4
        else:
            refused += 1
            # a refused shape answers before any launch: null pointers, no device touched
            assert lib.da_regress_fwd(None, max(f, 1), form, None, None, None, None, None, None, r, f, m, None) == -1
            assert lib.da_regress_bwd(None, max(f, 1), None, None, None, None, max(f, 1), form, None, None, None, 1.0, 0, r, f, m,
                                      None) == -1
    assert refused == 10
    # legal shapes with a null operand or a pitch below F are refused as well
    assert lib.da_regress_fwd(None, 32, 0, None, None, None, None, None, None, 4, 32, 3, None) == -1
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.da_regress_fwd(p, 16, 0, p, p, p, p, p, p, 1, 32, 1, None) == -1
    assert lib.da_regress_bwd(p, 32, p, p, p, p, 16, 0, p, p, p, 1.0, 0, 1, 32, 1, None) == -1


# ---- the oracle of the GPU tests against stock torch ---------------------------------------------------------------------------
@pytest.mark.parametrize('form', [0, 1])
@pytest.mark.parametrize('r,f,m', [(1, 1, 1), (3, 5, 2), (9, 33, 9), (17, 64, 16)])
def test_oracle_equals_stock_torch_autograd(r, f, m, form):
    c = R.make_case(r, f, m, form, seed=1)
    gscale = 0.25
    ref = R.run(c['x'], c['w'], c['bias'], c['target'], gscale=gscale, dtype=np.float64)
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=True)
    x, w, b = t(c['x']), t(c['w']), t(c['bias'])
    feat = torch.nn.functional.avg_pool1d(x.permute(0, 2, 1), 7).squeeze(-1) if form else x        # AvgPool1d(7) on (R, F, 7)
    out = torch.nn.functional.linear(feat, w, b)
    loss = torch.nn.MSELoss()(out, torch.tensor(c['target'], dtype=torch.float64))
    (gscale * loss).backward()
    close = lambda a, bb: R.rel_l2(a, bb) <= 1e-12
    assert close(ref['out'], out.detach().numpy()) and close(ref['loss'], loss.item()) and close(ref['feat'], feat.detach().numpy())
    assert close(ref['dx'], x.grad.numpy()) and close(ref['dW'], w.grad.numpy()) and close(ref['db'], b.grad.numpy())
    assert ref['dx'].shape == c['x'].shape and ref['out'].dtype == np.float64
    r32 = R.run(c['x'], c['w'], c['bias'], c['target'], gscale=gscale, dtype=np.float32)
    assert all(v.dtype == np.float32 for v in r32.values())
    assert R.rel_l2(r32['dW'], ref['dW']) < 1e-5 and (f < 33 or R.rel_l2(r32['dW'], ref['dW']) > 0)


def test_make_case_targets_span_the_scales_of_raw_metadata():
    c = R.make_case(64, 32, 9, 1)
    s = c['target'].std(axis=0)
    assert s[0] < 0.05 and s[-1] > 300 and (c['x'] >= 0).all() and c['x'].dtype == np.float32


# ---- the model surface -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('base,width', [('resnet18', 512), ('densenet18', 128), ('vgg11', 3584)])
def test_constructor_children_attributes_and_state_dict_keys(base, width):
    bb = M.base_networks[base]()
    model = M.CNNRegressor(bb, 9)
    assert [n for n, _ in model.named_children()] == ['breath_block', 'linear_final']
    assert model.seq_size == 224 and model.breath_block is bb and bb.n_out_filters == width
    want = [('breath_block.' + k, tuple(v.shape)) for k, v in bb.state_dict().items()] + \
        [('linear_final.weight', (9, width)), ('linear_final.bias', (9,))]
    assert [(k, tuple(v.shape)) for k, v in model.state_dict().items()] == want
    # a state_dict written under the reference's key names (they are the same names) loads strictly
    torch.manual_seed(1)
    other = M.CNNRegressor(M.base_networks[base](), 9)
    other.load_state_dict({k: v.clone() for k, v in model.state_dict().items()}, strict=True)
    assert all(torch.equal(a, b) for a, b in zip(model.state_dict().values(), other.state_dict().values()))


def test_refusals_of_the_model_and_the_trainer():
    with pytest.raises(TypeError, match='Backbone'):
        M.CNNRegressor(M.UNet(1), 3)
    with pytest.raises(TypeError, match='Backbone'):
        M.CNNRegressor(M.AutoencoderCNN(), 3)
    for m in (0, 17):
        with pytest.raises(ValueError, match=r'\[1, 16\]'):
            M.CNNRegressor(M.resnet18(), m)
    model = M.CNNRegressor(M.resnet18(), 3)
    with pytest.raises(Exception, match='input breaths must have sequence length of 224'):
        model(torch.zeros(4, 1, 223), None)
    with pytest.raises(Exception, match='input breaths must have sequence length of 224'):
        model.forward_loss(torch.zeros(4, 1, 223), torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match='MI355X only'):
        model(torch.zeros(4, 1, 224))
    with pytest.raises(TypeError):
        RegressorTrainer(M.CNNLinearNetwork(M.resnet18(), 2, 0))
    with pytest.raises(NotImplementedError, match='one GPU'):
        RegressorTrainer(model, world_size=2)
    with pytest.raises(NotImplementedError, match='folds in flight'):
        RegressorTrainer(model, folds_in_flight=2)
    with pytest.raises(ValueError, match='MSELoss'):
        RegressorTrainer(model, loss='bce')
    with pytest.raises(ValueError, match='carry_state'):
        RegressorTrainer(model, carry_state=True)
    from deepards_amd import functional as F_
    prev = F_.conv_dtype()
    try:
        F_.set_conv_dtype('f32x3p')
        with pytest.raises(NotImplementedError, match='float maps only'):
            RegressorTrainer(model)
        with pytest.raises(NotImplementedError, match='float maps only'):
            model(torch.zeros(4, 1, 224))
    finally:
        F_.set_conv_dtype(prev)
    tr = RegressorTrainer(model)
    with pytest.raises(ValueError, match=r'\(4, 3\) target'):
        tr.train_step(torch.zeros(4, 1, 224), torch.zeros(4, 2))
    with pytest.raises(ValueError, match='target'):
        tr.test_step(torch.zeros(4, 1, 224), None)


# ---- checkpoints ---------------------------------------------------------------------------------------------------------------
def _as_reference_regressor(fn):
    """Run fn() while this package's CNNRegressor and ResNet classes claim the reference's class paths."""
    import deepards_amd.models.regressor as G
    import deepards_amd.models.resnet as RN
    moved, fakes = [], {}
    for mod, refname in ((RN, 'deepards.models.resnet'), (G, 'deepards.models.torch_cnn_bm_regressor')):
        fake = fakes.setdefault(refname, types.ModuleType(refname))
        for name, obj in vars(mod).items():
            if isinstance(obj, type) and obj.__module__ == mod.__name__:
                moved.append((obj, obj.__module__))
                obj.__module__ = refname
                setattr(fake, name, obj)
    fakes['deepards'], fakes['deepards.models'] = types.ModuleType('deepards'), types.ModuleType('deepards.models')
    saved = {k: sys.modules.get(k) for k in fakes}
    sys.modules.update(fakes)
    try:
        return fn()
    finally:
        for obj, m in moved:
            obj.__module__ = m
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def test_reference_module_pickle_is_read_without_unpickling(tmp_path):
    from deepards_amd.checkpoint import checkpoint_kind, load_base_network, read_module_checkpoint
    torch.manual_seed(5)
    model = M.CNNRegressor(M.resnet18(), 7)
    path = str(tmp_path / 'ref_regressor.pth')
    _as_reference_regressor(lambda: torch.save(model, path))
    assert checkpoint_kind(path) == 'foreign'
    info = read_module_checkpoint(path)
    assert info['class_name'] == 'deepards.models.torch_cnn_bm_regressor.CNNRegressor' and info['network_name'] == 'resnet18'
    assert list(info['state_dict']) == list(model.state_dict())
    bb = load_base_network(path, T.base_networks, {})
    want, got = model.breath_block.state_dict(), bb.state_dict()
    assert list(want) == list(got) and all(torch.equal(want[k], got[k]) for k in want)
    fresh = M.CNNRegressor(M.resnet18(), 7)
    fresh.load_state_dict(info['state_dict'], strict=True)


@pytest.mark.parametrize('base', ['resnet18', 'densenet18', 'vgg11'])
def test_saved_regressor_seeds_a_base_network(tmp_path, base):
    from deepards_amd.checkpoint import checkpoint_kind, load_base_network, load_own_module
    drv = object.__new__(T.CNNRegressorModel)                                        # (the constructor needs a device; _save does not)
    drv.args = T.make_args()
    drv.n_bm_features = 9
    torch.manual_seed(3)
    model = drv.get_network(M.base_networks[base]())
    for p in model.parameters():
        p._da_grad = torch.zeros(1)
    path = str(tmp_path / 'reg.pth')
    drv._save(model, path)
    assert checkpoint_kind(path) == 'own' and isinstance(load_own_module(path), M.CNNRegressor)
    bb = load_base_network(path, T.base_networks, {})
    want, got = model.breath_block.state_dict(), bb.state_dict()
    assert type(bb) is type(model.breath_block) and list(want) == list(got) and all(torch.equal(want[k], got[k]) for k in want)
    assert not any('_da_grad' in q.__dict__ for q in bb.parameters())


def test_get_network_needs_a_dataset_type():
    drv = object.__new__(T.CNNRegressorModel)
    drv.args = T.make_args()
    with pytest.raises(Exception, match='without specifying which dataset you want to use'):
        drv.get_network(M.resnet18())


# ---- ingest and the store's host logic -------------------------------------------------------------------------------------------
def _reference_dataset_pickle(seqs, dataset_type, factors='scalar', nb=1, L=224, protocol=2):
    """A pickle with the class path deepards.dataset.ARDSRawDataset around ``seqs``."""
    mod, pkg = types.ModuleType('deepards.dataset'), types.ModuleType('deepards')

    class ARDSRawDataset(object):
        pass
    ARDSRawDataset.__module__, ARDSRawDataset.__qualname__ = 'deepards.dataset', 'ARDSRawDataset'
    mod.ARDSRawDataset = ARDSRawDataset
    d = ARDSRawDataset()
    d.all_sequences = seqs
    d.n_sub_batches, d.dataset_type, d.train, d.total_kfolds = nb, dataset_type, True, None
    if factors == 'scalar':                             # the old-pickle form
        d.scaling_factors = {None: (0.125, 2.5)}
    elif factors == 'broadcast':                        # the reference's wart on (1, L) rows: (n_sub_batches, L, L), one number
        d.scaling_factors = {None: (np.full((2, L, L), 0.125), np.full((2, L, L), 2.5))}
    elif factors == 'window':
        d.scaling_factors = {None: (np.full((nb, 1, L), 0.125), np.full((nb, 1, L), 2.5))}
    saved = {k: sys.modules.get(k) for k in ('deepards', 'deepards.dataset')}
    sys.modules['deepards'], sys.modules['deepards.dataset'] = pkg, mod
    try:
        return pickle.dumps(d, protocol=protocol)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def _breath_seqs(n, m, L=32, seed=0):
    rng = np.random.RandomState(seed)
    rows = rng.randn(n, 1, L)
    rows[:, :, L - 5:] = 0.0                                                          # the padding of a padded breath
    meta = rng.randn(n, m) * 10.0 ** np.linspace(-2, 3, m)
    pats = ['%04dRPI' % (i % 3) for i in range(n)]
    return rows, meta, pats, [[p, rows[i], meta[i], [np.nan]] for i, p in enumerate(pats)]


@pytest.mark.parametrize('factors', ['scalar', 'broadcast', None])
def test_breath_level_pickle_ingest_store_and_npz_round_trip(tmp_path, factors):
    rows, meta, pats, seqs = _breath_seqs(11, 9)
    dt = 'padded_breath_by_breath_with_full_bm_target'
    path = tmp_path / 'bm.pkl'
    path.write_bytes(_reference_dataset_pickle(seqs, dt, factors, L=32))
    ds = ingest.load_dataset(str(path))
    assert ds.breath_level and ds.windows.shape == (11, 1, 32) and ds.targets.shape == (11, 9) and ds.targets.dtype == np.float64
    assert np.array_equal(ds.windows, rows) and np.array_equal(ds.targets, meta)
    assert np.isnan(ds.hours).all() and ds.hours.shape == (11, 1) and ds.dataset_type == dt
    assert ds.patients.tolist() == pats and ds.patient_slot.tolist() == [i % 3 for i in range(11)]
    if factors:
        mu, std = ds.scaling_factors[None]
        assert mu.tolist() == [0.125] and std.tolist() == [2.5]
    else:
        assert ds.scaling_factors == {}
    with pytest.raises(ValueError, match='BreathMetaStore'):
        ds.to_store('cpu')
    store = BreathMetaStore.from_dataset(ds, device='cpu')
    assert len(store) == 11 and store.n_targets == 9 and store.padded and store.seq_len == 32
    assert store.tiles.shape == (11, 1, 1, 32) and store.targets.dtype == torch.float32
    assert np.array_equal(store.targets.numpy(), meta.astype(np.float32))
    if factors:
        assert store.mu == 0.125 and store.std == 2.5
    else:                                                                             # derived: the plain mean / std over the samples
        assert abs(store.mu - rows.mean()) < 1e-15 and abs(store.std - rows.std()) < 1e-15
    test = BreathMetaStore.from_dataset(ds, device='cpu', scaling_from=store)
    assert test.mu == store.mu and test.std == store.std
    with pytest.raises(ValueError, match='k-folds'):
        store.enable_kfolds(np.arange(11), 5)
    npz = str(tmp_path / 'bm.npz')
    ds.save_npz(npz)
    back = ingest.load_dataset(npz)
    assert back.breath_level and np.array_equal(back.windows, ds.windows) and np.array_equal(back.targets, ds.targets)
    assert back.targets.dtype == np.float64 and back.dataset_type == dt and np.isnan(back.hours).all()
    assert np.array_equal(back.patient_slot, ds.patient_slot) and set(back.scaling_factors) == set(ds.scaling_factors)
    for k in ds.scaling_factors:
        assert all(np.array_equal(a, b) for a, b in zip(back.scaling_factors[k], ds.scaling_factors[k]))
    again = BreathMetaStore.from_pickle(npz, device='cpu')
    assert again.mu == store.mu and again.std == store.std and torch.equal(again.targets, store.targets)


def test_non_finite_target_is_refused_with_its_row(tmp_path):
    rows, meta, pats, seqs = _breath_seqs(6, 3)
    seqs[4][2] = np.array([1.0, np.nan, 2.0])
    path = tmp_path / 'bad.pkl'
    path.write_bytes(_reference_dataset_pickle(seqs, 'padded_breath_by_breath_with_limited_bm_target', L=32))
    with pytest.raises(ValueError, match='sequence 4 has a non-finite target'):
        ingest.load_dataset(str(path))
    seqs[4][2] = np.array([1.0, np.inf, 2.0])
    path.write_bytes(_reference_dataset_pickle(seqs, 'padded_breath_by_breath_with_limited_bm_target', L=32))
    with pytest.raises(ValueError, match='sequence 4 has a non-finite target'):
        ingest.load_dataset(str(path))
    with pytest.raises(ValueError, match='breath 2 has a non-finite target'):
        BreathMetaStore(rows, np.where(np.arange(6)[:, None] == 2, np.nan, meta), device='cpu')


def test_from_windows_flattens_a_metadata_window_dataset(tmp_path):
    rng = np.random.RandomState(2)
    n, nb, L = 4, 3, 32
    w, meta = rng.randn(n, nb, 1, L), rng.randn(n, nb, 9)
    seqs = [['p%d' % (i % 2), w[i], meta[i], np.array([0.0, 1.0]), [float(i)] * nb] for i in range(n)]
    path = tmp_path / 'ft.pkl'
    path.write_bytes(_reference_dataset_pickle(seqs, 'padded_breath_by_breath_with_flow_time_features', 'window', nb=nb, L=L))
    ds = ingest.load_dataset(str(path))
    assert not ds.breath_level and ds.windows.shape == (n, nb, 1, L)
    store = BreathMetaStore.from_windows(ds, device='cpu')
    assert len(store) == n * nb and store.n_targets == 9 and store.padded and store.mu == 0.125 and store.std == 2.5
    assert np.array_equal(store.tiles.numpy().reshape(n, nb, 1, L), w)
    assert np.array_equal(store.targets.numpy(), meta.reshape(n * nb, 9).astype(np.float32))
    assert store.patient_slot.tolist() == [0, 0, 0, 1, 1, 1, 0, 0, 0, 1, 1, 1]
    assert len(BreathMetaStore.from_pickle(str(path), device='cpu')) == n * nb      # from_dataset hands a window dataset on
    plain = ingest.IngestedDataset(w, np.tile([[1.0, 0.0]], (n, 1)), ['a', 'a', 'b', 'b'], np.zeros((n, nb)), {}, nb,
                                   'unpadded_centered_sequences')
    with pytest.raises(ValueError, match='carries no per-breath metadata'):
        BreathMetaStore.from_windows(plain, device='cpu')


def test_store_batches_and_epoch_on_the_host():
    rows, meta, _, _ = _breath_seqs(7, 3)
    store = BreathMetaStore(rows, meta, mu=0.5, std=2.0, device='cpu')
    g = torch.Generator().manual_seed(4)
    batches = epoch_index_batches(store, 4, True, g)
    assert [len(b) for b in batches] == [4, 2]                                         # the odd tail of 3 is clipped
    assert [len(b) for b in epoch_index_batches(store, 4, True, torch.Generator().manual_seed(4), drop_odd=False)] == [4, 3]
    again = epoch_index_batches(store, 4, True, torch.Generator().manual_seed(4))
    assert all(torch.equal(a, b) for a, b in zip(batches, again))
    assert torch.cat(epoch_index_batches(store, 4, False, drop_odd=False)).tolist() == list(range(7))
    with pytest.raises(IndexError):
        store.batch([7])
    with pytest.raises(ValueError):
        BreathMetaStore(rows[:, 0], meta, device='cpu')
    with pytest.raises(ValueError):
        BreathMetaStore(rows, meta[:5], device='cpu')


# ---- the command line ------------------------------------------------------------------------------------------------------------
def test_parser_maps_and_refusals():
    p = build_parser()
    a = p.parse_args(['-n', 'cnn_regressor', '--base-network', 'resnet18', '-dt', 'padded_breath_by_breath_with_full_bm_target',
                      '-b', '128', '--load-base-network', 'x.pth'])
    assert a.network == 'cnn_regressor' and a.batch_size == 128 and a.load_base_network == 'x.pth'
    for dt in BM_TARGET_TYPES:
        assert p.parse_args(['-n', 'cnn_regressor', '-dt', dt]).dataset_type == dt
    assert BM_TARGET_TYPES == {'padded_breath_by_breath_with_limited_bm_target': 3,
                               'padded_breath_by_breath_with_experimental_bm_target': 7,
                               'padded_breath_by_breath_with_full_bm_target': 9}
    with pytest.raises(SystemExit):
        p.parse_args(['-n', 'cnn_linear'])
    with pytest.raises(SystemExit):
        T.build_parser().parse_args(['-dt', 'padded_breath_by_breath_with_full_bm_target'])      # the driver's own parser is as it was
    assert sorted(T.network_map) == PINNED_NETWORK_MAP
    assert T.regressor_network_map == {'cnn_regressor': T.CNNRegressorModel}
    assert T.CNNRegressorModel not in T.network_map.values()
    assert issubclass(T.CNNRegressorModel, (T.BaseTraining, T.RegressorMixin))
    with pytest.raises(SystemExit, match='its own command line'):
        T.main(['-n', 'cnn_regressor', '--cuda-no-dp'])
    with pytest.raises(SystemExit, match='MSELoss'):
        main(['-n', 'cnn_regressor', '-loss', 'bce'])
    with pytest.raises(SystemExit, match='--bm-to-linear'):
        main(['-n', 'cnn_regressor', '--bm-to-linear'])
    dt = 'padded_breath_by_breath_with_full_bm_target'
    with pytest.raises(ValueError, match='no class to stratify'):
        T.CNNRegressorModel(T.make_args(kfolds=5, dataset_type=dt))
    with pytest.raises(NotImplementedError, match='what is being pretrained'):
        T.CNNRegressorModel(T.make_args(freeze_base_network=True, dataset_type=dt))
    with pytest.raises(ValueError, match='MSELoss'):
        T.CNNRegressorModel(T.make_args(loss_func='confidence', dataset_type=dt))
    with pytest.raises(NotImplementedError, match='folds-in-flight'):
        T.CNNRegressorModel(T.make_args(folds_in_flight=2, dataset_type=dt))
    for kw in (dict(conv_dtype='bf16'), dict(conv_dtype='f32x3p'), dict(act_dtype='bf16')):
        with pytest.raises(NotImplementedError, match='float maps only'):
            T.CNNRegressorModel(T.make_args(dataset_type=dt, **kw))


def test_target_width_must_match_the_dataset_type():
    rows, meta, _, _ = _breath_seqs(6, 7)
    drv = object.__new__(T.CNNRegressorModel)
    drv.args = T.make_args(dataset_type='padded_breath_by_breath_with_full_bm_target',
                           train_store=BreathMetaStore(rows, meta, device='cpu'), test_store=None)
    with pytest.raises(ValueError, match='means 9 breath-metadata targets, the train dataset has 7'):
        drv.get_base_datasets()
    drv.args = T.make_args(dataset_type='padded_breath_by_breath_with_flow_time_features',
                           train_store=BreathMetaStore(rows, meta, device='cpu'), test_store=None)
    train, test = drv.get_base_datasets()
    assert drv.n_bm_features == 7 and test is None                                     # a window dataset: the width of its metadata


# ---- the goldens -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('net,r', [(n, r) for n in ('resnet18', 'densenet18') for r in (6, 5, 46)])
def test_numpy_oracle_reproduces_the_reference_golden(net, r):
    """What the GPU tests measure against -- oracle/np_ref with all R rows as one BatchNorm window and regress_ref as the head --
    is the real reference's float64 capture: output, loss, every gradient and (resnet18: every; densenet18: all but the last,
    which the reference applies as a function) ReLU decision."""
    from oracle.weights import digest
    from regressor_case import regressor_oracle
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'regressor_r%d_%s.npz' % (r, net)), allow_pickle=False)
    assert str(g['net']) == net and int(g['rows']) == r
    ref = regressor_oracle(net, r)
    assert ref['out'].shape == (r, 9) and np.abs(ref['out'] - g['out']).max() <= 1e-10 * np.abs(g['out']).max()
    assert abs(ref['loss'][0] - g['loss'][0]) <= 1e-10 * g['loss'][0]
    names = [k[5:] for k in g.files if k.startswith('grad/')]
    assert set(names) == set(ref['grads']) and 'linear_final.weight' in names
    for n in names:
        d, want = digest(ref['grads'][n]), g['grad/' + n]
        body = slice(None) if ref['grads'][n].size <= 1024 else slice(0, -3)
        assert np.abs(d - want)[body].max() <= 1e-9 * max(1.0, np.abs(want[body]).max()), n
        assert 0 <= float(g['err32/grad/' + n]) < 1e-2
    relus = [n for n in ref['tape'].order if ref['tape'].decisions[n]['kind'] == 'relu']
    n_ref = len([k for k in g.files if k.startswith('relu/')])
    assert len(relus) - n_ref == (0 if net == 'resnet18' else 1)
    for i, n in enumerate(relus[:n_ref]):
        mask = ref['tape'].decisions[n]['mask']
        assert tuple(g['relu_shape/%d' % i]) == mask.shape
        assert np.array_equal(np.unpackbits(g['relu/%d' % i])[:mask.size].astype(bool), mask.reshape(-1)), n
