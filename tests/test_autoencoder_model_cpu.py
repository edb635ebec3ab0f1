"""CPU tests of the autoencoder's implementation side: the library and its new entries (header, bindings, refusals before any
launch), the chunk plan, the decision-bit packing, the model's state_dict against the golden key list, the checkpoint reader, the
module's parser and the driver class's refusals.  Nothing here needs a GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from tools import ae_ref as R                                                       # noqa: E402

P = 4096            # a dummy non-null device address; never dereferenced
DA_EINVAL = -1
NEW = ('da_bn_maxpool2_idx_fwd', 'da_bn_maxpool2_idx_plan', 'da_bn_maxpool2_idx_bwd_workspace', 'da_bn_maxpool2_idx_bwd',
       'da_unpool2_fwd', 'da_unpool2_bwd', 'da_ae_out_fwd_workspace', 'da_ae_out_bwd_workspace', 'da_ae_out_fwd', 'da_ae_out_bwd')


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from deepards_amd import _lib
    return _lib.lib()


def test_library_builds_with_the_new_source_and_declares_it(lib):
    from deepards_amd import _lib
    assert 'autoencoder.hip' in _lib.SOURCES and os.path.exists(os.path.join(_lib.CSRC, 'autoencoder.hip'))
    header = set(_lib.header_symbols())
    for name in NEW:
        assert name in header and name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert header == set(_lib.SIGNATURES)


# ---- refusals: DA_EINVAL before any launch (every operand a dummy address: a launch would fault, a refusal returns) --------
def _pool_fwd(lib, rows=4, R=2, lin=8, c=64, ldy=None, null=None, sel_in=None):
    a = dict(y=P, out=P, sel=P, sel_in=sel_in, mean=P, invstd=P, gamma=P, beta=P)
    if null:
        a[null] = None
    return lib.da_bn_maxpool2_idx_fwd(a['y'], c if ldy is None else ldy, a['out'], a['sel'], a['sel_in'], rows, R, lin, c,
                                      a['mean'], a['invstd'], a['gamma'], a['beta'], None)


def _pool_bwd(lib, rows=4, R=2, lin=8, c=64, ldy=None, null=None):
    a = dict(dout=P, sel=P, y=P, dy=P, ds=P, ws=P, mean=P, invstd=P, gamma=P, beta=P)
    if null:
        a[null] = None
    return lib.da_bn_maxpool2_idx_bwd(a['dout'], a['sel'], a['y'], c if ldy is None else ldy, a['dy'], a['ds'], a['ws'], rows, R, lin,
                                      c, a['mean'], a['invstd'], a['gamma'], a['beta'], None)


@pytest.mark.parametrize('fn', [_pool_fwd, _pool_bwd])
def test_pool_entries_refuse_before_a_launch(lib, fn):
    assert fn(lib, c=48) == DA_EINVAL and fn(lib, c=16) == DA_EINVAL and fn(lib, c=0) == DA_EINVAL          # C % 32
    assert fn(lib, lin=7) == DA_EINVAL and fn(lib, lin=0) == DA_EINVAL and fn(lib, lin=1) == DA_EINVAL      # odd / short Lin
    assert fn(lib, rows=5, R=2) == DA_EINVAL and fn(lib, R=0) == DA_EINVAL and fn(lib, rows=-2) == DA_EINVAL  # R | rows
    assert fn(lib, ldy=32) == DA_EINVAL and fn(lib, ldy=66) == DA_EINVAL                                    # pitch
    assert fn(lib, rows=1 << 20, R=1, lin=1 << 10, c=64) == DA_EINVAL                                       # 2^32 elements
    names = ('y', 'out', 'mean', 'invstd', 'gamma', 'beta') if fn is _pool_fwd else \
        ('dout', 'sel', 'y', 'dy', 'ds', 'ws', 'mean', 'invstd', 'gamma', 'beta')
    for name in names:
        assert fn(lib, null=name) == DA_EINVAL, name
    assert fn(lib, rows=0) == 0                                                     # nothing to do: no launch, no error


def test_pool_forward_needs_a_source_of_decisions(lib):
    assert _pool_fwd(lib, null='sel', sel_in=None) == DA_EINVAL                     # neither a destination nor given bits
    assert _pool_fwd(lib, rows=0, null='sel', sel_in=P) == 0                        # teacher forcing without a copy is a shape


def test_unpool_entries_refuse_before_a_launch(lib):
    def fwd(rows=4, lo=4, c=64, v=P, sel=P, out=P):
        return lib.da_unpool2_fwd(v, None, sel, out, rows, lo, c, None)

    def bwd(rows=4, lo=4, c=64, dout=P, sel=P, dv=P):
        return lib.da_unpool2_bwd(dout, sel, dv, rows, lo, c, None)
    for fn, ptrs in ((fwd, ('v', 'sel', 'out')), (bwd, ('dout', 'sel', 'dv'))):
        assert fn(c=48) == DA_EINVAL and fn(c=0) == DA_EINVAL and fn(lo=0) == DA_EINVAL and fn(rows=-1) == DA_EINVAL
        assert fn(rows=1 << 20, lo=1 << 10, c=64) == DA_EINVAL
        for name in ptrs:
            assert fn(**{name: None}) == DA_EINVAL, name
        assert fn(rows=0) == 0


def test_output_stage_entries_refuse_before_a_launch(lib):
    def fwd(rows=4, l=8, null=None):
        a = [P] * 10
        if null is not None:
            a[null] = None
        return lib.da_ae_out_fwd(*a, rows, l, None)

    def bwd(rows=4, l=8, null=None):
        a = [P] * 9
        if null is not None:
            a[null] = None
        return lib.da_ae_out_bwd(*a, rows, l, 0, None)
    for fn, n in ((fwd, 10), (bwd, 9)):
        assert fn(l=7) == DA_EINVAL and fn(l=0) == DA_EINVAL and fn(rows=0) == DA_EINVAL and fn(rows=-1) == DA_EINVAL
        assert fn(rows=1 << 20, l=1 << 10) == DA_EINVAL
        for i in range(n):
            assert fn(null=i) == DA_EINVAL, i
    assert lib.da_ae_out_fwd_workspace(4, 7) == 0 and lib.da_ae_out_bwd_workspace(0, -2) == 0
    assert lib.da_ae_out_fwd_workspace(4, 8) == 4 * 1 and lib.da_ae_out_bwd_workspace(40, 224) == 4 * 196 * 280


# ---- the chunk plan ----------------------------------------------------------------------------------------------------------------
def _plan(lib, rows, R, lin, c):
    p, ch, ws = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
    rc = lib.da_bn_maxpool2_idx_plan(rows, R, lin, c, ctypes.byref(p), ctypes.byref(ch), ctypes.byref(ws))
    return rc, p.value, ch.value, ws.value


@pytest.mark.parametrize('rows,R,lin,c', [(1, 1, 2, 32), (3, 3, 6, 64), (5, 5, 28, 512), (40, 40, 224, 64), (1280, 1280, 224, 64),
                                          (1280, 1280, 14, 512), (12, 4, 16, 128), (6, 6, 86, 32), (7, 7, 258, 96)])
def test_chunk_plan_is_deterministic_and_covers_every_pair_once(lib, rows, R, lin, c):
    rc, p, ch, ws = _plan(lib, rows, R, lin, c)
    assert rc == 0 and (rc, p, ch, ws) == _plan(lib, rows, R, lin, c)
    npw = R * (lin // 2)
    seen = np.zeros(npw, dtype=np.int64)
    for k in range(p):
        assert k * ch < npw                                                         # no empty chunk
        seen[k * ch:min((k + 1) * ch, npw)] += 1
    assert (seen == 1).all() and ch % 32 == 0 and 1 <= p <= 65535
    assert ws == (rows // R) * p * 2 * c * 4 == lib.da_bn_maxpool2_idx_bwd_workspace(rows, R, lin, c)


def test_chunk_plan_refuses_what_the_launch_refuses(lib):
    for bad in ((4, 2, 7, 64), (4, 3, 8, 64), (4, 2, 8, 48), (0, 1, 8, 64), (4, 0, 8, 64)):
        assert _plan(lib, *bad)[0] == DA_EINVAL and lib.da_bn_maxpool2_idx_bwd_workspace(*bad) == 0
    from deepards_amd import hip_ops as H
    assert H.bn_maxpool2_idx_plan(40, 40, 224, 64).chunks > 1 and H.bn_maxpool2_idx_plan(1, 1, 2, 32).chunks == 1
    with pytest.raises(H.HipError, match='no launch'):
        H.bn_maxpool2_idx_plan(4, 2, 7, 64)


# ---- the decision bits ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,l', R.MODEL_SHAPES)
def test_sel_packing_round_trips_the_golden_bits(n, l):
    from deepards_amd import hip_ops as H
    g, sels = R.load_golden(n, l)
    for k, want in enumerate(sels, 1):
        raw = np.unpackbits(g['selbits/%d' % k])[:want.size].reshape(want.shape).astype(bool)
        words = H.sel_from_bool(torch.from_numpy(raw))
        c, lo = want.shape[1], want.shape[2]
        assert words.dtype == torch.int32 and tuple(words.shape) == (n, lo, c // 32)
        assert np.array_equal(H.sel_to_bool(words, c).numpy(), raw)
        # the packing itself: word ((row Lo + j) C + c) / 32, bit c % 32
        flat = words.numpy().astype(np.int64).reshape(-1) & 0xffffffff
        for row, ch, j in ((0, 0, 0), (n - 1, c - 1, lo - 1), (n // 2, 33 % c, lo // 2)):
            e = (row * lo + j) * c + ch
            assert bool((flat[e // 32] >> (ch % 32)) & 1) == bool(raw[row, ch, j])
    with pytest.raises(ValueError):
        H.sel_from_bool(torch.zeros(2, 48, 4, dtype=torch.bool))
    with pytest.raises(ValueError):
        H.sel_to_bool(torch.zeros(2, 4, 2, dtype=torch.int64))


# ---- the model -----------------------------------------------------------------------------------------------------------------
def _golden_keys():
    return [str(k) for k in R.load_golden(4, 16)[0]['keys']]


def test_state_dict_has_the_golden_keys_and_shared_tensors():
    import deepards_amd.models as M
    net = M.AutoencoderNetwork(M.AutoencoderCNN())
    sd = net.state_dict()
    assert list(sd.keys()) == _golden_keys() and len(sd) == 92
    cnn = net.base_network
    assert cnn.n_out_filters == 512 and net.breath_block is cnn.encoder and net.breath_block.n_out_filters == 512
    for k in range(1, 5):
        for leaf in ('weight', 'bias'):
            a = sd['base_network.conv_down%d.%s' % (k, leaf)]
            assert a.data_ptr() == sd['base_network.encoder.%d.%s' % (3 * (k - 1), leaf)].data_ptr() == \
                sd['breath_block.%d.%s' % (3 * (k - 1), leaf)].data_ptr()
        for leaf in ('weight', 'bias', 'running_mean', 'running_var', 'num_batches_tracked'):
            a = sd['base_network.bn%d.%s' % (k, leaf)]
            assert a.data_ptr() == sd['base_network.encoder.%d.%s' % (3 * (k - 1) + 1, leaf)].data_ptr() == \
                sd['breath_block.%d.%s' % (3 * (k - 1) + 1, leaf)].data_ptr()
    assert len(list(net.parameters())) == 24                                        # shared, not copied
    assert 'AutoencoderCNN' not in M.BACKBONES and not isinstance(cnn, M.Backbone)
    assert [tuple(getattr(cnn, 'conv_up%d' % k).weight.shape) for k in range(1, 5)] == [(512, 256, 3), (256, 128, 3), (128, 64, 3),
                                                                                          (64, 1, 3)]


def _reference_state_dict():
    params = R.seeded_params(0)
    sd = {k: torch.tensor(v, dtype=torch.float32) for k, v in R.full_state_dict(params, 'base_network.').items()}
    sd.update({'breath_block.' + k[len('encoder.'):]: torch.tensor(v, dtype=torch.float32)
               for k, v in R.full_state_dict(params).items() if k.startswith('encoder.')})
    return params, sd


def test_reference_state_dict_loads():
    import deepards_amd.models as M
    params, sd = _reference_state_dict()
    net = M.AutoencoderNetwork(M.AutoencoderCNN())
    full = net.state_dict()
    for k, v in full.items():                                                       # the buffers the restatement does not carry
        sd.setdefault(k, v.clone())
    net.load_state_dict(sd, strict=True)
    for name, v in params.items():
        assert np.array_equal(dict(net.base_network.named_parameters())[name].detach().numpy(), v.astype(np.float32)), name
    cnn = M.AutoencoderCNN()
    cnn.load_state_dict({k[len('base_network.'):]: v for k, v in sd.items() if k.startswith('base_network.')}, strict=True)


def test_model_refuses_what_it_does_not_run():
    import deepards_amd.models as M
    net = M.AutoencoderNetwork(M.AutoencoderCNN())
    with pytest.raises(Exception, match='4 dimensional'):
        net(torch.zeros(4, 1, 32), None)
    with pytest.raises(NotImplementedError, match='multiple of 16'):
        net(torch.zeros(2, 2, 1, 40), None)
    with pytest.raises(NotImplementedError, match='one channel'):
        net(torch.zeros(2, 2, 2, 32), None)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        net(torch.zeros(2, 2, 1, 32), None)
    with pytest.raises(NotImplementedError, match='second stage'):
        net.breath_block(torch.zeros(2, 1, 224))


def test_load_autoencoder_reads_a_state_dict_and_an_own_module(tmp_path):
    import deepards_amd.models as M
    from deepards_amd import checkpoint
    params, sd = _reference_state_dict()
    path = str(tmp_path / 'ae_state.pth')
    torch.save(sd, path)
    net = checkpoint.load_autoencoder(path)
    assert isinstance(net, M.AutoencoderNetwork)
    assert np.array_equal(net.base_network.conv_up4.weight.detach().numpy(), params['conv_up4.weight'].astype(np.float32))
    assert float(net.base_network.bn1.running_var.min()) == 1.0                    # buffers the file leaves out keep their defaults
    # the same file is still refused as a base network
    import deepards_amd.train_ards_detector as T
    with pytest.raises(ValueError, match='not built in this package'):
        checkpoint.load_base_network(path, T.base_networks, {})
    # DataParallel keys, and a whole module saved by this package
    torch.save({'module.' + k: v for k, v in sd.items()}, path)
    assert isinstance(checkpoint.load_autoencoder(path), M.AutoencoderNetwork)
    net.base_network.last_sels = [torch.zeros(1)]
    own = str(tmp_path / 'ae_module.pth')
    torch.save(net, own)
    back = checkpoint.load_autoencoder(own)
    assert isinstance(back, M.AutoencoderNetwork) and back.base_network.last_sels is None
    assert list(back.state_dict().keys()) == _golden_keys() and back.breath_block is back.base_network.encoder
    assert torch.equal(back.base_network.conv_down3.weight, net.base_network.conv_down3.weight)
    # a classifier's file is not an autoencoder
    torch.save({'breath_block.conv1.weight': torch.zeros(1)}, path)
    with pytest.raises(ValueError, match='not an autoencoder checkpoint'):
        checkpoint.load_autoencoder(path)


# ---- the command line and the driver class -----------------------------------------------------------------------------------
def test_module_parser_accepts_the_autoencoder_and_the_main_parser_does_not():
    import deepards_amd.autoencoder as A
    import deepards_amd.train_ards_detector as T
    ns = A.build_parser().parse_args(['-n', 'autoencoder', '--base-network', 'basic_cnn_ae', '-dt',
                                      'unpadded_downsampled_autoencoder_sequences', '-p', 'x.pkl', '--test-from-pickle', 'y.pkl',
                                      '--save-model', 'ae.pth'])
    assert (ns.network, ns.base_network, ns.dataset_type, ns.train_from_pickle, ns.save_model) == \
        ('autoencoder', 'basic_cnn_ae', 'unpadded_downsampled_autoencoder_sequences', 'x.pkl', 'ae.pth')
    with pytest.raises(SystemExit):
        A.build_parser().parse_args(['-n', 'cnn_linear'])
    with pytest.raises(SystemExit):
        T.build_parser().parse_args(['-n', 'autoencoder'])
    with pytest.raises(SystemExit):
        T.build_parser().parse_args(['--base-network', 'basic_cnn_ae'])
    assert T.build_parser().parse_args(['-dt', 'unpadded_downsampled_autoencoder_sequences']).dataset_type
    assert A.autoencoder_network_map == {'autoencoder': T.AutoencoderModel} and 'autoencoder' not in T.network_map
    assert issubclass(T.AutoencoderModel, (T.BaseTraining, T.RegressorMixin))


def test_autoencoder_model_refuses_the_second_stage_flags():
    import deepards_amd.train_ards_detector as T
    with pytest.raises(NotImplementedError, match='--load-base-network'):
        T.AutoencoderModel(T.make_args(network='autoencoder', load_base_network='some.pth', cuda_no_dp=True))
    with pytest.raises(NotImplementedError, match='--freeze-base-network'):
        T.AutoencoderModel(T.make_args(network='autoencoder', freeze_base_network=True, cuda_no_dp=True))
    with pytest.raises(NotImplementedError, match='folds-in-flight'):
        T.AutoencoderModel(T.make_args(network='autoencoder', folds_in_flight=2, cuda_no_dp=True))


def test_regressor_mixin_books_the_three_meters():
    import deepards_amd.train_ards_detector as T

    class Host(T.RegressorMixin):
        results = T.Results()
    r = np.random.RandomState(1)
    t, p = r.standard_normal((6, 8)), r.standard_normal((6, 8))
    h = Host()
    h.record_testing_results(t, p, 3)
    h.record_testing_results(t, t, 3)
    mae, r2, mse = T.regression_scores(t, p)
    assert h.results.get_meter('test_mae', 3) == [mae, 0.0] and h.results.get_meter('r2', 3) == [r2, 1.0]
    assert h.results.get_meter('test_mse', 3) == [mse, 0.0]
    h.set_loss_criterion()
    assert isinstance(h.criterion, torch.nn.MSELoss)
    assert h.perform_post_modeling_actions()['test_mse/3'] == mse / 2


def test_trainer_refuses_other_models_and_split_batches():
    import deepards_amd.models as M
    from deepards_amd.autoencoder import AutoencoderTrainer
    net = M.AutoencoderNetwork(M.AutoencoderCNN())
    with pytest.raises(NotImplementedError, match='one GPU'):
        AutoencoderTrainer(net, world_size=2)
    with pytest.raises(NotImplementedError, match='folds in flight'):
        AutoencoderTrainer(net, folds_in_flight=2)
    with pytest.raises(TypeError):
        AutoencoderTrainer(torch.nn.Linear(2, 2))
