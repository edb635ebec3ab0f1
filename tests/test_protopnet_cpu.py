"""CPU tests of the 1-D ProtoPNet: the model surface against goldens written from the reference's own classes (state_dict
keys, shapes, receptive-field info, last-layer initialisation), the receptive-field functions on hand-checkable cases, the
phase -> bucket-range table of the trainer, the refusals, the parser, the untouched network_map, and the float64 reference
of the GPU tests (tests/tools/ppnet_ref.py) against the reference's head numbers and a second composition of the loss."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'tools'))

import ppnet_ref as R  # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')


def _gold(name):
    z = np.load(os.path.join(GOLD, name), allow_pickle=False)
    return {k: z[k] for k in z.files}


# ---- model surface ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backbone, n_convs', [('densenet18', 2), ('densenet121', 6)])
def test_state_dict_keys_shapes_and_rf_info_are_the_references(backbone, n_convs):
    import deepards_amd.models as M
    g = _gold('ppnet_keys.npz')
    torch.manual_seed(0)
    model = M.construct_PPNet(getattr(M, backbone)(), 20)
    head = [(k, v) for k, v in model.state_dict().items() if not k.startswith('breath_block.')]
    assert [k for k, _ in head] == [str(n) for n in g[backbone + '/names']]
    assert ['x'.join(map(str, v.shape)) for _, v in head] == [str(s) for s in g[backbone + '/shapes']]
    assert model.proto_layer_rf_info == g[backbone + '/rf_info'].tolist()
    assert model.proto_layer_rf_info == {'densenet18': [7, 32, 279, 14.5], 'densenet121': [7, 32, 2071, 14.5]}[backbone]
    assert np.array_equal(model.last_layer.weight.detach().numpy(), g[backbone + '/last_layer'])
    assert np.array_equal(model.prototype_class_identity.numpy(), g[backbone + '/identity'])
    convs = [m for m in model.add_on_layers if isinstance(m, torch.nn.Conv1d)]
    assert len(convs) == n_convs and isinstance(model.add_on_layers[-1], torch.nn.Sigmoid)
    assert all(isinstance(m, torch.nn.ReLU) for m in list(model.add_on_layers)[1:-1:2])
    assert all(float(c.bias.detach().abs().max()) == 0.0 for c in convs)
    pv = model.prototype_vectors.detach()
    assert 0.0 <= float(pv.min()) and float(pv.max()) < 1.0
    assert not model.ones.requires_grad and bool((model.ones == 1).all())
    assert (model.epsilon, model.num_prototypes, model.num_classes, model.seq_len) == (1e-4, 20, 2, 224)
    # position-independent bits: the breath block of a PPNet keeps off the fused dense-block kernels; a plain DenseNet does not
    assert model.breath_block.features.block_kernels is False and getattr(M, backbone)().features.block_kernels is True
    assert model.prototype_class_identity_orig.shape == (20, 2)
    rep = repr(model)
    assert rep.startswith('PPNet(\n\tfeatures: DenseNet(') and rep.endswith(
        '\tseq_len: 224,\n\tprototype_shape: (20, 128, 1),\n\tproto_layer_rf_info: %s,\n\tnum_classes: 2,\n\tepsilon: 0.0001\n)'
        % (model.proto_layer_rf_info,))
    for name in ('conv_features', 'prototype_distances', 'distance_2_similarity', 'seq_forward', 'forward', 'push_forward',
                 'set_last_layer_incorrect_connection', 'ensure_incorrect_protos_zeroed'):
        assert callable(getattr(model, name)), name


def test_regular_add_on_identity_repeats_and_average_linear():
    import deepards_amd.models as M
    m = M.construct_PPNet(M.densenet121(), 3, add_on_layers_type='regular', prototype_shape=(8, 64, 1))
    convs = [c for c in m.add_on_layers if isinstance(c, torch.nn.Conv1d)]
    assert [(c.in_channels, c.out_channels) for c in convs] == [(1024, 64), (64, 64)]
    assert m.prototype_class_identity.shape == (3 * 8, 2) and m.last_layer.weight.shape == (2, 24)   # sub_batch_size repeats
    a = M.construct_PPNet(M.densenet18(), 20, average_linear=True)
    assert a.last_layer.weight.shape == (2, 20) and a.prototype_class_identity_linear_layer is a.prototype_class_identity_orig
    assert a.last_layer.bias is None


def test_last_layer_connection_and_zeroing():
    import deepards_amd.models as M
    m = M.construct_PPNet(M.densenet18(), 2, prototype_shape=(4, 32, 1), incorrect_strength=-0.25)
    want = torch.tensor([[1, 1, -0.25, -0.25] * 2, [-0.25, -0.25, 1, 1] * 2])
    assert torch.equal(m.last_layer.weight.data, want)
    m.last_layer.weight.data.mul_(3.0)
    m.ensure_incorrect_protos_zeroed()
    assert torch.equal(m.last_layer.weight.data, torch.tensor([[3., 3, 0, 0] * 2, [0, 0, 3., 3] * 2]))
    m.set_last_layer_incorrect_connection()
    assert torch.equal(m.last_layer.weight.data, want)
    d = torch.tensor([0.0, 1.0, 128.0], dtype=torch.float64)
    assert torch.allclose(m.distance_2_similarity(d), torch.log((d + 1) / (d + 1e-4)), rtol=0, atol=0)


def test_receptive_field_functions_on_hand_checked_cases():
    import deepards_amd.models as M
    # integer padding: conv k7 s2 p3 on 224 samples -> 112 positions, jump 2, field 7, first centre 0.5 + (3 - 3) * 1
    assert M.compute_layer_rf_info(7, 2, 3, [224, 1, 1, 0.5]) == [112, 2, 7, 0.5]
    # then pool k3 s2 p1: 56 positions, jump 4, field 7 + 2 * 2 = 11, centre 0.5 + (1 - 1) * 2
    assert M.compute_layer_rf_info(3, 2, 1, [112, 2, 7, 0.5]) == [56, 4, 11, 0.5]
    # 'VALID': k3 s1 on 10 -> 8, no padding: centre moves by (k - 1) / 2 jumps
    assert M.compute_layer_rf_info(3, 1, 'VALID', [10, 2, 5, 1.5]) == [8, 2, 9, 3.5]
    # 'SAME': k3 s2 on 10 (10 % 2 == 0: pad 1, left pad 0); on 9 (9 % 2 == 1: pad 2, left pad 1)
    assert M.compute_layer_rf_info(3, 2, 'SAME', [10, 1, 1, 0.5]) == [5, 2, 3, 1.5]
    assert M.compute_layer_rf_info(3, 2, 'SAME', [9, 1, 1, 0.5]) == [5, 2, 3, 0.5]
    # a k1 prototype layer changes nothing
    assert M.compute_proto_layer_rf_info_v2(224, [7, 3], [2, 2], [3, 1], 1) == [56, 4, 11, 0.5]
    info = [7, 32, 279, 14.5]
    assert M.compute_rf_protoL_at_spatial_location(224, 0, info) == [0, 154]          # 14.5 -+ 139.5, clipped to the row
    assert M.compute_rf_protoL_at_spatial_location(224, 6, info) == [67, 224]         # 206.5 -+ 139.5
    assert M.compute_rf_protoL_at_spatial_location(2000, 6, info) == [67, 346]
    assert M.compute_rf_prototype(224, [5, 3, 6], info) == [5, 67, 224]
    assert M.compute_rf_prototypes(224, [[5, 3, 6], [1, 0, 0]], info) == [[5, 67, 224], [1, 0, 154]]
    with pytest.raises(AssertionError):
        M.compute_rf_protoL_at_spatial_location(224, 7, info)


def test_refusals_come_with_a_reason():
    import deepards_amd.models as M
    from deepards_amd import train_ards_detector as T
    with pytest.raises(NotImplementedError, match="'log'"):
        M.construct_PPNet(M.densenet18(), 20, prototype_activation_function='linear')
    with pytest.raises(NotImplementedError, match="'log'"):
        M.construct_PPNet(M.densenet18(), 20, prototype_activation_function=lambda d: -d)
    with pytest.raises(NotImplementedError, match='kernel size 1'):
        M.construct_PPNet(M.densenet18(), 20, prototype_shape=(20, 128, 3))
    with pytest.raises(NotImplementedError, match='DenseNet'):
        M.construct_PPNet(M.resnet18(), 20)
    with pytest.raises(NotImplementedError, match='prototype_shape'):
        M.construct_PPNet(M.densenet18(), 20, prototype_shape=(20, 100, 1))
    with pytest.raises(NotImplementedError, match='prototype_shape'):
        M.construct_PPNet(M.densenet18(), 20, prototype_shape=(128, 128, 1))
    with pytest.raises(NotImplementedError, match='DenseNet'):
        T.ProtoPNet1DModel(T.make_args(base_network='resnet18'))
    with pytest.raises(NotImplementedError, match='folds-in-flight'):
        T.ProtoPNet1DModel(T.make_args(folds_in_flight=2))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        T.ProtoPNet1DModel(T.make_args(cuda=False))
    from deepards_amd.protopnet import ProtoPNetTrainer
    with pytest.raises(NotImplementedError, match='one GPU'):
        ProtoPNetTrainer(M.construct_PPNet(M.densenet18(), 20), world_size=2)
    with pytest.raises(TypeError, match='PPNet'):
        ProtoPNetTrainer(M.CNNLinearNetwork(M.densenet18(), 20, 0))
    with pytest.raises(ValueError, match='phase'):
        ProtoPNetTrainer(M.construct_PPNet(M.densenet18(), 20), phase='push')
    model = M.construct_PPNet(M.densenet18(), 20)
    with pytest.raises(RuntimeError, match='no CPU fallback|MI355X'):
        model(torch.zeros(1, 20, 1, 224), None)


# ---- trainer: phases ---------------------------------------------------------------------------------------------------------
def test_phase_to_bucket_range_table():
    from deepards_amd.protopnet import phase_ranges, PHASE_GROUPS, GROUPS, DECAYED
    bounds = {'breath_block': (0, 640), 'add_on': (640, 1024), 'prototypes': (1024, 1088), 'last_layer': (1088, 1152)}
    assert phase_ranges('warm', bounds, 1e-4) == [(640, 1024, 1e-4), (1024, 1088, 0.0)]
    assert phase_ranges('joint', bounds, 1e-4) == [(0, 1024, 1e-4), (1024, 1088, 0.0)]      # one launch for both decayed groups
    assert phase_ranges('last_layer', bounds, 1e-4) == [(1088, 1152, 1e-4)]
    assert phase_ranges('joint', bounds, 0.0) == [(0, 1088, 0.0)]                          # no decay anywhere: one range
    frozen = dict(bounds, breath_block=(0, 0))
    assert phase_ranges('joint', frozen, 1e-4) == [(640, 1024, 1e-4), (1024, 1088, 0.0)]
    with pytest.raises(ValueError):
        phase_ranges('push', bounds, 0.0)
    assert GROUPS == ('breath_block', 'add_on', 'prototypes', 'last_layer') and 'prototypes' not in DECAYED
    assert set(PHASE_GROUPS) == {'warm', 'joint', 'last_layer'}


def test_set_phase_switches_which_parameters_require_a_gradient():
    import deepards_amd.models as M
    from deepards_amd.protopnet import ProtoPNetTrainer
    model = M.construct_PPNet(M.densenet18(), 20)
    tr = ProtoPNetTrainer(model, use_graph=False)

    def on():
        return {n.split('.')[0] for n, p in model.named_parameters() if p.requires_grad}
    assert tr.phase == 'warm' and on() == {'add_on_layers', 'prototype_vectors'}
    assert tr.set_phase('joint') is tr and on() == {'breath_block', 'add_on_layers', 'prototype_vectors'}
    tr.set_phase('last_layer')
    assert on() == {'last_layer'}
    tr.set_phase('warm')
    assert on() == {'add_on_layers', 'prototype_vectors'} and not model.ones.requires_grad
    assert tr.clip == 0.0 and tr.momentum == 0.0 and tr.eval_test and tr.max_dist == 128.0
    assert ProtoPNetTrainer(model, clip_grad=True, clip_val=0.01).clip == 0.0              # taken and ignored: never clips


# ---- parser / configuration ------------------------------------------------------------------------------------------------
def test_parser_flags_and_defaults():
    from deepards_amd import train_ards_detector as T
    from deepards_amd.config import Configuration
    p = T.build_parser()
    ns = p.parse_args(['--n-warm-epochs', '2', '-pse', '4', '--push-every-n', '3', '--n-push-iters', '1', '--clust-lambda', '0.5',
                       '--sep-lambda', '0.1', '-np', '5', '-ic', '-0.1', '--average-linear-layer', '--use-l1', '-dt',
                       'unpadded_centered_with_bm'])
    assert (ns.n_warm_epochs, ns.push_start_epoch, ns.push_every_n, ns.n_push_iters, ns.clust_lambda, ns.sep_lambda,
            ns.n_prototypes, ns.incorrect_strength, ns.average_linear_layer, ns.use_l1, ns.dataset_type) == \
        (2, 4, 3, 1, 0.5, 0.1, 5, -0.1, True, True, 'unpadded_centered_with_bm')
    assert p.parse_args(['--push-start-epoch', '9', '--n-prototypes', '7', '--incorrect-strength', '0']).push_start_epoch == 9
    assert all(v is None for v in vars(p.parse_args([])).values()), 'every parser default must be None'
    for flag in ('--n-warm-epochs', '-pse', '--push-start-epoch', '--push-every-n', '--n-push-iters', '--clust-lambda',
                 '--sep-lambda', '-np', '--n-prototypes', '-ic', '--incorrect-strength', '--average-linear-layer', '--use-l1'):
        assert flag not in T.OUT_OF_SCOPE_FLAGS
    for flag in ('-vse', '--viz-start-epoch', '--prototype-results-dir'):                  # the figures stay out of scope
        assert flag in T.OUT_OF_SCOPE_FLAGS
    a = Configuration(p.parse_args([]), T.BUILD_DEFAULTS)
    ref = (3, 6, 6, 5, 0.8, 0.2, 10, -0.5)                                                 # the reference's defaults.yml:50-61
    assert (a.n_warm_epochs, a.push_start_epoch, a.push_every_n, a.n_push_iters, a.clust_lambda, a.sep_lambda, a.n_prototypes,
            a.incorrect_strength) == ref
    assert a.use_l1 is None and a.average_linear_layer is None
    m = T.make_args()
    assert (m.n_warm_epochs, m.push_start_epoch, m.push_every_n, m.n_push_iters, m.clust_lambda, m.sep_lambda, m.n_prototypes,
            m.incorrect_strength) == ref
    assert m.use_l1 is False and m.average_linear_layer is False
    assert Configuration(p.parse_args(['-np', '3']), T.BUILD_DEFAULTS).n_prototypes == 3


def test_network_map_is_untouched_and_the_driver_class_is_there():
    from deepards_amd import train_ards_detector as T
    assert sorted(T.network_map) == ['cnn_double_linear', 'cnn_linear', 'cnn_linear_compr_to_rf', 'cnn_linear_to_mean',
                                     'cnn_lstm', 'cnn_single_breath_linear']
    assert T.ProtoPNet1DModel not in T.network_map.values()
    for name in ('get_optimizer', 'calc_loss', 'run_train_epoch', 'run_test_epoch', 'get_network', 'push_func',
                 '_process_test_batch_results', 'train_and_test'):
        assert callable(getattr(T.ProtoPNet1DModel, name)), name


def test_library_surface():
    from deepards_amd import _lib
    assert 'protopnet.hip' in _lib.SOURCES
    assert set(_lib.header_symbols()) == set(_lib.SIGNATURES)
    for name in ('da_bias_act_fwd', 'da_bias_act_bwd', 'da_proto_fwd', 'da_proto_bwd', 'da_ppnet_loss'):
        assert name in _lib.SIGNATURES


# ---- the float64 reference of the GPU tests ----------------------------------------------------------------------------------
def _head_gold():
    g = _gold('ppnet_head.npz')
    hp = {k[3:]: v for k, v in g.items() if k.startswith('hp/')}
    return g, hp


def test_ppnet_ref_reproduces_the_references_head():
    """ppnet_ref in float64 against the reference's own float64 run of its modules (add_on_layers, _l2_convolution, min-pool,
    distance_2_similarity, last_layer) on the golden's seeded map and parameters: 1e-12 rel-l2 on every tensor."""
    g, hp = _head_gold()
    assert g['map'].shape == (40, 128, 7) and sorted(hp) == sorted(R.seeded_head(int(g['seed'])))
    mine = R.head_case(g['map'], hp, int(g['nb']), g['g_logits'], g['g_min'])
    names = ['logits', 'min_distances', 'dmap'] + ['grad/' + k for k in hp]
    for k in names:
        assert R.rel_l2(mine[k], g[k]) <= 1e-12, k
        assert 0 < float(g['err32/' + k]) < 1e-5, k
    # the golden's inputs are the seeded ones
    assert np.array_equal(g['map'], R.seeded_map(int(g['seed']), 40, 128, 7))
    for k, v in R.seeded_head(int(g['seed'])).items():
        assert np.array_equal(hp[k], v), k


def test_direct_and_expanded_distances_agree_and_the_direct_form_is_exact_on_a_patch():
    rng = np.random.default_rng(3)
    z = torch.from_numpy(rng.random((3, 32, 5)))
    protos = torch.from_numpy(rng.random((6, 32, 1)))
    protos[2, :, 0] = z[1, :, 3]
    a, b = R.l2_convolution(z, protos), R.l2_direct(z, protos)
    assert R.rel_l2(a.numpy(), b.numpy()) < 1e-13
    assert float(b[1, 2, 3]) == 0.0
    _, min_d, arg, sim = R.prototype_layer(z, protos, direct=True)
    assert int(arg[1, 2]) == 3 and float(min_d[1, 2]) == 0.0 and abs(float(sim[1, 2]) - np.log(1e4)) < 1e-12


def _independent_loss(logits, target, min_d, p, nb, max_dist, cl, sl):
    """calc_loss written a second time, with loops and numpy, from the issue's sentences."""
    logits, target, min_d = (np.asarray(a, np.float64) for a in (logits, target, min_d))
    b = logits.shape[0]
    cls = clu = sep = 0.0
    for i in range(b):
        e = np.exp(logits[i] - logits[i].max())
        s = e / e.sum()
        for c in range(2):
            cls -= target[i, c] * max(np.log(s[c]), -100.0) + (1 - target[i, c]) * max(np.log(1 - s[c]), -100.0)
        label = int(np.argmax(target[i]))
        best_c = best_s = 0.0                                   # the masked-out zeros take part in both maxima
        first_c = first_s = True
        for j in range(nb * p):
            own = ((j % p) // (p // 2)) == label
            v = max_dist - min_d[i, j]
            vc, vs = (v, 0.0) if own else (0.0, v)
            best_c = vc if first_c else max(best_c, vc)
            best_s = vs if first_s else max(best_s, vs)
            first_c = first_s = False
        clu += max_dist - best_c
        sep += max_dist - best_s
    cls, clu, sep = cls / (2 * b), clu / b, sep / b
    return cls + cl * clu + sl * sep, cls, clu, sep


@pytest.mark.parametrize('b, nb, p, far', [(1, 20, 20, False), (5, 3, 4, False), (2, 20, 20, True)])
def test_ppnet_ref_loss_against_a_second_composition(b, nb, p, far):
    rng = np.random.default_rng([b, nb, p])
    logits = rng.standard_normal((b, 2)) * 2
    target = np.eye(2)[rng.integers(0, 2, b)]
    min_d = rng.random((b, nb * p)) * 40
    if far:
        min_d[0] += 200.0                                         # a row beyond max_dist: both maxima are the zero
    got = R.calc_loss(torch.from_numpy(logits), torch.from_numpy(target), torch.from_numpy(min_d), p, nb, 128.0, 0.8, 0.2)
    want = _independent_loss(logits, target, min_d, p, nb, 128.0, 0.8, 0.2)
    for a, w in zip(got[:4], want):
        assert abs(float(a) - w) <= 1e-12 * max(1.0, abs(w))
    assert float(got[4]) == 0.0
    if far:
        md = torch.from_numpy(min_d).requires_grad_(True)
        R.calc_loss(torch.from_numpy(logits), torch.from_numpy(target), md, p, nb, 128.0, 0.8, 0.2)[0].backward()
        assert float(md.grad[0].abs().max()) == 0.0 and float(md.grad[1].abs().sum()) > 0
    w = torch.from_numpy(rng.standard_normal((2, nb * p)))
    l1 = R.calc_loss(torch.from_numpy(logits), torch.from_numpy(target), torch.from_numpy(min_d), p, nb, 128.0, 0.8, 0.2,
                     l1_weight=w, l1_identity=R.class_identity(p, nb))
    mask = 1 - R.class_identity(p, nb).numpy().T
    assert abs(float(l1[4]) - np.abs(w.numpy() * mask).sum()) < 1e-12
    assert abs(float(l1[0]) - (want[0] + 1e-4 * float(l1[4]))) < 1e-12


def test_numpy_push_first_minimum_strict_replacement_and_an_absent_class():
    rng = np.random.default_rng(11)
    b, nb, d, l, p = 4, 3, 8, 5, 4
    z = rng.random((b, nb, d, l)).astype(np.float32)
    dist = (rng.random((b, nb, p, l)) + 1.0).astype(np.float32)
    labels = np.array([0, 0, 1, 0])
    dist[1, 2, 0, 4] = dist[3, 0, 0, 1] = 0.5                      # a tie for prototype 0: the earlier window wins
    dist[0, 1, 3, 2] = 0.1                                         # the global minimum of prototype 3 lies in a window of class 0
    st = R.push_batch(R.push_state(p, d), z, dist, labels, start=10)
    assert st['source'][0].tolist() == [11, 2, 4] and st['min_dist'][0] == np.float32(0.5)
    assert np.array_equal(st['patches'][0], z[1, 2, :, 4])
    assert st['source'][3, 0] == 12 and st['min_dist'][3] > 0.1       # class 1 has window 2 only
    assert st['rf_boxes'][3].tolist() == [12, -1, -1, 1]
    before = {k: v.copy() for k, v in st.items()}
    worse = dist.copy()
    worse[worse < 1.0] = 1.0
    st = R.push_batch(st, z, np.maximum(worse, dist), labels, start=20)   # nothing strictly smaller: nothing changes
    assert all(np.array_equal(before[k], st[k]) for k in before)
    only0 = R.push_batch(R.push_state(p, d), z, dist, np.zeros(4, np.int64), start=0)
    assert np.isinf(only0['min_dist'][2:]).all() and not only0['patches'][2:].any() and (only0['source'][2:] == -1).all()
