"""GPU tests of the layers above the two loss kernels: HotPathTrainer's loss selection on cnn_lstm and
cnn_single_breath_linear (against the oracle's model restatement with the loss oracle chained in), ``last_breath``, the
per-patient LSTM state carry of ``--unshuffled``, the cnn_lstm driver and the unchanged bce path."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'tools'))
pytestmark = pytest.mark.gpu

from oracle import np_ref  # noqa: E402
from oracle.weights import seeded_params  # noqa: E402
import loss_ref  # noqa: E402
from decision_match import assert_gradients_match, fp32_noise, plain_twin  # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')


def log(*a):
    print(' '.join(str(x) for x in a))                 # achieved figures: read them with pytest -s


@pytest.fixture(scope='module')
def M():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    import deepards_amd.models as models
    return models


def _gold(name):
    z = np.load(os.path.join(GOLD, name), allow_pickle=False)
    return {k: z[k] for k in z.files}


def build_head(M, g, drop_rate=0.0):
    head, backbone = str(g['head']), str(g['backbone'])
    bb = M.resnet18(first_pool_type=str(g['first_pool_type'])) if backbone == 'resnet18' else M.densenet18(drop_rate=drop_rate)
    model = M.CNNLSTMNetwork(bb, 0, False, 16) if head == 'lstm' else M.CNNSingleBreathLinearNetwork(bb)
    sd = {k: torch.from_numpy(v) for k, v in seeded_params(backbone, int(g['seed']), bn_bias_shift=float(g['bn_bias_shift']),
                                                           head=head).items()}
    assert not model.load_state_dict(sd, strict=False).unexpected_keys
    return model.cuda().train()


class tapped(object):
    def __enter__(self):
        from deepards_amd import functional as F_
        F_.DECISION_TAP = []
        return F_.DECISION_TAP

    def __exit__(self, *exc):
        from deepards_amd import functional as F_
        F_.DECISION_TAP = None


def oracle_step(monkeypatch, g, loss, param, dtype=np.float64):
    """The oracle's model restatement (oracle/np_ref.py, pinned to these goldens by the existing parity tests) with the loss
    oracle (tests/tools/loss_ref.py, pinned to the reference's loss.py by tests/test_losses_cpu.py) in the place of its
    BCE: np_ref hands its loss function the (B * NB, 2) logits and the repeated target.  ``dtype``: the arithmetic of the whole
    run, loss included (float32: the noise figure of decision_match.fp32_noise)."""
    nb = g['x'].shape[1]

    def chained(logits2, target_rep):
        lg, tg = logits2.reshape(-1, nb, 2), target_rep[::nb]
        l, d = (loss_ref.vacillating if loss == 'vacillating' else loss_ref.confidence)(lg, tg, param, dtype=dtype)
        return l, d.reshape(logits2.shape)
    monkeypatch.setattr(np_ref, 'bce_with_logits', chained)
    head, backbone = str(g['head']), str(g['backbone'])
    p64 = {k: v.astype(dtype) for k, v in seeded_params(backbone, int(g['seed']), bn_bias_shift=float(g['bn_bias_shift']),
                                                        head=head).items()}
    return np_ref.cnn_linear_forward_backward(p64, g['x'].astype(dtype), g['target'].astype(dtype), backbone=backbone,
                                              first_pool_type=str(g['first_pool_type']), head=head)


@pytest.mark.parametrize('loss,param', [('vacillating', 2.0), ('confidence', 1.0)])
@pytest.mark.parametrize('gold', ['head_lstm_densenet18_b2.npz', 'head_lstm_densenet18_b2_active.npz',
                                  'head_single_breath_resnet18_b2.npz', 'head_single_breath_resnet18_b2_active.npz'])
def test_one_train_step_matches_the_chained_oracles(M, monkeypatch, gold, loss, param):
    """One train_step from the golden's weights: the loss within 1e-5 and every parameter gradient by the suite's one
    yardstick (decision_match.assert_gradients_match: per tensor 8 x the chained oracles' own float32 error, 1e-4 at the most,
    under the decisions the run took; no ReLU flips on '_active')
    of oracle loss gradient -> oracle model backward.  Then eager == graph-replayed steps, bit for bit."""
    from deepards_amd.train import HotPathTrainer
    g = _gold(gold)
    ref = oracle_step(monkeypatch, g, loss, param)
    assert np.abs(loss_ref.class_means(ref['logits']) - 0.5).min() >= 1e-3 or loss != 'vacillating'
    x, t = torch.from_numpy(g['x']).cuda(), torch.from_numpy(g['target']).cuda()
    model = build_head(M, g)
    tr = HotPathTrainer(model, use_graph=False, clip_grad=False, loss=loss, loss_param=param)
    with tapped() as taps:
        l0 = float(tr.train_step(x, t))
    log('%s %s(%g): loss %.8f vs oracle %.8f' % (gold[:-4], loss, param, l0, ref['loss']))
    assert abs(l0 - ref['loss']) < 1e-5
    ours = {n: p.grad.cpu().numpy().astype(np.float64) for n, p in model.named_parameters()
            if p.grad is not None and n in ref['grads']}
    assert set(ours) == {n for n, p in model.named_parameters() if p.grad is not None} and len(ours) > 10
    noise = fp32_noise(ref, oracle_step(monkeypatch, g, loss, param, dtype=np.float32))
    assert_gradients_match(ref, ours, noise, '%s %s' % (gold[:-4], loss), strict=float(g['bn_bias_shift']) > 0, taps=taps, log=log,
                           twin=plain_twin(os.path.join(GOLD, gold)))
    # eager and graph-replayed steps, bit for bit (step 1 is eager in both; 2 captures and replays; 3, 4 replay)
    ma, mb = build_head(M, g), build_head(M, g)
    ta = HotPathTrainer(ma, use_graph=False, loss=loss, loss_param=param)
    tb = HotPathTrainer(mb, use_graph=True, loss=loss, loss_param=param)
    for step in range(4):
        la, lb = ta.train_step(x, t).clone(), tb.train_step(x, t).clone()
        assert torch.equal(la, lb), (step, float(la), float(lb))
    for (k, p), (_, q) in zip(ma.state_dict().items(), mb.state_dict().items()):
        assert torch.equal(p, q), k
    ea, eb = ta.test_step(x, t), tb.test_step(x, t)                  # the test meter uses the same loss
    assert all(torch.equal(a, b) for a, b in zip(ea, eb))
    with torch.no_grad():
        out = ma(x, None)
        out = out[0] if isinstance(out, tuple) else out
    # (the test step's train-mode forward moved ResNet running statistics, not the output)
    want = (loss_ref.vacillating if loss == 'vacillating' else loss_ref.confidence)(out.double().cpu().numpy(), g['target'], param)[0]
    assert abs(float(ea[0]) - want) < 1e-5
    tb.release_graphs()


def test_two_replays_of_a_captured_step_give_the_same_loss(M):
    """The captured cnn_lstm step with the vacillating loss, replayed twice from the same state (snapshot / restore)."""
    from deepards_amd.train import HotPathTrainer
    g = _gold('head_lstm_densenet18_b2.npz')
    x, t = torch.from_numpy(g['x']).cuda(), torch.from_numpy(g['target']).cuda()
    tr = HotPathTrainer(build_head(M, g, drop_rate=0.2), use_graph=True, loss='vacillating', loss_param=float('inf'))
    tr.train_step(x, t)
    tr.train_step(x, t)                                   # captured now
    snap = tr.snapshot()
    a = tr.train_step(x, t).clone()
    pa = tr.bucket.p.clone()
    tr.restore(snap)
    b = tr.train_step(x, t).clone()
    assert torch.isfinite(a).all() and torch.equal(a, b) and torch.equal(pa, tr.bucket.p)
    tr.release_graphs()


@pytest.mark.parametrize('loss,param', [('bce', None), ('confidence', 0.25)])
def test_last_breath_is_all_breaths_on_the_outputs_cut_to_the_last_breath(M, loss, param):
    """loss_calc = last_breath (CNNLSTMModel.calc_loss, train_ards_detector.py:820-821): loss and gradients are those of the
    all_breaths loss on a copy of the outputs cut to the last breath; every other breath's logits get exactly zero."""
    from deepards_amd import hip_ops as H
    from deepards_amd.train import HotPathTrainer
    g = _gold('head_lstm_densenet18_b2.npz')
    x, t = torch.from_numpy(g['x']).cuda(), torch.from_numpy(g['target']).cuda()
    model = build_head(M, g)
    tr = HotPathTrainer(model, use_graph=False, loss=loss, loss_param=param, loss_calc='last_breath')
    with torch.no_grad():
        logits = model(x, None)[0]
    l_full, d_full = tr._loss(logits, t, want_grad=True)
    cut = logits[:, -1:, :].contiguous()                              # (B, 1, 2): all_breaths on the cut copy
    ref_tr = HotPathTrainer(build_head(M, g), use_graph=False, loss=loss, loss_param=param, loss_calc='all_breaths')
    l_cut, d_cut = ref_tr._loss(cut, t, want_grad=True)
    assert torch.equal(l_full, l_cut)
    assert d_full.shape == logits.shape and torch.equal(d_full[:, -1:, :], d_cut.view(cut.shape))
    assert (d_full[:, :-1, :] == 0).all()
    # through the whole step: the parameter gradients are those of backpropagating the cut gradient alone
    loss_step = tr.train_step(x, t).clone()
    from deepards_amd import functional as F_
    m2 = build_head(M, g)
    with F_.training_step(m2):                                        # the trainer's own sequence, with the cut gradient
        out2 = m2(x, None)[0]
        F_.flush_forward(defer=True)
        cut2 = out2.detach()[:, -1:, :].contiguous()
        l2, d2 = ref_tr._loss(cut2, t, want_grad=True)                # all_breaths on the outputs cut to the last breath
        dz = torch.zeros_like(out2)
        dz[:, -1:, :] = d2.view(cut2.shape)
        out2.backward(dz)
        F_.flush_backward()
    assert torch.equal(loss_step.view(1), l2.view(1))
    for (n, p), (_, q) in zip(model.named_parameters(), m2.named_parameters()):
        assert (p.grad is None) == (q.grad is None), n
        if p.grad is not None:
            assert torch.equal(p.grad, q.grad), n
    with pytest.raises(ValueError, match='per-breath outputs'):
        HotPathTrainer(build_head(M, g), loss='vacillating', loss_calc='last_breath')
    assert H.vacillating_loss is not None


def _fixture_store():
    from deepards_amd import ingest
    ds = ingest.load_npz(os.path.join(GOLD, 'test_dataset.npz'))
    store = ds.to_store(torch.device('cuda'))
    return ds, store


@pytest.mark.parametrize('use_graph', [False, True])
def test_unshuffled_state_carry_equals_the_hand_loop(M, use_graph):
    """cnn_lstm --unshuffled -b 1 over the fixture's first windows (patient slots 0 1 2 2 3 3 4: two carries, five starts
    from zero): the device-carried epoch == a loop that passes hx_cx to the model by hand and drops it at every patient
    boundary (train_ards_detector.py:841-849), losses and the final (hx, cx) bit for bit -- and != the zero-state run."""
    from deepards_amd.train import HotPathTrainer, run_train_epoch_from_store, run_test_epoch
    ds, store = _fixture_store()
    n = 7
    slots = ds.patient_slot[:n].tolist()
    assert slots == [0, 1, 2, 2, 3, 3, 4]
    store.set_kfold_indexes(np.arange(n))
    g = _gold('head_lstm_densenet18_b2.npz')
    kw = dict(use_graph=use_graph, loss='vacillating', loss_param=2.0)
    carried = HotPathTrainer(build_head(M, g), carry_state=True, **kw)
    losses = torch.stack(run_train_epoch_from_store(carried, store, batch_size=1, shuffle=False)).view(-1)
    hx, cx = carried.carried_state()
    # by hand: the model gets hx_cx from the caller; the trainer of the hand loop only supplies loss, backward and update
    model = build_head(M, g)
    hand = HotPathTrainer(model, **dict(kw, use_graph=False))
    zero = HotPathTrainer(build_head(M, g), **kw)
    hand_losses, zero_losses, state, last = [], [], None, None
    for i in range(n):
        x, t = store.batch([i])
        zero_losses.append(zero.train_step(x, t).clone())
        if slots[i] != last:
            state = None
        last = slots[i]
        if hand.bucket is None:                                      # the trainer's first (discovering) step, by hand
            for p in model.parameters():
                p.grad = None
        else:
            hand.bucket.zero_grad()
        from deepards_amd import functional as F_
        with F_.training_step(model):
            logits, state = model(x, None, state)
            F_.flush_forward(defer=True)
            l, d = hand._loss(logits.detach(), t, want_grad=True)
            logits.backward(d.view(logits.shape))
            F_.flush_backward()
        state = (state[0].detach(), state[1].detach())
        if hand.bucket is None:
            from deepards_amd.train import FlatBucket
            hand.bucket = FlatBucket([p for p in model.parameters() if p.requires_grad and p.grad is not None])
        hand._optimizer_step()
        hand_losses.append(l.clone())
    hand_losses, zero_losses = torch.stack(hand_losses).view(-1), torch.stack(zero_losses).view(-1)
    log('carry (graph %s): carried %s' % (use_graph, losses.tolist()))
    log('carry (graph %s): zero    %s' % (use_graph, zero_losses.tolist()))
    assert torch.equal(losses, hand_losses)
    assert torch.equal(hx.view(-1), state[0].view(-1)) and torch.equal(cx.view(-1), state[1].view(-1))
    assert torch.equal(losses[:3], zero_losses[:3])                   # nothing carried before the first repeat patient
    assert not torch.equal(losses[3], zero_losses[3])                 # window 3 starts from window 2's state
    # the test epoch carries too (:868-875), under model.eval(); its state does not leak from the train epoch
    res = run_test_epoch(carried, store, torch.as_tensor(ds.patient_slot), batch_size=1, shuffle=False)
    res0 = run_test_epoch(zero, store, torch.as_tensor(ds.patient_slot), batch_size=1, shuffle=False)
    assert res['votes'].sum() == n * 20 and np.isfinite(res['mean_loss'])
    assert res['mean_loss'] != res0['mean_loss']
    with pytest.raises(ValueError, match='one per step'):
        run_train_epoch_from_store(carried, store, batch_size=2, shuffle=False)
    carried.release_graphs()
    zero.release_graphs()


def test_cli_cnn_lstm_vacillating_runs_on_the_ingested_fixture():
    """``python -m deepards_amd.train_ards_detector -n cnn_lstm -loss vacillating --valpha 2.0 ...`` on the ingested fixture:
    one epoch of train and test, 20 per-breath votes per window, the test epoch under model.eval() (dropout off)."""
    from deepards_amd import train_ards_detector as T
    from deepards_amd import models as M_
    gold = os.path.join(GOLD, 'test_dataset.npz')
    seen = []
    orig = M_.CNNLSTMNetwork.forward

    def spy(self, x, metadata, hx_cx=None):
        seen.append((self.training, torch.is_grad_enabled()))
        return orig(self, x, metadata, hx_cx)
    M_.CNNLSTMNetwork.forward = spy
    try:
        cls, res = T.main(['--cuda-no-dp', '-n', 'cnn_lstm', '-loss', 'vacillating', '--valpha', '2.0', '--train-from-pickle', gold,
                           '--kfolds', '2', '-e', '1', '-b', '4', '--seed', '3', '--no-graph', '--folds-in-flight', '1'])
    finally:
        M_.CNNLSTMNetwork.forward = orig
    a = cls.args
    assert (a.network, a.loss_func, a.valpha, a.loss_calc, a.base_network) == ('cnn_lstm', 'vacillating', 2.0, 'all_breaths', 'densenet18')
    assert isinstance(cls.model, M_.CNNLSTMNetwork) and cls.optimizer.loss == 'vacillating' and cls.optimizer.eval_test
    assert cls.model.breath_block.drop_rate > 0                       # there is a dropout to switch off
    assert any(tr and ge for tr, ge in seen) and any(not ge for tr, ge in seen)
    assert all(not tr for tr, ge in seen if not ge), 'a test-epoch forward ran in train mode (dropout on)'
    assert all(tr for tr, ge in seen if ge)
    tested = []
    for fold in (0, 1):
        losses = res.get_meter('loss', fold)
        assert len(losses) >= 1 and np.isfinite(losses).all()
        r = res.patient_results[(fold, 1)]
        windows = sorted(set(r['window_abs_index'].tolist()))
        assert len(r['window_pred']) == 20 * len(windows) == r['votes'].sum()      # 20 predictions per window
        assert all((r['window_abs_index'] == w).sum() == 20 for w in windows)
        assert np.isfinite(res.get_meter('test_loss', fold)).all()
        tested += windows
    assert len(tested) >= 16 and len(set(tested)) == len(tested)      # (clip_odd_batches drops an odd tail window)
    # captured form and the confidence loss, --unshuffled with the carried state
    cls2, res2 = T.main(['--cuda-no-dp', '-n', 'cnn_lstm', '-loss', 'confidence', '--conf-beta', '0.25', '--train-from-pickle', gold,
                         '--kfolds', '2', '-e', '1', '-b', '1', '--unshuffled', '--seed', '3', '-lc', 'last_breath'])
    assert cls2.optimizer.carry_state and cls2.optimizer.loss_calc == 'last_breath' and cls2.optimizer.use_graph
    for fold in (0, 1):
        assert np.isfinite(res2.get_meter('loss', fold)).all() and np.isfinite(res2.get_meter('test_loss', fold)).all()
        r = res2.patient_results[(fold, 1)]
        assert r['votes'].sum() == 20 * len(set(r['window_abs_index'].tolist()))


def test_default_loss_and_bce_by_name_are_the_same_trainer(M):
    """cnn_linear with the default loss and with loss='bce': three steps, bit-identical losses, logits and parameters, and
    the fused head-plus-loss path in both."""
    from deepards_amd.train import HotPathTrainer
    from deepards_amd import functional as F_
    from oracle.weights import seeded_batch
    x, t = seeded_batch(4, 20, 9)
    xt, tt = torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda()

    def mk():
        model = M.CNNLinearNetwork(M.resnet18(), 20, 0)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_params('resnet18', 4).items()}, strict=False)
        return model.cuda().train()
    calls = []
    orig = F_.head_loss
    F_.head_loss = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    try:
        ta, tb = HotPathTrainer(mk(), use_graph=True), HotPathTrainer(mk(), use_graph=True, loss='bce')
        assert ta._plain_bce and tb._plain_bce and (ta.loss, ta.loss_calc, ta.carry_state) == ('bce', 'all_breaths', False)
        for step in range(3):
            la, lb = ta.train_step(xt + step, tt).clone(), tb.train_step(xt + step, tt).clone()
            assert torch.equal(la, lb) and torch.equal(ta.last_logits, tb.last_logits)
    finally:
        F_.head_loss = orig
    assert len(calls) >= 4                                            # both trainers went through the fused head
    assert torch.equal(ta.bucket.p, tb.bucket.p)
    ta.release_graphs()
    tb.release_graphs()
