"""GPU tests of the whole-patient recurrence kernels (csrc/seq_wide.hip, deepards_amd/seq_wide_ops.py), the two autograd
Functions around them, the nested networks and their trainer.

Yardstick (that of tests/test_lstm_seq_gpu.py): the case in float64 stock torch on the CPU is the truth; the SAME case in float32
stock torch gives the error a float32 implementation makes; the kernels may err at most MARGIN = 8 times that, both relative
to the output's max magnitude (the factor cancels).  Every figure is printed before it is asserted."""
import ctypes
import os
import sys
import zlib

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
MARGIN = 8.0

from tools import poison as P                                                        # noqa: E402
from tools import nested_ref as NR                                                   # noqa: E402
from test_nested_cpu import KINDS, NB, W, build, golden, golden_params               # noqa: E402

if torch.cuda.is_available():
    from deepards_amd import _lib, hip_ops as H, seq_wide_ops as SW, functional as F_
else:                                   # collected without a GPU (-m "not gpu" deselects every test of this file)
    _lib = H = SW = F_ = None

HID = 128


def rng_of(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def judge(what, got, ref64, ref32):
    """max |got - ref64| <= MARGIN * max |ref32 - ref64|, printed first."""
    got, ref64, ref32 = (np.asarray(v, np.float64) for v in (got, ref64, ref32))
    assert got.shape == ref64.shape, '%s: shape %s vs %s' % (what, got.shape, ref64.shape)
    assert np.isfinite(got).all(), what
    e, e32, mag = np.abs(got - ref64).max(), np.abs(ref32 - ref64).max(), np.abs(ref64).max()
    ratio = e / e32 if e32 > 0 else (0.0 if e == 0 else float('inf'))
    print('%-52s err %.3e  fp32 torch %.3e  ratio %6.2f  (max |ref| %.3e)' % (what, e, e32, ratio, mag))
    assert e <= MARGIN * e32, '%s: error %.3e is %.2f x the float32 torch error %.3e (allowed %g x)' % (what, e, ratio, e32, MARGIN)


def cu(*ts):
    return [t.cuda().contiguous() for t in ts]


def case(kind, s, t, scale, *key):
    """weights (torch's default initialisation), inputs in [0, 1) * scale (medians of ReLU features are >= 0), dhs."""
    g = rng_of(kind, s, t, scale, *key)
    ws = NR.default_weights(kind, g)
    x = torch.rand(s, t, HID, generator=g) * scale
    dhs = torch.randn(s, t, HID, generator=g)
    return ws, x, dhs


def function_of(kind):
    return F_.WideLSTMFunction if kind == 'lstm' else F_.WideRNNFunction


def device_run(kind, ws, x, dhs):
    """The Function on the device: hs and [dw_ih, dw_hh, db_ih, db_hh, dx] of sum(hs * dhs) (device tensors)."""
    s, t, _ = x.shape
    wd = [w.requires_grad_(True) for w in cu(*ws)]
    xd = x.reshape(s * t, HID).cuda().requires_grad_(True)
    hs = function_of(kind).apply(xd, *wd, s)
    (hs * dhs.cuda()).sum().backward()
    return hs.detach(), [w.grad for w in wd] + [xd.grad.view(s, t, HID)]


# ---- the recurrence kernels against float64 torch -------------------------------------------------------------------------
@pytest.mark.parametrize('scale', [1.0, 50.0])
@pytest.mark.parametrize('s', [1, 3])
@pytest.mark.parametrize('t', [1, 2, 3, 65, 257])
@pytest.mark.parametrize('kind', KINDS)
def test_recurrence_against_float64(kind, t, s, scale):
    """hs, dW_ih, dW_hh, both bias gradients and dx.  T = 1 has no recurrence, 2 and 3 take both parities of the double
    buffer, 65 and 257 are one past a wave and one past the prefetch ring's unrolled groups; scale 50: saturated gates."""
    ws, x, dhs = case(kind, s, t, scale)
    hs64, g64 = NR.recurrence(kind, x, ws, dhs, torch.float64)
    hs32, g32 = NR.recurrence(kind, x, ws, dhs, torch.float32)
    hs, grads = device_run(kind, ws, x, dhs)
    tag = '%s T %d S %d x%g ' % (kind, t, s, scale)
    judge(tag + 'hs', hs.cpu().numpy(), hs64, hs32)
    for name, got, r64, r32 in zip(('dw_ih', 'dw_hh', 'db_ih', 'db_hh', 'dx'), grads, g64, g32):
        judge(tag + name, got.cpu().numpy(), r64, r32)


# ---- bits -------------------------------------------------------------------------------------------------------------------------
def raw_run(kind, gx, w_hh, b_ih, b_hh, dhs):
    if kind == 'lstm':
        hs, cs, gates = SW.lstm_fwd(gx, w_hh, b_ih, b_hh)
        return hs, cs, gates, SW.lstm_bwd(dhs, w_hh, cs, gates)
    hs = SW.rnn_fwd(gx, w_hh, b_ih, b_hh)
    return hs, SW.rnn_bwd(dhs, w_hh, hs)


def raw_case(kind, s, t, *key):
    g = rng_of('raw', kind, s, t, *key)
    _, w_hh, b_ih, b_hh = NR.default_weights(kind, g)
    gx = torch.randn(s, t, w_hh.shape[0], generator=g)
    dhs = torch.randn(s, t, HID, generator=g)
    return cu(gx, w_hh, b_ih, b_hh, dhs)


@pytest.mark.parametrize('kind', KINDS)
def test_same_bits_every_call_and_for_every_neighbourhood(kind):
    """Two calls give equal bits; sequence k of an S = 3 call equals the same sequence run alone, forward and backward."""
    for t in (3, 70):
        gx, w_hh, b_ih, b_hh, dhs = raw_case(kind, 3, t)
        a = raw_run(kind, gx, w_hh, b_ih, b_hh, dhs)
        b = raw_run(kind, gx, w_hh, b_ih, b_hh, dhs)
        assert all(P.same_bits(u, v) for u, v in zip(a, b))
        for k in range(3):
            alone = raw_run(kind, gx[k:k + 1].contiguous(), w_hh, b_ih, b_hh, dhs[k:k + 1].contiguous())
            assert all(P.same_bits(u[0], v[k]) for u, v in zip(alone, a)), (t, k)


# ---- memory discipline ------------------------------------------------------------------------------------------------------------
def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


@pytest.mark.parametrize('t', [1, 65])
@pytest.mark.parametrize('kind', KINDS)
def test_outputs_are_fully_written_guards_intact_inputs_unchanged(kind, t):
    """Every operand and output of the two entry points inside pattern-filled guard bands, the outputs pattern-filled too:
    no output element keeps the pattern, the results are the plain call's bits, no guard word changes, no input changes."""
    lib, st, s = _lib.lib(), H._stream(), 2
    gx, w_hh, b_ih, b_hh, dhs = raw_case(kind, s, t, 'guard')
    clean = raw_run(kind, gx, w_hh, b_ih, b_hh, dhs)
    handles = []

    def gd(tensor, poison=False):
        v, hd = P.guarded(tensor)
        handles.append(hd)
        return P.fill_poison(v) if poison else v
    ins = [gd(v) for v in (gx, w_hh, b_ih, b_hh, dhs)]
    ggx, gw, gbi, gbh, gdh = ins
    outs = [gd(torch.zeros_like(v), poison=True) for v in clean]
    if kind == 'lstm':
        ghs, gcs, ggates, gdz = outs
        assert lib.da_seqw_lstm_fwd(_ptr(ggx), _ptr(gw), _ptr(gbi), _ptr(gbh), _ptr(ghs), _ptr(gcs), _ptr(ggates), s, t, HID, st) == 0
        assert lib.da_seqw_lstm_bwd(_ptr(gdh), _ptr(gw), _ptr(gcs), _ptr(ggates), _ptr(gdz), s, t, HID, st) == 0
    else:
        ghs, gdz = outs
        assert lib.da_seqw_rnn_fwd(_ptr(ggx), _ptr(gw), _ptr(gbi), _ptr(gbh), _ptr(ghs), s, t, HID, st) == 0
        assert lib.da_seqw_rnn_bwd(_ptr(gdh), _ptr(gw), _ptr(ghs), _ptr(gdz), s, t, HID, st) == 0
    torch.cuda.synchronize()
    P.assert_guards_intact(handles)
    for o, c in zip(outs, clean):
        assert not P.has_poison(o) and P.same_bits(o, c)
    for i, c in zip(ins, (gx, w_hh, b_ih, b_hh, dhs)):
        assert P.same_bits(i, c)
    with P.poisoned_allocations() as stats:
        again = raw_run(kind, gx, w_hh, b_ih, b_hh, dhs)
    assert stats.filled > 0 and all(P.same_bits(u, v) and not P.has_poison(u) for u, v in zip(again, clean))


def test_refused_shapes_return_minus_one_and_touch_nothing():
    lib, st = _lib.lib(), H._stream()
    for h, t in ((64, 4), (130, 4), (128, 0)):
        tt = max(t, 1)
        a = torch.randn(1, tt, 4 * h).cuda()
        w, b = torch.randn(4 * h, h).cuda(), torch.randn(4 * h).cuda()
        outs = [P.fill_poison(torch.empty(1, tt, 4 * h).cuda()) for _ in range(3)]
        assert lib.da_seqw_rnn_fwd(_ptr(a), _ptr(w), _ptr(b), _ptr(b), _ptr(outs[0]), 1, t, h, st) == -1
        assert lib.da_seqw_rnn_bwd(_ptr(a), _ptr(w), _ptr(a), _ptr(outs[0]), 1, t, h, st) == -1
        assert lib.da_seqw_lstm_fwd(_ptr(a), _ptr(w), _ptr(b), _ptr(b), _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]), 1, t, h, st) == -1
        assert lib.da_seqw_lstm_bwd(_ptr(a), _ptr(w), _ptr(a), _ptr(a), _ptr(outs[0]), 1, t, h, st) == -1
        torch.cuda.synchronize()
        assert all(P.count_poison(o) == o.numel() for o in outs)
    with pytest.raises(ValueError, match='hidden size is 128'):
        SW.rnn_fwd(torch.randn(1, 4, 64).cuda(), torch.randn(64, 64).cuda(), torch.randn(64).cuda(), torch.randn(64).cuda())


# ---- the whole models against the goldens ------------------------------------------------------------------------------------------
def device_model(kind):
    z = golden(kind)
    m = build(kind)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in golden_params(z).items()}, strict=True)
    return z, m.cuda()


@pytest.mark.parametrize('kind', KINDS)
def test_model_against_the_golden(kind):
    """Logits and every parameter gradient of sum(logits * r) within 8 x the reference's own float32 error; the medians select
    the golden's breaths wherever the median is non-zero; window_linear gets no gradient."""
    z, m = device_model(kind)
    picked = []
    orig = H.window_median_fwd

    def spy(feat, nb):
        out, idx = orig(feat, nb)
        picked.append((out, idx))
        return out, idx
    H.window_median_fwd = spy
    try:
        logits = m(torch.from_numpy(z['x']).cuda(), None)
    finally:
        H.window_median_fwd = orig
    assert tuple(logits.shape) == (1, W, 2)
    (logits * torch.from_numpy(z['r']).cuda()).sum().backward()
    med, idx = picked[0]
    live = med.detach().cpu().numpy() != 0
    assert live.any() and np.array_equal(idx.cpu().numpy()[live], z['idx'][live])
    judge(kind + ' logits', logits.detach().cpu().numpy(), z['logits'], z['logits32'])
    for name, p in m.named_parameters():
        if name.startswith('window_linear.'):
            assert p.grad is None
            continue
        ref = z['grad/' + name]
        got = p.grad.cpu().numpy().astype(np.float64)
        e, e32 = np.abs(got - ref).max(), float(z['err32/' + name])
        print('%-52s err %.3e  fp32 reference %.3e  ratio %6.2f  (max |ref| %.3e)' %
              (kind + ' grad ' + name, e, e32, e / e32 if e32 > 0 else float(e > 0) * np.inf, np.abs(ref).max()))
        assert np.isfinite(got).all() and e <= MARGIN * e32, name


# ---- trainer ----------------------------------------------------------------------------------------------------------------------
def patients():
    """Three patients of W = 5, 2, 5 windows (the shape changes, then repeats) from the golden's real rows, NB = 4."""
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'test_dataset_windows.npz'))
    rows = ((z['x'][:, :NB] - float(z['mu'])) / float(z['std'])).astype(np.float32)
    xs = [rows[0:5], rows[5:7], rows[7:12]]
    ts = [[0.0, 1.0], [1.0, 0.0], [0.0, 1.0]]
    return [(torch.from_numpy(np.ascontiguousarray(x)).unsqueeze(0).cuda(), torch.tensor([t]).cuda()) for x, t in zip(xs, ts)]


@pytest.mark.parametrize('loss_calc', ['all_breaths', 'last_breath'])
@pytest.mark.parametrize('kind', KINDS)
def test_trainer_eager_and_captured_steps_agree(kind, loss_calc):
    """Three steps (W = 5, 2, 5), eager and captured: the same parameters bit for bit; each step's loss is the restated
    formula on the step's own logits; window_linear keeps its bits under weight decay; test_step returns (1, W, 2) and moves
    no parameter."""
    from deepards_amd.train import HotPathTrainer
    data = patients()
    runs = []
    for use_graph in (False, True):
        _, m = device_model(kind)
        wl = [m.window_linear.weight.detach().clone(), m.window_linear.bias.detach().clone()]
        tr = HotPathTrainer(m, optimizer='sgd', learning_rate=1e-2, weight_decay=1e-2, use_graph=use_graph, loss_calc=loss_calc)
        losses = []
        for x, t in data:
            loss = tr.train_step(x, t).clone()
            logits = tr.last_logits.clone()
            assert tuple(logits.shape) == (1, x.shape[1], 2)
            want = float(NR.loss(logits.double().cpu(), t.double().cpu(), loss_calc))
            print('%s %s graph %d W %d: loss %.9f restated %.9f' % (kind, loss_calc, use_graph, x.shape[1], float(loss), want))
            assert abs(float(loss) - want) <= 1e-5 * max(1.0, abs(want))        # float32 rounding of a mean of <= 10 softplus terms
            losses.append(loss)
        assert P.same_bits(m.window_linear.weight.detach(), wl[0]) and P.same_bits(m.window_linear.bias.detach(), wl[1])
        before = [p.detach().clone() for p in m.parameters()]
        tl, tlogits, tpred = tr.test_step(*data[1])
        assert tuple(tlogits.shape) == (1, 2, 2) and torch.isfinite(tl).all()
        assert all(P.same_bits(a, b.detach()) for a, b in zip(before, m.parameters()))
        runs.append((losses, before))
        tr.release_graphs()
    (l0, p0), (l1, p1) = runs
    assert all(P.same_bits(a, b) for a, b in zip(l0, l1)) and all(P.same_bits(a, b) for a, b in zip(p0, p1))
    fresh = device_model(kind)[1]
    r = getattr(fresh, kind)
    assert not P.same_bits(dict(zip([n for n, _ in fresh.named_parameters()], p0))[kind + '.weight_hh_l0'], r.weight_hh_l0.detach())


# ---- whole-patient data and the driver ------------------------------------------------------------------------------------------------
DATASET = os.path.join(ROOT, 'tests', 'golden', 'test_dataset.npz')


def test_patient_item_is_the_tile_stores_gather_of_the_patients_windows():
    """item(p) against the window store's own batch of the same windows (bit for bit: it is that launch), whatever fold is
    selected; the target is the patient's one row; the fold's patients are the window path's."""
    from deepards_amd import ingest
    from deepards_amd.nested import PatientSequenceStore
    ds = ingest.load_dataset(DATASET)
    ds.total_kfolds, ds.train = 2, True
    ps = PatientSequenceStore.from_windows(ds)
    test = ps.make_test_store_if_kfold()
    for fold in (0, 1):
        ps.set_kfold_indexes_for_fold(fold)
        test.set_kfold_indexes_for_fold(fold)
        tr_pat, te_pat = [ps.patient_ids[i] for i in ps.selected], [test.patient_ids[i] for i in test.selected]
        assert sorted(tr_pat + te_pat) == list(range(12)) and not set(tr_pat) & set(te_pat)
        assert sorted(te_pat) == sorted(ps.store.kfold_patient_splits[fold]['test'].tolist())
        ps.store.set_kfold_indexes_for_fold(fold)                      # a fold-relative index list on the window store: ignored
        for view in (ps, test):
            for p in range(len(view)):
                idx = view.indices(p)
                x, t = view.item(p)
                assert tuple(x.shape) == (len(idx), 20, 1, 224) and tuple(t.shape) == (1, 2)
                saved, view.store.kfold_indexes = view.store.kfold_indexes, None
                wx, wt = view.store.batch(torch.from_numpy(idx))
                view.store.kfold_indexes = saved
                assert P.same_bits(x, wx) and P.same_bits(t, wt[:1]) and int(t.argmax()) == view.target_label(p)


def test_driver_trains_tests_saves_and_seeds_a_classifier(tmp_path):
    """CNNToNestedLSTMModel: two folds of one epoch on the fixture -- a loss per train patient, patient-level results for every
    test patient with one vote per window; the saved model reloads through load_own_module; --load-base-network of it seeds a
    cnn_linear breath block."""
    from deepards_amd import train_ards_detector as T
    from deepards_amd import checkpoint as C
    import deepards_amd.models as M
    args = T.make_args(train_from_pickle=DATASET, kfolds=2, epochs=1, batch_size=16, seed=3, base_network='densenet18', cuda=False,
                       cuda_no_dp=True, save_model='nested.pth', saved_models_dir=str(tmp_path), loss_calc='last_breath')
    cls = T.CNNToNestedLSTMModel(args)
    assert args.batch_size == 1
    res = cls.train_and_test()
    summary = cls.perform_post_modeling_actions()
    assert type(cls.model) is M.CNNToNestedLSTMNetwork and cls.optimizer.use_graph is False
    slots = np.load(DATASET)['patient_slot']
    seen = []
    for fold in (0, 1):
        r = res.patient_results[(fold, 1)]
        pats = r['patients'].tolist()
        seen += pats
        assert len(res.get_meter('loss', fold)) == 12 - len(pats) and np.isfinite(res.get_meter('loss', fold)).all()
        assert np.isfinite(r['mean_loss']) and np.isfinite(res.get_meter('test_loss', fold)).all()
        for p in range(12):
            assert int(r['votes'][p].sum()) == (int((slots == p).sum()) if p in pats else 0)       # one vote per window
        assert sorted(r['window_abs_index'].tolist()) == sorted(np.flatnonzero(np.isin(slots, pats)).tolist())
        assert set(r['window_pred'].tolist()) <= {0, 1} and summary[(fold, 1)]['patients'] == pats
    assert sorted(seen) == list(range(12))                                                          # every patient tested once
    path = os.path.join(str(tmp_path), 'nested-fold1.pth')
    assert os.path.exists(path) and os.path.exists(os.path.join(str(tmp_path), 'nested-fold0.pth'))
    back = C.load_own_module(path)
    assert type(back) is M.CNNToNestedLSTMNetwork
    want = cls.model.state_dict()
    assert list(back.state_dict().keys()) == list(want.keys())
    assert all(torch.equal(v.cpu(), back.state_dict()[k]) for k, v in want.items())
    stage2 = T.network_map['cnn_linear'](T.make_args(train_from_pickle=DATASET, kfolds=2, epochs=1, batch_size=4, seed=3,
                                                     base_network='densenet18', cuda=False, cuda_no_dp=True,
                                                     load_base_network=path, folds_in_flight=1, debug=True,
                                                     no_test_after_epochs=True))
    first = stage2.get_model().breath_block.state_dict()
    assert all(torch.equal(v.cpu(), first[k].cpu()) for k, v in back.breath_block.state_dict().items())
    assert np.isfinite(stage2.train_and_test().get_meter('loss', 0)).all()


def test_command_line_runs_the_rnn(tmp_path):
    from deepards_amd import nested
    cls, res = nested.main(['-n', 'cnn_to_nested_rnn', '--base-network', 'densenet18', '--cuda-no-dp', '-p', DATASET, '--kfolds', '2',
                            '-e', '1', '-b', '8', '--seed', '1'])
    assert cls.args.batch_size == 1 and sorted(cls.summary) == [(0, 1), (1, 1)]
    assert all(np.isfinite(res.get_meter('loss', f)).all() and len(res.get_meter('loss', f)) > 0 for f in (0, 1))
