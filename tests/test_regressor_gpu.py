"""GPU tests of the breath-metadata pretraining stage: the head kernels against the float64 numpy reference at their shape edges
(bounds from the reference's own float32 error), their memory discipline and determinism, the whole model against goldens from
the real reference, the trainer (eager == captured, tail batches, test step) and two epochs of the driver class."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'tools'))

import poison as P                                                                  # noqa: E402
import regress_ref as R                                                             # noqa: E402
from decision_match import assert_gradients_match, bound, fp32_noise               # noqa: E402
from regressor_case import M_OUT, regressor_case, regressor_oracle                  # noqa: E402
from oracle.weights import digest                                                   # noqa: E402
from deepards_amd import hip_ops as H, regress_ops as RO                            # noqa: E402,F401  (hip_ops first: it re-exports the family)
from deepards_amd import train_ards_detector as T                                   # noqa: E402
from deepards_amd.regressor import BreathMetaStore, RegressorTrainer, epoch_index_batches   # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FORWARD_BOUND = 1e-4                   # the project's stated forward bound (BASELINE north star), relative to the tensor's scale


def log(*a):
    """Every measured figure is printed before it is judged (``pytest -s`` shows them; a failing test's report holds them)."""
    print(' '.join(str(x) for x in a))


@pytest.fixture(scope='module')
def M():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    import deepards_amd.models as models
    return models


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- the head against regress_ref ------------------------------------------------------------------------------------------------
RPB = RO.ROWS_PER_BLOCK                 # test_head_rows_per_block holds it to da_regress_rows_per_block()
ROWS = (1, RPB - 1, RPB, RPB + 1, 2 * RPB + 3)
WIDTHS = (32, 256, 288, 3584)           # fewer columns than one wave's 16-byte sweep, exactly one sweep, a tail, the VGG width
OUTPUTS = (1, 3, 9, 16)
LAYOUTS = ('map', 'map_ld', 'flat', 'flat_ld')


def _head_cases():
    """Every (R, F) pair once; M, the layout, gscale and accumulate cycle so that each value meets each R and each F; then the
    scalar path (F no multiple of 4) in both forms."""
    cases = []
    for i, r in enumerate(ROWS):
        for j, f in enumerate(WIDTHS):
            cases.append((r, f, OUTPUTS[(i + j) % 4], LAYOUTS[(3 * i + j) % 4], (1.0, 0.25)[(i + j // 2) % 2], bool((i // 2 + j) % 2)))
    cases += [(RPB + 1, 30, 3, 'map', 0.25, True), (2 * RPB + 3, 65, 16, 'flat', 1.0, False), (3, 34, 9, 'map_ld', 1.0, True)]
    return cases


HEAD_CASES = _head_cases()


def test_head_rows_per_block_and_case_coverage():
    assert RO.regress_rows_per_block() == RPB
    for vals, pos in ((ROWS, 0), (WIDTHS, 1), (OUTPUTS, 2), (LAYOUTS, 3), ((1.0, 0.25), 4), ((False, True), 5)):
        assert set(vals) <= {c[pos] for c in HEAD_CASES}
    assert {(c[3].startswith('map'), c[5]) for c in HEAD_CASES} == {(a, b) for a in (True, False) for b in (True, False)}


def _place(x, layout, name):
    """x on the device between guard bands; '*_ld': as a slice of a wider pattern-filled buffer."""
    t = cuda(x)
    if not layout.endswith('_ld'):
        return P.guarded(t, name=name)
    f = t.shape[-1]
    ld, off = f + 36, 4                                   # (multiples of 4: the slice stays on the 16-byte path when F is)
    if t.dim() == 3:
        return P.pitched(t, ld, off, name=name)
    v, h = P.pitched(t.view(t.shape[0], 1, f), ld, off, name=name)
    return v[:, 0, :], h


def _run_head(c, layout, gscale, accumulate, dw0, db0):
    """One forward + backward with every output and the workspace between guard bands, starting from the poison pattern."""
    r, m, f = c['target'].shape[0], c['w'].shape[0], c['w'].shape[1]
    form = RO.MAP if layout.startswith('map') else RO.FLAT
    handles = []

    def keep(pair):
        handles.append(pair[1])
        return pair[0]
    x = keep(_place(c['x'], layout, 'x'))
    w, bias, target = (keep(P.guarded(cuda(c[k]), name=k)) for k in ('w', 'bias', 'target'))
    empty = lambda shape, name, lay='': keep(_place(np.zeros(shape, dtype=np.float32), lay, name))
    feat = empty((r, f), 'feat') if form == RO.MAP else None
    out, loss = empty((r, m), 'out'), empty((1,), 'loss')
    dx = empty(c['x'].shape, 'dx', layout)
    dw, db = keep(P.guarded(cuda(dw0), name='dW')), keep(P.guarded(cuda(db0), name='db'))
    work = empty((max(RO.regress_workspace(r, f, m) // 4, 1),), 'workspace')
    fresh = [t for t in (feat, out, loss, work) if t is not None] + ([] if accumulate else [dw, db])
    for t in fresh:
        P.fill_poison(t)
    # (dx may be a slice: every element of the slice gets the pattern, the buffer around it holds it already)
    dx.copy_(P.fill_poison(torch.empty(dx.shape, device='cuda', dtype=torch.float32)))
    got_feat, _, _ = RO.regress_fwd(x, w, bias, target, bufs=(feat, out, loss))
    RO.regress_bwd(got_feat, w, out, target, form, dx=dx, dparams=(dw, db), accumulate=accumulate, gscale=gscale, workspace=work)
    torch.cuda.synchronize()
    P.assert_guards_intact(handles)
    res = dict(out=out, loss=loss, dx=dx, dW=dw, db=db)
    if form == RO.MAP:
        res['feat'] = feat
    for k, t in res.items():
        assert not P.has_poison(t), '%s: an output element was never written' % k
    n_part = RO.regress_workspace(r, f, m) // 4
    assert not P.has_poison(work[:n_part]), 'a partial row was read before it was written'
    return {k: t.clone() for k, t in res.items()}


@pytest.mark.parametrize('r,f,m,layout,gscale,accumulate', HEAD_CASES,
                         ids=['r%d_f%d_m%d_%s_g%s_%s' % (c[0], c[1], c[2], c[3], c[4], 'acc' if c[5] else 'ow') for c in HEAD_CASES])
def test_head_matches_float64_reference_within_the_float32_yardstick(M, r, f, m, layout, gscale, accumulate):
    """Per tensor: rel-l2(ours, fp64) <= min(max(8 err32, 16 2^-23), 1e-4), err32 the rel-l2 of regress_ref's float32 run against
    its float64 run on the same operands.  Outputs and workspace start from poison between guard bands;
    a second run gives the same bits."""
    form = 1 if layout.startswith('map') else 0
    c = R.make_case(r, f, m, form, seed=3)
    rng = np.random.RandomState(r * 31 + f)
    dw0 = (rng.randn(m, f) * 0.5).astype(np.float32) if accumulate else np.zeros((m, f), dtype=np.float32)
    db0 = (rng.randn(m) * 0.5).astype(np.float32) if accumulate else np.zeros((m,), dtype=np.float32)
    ref64 = R.run(c['x'], c['w'], c['bias'], c['target'], gscale=gscale, dtype=np.float64)
    ref32 = R.run(c['x'], c['w'], c['bias'], c['target'], gscale=gscale, dtype=np.float32)
    for k, start in (('dW', dw0), ('db', db0)):                       # (+)=: the destination's start is part of the result
        ref64[k] = start.astype(np.float64) + ref64[k]
        ref32[k] = start + ref32[k]
    got = _run_head(c, layout, gscale, accumulate, dw0, db0)
    again = _run_head(c, layout, gscale, accumulate, dw0, db0)
    tag = 'head r%d f%d m%d %s g%s %s' % (r, f, m, layout, gscale, 'acc' if accumulate else 'ow')
    bad = []
    for k, t in got.items():
        assert P.same_bits(t, again[k]), '%s %s: a second run gives other bits: %s' % (tag, k, P.diff_report(t, again[k]))
        ours = t.cpu().numpy().astype(np.float64)
        err, err32 = R.rel_l2(ours, ref64[k]), R.rel_l2(ref32[k], ref64[k])
        lim = bound(err32)
        log('%s %-4s rel-l2 %.3e  err32 %.3e  bound %.3e' % (tag, k, err, err32, lim))
        if not err <= lim:
            bad.append((k, err, err32, lim))
    assert not bad, (tag, bad)


def test_head_refuses_what_it_does_not_take(M):
    x = torch.zeros((4, 7, 32), device='cuda')
    w, b, t = torch.zeros((3, 32), device='cuda'), torch.zeros(3, device='cuda'), torch.zeros((4, 3), device='cuda')
    with pytest.raises(ValueError, match='7 positions'):
        RO.regress_fwd(torch.zeros((4, 6, 32), device='cuda'), w, b, t)
    with pytest.raises(ValueError, match='one pitch'):
        RO.regress_fwd(x.permute(0, 2, 1)[:, :7, :7], w, b, t)
    with pytest.raises(ValueError, match='target must be'):
        RO.regress_fwd(x, w, b, t[:3])
    with pytest.raises(ValueError, match='1 <= M <= 16'):
        RO.regress_fwd(x, torch.zeros((17, 32), device='cuda'), torch.zeros(17, device='cuda'), torch.zeros((4, 17), device='cuda'))
    feat, out, _ = RO.regress_fwd(x, w, b, t)
    with pytest.raises(ValueError, match='workspace'):
        RO.regress_bwd(feat, w, out, t, RO.MAP, workspace=torch.zeros(8, device='cuda'))
    with pytest.raises(ValueError, match='accumulate needs dparams'):
        RO.regress_bwd(feat, w, out, t, RO.MAP, accumulate=True)


# ---- the whole model against the reference's goldens -------------------------------------------------------------------------------
def _build(M, net, r):
    c = regressor_case(net, r)
    bb = M.resnet18() if net == 'resnet18' else M.densenet18(drop_rate=0.0)
    model = M.CNNRegressor(bb, M_OUT)
    missing = model.load_state_dict({k: torch.from_numpy(v) for k, v in c['params'].items()}, strict=False)
    assert not missing.unexpected_keys
    return model.cuda().train(), c


class tapped(object):
    """The post-ReLU activations the block Functions record (functional.DECISION_TAP): the decisions this forward takes."""

    def __enter__(self):
        from deepards_amd import functional as F_
        F_.DECISION_TAP = []
        return F_.DECISION_TAP

    def __exit__(self, *exc):
        from deepards_amd import functional as F_
        F_.DECISION_TAP = None


_ORACLE = {}


def _oracle(net, r):
    """(float64 oracle, its float32 noise figure) once per case; tests share it and leave it unchanged."""
    if (net, r) not in _ORACLE:
        ref = regressor_oracle(net, r)
        _ORACLE[(net, r)] = (ref, fp32_noise(ref, regressor_oracle(net, r, np.float32)))
    return _ORACLE[(net, r)]


@pytest.mark.parametrize('net,r', [(n, r) for n in ('resnet18', 'densenet18') for r in (6, 5, 46)])
def test_model_matches_the_reference_golden(M, net, r):
    """Output and loss: within 1e-4 of their scale (max |value|) against the reference's float64 capture.  Gradients, every
    parameter: the suite's yardstick (decision_match.assert_gradients_match, unchanged) against the numpy oracle's exact
    gradients under the decisions this run took -- the oracle IS the reference's capture (held here at 1e-9, every tensor)."""
    g = np.load(os.path.join(GOLDEN, 'regressor_r%d_%s.npz' % (r, net)), allow_pickle=False)
    model, c = _build(M, net, r)
    assert list(model.state_dict().keys()) == [str(k) for k in g['keys']]
    x, t = cuda(c['x']), cuda(c['target'])
    with tapped() as taps:
        loss, out = model.forward_loss(x, t)
    loss.backward()
    assert tuple(out.shape) == (r, M_OUT)
    ours_out, ours_loss = out.detach().cpu().numpy().astype(np.float64), float(loss.detach())
    scale = float(np.abs(g['out']).max())
    err_out, err_loss = float(np.abs(ours_out - g['out']).max()) / scale, abs(ours_loss - float(g['loss'][0])) / float(g['loss'][0])
    log('model %s r%d out %.3e of its scale (reference float32: rel-l2 %.3e)  loss %.3e relative (reference float32 %.3e)' %
        (net, r, err_out, float(g['err32/out']), err_loss, float(g['err32/loss'])))
    assert err_out <= FORWARD_BOUND and err_loss <= FORWARD_BOUND
    ref, noise = _oracle(net, r)
    assert np.abs(ref['out'] - g['out']).max() <= 1e-9 * scale
    ours = {}
    for n, p in model.named_parameters():
        key = 'grad/' + n
        if key not in g.files:
            assert p.grad is None, n
            continue
        ours[n] = p.grad.cpu().numpy().astype(np.float64)
        body = slice(None) if p.numel() <= 1024 else slice(0, -3)
        assert np.abs(digest(ref['grads'][n]) - g[key])[body].max() <= 1e-9 * max(1.0, np.abs(g[key][body]).max()), n
    relus = [n for n in ref['tape'].order if ref['tape'].decisions[n]['kind'] == 'relu']
    n_ref = len([k for k in g.files if k.startswith('relu/')])
    assert 0 <= len(relus) - n_ref <= 1                  # (the reference's DenseNet applies its last ReLU as a function: no module call)
    for i, n in enumerate(relus[:n_ref]):                # the oracle takes the reference's decisions
        mask = ref['tape'].decisions[n]['mask']
        assert np.array_equal(np.unpackbits(g['relu/%d' % i])[:mask.size].astype(bool), mask.reshape(-1)), n
    assert_gradients_match(ref, ours, noise, 'regressor %s r%d' % (net, r), log=log, taps=taps)


def test_forward_is_the_head_without_the_loss(M):
    """``forward`` gives forward_loss's output bit for bit, (B, M) also for B = 1, and is differentiable: with the MSE gradient
    handed in as the upstream gradient the parameters get forward_loss's gradients."""
    model, c = _build(M, 'densenet18', 6)
    x, t = cuda(c['x']), cuda(c['target'])
    loss, out = model.forward_loss(x, t)
    loss.backward()
    want = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    model.zero_grad(set_to_none=True)
    plain = model(x, None)
    assert torch.equal(plain.detach(), out)
    plain.backward((2.0 * (plain.detach() - t) / t.numel()))
    for n, p in model.named_parameters():
        if n in want:
            assert R.rel_l2(p.grad.cpu().numpy(), want[n].cpu().numpy()) <= 1e-5, n
    with torch.no_grad():
        assert tuple(model(x[:1], None).shape) == (1, M_OUT) and tuple(model(x[:1]).shape) == (1, M_OUT)


# ---- the trainer ---------------------------------------------------------------------------------------------------------------------
def _trainer(M, optimizer, use_graph, r=6, **kw):
    model, c = _build(M, 'resnet18', r)
    return RegressorTrainer(model, optimizer=optimizer, use_graph=use_graph, **kw), c


@pytest.mark.parametrize('optimizer', ['sgd', 'adam'])
def test_eager_and_captured_steps_give_the_same_parameters(M, optimizer):
    eager, c = _trainer(M, optimizer, False)
    graph, _ = _trainer(M, optimizer, True)
    rng = np.random.RandomState(5)
    for step in range(3):
        x = cuda(c['x'] + 0.01 * rng.randn(*c['x'].shape).astype(np.float32))
        t = cuda(c['target'])
        le, lg = eager.train_step(x, t).clone(), graph.train_step(x, t).clone()
        assert lg.is_cuda and graph.last_loss.is_cuda and torch.equal(le, lg), (step, le, lg)
    assert len(graph._graphs) == 1 and not eager._graphs
    torch.cuda.synchronize()
    for (n, p), (_, q) in zip(eager.model.named_parameters(), graph.model.named_parameters()):
        assert P.same_bits(p.detach(), q.detach()), (n, P.diff_report(p.detach(), q.detach()))
    for a, b in zip(eager.model.buffers(), graph.model.buffers()):
        assert P.same_bits(a, b)
    graph.release_graphs()


def test_tail_batch_gets_its_own_graph_and_test_step_is_a_no_grad_forward(M):
    tr, c = _trainer(M, 'sgd', True)
    x, t = cuda(c['x']), cuda(c['target'])
    for _ in range(3):
        tr.train_step(x, t)
    first = tr._graphs[(6, 1, 224)]
    for _ in range(2):
        tr.train_step(x[:4], t[:4])                                                   # a tail batch of another R
    assert len(tr._graphs) == 2 and tr._graphs[(6, 1, 224)] is first and tr.static_batch(4)[0].shape[0] == 4
    tr.train_step(x, t)
    assert tr._graphs[(6, 1, 224)] is first and tr.steps == 6
    torch.cuda.synchronize()
    grads, params = tr.bucket.g.clone(), tr.bucket.p.clone()
    loss, out = tr.test_step(x, t)
    loss2, out2 = tr.test_step(x, t)                                                  # the replay of the captured test step
    with torch.no_grad():
        want_loss, want_out = tr.model.forward_loss(x, t)
    assert tuple(out.shape) == (6, M_OUT) and tuple(loss.shape) == (1,)
    assert torch.equal(out, want_out) and torch.equal(loss, want_loss) and torch.equal(out2, want_out) and torch.equal(loss2, want_loss)
    assert torch.equal(tr.bucket.g, grads) and torch.equal(tr.bucket.p, params) and tr.model.training
    tr.release_graphs()


def test_loss_falls_on_a_fixed_batch(M):
    """Targets that are a linear function of two waveform statistics (each row's mean and standard deviation)."""
    torch.manual_seed(2)
    model = M.CNNRegressor(M.resnet18(), 3).cuda()
    x = cuda(regressor_case('resnet18', 46)['x'][:16])
    mean, std = x.mean(dim=2), x.std(dim=2)
    t = torch.cat([2.0 * mean + 0.5 * std, mean - std, 0.25 * mean + 3.0 * std], dim=1).contiguous()
    tr = RegressorTrainer(model, optimizer='sgd', learning_rate=1e-3, clip_grad=False)
    losses = [float(tr.train_step(x, t)) for _ in range(20)]
    log('loss over 20 steps on a fixed batch: ' + ' '.join('%.4f' % v for v in losses))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    tr.release_graphs()


# ---- the driver class ----------------------------------------------------------------------------------------------------------------
def _synthetic_store(n, seed, scaling_from=None):
    rng = np.random.RandomState(seed)
    t_ = np.arange(224)[None, :]
    per = rng.uniform(60, 140, (n, 1))
    amp = rng.uniform(20, 60, (n, 1))
    rows = amp * np.sin(2 * np.pi * t_ / per) + rng.randn(n, 224)
    rows[:, 200:] = 0.0                                                               # the zero padding of a padded breath
    stats = np.concatenate([per / 100.0, amp / 40.0], axis=1)
    meta = stats @ rng.randn(2, M_OUT) + 0.05 * rng.randn(n, M_OUT)
    return BreathMetaStore(rows[:, None, :], meta, device='cuda', scaling_from=scaling_from,
                           dataset_type='padded_breath_by_breath_with_full_bm_target'), meta


def test_driver_two_epochs_meters_save_and_second_stage(M, tmp_path):
    from deepards_amd.checkpoint import load_base_network
    from deepards_amd.train import HotPathTrainer
    train, _ = _synthetic_store(64, 0)
    test, test_meta = _synthetic_store(32, 1, scaling_from=train)
    assert test.mu == train.mu and train.padded
    x, t = train.batch(list(range(16)))
    assert tuple(x.shape) == (16, 1, 224) and tuple(t.shape) == (16, M_OUT) and x.dtype == torch.float32
    raw = train.tiles[:16, 0, 0].cpu().numpy()
    want = np.where(raw != 0, raw - train.mu, raw) / train.std                        # padded: mu off non-zero samples only
    assert np.abs(x[:, 0].cpu().numpy() - want).max() <= 1e-6 * np.abs(want).max()
    args = T.make_args(network='cnn_regressor', base_network='densenet18', cuda_no_dp=True, batch_size=16, epochs=2, seed=3,
                       dataset_type='padded_breath_by_breath_with_full_bm_target', train_store=train, test_store=test,
                       save_model='reg.pth', saved_models_dir=str(tmp_path))
    drv = T.CNNRegressorModel(args)
    assert drv.n_bm_features == M_OUT
    drv.train_and_test()
    summary = drv.perform_post_modeling_actions()
    n_test_batches = 2 * 2                                                            # 2 epochs x 32 / 16
    for name in ('test_mae', 'r2', 'test_mse', 'test_loss'):
        assert len(drv.results.get_meter(name, 0)) == n_test_batches, name
        assert np.isfinite(summary['%s/0' % name])
    assert len(drv.results.get_meter('loss', 0)) == 2 * 4
    # the last epoch's predictions against regression_scores recomputed from them
    batches = epoch_index_batches(test, 16, True, drv._epoch_generator(0, 2, 500009), drop_odd=False)
    preds = np.asarray(drv.preds, dtype=np.float64)
    assert preds.shape == (32, M_OUT)
    for k, idx in enumerate(batches):
        tgt = test_meta[idx.numpy()].astype(np.float32)
        mae, r2, mse = T.regression_scores(tgt, preds[16 * k:16 * (k + 1)])
        at = n_test_batches - len(batches) + k
        for name, v in (('test_mae', mae), ('r2', r2), ('test_mse', mse)):
            assert abs(drv.results.get_meter(name, 0)[at] - v) <= 1e-9 * max(1.0, abs(v)), (name, k)
        assert abs(drv.results.get_meter('test_loss', 0)[at] - mse) <= 1e-5 * mse      # MSELoss is the mean over B M: the same figure
    path = os.path.join(str(tmp_path), 'reg.pth')
    bb = load_base_network(path, T.base_networks, {})
    want, got = drv.model.breath_block.state_dict(), bb.state_dict()
    assert list(want) == list(got) and all(torch.equal(want[k].cpu(), got[k]) for k in want)
    # the second stage: a classifier on the pretrained breath block runs a captured step
    clf = M.CNNLinearNetwork(bb, 20, 0).cuda()
    tr = HotPathTrainer(clf)
    xw = torch.randn((2, 20, 1, 224), device='cuda')
    tw = torch.tensor([[1.0, 0.0], [0.0, 1.0]], device='cuda')
    for _ in range(3):
        loss = tr.train_step(xw, tw)
    assert len(tr._graphs) == 1 and bool(torch.isfinite(loss).all())
    tr.release_graphs()
