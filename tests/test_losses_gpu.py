"""GPU tests of the two per-breath loss kernels (da_vacillating_loss / da_confidence_loss, csrc/head_optim.hip) against the
goldens captured from the reference's deepards/loss.py (tests/golden/loss_*.npz; the reference itself is never read here),
their autograd Functions, bit-identical graph replay, and the memory discipline of tests/test_memory_discipline_gpu.py
(same tools, same five checks) for the two new wrappers."""
import glob
import os
import sys
import zlib

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'tools'))
pytestmark = pytest.mark.gpu

import loss_ref  # noqa: E402
from tools import poison as P  # noqa: E402

LOSS_GOLD = sorted(glob.glob(os.path.join(ROOT, 'tests', 'golden', 'loss_*.npz')))


def log(*a):
    print(' '.join(str(x) for x in a))                 # achieved figures: read them with pytest -s


@pytest.fixture(scope='module')
def H():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from deepards_amd import hip_ops
    return hip_ops


def _gold(path):
    z = np.load(path, allow_pickle=False)
    return {k: z[k] for k in z.files}


def _run(H, g, **kw):
    x, t = torch.from_numpy(g['logits']).cuda(), torch.from_numpy(g['target']).cuda()
    if str(g['kind']) == 'vacillating':
        return H.vacillating_loss(x, t, float(g['alpha']), **kw)
    return H.confidence_loss(x, t, float(g['beta']), **kw)


def bounds(g):
    """Per case: 3 x the reference's own fp32-vs-fp64 error (the factor covers another, equally valid fp32 summation
    order), floored at what tests/test_hip_ops_gpu.py holds da_bce_logits to: 1e-6 on the loss, 1e-6 (1 + max|grad|) on
    the gradient."""
    b_loss = max(3.0 * abs(float(g['loss32']) - float(g['loss64'])), 1e-6)
    b_grad = max(3.0 * float(np.abs(g['grad32'].astype(np.float64) - g['grad64']).max()), 1e-6 * (1.0 + float(np.abs(g['grad64']).max())))
    return b_loss, b_grad


@pytest.mark.parametrize('path', LOSS_GOLD, ids=[os.path.basename(p)[:-4] for p in LOSS_GOLD])
def test_kernels_match_the_reference_goldens(H, path):
    g = _gold(path)
    loss, d = _run(H, g)
    got_l, got_d = float(loss.double().cpu()), d.double().cpu().numpy()
    assert np.isfinite(got_l) and np.isfinite(got_d).all()          # alpha = inf included: no NaN, no inf
    assert got_d.shape == g['grad64'].shape
    e_loss, e_grad = abs(got_l - float(g['loss64'])), float(np.abs(got_d - g['grad64']).max())
    b_loss, b_grad = bounds(g)
    log('%-30s loss err %.3e (bound %.3e, reference fp32 %.3e)  grad err %.3e (bound %.3e, reference fp32 %.3e)' %
        (os.path.basename(path)[:-4], e_loss, b_loss, abs(float(g['loss32']) - float(g['loss64'])), e_grad, b_grad,
         float(np.abs(g['grad32'].astype(np.float64) - g['grad64']).max())))
    assert e_loss <= b_loss
    assert e_grad <= b_grad
    # forward-only call: the same loss bits, no gradient; gscale multiplies the gradient only
    loss2, none = _run(H, g, want_grad=False)
    assert none is None and torch.equal(loss2, loss)
    loss3, d3 = _run(H, g, gscale=0.25)
    assert torch.equal(loss3, loss)
    assert np.abs(d3.double().cpu().numpy() - 0.25 * got_d).max() <= 1e-7 * np.abs(got_d).max()


def test_wrappers_refuse_what_the_kernels_do_not_define(H):
    x2, t = torch.randn(8, 2, device='cuda'), torch.eye(2, device='cuda').repeat(4, 1)
    with pytest.raises(ValueError, match='per-breath outputs'):
        H.vacillating_loss(x2, t, 2.0)
    with pytest.raises(ValueError, match='alpha must be > 0'):
        H.vacillating_loss(torch.randn(8, 5, 2, device='cuda'), t, 0.0)
    with pytest.raises(ValueError):
        H.confidence_loss(torch.randn(8, 5, 2, device='cuda'), t[:4], 1.0)
    with pytest.raises(ValueError):
        H.confidence_loss(torch.randn(8, 5, 3, device='cuda'), t, 1.0)


@pytest.mark.parametrize('shape', [(64, 20, 2), (3, 70, 2), (130, 1, 2)])
def test_kernels_match_the_oracle_on_other_shapes(H, shape):
    """More windows than waves, more breaths than lanes, one breath: against tests/tools/loss_ref.py (pinned to the goldens
    by tests/test_losses_cpu.py) at the da_bce_logits bound."""
    rng = np.random.RandomState(sum(shape))
    x = (rng.standard_normal(shape) + rng.choice([-1.0, 1.0], size=(shape[0], 1, 1)) * np.array([-0.8, 0.8])).astype(np.float32)
    t = np.eye(2, dtype=np.float32)[rng.randint(0, 2, shape[0])]
    xs, ts = torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda()
    runs = [('confidence', H.confidence_loss(xs, ts, 0.5), loss_ref.confidence(x, t, 0.5))]
    if np.abs(loss_ref.class_means(x) - 0.5).min() >= 1e-3:
        for alpha in (float('inf'), 1.0):
            runs.append(('vacillating %g' % alpha, H.vacillating_loss(xs, ts, alpha), loss_ref.vacillating(x, t, alpha)))
    assert len(runs) == 3 or shape[1] == 1
    for name, (loss, d), (rl, rd) in runs:
        e_l, e_d = abs(float(loss.double().cpu()) - rl), np.abs(d.double().cpu().numpy() - rd).max()
        log('%s %s: loss err %.3e grad err %.3e' % (name, shape, e_l, e_d))
        assert e_l <= 1e-6 * (1 + abs(rl)) and e_d <= 1e-6 * (1 + np.abs(rd).max())


def test_functions_honour_the_incoming_gradient_scale(H):
    from deepards_amd import functional as F_
    g = _gold(os.path.join(ROOT, 'tests', 'golden', 'loss_vac_a2_4x20.npz'))
    t = torch.from_numpy(g['target']).cuda()
    for crit, op in ((F_.VacillatingLoss(2.0), lambda x: H.vacillating_loss(x, t, 2.0)),
                     (F_.ConfidencePenaltyLoss(0.25), lambda x: H.confidence_loss(x, t, 0.25))):
        x = torch.from_numpy(g['logits']).cuda().requires_grad_(True)
        loss = crit(x, t)
        ref_loss, ref_d = op(x.detach())
        assert loss.dim() == 0 and torch.equal(loss.detach().view(1), ref_loss)
        (2.5 * loss).backward()
        assert torch.equal(x.grad, ref_d * 2.5)
        # the reference's calling convention: the target already repeated over the breaths
        x2 = torch.from_numpy(g['logits']).cuda().requires_grad_(True)
        loss2 = crit(x2, t.unsqueeze(1).repeat(1, x2.shape[1], 1))
        assert torch.equal(loss2, loss)


def test_graph_replays_are_bit_identical(H):
    g = _gold(os.path.join(ROOT, 'tests', 'golden', 'loss_vac_ainf_4x20.npz'))
    x, t = torch.from_numpy(g['logits']).cuda(), torch.from_numpy(g['target']).cuda()
    eager = [H.vacillating_loss(x, t, float('inf')), H.confidence_loss(x, t, 1.0)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        H.vacillating_loss(x, t, float('inf'))
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = [H.vacillating_loss(x, t, float('inf')), H.confidence_loss(x, t, 1.0)]
    seen = []
    for _ in range(2):
        for o in out:
            for q in o:
                q.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        seen.append([q.clone() for o in out for q in o])
    for a, b in zip(seen[0], seen[1]):
        assert torch.equal(a, b)
    for a, b in zip(seen[0], [q for o in eager for q in o]):
        assert torch.equal(a, b)


# ---- memory discipline: the five checks of tests/test_memory_discipline_gpu.py for the two wrappers --------------------------
def _cases():
    from deepards_amd import hip_ops as H_
    cases = []
    for w, nb in ((4, 20), (1, 20), (64, 20), (37, 1), (3, 70)):
        name = 'breath_losses_w%d_nb%d' % (w, nb)

        def build(w=w, nb=nb, name=name):
            gen = torch.Generator().manual_seed(zlib.crc32(name.encode()))
            x = torch.randn(w, nb, 2, generator=gen)
            x[:, :, 1] += torch.where(torch.arange(w) % 2 == 0, 0.9, -0.9)[:, None]     # class means away from 0.5
            t = torch.zeros(w, 2)
            t[torch.arange(w), torch.arange(w) % 2] = 1
            return dict(logits=x.cuda(), target=t.cuda())

        def call(logits, target, nb=nb):
            vac = H_.vacillating_loss(logits, target, 2.0) if nb > 1 else None
            vac_inf = H_.vacillating_loss(logits, target, float('inf')) if nb > 1 else None
            flat = logits if nb > 1 else logits.view(-1, 2)
            return dict(conf=H_.confidence_loss(flat, target, 0.5), conf_fwd=H_.confidence_loss(flat, target, 0.5, want_grad=False)[0],
                        vac=vac, vac_inf=vac_inf)
        rows = None
        if w >= 2:
            rows = dict(inputs=('logits',), R=1, windows=w, mid=w // 2,
                        axis={'conf[0]': None, 'conf_fwd': None, 'vac[0]': None, 'vac_inf[0]': None})
        cases.append(P.OpCase(name, 'breath_loss', build, call, rows=rows,
                              note='the losses reduce over the batch (exempt from check 4); a window\'s gradient depends on its '
                                   'own logits only; the wrappers allocate their results: check 3 has no destination to dirty'))
    return cases


CASES = _cases() if torch.cuda.is_available() else []


@pytest.mark.parametrize('check', ['uninitialised', 'guards', 'isolation', 'repeat'])
def test_loss_wrappers_memory_discipline(H, check):
    assert len(CASES) == 5
    problems = []
    for i, c in enumerate(CASES):
        problems += P.run_check(check, c, other=CASES[(i + 1) % len(CASES)])
    assert not problems, '\n'.join(problems)
