"""GPU tests of the siamese pretraining kernels (csrc/siamese.hip, deepards_amd/siamese_ops.py): the triplet draw bit for bit
against its numpy restatement, the head's forward and backward against the float64 oracle of tests/siamese_ref.py within the
componentwise bound |got - ref| <= 4 (n + 2) 2^-24 S, run-to-run bit identity, poisoned outputs and guard bands.

The backward is judged as the kernel it is: the oracle's gradients are taken from the u and z the forward KERNEL produced (its
inputs), so the forward's own rounding is not booked twice.  Every figure is printed before it is asserted."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

from tools import poison as P                                                       # noqa: E402
import siamese_ref as R                                                             # noqa: E402

if torch.cuda.is_available():
    from deepards_amd import _lib, hip_ops as H, siamese_ops as SO
else:                                   # collected without a GPU (-m "not gpu" deselects every test of this file)
    _lib = H = SO = None

COUNTS = [2, 3, 2, 5, 4]                # windows per patient of the draw fixture, N = 16


def cu(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


# ---- the draw ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('literal', [0, 1])
@pytest.mark.parametrize('b', [1, 16])
def test_draw_equals_the_numpy_restatement(b, literal):
    ps, pc, pat = R.patient_tables(COUNTS)
    n = len(ps)
    anchors = np.arange(n, dtype=np.int64)[:b] if b == n else np.array([n - 1], dtype=np.int64)
    dps, dpc, da = cu(ps, pc, anchors)
    for seed in (1234, 0xdeadbeef):
        for step in (0, 7, 255, 2 ** 31, 2 ** 32 - 1):
            got = SO.siamese_draw(da, dps, dpc, seed, step, literal).cpu().numpy()
            ref = R.draw(anchors, ps, pc, seed, step, literal)
            assert got.dtype == np.int64 and np.array_equal(got, ref), (seed, step, got, ref)
            neg = got[-b:]
            assert (pat[neg] != pat[anchors]).all() and (got >= 0).all() and (got < n).all()


def test_draw_refusals_and_guard_bands():
    ps, pc, _ = R.patient_tables(COUNTS)
    dps, dpc, da = cu(ps, pc, np.arange(16, dtype=np.int64))
    lib, st = _lib.lib(), H._stream()
    out = P.fill_poison(torch.empty(64, dtype=torch.int64, device='cuda'))
    assert lib.da_siamese_draw(_ptr(da), _ptr(dps), _ptr(dpc), _ptr(out), 16, 1, 1, 0, 1, st) == -1          # N < 2
    assert lib.da_siamese_draw(_ptr(da), _ptr(dps), _ptr(dpc), _ptr(out), 0, 16, 1, 0, 1, st) == -1          # B < 1
    for hole in range(4):
        args = [_ptr(da), _ptr(dps), _ptr(dpc), _ptr(out)]
        args[hole] = None
        assert lib.da_siamese_draw(*args, 16, 16, 1, 0, 1, st) == -1
    torch.cuda.synchronize()
    assert P.count_poison(out) == out.numel()
    with pytest.raises(ValueError):
        SO.siamese_draw(da, dps[:1], dpc[:1], 1, 0, True)
    for literal, width in ((1, 64), (0, 48)):
        handles = []
        views = []
        for t in (da, dps, dpc, torch.zeros(width, dtype=torch.int64, device='cuda')):
            v, hd = P.guarded(t)
            handles.append(hd)
            views.append(v)
        P.fill_poison(views[3])
        assert lib.da_siamese_draw(*[_ptr(v) for v in views], 16, 16, 1234, 3, literal, st) == 0
        torch.cuda.synchronize()
        P.assert_guards_intact(handles)
        assert not P.has_poison(views[3])
        assert np.array_equal(views[3].cpu().numpy(), R.draw(np.arange(16), ps, pc, 1234, 3, literal))


# ---- the head ---------------------------------------------------------------------------------------------------------------
def head_batches(nb):
    """B = 1, 3 and the values that put B NB one below, at and one above the row kernels' block (where NB divides them)."""
    rpb = SO.head_rows_per_block()
    edge = {r // nb for r in (rpb - 1, rpb, rpb + 1, 2 * rpb, 2 * rpb + 1) if r % nb == 0 and r >= nb}
    return sorted({1, 3} | edge)


def run_head(case, b, nb, shared, accumulate=False, prior=None, gscale=1.0):
    d = {k: (torch.from_numpy(v).cuda() if isinstance(v, np.ndarray) else v) for k, v in case.items()}
    fa_neg = d['fa_pos'] if shared else d['fa_neg']
    ops = (d['fa_pos'], d['fc_pos'], fa_neg, d['fc_neg'])
    params = (d['W1'], d['b1'], d['W2'], d['b2'])
    u, z, loss = SO.siamese_head_fwd(*ops, *params, b, nb)
    dparams = None
    if accumulate:
        dparams = tuple(p.clone() for p in prior)
    grads, dparams = SO.siamese_head_bwd(*ops, *params, u, z, b, nb, dparams=dparams, accumulate=accumulate, gscale=gscale)
    return u, z, loss, grads, dparams


def check(name, got, ref, n, S, extra_S=0.0):
    got = np.asarray(got, dtype=np.float64)
    tol = R.bound(n, np.asarray(S) + extra_S)
    err = np.abs(got - ref)
    worst = float((err / np.maximum(tol, 1e-300)).max()) if err.size else 0.0
    print('%-8s n %5d  max err %.3e  max err / bound %.3f' % (name, n, float(err.max()), worst))
    assert np.isfinite(got).all(), name
    assert (err <= tol).all(), '%s: %d elements outside the bound, worst ratio %.3f' % (name, int((err > tol).sum()), worst)


@pytest.mark.parametrize('shared', [False, True])
@pytest.mark.parametrize('nb', [1, 2, 20, 33])
@pytest.mark.parametrize('d', [1, 63, 64, 65, 512, 1000])
def test_head_against_the_float64_oracle(d, nb, shared):
    for b in head_batches(nb):
        case = R.make_case(b, nb, d, shared)
        ns = R.sum_lengths(b, nb, d, shared)
        print('B %d NB %d D %d shared %s' % (b, nb, d, shared))
        for accumulate in (False, True):
            prior = cu(*[np.random.RandomState(5).randn(*case[k].shape).astype(np.float32) for k in ('W1', 'b1', 'W2', 'b2')])
            u, z, loss, grads, dparams = run_head(case, b, nb, shared, accumulate, prior, gscale=0.5 if accumulate else 1.0)
            fwd = R.head_forward(case['fa_pos'], case['fc_pos'], case['fa_neg'], case['fc_neg'], case['W1'], case['b1'], case['W2'],
                                 case['b2'], b, nb)
            p, w = case['big']
            assert np.abs(fwd['z'][p, w]).min() > 40                                 # the saturated pair is in the case
            if not accumulate:
                check('u', u.cpu().numpy(), fwd['u'], ns['u'], fwd['S_u'])
                check('z', z.cpu().numpy(), fwd['z'], ns['z'], fwd['S_z'])
                check('loss', loss.cpu().numpy()[0], fwd['loss'], ns['loss'], fwd['S_loss'])
            bwd = R.head_backward(case['fa_pos'], case['fc_pos'], case['fa_neg'], case['fc_neg'], case['W1'], case['W2'],
                                  u.cpu().numpy(), z.cpu().numpy(), b, nb, shared, gscale=0.5 if accumulate else 1.0)
            for name, g in zip(('dfa_pos', 'dfc_pos', 'dfa_neg', 'dfc_neg'), grads):
                if g is None:
                    assert shared and name == 'dfa_neg'
                    continue
                check(name, g.cpu().numpy(), bwd[name], ns[name], bwd['S_' + name])
            equal = case['fc_pos'] == case['fa_pos']                                    # fc == fa: exactly zero, not NaN
            assert equal.any() and (grads[1].cpu().numpy()[equal] == 0).all()
            for name, g, pr in zip(('dW1', 'db1', 'dW2', 'db2'), dparams, prior):
                before = pr.cpu().numpy().astype(np.float64) if accumulate else 0.0
                check(name, g.cpu().numpy(), bwd[name] + before, ns[name] + (1 if accumulate else 0), bwd['S_' + name],
                      np.abs(before))


@pytest.mark.parametrize('shared', [False, True])
@pytest.mark.parametrize('b,nb,d', [(3, 20, 512), (9, 1, 65), (2, 33, 16)])
def test_head_runs_are_bit_identical_and_need_no_initialised_memory(b, nb, d, shared):
    case = R.make_case(b, nb, d, shared, seed=1)
    first = run_head(case, b, nb, shared)
    second = run_head(case, b, nb, shared)
    with P.poisoned_allocations() as stats:
        third = run_head(case, b, nb, shared)
    assert stats.filled > 0
    flat = lambda r: [r[0], r[1], r[2]] + [g for g in r[3] if g is not None] + list(r[4])
    for x, y, w in zip(flat(first), flat(second), flat(third)):
        assert P.same_bits(x, y) and P.same_bits(x, w) and not P.has_poison(w)


@pytest.mark.parametrize('shared', [False, True])
@pytest.mark.parametrize('b,nb,d', [(3, 3, 64), (1, 7, 65), (2, 20, 512)])
def test_head_guard_bands_stay_intact(b, nb, d, shared):
    """Operands (row slices of one tensor, as the model passes them), parameters, outputs, gradient slices and the workspace
    inside pattern-filled guard bands, the outputs pre-filled with the pattern: the plain call's bits, no guard word changed,
    no pattern left in an output."""
    lib, st = _lib.lib(), H._stream()
    case = R.make_case(b, nb, d, shared, seed=2)
    plain = run_head(case, b, nb, shared)
    rows = b * nb
    handles = []

    def gd(t):
        v, hd = P.guarded(t)
        handles.append(hd)
        return v
    names = ('fa_pos', 'fc_pos', 'fc_neg') if shared else ('fa_pos', 'fc_pos', 'fa_neg', 'fc_neg')
    feats = gd(torch.from_numpy(np.concatenate([case[k] for k in names])).cuda())
    sl = [feats[i * rows:(i + 1) * rows] for i in range(len(names))]
    ops = (sl[0], sl[1], sl[0], sl[2]) if shared else tuple(sl)
    w1, b1, w2, b2 = [gd(t) for t in cu(case['W1'], case['b1'], case['W2'], case['b2'])]
    u, z, loss = gd(torch.zeros(2, rows, 2).cuda()), gd(torch.zeros(2, b, 2).cuda()), gd(torch.zeros(1).cuda())
    dfeats = gd(torch.zeros_like(feats))
    gs = [dfeats[i * rows:(i + 1) * rows] for i in range(len(names))]
    grads = (gs[0], gs[1], None, gs[2]) if shared else tuple(gs)
    dps = [gd(torch.zeros_like(t)) for t in (w1, b1, w2, b2)]
    work = gd(torch.zeros(lib.da_siamese_head_bwd_workspace(b, nb, d) // 4, device='cuda'))
    for t in (u, z, loss, dfeats, work) + tuple(dps):
        P.fill_poison(t)
    assert lib.da_siamese_head_fwd(*[_ptr(t) for t in ops], d, _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(u), _ptr(z),
                                   _ptr(loss), b, nb, d, st) == 0
    assert lib.da_siamese_head_bwd(*[_ptr(t) for t in ops], d, _ptr(w1), _ptr(w2), _ptr(u), _ptr(z), *[_ptr(t) for t in grads], d,
                                   *[_ptr(t) for t in dps], _ptr(work), 1.0, 0, b, nb, d, st) == 0
    torch.cuda.synchronize()
    P.assert_guards_intact(handles)
    got = [u, z, loss] + [g for g in grads if g is not None] + dps
    want = [plain[0], plain[1], plain[2]] + [g for g in plain[3] if g is not None] + list(plain[4])
    for x, y in zip(got, want):
        assert not P.has_poison(x) and P.same_bits(x.contiguous(), y.contiguous())


def test_head_refusals_touch_nothing():
    lib, st = _lib.lib(), H._stream()
    f = torch.randn(4, 8).cuda()
    w1, b1, w2, b2 = torch.randn(2, 8).cuda(), torch.randn(2).cuda(), torch.randn(2, 4).cuda(), torch.randn(2).cuda()
    outs = [P.fill_poison(torch.empty(n).cuda()) for n in (64, 64, 64, 64, 64)]
    u, z, loss, g, work = outs
    for b, nb, d, ld in ((0, 2, 8, 8), (2, 0, 8, 8), (2, 2, 0, 8), (2, 2, 8, 4)):
        assert lib.da_siamese_head_fwd(_ptr(f), _ptr(f), _ptr(f), _ptr(f), ld, _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(u),
                                       _ptr(z), _ptr(loss), b, nb, d, st) == -1
        assert lib.da_siamese_head_bwd(_ptr(f), _ptr(f), _ptr(f), _ptr(f), ld, _ptr(w1), _ptr(w2), _ptr(u), _ptr(z), _ptr(g),
                                       _ptr(g), None, _ptr(g), 8, _ptr(g), _ptr(g), _ptr(g), _ptr(g), _ptr(work), 1.0, 0, b, nb, d,
                                       st) == -1
    assert lib.da_siamese_head_fwd(None, _ptr(f), _ptr(f), _ptr(f), 8, _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(u), _ptr(z),
                                   _ptr(loss), 2, 2, 8, st) == -1
    assert lib.da_siamese_head_bwd_workspace(0, 2, 8) == 0
    torch.cuda.synchronize()
    for o in outs:
        assert P.count_poison(o) == o.numel()
    with pytest.raises(ValueError):
        SO.siamese_head_fwd(f, f, f, f, w1, b1, torch.randn(2, 6).cuda(), b2, 2, 2)


# ================================================================================================================================
# models: the one-pass triplet path against the eager composition and a float64 restatement
# ================================================================================================================================
KINDS = ('linear', 'lstm', 'transformer')


def build(kind, base, nb, drop=0.0, seed=5, tfm_dropout=0.0):
    from deepards_amd import models as M
    torch.manual_seed(seed)
    bb = M.resnet18() if base == 'resnet18' else M.densenet18(drop_rate=drop)
    if kind == 'linear':
        model = M.SiameseCNNLinearNetwork(bb, nb)
    elif kind == 'lstm':
        model = M.SiameseCNNLSTMNetwork(bb, 8, nb)
    else:
        model = M.SiameseCNNTransformerNetwork(bb, 16, nb)
        for blk in model.transformer.blocks:
            blk.dropout = tfm_dropout
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():                                   # BatchNorm affine parameters away from 1 / 0, a livelier head
        for n, p in model.named_parameters():
            if ('norm' in n or 'bn' in n) and p.dim() == 1:
                p.copy_(torch.rand(p.shape, generator=g) + 0.5 if n.endswith('weight') else torch.randn(p.shape, generator=g) * 0.1)
        model.linear_intermediate.weight.mul_(4.0)
    return model.cuda().train()


def triplet_windows(b, nb, seed=0):
    g = torch.Generator().manual_seed(100 + seed + 10 * b + nb)
    seq, pos, neg = (torch.randn(b, nb, 1, 224, generator=g).cuda() for _ in range(3))
    return seq, pos, neg


def grads_of(model):
    return {n: p.grad.detach().double().cpu().numpy() for n, p in model.named_parameters() if p.grad is not None}


def fused_run(kind, base, b, nb, literal):
    model = build(kind, base, nb)
    seq, pos, neg = triplet_windows(b, nb)
    batch = torch.cat([seq, pos, seq, neg] if literal else [seq, pos, neg], dim=0)
    loss, zp, zn = model.forward_triplet(batch, literal=literal)
    loss.backward()
    torch.cuda.synchronize()
    return dict(loss=float(loss.detach()), z=torch.stack([zp, zn]).detach().double().cpu().numpy(), grads=grads_of(model)), model


_EAGER, _REF64 = {}, {}


def eager_run(kind, base, b, nb):
    """The reference's training body on this package's modules: model(seq, pos), model(seq, neg), stock BCE, autograd."""
    key = (kind, base, b, nb)
    if key not in _EAGER:
        model = build(kind, base, nb)
        seq, pos, neg = triplet_windows(b, nb)
        zp, zn = model(seq, pos), model(seq, neg)
        crit = torch.nn.BCEWithLogitsLoss()
        loss = crit(zp, torch.tensor([[0.0, 1.0]]).cuda().repeat(b, 1)) + crit(zn, torch.tensor([[1.0, 0.0]]).cuda().repeat(b, 1))
        loss.backward()
        torch.cuda.synchronize()
        _EAGER[key] = dict(loss=float(loss.detach()), z=torch.stack([zp, zn]).detach().double().cpu().numpy(), grads=grads_of(model))
    return _EAGER[key]


def _torch_block(x, P):
    """One Block of models/transformer.py in stock torch (no dropout); the second residual adds the block INPUT."""
    wq, bq, wk, bk, wv, bv, wj, bj, g1, be1, w0, b0, w2, b2, g2, be2 = P
    B, T, D = x.shape
    hd = wq.shape[0]
    hs = hd // 4
    lin = torch.nn.functional.linear
    split = lambda a: a.reshape(B, T, 4, hs).transpose(1, 2)
    q, k, v = split(lin(x, wq, bq)), split(lin(x, wk, bk)), split(lin(x, wv, bv))
    w = torch.softmax(q @ k.transpose(-1, -2) / (hs ** 0.5), dim=-1)
    joint = lin((w @ v).transpose(1, 2).reshape(B, T, hd), wj, bj)
    att = torch.nn.functional.layer_norm(joint + x, (D,), g1, be1, 1e-5)
    f = lin(torch.relu(lin(att, w0, b0)), w2, b2)
    return torch.nn.functional.layer_norm(f + x, (D,), g2, be2, 1e-5)


def ref64_run(kind, base, b, nb):
    """The same network in float64 stock torch on the CPU: oracle.torch_ref's breath block window by window, nn-functional time
    layer and head.  -> loss, z, parameter gradients, and the head term of the tolerance (see the test)."""
    key = (kind, base, b, nb)
    if key in _REF64:
        return _REF64[key]
    from oracle import torch_ref
    model = build(kind, base, nb).cpu()
    p = {n: q.detach().double().requires_grad_(True) for n, q in model.named_parameters()}
    seq, pos, neg = (t.cpu().double() for t in triplet_windows(b, nb))
    block = torch_ref.resnet18_block if base == 'resnet18' else torch_ref.densenet18_block

    def tower(x):
        feat = torch.cat([block(p, x[i]) for i in range(x.shape[0])], dim=0)          # (B NB, F), BatchNorm per window
        if kind == 'lstm':
            lstm = torch.nn.LSTM(feat.shape[1], 8, batch_first=True).double()
            names = ('weight_ih_l0', 'weight_hh_l0', 'bias_ih_l0', 'bias_hh_l0')
            out = torch.func.functional_call(lstm, {n: p['lstm.' + n] for n in names}, (feat.view(x.shape[0], nb, -1),))[0]
            return out.reshape(x.shape[0] * nb, -1)
        if kind == 'transformer':
            from tools.transformer_ref import PARAM_NAMES
            y = feat.view(x.shape[0], nb, -1)
            for i in (0, 1):
                y = _torch_block(y, [p['transformer.blocks.%d.%s' % (i, n)] for n in PARAM_NAMES])
            return y.reshape(x.shape[0] * nb, -1)
        return feat
    fa, fp, fn = tower(seq), tower(pos), tower(neg)
    for t in (fa, fp, fn):
        t.retain_grad()
    lin = torch.nn.functional.linear
    head = lambda a, c: lin(lin(torch.abs(c - a), p['linear_intermediate.weight'], p['linear_intermediate.bias']).view(b, -1),
                            p['linear_final.weight'], p['linear_final.bias'])
    zp, zn = head(fa, fp), head(fa, fn)
    crit = torch.nn.BCEWithLogitsLoss()
    loss = crit(zp, torch.tensor([[0.0, 1.0]]).double().repeat(b, 1)) + crit(zn, torch.tensor([[1.0, 0.0]]).double().repeat(b, 1))
    loss.backward()
    # the head's own float32 error at these operands, from the oracle of the kernel tests (shared-anchor form: the wider sums)
    num = lambda t: t.detach().numpy()
    W1, b1, W2, b2 = (num(p[n]) for n in ('linear_intermediate.weight', 'linear_intermediate.bias', 'linear_final.weight',
                                          'linear_final.bias'))
    d = fa.shape[1]
    fwd = R.head_forward(num(fa), num(fp), num(fa), num(fn), W1, b1, W2, b2, b, nb)
    bwd = R.head_backward(num(fa), num(fp), num(fa), num(fn), W1, W2, fwd['u'], fwd['z'], b, nb, True)
    ns = R.sum_lengths(b, nb, d, True)
    # forward: the z bound also carries u's (its input) -- bound(D, S_u) pushed through |W2|
    z_tol = R.bound(ns['z'], fwd['S_z']) + (R.bound(ns['u'], fwd['S_u']).reshape(2, b, 2 * nb) @ np.abs(W2).T)
    dfeat_tol = np.sqrt(sum(float((R.bound(ns[k], bwd['S_' + k]) ** 2).sum()) for k in ('dfa_pos', 'dfc_pos', 'dfc_neg')))
    dfeat_norm = np.sqrt(sum(float((num(t.grad) ** 2).sum()) for t in (fa, fp, fn)))
    out = dict(loss=float(loss.detach()), z=np.stack([num(zp), num(zn)]), grads={n: num(q.grad) for n, q in p.items() if q.grad is not None},
               z_tol=z_tol, loss_tol=float(R.bound(ns['loss'], fwd['S_loss'])) + float(z_tol.sum()) / (2 * b),
               feat_rel=dfeat_tol / dfeat_norm,
               head_tol={'linear_intermediate.weight': R.bound(ns['dW1'], bwd['S_dW1']),
                         'linear_intermediate.bias': R.bound(ns['db1'], bwd['S_db1']),
                         'linear_final.weight': R.bound(ns['dW2'], bwd['S_dW2']), 'linear_final.bias': R.bound(ns['db2'], bwd['S_db2'])})
    _REF64[key] = out
    return out


def rel(a, ref):
    n = float(np.linalg.norm(ref))
    return float(np.linalg.norm(np.asarray(a, dtype=np.float64) - ref)) / (n if n > 0 else 1.0)


@pytest.mark.parametrize('literal', [True, False])
@pytest.mark.parametrize('b,nb', [(2, 4), (3, 2)])
@pytest.mark.parametrize('base', ['resnet18', 'densenet18'])
@pytest.mark.parametrize('kind', KINDS)
def test_forward_triplet_against_the_eager_composition_and_float64(kind, base, b, nb, literal):
    """Both paths are measured against the float64 network; the one-pass path may be at most twice as far from it as the eager
    composition, plus the head kernels' own bound at these operands:
      logits  componentwise, + bound(2 NB, S_z) with u's bound pushed through |W2|
      loss    + bound(4 B, S_loss) and the logits' term averaged
      head parameters' gradients  componentwise, + their bound of the kernel tests
      every other gradient  in relative l2 over the tensor, + ||bound(dfeat)|| / ||dfeat||: they are linear in the gradient the
                            head hands the tower, so that is the relative perturbation the head's rounding can cause."""
    fused, _ = fused_run(kind, base, b, nb, literal)
    eager, ref = eager_run(kind, base, b, nb), ref64_run(kind, base, b, nb)
    dz_f, dz_e = np.abs(fused['z'] - ref['z']), np.abs(eager['z'] - ref['z'])
    dl_f, dl_e = abs(fused['loss'] - ref['loss']), abs(eager['loss'] - ref['loss'])
    print('%s %s B %d NB %d literal %s: logits fused %.3e eager %.3e | loss fused %.3e eager %.3e (loss %.6f)' %
          (kind, base, b, nb, literal, dz_f.max(), dz_e.max(), dl_f, dl_e, ref['loss']))
    assert (dz_f <= 2 * dz_e.max() + ref['z_tol']).all()
    assert dl_f <= 2 * dl_e + ref['loss_tol']
    assert set(fused['grads']) == set(eager['grads']) == set(ref['grads'])
    worst = (0.0, 0.0, '')
    gmax = max(float(np.linalg.norm(g)) for n, g in ref['grads'].items() if n not in ref['head_tol'])
    for n, g64 in ref['grads'].items():
        if n in ref['head_tol']:
            ef, ee = np.abs(fused['grads'][n] - g64), np.abs(eager['grads'][n] - g64)
            assert (ef <= 2 * ee.max() + ref['head_tol'][n]).all(), n
            continue
        if float(np.linalg.norm(g64)) < 1e-9 * gmax:
            # a gradient that is zero in exact arithmetic (a key bias: softmax does not see it; the last ff_norm.bias: it cancels
            # in compr - x): float32 leaves the rounding of its cancelling terms, judged in absolute l2 at the largest gradient's scale
            nf, ne = float(np.linalg.norm(fused['grads'][n] - g64)), float(np.linalg.norm(eager['grads'][n] - g64))
            assert nf <= 2 * ne + ref['feat_rel'] * gmax, '%s (zero): fused %.3e eager %.3e, scale %.3e' % (n, nf, ne, gmax)
            continue
        rf, re_ = rel(fused['grads'][n], g64), rel(eager['grads'][n], g64)
        worst = max(worst, (rf, re_, n))
        assert rf <= 2 * re_ + ref['feat_rel'], '%s: fused %.3e eager %.3e head term %.3e' % (n, rf, re_, ref['feat_rel'])
    print('    worst tower gradient rel-l2: fused %.3e eager %.3e (%s), head term %.3e' % (worst + (ref['feat_rel'],)))


def test_literal_form_moves_the_running_statistics_like_the_four_calls():
    """resnet18, literal form: BatchNorm's running statistics and num_batches_tracked after the one 4 B-window pass against
    those after model(seq, pos), model(seq, neg) -- the reference's order seq, pos, seq, neg, window by window.  BIT equality:
    the update of the windows of one pass is a closed form (csrc/bn.hip, bn_running_multi_kernel), so ONE update over 4 B
    windows would agree with two over 2 B only to rounding (measured without the grouping: up to 2 ulp at a buffer's largest
    magnitude); the literal pass therefore books one update per call it stands for (functional.running_update_groups), and a
    window's batch statistics do not depend on the windows beside it."""
    b, nb = 2, 4
    seq, pos, neg = triplet_windows(b, nb)
    one, four = build('linear', 'resnet18', nb), build('linear', 'resnet18', nb)
    with torch.no_grad():
        one.forward_triplet(torch.cat([seq, pos, seq, neg], dim=0), literal=True)
        four(seq, pos)
        four(seq, neg)
    torch.cuda.synchronize()
    bufs_one, bufs_four = dict(one.named_buffers()), dict(four.named_buffers())
    moved = tracked = 0
    for n, v in bufs_one.items():
        if n.endswith('num_batches_tracked'):
            assert int(v) == int(bufs_four[n]), n
            tracked = max(tracked, int(v))
            continue
        diff = float((v.double() - bufs_four[n].double()).abs().max())
        if diff:
            print('%s differs by %.3e = %.2f ulp at its largest magnitude' % (n, diff, diff / float(np.spacing(np.float32(
                v.abs().max().item())))))
        assert P.same_bits(v, bufs_four[n]), n
        moved += int(n.endswith('running_mean') and bool((v != 0).any()))
    assert moved > 10 and tracked > 0


# ================================================================================================================================
# the store on the device, the trainer, the driver
# ================================================================================================================================
def synthetic_store(n_patients=4, per=3, nb=2, seed=0, **kw):
    from deepards_amd.siamese import SiameseTileStore
    rng = np.random.RandomState(seed)
    n = n_patients * per
    w = rng.randn(n, nb, 1, 224) * 3.0 + 1.0
    pats = np.repeat(np.arange(n_patients), per)[rng.permutation(n)]
    return SiameseTileStore(w, pats, **kw), w, pats


@pytest.mark.parametrize('literal', [True, False])
def test_triplet_batch_is_the_draw_then_the_gather(literal):
    store, w, pats = synthetic_store(seed=3)
    anchors = [0, 5, 11, 2]
    batch, idx = store.triplet_batch(anchors, step=9, literal=literal)
    ps, pc = store.pat_start.cpu().numpy(), store.pat_count.cpu().numpy()
    want = R.draw(np.array(anchors), ps, pc, store.seed, 9, literal)
    assert np.array_equal(idx.cpu().numpy(), want) and batch.shape == (len(want), 2, 1, 224)
    tiles = w[store.original_index]
    ref = ((tiles[want] - store.mu) / store.std).astype(np.float32)
    assert np.allclose(batch.cpu().numpy(), ref, rtol=1e-6, atol=1e-6)               # (the gather's bits are pinned by its own tests)
    sorted_pats = store.patients
    neg = want[-4:]
    assert (sorted_pats[neg] != sorted_pats[anchors]).all() and (sorted_pats[want[4:8]] == sorted_pats[anchors]).all()
    dev = store.anchors_on_device(anchors)
    again, idx2 = store.triplet_batch(dev, step=9, literal=literal, out=torch.empty_like(batch))
    assert torch.equal(again, batch) and torch.equal(idx2, idx) and store.draws == 2


def trainer_of(kind, base, nb, share, use_graph, drop=0.2, optimizer='sgd'):
    from deepards_amd.siamese import SiameseTrainer
    return SiameseTrainer(build(kind, base, nb, drop=drop, tfm_dropout=0.2), share_anchor=share, use_graph=use_graph,
                          optimizer=optimizer)


@pytest.mark.parametrize('kind,base,share,optimizer', [('linear', 'densenet18', False, 'sgd'), ('linear', 'resnet18', True, 'adam'),
                                                       ('lstm', 'densenet18', True, 'sgd'), ('transformer', 'resnet18', False, 'sgd')])
def test_five_eager_steps_equal_five_captured_steps(kind, base, share, optimizer):
    store, _, _ = synthetic_store(seed=1)
    batches = [store.triplet_batch([i, i + 3, i + 6], step=i, literal=not share)[0] for i in range(5)]
    runs = []
    for use_graph in (False, True):
        tr = trainer_of(kind, base, 2, share, use_graph, optimizer=optimizer)
        start = [p.detach().clone() for p in tr.model.parameters()]
        losses = torch.cat([tr.train_step(x).clone() for x in batches])
        runs.append((losses, tr.bucket.p.clone(), tr.last_logits.clone()))
        assert tr.last_loss.is_cuda and tr.last_logits.shape == (2, 3, 2) and tr.steps == 5
        assert any(not torch.equal(a, p.detach()) for a, p in zip(start, tr.model.parameters()))
        if use_graph:
            assert len(tr._graphs) == 1
            tr.release_graphs()
    assert torch.isfinite(runs[0][0]).all()
    assert all(P.same_bits(a, c) for a, c in zip(runs[0], runs[1]))
    with pytest.raises(ValueError):
        tr.train_step(batches[0][:5])
    with pytest.raises(ValueError):
        tr.train_step(batches[0], torch.zeros(1).cuda())


def test_literal_anchor_passes_draw_their_own_dropout_masks():
    """pos = neg: with dropout on, the literal form's two anchor passes (and the two copies of the compared window) take
    different masks, so the two pairs' logits differ; with dropout off they are the same bits."""
    nb = 2
    seq, pos, _ = triplet_windows(2, nb)
    batch = torch.cat([seq, pos, seq, pos], dim=0)
    for drop, same in ((0.2, False), (0.0, True)):
        model = build('linear', 'densenet18', nb, drop=drop)
        with torch.no_grad():
            _, zp, zn = model.forward_triplet(batch, literal=True)
        assert torch.isfinite(zp).all() and torch.equal(zp, zn) == same, drop


def test_test_step_is_deterministic_and_counts_on_the_device():
    store, _, _ = synthetic_store(seed=2)
    for share, use_graph in ((False, True), (True, False)):
        tr = trainer_of('linear', 'densenet18', 2, share, use_graph)
        batch, _ = store.triplet_batch([1, 4, 7, 10], step=0, literal=not share)
        tr.train_step(batch)
        first, second = tr.test_step(batch), tr.test_step(batch)
        assert not tr.model.training                                                 # model.eval(): dropout off
        for x, y in zip(first, second):
            assert P.same_bits(x, y)
        loss, acc, z = first
        preds = z.cpu().numpy().reshape(-1, 2).argmax(axis=1)
        want = np.array([1] * 4 + [0] * 4)
        assert acc.shape == (1,) and abs(float(acc) - float((preds == want).mean())) < 1e-7
        ref = R.head_forward  # (the loss of the logits the step returned, by the stable form)
        zz = z.double().cpu().numpy()
        terms = np.maximum(zz, 0) - zz * R.TARGET[:, None, :] + np.log1p(np.exp(-np.abs(zz)))
        assert abs(float(loss) - terms.sum() / 8) < 1e-5 and ref is not None
        tr.train_step(batch)
        assert tr.model.training
        tr.release_graphs()


def test_test_step_on_running_statistics_is_refused():
    store, _, _ = synthetic_store(seed=2)
    tr = trainer_of('linear', 'resnet18', 2, False, False)
    batch, _ = store.triplet_batch([1, 4], step=0, literal=True)
    with pytest.raises(NotImplementedError, match='running statistics'):
        tr.test_step(batch)
    assert torch.isfinite(tr.train_step(batch)).all()


def test_driver_pretrains_saves_and_seeds_a_classifier(tmp_path, capsys):
    """SiameseCNNLinearModel for 2 epochs on a 12-window store: meters filled, model saved; the file then seeds a cnn_linear run
    through --load-base-network.  A resnet18 run trains and skips its test epochs with one notice."""
    from deepards_amd import train_ards_detector as T
    from deepards_amd.checkpoint import load_base_network
    train, _, _ = synthetic_store(n_patients=4, per=3, nb=20, seed=4)
    test, _, _ = synthetic_store(n_patients=2, per=3, nb=20, seed=5, scaling_from=train)
    args = T.make_args(train_store=train, test_store=test, epochs=2, batch_size=4, seed=3, base_network='densenet18', cuda=False,
                       cuda_no_dp=True, save_model='pretrained', saved_models_dir=str(tmp_path), n_sub_batches=20)
    cls = T.SiameseCNNLinearModel(args)
    res = cls.train_and_test()
    summary = cls.perform_post_modeling_actions()
    assert len(res.get_meter('loss', 0)) == 6 and np.isfinite(res.get_meter('loss', 0)).all()
    for epoch in (1, 2):
        acc, tl = res.get_meter('accuracy_epoch_%d' % epoch, 0), res.get_meter('test_loss_epoch_%d' % epoch, 0)
        assert len(acc) == len(tl) == 2 and all(0.0 <= a <= 1.0 for a in acc) and np.isfinite(tl).all()
    assert len(res.get_meter('accuracy', 0)) == 4 and 'accuracy/0' in summary and 'test_loss/0' in summary
    path = os.path.join(str(tmp_path), 'pretrained.pth')
    assert os.path.exists(path)
    bb = load_base_network(path, T.base_networks, {})
    assert bb.network_name == 'densenet18'
    want = cls.model.breath_block.state_dict()
    assert all(torch.equal(v.cpu(), bb.state_dict()[k]) for k, v in want.items())
    # stage two: the classifier on top of the pretrained block
    gold = os.path.join(ROOT, 'tests', 'golden', 'test_dataset.npz')
    stage2 = T.network_map['cnn_linear'](T.make_args(train_from_pickle=gold, kfolds=2, epochs=1, batch_size=4, seed=3,
                                                     base_network='densenet18', cuda=False, cuda_no_dp=True, only_fold=None,
                                                     load_base_network=path, folds_in_flight=1, debug=True,
                                                     no_test_after_epochs=True))
    first = stage2.get_model().breath_block.state_dict()
    assert all(torch.equal(v.cpu(), first[k].cpu()) for k, v in bb.state_dict().items())
    res2 = stage2.train_and_test()
    assert np.isfinite(res2.get_meter('loss', 0)).all()
    capsys.readouterr()
    rn = T.SiameseCNNLinearModel(T.make_args(train_store=train, test_store=test, epochs=2, batch_size=4, seed=3,
                                             base_network='resnet18', cuda=False, cuda_no_dp=True))
    res3 = rn.train_and_test()
    out = capsys.readouterr().out
    assert out.count('the test epochs are skipped') == 1 and 'running statistics' in out
    assert len(res3.get_meter('loss', 0)) == 6 and res3.get_meter('accuracy', 0) == []
