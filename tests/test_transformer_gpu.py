"""GPU tests of the cnn_transformer head: the three block kernels against the float64 oracle (tests/tools/transformer_ref.py,
pinned to the reference classes by tests/test_transformer_cpu.py), dropout, memory discipline, graph replay, the whole model
against the reference's goldens, the trainer, checkpoints and the driver class.

Bound (per tensor): rel-l2 against float64 <= 4 x the reference's own fp32-vs-fp64 rel-l2 of that tensor (two fp32
evaluations each within e of the exact value differ by up to 2 e, a factor 2 more for the summation order), not below
16 * 2^-23 and not above the project's gradient criterion 1e-4.  The reference figure comes from the golden where the
shape has one (``err32/<tensor>``), else from the oracle evaluated in float32 on the CPU.  Where the float32 oracle is at hand
``y`` and ``dx`` are judged per token row as well, by the same rule with err32 of that row: one wrong token among 63 moves the
tensor's rel-l2 by an eighth of its own error only.  Figures: pytest -s."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'tools'))
pytestmark = pytest.mark.gpu

from oracle.weights import seeded_params  # noqa: E402
import transformer_ref as R  # noqa: E402
import poison as P  # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
FLOOR, CEIL = 16 * 2.0 ** -23, 1e-4
SEED_STEP = 0x9E3779B97F4A7C15 >> 1


def log(*a):
    print(' '.join(str(x) for x in a))


def bound(err32):
    return min(max(4 * err32, FLOOR), CEIL)


@pytest.fixture(scope='module')
def M():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    import deepards_amd.models as models
    return models


def _gold(name):
    z = np.load(os.path.join(GOLD, name), allow_pickle=False)
    return {k: z[k] for k in z.files}


def make_case(b, t, d, h, seed, nblocks=2):
    """Seeded input, block parameters (nn.Linear-like scales, LayerNorm gamma ~ U(.5, 1.5)), head and target, float32."""
    rng = np.random.default_rng([seed, b, t, d, h])
    u = lambda shape, k: rng.uniform(-1, 1, shape) / np.sqrt(k)
    blocks = []
    for _ in range(nblocks):
        blocks.append([u((h, d), d), u((h,), d), u((h, d), d), u((h,), d), u((h, d), d), u((h,), d), u((d, h), h), u((d,), h),
                       rng.uniform(.5, 1.5, d), rng.standard_normal(d) * .1, u((h, d), d), u((h,), d), u((d, h), h), u((d,), h),
                       rng.uniform(.5, 1.5, d), rng.standard_normal(d) * .1])
    blocks = [[a.astype(np.float32) for a in blk] for blk in blocks]
    return dict(x=rng.standard_normal((b, t, d)).astype(np.float32), blocks=blocks, wf=u((2, d), d).astype(np.float32),
                bf=u((2,), d).astype(np.float32), target=np.eye(2, dtype=np.float32)[rng.integers(0, 2, b)])


def golden_case(name):
    g = _gold(name)
    blocks = [[g['param/blocks.%d.%s' % (i, n)] for n in R.PARAM_NAMES] for i in range(2)]
    c = dict(x=g['x'], blocks=blocks, wf=g['param/linear_final.weight'], bf=g['param/linear_final.bias'], target=g['target'])
    err = {'y': float(g['err32/y']), 'logits': float(g['err32/logits']), 'dx': float(g['err32/dx']),
           'dwf': float(g['err32/grad/linear_final.weight']), 'dbf': float(g['err32/grad/linear_final.bias'])}
    for i in range(2):
        err['weights%d' % i] = float(g['err32/weights%d' % i])
        for n in R.PARAM_NAMES:
            err['g%d.%s' % (i, n)] = float(g['err32/grad/blocks.%d.%s' % (i, n)])
    return c, err


def oracle(c, dtype=np.float64, masks=None, p=0.0):
    o = R.transformer_loss(c['x'].astype(dtype), c['blocks'], c['wf'], c['bf'], c['target'], masks, p)
    flat = {'y': o['y'], 'logits': o['logits'], 'dx': o['dx'], 'dwf': o['dwf'], 'dbf': o['dbf']}
    for i, (w, gr) in enumerate(zip(o['weights'], o['grads'])):
        flat['weights%d' % i] = w
        for n, a in zip(R.PARAM_NAMES, gr):
            flat['g%d.%s' % (i, n)] = a
    return flat


def run_gpu(M, c, p=0.0, seed=None):
    """The head on the device through the model classes: Transformer -> Linear2Function -> BCE, one backward."""
    from deepards_amd import functional as F_
    b, t, d = c['x'].shape
    h = c['blocks'][0][0].shape[0]
    tfm = M.Transformer(d, h, len(c['blocks']), 4, dropout=p)
    for blk, arrs in zip(tfm.blocks, c['blocks']):
        for q, a in zip(blk.block_params(), arrs):
            q.data.copy_(torch.from_numpy(a))
    tfm = tfm.cuda().train()
    if seed is not None:
        tfm._drop_seed.fill_(seed)
    x = torch.from_numpy(c['x']).cuda().requires_grad_(True)
    wf, bf = [torch.from_numpy(c[k]).cuda().requires_grad_(True) for k in ('wf', 'bf')]
    y = tfm(x)
    logits = F_.Linear2Function.apply(y.reshape(b * t, d), wf, bf)
    tgt = torch.from_numpy(c['target']).cuda().unsqueeze(1).expand(-1, t, -1).reshape(-1, 2).contiguous()
    loss = F_.bce_with_logits(logits, tgt)
    loss.backward()
    out = {'y': y, 'logits': logits.view(b, t, 2), 'dx': x.grad, 'dwf': wf.grad, 'dbf': bf.grad}
    for i, blk in enumerate(tfm.blocks):
        out['weights%d' % i] = blk.attention.weights
        for n, q in zip(R.PARAM_NAMES, blk.block_params()):
            out['g%d.%s' % (i, n)] = q.grad
    return {k: v.detach().double().cpu().numpy() for k, v in out.items()}, tfm


def form(t, d, h):
    """(tokens per wave and pass of the forward, of the backward, LDS bytes of the forward, of the backward) at (T, D, H)."""
    from deepards_amd import hip_ops as H
    return H.tfm_block_form(t, d, h)


def rel_l2(a, b):
    nb = float(np.linalg.norm(b))
    return float(np.linalg.norm(a - b) / (nb if nb > 1e-9 else 1.0))      # ~zero references: absolute (see compare)


def compare_rows(tag, got, ref64, ref32):
    """``y`` and ``dx`` token by token: rel-l2 of row (b, t) against the bound of that row's own float32 error."""
    bad = []
    for k in ('y', 'dx'):
        worst = (0.0, None, 0.0, 0.0)
        for idx in np.ndindex(*ref64[k].shape[:2]):
            e, bd = rel_l2(got[k][idx], ref64[k][idx]), bound(R.rel_l2(ref32[k][idx], ref64[k][idx]))
            if not e / bd < worst[0]:                                   # (a NaN ratio is kept, and fails below)
                worst = (e / bd, idx, e, bd)
        log('%s %-42s worst token row (b, t) = %s: rel-l2 %.3e  bound %.3e  ratio %.3f' % (tag, k + ' per token', worst[1], worst[2],
                                                                                      worst[3], worst[0]))
        if not worst[0] <= 1:
            bad.append((k, 'token row', worst[1], worst[2], worst[3]))
    return bad


def compare(tag, got, ref64, err32, ref32=None):
    bad = []
    for k in sorted(ref64):
        # (k_linear.bias: a constant added to every key's score leaves the softmax unchanged, so its gradient is zero in
        # exact arithmetic -- ~1e-17 in the oracle; rel_l2 judges such a ~zero reference absolutely)
        e, bd = rel_l2(got[k], ref64[k]), bound(err32[k])
        log('%s %-42s rel-l2 %.3e  reference fp32 %.3e  bound %.3e' % (tag, k, e, err32[k], bd))
        assert np.isfinite(got[k]).all(), (tag, k)
        if not e <= bd:
            bad.append((k, e, bd))
    if ref32 is not None:
        bad += compare_rows(tag, got, ref64, ref32)
    assert not bad, bad


SHAPES = [(1, 20, 128, 16), (3, 20, 128, 16), (2, 5, 128, 8), (2, 1, 128, 16), (1, 64, 128, 64), (2, 20, 512, 16)]
# (B, T, D, H) -> tokens per wave and pass (forward, backward): the form each corner means to reach, asserted through
# tfm_block_form so that a moved threshold fails here instead of moving the case to the other form
CORNERS = {(2, 23, 128, 16): (5, 3),      # forward: two passes, the second with 3 of its 20 slots filled; backward 2 passes, 11 of 12
           (2, 7, 1024, 16): (1, 1),      # one token through D > 512; T % 4 = 3: the clamped tail of the second pass
           (1, 63, 64, 64): (1, 1),       # one token through T H > 1024; T % 4 = 3; the smallest D (one lane stride)
           (2, 33, 256, 40): (1, 1),      # T % 4 = 1; head size 10
           (3, 9, 192, 24): (5, 3),       # D of three lane strides, no power of two; head size 6
           (2, 13, 576, 56): (1, 1),      # D = 9 x 64; head size 14
           (1, 64, 512, 16): (5, 3),      # T H = 1024 at D = 512: the backward above 64 KB of LDS
           (1, 64, 2048, 64): (1, 1)}     # the largest shape taken
SHAPES += list(CORNERS)
GOLDENS = {(2, 5, 128, 8): 'tfm_block_2x5x128x8.npz', (2, 20, 512, 16): 'tfm_block_2x20x512x16.npz'}


@pytest.mark.parametrize('shape', SHAPES, ids=['x'.join(map(str, s)) for s in SHAPES])
def test_block_kernels_against_the_fp64_oracle(M, shape):
    r32 = None
    if shape in GOLDENS:
        c, err32 = golden_case(GOLDENS[shape])
        ref = oracle(c)
    else:
        c = make_case(*shape, seed=1)
        r32 = oracle(c, np.float32)
        ref = oracle(c)
        err32 = {k: R.rel_l2(r32[k], ref[k]) for k in ref}
    if shape in CORNERS:
        b, t, d, h = shape
        tf, tb, lf, lb = form(t, d, h)
        log('x'.join(map(str, shape)), 'form: tokens per wave (%d, %d), LDS bytes (%d, %d)' % (tf, tb, lf, lb))
        assert (tf, tb) == CORNERS[shape]
        if shape == (2, 23, 128, 16):
            assert -(-(-(-t // 4)) // tf) == 2 and t - 4 * tf == 3
        if shape == (1, 64, 512, 16):
            assert lb > 64 * 1024 >= lf
        if shape == (1, 64, 2048, 64):
            assert lb == 148480
    got, _ = run_gpu(M, c)
    compare('x'.join(map(str, shape)), got, ref, err32, r32)


@pytest.mark.parametrize('kind', ['golden', 'saturated_softmax', 'shifted_input'])
def test_block_kernels_at_2x20x128x16(M, kind):
    """The golden shape; q / k weights x 30 (the softmax saturates: no NaN); input + 1000 (LayerNorm cancellation)."""
    c, err32 = golden_case('tfm_block_2x20x128x16.npz')
    if kind != 'golden':
        c = dict(c, blocks=[list(b) for b in c['blocks']])
        if kind == 'saturated_softmax':
            for blk in c['blocks']:
                blk[0], blk[2] = blk[0] * 30, blk[2] * 30
        else:
            c['x'] = c['x'] + np.float32(1000)
        r32, ref = oracle(c, np.float32), oracle(c)
        err32 = {k: R.rel_l2(r32[k], ref[k]) for k in ref}
    got, _ = run_gpu(M, c)
    compare(kind, got, oracle(c), err32)


def device_masks(tfm, b, t, d, p):
    """The masks the device used: H.dropout with the same seed, salt and p over ones (the pattern of test_model_gpu)."""
    from deepards_amd import hip_ops as H
    ones = torch.ones(b * t, d, device='cuda')
    return [[(H.dropout(ones, tfm._drop_seed, 2 * i + 1 + s, p) > 0).view(b, t, d).cpu().numpy() for s in range(2)]
            for i in range(len(tfm.blocks))]


def _dropout_against_the_oracle(M, shape, p, tag, rows=False):
    """The block with dropout: the device's masks (H.dropout with the block's seed and salts) given to the oracle."""
    b, t, d, h = shape
    c = make_case(b, t, d, h, seed=2)
    got, tfm = run_gpu(M, c, p=p, seed=12345)
    assert int(tfm._drop_seed) == 12345 + SEED_STEP                    # bumped once, then used
    masks = device_masks(tfm, b, t, d, p)
    assert all(0.7 < m.mean() < 0.9 for pair in masks for m in pair)
    ref, r32 = oracle(c, masks=masks, p=p), oracle(c, np.float32, masks=masks, p=p)
    compare(tag, got, ref, {k: R.rel_l2(r32[k], ref[k]) for k in ref}, r32 if rows else None)
    return tfm


def test_dropout_on_the_one_token_form(M):
    """(2, 7, 1024, 16): one token per wave, the second pass with a clamped token whose mask index is its neighbour's."""
    assert form(7, 1024, 16)[:2] == (1, 1)
    _dropout_against_the_oracle(M, (2, 7, 1024, 16), 0.2, 'dropout 2x7x1024x16', rows=True)


def test_dropout_masks_are_the_generators_and_the_block_follows_the_oracle(M):
    p = 0.2
    assert form(20, 128, 16)[:2] == (5, 3)
    tfm = _dropout_against_the_oracle(M, (2, 20, 128, 16), p, 'dropout')
    # the generator's rate: a (20 * 64, 512) mask keeps 0.8 within 5 sigma
    from deepards_amd import hip_ops as H
    n = 20 * 64 * 512
    kept = float((H.dropout(torch.ones(20 * 64, 512, device='cuda'), tfm._drop_seed, 1, p) > 0).double().mean())
    sigma = np.sqrt(0.8 * 0.2 / n)
    log('kept fraction %.6f (5 sigma = %.6f)' % (kept, 5 * sigma))
    assert abs(kept - 0.8) <= 5 * sigma


def _op_inputs(shape, seed=3, p=0.2):
    c = make_case(*shape, seed=seed, nblocks=1)
    x = torch.from_numpy(c['x']).cuda()
    params = [torch.from_numpy(a).cuda() for a in c['blocks'][0]]
    dy = torch.from_numpy(np.random.default_rng(seed).standard_normal(c['x'].shape).astype(np.float32)).cuda()
    drop = (torch.full((1,), 777, dtype=torch.int64, device='cuda'), 1, 2, p)
    return x, params, dy, drop


@pytest.mark.parametrize('shape', [(3, 20, 128, 16), (2, 5, 128, 8), (1, 64, 128, 64), (2, 7, 1024, 16), (1, 63, 64, 64), (2, 23, 128, 16)],
                         ids=lambda s: 'x'.join(map(str, s)))
def test_memory_discipline_of_the_three_launches(M, shape):
    """Every output and saved tensor fully written from NaN-poisoned allocations with the bits of the clean run; operands
    inside guard bands: same bits, guards intact, inputs unchanged; accumulate adds exactly once."""
    from deepards_amd import hip_ops as H
    if shape in CORNERS:
        assert form(*shape[1:])[:2] == CORNERS[shape]

    def run(x, params, dy, drop, grads=None, accumulate=False):
        y, saved = H.tfm_block_fwd(x, params, drop)
        dx, work = H.tfm_block_bwd(dy, x, params, saved, drop)
        g = H.tfm_block_pgrad(dy, x, params, saved, work, grads=grads, accumulate=accumulate, drop=drop)
        torch.cuda.synchronize()
        return [y] + list(saved) + [dx] + list(work) + list(g)

    x, params, dy, drop = _op_inputs(shape)
    clean = run(x, params, dy, drop)
    with P.poisoned_allocations() as stats:
        pois = run(x, params, dy, drop)
    assert stats.filled >= 6
    for i, (a, b) in enumerate(zip(pois, clean)):
        assert not P.has_poison(a), 'result %d holds the pattern' % i
        assert P.same_bits(a, b), 'result %d: %s' % (i, P.diff_report(a, b))
    # guard bands around every operand and every gradient destination
    handles, keep = [], [x.clone(), dy.clone()] + [q.clone() for q in params]

    def wrap(t, name):
        v, hd = P.guarded(t, name=name)
        handles.append(hd)
        return v
    gx, gdy = wrap(x, 'x'), wrap(dy, 'dy')
    gparams = [wrap(q, 'param%d' % i) for i, q in enumerate(params)]
    dests = [wrap(P.fill_poison(torch.empty_like(q)), 'grad%d' % i) for i, q in enumerate(params)]
    guarded = run(gx, gparams, gdy, drop, grads=dests)
    for i, (a, b) in enumerate(zip(guarded, clean)):
        assert P.same_bits(a.contiguous(), b), 'guarded result %d: %s' % (i, P.diff_report(a.contiguous(), b))
    P.assert_guards_intact(handles)
    for a, b in zip([gx, gdy] + gparams, keep):
        assert P.same_bits(a.contiguous(), b), 'an input changed'
    # accumulate: destination + gradient, exactly once
    base = [torch.full_like(q, 0.5) for q in params]
    acc = run(x, params, dy, drop, grads=[b.clone() for b in base], accumulate=True)[-16:]
    for a, g in zip(acc, clean[-16:]):
        assert torch.equal(a, g + 0.5)


def build_model(M, backbone, g=None, p=0.0, seed=11):
    if g is not None:
        bb = M.resnet18(first_pool_type=str(g['first_pool_type'])) if backbone == 'resnet18' else M.densenet18(drop_rate=0)
        model = M.CNNTransformerNetwork(bb, 0, False, int(g['hidden']), int(g['blocks']))
        sd = {k: torch.from_numpy(v) for k, v in seeded_params(backbone, int(g['seed']), bn_bias_shift=float(g['bn_bias_shift']),
                                                               head='single_breath').items() if k.startswith('breath_block.')}
        sd.update({k[len('param/'):]: torch.from_numpy(v) for k, v in g.items() if k.startswith('param/')})
    else:
        torch.manual_seed(seed)
        bb = M.resnet18() if backbone == 'resnet18' else M.densenet18(drop_rate=0)
        model = M.CNNTransformerNetwork(bb, 0, False, 16, 2)
        sd = {}
    assert not model.load_state_dict(sd, strict=False).unexpected_keys
    for blk in model.transformer.blocks:
        blk.dropout = p
    return model.cuda().train()


class tapped(object):
    """Record the post-ReLU activations of the breath block (functional.DECISION_TAP) for decision_match.hip_relu_flips."""

    def __enter__(self):
        from deepards_amd import functional as F_
        F_.DECISION_TAP = []
        return F_.DECISION_TAP

    def __exit__(self, *exc):
        from deepards_amd import functional as F_
        F_.DECISION_TAP = None


@pytest.mark.parametrize('backbone', ['resnet18', 'densenet18'])
def test_whole_model_against_the_reference_goldens(M, backbone):
    """CNNTransformerNetwork on the seeded backbones of oracle.weights, p = 0.  Logits: against the reference's fp64 logits of
    the golden, at the bound.  Gradients: every parameter under the suite's gradient criterion (decision_match.
    assert_gradients_match: per tensor 8 x the oracle's own float32 error, 1e-4 at the most, against the fp64 oracle under the
    activation decisions this run took) -- the oracle is
    np_ref's breath block with transformer_ref as its head, pinned to the golden's logits, loss and gradient digests by
    tests/test_transformer_cpu.py."""
    from deepards_amd import functional as F_
    from decision_match import assert_gradients_match, fp32_noise
    g = _gold('tfm_model_b2_%s.npz' % backbone)
    model = build_model(M, backbone, g)
    assert list(model.state_dict().keys()) == [str(n) for n in g['names']]
    x, t = torch.from_numpy(g['x']).cuda(), torch.from_numpy(g['target']).cuda()
    with tapped() as taps:
        out = model(x, None)
    assert out.shape == (2, 20, 2)
    loss = F_.bce_with_logits(out.reshape(-1, 2), t.unsqueeze(1).expand(-1, 20, -1).reshape(-1, 2).contiguous())
    loss.backward()
    e = R.rel_l2(out.detach().double().cpu().numpy(), g['logits'])
    log('%s logits rel-l2 %.3e (reference fp32 %.3e, bound %.3e), loss %.8f vs %.8f' %
        (backbone, e, float(g['err32/logits']), bound(float(g['err32/logits'])), float(loss), float(g['loss'])))
    assert e <= bound(float(g['err32/logits'])) and abs(float(loss) - float(g['loss'])) < 1e-5
    ref = R.model_reference(g, backbone)
    ours = {n: q.grad.double().cpu().numpy() for n, q in model.named_parameters() if q.grad is not None and n in ref['grads']}
    assert set(ours) == set(ref['grads'])
    noise = fp32_noise(ref, R.model_reference(g, backbone, dtype=np.float32))
    # (k_linear.bias: a constant added to every key's score leaves the softmax unchanged -- its gradient is zero in exact
    # arithmetic, ~1e-19 in the oracle, and has no relative scale in any precision)
    zero = ['transformer.blocks.%d.attention.k_linear.bias' % i for i in range(int(g['blocks']))]
    assert_gradients_match(ref, ours, noise, 'cnn_transformer ' + backbone, log=log, taps=taps, zero=zero)
    w = model.transformer.blocks[0].attention.weights
    assert w.shape == (2, 4, 20, 20) and torch.allclose(w.sum(-1), torch.ones(2, 4, 20, device='cuda'), atol=1e-5)


@pytest.mark.parametrize('optimizer', ['sgd', 'adam'])
def test_trainer_eager_and_captured_steps_are_bit_equal(M, optimizer):
    from deepards_amd.train import HotPathTrainer
    g = _gold('tfm_model_b2_densenet18.npz')
    x, t = torch.from_numpy(g['x']).cuda(), torch.from_numpy(g['target']).cuda()
    runs = []
    for use_graph in (False, True):
        tr = HotPathTrainer(build_model(M, 'densenet18', p=0.2), optimizer=optimizer, use_graph=use_graph)
        losses = [tr.train_step(x, t).clone() for _ in range(3)]
        runs.append((torch.cat([l.reshape(-1) for l in losses]), tr.bucket.p.clone(),
                     tr.model.transformer._drop_seed.clone()))
        if use_graph:
            tr.release_graphs()
    assert torch.isfinite(runs[0][0]).all()
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert int(runs[0][2]) == int(runs[1][2]) == (3 * SEED_STEP + 2 ** 63) % 2 ** 64 - 2 ** 63       # one bump per step


def test_replayed_step_is_deterministic_and_draws_fresh_masks(M):
    """A captured train step replayed 3x from the same state with the seed reset: the same bits each time; without the
    reset consecutive replays use different masks and the seed buffer holds the bumped value."""
    from deepards_amd.train import HotPathTrainer
    g = _gold('tfm_model_b2_resnet18.npz')
    x, t = torch.from_numpy(g['x']).cuda(), torch.from_numpy(g['target']).cuda()
    tr = HotPathTrainer(build_model(M, 'resnet18', p=0.2), use_graph=True, loss='vacillating', loss_param=2.0)
    with pytest.raises(ValueError, match='carry_state'):
        HotPathTrainer(tr.model, carry_state=True)
    tr.train_step(x, t)
    tr.train_step(x, t)                                   # captured now
    snap = tr.snapshot()                                  # (module buffers are part of it: restore() resets the seed)
    seed0 = int(tr.model.transformer._drop_seed)
    outs = []
    for _ in range(3):
        tr.restore(snap)
        outs.append((tr.train_step(x, t).clone(), tr.bucket.p.clone()))
    assert torch.isfinite(outs[0][0]).all()
    assert all(torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1]) for o in outs[1:])
    assert int(tr.model.transformer._drop_seed) == seed0 + SEED_STEP
    tr.restore(snap)
    tr.use_graph = False                                  # the same step eagerly, from the same state and seed
    eager = (tr.train_step(x, t).clone(), tr.bucket.p.clone())
    tr.use_graph = True
    assert torch.equal(eager[0], outs[0][0]) and torch.equal(eager[1], outs[0][1]), 'replay differs from the eager step'
    # without the reset: consecutive replays draw other masks, and the seed buffer holds the bumped value
    tr.restore(snap)
    l1, p1 = tr.train_step(x, t).clone(), tr.bucket.p.clone()
    tr.bucket.p.copy_(snap['p'])
    for k, v in snap['state'].items():
        tr.state[k].copy_(v)
    l2 = tr.train_step(x, t).clone()
    assert int(tr.model.transformer._drop_seed) == (seed0 + 2 * SEED_STEP + 2 ** 63) % 2 ** 64 - 2 ** 63
    assert torch.equal(l1, outs[0][0]) and not torch.equal(l2, l1), 'the second replay drew the first one\'s masks'
    tr.restore(snap)
    la, ga, _ = tr.test_step(x, t)
    lb, gb, _ = tr.test_step(x, t)
    assert ga.shape == (2, 20, 2) and not torch.equal(ga, gb), 'two consecutive test steps drew the same dropout masks'
    assert torch.isfinite(la).all() and torch.isfinite(lb).all()
    tr.release_graphs()
    tr2 = HotPathTrainer(build_model(M, 'densenet18', p=0.2), use_graph=False, loss='bce', loss_calc='last_breath')
    assert torch.isfinite(tr2.train_step(x, t)).all()


def _run_tfm_dp_children(tmp_path, gold_path, p, world=2):
    """`world` FRESH child processes (tests/tools/tfm_dp_child.py), all on cuda:0, gradients over gloo."""
    import subprocess
    port = 29500 + (os.getpid() * 7 + int(p * 100) + 41) % 3000
    procs, outs = [], []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
        outs.append(str(tmp_path / ('tfm_dp_p%d_rank%d.npz' % (int(p * 100), r))))
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, 'tests', 'tools', 'tfm_dp_child.py'), gold_path, outs[-1],
                                       str(p)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    logs = []
    for p_ in procs:
        try:
            o, _ = p_.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        logs.append(o.decode(errors='replace'))
    for r, p_ in enumerate(procs):
        assert p_.returncode == 0, 'rank %d failed:\n%s' % (r, logs[r][-4000:])
    return [dict(np.load(o, allow_pickle=False)) for o in outs]


def test_two_ranks_over_gloo_follow_the_single_process_run(M, tmp_path):
    """Two processes on this GPU, gloo all-reduce of the flat bucket, rank r on window r of the golden's B = 2 batch; rank 1
    starts from another initialisation and another dropout seed.  p = 0: the replicas end bit-identical, and the mean of the
    rank losses and the parameters equal this build's single-process B = 2 run at the bounds of
    test_model_gpu.py::test_data_parallel_two_processes_trajectory (losses 2e-6, parameters 2e-5: other fp32 summation
    orders, not bit for bit).  p = 0.2: three finite steps, bit-identical replicas, rank 0's seed on both ranks, bumped once
    per step (each rank draws its masks by the index in its LOCAL (B_local T, D) tensor, as the DenseNet dropout does)."""
    from deepards_amd.train import HotPathTrainer
    path = os.path.join(GOLD, 'tfm_model_b2_densenet18.npz')
    g = _gold('tfm_model_b2_densenet18.npz')
    r0, r1 = _run_tfm_dp_children(tmp_path, path, 0.0)
    assert int(r0['allreduce_calls']) == int(r1['allreduce_calls']) == 3
    names = [k for k in r0 if k.startswith('p/')]
    assert all(np.array_equal(r0[k], r1[k]) for k in names)
    losses = (r0['losses'] + r1['losses']) / 2
    model = build_model(M, 'densenet18', g)
    tr = HotPathTrainer(model, optimizer='sgd', use_graph=True)
    x, t = torch.from_numpy(g['x']).cuda(), torch.from_numpy(g['target']).cuda()
    single = np.array([float(tr.train_step(x, t)) for _ in range(3)])
    tr.release_graphs()
    worst = max(float(np.abs(r0['p/' + n] - q.detach().cpu().numpy()).max()) for n, q in model.named_parameters())
    log('dp2 losses', losses.tolist(), 'single', single.tolist(), 'params max abs diff %.3e' % worst)
    assert np.isfinite(losses).all() and np.abs(losses - single).max() < 2e-6
    assert worst < 2e-5
    moved = max(float(np.abs(r0['p/' + n] - g['param/' + n]).max()) for n in
                ('transformer.blocks.0.attention.q_linear.weight', 'transformer.blocks.1.ff.2.weight', 'linear_final.weight'))
    assert moved > 1e-6, 'the head did not train'
    d0, d1 = _run_tfm_dp_children(tmp_path, path, 0.2)
    assert np.isfinite(d0['losses']).all() and np.isfinite(d1['losses']).all()
    assert all(np.array_equal(d0[k], d1[k]) for k in names)
    assert int(d0['seed'][0]) == int(d1['seed'][0]) == (3 * SEED_STEP + 2 ** 63) % 2 ** 64 - 2 ** 63
    assert not np.array_equal(d0['losses'], r0['losses'])


def test_checkpoints_round_trip(M, tmp_path):
    from deepards_amd import checkpoint as C
    model = build_model(M, 'densenet18')
    path = str(tmp_path / 'whole.pth')
    torch.save(model.cpu(), path)
    assert C.checkpoint_kind(path) == 'own'
    back = C.load_own_module(path)
    assert isinstance(back, M.CNNTransformerNetwork)
    sd = model.state_dict()
    assert list(back.state_dict().keys()) == list(sd.keys()) and '_drop_seed' not in ''.join(sd.keys())
    assert all(torch.equal(back.state_dict()[k], sd[k]) for k in sd)
    g = _gold('tfm_model_b2_densenet18.npz')
    assert [str(n) for n in g['names']] == list(sd.keys())                   # the reference's keys, in its order
    path2 = str(tmp_path / 'sd.pth')
    torch.save(sd, path2)
    fresh = C.load_model_weights(path2, lambda: build_model(M, 'densenet18', seed=99).cpu())
    assert all(torch.equal(fresh.state_dict()[k], sd[k]) for k in sd)


@pytest.mark.parametrize('backbone', ['resnet18', 'densenet18'])
def test_driver_class_trains_and_tests_on_the_ingested_fixture(M, backbone):
    """``CNNTransformerModel(make_args(...)).train_and_test()``: one epoch, 2 folds, a vote for every breath of every test
    window; the test epoch runs train-mode modules under no_grad (train_ards_detector.py:448)."""
    from deepards_amd import train_ards_detector as T
    from deepards_amd import models as M_
    seen = []
    orig = M_.CNNTransformerNetwork.forward

    def spy(self, x, metadata):
        seen.append((self.training, torch.is_grad_enabled()))
        return orig(self, x, metadata)
    M_.CNNTransformerNetwork.forward = spy
    try:
        cls = T.CNNTransformerModel(T.make_args(train_from_pickle=os.path.join(GOLD, 'test_dataset.npz'), kfolds=2, epochs=1,
                                                batch_size=4, seed=3, base_network=backbone, cuda=False, cuda_no_dp=True))
        res = cls.train_and_test()
    finally:
        M_.CNNTransformerNetwork.forward = orig
    assert any(tr and ge for tr, ge in seen) and any(tr and not ge for tr, ge in seen) and all(tr for tr, _ in seen)
    tested = []
    for fold in (0, 1):
        assert np.isfinite(res.get_meter('loss', fold)).all() and np.isfinite(res.get_meter('test_loss', fold)).all()
        r = res.patient_results[(fold, 1)]
        windows = sorted(set(r['window_abs_index'].tolist()))
        assert len(r['window_pred']) == 20 * len(windows) == r['votes'].sum()
        tested += windows
    assert len(set(tested)) == len(tested) == 20
