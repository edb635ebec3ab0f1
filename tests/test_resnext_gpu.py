"""The se_resnext50_32x4d / se_resnext101_32x4d backbones on the GPU: the grouped k3 kernels (csrc/conv_grouped.hip), the
chained SEBlockFunction on the ResNeXt bottleneck, the whole model and the trainer.

Exact cases: integer operands (tests/tools/exact_conv.operand, amplitude 2) and integer weights in {-2 .. 2}: a direct fp32
kernel forms only integers below 2^24 on them whatever its tiling and fold order (asserted on the CPU first), so the result
must EQUAL the float64 grouped convolution.  Float cases: rel-l2 against float64 torch on the CPU <= min(max(4 err32, 16
2^-23), 1e-4), err32 = stock fp32 conv1d(groups=32) on the CPU against float64 (the kernels alone) or the golden's own figure
(blocks, models): the bound of tests/test_sebn_gpu.py.  The block cases keep every ReLU pre-activation of the oracle at least
1e-3 from zero (asserted here, on the CPU).  Figures: pytest -s."""
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'tools'))
pytestmark = pytest.mark.gpu

from oracle.weights import digest  # noqa: E402
import resnext_ref as R  # noqa: E402
import sebn_ref  # noqa: E402
import poison as P  # noqa: E402
import exact_conv as E  # noqa: E402
import decision_match as DM  # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
FLOOR, CEIL = 16 * 2.0 ** -23, 1e-4
GROUPS = 32
WIDTHS = (128, 256, 512, 1024)
FWD, DGRAD, WGRAD = 0, 1, 2


def log(*a):
    print(' '.join(str(x) for x in a))


def bound(err32):
    return min(max(4 * err32, FLOOR), CEIL)


@pytest.fixture(scope='module')
def H():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from deepards_amd import hip_ops
    return hip_ops


@pytest.fixture(scope='module')
def M():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    import deepards_amd.models as models
    return models


@functools.lru_cache(maxsize=None)
def _gold(name):
    z = np.load(os.path.join(GOLD, name), allow_pickle=False)
    return {k: z[k] for k in z.files}


def cu(a):
    a = a.numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return torch.from_numpy(np.ascontiguousarray(a.astype(np.float32))).cuda()


def host(t):
    return t.detach().double().cpu().numpy()


def check(tag, name, got, ref64, err32, problems):
    e, bd = R.rel_l2(host(got).reshape(np.shape(ref64)), ref64), bound(err32)
    log('%s %-28s rel-l2 %.3e  reference fp32 %.3e  bound %.3e' % (tag, name, e, err32, bd))
    if not e <= bd:
        problems.append('%s %s: rel-l2 %.3e > bound %.3e (reference fp32 %.3e)' % (tag, name, e, bd, err32))


def sid(s):
    return 'x'.join(map(str, s))


# ---- float64 grouped convolution on the CPU (operands (rows, L, C) channels-last) -----------------------------------------
def ref_fwd(x, w, stride, dtype=torch.float64):
    return TF.conv1d(R._t(x, dtype).permute(0, 2, 1), R._t(w, dtype), stride=stride, padding=1, groups=GROUPS).permute(0, 2, 1)


def ref_all(x, w, dy, stride, dtype=torch.float64):
    """-> y, dx, dw of the grouped conv as arrays of ``dtype`` widened to float64."""
    xt, wt = R._t(x, dtype).clone().requires_grad_(True), R._t(w, dtype).clone().requires_grad_(True)
    y = ref_fwd(xt, wt, stride, dtype)
    dx, dw = torch.autograd.grad(y, [xt, wt], R._t(dy, dtype))
    return tuple(t.detach().double().numpy() for t in (y, dx, dw))


def out_len(l, stride):
    return (l - 1) // stride + 1


@functools.lru_cache(maxsize=None)
def int_case(rows, l, c, stride, seed=0):
    """Integer x, w, dy (float64, channels-last), the float64 results, with the bit budget asserted: every partial sum of
    absolute values stays below 2^24, so fp32 holds every intermediate of any summation order exactly."""
    lo = out_len(l, stride)
    x = np.ascontiguousarray(E.operand(11 + seed, rows, c, l, amp=2).transpose(0, 2, 1))
    dy = np.ascontiguousarray(E.operand(12 + seed, rows, c, lo, amp=2).transpose(0, 2, 1))
    w = E.weight(13 + seed, c, c // GROUPS, 3, amp=2)
    y, dx, dw = ref_all(x, w, dy, stride)
    peak = max(float(np.max(a)) for a in ref_all(np.abs(x), np.abs(w), np.abs(dy), stride))
    assert peak < E.EXACT_INT, peak
    return x, w, dy, y, dx, dw


def run_all(H, x, w, dy, stride):
    xt, wt, dyt = cu(x), cu(w), cu(dy)
    y = H.gconv3_fwd(xt, wt, stride)
    dx = H.gconv3_dgrad(dyt, wt, stride, xt.shape[1])
    dw = H.gconv3_wgrad(dyt, xt, stride)
    torch.cuda.synchronize()
    return y, dx, dw


def _tile_edge_shapes(H):
    """Per width: one row past the last full block of tiles, and one position past a tile, as gconv3_plan reports them."""
    from deepards_amd import gconv_ops as G
    shapes = []
    for c in WIDTHS:
        for stride in (1, 2):
            p = G.gconv3_plan(FWD, 1, 8 * stride, c, stride)
            tp, nt = p.tile_positions, p.tiles_per_block
            shapes.append((nt + 1, (tp - 1) * stride + 1, c, stride))             # Lo = one full tile a row, nt + 1 rows: one row past a block
            shapes.append((2, tp * stride + 1, c, stride))                        # Lo = tile + 1: a one-position tile per row
    return shapes


EXACT_SHAPES = [(3, 7, c, 1) for c in WIDTHS] + [(3, 14, c, 2) for c in WIDTHS] + \
    [(1, 1, 128, 1), (1, 1, 1024, 2), (2, 2, 256, 2), (2, 5, 512, 2), (4, 56, 128, 1), (6, 56, 256, 2)]


def _exact(H, shape):
    rows, l, c, stride = shape
    x, w, dy, y, dx, dw = int_case(*shape)
    gy, gdx, gdw = run_all(H, x, w, dy, stride)
    assert np.array_equal(host(gy), y), 'forward differs from the float64 grouped convolution'
    assert np.array_equal(host(gdx), dx), 'data gradient differs'
    assert np.array_equal(host(gdw), dw), 'weight gradient differs'


@pytest.mark.parametrize('shape', EXACT_SHAPES, ids=sid)
def test_exact_on_integer_operands(H, shape):
    _exact(H, shape)


def test_exact_one_past_every_tile_edge(H):
    """A single row past the tiles of one block and a single position past a tile, per width and stride, with the tile sizes
    read from the plan; for the weight gradient a case whose rows Lo exceeds one partial chunk by one position."""
    from deepards_amd import gconv_ops as G
    for shape in _tile_edge_shapes(H):
        _exact(H, shape)
    for c, stride in ((128, 1), (1024, 2)):
        p = G.gconv3_plan(WGRAD, 1, 8 * stride, c, stride)
        chunk = p.tile_positions * p.tiles_per_block                              # output positions of one chunk of one row
        l = chunk * stride + 1                                                    # Lo = chunk + 1 in a single row
        assert out_len(l, stride) == chunk + 1
        q = G.gconv3_plan(WGRAD, 1, l, c, stride)
        assert q.grid[0] == 2 and q.tiles == p.tiles_per_block + 1
        _exact(H, (1, l, c, stride))


def test_groups_do_not_mix(H):
    """One group's input all zero: exactly that group's outputs are zero.  A nonzero value in one group only: no other
    group's output, data gradient or weight gradient sees it."""
    for c, stride in ((128, 1), (512, 2), (1024, 1)):
        cg, g = c // GROUPS, 5
        rows, l = 3, 9
        lo = out_len(l, stride)
        rng = np.random.default_rng([c, stride])
        x = rng.integers(1, 3, (rows, l, c)).astype(np.float64)                   # strictly positive
        w = rng.integers(1, 3, (c, cg, 3)).astype(np.float64)
        x[:, :, g * cg:(g + 1) * cg] = 0
        y = host(H.gconv3_fwd(cu(x), cu(w), stride))
        zero = ~np.any(y != 0, axis=(0, 1))
        assert np.array_equal(np.flatnonzero(zero), np.arange(g * cg, (g + 1) * cg))
        x = np.zeros((rows, l, c))
        x[:, :, g * cg:(g + 1) * cg] = rng.integers(1, 3, (rows, l, cg))
        dy = np.zeros((rows, lo, c))
        dy[:, :, g * cg:(g + 1) * cg] = rng.integers(1, 3, (rows, lo, cg))
        ones = np.ones((rows, lo, c))
        gy, gdx, _ = run_all(H, x, w, dy, stride)
        _, _, gdw = run_all(H, x, w, ones, stride)
        inside = np.zeros(c, bool)
        inside[g * cg:(g + 1) * cg] = True
        assert not np.any(host(gy)[:, :, ~inside]) and np.all(host(gy)[:, :, inside] > 0)
        assert not np.any(host(gdx)[:, :, ~inside]) and np.any(host(gdx)[:, :, inside] > 0)
        assert not np.any(host(gdw)[~inside]) and np.all(host(gdw)[inside].sum(2) > 0)


# ---- float operands at the six block shapes ---------------------------------------------------------------------------------
# (rows, L of the conv's input, width, stride) of conv2 in the six resnext_block_* goldens
BLOCK_CONV_SHAPES = [(4, 56, 128, 1), (4, 56, 128, 1), (6, 56, 256, 2), (6, 28, 512, 2), (5, 14, 1024, 2), (5, 7, 1024, 1)]


@pytest.mark.parametrize('i', range(6))
def test_float_operands_against_float64(H, i):
    rows, l, c, stride = BLOCK_CONV_SHAPES[i]
    rng = np.random.default_rng([31, i])
    f = np.float32
    x, dy = rng.standard_normal((rows, l, c)).astype(f), rng.standard_normal((rows, out_len(l, stride), c)).astype(f)
    w = (rng.standard_normal((c, c // GROUPS, 3)) / np.sqrt(3 * c // GROUPS)).astype(f)
    r64, r32 = ref_all(x, w, dy, stride), ref_all(x, w, dy, stride, torch.float32)
    got = run_all(H, x, w, dy, stride)
    bad = []
    for name, g, a, b in zip(('y', 'dx', 'dw'), got, r64, r32):
        check(sid(BLOCK_CONV_SHAPES[i]), name, g, a, R.rel_l2(b, a), bad)
    assert not bad, '\n'.join(bad)


# ---- accumulate and determinism ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(3, 14, 128, 2), (5, 7, 1024, 1), (2, 5, 512, 2)], ids=sid)
def test_accumulate_adds_exactly_and_runs_are_bit_equal(H, shape):
    rows, l, c, stride = shape
    x, w, dy, y, dx, dw = int_case(*shape)
    base_dx = np.ascontiguousarray(E.operand(21, rows, c, l, amp=2).transpose(0, 2, 1))
    base_dw = E.weight(22, c, c // GROUPS, 3, amp=2)
    xt, wt, dyt = cu(x), cu(w), cu(dy)
    gdx = H.gconv3_dgrad(dyt, wt, stride, l, out=cu(base_dx), accumulate=True)
    gdw = H.gconv3_wgrad(dyt, xt, stride, out=cu(base_dw), accumulate=True)
    assert np.array_equal(host(gdx), dx + base_dx) and np.array_equal(host(gdw), dw + base_dw)
    rng = np.random.default_rng(5)
    xf, wf, dyf = (cu(rng.standard_normal(a.shape)) for a in (x, w, dy))
    first = (H.gconv3_fwd(xf, wf, stride), H.gconv3_dgrad(dyf, wf, stride, l), H.gconv3_wgrad(dyf, xf, stride))
    again = (H.gconv3_fwd(xf, wf, stride), H.gconv3_dgrad(dyf, wf, stride, l), H.gconv3_wgrad(dyf, xf, stride))
    assert all(torch.equal(a, b) for a, b in zip(first, again))


# ---- memory discipline --------------------------------------------------------------------------------------------------------
WRAPPERS = ('gconv3_fwd', 'gconv3_dgrad', 'gconv3_wgrad')
OP_SHAPES = ((4, 9, 128, 1), (3, 17, 256, 2), (6, 7, 1024, 2))
N_OP_CASES = len(OP_SHAPES) * 3 + 1


def _op_cases(H):
    cases = []

    def operands(shape):
        rows, l, c, stride = shape
        rng = np.random.default_rng([41] + list(shape))
        return (cu(rng.standard_normal((rows, l, c))), cu(rng.standard_normal((c, c // GROUPS, 3))),
                cu(rng.standard_normal((rows, out_len(l, stride), c))))
    for shape in OP_SHAPES + ((70, 3, 128, 1),):                # the last: more than one chunk of weight-gradient partials
        rows, l, c, stride = shape
        tag = sid(shape)

        def b_fwd(shape=shape):
            x, w, dy = operands(shape)
            return dict(x=x, w=w, out=torch.zeros_like(dy))

        def b_dg(shape=shape):
            x, w, dy = operands(shape)
            return dict(dy=dy, w=w, out=torch.zeros_like(x))

        def b_wg(shape=shape):
            x, w, dy = operands(shape)
            return dict(dy=dy, x=x, out=torch.zeros_like(w))
        if shape in OP_SHAPES:
            cases.append(P.OpCase('gconv3_fwd_' + tag, 'gconv3', b_fwd, lambda x, w, out, s=stride: H.gconv3_fwd(x, w, s, out=out),
                                  dests=('out',), rows=dict(inputs=('x',), R=1, axis={})))
            cases.append(P.OpCase('gconv3_dgrad_' + tag, 'gconv3', b_dg,
                                  lambda dy, w, out, s=stride, l=l: H.gconv3_dgrad(dy, w, s, l, out=out),
                                  dests=('out',), rows=dict(inputs=('dy',), R=1, axis={})))
        cases.append(P.OpCase('gconv3_wgrad_' + tag, 'gconv3', b_wg, lambda dy, x, out, s=stride: H.gconv3_wgrad(dy, x, s, out=out),
                              dests=('out',), rows=None))
    return cases


CHECKS = {'uninitialised': P.check_uninitialised, 'guards': P.check_guards, 'dirty_out': P.check_dirty_out, 'isolation': P.check_isolation}


@pytest.mark.parametrize('check', sorted(CHECKS))
@pytest.mark.parametrize('i', range(N_OP_CASES))
def test_memory_discipline(H, i, check):
    cases = _op_cases(H)
    assert len(cases) == N_OP_CASES
    problems = CHECKS[check](cases[i])
    assert not problems, '\n'.join(problems)


def test_every_new_wrapper_has_a_memory_discipline_row(H):
    from deepards_amd import gconv_ops as G
    names = {c.name for c in _op_cases(H)}
    launching = sorted(n for n, f in vars(G).items() if callable(f) and n.startswith('gconv3_') and
                       n not in ('gconv3_ok', 'gconv3_plan', 'gconv3_out_len', 'gconv3_workspace_floats'))
    assert launching == sorted(WRAPPERS)
    assert all(getattr(H, n) is getattr(G, n) for n in WRAPPERS + ('gconv3_ok', 'gconv3_plan'))
    assert all(any(n.startswith(w + '_') for n in names) for w in WRAPPERS)
    p = G.gconv3_plan(WGRAD, 70, 3, 128, 1)
    assert p.grid[0] > 1, 'the multi-chunk row writes a single partial'


@pytest.mark.parametrize('c,stride,exc', [(96, 1, NotImplementedError), (64, 1, NotImplementedError), (2048, 2, NotImplementedError),
                                          (128, 3, NotImplementedError)], ids=['C=96', 'C=64', 'C=2048', 'stride=3'])
def test_refused_calls_touch_nothing(H, c, stride, exc):
    """An unsupported shape raises before any launch: poisoned destinations keep the pattern, guards and inputs are unchanged."""
    rows, l = 2, 6
    lo = out_len(l, stride)
    rng = np.random.default_rng(c)
    cg = max(c // GROUPS, 1)
    handles = []

    def g(t):
        v, h = P.guarded(t)
        handles.append(h)
        return v
    x, w, dy = g(cu(rng.standard_normal((rows, l, c)))), g(cu(rng.standard_normal((c, cg, 3)))), g(cu(rng.standard_normal((rows, lo, c))))
    keep = [t.clone() for t in (x, w, dy)]
    oy, odx, odw = (g(P.fill_poison(torch.empty_like(t))) for t in (dy, x, w))
    for call in (lambda: H.gconv3_fwd(x, w, stride, out=oy), lambda: H.gconv3_dgrad(dy, w, stride, l, out=odx),
                 lambda: H.gconv3_wgrad(dy, x, stride, out=odw)):
        with pytest.raises(exc):
            call()
    torch.cuda.synchronize()
    assert all(P.count_poison(t) == t.numel() for t in (oy, odx, odw))
    assert all(torch.equal(a, b) for a, b in zip(keep, (x, w, dy)))
    P.assert_guards_intact(handles)
    # wrong dtype, a transposed view, a weight of another layout, a CPU operand: ValueError, with the shape in the message
    x2, w2 = cu(rng.standard_normal((rows, l, 128))), cu(rng.standard_normal((128, 4, 3)))
    for bad_x, bad_w in ((x2.double(), w2), (x2.permute(1, 0, 2), w2), (x2, w2.permute(0, 2, 1).contiguous()), (x2.cpu(), w2)):
        with pytest.raises(ValueError):
            H.gconv3_fwd(bad_x, bad_w, 1)


# ---- the chained block ----------------------------------------------------------------------------------------------------
BLOCK_TAGS = ['e1_4x2x56x64', 'id_4x2x56x256', 's2_6x3x28x256', 's2_6x3x14x512', 's2_5x5x7x1024', 'id_5x5x7x2048']


@functools.lru_cache(maxsize=None)
def block_ref(tag):
    g = _gold('resnext_block_%s.npz' % tag)
    rows, R_, l_out, cin, planes, stride, ds, seed = (int(v) for v in g['cfg'])
    _, params, dout = R.block_draws(rows, R_, l_out, cin, planes, stride, bool(ds), seed)
    x = g['x']
    r = {k: v.numpy() for k, v in R.block_case(x, params, stride, R_, dout).items()}
    return g, x, params, dout, (cin, planes, stride, bool(ds), R_), r


@pytest.mark.parametrize('tag', BLOCK_TAGS)
def test_chained_block_function(H, M, tag):
    """SEBlockFunction on an SEResNeXtBottleneck through the module, forward and backward, against the oracle at the golden's
    err32; every ReLU decision (the two hidden maps through the decision tap, the output) must be the oracle's.  Then the
    same block inside a training step with gradient destinations on every parameter: the grouped weight gradient is written
    into its destination by its own launch, the others by the queued folds; same gradients at the same bound."""
    import deepards_amd.models.seresnext as X
    from deepards_amd import functional as F_
    g, x, params, dout, (cin, planes, stride, has_ds, R_), ref = block_ref(tag)
    m = {k: float(np.abs(ref['pre/' + k]).min()) for k in ('h1', 'h2', 'hid', 'out')}
    assert min(m.values()) >= R.MARGIN, m
    ds = None
    if has_ds:
        ds = torch.nn.Sequential(torch.nn.Conv1d(cin, planes * 4, kernel_size=1, stride=stride, bias=False), torch.nn.BatchNorm1d(planes * 4))
    blk = X.SEResNeXtBottleneck(cin, planes, 32, 16, stride, ds)
    assert not blk.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=False).unexpected_keys
    blk = blk.cuda().train()
    xt = cu(x).requires_grad_(True)
    F_.DECISION_TAP = taps = []
    try:
        out = blk.forward_rlc(xt, R_)
    finally:
        F_.DECISION_TAP = None
    out.backward(cu(dout))
    torch.cuda.synchronize()
    assert len(taps) == 3
    for t, k in zip(taps, ('h1', 'h2', 'out')):
        assert np.array_equal(host(t) > 0, ref['pre/' + k] > 0), 'ReLU decisions of %s differ from the oracle\'s' % k
    bad = []
    check(tag, 'out', out, ref['out'], float(g['err32/out']), bad)
    check(tag, 'dx', xt.grad, ref['dx'], float(g['err32/dx']), bad)
    for n, q in blk.named_parameters():
        check(tag, 'grad/' + n, q.grad, ref['grad/' + n], float(g['err32/grad/' + n]), bad)
    assert not bad, '\n'.join(bad)
    for n, q in blk.named_parameters():
        q.grad = None
        q._da_grad = torch.zeros_like(q)
    xs = cu(x).requires_grad_(True)
    try:
        with F_.training_step(blk):
            o2 = blk.forward_rlc(xs, R_)
            F_.flush_forward(defer=True)
            o2.backward(cu(dout))
            F_.flush_backward()
        torch.cuda.synchronize()
    finally:
        dests = {n: q.__dict__.pop('_da_grad') for n, q in blk.named_parameters()}
    assert torch.equal(o2, out) and all(q.grad is None for q in blk.parameters())
    check(tag + ' step', 'dx', xs.grad, ref['dx'], float(g['err32/dx']), bad)
    for n in dests:
        check(tag + ' step', 'grad/' + n, dests[n], ref['grad/' + n], float(g['err32/grad/' + n]), bad)
    assert not bad, '\n'.join(bad)
    w = x.shape[0] // R_
    bns = [blk.bn1, blk.bn2, blk.bn3] + ([blk.downsample[1]] if has_ds else [])
    assert all(int(b.num_batches_tracked) == 2 * w for b in bns)


# ---- the whole model -----------------------------------------------------------------------------------------------------
def build_model(M, g, net='se_resnext50_32x4d', head='linear'):
    nb = int(g['nb'])
    bb = getattr(M, net)()
    model = M.CNNLinearNetwork(bb, nb, 0) if head == 'linear' else M.CNNSingleBreathLinearNetwork(bb)
    params = R.seeded_params(net, int(g['seed']), nb, bn_bias_shift=float(g['bn_bias_shift']), fc1_bias_shift=float(g['fc1_bias_shift']))
    sd = {k: torch.from_numpy(v) for k, v in params.items() if head == 'linear' or k.startswith('breath_block.')}
    assert not model.load_state_dict(sd, strict=False).unexpected_keys
    return model.cuda().train(), params


class _NoTape(object):
    """The tape of an oracle whose input was moved until no decision is ambiguous: nothing to flip."""
    order, decisions = (), {}


def test_whole_model_gradients_against_the_golden(M):
    """CNNLinearNetwork(se_resnext50_32x4d(), 2, 0) at B = 2 with the shifted biases on the decided input: logits and loss
    against the golden, every parameter gradient through decision_match.assert_gradients_match against the float64
    restatement (tests/test_resnext_cpu.py pins that to the golden's digests) with the golden's err32 per tensor; the golden
    lists at most 4 tensors above 2.5e-5 (``unpinned``)."""
    from deepards_amd import functional as F_
    g = _gold('resnext_model_se_resnext50_32x4d_b2_grads.npz')
    model, params = build_model(M, g)
    assert list(model.state_dict().keys()) == [str(n) for n in g['names']]
    x, t = torch.from_numpy(g['x']).cuda(), torch.from_numpy(g['target']).cuda()
    out = model(x, None)
    assert out.shape == (2, 2)
    loss = F_.bce_with_logits(out, t)
    loss.backward()
    bad = []
    check('model', 'logits', out, g['logits'], float(g['err32/logits']), bad)
    check('model', 'loss', loss, g['loss'], float(g['err32/loss']), bad)
    assert not bad, '\n'.join(bad)
    unpinned = {str(n) for n in g['unpinned']}
    assert len(unpinned) <= 4 and len(list(model.named_parameters())) == 225
    r64 = R.model_case('se_resnext50_32x4d', g['x'], g['target'], params)
    r32 = R.model_case('se_resnext50_32x4d', g['x'], g['target'], params, dtype=torch.float32)
    grads = {k[5:]: v.numpy() for k, v in r64.items() if k.startswith('grad/')}
    noise = {None: 0}
    for n, e in grads.items():
        key = 'grad/' + n
        d = digest(e) if 'dig/' + key in g else e                       # the in-test oracle IS the golden's, tensor by tensor
        stored = g['dig/' + key] if 'dig/' + key in g else g[key]
        assert R.rel_l2(d.reshape(stored.shape), stored) <= max(8 * float(g['err32/' + key]), FLOOR), key
        g32 = r32[key].double().numpy()
        noise[n] = dict(err32=float(g['err32/' + key]), abs=float(np.linalg.norm(g32 - e)), norm=float(np.linalg.norm(e)))
    ref = dict(grads=grads, tape=_NoTape(), rebackward=lambda flips: grads)
    ours = {n: host(q.grad) for n, q in model.named_parameters()}
    assert set(ours) == set(grads)
    # (active: the +2 shifts leave every ReLU active, the case the yardstick's own cap of 2 unpinned tensors does not cover;
    # the cap here is the golden's 4, counted by the yardstick's rule 8 err32 > 1e-4 as well)
    assert sum(DM.MARGIN * v['err32'] > DM.NORTH_STAR for k, v in noise.items() if k is not None) <= 4
    DM.assert_gradients_match(ref, ours, noise, tag='se_resnext50_32x4d b2', strict=True, max_flips=0, log=log, active=True)


@pytest.mark.parametrize('name,net', [('resnext_model_se_resnext50_32x4d_nb20.npz', 'se_resnext50_32x4d'),
                                      ('resnext_model_se_resnext101_32x4d_nb2_shifted.npz', 'se_resnext101_32x4d')])
def test_whole_model_logits_and_loss(M, name, net):
    from deepards_amd import functional as F_
    g = _gold(name)
    model, _ = build_model(M, g, net)
    assert list(model.state_dict().keys()) == [str(n) for n in g['names']]
    with torch.no_grad():
        out = model(torch.from_numpy(g['x']).cuda(), None)
        loss = F_.bce_with_logits(out, torch.from_numpy(g['target']).cuda())
    bad = []
    check(name, 'logits', out, g['logits'], float(g['err32/logits']), bad)
    check(name, 'loss', loss, g['loss'], float(g['err32/loss']), bad)
    assert not bad, '\n'.join(bad)


# ---- trainer -----------------------------------------------------------------------------------------------------------------
def test_trainer_eager_and_captured_steps_are_bit_equal(M):
    """se_resnext50_32x4d at B = 2, NB = 2: four eager steps against the eager first step plus THREE replays of the captured
    step leave the same losses, parameters and optimiser state, bit for bit; every grouped conv weight moved."""
    from deepards_amd.train import HotPathTrainer
    g = _gold('resnext_model_se_resnext50_32x4d_b2_grads.npz')
    x, t = torch.from_numpy(g['x']).cuda(), torch.from_numpy(g['target']).cuda()
    runs = []
    for use_graph in (False, True):
        model, _ = build_model(M, g)
        start = {n: q.detach().clone() for n, q in model.named_parameters()}
        tr = HotPathTrainer(model, optimizer='sgd', use_graph=use_graph)
        losses = []
        for step in range(4):
            losses.append(tr.train_step(x, t).detach().clone().reshape(-1))
            assert len(tr._graphs) == (1 if use_graph and step >= 1 else 0)      # step 0 is the eager first step, then replays
        losses = torch.cat(losses)
        if use_graph:
            assert tr.grad_overwrite, 'a gradient writer without an overwrite form ran: the capture fell back to the zero-fill'
        runs.append((losses, tr.bucket.p.clone(), {k: v.clone() for k, v in tr.state.items()}))
        moved = {n: float((q.detach() - start[n]).abs().max()) for n, q in model.named_parameters() if n.endswith('conv2.weight')}
        assert len(moved) == 16 and min(moved.values()) > 0, 'grouped weights that did not move: %s' % [n for n, v in moved.items() if v == 0]
        if use_graph:
            tr.release_graphs()
    assert torch.isfinite(runs[0][0]).all()
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert set(runs[0][2]) == set(runs[1][2])
    assert all(torch.equal(runs[0][2][k], runs[1][2][k]) for k in runs[0][2])


def test_one_captured_step_on_se_resnext101(M):
    """33 blocks in one graph: with learning rate and weight decay 0 the eager first step leaves the golden's parameters where
    they are, the second call captures and replays, and the REPLAY's own logits and loss are held to the bound; a second
    replay gives the same bits."""
    from deepards_amd.train import HotPathTrainer
    g = _gold('resnext_model_se_resnext101_32x4d_nb2_shifted.npz')
    x, t = torch.from_numpy(g['x']).cuda(), torch.from_numpy(g['target']).cuda()
    model, _ = build_model(M, g, 'se_resnext101_32x4d')
    tr = HotPathTrainer(model, optimizer='sgd', learning_rate=0.0, weight_decay=0.0, use_graph=True)
    tr.train_step(x, t)
    assert not tr._graphs
    p0 = tr.bucket.p.clone()
    bad = []
    for replay in (1, 2):
        loss = tr.train_step(x, t)
        assert len(tr._graphs) == 1 and tr.grad_overwrite
        assert torch.equal(tr.bucket.p, p0)
        check('se_resnext101 replay %d' % replay, 'logits', tr.last_logits, g['logits'], float(g['err32/logits']), bad)
        check('se_resnext101 replay %d' % replay, 'loss', loss, g['loss'], float(g['err32/loss']), bad)
        if replay == 1:
            first = (loss.detach().clone(), tr.last_logits.detach().clone(), tr.bucket.g.clone())
    assert not bad, '\n'.join(bad)
    assert torch.equal(first[0], loss) and torch.equal(first[1], tr.last_logits) and torch.equal(first[2], tr.bucket.g)
    assert torch.isfinite(tr.bucket.g).all() and float(tr.bucket.g.abs().max()) > 0
    tr.release_graphs()


def test_per_breath_head_with_the_confidence_loss(M):
    from deepards_amd.train import HotPathTrainer
    g = _gold('resnext_model_se_resnext50_32x4d_b2_grads.npz')
    x, t = torch.from_numpy(g['x']).cuda(), torch.from_numpy(g['target']).cuda()
    tr = HotPathTrainer(build_model(M, g, head='single_breath')[0], use_graph=False, loss='confidence', loss_param=0.5)
    assert torch.isfinite(tr.train_step(x, t)).all()


# ---- unchanged paths ---------------------------------------------------------------------------------------------------------
def test_se_resnet50_block_keeps_its_bits_through_both_unit_forms(H, M):
    """The SE-ResNet bottleneck through the three-field units (the form its module hands in) against the SAME block with every
    unit spelt out as (k, precise, BNState, stride, groups): output, dx and every gradient bit for bit, on the stride-2
    chained-block golden of se_resnet50 -- and the three-field form still meets that golden at its bound."""
    from deepards_amd import functional as F_
    g = _gold('sebn_block_s2_6x3x28x512.npz')
    rows, R_, l_out, cin, planes, stride, ds, seed = (int(v) for v in g['cfg'])
    _, params, dout = sebn_ref.block_draws(rows, R_, l_out, cin, planes, stride, bool(ds), seed)
    dsm = torch.nn.Sequential(torch.nn.Conv1d(cin, planes * 4, kernel_size=1, stride=stride, bias=False), torch.nn.BatchNorm1d(planes * 4))
    blk = M.SEResNetBottleneck(cin, planes, 1, 16, stride, dsm)
    assert not blk.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=False).unexpected_keys
    blk = blk.cuda().train()

    def run(spell):
        units = [(blk.conv1, blk.bn1, False), (blk.conv2, blk.bn2, True), (blk.conv3, blk.bn3, False)]
        se, fam = blk.se_module, H.se_gate_family(blk.se_module.fc1.in_channels, blk.se_module.fc1.out_channels)
        ps = [t for conv, bn, _ in units for t in (conv.weight, bn.weight, bn.bias)]
        ps += [se.fc1.weight, se.fc1.bias, se.fc2.weight, se.fc2.bias, dsm[0].weight, dsm[1].weight, dsm[1].bias]
        us = [(conv.kernel_size[0], pr, F_.BNState(bn)) + ((conv.stride[0], 1) if spell else ()) for conv, bn, pr in units]
        xt = cu(g['x']).requires_grad_(True)
        out = F_.SEBlockFunction.apply(xt, stride, R_, fam, us, F_.BNState(dsm[1]), *ps)
        grads = torch.autograd.grad(out, [xt] + ps, cu(dout))
        torch.cuda.synchronize()
        return [out.detach()] + [t.detach() for t in grads]
    old, new = run(False), run(True)
    assert digest(host(old[0])).tobytes() == digest(host(new[0])).tobytes()
    assert all(torch.equal(a, b) for a, b in zip(old, new))
    ref = sebn_ref.block_case(g['x'], params, stride, R_, dout)
    bad = []
    check('se_resnet50 s2', 'out', old[0], ref['out'].numpy(), float(g['err32/out']), bad)
    check('se_resnet50 s2', 'dx', old[1], ref['dx'].numpy(), float(g['err32/dx']), bad)
    assert not bad, '\n'.join(bad)
