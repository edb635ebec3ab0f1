"""The vgg11 / vgg13 backbones on the GPU: the fused BatchNorm-ReLU-MaxPool(2) kernels and the adaptive-pool feature kernels
(csrc/vgg.hip), VGGStageFunction with a non-zero conv bias, the whole model, the trainer and the driver.

Bound per tensor (the one of tests/test_se_gpu.py): rel-l2 against the float64 oracle <= min(max(4 err32, 16 2^-23), 1e-4),
err32 = the reference's own fp32-against-fp64 rel-l2 from the golden where the shape has one, else tests/tools/vgg_ref.py
evaluated in float32 on the CPU.  The kernel and stage cases keep every ReLU pre-activation, and every gap of a pool pair that
is not both negative, at least 1e-3 from zero in float64 (asserted here, on the CPU): no element is left out of a comparison.
The stage cases compare against vgg_ref's float64 evaluation, element by element; tests/test_vgg_cpu.py shows that evaluation to
be the reference's (the golden's digests).  Figures: pytest -s."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'tools'))
pytestmark = pytest.mark.gpu

from oracle.weights import digest  # noqa: E402
import vgg_ref as R  # noqa: E402
import poison as P  # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
FLOOR, CEIL = 16 * 2.0 ** -23, 1e-4
# (rows, R, L, C) of the pooled tail alone: L = 2 (one pair) and odd lengths 3, 7, 15 (a dropped position), the four channel
# counts, an odd R, and windows of 1400 positions (two-stage statistics, 3 chunks of pairs per window in the backward)
TAIL_SHAPES = [(4, 2, 2, 64), (6, 3, 3, 128), (4, 2, 7, 256), (6, 3, 15, 256), (4, 2, 14, 512), (4, 2, 700, 128), (8, 4, 224, 64)]
STAGE_TAGS = ['s64_64p_2', 's64_128p_3', 's256_256p_7', 's128_256_15', 's128_256p_15', 's512_512p_14', 's512_512_14', 's64_128p_700',
              'first_224p', 'first_30p', 'first_30']
POOL_SHAPES = [(3, 7, 32), (3, 16, 512), (2, 3, 64), (2, 8, 64), (2, 14, 96)]          # (rows, Lin, C) -> 7 positions


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
    log('%s %-22s rel-l2 %.3e  reference fp32 %.3e  bound %.3e' % (tag, name, e, err32, bd))
    if not e <= bd:
        problems.append('%s %s: rel-l2 %.3e > bound %.3e (reference fp32 %.3e)' % (tag, name, e, bd, err32))


# ---- the pooled tail, each kernel alone ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tail_ref(shape):
    """(case, float64 oracle, err32 per tensor) of one tail shape, computed once."""
    rows, R_, l, c = shape
    case = R.tail_inputs(rows, R_, l, c, seed=3)
    r64 = {k: v.numpy() for k, v in R.stage_tail(R=R_, pool=True, **case).items()}
    r32 = R.stage_tail(R=R_, pool=True, dtype=torch.float32, **case)
    err = {k: R.rel_l2(r32[k].double().numpy(), r64[k]) for k in r64}
    if l % 2:                       # the position the pool drops, on its own
        err['dy_last'] = R.rel_l2(r32['dy'][:, -1].double().numpy(), r64['dy'][:, -1])
    return case, r64, err


@pytest.mark.parametrize('shape', TAIL_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_pool_kernels_alone_against_the_oracle(H, shape):
    rows, R_, l, c = shape
    case, ref, err = tail_ref(shape)
    mz, mg = R.decision_margins(ref['z'], True)
    assert mz >= R.MARGIN and mg >= R.MARGIN, (mz, mg)
    g = {k: cu(v) for k, v in case.items()}
    tag, bad = 'x'.join(map(str, shape)), []
    mean, invstd = H.vgg_stats(g['y'], R_)
    check(tag, 'mean', mean, ref['mean'], err['mean'], bad)
    check(tag, 'invstd', invstd, ref['invstd'], err['invstd'], bad)
    # each kernel on the ORACLE's statistics (rounded to float): its own error alone
    mean, invstd = cu(ref['mean']), cu(ref['invstd'])
    out = H.bn_relu_maxpool2_fwd(g['y'], R_, mean, invstd, g['gamma'], g['beta'])
    assert tuple(out.shape) == (rows, l // 2, c)
    check(tag, 'out', out, ref['out'], err['out'], bad)
    assert np.array_equal(host(out) > 0, ref['out'] > 0)
    dy, ds = H.bn_relu_maxpool2_bwd(g['dout'], g['y'], R_, mean, invstd, g['gamma'], g['beta'])
    check(tag, 'dy', dy, ref['dy'], err['dy'], bad)
    check(tag, 'ds1', ds[0], ref['ds1'], err['ds1'], bad)
    check(tag, 'ds2', ds[1], ref['ds2'], err['ds2'], bad)
    if l % 2:                       # the dropped position: no gradient arrives there, yet dy is not zero
        assert float(np.abs(ref['dz'][:, -1]).max()) == 0 and float(np.abs(ref['dy'][:, -1]).min()) > 0
        check(tag, 'dy[:, -1]', dy[:, -1], ref['dy'][:, -1], err['dy_last'], bad)
    dgamma, dbeta = torch.empty(c, device='cuda'), torch.empty(c, device='cuda')
    H.bn_param_grad_multi([(ds, dgamma, dbeta)], accumulate=False)
    check(tag, 'dgamma', dgamma, ref['dgamma'], err['dgamma'], bad)
    check(tag, 'dbeta', dbeta, ref['dbeta'], err['dbeta'], bad)
    dy2, ds2 = H.bn_relu_maxpool2_bwd(g['dout'], g['y'], R_, mean, invstd, g['gamma'], g['beta'])
    assert torch.equal(dy, dy2) and torch.equal(ds, ds2)                     # fixed summation order
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('shape', [(4, 2, 6, 32), (6, 3, 9, 64), (2, 1, 35, 32)], ids=lambda s: 'x'.join(map(str, s)))
def test_pool_routing_on_integers(H, shape):
    """Integer y / dout with mean 0, invstd 1, gamma in {+-1, +-2}, integer beta: z is exact, so the pooled output is compared
    with array_equal, and so is the routing -- ties included: an equal positive pair sends its gradient to the FIRST member,
    a pair of two non-positive members sends it nowhere.  The routed dz is read back from dy = gamma (dz - s1 / n - y s2 / n)
    (s1, s2: the kernel's own window sums, themselves exact integers here)."""
    rows, R_, l, c = shape
    rng = np.random.default_rng([rows, l, c])
    y = rng.integers(-3, 4, (rows, l, c)).astype(np.float32)
    y[:, 1] = y[:, 0]                                     # ties in the first pair of every row: positive, zero and negative ones
    gamma = rng.choice([-2.0, -1.0, 1.0, 2.0], c).astype(np.float32)
    beta = rng.integers(-1, 2, c).astype(np.float32)
    dout = rng.integers(1, 9, (rows, l // 2, c)).astype(np.float32)
    z = y.astype(np.float64) * gamma + beta
    lo = l // 2
    pr = np.maximum(z[:, :lo * 2], 0).reshape(rows, lo, 2, c)
    first = pr[:, :, 0] >= pr[:, :, 1]
    assert int((pr[:, :, 0] == pr[:, :, 1]).sum()) > rows and int(((pr[:, :, 0] == pr[:, :, 1]) & (pr[:, :, 0] > 0)).sum()) > 0
    dz = np.zeros((rows, l, c))
    dzp = dz[:, :lo * 2].reshape(rows, lo, 2, c)
    dzp[:, :, 0] = np.where(first & (pr[:, :, 0] > 0), dout, 0)
    dzp[:, :, 1] = np.where(~first, dout, 0)
    dz[:, :lo * 2] = dzp.reshape(rows, lo * 2, c)
    w = rows // R_
    mean, invstd = torch.zeros(w, c, device='cuda'), torch.ones(w, c, device='cuda')
    out = H.bn_relu_maxpool2_fwd(cu(y), R_, mean, invstd, cu(gamma), cu(beta))
    assert np.array_equal(host(out), pr.max(2))
    dy, ds = H.bn_relu_maxpool2_bwd(cu(dout), cu(y), R_, mean, invstd, cu(gamma), cu(beta))
    s1, s2 = dz.reshape(w, R_ * l, c).sum(1), (dz * y).reshape(w, R_ * l, c).sum(1)
    assert np.array_equal(host(ds[0]), s1) and np.array_equal(host(ds[1]), s2)
    n = R_ * l
    back = host(dy) / gamma + np.repeat(s1, R_, 0)[:, None, :] / n + y * np.repeat(s2, R_, 0)[:, None, :] / n
    assert float(np.abs(back - np.rint(back)).max()) < 1e-3
    assert np.array_equal(np.rint(back), dz)


def test_unsupported_shapes_are_refused(H):
    L = H._lib.lib()
    t = torch.zeros(4, 4, 64, device='cuda')
    s = torch.zeros(2, 64, device='cuda')
    v = torch.zeros(64, device='cuda')
    o = torch.zeros(4, 2, 64, device='cuda')
    ok = lambda rows, R_, l, c, ld: L.da_bn_relu_maxpool2_fwd(H._p(t), ld, H._p(o), rows, R_, l, c, H._p(s), H._p(s), H._p(v), H._p(v), H._stream())
    assert ok(4, 2, 2, 32, 32) == 0
    for args in ((4, 2, 1, 32, 32), (4, 2, 2, 48, 48), (4, 3, 2, 32, 32), (4, 2, 2, 32, 16), (1 << 20, 2, 1 << 10, 32, 32)):
        assert ok(*args) == -1, args
    d, ws = torch.zeros(4, 4, 64, device='cuda'), torch.zeros(1024, device='cuda')
    bw = lambda rows, R_, l, c: L.da_bn_relu_maxpool2_bwd(H._p(o), H._p(t), c, H._p(d), H._p(s), H._p(ws), rows, R_, l, c, H._p(s), H._p(s),
                                                          H._p(v), H._p(v), H._stream())
    for args in ((4, 2, 1, 32), (4, 2, 2, 40), (1 << 20, 2, 1 << 10, 32)):
        assert bw(*args) == -1, args
    assert L.da_adaptive_avgpool_flat_fwd(H._p(t), H._p(d), 1 << 20, 1 << 10, 7, 32, H._stream()) == -1
    assert L.da_adaptive_avgpool_flat_bwd(H._p(t), H._p(d), 2, 0, 7, 32, H._stream()) == -1
    with pytest.raises(ValueError):
        H.bn_relu_maxpool2_fwd(torch.zeros(4, 1, 64, device='cuda'), 2, s, s, v, v)
    with pytest.raises(ValueError):
        H.bn_relu_maxpool2_fwd(torch.zeros(4, 4, 48, device='cuda'), 2, s[:, :48].contiguous(), s[:, :48].contiguous(), v[:48], v[:48])


# ---- AdaptiveAvgPool1d(7) + view ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pool_ref(shape):
    rows, lin, c = shape
    rng = np.random.default_rng([rows, lin, c, 4])
    x, dfeat = rng.standard_normal((rows, lin, c)).astype(np.float32), rng.standard_normal((rows, c * 7)).astype(np.float32)
    r64 = {k: v.numpy() for k, v in R.adaptive_pool_case(x, 7, dfeat).items()}
    r32 = R.adaptive_pool_case(x, 7, dfeat, dtype=torch.float32)
    return x, dfeat, r64, {k: R.rel_l2(r32[k].double().numpy(), r64[k]) for k in r64}


@pytest.mark.parametrize('shape', POOL_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_adaptive_pool_flat(H, shape):
    x, dfeat, ref, err = pool_ref(shape)
    bad = []
    feat = H.adaptive_avgpool_flat_fwd(cu(x), 7)
    assert tuple(feat.shape) == (shape[0], shape[2] * 7)
    check(str(shape), 'feat', feat, ref['feat'], err['feat'], bad)
    dx = H.adaptive_avgpool_flat_bwd(cu(dfeat), shape[1], 7)
    check(str(shape), 'dx', dx, ref['dx'], err['dx'], bad)
    if shape[1] == 7:               # the identity pool: the transposing copy, bit for bit
        assert torch.equal(feat, cu(x).permute(0, 2, 1).reshape(shape[0], -1)) and torch.equal(dx, cu(dfeat).view(shape[0], -1, 7).permute(0, 2, 1))
    assert not bad, '\n'.join(bad)


# ---- one stage through VGGStageFunction, non-zero conv bias ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stage_ref(tag):
    g = _gold('vgg_stage_cases.npz')
    rows, R_, lin, cin, c, pool, seed = (int(v) for v in g[tag + '/cfg'])
    x = g[tag + '/x'] if tag + '/x' in g else _gold('vgg_stage_x700.npz')[tag + '/x']
    p, dout = R.stage_params(cin, c, seed), R.stage_dout(rows, lin, c, pool, seed)
    r64 = {k: v.numpy() for k, v in R.stage_case(x, p, R_, bool(pool), dout).items()}
    return (rows, R_, lin, cin, c, bool(pool)), x, p, dout, r64, {k: float(g['err32/%s/%s' % (tag, k)]) for k in r64 if k != 'z'}


@pytest.mark.parametrize('tag', STAGE_TAGS)
def test_stage_function(H, tag):
    from deepards_amd import functional as F_
    (rows, R_, lin, cin, c, pool), x, p, dout, ref, err = stage_ref(tag)
    mz, mg = R.decision_margins(ref['z'], pool)
    assert mz >= R.MARGIN and mg >= R.MARGIN, (mz, mg)
    first = cin == 1
    bn = torch.nn.BatchNorm1d(c).cuda()
    w, b, gamma, beta = (cu(p[k]).requires_grad_(True) for k in ('w', 'b', 'gamma', 'beta'))
    xt = cu(x).reshape(rows, lin) if first else cu(x).requires_grad_(True)
    from deepards_amd.models import vgg as V
    out = F_.VGGStageFunction.apply(xt, w, b, gamma, beta, R_, F_.BNState(bn), pool, first, min(cin, c) >= V.PRECISE_MIN_C)
    out.backward(cu(dout))
    bad = []
    check(tag, 'out', out, ref['out'], err['out'], bad)
    if not first:
        check(tag, 'dx', xt.grad, ref['dx'], err['dx'], bad)
    check(tag, 'dw', w.grad, ref['dw'], err['dw'], bad)
    check(tag, 'dgamma', gamma.grad, ref['dgamma'], err['dgamma'], bad)
    check(tag, 'dbeta', beta.grad, ref['dbeta'], err['dbeta'], bad)
    # the conv bias: its gradient is exactly 0, and the running mean is that of conv + b
    assert b.grad is not None and tuple(b.grad.shape) == (c,) and float(b.grad.abs().max()) == 0
    check(tag, 'running_mean', bn.running_mean, ref['running_mean'], err['running_mean'], bad)
    check(tag, 'running_var', bn.running_var, ref['running_var'], err['running_var'], bad)
    assert int(bn.num_batches_tracked) == rows // R_
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('overwrite', [False, True], ids=['accumulate', 'overwrite'])
@pytest.mark.parametrize('tag', ['s256_256p_7', 's128_256_15', 's128_256p_15', 's512_512p_14', 's512_512_14', 'first_224p'])
def test_stage_inside_a_training_step(H, tag, overwrite):
    """The stage inside ``training_step`` with gradient destinations on every parameter, against the same oracle at the same
    bound: the weight packed by the step's batched repack (F(2,3) for the 512-channel convs), the weight gradient through the
    batched launch and its chained reduction, dgamma / dbeta and the ``mean + b`` running update through the step's tail launch.
    accumulate: zero-filled destinations, as in a step that clears its bucket.  overwrite (``grad_overwrite``, a step captured
    without the zero-fill): destinations full of 7s -- every one, the conv bias's exact 0 included, must be written."""
    from deepards_amd import functional as F_
    from deepards_amd.models import vgg as V
    (rows, R_, lin, cin, c, pool), x, p, dout, ref, err = stage_ref(tag)
    first = cin == 1
    conv, bn = torch.nn.Conv1d(cin, c, 3, padding=1), torch.nn.BatchNorm1d(c)
    conv.precise_conv = min(cin, c) >= V.PRECISE_MIN_C
    net = torch.nn.Sequential(conv, bn).cuda().train()
    with torch.no_grad():
        for q, k in ((conv.weight, 'w'), (conv.bias, 'b'), (bn.weight, 'gamma'), (bn.bias, 'beta')):
            q.copy_(cu(p[k]))
    dests = {}
    for n, q in net.named_parameters():
        dests[n] = q._da_grad = torch.full_like(q, 7.0 if overwrite else 0.0)
    xt = cu(x).reshape(rows, lin) if first else cu(x).requires_grad_(True)
    try:
        F_.grad_overwrite(overwrite)
        with F_.training_step(net):
            out = F_.VGGStageFunction.apply(xt, conv.weight, conv.bias, bn.weight, bn.bias, R_, F_.BNState(bn), pool, first, conv.precise_conv)
            F_.flush_forward(defer=True)
            out.backward(cu(dout))
            F_.flush_backward()
        torch.cuda.synchronize()
    finally:
        F_.grad_overwrite(False)
        for q in net.parameters():
            q.__dict__.pop('_da_grad', None)
    assert all(q.grad is None for q in net.parameters())
    bad, name = [], tag + (' overwrite' if overwrite else ' step')
    check(name, 'out', out, ref['out'], err['out'], bad)
    if not first:
        check(name, 'dx', xt.grad, ref['dx'], err['dx'], bad)
    check(name, 'dw', dests['0.weight'], ref['dw'], err['dw'], bad)
    check(name, 'dgamma', dests['1.weight'], ref['dgamma'], err['dgamma'], bad)
    check(name, 'dbeta', dests['1.bias'], ref['dbeta'], err['dbeta'], bad)
    assert float(dests['0.bias'].abs().max()) == 0
    check(name, 'running_mean', bn.running_mean, ref['running_mean'], err['running_mean'], bad)
    check(name, 'running_var', bn.running_var, ref['running_var'], err['running_var'], bad)
    assert int(bn.num_batches_tracked) == rows // R_
    assert not bad, '\n'.join(bad)


# ---- memory discipline ---------------------------------------------------------------------------------------------------------
def _op_cases(H):
    cases = []
    for shape in (TAIL_SHAPES[2], TAIL_SHAPES[5]):
        rows, R_, l, c = shape
        tag = 'x'.join(map(str, shape))

        def b_fwd(shape=shape):
            case, _, _ = tail_ref(shape)
            return dict(y=cu(case['y']), gamma=cu(case['gamma']), beta=cu(case['beta']),
                        out=torch.zeros(shape[0], shape[2] // 2, shape[3], device='cuda'))

        def c_fwd(y, gamma, beta, out, R_=R_):
            mean, invstd = H.vgg_stats(y, R_)
            return dict(mean=mean, invstd=invstd, out=H.bn_relu_maxpool2_fwd(y, R_, mean, invstd, gamma, beta, out=out))
        cases.append(P.OpCase('bn_relu_maxpool2_fwd_' + tag, 'vgg', b_fwd, c_fwd, dests=('out',), rows=dict(inputs=('y',), R=R_, axis={})))

        def b_bwd(shape=shape):
            case, _, _ = tail_ref(shape)
            return dict(dout=cu(case['dout']), y=cu(case['y']), gamma=cu(case['gamma']), beta=cu(case['beta']), out=torch.zeros_like(cu(case['y'])))

        def c_bwd(dout, y, gamma, beta, out, R_=R_):
            mean, invstd = H.vgg_stats(y, R_)
            dy, ds = H.bn_relu_maxpool2_bwd(dout, y, R_, mean, invstd, gamma, beta, out=out)
            return dict(dy=dy, ds=ds)
        cases.append(P.OpCase('bn_relu_maxpool2_bwd_' + tag, 'vgg', b_bwd, c_bwd, dests=('out',),
                              rows=dict(inputs=('dout', 'y'), R=R_, axis={'ds': 1})))
    for shape in (POOL_SHAPES[1], POOL_SHAPES[2]):
        rows, lin, c = shape
        tag = 'x'.join(map(str, shape))

        def b_ap(shape=shape):
            x, dfeat, _, _ = pool_ref(shape)
            return dict(x=cu(x), dfeat=cu(dfeat), out=torch.zeros(shape[0], shape[2] * 7, device='cuda'), dx=torch.zeros_like(cu(x)))

        def c_ap(x, dfeat, out, dx, lin=lin):
            return dict(feat=H.adaptive_avgpool_flat_fwd(x, 7, out=out), dx=H.adaptive_avgpool_flat_bwd(dfeat, lin, 7, out=dx))
        cases.append(P.OpCase('adaptive_avgpool_flat_' + tag, 'vgg', b_ap, c_ap, dests=('out', 'dx'),
                              rows=dict(inputs=('x', 'dfeat'), R=1, axis={})))
    mshape = (6, 64)

    def b_mb():
        rng = np.random.default_rng(8)
        return dict(mean=cu(rng.standard_normal(mshape)), bias=cu(rng.standard_normal(mshape[1])), dbias=torch.zeros(mshape[1], device='cuda'))
    cases.append(P.OpCase('bn_mean_bias', 'vgg', b_mb, lambda mean, bias, dbias: dict(mean_b=H.bn_mean_bias(mean, bias, dbias=dbias), dbias=dbias),
                          dests=('dbias',), rows=dict(inputs=('mean',), R=1, axis={'dbias': None})))
    return cases


CHECKS = {'uninitialised': P.check_uninitialised, 'guards': P.check_guards, 'dirty_out': P.check_dirty_out, 'isolation': P.check_isolation}
N_OP_CASES = 7


@pytest.mark.parametrize('check', sorted(CHECKS))
@pytest.mark.parametrize('i', range(N_OP_CASES))
def test_memory_discipline(H, i, check):
    cases = _op_cases(H)
    assert len(cases) == N_OP_CASES
    problems = CHECKS[check](cases[i])
    assert not problems, '\n'.join(problems)


# ---- the whole model -----------------------------------------------------------------------------------------------------------
def build_model(M, g, arch='vgg11', nb=20, head='linear'):
    bb = M.base_networks[arch]()
    model = M.CNNLinearNetwork(bb, nb, 0) if head == 'linear' else M.CNNSingleBreathLinearNetwork(bb)
    params = R.seeded_vgg_params(arch, int(g['seed']), nb, bn_bias_shift=float(g['bn_bias_shift']))
    sd = {k: torch.from_numpy(v) for k, v in params.items() if head == 'linear' or k.startswith('breath_block.')}
    assert not model.load_state_dict(sd, strict=False).unexpected_keys
    return model.cuda().train()


@pytest.mark.parametrize('nb', [1, 4])
def test_whole_model_against_the_margin_goldens(M, nb):
    """CNNLinearNetwork(vgg11_bn(), nb, 0) at B = 2, BatchNorm betas + 2, NON-zero conv biases: logits, loss and every parameter
    gradient (digests).  Each golden's seed is one whose reference fp32 run takes every ReLU / pool decision as its float64 run
    does.  nb = 1 (200 704 decisions): the smallest margin is 8 x that run's fp32 error, as asked.  nb = 4 (802 816): no seed
    walked reaches 8 x; the file records the 4.6 / 2.9 its seed has (``margin_ratio``)."""
    from deepards_amd import functional as F_
    g = _gold('vgg_model_vgg11_nb%d.npz' % nb)
    model = build_model(M, g, nb=nb)
    assert list(model.state_dict().keys()) == [str(n) for n in g['names']]
    x, t = torch.from_numpy(g['x']).cuda(), torch.from_numpy(g['target']).cuda()
    out = model(x, None)
    assert out.shape == (2, 2)
    loss = F_.bce_with_logits(out, t)
    loss.backward()
    bad = []
    check('model', 'logits', out, g['logits'], float(g['err32/logits']), bad)
    check('model', 'loss', loss, g['loss'], float(g['err32/loss']), bad)
    for n, q in model.named_parameters():
        assert q.grad is not None, n
        key = 'grad/' + n
        if n.startswith('breath_block.features.') and n.endswith('.bias') and q.shape[0] == getattr(
                model.breath_block.features[int(n.split('.')[2])], 'out_channels', -1):
            assert float(q.grad.abs().max()) == 0, n                        # a conv bias: exactly 0
            continue
        ref = g['dig/' + key] if 'dig/' + key in g else g[key]
        got = digest(host(q.grad)) if 'dig/' + key in g else host(q.grad)
        e, bd = R.rel_l2(got.reshape(ref.shape), ref), bound(float(g['err32/' + key]))
        log('model %-44s digest rel-l2 %.3e  reference fp32 %.3e  bound %.3e' % (key, e, float(g['err32/' + key]), bd))
        if not e <= bd:
            bad.append('%s: digest rel-l2 %.3e > bound %.3e' % (key, e, bd))
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('arch', ['vgg11', 'vgg13'])
def test_whole_model_logits_at_nb20(M, arch):
    g = _gold('vgg_model_%s_nb20.npz' % arch)
    model = build_model(M, g, arch)
    x, t = torch.from_numpy(g['x']).cuda(), torch.from_numpy(g['target']).cuda()
    with torch.no_grad():
        out = model(x, None)
        loss, logits = model.forward_loss(x, t)                              # the fused head on the flat features
    bad = []
    check(arch, 'logits', out, g['logits'], float(g['err32/logits']), bad)
    check(arch, 'fused logits', logits, g['logits'], float(g['err32/logits']), bad)
    check(arch, 'fused loss', loss, g['loss'], float(g['err32/loss']), bad)
    assert not bad, '\n'.join(bad)


def test_backbone_features_at_seq_len_512(M):
    g = _gold('vgg_backbone_512.npz')
    bb = M.vgg11_bn()
    params = R.seeded_vgg_params('vgg11', int(g['seed']), 20)
    bb.load_state_dict({k[len('breath_block.'):]: torch.from_numpy(v) for k, v in params.items() if k.startswith('breath_block.')}, strict=False)
    with torch.no_grad():
        feat = bb.cuda().train()(torch.from_numpy(g['x']).cuda())
    assert tuple(feat.shape) == (20, 3584)
    e, bd = R.rel_l2(digest(host(feat)), g['dig/feat']), bound(float(g['err32/feat']))
    log('seq_len 512 features digest rel-l2 %.3e bound %.3e' % (e, bd))
    assert e <= bd


# ---- trainer and driver ----------------------------------------------------------------------------------------------------------
def _conv_biases(model):
    return [m.bias for m in model.breath_block.features if isinstance(m, torch.nn.Conv1d)]


def test_trainer_eager_and_captured_steps_are_bit_equal(M):
    """Three steps, eager and captured: bit-equal losses, bucket and optimizer state.  The conv biases (the reference's zero
    initialisation) are live parameters of the bucket, get a gradient of exactly 0 in both forms of the captured step (with and
    without the bucket's zero-fill) and stay exactly 0 under weight decay."""
    from deepards_amd import train as T_
    g = _gold('vgg_model_vgg11_nb4.npz')
    x, t = torch.from_numpy(g['x']).cuda(), torch.from_numpy(g['target']).cuda()
    runs = []
    for use_graph, overwrite in ((False, True), (True, True), (True, False)):
        model = build_model(M, g, nb=4)
        for b in _conv_biases(model):
            b.data.zero_()
        prev = T_._GRAD_OVERWRITE
        T_._GRAD_OVERWRITE = overwrite
        try:
            tr = T_.HotPathTrainer(model, optimizer='sgd', use_graph=use_graph)
            losses = []
            for step in range(3):
                if step == 2:       # before a pure replay: a step without the zero-fill must WRITE the biases' zero gradient
                    for b in _conv_biases(model):
                        assert b.grad.data_ptr() == b._da_grad.data_ptr()
                        b.grad.fill_(7.0)
                    torch.cuda.synchronize()
                losses.append(tr.train_step(x, t).detach().clone().reshape(-1))
            losses = torch.cat(losses)
        finally:
            T_._GRAD_OVERWRITE = prev
        if use_graph:
            assert tr.grad_overwrite == overwrite
        live = {id(q) for q in tr.bucket.params}
        for b in _conv_biases(model):
            assert id(b) in live and float(b.detach().abs().max()) == 0 and float(b.grad.abs().max()) == 0
        runs.append((losses, tr.bucket.p.clone(), {k: v.clone() for k, v in tr.state.items()}))
        if use_graph:
            tr.release_graphs()
    assert torch.isfinite(runs[0][0]).all() and float((runs[0][0][0] - runs[0][0][2]).abs()) > 0
    for other in runs[1:]:
        assert torch.equal(runs[0][0], other[0]) and torch.equal(runs[0][1], other[1])
        assert set(runs[0][2]) == set(other[2]) and all(torch.equal(runs[0][2][k], other[2][k]) for k in other[2])


def test_per_breath_head_with_the_confidence_loss(M):
    from deepards_amd.train import HotPathTrainer
    g = _gold('vgg_model_vgg11_nb4.npz')
    x, t = torch.from_numpy(g['x']).cuda(), torch.from_numpy(g['target']).cuda()
    tr = HotPathTrainer(build_model(M, g, nb=4, head='single_breath'), use_graph=False, loss='confidence', loss_param=0.5)
    assert torch.isfinite(tr.train_step(x, t)).all()


def test_driver_trains_and_tests_on_the_fixture():
    from deepards_amd import train_ards_detector as T
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    cls = T.network_map['cnn_linear'](T.make_args(train_from_pickle=os.path.join(GOLD, 'test_dataset.npz'), kfolds=2, epochs=1,
                                                  batch_size=4, seed=3, base_network='vgg11', cuda=False, cuda_no_dp=True))
    res = cls.train_and_test()
    assert cls.model.breath_block.network_name == 'vgg11' and cls.model.linear_final.weight.shape[1] == 3584 * 20
    for fold in (0, 1):
        assert len(res.get_meter('loss', fold)) > 0
        assert np.isfinite(res.get_meter('loss', fold)).all() and np.isfinite(res.get_meter('test_loss', fold)).all()
        assert np.isfinite(res.patient_results[(fold, 1)]['mean_loss'])


def test_load_base_network_from_every_kind_of_file(M, tmp_path):
    """--load-base-network from a state_dict file, from an own whole-module pickle, and from a whole module saved under the
    reference's class paths (deepards.models.vgg.VGG has no network_name: the configured base network names it)."""
    from deepards_amd import checkpoint as C
    from vgg_ref_paths import as_reference_classes
    torch.manual_seed(2)
    m = M.CNNLinearNetwork(M.vgg11_bn(), 20, 0)
    m.breath_block.features[1].weight.data.uniform_(0.5, 1.5)
    sdp, own, ref = (str(tmp_path / n) for n in ('sd.pth', 'own.pth', 'ref.pth'))
    torch.save(m.state_dict(), sdp)
    torch.save(m, own)

    def save_ref(_M):
        name = m.breath_block.__dict__.pop('network_name')
        try:
            torch.save(m, ref)
        finally:
            m.breath_block.network_name = name
    as_reference_classes(save_ref)
    assert [C.checkpoint_kind(p) for p in (sdp, own, ref)] == ['state_dict', 'own', 'foreign']
    info = C.read_module_checkpoint(ref)
    assert info['breath_block_class'] == 'deepards.models.vgg.VGG' and info['network_name'] is None
    assert list(info['state_dict']) == list(m.state_dict())
    for path in (sdp, own, ref):
        bb = C.load_base_network(path, M.base_networks, {'base_network': 'vgg11'})
        assert bb.network_name == 'vgg11' and isinstance(bb, M.VGG)
        assert list(bb.state_dict()) == list(m.breath_block.state_dict())
        assert all(torch.equal(a, b) for a, b in zip(bb.state_dict().values(), m.breath_block.state_dict().values()))
    got = C.load_model_weights(ref, lambda: M.CNNLinearNetwork(M.vgg11_bn(), 20, 0))               # strict keys
    assert all(torch.equal(a, b) for a, b in zip(got.state_dict().values(), m.state_dict().values()))
    # and the loaded block runs
    x = torch.from_numpy(_gold('vgg_model_vgg11_nb20.npz')['x'][0]).cuda()
    with torch.no_grad():
        assert torch.equal(bb.cuda().train()(x), m.breath_block.cuda().train()(x))
