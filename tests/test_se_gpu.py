"""The se_resnet18 backbone on the GPU: the five SE-tail kernels (csrc/se.hip), the chained SEBlockFunction on an SEBasicBlock, the
ceil-mode stem pool (csrc/stem_pool.hip, pool_mode 2), the whole model, the trainer and the driver.

Bound per tensor (the one of tests/test_transformer_gpu.py): rel-l2 against the float64 oracle <= min(max(4 err32, 16 2^-23),
1e-4), err32 = the reference's own fp32-against-fp64 rel-l2 from the golden where the shape has one, else tests/tools/se_ref.py
evaluated in float32 on the CPU.  The kernel cases keep every ReLU pre-activation of the oracle at least 1e-3 from zero
(asserted here, on the CPU): no element is left out of a comparison and the ReLU masks must be the oracle's.  Figures: pytest -s."""
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
import se_ref as R  # noqa: E402
import poison as P  # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
FLOOR, CEIL = 16 * 2.0 ** -23, 1e-4
# (rows, R, L, C): the four stage shapes at two windows, an odd R, an odd L below 7, rows that the gate's row tile (4) does not divide
SHAPES = [(6, 3, 7, 64), (4, 2, 56, 64), (6, 3, 28, 128), (4, 2, 14, 256), (5, 5, 7, 512), (4, 2, 5, 512)]
# the gate's row tile with 3 rows left over; then rows beyond one chunk (C / 2 rows) of the gate backward's parameter-gradient
# partials: 32 + 1, 32 + 8 (the whole model's 40 rows), 32 + 32 + 2 (17 row tiles), 64 + 2 and 64 + 64 + 1 at L = 1
SHAPES += [(7, 7, 3, 64), (33, 3, 3, 64), (40, 20, 5, 64), (66, 3, 3, 64), (66, 2, 3, 128), (129, 3, 1, 128)]
# (rows, R, L, C, Cr): reductions other than 4 -- C / Cr = 1; Cr = 256 (one thread per hidden unit, tpo = 256 / Cr = 1);
# Cr = 16 (tpo = 16) at C = 512 (8 strides of a part over the 128 channel quads) and at C = 256
SHAPES += [(6, 3, 7, 64, 64), (5, 5, 7, 512, 256), (6, 3, 7, 512, 16), (4, 2, 14, 256, 16)]
MULTI_CHUNK = (66, 3, 3, 64)
GRID_CAP = 16384 * 256                # threads of a capped elementwise launch (grid_stride_blocks, csrc/common.h)


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


def mask_bits(mask, shape):
    """The bit mask of se_scale_fwd as a boolean array of the activation's shape."""
    return np.unpackbits(mask.cpu().view(torch.uint8).numpy(), bitorder='little').astype(bool).reshape(shape)


# ---- the five kernels, each alone ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tail_ref(shape):
    """(case, float64 oracle, err32 per tensor) of one kernel shape, computed once."""
    case = R.tail_case(*shape[:4], cr=shape[4] if len(shape) > 4 else None)
    r64 = {k: v.numpy() for k, v in R.se_tail(R=shape[1], **case).items()}
    r32 = R.se_tail(R=shape[1], dtype=torch.float32, **case)
    err = {k: R.rel_l2(r32[k].double().numpy(), r64[k]) for k in r64 if k != 'mask'}
    return case, r64, err


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_each_kernel_alone_against_the_oracle(H, shape):
    """Every kernel on the ORACLE's operands (rounded to float32), so that one kernel's error is not another's input."""
    rows, R_, l, c = shape[:4]
    case, ref, err = tail_ref(shape)
    assert case['w1'].shape == (shape[4] if len(shape) > 4 else c // R.REDUCTION, c, 1)
    hm, om = R.tail_margins(case, R_)
    assert hm >= R.MARGIN and om >= R.MARGIN, (hm, om)
    tag = 'x'.join(map(str, shape))
    g = {k: cu(v) for k, v in case.items()}
    o = {k: cu(v) for k, v in ref.items() if k != 'mask'}
    bad = []
    mean, invstd = H.se_stats(g['y2'], R_)
    check(tag, 'mean', mean, ref['mean'], err['mean'], bad)
    check(tag, 'invstd', invstd, ref['invstd'], err['invstd'], bad)
    bn = (o['mean'], o['invstd'], g['gamma'], g['beta'])
    pool, hid, s = H.se_gate_fwd(g['y2'], R_, *bn, g['w1'], g['b1'], g['w2'], g['b2'])
    for k, v in (('pool', pool), ('hid', hid), ('s', s)):
        check(tag, k, v, ref[k], err[k], bad)
    assert np.array_equal(host(hid) > 0, ref['pre1'] > 0), 'hidden ReLU decisions differ from the oracle\'s'
    out, mask = H.se_scale_fwd(g['y2'], R_, *bn, o['s'], g['res'])
    check(tag, 'out', out, ref['out'], err['out'], bad)
    assert mask.dtype == torch.int64 and mask.numel() * 64 == out.numel()
    assert np.array_equal(mask_bits(mask, ref['mask'].shape), ref['mask']), 'ReLU mask differs from the oracle\'s'
    assert np.array_equal(host(out) > 0, ref['mask'])
    gg, dsum = H.se_bwd_reduce(g['dout'], mask, g['y2'], R_, *bn)
    assert torch.equal(gg, g['dout'] * cu(ref['mask']))                # g is a masked copy of dout, not arithmetic
    check(tag, 'dsum', dsum, ref['dsum'], err['dsum'], bad)
    dpool, (dw1, db1, dw2, db2) = H.se_gate_bwd(o['dsum'], o['s'], o['hid'], o['pool'], g['w1'], g['w2'])
    assert dw1.shape == g['w1'].shape and dw2.shape == g['w2'].shape
    for k, v in (('dpool', dpool), ('dw1', dw1), ('db1', db1), ('dw2', dw2), ('db2', db2)):
        check(tag, k, v, ref[k], err[k], bad)
    dz = H.se_bwd_scale(gg, o['s'], o['dpool'])
    check(tag, 'dz', dz, ref['dz'], err['dz'], bad)
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('shape', [SHAPES[0], SHAPES[4], MULTI_CHUNK], ids=lambda s: 'x'.join(map(str, s)))
def test_gate_bwd_accumulates_and_is_deterministic(H, shape):
    """(66, 3, 3, 64): three chunks of parameter-gradient partials, the last of two rows."""
    rows, R_, l, c = shape
    case, ref, _ = tail_ref(shape)
    g = {k: cu(v) for k, v in case.items()}
    o = {k: cu(ref[k]) for k in ('dsum', 's', 'hid', 'pool')}
    run = lambda **kw: H.se_gate_bwd(o['dsum'], o['s'], o['hid'], o['pool'], g['w1'], g['w2'], **kw)
    dpool, fresh = run()
    torch.manual_seed(1)
    fill = [torch.randn_like(t) for t in fresh]
    acc = [t.clone() for t in fill]
    dpool2, got = run(grads=acc, accumulate=True)
    assert all(a is b for a, b in zip(got, acc)) and torch.equal(dpool, dpool2)
    for a, f, t in zip(acc, fill, fresh):
        assert torch.equal(a, f + t)                                    # accumulate == overwrite + the fill, bit for bit
    over = [torch.full_like(t, float('nan')) for t in fresh]
    run(grads=over)
    assert all(torch.equal(a, b) for a, b in zip(over, fresh))
    # the same bits twice, and again after a call on another shape
    again = run()[1]
    assert all(torch.equal(a, b) for a, b in zip(again, fresh))
    other = SHAPES[2]
    oc, oref, _ = tail_ref(other)
    H.se_gate_bwd(cu(oref['dsum']), cu(oref['s']), cu(oref['hid']), cu(oref['pool']), cu(oc['w1']), cu(oc['w2']))
    after = run()[1]
    assert all(torch.equal(a, b) for a, b in zip(after, fresh))
    with pytest.raises(ValueError):
        run(accumulate=True)


def _sampled(tag, name, got, idx, ref64, ref32, problems):
    """`got` at the flat positions `idx` against the float64 formula there, under the file's bound (err32: the same formula in
    float32 on the CPU)."""
    check(tag, name, got.reshape(-1)[idx], ref64, R.rel_l2(ref32.astype(np.float64), ref64), problems)


def test_elementwise_kernels_beyond_the_grid_cap(H):
    """se_scale_fwd and se_bwd_scale where the capped grid's stride loop runs a second iteration: 4 x 16400 x 512 = 33.6 M
    elements, 4 198 400 (8 channels each) and 8 396 800 (4 channels each) threads of work against 4 194 304 launched.  The full call
    against the same wrapper on slices below the cap (a window of 2 rows, one row), bit for bit, outputs and mask words; and
    a few hundred positions, the last element among them, against the float64 formula."""
    rows, R_, l, c = 4, 2, 16400, 512
    assert rows * l * (c // 8) > GRID_CAP >= R_ * l * (c // 8) and rows * l * (c // 4) > GRID_CAP >= l * (c // 4)
    gen = torch.Generator(device='cuda').manual_seed(5)
    rnd = lambda *shape: torch.randn(*shape, device='cuda', generator=gen)
    uni = lambda *shape: torch.rand(*shape, device='cuda', generator=gen)
    w = rows // R_
    y2, res = rnd(rows, l, c) * 1.5 + 0.3, rnd(rows, l, c)
    mean, invstd, gamma, beta = rnd(w, c) * 0.2 + 0.3, uni(w, c) + 0.5, uni(c) + 0.5, rnd(c) * 0.1
    gamma[3] = -0.7
    s, dpool = uni(rows, c) * 0.98 + 0.01, rnd(rows, c)
    n = rows * l * c
    rng = np.random.default_rng(5)
    # the last element, the first, the two sides of the first element beyond each capped grid, 300 anywhere
    idx_np = np.unique(np.concatenate([[n - 1, 0, GRID_CAP * 8 - 1, GRID_CAP * 8, GRID_CAP * 4 - 1, GRID_CAP * 4], rng.integers(0, n, 300)]))
    idx = torch.from_numpy(idx_np).cuda()
    row, ch, win = idx_np // (l * c), idx_np % c, idx_np // (R_ * l * c)
    at = lambda t: t.reshape(-1)[idx].cpu().numpy()
    rc = lambda t, r: t.cpu().numpy()[r, ch]
    bad = []

    out, mask = H.se_scale_fwd(y2, R_, mean, invstd, gamma, beta, s, res)
    parts = [H.se_scale_fwd(y2[k * R_:(k + 1) * R_], R_, mean[k:k + 1], invstd[k:k + 1], gamma, beta, s[k * R_:(k + 1) * R_],
                            res[k * R_:(k + 1) * R_]) for k in range(w)]
    assert torch.equal(out, torch.cat([p[0] for p in parts])), 'se_scale_fwd: the full call differs from its windows'
    assert torch.equal(mask, torch.cat([p[1] for p in parts])), 'se_scale_fwd: mask words differ from the windows\''
    del parts

    def pre(dt):
        v = lambda a: a.astype(dt)
        z = (v(at(y2)) - v(rc(mean, win))) * v(rc(invstd, win)) * v(gamma.cpu().numpy()[ch]) + v(beta.cpu().numpy()[ch])
        return z * v(rc(s, row)) + v(at(res))
    p64 = pre(np.float64)
    _sampled('grid cap', 'out', out, idx, np.maximum(p64, 0), np.maximum(pre(np.float32), 0), bad)
    bits = ((mask.view(torch.uint8)[idx // 8].cpu().numpy() >> (idx_np % 8)) & 1).astype(bool)
    assert np.array_equal(bits, at(out) > 0)
    sure = np.abs(p64) >= R.MARGIN
    assert sure.sum() > 250 and np.array_equal(bits[sure], p64[sure] > 0), 'ReLU mask differs from the formula\'s'
    del out, mask, y2

    dz = H.se_bwd_scale(res, s, dpool)                                 # (res stands for g: any float activation)
    rowsl = [H.se_bwd_scale(res[r:r + 1], s[r:r + 1], dpool[r:r + 1]) for r in range(rows)]
    assert torch.equal(dz, torch.cat(rowsl)), 'se_bwd_scale: the full call differs from its rows'
    del rowsl
    f = lambda dt: at(res).astype(dt) * rc(s, row).astype(dt) + rc(dpool, row).astype(dt) / dt(l)
    _sampled('grid cap', 'dz', dz, idx, f(np.float64), f(np.float32), bad)
    assert not bad, '\n'.join(bad)


def test_unsupported_shapes_are_refused(H):
    y = torch.zeros(2, 7, 96, device='cuda')
    st = torch.zeros(1, 96, device='cuda')
    v = torch.zeros(96, device='cuda')
    w1, b1, w2, b2 = torch.zeros(24, 96, 1, device='cuda'), torch.zeros(24, device='cuda'), torch.zeros(96, 24, 1, device='cuda'), v
    with pytest.raises(H.HipError):
        H.se_gate_fwd(y, 2, st, st, v, v, w1, b1, w2, b2)              # C = 96: not a multiple of 64
    with pytest.raises(ValueError):
        H.se_scale_fwd(torch.zeros(2, 7, 64, device='cuda'), 2, st, st, v, v, torch.zeros(2, 64, device='cuda'),
                       torch.zeros(2, 7, 64, device='cuda'))           # statistics of another width


# ---- the chained block ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def block_ref(tag):
    g = _gold('se_block_cases.npz')
    rows, R_, l_out, planes, stride, seed = (int(v) for v in g[tag + '/cfg'])
    x, params, dout = R.block_inputs(rows, R_, l_out, planes, stride, seed)
    assert np.array_equal(x, g[tag + '/x'])
    r = {k: v.numpy() for k, v in R.block_case(x, params, stride, R_, dout).items()}
    return x, params, dout, stride, R_, r


BLOCK_TAGS = ['id_6x3x7x64', 'id_4x2x56x64', 'id_5x5x7x512', 'id_4x2x5x512', 's2_6x3x28x128', 's2_4x2x14x256', 's2_5x5x7x512']


@pytest.mark.parametrize('winograd', [True, False], ids=['default', 'DA_WINOGRAD=0'])
@pytest.mark.parametrize('tag', BLOCK_TAGS)
def test_chained_block_function(H, M, tag, winograd):
    """SEBlockFunction on an SEBasicBlock (identity and stride-2 entries) through the module, forward and backward, against the oracle at
    the golden's err32; the ReLU decisions of the output must be the oracle's.  Then the same block inside a training step
    with gradient destinations on every parameter (the batched weight-gradient launch, the queued folds, the SE parameters
    written in place): the destinations hold the same gradients at the same bound.

    The block's k3 s1 convs keep off the F(4,3) Winograd kernels (hip_ops._wino, ``precise``): with them the three
    512-channel cases measured 1.9e-06 .. 3.2e-06 on the parameter gradients against the 1.907e-06 bound (out 0.9e-06)."""
    g = _gold('se_block_cases.npz')
    x, params, dout, stride, R_, ref = block_ref(tag)
    m = R.block_margins(x, params, stride, R_)
    assert min(m.values()) >= R.MARGIN, m
    planes, cin = params['conv1.weight'].shape[:2]
    ds = None
    if stride != 1:
        ds = torch.nn.Sequential(torch.nn.Conv1d(cin, planes, kernel_size=1, stride=stride, bias=False), torch.nn.BatchNorm1d(planes))
    blk = M.SEBasicBlock(cin, planes, 1, 4, stride, ds)
    assert not blk.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=False).unexpected_keys
    blk = blk.cuda().train()
    xt = cu(x).requires_grad_(True)
    prev = H.WINOGRAD_WGRAD
    H.WINOGRAD_WGRAD = winograd
    try:
        out = blk.forward_rlc(xt, R_)
        out.backward(cu(dout))
        torch.cuda.synchronize()
    finally:
        H.WINOGRAD_WGRAD = prev
    bad = []
    name = '%s %s' % (tag, 'wino' if winograd else 'direct')
    check(name, 'out', out, ref['out'], float(g['err32/%s/out' % tag]), bad)
    assert np.array_equal(host(out) > 0, ref['pre/out'] > 0), 'output ReLU decisions differ from the oracle\'s'
    check(name, 'dx', xt.grad, ref['dx'], float(g['err32/%s/dx' % tag]), bad)
    for n, q in blk.named_parameters():
        check(name, 'grad/' + n, q.grad, ref['grad/' + n], float(g['err32/%s/grad/%s' % (tag, n)]), bad)
    assert not bad, '\n'.join(bad)
    # inside a training step, every gradient written into a destination (zero-filled: the writers accumulate outside a capture)
    from deepards_amd import functional as F_
    fill = {}
    for n, q in blk.named_parameters():
        q.grad = None
        fill[n] = torch.zeros_like(q)
        q._da_grad = fill[n].clone()
    xs = cu(x).requires_grad_(True)
    H.WINOGRAD_WGRAD = winograd
    try:
        with F_.training_step(blk):
            o2 = blk.forward_rlc(xs, R_)
            F_.flush_forward(defer=True)
            o2.backward(cu(dout))
            F_.flush_backward()
        torch.cuda.synchronize()
    finally:
        H.WINOGRAD_WGRAD = prev
        dests = {n: q.__dict__.pop('_da_grad') for n, q in blk.named_parameters()}
    assert torch.equal(o2, out) and all(q.grad is None for q in blk.parameters())
    check(name + ' step', 'dx', xs.grad, ref['dx'], float(g['err32/%s/dx' % tag]), bad)
    for n in dests:
        check(name + ' step', 'grad/' + n, dests[n], ref['grad/' + n], float(g['err32/%s/grad/%s' % (tag, n)]), bad)
    assert not bad, '\n'.join(bad)
    # running statistics: one momentum update per window (the reference's loop), bn2's from the statistics-only pass
    w = x.shape[0] // R_
    assert int(blk.bn2.num_batches_tracked) == 2 * w == int(blk.bn1.num_batches_tracked)       # (two forwards)
    assert torch.isfinite(blk.bn2.running_var).all() and float((blk.bn2.running_mean != 0).float().mean()) > 0.9


def test_basic_block_gate_stays_narrow_at_512_32(H, M, monkeypatch):
    """An SEBasicBlock of 512 planes with reduction 16 has the gate (C, Cr) = (512, 32): the one shape both kernel families take
    at which H.se_gate_family names the wide one (se_ops.WIDE_SHARED, timed for the bottleneck).  The basic block names its
    family itself: forward and backward run the narrow gate kernels and never the wide ones."""
    from deepards_amd import functional as F_
    assert H.se_gate_family(512, 32) == H.SE_WIDE and H.se_narrow_ok(512, 32)
    calls = {}

    def counted(name):
        fn = getattr(H, name)

        def wrapper(*a, **kw):
            calls[name] = calls.get(name, 0) + 1
            return fn(*a, **kw)
        return wrapper
    names = ('se_gate_fwd', 'se_wide_gate_fwd', 'se_gate_bwd', 'se_wide_gate_bwd')
    for n in names:
        monkeypatch.setattr(H, n, counted(n))
    assert F_.H is H
    torch.manual_seed(11)
    blk = M.SEBasicBlock(512, 512, 1, 16).cuda().train()
    x = torch.randn(2, 3, 512, device='cuda').requires_grad_(True)             # (rows 2, L 3, C 512), one window of R = 2 rows
    out = blk.forward_rlc(x, 2)
    out.backward(torch.randn_like(out))
    torch.cuda.synchronize()
    assert calls == {'se_gate_fwd': 1, 'se_gate_bwd': 1}, calls
    assert tuple(out.shape) == (2, 3, 512) and torch.isfinite(out).all() and torch.isfinite(x.grad).all()
    assert all(q.grad is not None and torch.isfinite(q.grad).all() for q in blk.parameters())


# ---- memory discipline ----------------------------------------------------------------------------------------------------
def _tail_inputs(shape):
    case, ref, _ = tail_ref(shape)
    return {k: cu(v) for k, v in case.items()}, {k: cu(v) for k, v in ref.items() if k != 'mask'}


def _op_cases(H):
    cases, last = [], []              # (last: rows added behind the first eleven, whose indices are test ids)
    for shape in (SHAPES[0], SHAPES[5]):
        rows, R_, l, c = shape
        tag = 'x'.join(map(str, shape))

        def b_fwd(shape=shape):
            g, _ = _tail_inputs(shape)
            return dict(y2=g['y2'], res=g['res'], gamma=g['gamma'], beta=g['beta'], w1=g['w1'], b1=g['b1'], w2=g['w2'], b2=g['b2'],
                        out=torch.zeros_like(g['y2']))

        def c_fwd(y2, res, gamma, beta, w1, b1, w2, b2, out, R_=R_):
            mean, invstd = H.se_stats(y2, R_)
            pool, hid, s = H.se_gate_fwd(y2, R_, mean, invstd, gamma, beta, w1, b1, w2, b2)
            o, mask = H.se_scale_fwd(y2, R_, mean, invstd, gamma, beta, s, res, out=out)
            return dict(mean=mean, invstd=invstd, pool=pool, hid=hid, s=s, out=o, mask=mask)
        cases.append(P.OpCase('se_fwd_' + tag, 'se', b_fwd, c_fwd, dests=('out',),
                              rows=dict(inputs=('y2', 'res'), R=R_, axis={})))

        def b_red(shape=shape):
            g, o = _tail_inputs(shape)
            _, mask = H.se_scale_fwd(g['y2'], shape[1], o['mean'], o['invstd'], g['gamma'], g['beta'], o['s'], g['res'])
            return dict(dout=g['dout'], mask=mask, y2=g['y2'], mean=o['mean'], invstd=o['invstd'], gamma=g['gamma'], beta=g['beta'])
        cases.append(P.OpCase('se_bwd_reduce_' + tag, 'se', b_red,
                              lambda dout, mask, y2, mean, invstd, gamma, beta, R_=R_: H.se_bwd_reduce(dout, mask, y2, R_, mean, invstd, gamma, beta),
                              rows=dict(inputs=('dout', 'y2'), R=R_, axis={})))

        def b_gbw(shape=shape):
            g, o = _tail_inputs(shape)
            return dict(dsum=o['dsum'], s=o['s'], hid=o['hid'], pool=o['pool'], w1=g['w1'], w2=g['w2'],
                        grads=[torch.zeros_like(g['w1']), torch.zeros_like(g['b1']), torch.zeros_like(g['w2']), torch.zeros_like(g['b2'])])
        # the parameter gradients sum over all rows: a NaN row reaches them, so the isolation check leaves them out by name
        cases.append(P.OpCase('se_gate_bwd_' + tag, 'se', b_gbw,
                              lambda dsum, s, hid, pool, w1, w2, grads: H.se_gate_bwd(dsum, s, hid, pool, w1, w2, grads=grads),
                              dests=('grads',),
                              rows=dict(inputs=('dsum', 's', 'hid', 'pool'), R=1,
                                        axis={'[1][0]': None, '[1][1]': None, '[1][2]': None, '[1][3]': None})))

        def b_bsc(shape=shape):
            g, o = _tail_inputs(shape)
            return dict(g=o['g'], s=o['s'], dpool=o['dpool'], out=torch.zeros_like(o['g']))
        cases.append(P.OpCase('se_bwd_scale_' + tag, 'se', b_bsc, lambda g, s, dpool, out: H.se_bwd_scale(g, s, dpool, out=out),
                              dests=('out',), rows=dict(inputs=('g', 's', 'dpool'), R=1, axis={})))
    shape = MULTI_CHUNK                # three chunks of partials: every partial written and folded, none twice

    def b_gbw3():
        g, o = _tail_inputs(MULTI_CHUNK)
        return dict(dsum=o['dsum'], s=o['s'], hid=o['hid'], pool=o['pool'], w1=g['w1'], w2=g['w2'],
                    grads=[torch.zeros_like(g['w1']), torch.zeros_like(g['b1']), torch.zeros_like(g['w2']), torch.zeros_like(g['b2'])])
    last.append(P.OpCase('se_gate_bwd_' + 'x'.join(map(str, shape)), 'se', b_gbw3,
                         lambda dsum, s, hid, pool, w1, w2, grads: H.se_gate_bwd(dsum, s, hid, pool, w1, w2, grads=grads),
                         dests=('grads',),
                         rows=dict(inputs=('dsum', 's', 'hid', 'pool'), R=1,
                                   axis={'[1][0]': None, '[1][1]': None, '[1][2]': None, '[1][3]': None})))
    for tag, rows, R_, lin in (('224', 4, 2, 224), ('30', 6, 2, 30), ('16', 4, 2, 16)):
        def b_stem(rows=rows, R_=R_, lin=lin):
            x, w, gamma, beta, dout = R.stem_inputs(rows, R_, lin, 64, 3)
            return dict(x=cu(x), w=cu(w), gamma=cu(gamma), beta=cu(beta), dout=cu(dout))

        def c_stem(x, w, gamma, beta, dout, R_=R_):
            y0 = H.stem_conv_fwd(x, w)
            mean, invstd = H.bn_stats(y0, R_)
            out0 = H.bn_relu_pool_fwd(y0, R_, mean, invstd, gamma, beta, 2)
            dz = H.pool_bwd(dout, y0, R_, mean, invstd, gamma, beta, 2)
            out, m2, i2 = H.stem_fused_fwd(x, w, R_, gamma, beta, 2)
            dw, ds = H.stem_fused_bwd(dout, x, w, R_, m2, i2, gamma, beta, 2)
            return dict(out0=out0, dz=dz, out=out, mean=m2, invstd=i2, dw=dw, ds=ds)
        # dw sums over all rows; ds is (2, W, C): its window axis is 1
        cases.append(P.OpCase('stem_pool_mode2_' + tag, 'stem', b_stem, c_stem,
                              rows=dict(inputs=('x', 'dout'), R=R_, axis={'dw': None, 'ds': 1})))
    return cases + last


CHECKS = {'uninitialised': P.check_uninitialised, 'guards': P.check_guards, 'dirty_out': P.check_dirty_out, 'isolation': P.check_isolation}
N_OP_CASES = 12


@pytest.mark.parametrize('check', sorted(CHECKS))
@pytest.mark.parametrize('i', range(N_OP_CASES))
def test_memory_discipline(H, i, check):
    cases = _op_cases(H)
    assert len(cases) == N_OP_CASES
    problems = CHECKS[check](cases[i])
    assert not problems, '\n'.join(problems)


# ---- the ceil-mode stem pool -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', ['stem_224', 'stem_30', 'stem_16', 'stem_14'])
def test_stem_pool_mode_2(H, tag):
    """Lc = 112, 15, 8 (clipped last window) and 7 (none clipped): the fused and per-op forms, forward and backward."""
    g = _gold('se_block_cases.npz')
    rows, R_, lin, c, seed = (int(v) for v in g[tag + '/cfg'])
    x, w, gamma, beta, dout = R.stem_inputs(rows, R_, lin, c, seed)
    ref = {k: v.numpy() for k, v in R.stem_case(x, w, gamma, beta, R_, dout).items()}
    lp = R.pool_len_ceil(lin // 2)
    xt, wt, gt, bt, dt = cu(x), cu(w), cu(gamma), cu(beta), cu(dout)
    assert H.stem_fused_ok(xt, wt, R_)
    # per-op form
    y0 = H.stem_conv_fwd(xt, wt)
    mean0, invstd0 = H.bn_stats(y0, R_, 1e-5)
    out0 = H.bn_relu_pool_fwd(y0, R_, mean0, invstd0, gt, bt, 2)
    assert tuple(out0.shape) == (rows, lp, c)
    bad = []
    err = lambda k: float(g['err32/%s/%s' % (tag, k)])
    check(tag, 'out (per-op)', out0, ref['out'], err('out'), bad)
    dz = H.pool_bwd(dt, y0, R_, mean0, invstd0, gt, bt, 2)
    # the routed gradient is a copy (or, where one position is the first maximum of two windows, an exact sum) of dout:
    # bit for bit the oracle's routing on the map this run pooled
    a = torch.relu((y0.double().cpu().reshape(rows // R_, -1, c) - mean0.double().cpu()[:, None]) * invstd0.double().cpu()[:, None]
                   * torch.from_numpy(gamma).double() + torch.from_numpy(beta).double()).reshape(rows, lin // 2, c)
    routed = R.ceil_pool_routing(a, torch.from_numpy(dout).double())
    assert torch.equal(dz.cpu(), routed.float()), 'routed gradient differs from the oracle\'s first-maximum rule'
    assert float((a[1] == a[1, :1]).double().mean()) == 1.0             # the silent row: every window is a three-way tie
    assert float(a[:, :, 5].abs().max()) == 0.0                         # the all-negative channel: the ReLU gives 0, 0, 0
    dy0, dg0, db0, _, _ = H.bn_bwd(dz, y0, R_, mean0, invstd0, gt, bt, 1, dx=dz.clone())
    dw0 = H.stem_conv_wgrad(dy0, xt)
    check(tag, 'dw (per-op)', dw0, ref['dw'], err('dw'), bad)
    check(tag, 'dgamma (per-op)', dg0, ref['dgamma'], err('dgamma'), bad)
    check(tag, 'dbeta (per-op)', db0, ref['dbeta'], err('dbeta'), bad)
    # fused form: the forward bit for bit the per-op one, as modes 0 / 1
    out, mean, invstd = H.stem_fused_fwd(xt, wt, R_, gt, bt, 2)
    assert torch.equal(mean, mean0) and torch.equal(invstd, invstd0) and torch.equal(out, out0)
    out3, _, _ = H.stem_fused_fwd(xt, wt, R_, gt, bt, 2, out_x3=True)
    assert torch.equal(out3, H.bn_relu_pool_fwd(y0, R_, mean0, invstd0, gt, bt, 2, out_x3=True))
    dw, ds = H.stem_fused_bwd(dt, xt, wt, R_, mean, invstd, gt, bt, 2)
    dg, db = torch.zeros(c, device='cuda'), torch.zeros(c, device='cuda')
    H.bn_param_grad_multi([(ds, dg, db)], accumulate=False)
    check(tag, 'dw (fused)', dw, ref['dw'], err('dw'), bad)
    check(tag, 'dgamma (fused)', dg, ref['dgamma'], err('dgamma'), bad)
    check(tag, 'dbeta (fused)', db, ref['dbeta'], err('dbeta'), bad)
    assert not bad, '\n'.join(bad)
    # the two backward forms route the same elements: their sums differ by fp32 summation order only (the bounds
    # tests/test_stem_fused_gpu.py holds modes 0 / 1 to)
    for p_, q_ in ((dw, dw0), (dg, dg0), (db, db0)):
        assert float((p_ - q_).abs().max()) <= 2e-5 * float(q_.abs().max())
    acc = dw0.clone()
    H.stem_fused_bwd(dt, xt, wt, R_, mean, invstd, gt, bt, 2, dw=acc, accumulate=True)
    assert float((acc - 2 * dw0).abs().max()) <= 4e-5 * float(dw0.abs().max())


def test_stem_function_takes_both_forms_of_mode_2(H):
    """StemFunction with POOL_MAX_CEIL through the recomputing kernels and -- DA_STEM_FUSED=0 -- the per-op ones."""
    from deepards_amd import functional as F_
    x, w, gamma, beta, dout = R.stem_inputs(4, 2, 224, 64, 9)
    bn = torch.nn.BatchNorm1d(64).cuda()
    res = []
    prev = F_._STEM_FUSED
    try:
        for fused in (True, False):
            F_._STEM_FUSED = fused
            wt, gt, bt = (cu(a).requires_grad_(True) for a in (w, gamma, beta))
            out = F_.StemFunction.apply(cu(x), wt, gt, bt, 2, F_.POOL_MAX_CEIL, F_.BNState(bn), False)
            out.backward(cu(dout))
            res.append((out.detach(), wt.grad, gt.grad, bt.grad))
    finally:
        F_._STEM_FUSED = prev
    assert tuple(res[0][0].shape) == (4, 56, 64) and torch.equal(res[0][0], res[1][0])
    for a, b in zip(res[0][1:], res[1][1:]):
        assert float((a - b).abs().max()) <= 2e-5 * float(b.abs().max())


# ---- the whole model -----------------------------------------------------------------------------------------------------
def build_model(M, g, head='linear'):
    bb = M.se_resnet18()
    model = M.CNNLinearNetwork(bb, 20, 0) if head == 'linear' else M.CNNSingleBreathLinearNetwork(bb)
    params = R.seeded_se_params(int(g['seed']), 20, bn_bias_shift=float(g['bn_bias_shift']), fc1_bias_shift=float(g['fc1_bias_shift']))
    sd = {k: torch.from_numpy(v) for k, v in params.items() if head == 'linear' or k.startswith('breath_block.')}
    assert not model.load_state_dict(sd, strict=False).unexpected_keys
    return model.cuda().train()


def test_whole_model_against_the_shifted_golden(M):
    from deepards_amd import functional as F_
    g = _gold('se_model_b2.npz')
    model = build_model(M, g)
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
        ref = g['dig/' + key] if 'dig/' + key in g else g[key]
        got = digest(host(q.grad)) if 'dig/' + key in g else host(q.grad)
        e, bd = R.rel_l2(got.reshape(ref.shape), ref), bound(float(g['err32/' + key]))
        log('model %-60s digest rel-l2 %.3e  reference fp32 %.3e  bound %.3e' % (key, e, float(g['err32/' + key]), bd))
        if not e <= bd:
            bad.append('%s: digest rel-l2 %.3e > bound %.3e' % (key, e, bd))
    assert not bad, '\n'.join(bad)


def test_whole_model_logits_on_the_unshifted_golden(M):
    g = _gold('se_model_b2_unshifted.npz')
    model = build_model(M, g)
    with torch.no_grad():
        out = model(torch.from_numpy(g['x']).cuda(), None)
    bad = []
    check('model unshifted', 'logits', out, g['logits'], float(g['err32/logits']), bad)
    assert not bad, '\n'.join(bad)
    # the pooled features through forward_windows(pooled=True) and the map through features() agree with the head's path
    bb = model.breath_block
    with torch.no_grad():
        x = torch.from_numpy(g['x'][0]).cuda()
        feat = bb(x)
        fmap = bb.features(x)
    assert tuple(feat.shape) == (20, 512) and tuple(fmap.shape) == (20, 512, 7)
    assert torch.allclose(bb.logits(fmap).squeeze(-1), feat, rtol=1e-5, atol=1e-6)


# ---- trainer and driver --------------------------------------------------------------------------------------------------
def test_trainer_eager_and_captured_steps_are_bit_equal(M):
    from deepards_amd.train import HotPathTrainer
    g = _gold('se_model_b2_unshifted.npz')
    x, t = torch.from_numpy(g['x']).cuda(), torch.from_numpy(g['target']).cuda()
    runs = []
    for use_graph in (False, True):
        model = build_model(M, g)
        start = {n: q.detach().clone() for n, q in model.named_parameters()}
        tr = HotPathTrainer(model, optimizer='sgd', use_graph=use_graph)
        losses = torch.cat([tr.train_step(x, t).clone().reshape(-1) for _ in range(3)])
        runs.append((losses, tr.bucket.p.clone(), {k: v.clone() for k, v in tr.state.items()}))
        moved = {n: float((q.detach() - start[n]).abs().max()) for n, q in model.named_parameters() if 'se_module' in n}
        assert len(moved) == 32 and min(moved.values()) > 0, 'SE parameters that did not move: %s' % [n for n, v in moved.items() if v == 0]
        if use_graph:
            tr.release_graphs()
    assert torch.isfinite(runs[0][0]).all()
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert set(runs[0][2]) == set(runs[1][2]) and 'buf' in runs[0][2]
    assert all(torch.equal(runs[0][2][k], runs[1][2][k]) for k in runs[0][2])


def test_per_breath_head_with_the_confidence_loss(M):
    from deepards_amd.train import HotPathTrainer
    g = _gold('se_model_b2_unshifted.npz')
    x, t = torch.from_numpy(g['x']).cuda(), torch.from_numpy(g['target']).cuda()
    tr = HotPathTrainer(build_model(M, g, head='single_breath'), use_graph=False, loss='confidence', loss_param=0.5)
    assert torch.isfinite(tr.train_step(x, t)).all()


def test_driver_trains_and_tests_on_the_fixture():
    from deepards_amd import train_ards_detector as T
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    cls = T.network_map['cnn_linear'](T.make_args(train_from_pickle=os.path.join(GOLD, 'test_dataset.npz'), kfolds=2, epochs=1,
                                                  batch_size=4, seed=3, base_network='se_resnet18', cuda=False, cuda_no_dp=True))
    res = cls.train_and_test()
    assert cls.model.breath_block.network_name == 'se_resnet18'
    for fold in (0, 1):
        assert len(res.get_meter('loss', fold)) > 0
        assert np.isfinite(res.get_meter('loss', fold)).all() and np.isfinite(res.get_meter('test_loss', fold)).all()
        assert np.isfinite(res.patient_results[(fold, 1)]['mean_loss'])
