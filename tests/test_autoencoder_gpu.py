"""The autoencoder on the GPU: the pool-with-index, unpool and output-stage kernels (csrc/autoencoder.hip) against the float64
pieces of tests/tools/ae_ref.py, the decision condition, the whole model teacher-forced with the golden bits, ``eval()``, the
trainer, the driver class and the memory discipline of every new wrapper.

Bound per tensor (ae_ref.bound, the project's): rel-l2 against float64 <= min(max(4 err32, 16 2^-23), 1e-4).  err32 is the
rel-l2 of the SAME ae_ref pieces evaluated in float32 on the CPU on the same inputs (kernel and output-stage tests, eval), or the
golden's ``err32/<name>`` -- the real reference classes in float32 against float64 -- for the whole model.  Values are compared
with the decisions handed in (teacher forcing), so that no comparison depends on how a near-tie fell; the free-running
decisions are held to their own condition: they may differ from the float64 ones only on pairs whose float64 gap is below 1e-4.
Figures: pytest -s."""
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

import ae_ref as R  # noqa: E402
import poison as P  # noqa: E402

F64, F32 = torch.float64, torch.float32


def log(*a):
    print(' '.join(str(x) for x in a))


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


def cl(a):
    """(N, C, L) array -> (N, L, C) float32 CUDA tensor."""
    return torch.as_tensor(np.asarray(a), dtype=F32).permute(0, 2, 1).contiguous().cuda()


def ncl(t):
    """(N, L, C) CUDA tensor -> (N, C, L) float64 array."""
    return t.detach().permute(0, 2, 1).cpu().numpy().astype(np.float64)


def dev(a):
    return torch.as_tensor(np.asarray(a), dtype=F32).contiguous().cuda()


def held(name, got, ref64, ref32, cancelled=None):
    """rel-l2 of ``got`` against float64 within ae_ref.bound(err32).  ``cancelled``: the term whose cancellation leaves the
    tensor (BatchNorm's dy over a window of two positions is mathematically ~eps / var of its terms).  Where the float32
    reference ITSELF is past the bound's cap -- no float32 evaluation can then be asked to hold it -- both errors are taken
    relative to that term's norm instead of the tensor's."""
    err32 = R.rel_l2(ref32, ref64)
    err = R.rel_l2(got, ref64)
    if cancelled is not None and err32 > R.BOUND_CAP:
        s = float(np.sqrt(np.sum(np.asarray(cancelled, dtype=np.float64) ** 2)))
        diff = lambda a: float(np.sqrt(np.sum((np.asarray(a, dtype=np.float64) - ref64) ** 2))) / s    # noqa: E731
        err32, err = diff(ref32), diff(got)
        name += ' (relative to the cancelled term)'
    log('%-28s err %.3e  err32 %.3e  bound %.3e' % (name, err, err32, R.bound(err32)))
    assert err <= R.bound(err32), '%s: rel-l2 %.3e over the bound %.3e (err32 %.3e)' % (name, err, R.bound(err32), err32)


def f32ok(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


# ---- the pool kernels ------------------------------------------------------------------------------------------------------------
def _multi_chunk_rows(H):
    """The smallest one-window (rows, 2, 32) map whose backward takes more than one chunk, by the plan function."""
    rows = 1
    while H.bn_maxpool2_idx_plan(rows, rows, 2, 32).chunks < 2:
        rows += 1
    assert H.bn_maxpool2_idx_plan(rows - 1, rows - 1, 2, 32).chunks == 1
    return rows


# (rows, R, Lin, C); 'multi': the smallest multi-chunk shape; the last one has two windows and a channel count that is no power of 2
POOL_SHAPES = [(1, 1, 2, 32), (3, 3, 6, 64), (5, 5, 28, 512), (40, 40, 224, 64), 'multi', (6, 3, 10, 96)]


def _pool_inputs(rows, lin, c, seed):
    r = np.random.RandomState(seed)
    y = f32ok(r.standard_normal((rows, c, lin)) * 1.5 + 0.3)
    gamma = f32ok(r.uniform(0.5, 1.5, c))
    gamma[::3] *= -1.0                                           # negative: the decision is on z, not on y
    gamma[4::5] = 0.0                                            # zero: every pair of the channel ties -> bit 0
    beta = f32ok(r.uniform(-0.5, 0.5, c))
    dout = f32ok(r.standard_normal((rows, c, lin // 2)))
    if lin >= 6:                                                 # exact ties in y: the first member is kept
        y[:, 1::2, 3] = y[:, 1::2, 2]
    return y, gamma, beta, dout


def _pool_ref(y, R_, gamma, beta, dout, sel, dtype):
    yt, g, b = R._t(y, dtype, True), R._t(gamma, dtype, True), R._t(beta, dtype, True)
    mean, var = R.bn_stats(yt, R_)
    z = R.bn_apply(yt, mean, var, g, b)
    out, s, gap = R.pool2(z, None if sel is None else torch.as_tensor(sel))
    (out * R._t(dout, dtype)).sum().backward()
    return dict(out=out.detach().numpy(), sel=s.numpy(), gap=gap.numpy(), dy=yt.grad.numpy(), dgamma=g.grad.numpy(),
                dbeta=b.grad.numpy(), mean=mean.detach().numpy(), var=var.detach().numpy())


@pytest.mark.parametrize('shape', POOL_SHAPES, ids=str)
def test_pool_kernels_against_float64(H, shape):
    rows, R_, lin, c = (lambda n: (n, n, 2, 32))(_multi_chunk_rows(H)) if shape == 'multi' else shape
    if shape == 'multi':
        assert H.bn_maxpool2_idx_plan(rows, R_, lin, c).chunks == 2
    y, gamma, beta, dout = _pool_inputs(rows, lin, c, 11)
    free = _pool_ref(y, R_, gamma, beta, dout, None, F64)
    r32 = _pool_ref(y, R_, gamma, beta, dout, free['sel'], F32)
    yd, gd, bd, dd = cl(y), dev(gamma), dev(beta), cl(dout)
    mean, invstd = dev(free['mean']), dev(1.0 / np.sqrt(free['var'] + R.EPS))
    # free-running: the decisions
    out_free, sel = H.bn_maxpool2_idx_fwd(yd, R_, mean, invstd, gd, bd)
    bits = H.sel_to_bool(sel.cpu(), c).numpy()
    differ = bits != free['sel']
    log(shape, 'decisions that differ from float64:', int(differ.sum()), 'of', differ.size)
    assert not differ.any() or float(free['gap'][differ].max()) < 1e-4
    assert not bits[:, 4::5].any()                               # gamma = 0: all ties, all bits 0
    if lin >= 6:
        assert not bits[:, 1::2, 1].any()                        # y[2] == y[3] exactly: the first is kept
    # teacher-forced with the float64 decisions: the values
    forced = H.sel_from_bool(torch.from_numpy(free['sel'])).cuda()
    out, taken = H.bn_maxpool2_idx_fwd(yd, R_, mean, invstd, gd, bd, sel_in=forced)
    assert taken is forced
    held('pool out', ncl(out), free['out'], r32['out'])
    same = ~differ
    assert np.array_equal(ncl(out_free)[same], ncl(out)[same])  # where the decisions agree the two runs are one computation
    dy, ds = H.bn_maxpool2_idx_bwd(dd, forced, yd, R_, mean, invstd, gd, bd)
    dg, db = torch.empty_like(gd), torch.empty_like(bd)
    H.bn_param_grad_multi([(ds, dg, db)], accumulate=False)
    kdz = R.unpool2(torch.tensor(dout), torch.from_numpy(free['sel'])).numpy() * \
        np.repeat(gamma[None, :] / np.sqrt(free['var'] + R.EPS), R_, axis=0)[:, :, None]
    held('pool dy', ncl(dy), free['dy'], r32['dy'], cancelled=kdz)
    held('pool dgamma', dg.cpu().numpy(), free['dgamma'], r32['dgamma'])
    held('pool dbeta', db.cpu().numpy(), free['dbeta'], r32['dbeta'])
    assert float(dy.permute(0, 2, 1)[:, 4::5].abs().max()) == 0  # gamma = 0: no gradient reaches y


def test_pool_takes_flipped_bits_as_given_and_copies_them(H):
    rows, lin, c = 3, 6, 64
    y, gamma, beta, dout = _pool_inputs(rows, lin, c, 5)
    free = _pool_ref(y, rows, gamma, beta, dout, None, F64)
    flipped = ~free['sel']
    want = _pool_ref(y, rows, gamma, beta, dout, flipped, F64)
    w32 = _pool_ref(y, rows, gamma, beta, dout, flipped, F32)
    yd, gd, bd = cl(y), dev(gamma), dev(beta)
    mean, invstd = dev(free['mean']), dev(1.0 / np.sqrt(free['var'] + R.EPS))
    given = H.sel_from_bool(torch.from_numpy(flipped)).cuda()
    copy = torch.zeros_like(given)
    out, taken = H.bn_maxpool2_idx_fwd(yd, rows, mean, invstd, gd, bd, sel_in=given, sel=copy)
    assert taken is copy and torch.equal(copy, given)
    held('pool out, flipped bits', ncl(out), want['out'], w32['out'])
    dy, _ = H.bn_maxpool2_idx_bwd(cl(dout), given, yd, rows, mean, invstd, gd, bd)
    held('pool dy, flipped bits', ncl(dy), want['dy'], w32['dy'])


def test_pool_ties_and_signed_zeros(H):
    """-0.0 against +0.0 is a tie in either order: bit 0, and the FIRST member's bits come out.  mean = +0, beta = -0, gamma =
    invstd = 1 make z = fmaf(y, 1, -0.0) keep the sign of a zero y."""
    rows, lin, c = 2, 4, 32
    y = torch.ones((rows, lin, c), dtype=F32)
    y[0, 0], y[0, 1] = -0.0, 0.0
    y[0, 2], y[0, 3] = 0.0, -0.0
    y[1, 0], y[1, 1] = 2.5, 2.5                                  # an exact tie
    y[1, 2], y[1, 3] = 1.0, float(np.nextafter(np.float32(1.0), np.float32(2.0)))       # one ulp: the second wins
    z = torch.zeros((1, c), dtype=F32).cuda()
    out, sel = H.bn_maxpool2_idx_fwd(y.cuda(), rows, z, torch.ones_like(z), torch.ones(c, device='cuda'), -torch.zeros(c, device='cuda'))
    bits = H.sel_to_bool(sel.cpu(), c).numpy()
    assert not bits[0].any() and not bits[1, :, 0].any() and bits[1, :, 1].all()
    o = out.cpu().view(torch.int32)
    assert (o[0, 0] == torch.tensor(-0.0).view(torch.int32)).all() and (o[0, 1] == 0).all()
    assert torch.equal(out.cpu()[1, 0], y[1, 0]) and torch.equal(out.cpu()[1, 1], y[1, 3])


# ---- unpool ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows,lo,c', [(1, 1, 32), (3, 3, 64), (5, 14, 512), (40, 112, 64), (7, 9, 96)])
def test_unpool_against_float64(H, rows, lo, c):
    r = np.random.RandomState(3)
    v, bias = f32ok(r.standard_normal((rows, c, lo))), f32ok(r.uniform(-0.5, 0.5, c))
    sel = r.rand(rows, c, lo) < 0.5
    words = H.sel_from_bool(torch.from_numpy(sel)).cuda()
    for b in (bias, None):
        add = 0.0 if b is None else b[None, :, None]
        want = R.unpool2(torch.tensor(v + add), torch.from_numpy(sel)).numpy()
        w32 = R.unpool2(torch.tensor(v, dtype=F32) + torch.tensor(add, dtype=F32), torch.from_numpy(sel)).numpy()
        out = H.unpool2_fwd(cl(v), words, None if b is None else dev(b))
        held('unpool out (%s bias)' % ('with' if b is not None else 'no'), ncl(out), want, w32)
        o = out.permute(0, 2, 1).contiguous().cpu().view(torch.int32).numpy().reshape(rows, c, lo, 2)
        partner = np.where(sel, o[..., 0], o[..., 1])
        assert (partner == 0).all()                              # bitwise +0.0
        if b is None:
            assert np.array_equal(ncl(out), want)                # a copy and zeros: exact
    dout = r.standard_normal((rows, c, 2 * lo)).astype(np.float32)
    dv = H.unpool2_bwd(cl(dout), words)
    pairs = dout.reshape(rows, c, lo, 2)
    assert np.array_equal(ncl(dv), np.where(sel, pairs[..., 1], pairs[..., 0]).astype(np.float64))


# ---- the output stage --------------------------------------------------------------------------------------------------------------
def _out_ref(v, b3, sel, w4, b4, x, dtype):
    vt, b3t, w4t, b4t = (R._t(a, dtype, True) for a in (v, b3, w4, b4))
    u = R.unpool2(vt + b3t[None, :, None], torch.from_numpy(sel))
    recon = TF.conv_transpose1d(u, w4t, b4t, padding=1)
    xt = R._t(x, dtype)
    loss = ((recon - xt) ** 2).mean()
    dr, = torch.autograd.grad(loss, recon, retain_graph=True)
    loss.backward()
    return dict(recon=recon.detach().numpy()[:, 0], dr=dr.numpy()[:, 0], loss=loss.detach().numpy().reshape(1), dv=vt.grad.numpy(),
                dw4=w4t.grad.numpy(), db4=b4t.grad.numpy(), db3=b3t.grad.numpy())


@pytest.mark.parametrize('rows,l', [(1, 2), (3, 6), (4, 16), (40, 224)])
def test_output_stage_against_float64(H, rows, l):
    r = np.random.RandomState(7)
    c, lo = 64, l // 2
    v, b3 = f32ok(r.standard_normal((rows, c, lo))), f32ok(r.uniform(-0.5, 0.5, c))
    w4, b4 = f32ok(r.uniform(-1, 1, (c, 1, 3)) / np.sqrt(192.0)), f32ok(r.uniform(-0.5, 0.5, 1))
    x = f32ok(r.standard_normal((rows, 1, l)))
    sel = r.rand(rows, c, lo) < 0.5
    sel[:, :, 0] = np.arange(c)[None, :] % 2 == 0                # both kinds at the row ends: the l = 0 and l = L - 1 taps
    sel[:, :, -1] = np.arange(c)[None, :] % 3 == 0
    want, w32 = _out_ref(v, b3, sel, w4, b4, x, F64), _out_ref(v, b3, sel, w4, b4, x, F32)
    words = H.sel_from_bool(torch.from_numpy(sel)).cuda()
    vd, b3d, w4d, b4d, xd = cl(v), dev(b3), dev(w4), dev(b4), dev(x[:, 0])
    recon, dr, loss = H.ae_out_fwd(vd, b3d, words, w4d, b4d, xd)
    dv, dw4, db4 = H.ae_out_bwd(dr, vd, b3d, words, w4d)
    db3 = H.reduce_rows(dv.view(-1, c))
    got = dict(recon=recon.cpu().numpy(), dr=dr.cpu().numpy(), loss=loss.cpu().numpy(), dv=ncl(dv), dw4=dw4.cpu().numpy(),
               db4=db4.cpu().numpy(), db3=db3.cpu().numpy())
    for name in ('recon', 'dr', 'loss', 'dv', 'dw4', 'db4', 'db3'):
        held('out stage (%d, %d) %s' % (rows, l, name), got[name], want[name], w32[name])
    for edge in (0, l - 1):                                      # the first and last output of every row, on their own
        held('out stage recon[%d]' % edge, got['recon'][:, edge], want['recon'][:, edge], w32['recon'][:, edge])
    # accumulate: added to what the destinations hold
    dw_acc, db_acc = torch.ones_like(dw4), torch.ones_like(db4)
    H.ae_out_bwd(dr, vd, b3d, words, w4d, dw4=dw_acc, db4=db_acc, accumulate=True)
    assert torch.equal(dw_acc, 1.0 + dw4) and torch.equal(db_acc, 1.0 + db4)


# ---- the whole model -----------------------------------------------------------------------------------------------------------------
_REF = {}


def _ref(n, l, forced):
    """ae_ref in float64 at a golden shape: teacher-forced with the golden bits, or free-running.  Computed once."""
    if (n, l, forced) not in _REF:
        g, sels = R.load_golden(n, l)
        seed = int(g['seed'][0])
        x, p = R.seeded_rows(n, l, seed), R.seeded_params(seed)
        _REF[(n, l, forced)] = (g, sels, x, p, R.model(x, p, sels=sels if forced else None))
    return _REF[(n, l, forced)]


def _cnn(M, p):
    cnn = M.AutoencoderCNN()
    missing, unexpected = cnn.load_state_dict({k: torch.tensor(v, dtype=F32) for k, v in R.full_state_dict(p).items()}, strict=False)
    assert not unexpected and all(k.split('.')[-1] in ('running_mean', 'running_var', 'num_batches_tracked') for k in missing)
    return cnn.cuda()


def _windows(n):
    return {4: (2, 2), 6: (2, 3), 3: (1, 3)}[n]


@pytest.mark.parametrize('network', [False, True], ids=['cnn', 'network'])
@pytest.mark.parametrize('n,l', R.MODEL_SHAPES)
def test_model_teacher_forced_with_the_golden_bits(M, H, n, l, network):
    g, sels, x, p, m64 = _ref(n, l, True)
    cnn = _cnn(M, p)
    words = [H.sel_from_bool(torch.from_numpy(s)).cuda() for s in sels]
    xd = dev(x)
    if network:
        net = M.AutoencoderNetwork(cnn)
        loss, recon = net.forward_loss(xd.view(*_windows(n), 1, l), None, sels=words)
    else:
        loss, recon = cnn.forward_loss(xd, words)
    assert tuple(recon.shape) == (n, 1, l) and not recon.requires_grad
    loss.backward()
    torch.cuda.synchronize()

    def check(name, got):
        err, b = R.rel_l2(got, m64[name]), R.bound(float(np.ravel(g['err32/' + name])[0]))
        log('%-28s err %.3e  bound %.3e' % (name, err, b))
        assert err <= b, '%s: rel-l2 %.3e over the bound %.3e' % (name, err, b)
    check('recon', recon.detach().cpu().numpy())
    check('loss', loss.detach().cpu().numpy())
    grads = {name: q.grad for name, q in cnn.named_parameters() if not name.startswith('encoder.')}
    assert len(grads) == 24 and all(v is not None for v in grads.values())
    zeros = ['conv_down%d.bias' % k for k in range(1, 5)]
    for name, v in grads.items():
        if name in zeros:
            assert 'exact_zero/grad/' + name in g.files and float(v.abs().max()) == 0.0, name
        else:
            check('grad/' + name, v.detach().cpu().numpy())
    for k in range(1, 5):
        bn = getattr(cnn, 'bn%d' % k)
        check('running_mean/bn%d' % k, bn.running_mean.cpu().numpy())
        check('running_var/bn%d' % k, bn.running_var.cpu().numpy())
        assert int(bn.num_batches_tracked) == 1
    for a, b in zip(cnn.last_sels, words):                       # the bits were taken as given
        assert torch.equal(a, b)


@pytest.mark.parametrize('n,l', R.MODEL_SHAPES)
def test_free_running_decisions_meet_the_condition(M, H, n, l):
    g, _, x, p, m64 = _ref(n, l, False)
    cnn = _cnn(M, p)
    with torch.no_grad():
        cnn(dev(x))
    mine = [H.sel_to_bool(s.cpu()).numpy() for s in cnn.last_sels]
    for k, (pairs, differ, gap, near) in enumerate(R.decision_report(mine, m64['sel'], m64['gap']), 1):
        log('stage %d: %d pairs, %d differ (largest float64 gap %.3e), %d within 1e-4' % (k, pairs, differ, gap, near))
        assert differ == 0 or gap < 1e-4
        assert near <= 0.0005 * pairs                            # (the condition cannot hide a wrong kernel)


def test_encoder_output_at_the_golden_shape(M):
    g, _, x, p, _ = _ref(3, 224, False)
    want = R.model(x, p, encoder_only=True)['encoded']
    cnn = _cnn(M, p)
    net = M.AutoencoderNetwork(cnn)
    with pytest.raises(NotImplementedError, match='second stage'):
        net.breath_block(dev(x))
    with torch.no_grad():
        enc = net.breath_block(dev(x))
    assert tuple(enc.shape) == (3, 512, 1)
    err, b = R.rel_l2(enc.cpu().numpy(), want), R.bound(float(np.ravel(g['err32/encoded'])[0]))
    log('encoded err %.3e bound %.3e' % (err, b))
    assert err <= b


def test_f32_only(M):
    from deepards_amd import functional as F_
    cnn = M.AutoencoderCNN().cuda()
    x = torch.randn(4, 1, 32, device='cuda')
    for name in ('bf16', 'f32x3p'):
        F_.set_conv_dtype(name)
        try:
            with pytest.raises(NotImplementedError, match='fp32 conv arithmetic'):
                cnn(x)
        finally:
            F_.set_conv_dtype('f32')


# ---- eval() ---------------------------------------------------------------------------------------------------------------------------
EVAL_SEED, EVAL_ROWS, EVAL_L = 23, 4, 16       # (the search of _eval_case's docstring)


def _eval_buffers(seed):
    r = np.random.RandomState(100 + seed)
    return {k: (f32ok(r.uniform(-0.3, 0.3, R.CHANNELS[k])), f32ok(r.uniform(0.5, 2.0, R.CHANNELS[k]))) for k in range(1, 5)}


def _eval_compose(x, p, buffers, dtype):
    """The network from stock torch functions with eval-mode batch_norm on given running buffers.  -> recon, the smallest gap of
    a pool pair over the four stages."""
    t = {k: torch.tensor(v, dtype=dtype) for k, v in p.items()}
    h, idx, gap = torch.tensor(x, dtype=dtype), [], float('inf')
    for k in range(1, 5):
        y = TF.conv1d(h, t['conv_down%d.weight' % k], t['conv_down%d.bias' % k], padding=1)
        rm, rv = (torch.tensor(b, dtype=dtype) for b in buffers[k])
        z = TF.batch_norm(y, rm, rv, t['bn%d.weight' % k], t['bn%d.bias' % k], training=False, eps=R.EPS)
        gap = min(gap, float((z[:, :, 0::2] - z[:, :, 1::2]).abs().min()))
        h, i = TF.max_pool1d(z, 2, return_indices=True)
        idx.append(i)
    for k in range(1, 5):
        h = TF.conv_transpose1d(TF.max_unpool1d(h, idx[4 - k], 2), t['conv_up%d.weight' % k], t['conv_up%d.bias' % k], padding=1)
    return h.numpy(), gap


def _eval_case():
    """x (2, 2, 1, 16), ae_ref's seeded parameters (BatchNorm weights of both signs), running buffers drawn here.  A pool
    decision that differs between two arithmetics moves a value to the neighbouring position, which no rounding bound covers; so
    the case is one whose smallest float64 gap over all 8192 pool pairs is at least 1e-4 (the decision condition's threshold, two
    orders above fp32 rounding of values of this size): the first seed from 0 for which that holds at this shape, found by this
    same function on the CPU, and asserted again here."""
    seed = EVAL_SEED
    x, p = R.seeded_rows(EVAL_ROWS, EVAL_L, seed), R.seeded_params(seed)
    buffers = _eval_buffers(seed)
    want, gap = _eval_compose(x, p, buffers, F64)
    assert gap >= 1e-4, 'the eval case must have no near-tie (smallest float64 gap %.3e)' % gap
    w32, _ = _eval_compose(x, p, buffers, F32)
    return x, p, buffers, want, w32


def test_test_step_runs_on_running_statistics(M):
    from deepards_amd.autoencoder import AutoencoderTrainer
    x, p, buffers, want, w32 = _eval_case()
    for use_graph in (False, True):
        cnn = _cnn(M, p)
        for k in range(1, 5):
            bn = getattr(cnn, 'bn%d' % k)
            bn.running_mean.copy_(dev(buffers[k][0]))
            bn.running_var.copy_(dev(buffers[k][1]))
            bn.num_batches_tracked.fill_(5)
        net = M.AutoencoderNetwork(cnn)
        before = {k: v.clone() for k, v in net.state_dict().items()}
        tr = AutoencoderTrainer(net, use_graph=use_graph)
        xd = dev(x).view(2, EVAL_ROWS // 2, 1, EVAL_L)
        recon = tr.test_step(xd)
        again = tr.test_step(xd)
        assert not net.training and tuple(recon.shape) == (EVAL_ROWS, 1, EVAL_L) and torch.equal(recon, again)
        held('test_step recon (graph %s)' % use_graph, recon.cpu().numpy(), want, w32)
        held('test_step loss', tr.last_test_loss.cpu().numpy(), ((want - x) ** 2).mean().reshape(1),
             ((w32.astype(np.float32) - x.astype(np.float32)) ** 2).mean(dtype=np.float32).reshape(1))
        for k, v in net.state_dict().items():                    # eval() moves no buffer and no parameter
            assert torch.equal(v, before[k]), k
        tr.release_graphs()


# ---- the trainer ------------------------------------------------------------------------------------------------------------------------
def _trainer_run(M, use_graph, optimizer, steps=4):
    from deepards_amd.autoencoder import AutoencoderTrainer
    p = R.seeded_params(1)
    net = M.AutoencoderNetwork(_cnn(M, p))
    tr = AutoencoderTrainer(net, optimizer=optimizer, learning_rate=0.01 if optimizer == 'sgd' else 1e-3, use_graph=use_graph)
    batches = [dev(R.seeded_rows(8, 32, 20 + i)).view(2, 4, 1, 32) for i in range(2)]
    losses = [tr.train_step(batches[i % 2]).detach().clone() for i in range(steps)]
    torch.cuda.synchronize()
    out = dict(loss=torch.cat(losses), p=tr.bucket.p.clone(), state={k: v.clone() for k, v in tr.state.items()},
               buffers=[b.clone() for b in net.buffers()], overwrite=tr.grad_overwrite)
    tr.release_graphs()
    return out


@pytest.mark.parametrize('optimizer', ['sgd', 'adam'])
def test_captured_step_matches_the_eager_step_bit_for_bit(M, optimizer):
    eager, graph, graph2 = (_trainer_run(M, g, optimizer) for g in (False, True, True))
    assert torch.isfinite(eager['loss']).all() and float((eager['loss'][0] - eager['loss'][2]).abs()) > 0
    log('losses', eager['loss'].tolist(), 'captured without the gradient zero-fill:', graph['overwrite'])
    for other in (graph, graph2):
        assert torch.equal(eager['loss'], other['loss']) and torch.equal(eager['p'], other['p'])
        assert set(eager['state']) == set(other['state']) and all(torch.equal(eager['state'][k], other['state'][k]) for k in eager['state'])
        assert all(torch.equal(a, b) for a, b in zip(eager['buffers'], other['buffers']))


def test_twenty_sgd_steps_lower_the_loss_and_snapshot_round_trips(M):
    from deepards_amd.autoencoder import AutoencoderTrainer
    net = M.AutoencoderNetwork(_cnn(M, R.seeded_params(2)))
    tr = AutoencoderTrainer(net, optimizer='sgd', learning_rate=0.01, clip_grad=False)
    x = dev(R.seeded_rows(8, 32, 9)).view(2, 4, 1, 32)
    losses = [float(tr.train_step(x)) for _ in range(20)]
    log('loss over 20 steps: %.5f -> %.5f' % (losses[0], losses[-1]))
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    with pytest.raises(ValueError, match='batch alone'):
        tr.train_step(x, x)
    with pytest.raises(ValueError, match='windows'):
        tr.train_step(x.view(8, 1, 32))
    snap = tr.snapshot()
    nxt = float(tr.train_step(x))
    tr.train_step(x)
    tr.restore(snap)
    assert torch.equal(tr.bucket.p, snap['p']) and all(torch.equal(a, b) for a, b in zip(net.buffers(), snap['buffers']))
    assert all(torch.equal(tr.state[k], v) for k, v in snap['state'].items()) and tr.steps == snap['steps']
    assert float(tr.train_step(x)) == nxt
    tr.release_graphs()


def test_driver_class_trains_and_books_the_regression_meters(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from deepards_amd import train_ards_detector as T
    from deepards_amd.ingest import IngestedDataset
    r = np.random.RandomState(4)
    n, nb, l = 16, 2, 32
    w = r.standard_normal((n, nb, 1, l)) * 3.0 + 10.0
    patients = np.repeat(['a', 'b', 'c', 'd'], n // 4)
    target = np.where(np.isin(patients, ['a', 'c'])[:, None], [[0.0, 1.0]], [[1.0, 0.0]])
    path = IngestedDataset(w, target, patients, np.zeros((n, nb)), {}, nb, 'unpadded_downsampled_autoencoder_sequences').save_npz(
        str(tmp_path / 'ae_train.npz'))
    cls = T.AutoencoderModel(T.make_args(network='autoencoder', base_network='basic_cnn_ae', train_from_pickle=path, kfolds=2,
                                         epochs=2, batch_size=4, seed=3, cuda=False, cuda_no_dp=True, n_sub_batches=nb,
                                         save_model='ae.pth', saved_models_dir=str(tmp_path)))
    res = cls.train_and_test()
    summary = cls.perform_post_modeling_actions()
    for fold in (0, 1):
        assert len(res.get_meter('loss', fold)) > 0 and np.isfinite(res.get_meter('loss', fold)).all()
        for name in ('test_mae', 'r2', 'test_mse', 'test_loss'):
            vals = res.get_meter(name, fold)
            assert len(vals) > 0 and np.isfinite(vals).all(), name
            assert '%s/%d' % (name, fold) in summary
        # test_mse is sklearn's mean over samples and outputs of the batch: the step's own loss, computed on the host
        assert np.allclose(res.get_meter('test_mse', fold), res.get_meter('test_loss', fold), rtol=1e-4)
    from deepards_amd import checkpoint
    back = checkpoint.load_autoencoder(str(tmp_path / 'ae-fold1.pth'))
    assert all(torch.equal(a.cpu(), b.cpu()) for a, b in zip(back.state_dict().values(), cls.model.state_dict().values()))
    with pytest.raises(ValueError, match='not built in this package'):
        checkpoint.load_base_network(str(tmp_path / 'ae-fold1.pth'), T.base_networks, {})


# ---- memory discipline: the five checks of tests/tools/poison.py on every new wrapper --------------------------------------------
def _rand(shape, seed):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape).astype(np.float32)).cuda()


def _words(shape, seed):
    return torch.from_numpy(np.random.RandomState(seed).randint(-2 ** 31, 2 ** 31, size=shape, dtype=np.int64).astype(np.int32)).cuda()


def _stats(w, c, seed):
    r = np.random.RandomState(seed)
    return (dev(r.uniform(-0.5, 0.5, (w, c))), dev(r.uniform(0.5, 1.5, (w, c))), dev(r.uniform(-1.5, 1.5, c)), dev(r.uniform(-0.5, 0.5, c)))


def _op_cases():
    from deepards_amd import hip_ops as H
    cases = []
    for tag, (rows, R_, lin, c) in (('a', (4, 2, 6, 64)), ('b', (6, 3, 130, 32))):
        w, lo = rows // R_, lin // 2

        def pool_build(rows=rows, R_=R_, lin=lin, c=c, w=w, lo=lo):
            mean, invstd, gamma, beta = _stats(w, c, 1)
            return dict(y=_rand((rows, lin, c), 2), R=R_, mean=mean, invstd=invstd, gamma=gamma, beta=beta,
                        out=torch.zeros((rows, lo, c), device='cuda'), sel=torch.zeros((rows, lo, c // 32), dtype=torch.int32, device='cuda'))

        def forced_build(rows=rows, lo=lo, c=c, build=pool_build):
            d = build()
            d.pop('sel')
            d['sel_in'] = _words((rows, lo, c // 32), 3)
            return d

        def bwd_build(rows=rows, R_=R_, lin=lin, c=c, w=w, lo=lo):
            mean, invstd, gamma, beta = _stats(w, c, 1)
            return dict(dout=_rand((rows, lo, c), 4), sel=_words((rows, lo, c // 32), 3), y=_rand((rows, lin, c), 2), R=R_, mean=mean,
                        invstd=invstd, gamma=gamma, beta=beta, out=torch.zeros((rows, lin, c), device='cuda'))
        axis2 = {'[0]': 0, '[1]': 0}
        cases += [
            P.OpCase('bn_maxpool2_idx_fwd/' + tag, 'pool_fwd', pool_build,
                     lambda y, R, mean, invstd, gamma, beta, out, sel: H.bn_maxpool2_idx_fwd(y, R, mean, invstd, gamma, beta, out=out, sel=sel),
                     dests=('out', 'sel'), rows=dict(inputs=['y'], R=R_, axis=axis2)),
            P.OpCase('bn_maxpool2_idx_fwd/forced/' + tag, 'pool_fwd_forced', forced_build,
                     lambda y, R, mean, invstd, gamma, beta, out, sel_in: H.bn_maxpool2_idx_fwd(y, R, mean, invstd, gamma, beta, sel_in=sel_in,
                                                                                               out=out)[0],
                     dests=('out',), rows=dict(inputs=['y'], R=R_, axis={'': 0})),
            P.OpCase('bn_maxpool2_idx_bwd/' + tag, 'pool_bwd', bwd_build,
                     lambda dout, sel, y, R, mean, invstd, gamma, beta, out: H.bn_maxpool2_idx_bwd(dout, sel, y, R, mean, invstd, gamma, beta,
                                                                                                   out=out),
                     dests=('out',), rows=dict(inputs=['dout', 'y'], R=R_, axis={'[0]': 0, '[1]': 1})),
        ]
    for tag, (rows, lo, c) in (('a', (4, 3, 64)), ('b', (3, 17, 96))):
        def un_build(rows=rows, lo=lo, c=c):
            return dict(v=_rand((rows, lo, c), 5), sel=_words((rows, lo, c // 32), 6), bias=_rand((c,), 7),
                        out=torch.zeros((rows, 2 * lo, c), device='cuda'))

        def unb_build(rows=rows, lo=lo, c=c):
            return dict(dout=_rand((rows, 2 * lo, c), 8), sel=_words((rows, lo, c // 32), 6), out=torch.zeros((rows, lo, c), device='cuda'))
        cases += [
            P.OpCase('unpool2_fwd/' + tag, 'unpool_fwd', un_build, lambda v, sel, bias, out: H.unpool2_fwd(v, sel, bias, out=out),
                     dests=('out',), rows=dict(inputs=['v'], R=1, axis={'': 0})),
            P.OpCase('unpool2_bwd/' + tag, 'unpool_bwd', unb_build, lambda dout, sel, out: H.unpool2_bwd(dout, sel, out=out),
                     dests=('out',), rows=dict(inputs=['dout'], R=1, axis={'': 0})),
        ]
    for tag, (rows, l) in (('a', (4, 6)), ('b', (9, 40))):
        def of_build(rows=rows, l=l):
            return dict(v=_rand((rows, l // 2, 64), 9), bias3=_rand((64,), 10), sel1=_words((rows, l // 2, 2), 11),
                        w4=_rand((64, 1, 3), 12), bias4=_rand((1,), 13), x=_rand((rows, l), 14))

        def ob_build(rows=rows, l=l):
            return dict(dr=_rand((rows, l), 15), v=_rand((rows, l // 2, 64), 9), bias3=_rand((64,), 10), sel1=_words((rows, l // 2, 2), 11),
                        w4=_rand((64, 1, 3), 12), dw4=torch.zeros((64, 1, 3), device='cuda'), db4=torch.zeros((1,), device='cuda'))
        cases += [
            P.OpCase('ae_out_fwd/' + tag, 'out_fwd', of_build, lambda v, bias3, sel1, w4, bias4, x: H.ae_out_fwd(v, bias3, sel1, w4, bias4, x),
                     rows=dict(inputs=['v', 'x'], R=1, axis={'[0]': 0, '[1]': 0, '[2]': None})),
            P.OpCase('ae_out_bwd/' + tag, 'out_bwd', ob_build,
                     lambda dr, v, bias3, sel1, w4, dw4, db4: H.ae_out_bwd(dr, v, bias3, sel1, w4, dw4=dw4, db4=db4),
                     dests=('dw4', 'db4'), rows=dict(inputs=['dr', 'v'], R=1, axis={'[0]': 0, '[1]': None, '[2]': None})),
        ]
    return cases


_CASE_NAMES = ['%s/%s' % (op, tag) for op in ('bn_maxpool2_idx_fwd', 'bn_maxpool2_idx_fwd/forced', 'bn_maxpool2_idx_bwd', 'unpool2_fwd',
                                              'unpool2_bwd', 'ae_out_fwd', 'ae_out_bwd') for tag in ('a', 'b')]


@pytest.mark.parametrize('check', P.CHECKS)
@pytest.mark.parametrize('name', _CASE_NAMES)
def test_memory_discipline(H, name, check):
    cases = {c.name: c for c in _op_cases()}
    assert sorted(cases) == sorted(_CASE_NAMES)
    case = cases[name]
    other = next(c for c in cases.values() if c.family == case.family and c is not case)
    problems = P.run_check(check, case, other)
    assert not problems, '\n'.join(problems)
