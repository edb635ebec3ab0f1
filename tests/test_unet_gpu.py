"""The UNet autoencoder on the GPU: its elementwise kernels bit for bit against float32 numpy (slices of pitched buffers inside
guard bands), the upsample and the output stage against float64 within componentwise / per-tensor bounds, the k3 convs at the
concat's channel counts on exact integer operands, the whole model against the goldens of the real reference classes and against
tests/tools/unet_ref.py under the decisions the run took, eval(), the trainer (eager = captured, bit for bit) and the driver."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'tools'))
pytestmark = pytest.mark.gpu

import unet_ref as R  # noqa: E402
import exact_conv as X  # noqa: E402
import poison as P  # noqa: E402
from oracle.weights import digest  # noqa: E402

F64, F32 = torch.float64, torch.float32
U = 2.0 ** -24


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


def dev(a):
    return torch.as_tensor(np.asarray(a), dtype=F32).contiguous().cuda()


def cl(a):
    """(N, C, L) array -> (N, L, C) float32 CUDA tensor."""
    return torch.as_tensor(np.asarray(a), dtype=F32).permute(0, 2, 1).contiguous().cuda()


def ncl(t):
    """(N, L, C) CUDA tensor -> (N, C, L) float64 array."""
    return t.detach().permute(0, 2, 1).cpu().numpy().astype(np.float64)


def host(t):
    return t.detach().cpu().numpy()


def held(name, got, ref64, ref32):
    """rel-l2 of ``got`` against float64 within ae_ref.bound(err32), err32 the float32 reference's own error."""
    err32, err = R.rel_l2(ref32, ref64), R.rel_l2(got, ref64)
    log('%-28s err %.3e  err32 %.3e  bound %.3e' % (name, err, err32, R.bound(err32)))
    assert err <= R.bound(err32), '%s: rel-l2 %.3e over the bound %.3e (err32 %.3e)' % (name, err, R.bound(err32), err32)


def same(name, got, want):
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), '%s: %d of %d elements differ in their bits, first %r vs %r' % (
        name, int(bad.sum()), bad.size, got[bad][0], want[bad][0])


# ---- the elementwise kernels: bit for bit -------------------------------------------------------------------------------------
LD, OFF = 160, 32
ELEMENTWISE = [(3, 2, 32), (3, 6, 32), (3, 2, 96), (3, 6, 96), (5, 26, 64)]          # (the last: more than one block)


def _relu(v):
    return np.where(v > 0, v, np.float32(0)).astype(np.float32)


def _vals(shape, seed, bias=None):
    """Normal values with hand-placed pairs at the head of every row (positions 0..1 and, from L = 6, 2..5) of the first channels:
    equal positives (the first wins), both <= 0, -0.0 / +0.0, and a bias pushing a value across 0 either way."""
    r = np.random.RandomState(seed)
    a = r.standard_normal(shape).astype(np.float32)
    a[r.random_sample(shape) < 0.1] = 0.0
    b = np.zeros(shape[2], np.float32) if bias is None else bias
    a[:, 0, 0], a[:, 1, 0] = 1.5 - b[0], 1.5 - b[0]                                  # equal positives after the bias
    a[:, 0, 1], a[:, 1, 1] = -0.0, 0.0
    a[:, 0, 2], a[:, 1, 2] = 0.0, -0.0
    a[:, 0, 3], a[:, 1, 3] = -2.0 - abs(b[3]), -1.0 - abs(b[3])                      # both <= 0
    if shape[1] >= 6:
        a[:, 2, 0], a[:, 3, 0] = -b[0], np.nextafter(np.float32(-b[0]), np.float32(1e9))      # exactly 0 after the bias, and one ulp over
        a[:, 4, 1], a[:, 5, 1] = np.float32(1e-3), np.float32(-1e-3)                          # (bias[1] is made +-2e-3: across 0)
    return a


def _bias(c, seed):
    b = np.random.RandomState(seed).uniform(-0.5, 0.5, c).astype(np.float32)
    b[1] = np.float32(-2e-3 if seed % 2 else 2e-3)
    b[2] = np.float32(-0.0)                                                          # (y = -0.0 stays -0.0 under this bias)
    return b


@pytest.mark.parametrize('rows,l,c', ELEMENTWISE, ids=str)
def test_elementwise_kernels_bit_for_bit_in_slices_inside_guards(H, rows, l, c):
    b = _bias(c, l + c)
    y = _vals((rows, l, c), 1 + l + c, b)
    act = _relu(y + b)
    pooled = np.where(act[:, 1::2] > act[:, 0::2], act[:, 1::2], act[:, 0::2])
    with P.poisoned_allocations():
        # bias_relu, in place on a slice
        v, g = P.pitched(dev(y), LD, OFF, name='y')
        assert H.unet_bias_relu(v, dev(b)) is v
        same('bias_relu', host(v), act)
        P.assert_guards_intact(g)
        # bias_relu + pool: the skip in place, the pooled map contiguous
        v, g = P.pitched(dev(y), LD, OFF, name='y')
        out = H.unet_bias_relu_pool2_fwd(v, dev(b))
        same('pool skip', host(v), act)
        same('pooled', host(out), pooled)
        assert out.is_contiguous() and not P.has_poison(out)
        P.assert_guards_intact(g)
        # the gradients that reach a skip map
        r = np.random.RandomState(7)
        dsk, dpo = r.standard_normal((rows, l, c)).astype(np.float32), r.standard_normal((rows, l // 2, c)).astype(np.float32)
        second = act[:, 1::2] > act[:, 0::2]
        want = dsk.copy()
        want[:, 0::2] = np.where(second, dsk[:, 0::2], dsk[:, 0::2] + dpo)
        want[:, 1::2] = np.where(second, dsk[:, 1::2] + dpo, dsk[:, 1::2])
        want = np.where(act > 0, want, np.float32(0)).astype(np.float32)
        av, ga = P.pitched(dev(act), LD, OFF, name='a')
        dv, gd = P.pitched(dev(dsk), LD + 32, 64, name='dskip')
        dy = H.unet_pool2_skip_bwd(dev(dpo), dv, av)
        same('pool2_skip_bwd', host(dy), want)
        assert dy.is_contiguous()
        P.assert_guards_intact([ga, gd])
        same('a untouched', host(av), act)
        # relu_bwd, out of place and in place
        d = r.standard_normal((rows, l, c)).astype(np.float32)
        want = np.where(act > 0, d, np.float32(0)).astype(np.float32)
        same('relu_bwd', host(H.unet_relu_bwd(dev(d), av)), want)
        dd, gdd = P.guarded(dev(d), name='dout')
        assert H.unet_relu_bwd(dd, av, out=dd) is dd
        same('relu_bwd in place', host(dd), want)
        P.assert_guards_intact([ga, gdd])
    # -0.0 never leaves a relu, and ties at zero keep the first member
    assert not np.signbit(host(out)).any() and not np.signbit(act).any()


def test_elementwise_wrappers_refuse_bad_operands(H):
    y = torch.zeros(3, 6, 32, device='cuda')
    with pytest.raises(ValueError):
        H.unet_bias_relu(y, torch.zeros(16, device='cuda'))
    with pytest.raises(ValueError):
        H.unet_bias_relu_pool2_fwd(torch.zeros(3, 5, 32, device='cuda'), torch.zeros(32, device='cuda'))
    with pytest.raises(ValueError):
        H.unet_relu_upsample2_fwd(y, torch.zeros(32, device='cuda'), torch.zeros(3, 11, 32, device='cuda'))
    with pytest.raises(ValueError):
        H.unet_pool2_skip_bwd(torch.zeros(3, 3, 32, device='cuda'), torch.zeros(3, 6, 64, device='cuda'), y)
    with pytest.raises(ValueError):
        H.unet_out_fwd(y, torch.zeros(1, 32, 1, device='cuda'), torch.zeros(1, device='cuda'), torch.zeros(3, 6, device='cuda'))


# ---- the upsample ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', [32, 64])
@pytest.mark.parametrize('l', [1, 2, 3, 28])
def test_upsample_forward_and_backward_against_float64(H, l, c):
    rows = 3
    b = _bias(c, l)
    r = np.random.RandomState(100 * l + c)
    y = r.standard_normal((rows, l, c)).astype(np.float32)
    y[:, 0, 0] = -b[0]                                                              # y + b exactly 0: masked
    y[:, -1, 3] = np.nextafter(np.float32(-b[3]), np.float32(1e9))                  # one ulp of the bias over (a normal number)
    pre = (y + b).astype(np.float32)
    x = _relu(pre).astype(np.float64)
    want = R.upsample2(x.transpose(0, 2, 1)).transpose(0, 2, 1)                     # (rows, 2 L, C)
    scale = R.upsample_terms(x.transpose(0, 2, 1)).transpose(0, 2, 1)
    with P.poisoned_allocations():
        ov, go = P.pitched(torch.empty(rows, 2 * l, c, device='cuda'), LD, OFF, name='out')
        H.unet_relu_upsample2_fwd(dev(y), dev(b), ov)
        got = host(ov).astype(np.float64)
        P.assert_guards_intact(go)
        err = np.abs(got - want)
        log('upsample fwd L %d C %d: worst err / bound %.3f' % (l, c, float((err / np.maximum(4 * U * scale, 1e-300)).max())))
        assert (err <= 4 * U * scale).all()
        same('out[0] = x[0]', got[:, 0].astype(np.float32), x[:, 0].astype(np.float32))
        same('out[2L-1] = x[L-1]', got[:, -1].astype(np.float32), x[:, -1].astype(np.float32))
        d = r.standard_normal((rows, 2 * l, c)).astype(np.float32)
        dv, gd = P.pitched(dev(d), LD, OFF, name='d')
        dy = H.unet_relu_upsample2_bwd(dv, dev(y), dev(b))
        P.assert_guards_intact(gd)
    got = host(dy).astype(np.float64)
    d64 = d.astype(np.float64).transpose(0, 2, 1)
    want = R.upsample2_t(d64).transpose(0, 2, 1)
    scale = R.upsample_t_terms(d64).transpose(0, 2, 1)
    mask = pre > 0
    assert (got[~mask] == 0).all() and not np.signbit(host(dy)[~mask]).any()
    assert (np.abs(got - want)[mask] <= (8 * U * scale)[mask]).all()
    assert (got[mask] != 0).mean() > 0.99                                           # the mask is exactly float32(y) + float32(b) > 0


# ---- the output stage -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows,l', [(3, 8), (5, 40)])
def test_output_stage_against_float64(H, rows, l):
    r = np.random.RandomState(rows * l)
    a = _relu(r.standard_normal((rows, l, 64)).astype(np.float32))
    w = (r.standard_normal((1, 64, 1)) * 0.3).astype(np.float32)
    b = np.array([0.25], np.float32)
    x = r.standard_normal((rows, l)).astype(np.float32)

    def ref(dt):
        a_, w_, x_ = a.astype(dt), w.astype(dt)[0, :, 0], x.astype(dt)
        recon = (a_ * w_).sum(axis=2, dtype=dt) + dt(b[0])
        e = recon - x_
        dr = dt(2) * e / dt(rows * l)
        return dict(recon=recon, dr=dr, loss=np.array([(e * e).mean(dtype=dt)]), dy=np.where(a_ > 0, dr[:, :, None] * w_, dt(0)),
                    dw=np.einsum('nl,nlc->c', dr, a_).reshape(1, 64, 1), db=np.array([dr.sum(dtype=dt)]))
    r64, r32 = ref(np.float64), ref(np.float32)
    with P.poisoned_allocations():
        recon, dr, loss = H.unet_out_fwd(dev(a), dev(w), dev(b), dev(x))
        dy, dw, db = H.unet_out_bwd(dr, dev(a), dev(w))
        again = H.unet_out_fwd(dev(a), dev(w), dev(b), dev(x))
    assert all(torch.equal(p, q) for p, q in zip((recon, dr, loss), again))
    scale = abs(float(b[0])) + (np.abs(a.astype(np.float64)) * np.abs(w.astype(np.float64)[0, :, 0])).sum(axis=2)
    assert (np.abs(host(recon).astype(np.float64) - r64['recon']) <= 66 * U * scale).all()
    for name, got in (('dr', dr), ('loss', loss), ('dy', dy), ('dw', dw), ('db', db)):
        held('out %s rows %d L %d' % (name, rows, l), host(got), r64[name], r32[name])
    assert (host(dy)[a <= 0] == 0).all()
    # with destinations: written there, or added
    dw2, db2 = torch.full((1, 64, 1), 2.0, device='cuda'), torch.full((1,), 3.0, device='cuda')
    H.unet_out_bwd(dr, dev(a), dev(w), dw=dw2, db=db2, accumulate=True)
    assert torch.equal(dw2, dw + 2.0) and torch.equal(db2, db + 3.0)
    H.unet_out_bwd(dr, dev(a), dev(w), dw=dw2, db=db2)
    assert torch.equal(dw2, dw) and torch.equal(db2, db)


# ---- the k3 convs at the concat's channel counts -----------------------------------------------------------------------------------
@pytest.mark.parametrize('l', [3, 8])
@pytest.mark.parametrize('ci,co', [(768, 256), (384, 128), (192, 64)])
def test_convs_at_the_concat_shapes_are_exact_on_integer_operands(H, ci, co, l):
    """Integer operands in {-2 .. 2}: every intermediate of the direct and F(2,3) kernels (halves in the taps) is an fp32 number,
    so forward, data gradient and weight gradient must EQUAL the float64 conv (tests/tools/exact_conv.py's argument).  The input
    is a whole pitched buffer (the concat), and the output of the skip conv -- co -> co, as dconv_down writes it -- a slice."""
    from deepards_amd import functional as F_
    import torch.nn.functional as TF
    rows = 4
    assert H.conv_kernel(co, ci, 3, 1, 1, False, l) in (H.WINO2, H.DIRECT)
    x, w, dy = X.operand(1, rows, ci, l), X.weight(2, co, ci, 3), X.operand(3, rows, co, l)
    xt, wt, dyt = (torch.tensor(v, dtype=F64, requires_grad=True) for v in (x, w, dy))
    yt = TF.conv1d(xt, wt, padding=1)
    yt.backward(dyt)
    xd, wd, dyd = cl(x), dev(w), cl(dy)
    assert np.array_equal(ncl(F_._conv_fwd(xd, wd, 1, 1)), yt.detach().numpy())
    assert np.array_equal(ncl(F_._conv_dgrad(dyd, wd, 1, 1, l)), xt.grad.numpy())
    assert np.array_equal(host(F_._wgrad(dyd, xd, 3, 1, 1, None)), wt.grad.numpy())
    (slab,) = H.conv_wgrad_multi([(dyd, xd, 3, 1, 1)])                               # the batched form a training step launches
    dw = torch.empty(co, ci, 3, device='cuda')
    H.wgrad_reduce_multi([(slab, dw)], accumulate=False)
    assert np.array_equal(host(dw), wt.grad.numpy())
    # the skip conv co -> co into the last co channels of a (rows, L, 3 co) buffer; its neighbour slice stays as it was
    ws, a = X.weight(4, co, co, 3), X.operand(5, rows, co, l)
    cat = P.fill_poison(torch.empty(rows, l, 3 * co, device='cuda'))
    F_._conv_fwd(cl(a), dev(ws), 1, 1, out=cat[:, :, 2 * co:])
    want = TF.conv1d(torch.tensor(a, dtype=F64), torch.tensor(ws, dtype=F64), padding=1).numpy()
    assert np.array_equal(ncl(cat[:, :, 2 * co:]), want)
    assert P.count_poison(cat[:, :, :2 * co]) == rows * l * 2 * co


# ---- the whole model -----------------------------------------------------------------------------------------------------------------
def _unet(M, params):
    net = M.UNet(1)
    net.load_state_dict({k: torch.tensor(v, dtype=F32) for k, v in R.full_state_dict(params).items()}, strict=True)
    return net.cuda()


_RUNS = {}


def _run(M, n, l):
    """One train-mode pass of the model at a golden shape (shared by the tests below): its outputs, gradients and decisions."""
    if (n, l) not in _RUNS:
        from deepards_amd import functional as F_
        g = R.load_golden(n, l)
        seed = int(g['seed'][0])
        params, x = R.seeded_params(seed), R.seeded_rows(n, l, seed)
        net = M.AutoencoderNetwork(_unet(M, params))
        net.train()
        F_.DECISION_TAP = tap = []
        try:
            loss, recon = net.forward_loss(dev(x).view(1, n, 1, l))
        finally:
            F_.DECISION_TAP = None
        loss.backward()
        torch.cuda.synchronize()
        assert len(tap) == 14
        acts, relu, pool = [], [], []
        for t in tap:                                  # a stored activated map, or (y, bias) of a fused upsample input
            pre = t if isinstance(t, torch.Tensor) else (t[0] + t[1])            # (the same float32 add as the kernels')
            acts.append(pre)
            relu.append(ncl(pre) > 0)
        for k in (1, 3, 5):                            # the skip maps: dconv_down1..3's second ReLU
            a = ncl(acts[k])
            pool.append(a[:, :, 1::2] > a[:, :, 0::2])
        grads = {name: host(p.grad) for name, p in net.base_network.named_parameters()}
        _RUNS[(n, l)] = dict(g=g, x=x, params=params, net=net, recon=host(recon), loss=host(loss), grads=grads, dec=(relu, pool))
    return _RUNS[(n, l)]


@pytest.mark.parametrize('n,l', R.MODEL_SHAPES)
def test_model_output_and_loss_against_the_reference_golden(M, n, l):
    run = _run(M, n, l)
    g = run['g']
    assert run['recon'].shape == (n, 1, l)
    for name, got, want in (('recon', run['recon'], g['full/recon']), ('loss', run['loss'], g['loss'])):
        err, bnd = R.rel_l2(got, want), R.bound(float(g['err32/' + name]))
        log('%s (%d, %d): err %.3e  err32 %.3e  bound %.3e' % (name, n, l, err, float(g['err32/' + name]), bnd))
        assert err <= bnd, name


@pytest.mark.parametrize('n,l', R.MODEL_SHAPES)
def test_model_gradients_under_the_decisions_the_run_took(M, n, l):
    run = _run(M, n, l)
    g = run['g']
    flips, near = R.decisions_differ(run['dec'], R.golden_decisions(g)), int(g['near'][0])
    log('(%d, %d): %d decisions differ from the golden\'s, %d of its decisions are near-ties' % (n, l, flips, near))
    assert flips <= near                               # (the matching below cannot hide a wrong mask)
    ref = R.forward_backward(run['x'], run['params'], decisions=run['dec'])
    worst = []
    for name, _ in R.param_names():
        err, bnd = R.rel_l2(run['grads'][name], ref['grad/' + name]), R.bound(float(g['err32/grad/' + name]))
        log('%-24s err %.3e  err32 %.3e  bound %.3e' % (name, err, float(g['err32/grad/' + name]), bnd))
        if err > bnd:
            worst.append((name, err, bnd))
    assert not worst, worst


def test_eval_is_the_same_function_and_the_encoder_matches_the_golden(M):
    n, l = 3, 224
    run = _run(M, n, l)
    net, g = run['net'], run['g']
    xd = dev(run['x']).view(1, n, 1, l)
    net.eval()
    try:
        out = net(xd)
        loss, out2 = net.forward_loss(xd)
        assert not out.requires_grad and np.array_equal(host(out), run['recon']) and np.array_equal(host(loss), run['loss'])
        assert torch.equal(out, out2)
    finally:
        net.train()
    with torch.no_grad():
        enc = net.breath_block(xd.view(n, 1, l))
    assert tuple(enc.shape) == (n, 512, l // 8)
    err, bnd = R.rel_l2(digest(host(enc)), g['dig/encoded']), R.bound(float(g['err32/encoded']))
    log('encoded: err %.3e bound %.3e' % (err, bnd))
    assert err <= bnd
    with pytest.raises(NotImplementedError, match='second stage'):
        net.breath_block(xd.view(n, 1, l))


def test_f32_only(M):
    from deepards_amd import functional as F_
    net = _unet(M, R.seeded_params(0))
    x = dev(R.seeded_rows(2, 16))
    for dtype in ('bf16', 'f32x3p'):
        F_.set_conv_dtype(dtype)
        try:
            with pytest.raises(NotImplementedError, match='fp32 conv arithmetic'):
                net(x)
        finally:
            F_.set_conv_dtype('f32')


# ---- the trainer and the driver ------------------------------------------------------------------------------------------------------
def _trainer_run(M, use_graph, optimizer, steps=3):
    from deepards_amd.autoencoder import AutoencoderTrainer
    net = M.AutoencoderNetwork(_unet(M, R.seeded_params(1)))
    tr = AutoencoderTrainer(net, optimizer=optimizer, learning_rate=0.01 if optimizer == 'sgd' else 1e-3, use_graph=use_graph)
    batches = [dev(R.seeded_rows(8, 16, 20)).view(2, 4, 1, 16), dev(R.seeded_rows(6, 24, 21)).view(2, 3, 1, 24)]   # two input shapes
    losses = [tr.train_step(batches[i % 2]).detach().clone() for i in range(steps)]
    recon = tr.test_step(batches[0])
    torch.cuda.synchronize()
    out = dict(loss=torch.cat(losses), p=tr.bucket.p.clone(), state={k: v.clone() for k, v in tr.state.items()},
               recon=recon.clone(), test_loss=tr.last_test_loss.clone(), training=net.training)
    tr.release_graphs()
    return out


@pytest.mark.parametrize('optimizer', ['sgd', 'adam'])
def test_captured_step_matches_the_eager_step_bit_for_bit(M, optimizer):
    eager, graph, graph2 = (_trainer_run(M, g, optimizer) for g in (False, True, True))
    assert torch.isfinite(eager['loss']).all() and float((eager['loss'][0] - eager['loss'][2]).abs()) > 0
    log('losses', eager['loss'].tolist())
    for other in (graph, graph2):
        assert torch.equal(eager['loss'], other['loss']) and torch.equal(eager['p'], other['p'])
        assert set(eager['state']) == set(other['state']) and all(torch.equal(eager['state'][k], other['state'][k]) for k in eager['state'])
        assert torch.equal(eager['recon'], other['recon']) and torch.equal(eager['test_loss'], other['test_loss'])
    assert tuple(eager['recon'].shape) == (8, 1, 16) and tuple(eager['test_loss'].shape) == (1,) and not eager['training']


def test_test_step_returns_the_reconstruction_and_its_loss(M):
    from deepards_amd.autoencoder import AutoencoderTrainer
    params = R.seeded_params(2)
    x = R.seeded_rows(4, 16, 5)
    want = R.forward_backward(x, params, backward=False)
    for net in (M.AutoencoderNetwork(_unet(M, params)), _unet(M, params)):
        tr = AutoencoderTrainer(net, use_graph=False)
        xd = dev(x).view(2, 2, 1, 16) if isinstance(net, M.AutoencoderNetwork) else dev(x)
        recon = tr.test_step(xd)
        assert tuple(recon.shape) == (4, 1, 16) and R.rel_l2(host(recon), want['recon']) <= 1e-4
        assert R.rel_l2(host(tr.last_test_loss), want['loss']) <= 1e-4
        with pytest.raises(ValueError, match='batch alone'):
            tr.train_step(xd, xd)


def test_driver_class_trains_the_unet_and_books_the_regression_meters(tmp_path, M):
    from deepards_amd import train_ards_detector as T
    from deepards_amd.ingest import IngestedDataset
    r = np.random.RandomState(4)
    n, nb, l = 16, 2, 32
    w = r.standard_normal((n, nb, 1, l)) * 3.0 + 10.0
    patients = np.repeat(['a', 'b', 'c', 'd'], n // 4)
    target = np.where(np.isin(patients, ['a', 'c'])[:, None], [[0.0, 1.0]], [[1.0, 0.0]])
    path = IngestedDataset(w, target, patients, np.zeros((n, nb)), {}, nb, 'unpadded_downsampled_autoencoder_sequences').save_npz(
        str(tmp_path / 'unet_train.npz'))
    cls = T.AutoencoderModel(T.make_args(network='autoencoder', base_network='unet', train_from_pickle=path, kfolds=2,
                                         epochs=2, batch_size=4, seed=3, cuda=False, cuda_no_dp=True, n_sub_batches=nb,
                                         save_model='unet.pth', saved_models_dir=str(tmp_path)))
    res = cls.train_and_test()
    summary = cls.perform_post_modeling_actions()
    assert isinstance(cls.model.base_network, M.UNet)
    for fold in (0, 1):
        assert len(res.get_meter('loss', fold)) > 0 and np.isfinite(res.get_meter('loss', fold)).all()
        for name in ('test_mae', 'r2', 'test_mse', 'test_loss'):
            vals = res.get_meter(name, fold)
            assert len(vals) > 0 and np.isfinite(vals).all(), name
            assert '%s/%d' % (name, fold) in summary
        assert np.allclose(res.get_meter('test_mse', fold), res.get_meter('test_loss', fold), rtol=1e-4)
    from deepards_amd import checkpoint
    back = checkpoint.load_autoencoder(str(tmp_path / 'unet-fold1.pth'))
    assert isinstance(back.base_network, M.UNet)
    assert all(torch.equal(a.cpu(), b.cpu()) for a, b in zip(back.state_dict().values(), cls.model.state_dict().values()))
    # default arguments still build the CNN autoencoder
    assert isinstance(T.AutoencoderModel(T.make_args(network='autoencoder', cuda_no_dp=True)).get_base_network(), M.AutoencoderCNN)
