"""bf16 ACTIVATION STORAGE (BASELINE configs C3 / C5: "bf16 storage with fp32 accumulate / statistics").

The reference is fp32-only (SURVEY finding 8): there is no bf16 reference, so every bound in this file is builder-stated
-- **parity unpinned**.  What IS pinned:

* kernel level, differentially: each activation kernel run with bf16 storage equals the SAME kernel run with fp32
  storage (which tests/test_hip_ops_gpu.py pins to the numpy oracle) on inputs that are exactly representable in bf16,
  up to the one rounding of its outputs to bf16 (|a - b| <= 2^-7 |b|: one bf16 ulp, a value on a rounding boundary may
  land on either side when the fp32 sums differ in their last bits);
* model level: logits / loss / gradients against the numpy oracle run with the same rounding model
  (np_ref ... bf16_convs=True, bf16_storage=True: operands of the residual-block convs AND every stored activation /
  activation gradient rounded to bf16), and a training run whose loss goes down.
"""
import os

import numpy as np
import pytest
import torch

from oracle import np_ref
from oracle.weights import seeded_params, seeded_batch

pytestmark = pytest.mark.gpu
LOG = os.path.join(os.path.dirname(os.path.dirname(__file__)), 'gpurun_out', 'parity_model.log')


def log(*a):
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, 'a') as f:
        f.write(' '.join(str(x) for x in a) + '\n')


@pytest.fixture(scope='module')
def H():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from deepards_amd import hip_ops
    return hip_ops


class storage(object):
    """with storage(H, 'bf16'): ... -- activation storage switched for the block, fp32 restored afterwards."""

    def __init__(self, H, name):
        self.H, self.name = H, name

    def __enter__(self):
        self.H.set_act_dtype(self.name)

    def __exit__(self, *exc):
        self.H.set_act_dtype('f32')


def bf(t):
    """float32 tensor with bf16-representable values."""
    return t.bfloat16().float()


def one_ulp(a16, ref32, name, slack=1.0):
    """a16 (bf16 tensor) == ref32 rounded to bf16, up to one bf16 ulp of the reference."""
    a, r = a16.float(), ref32.float()
    tol = slack * (2.0 ** -7) * r.abs() + 1e-30
    bad = (a - r).abs() > tol + 1e-6 * r.abs().max()
    assert not bool(bad.any()), '%s: %d of %d elements beyond one bf16 ulp, worst %.3e' % (
        name, int(bad.sum()), bad.numel(), float(((a - r).abs() / (r.abs() + 1e-20))[bad].max()))


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return bf(torch.randn(shape, generator=g) * scale).cuda()


@pytest.mark.parametrize('store', ['f32', 'bf16'])
@pytest.mark.parametrize('ci,co,lo,rows', [(64, 128, 28, 40), (128, 256, 14, 23), (256, 512, 7, 60), (64, 64, 5, 3)])
def test_stride2_block_entry_data_gradients_in_one_launch_bf16(H, store, ci, co, lo, rows):
    """conv_dgrad_bf16_s2_pair (the k3 s2 conv's and the 1x1 s2 downsample's data gradients as one launch: the even input
    positions contract over TWO sources) == the two launches (the second accumulating): bit for bit with float storage (the
    first source's sums are kept apart and added at the end, as the second launch adds onto the first's stored result), to a
    bf16 ulp of the scale with bf16 storage (there the first launch's stored sum is rounded once more); and against fp64 on the
    bf16-rounded operands."""
    with storage(H, store):
        dt = torch.bfloat16 if store == 'bf16' else torch.float32
        dy1, dyd = rnd((rows, lo, co), 1).to(dt), rnd((rows, lo, co), 2).to(dt)
        g = torch.Generator().manual_seed(7)
        w1, wd = torch.randn(co, ci, 3, generator=g).cuda() * 0.05, torch.randn(co, ci, 1, generator=g).cuda() * 0.05
        _, w1d = H.pack_conv3_bf16(w1)
        wdd = wd[:, :, 0].t().contiguous().bfloat16().unsqueeze(0).contiguous()      # (1, Ci, Co): the data-gradient pack of a 1x1 conv
        ref = H.conv_dgrad_bf16_s2(dy1, w1d, 2 * lo)
        H.conv_dgrad_bf16_s2(dyd, wdd, 2 * lo, out=ref, accumulate=True)
        got = H.conv_dgrad_bf16_s2_pair(dy1, w1d, dyd, wdd, 2 * lo)
        r64 = torch.nn.functional.conv_transpose1d(dy1.double().permute(0, 2, 1), bf(w1).double(), stride=2, padding=1, output_padding=1) + \
            torch.nn.functional.conv_transpose1d(dyd.double().permute(0, 2, 1), bf(wd).double(), stride=2, padding=0, output_padding=1)
        r64 = r64.permute(0, 2, 1)
        scale = float(r64.abs().max())
        if store == 'f32':
            assert torch.equal(got, ref)
            assert float((got.double() - r64).abs().max()) <= 2e-6 * scale
        else:
            assert float((got.double() - ref.double()).abs().max()) <= 2.0 ** -6 * scale
            assert float((got.double() - r64).abs().max()) <= 2.0 ** -7 * scale


@pytest.mark.parametrize('store', ['f32', 'bf16'])
@pytest.mark.parametrize('C,L,R,W', [(64, 56, 20, 4), (128, 28, 20, 3), (256, 14, 20, 64), (512, 7, 20, 5)])
def test_batchnorm_backward_with_a_two_term_upstream_gradient(H, store, C, L, R, W):
    """bn_bwd_two / bn_bwd_pair(dout2=...): the upstream gradient as dout + dout2, summed while the kernel loads them == the
    mask-form backward of the sum formed beforehand -- bit for bit with float storage (one fp32 add either way), to a bf16 ulp
    of the gradient scale with bf16 storage (the stored sum is rounded, the in-kernel one is not)."""
    with storage(H, store):
        dt = torch.bfloat16 if store == 'bf16' else torch.float32
        rows = W * R
        x, res, xd = rnd((rows, L, C), 1).to(dt), rnd((rows, L, C), 2).to(dt), rnd((rows, L, C), 6).to(dt)
        da, db = rnd((rows, L, C), 3).to(dt), rnd((rows, L, C), 4).to(dt)
        g = torch.Generator().manual_seed(5)
        gamma, beta = (torch.rand(C, generator=g) + 0.5).cuda(), (torch.randn(C, generator=g) * 0.3).cuda()
        assert H.bn_two_ok(x, R)
        out, mean, invstd, mask = H.bn_fwd(x, R, gamma, beta, relu=True, res=res, want_mask=True)
        _, md, idd = H.bn_fwd(xd, R, gamma, beta, relu=False)
        dsum = (da.float() + db.float()).to(dt)
        dy, _, _, gq, ds = H.bn_bwd(dsum, x, R, mean, invstd, gamma, beta, 2, want_g=True, defer_param_grads=True, mask=mask)
        dy2, gq2, ds2 = H.bn_bwd_two(da, db, x, R, mean, invstd, gamma, beta, mask, want_g=True)
        (p1, ps1), (p2, ps2) = H.bn_bwd_pair(dsum, [(x, mean, invstd, gamma, beta, None), (xd, md, idd, gamma, beta, None)], R, mask)
        (q1, qs1), (q2, qs2) = H.bn_bwd_pair(da, [(x, mean, invstd, gamma, beta, None), (xd, md, idd, gamma, beta, None)], R, mask,
                                             dout2=db)
        pairs = (('dy', dy, dy2), ('g', gq, gq2), ('ds', ds, ds2), ('pair dx 0', p1, q1), ('pair ds 0', ps1, qs1),
                 ('pair dx 1', p2, q2), ('pair ds 1', ps2, qs2))
        for name, a, b in pairs:
            if store == 'f32':
                assert torch.equal(a, b), name
            else:
                tol = 2.0 ** -6 * float(a.float().abs().max())
                assert float((a.float() - b.float()).abs().max()) <= tol, name
    assert not H.bn_two_ok(torch.empty(40, 512, 64, device='cuda'), 40)      # two-stage geometry: no two-term form


@pytest.mark.parametrize('store', ['f32', 'bf16'])
@pytest.mark.parametrize('C,L,R,W', [(512, 7, 20, 5), (512, 7, 20, 64), (128, 7, 20, 3), (64, 7, 8, 2), (32, 5, 20, 2)])
def test_batchnorm_with_the_heads_pool_folded_in(H, store, C, L, R, W):
    """bn_fwd_pool / bn_bwd_pool (the last block's bn2 + residual + ReLU whose map is never stored; its backward from the
    gradient of the pooled features) == bn_fwd(mask) -> head_fwd's pooling and head_bwd's broadcast -> bn_bwd(mask), bit for
    bit, in both activation storage types; head_flat_fwd / head_flat_bwd == head_fwd / head_bwd on the stored map."""
    with storage(H, store):
        dt = torch.bfloat16 if store == 'bf16' else torch.float32
        rows = W * R
        x, res = rnd((rows, L, C), 1).to(dt), rnd((rows, L, C), 2).to(dt)
        g = torch.Generator().manual_seed(3)
        gamma, beta = (torch.rand(C, generator=g) + 0.5).cuda(), (torch.randn(C, generator=g) * 0.3).cuda()
        w, bias = (torch.randn(2, R * C, generator=g) * 0.02).cuda(), torch.randn(2, generator=g).cuda()
        target = torch.zeros(W, 2).cuda()
        target[::2, 0] = 1
        target[1::2, 1] = 1
        assert H.bn_pool_ok(x, R)
        # the stored-map chain
        out, mean, invstd, mask = H.bn_fwd(x, R, gamma, beta, relu=True, res=res, want_mask=True)
        flat, part, logits, loss = H.head_fwd(out, w, bias, target, R, finish=False)
        dw, db = torch.zeros_like(w), torch.zeros(2).cuda()
        dx, _, _ = H.head_bwd(part, bias, target, flat, w, logits, loss, R, L, dw=dw, dbias=db, accumulate=True)
        dy, _, _, gq, ds = H.bn_bwd(dx, x, R, mean, invstd, gamma, beta, 2, want_g=True, defer_param_grads=True, mask=mask)
        # the pooled chain
        feat, mean2, invstd2, mask2 = H.bn_fwd_pool(x, R, gamma, beta, res=res)
        flat2, part2, logits2, loss2 = H.head_flat_fwd(feat, w, bias, target, R, finish=False)
        dw2, db2 = torch.zeros_like(w), torch.zeros(2).cuda()
        dfeat, _, _ = H.head_flat_bwd(part2, bias, target, flat2, w, logits2, loss2, R, dw=dw2, dbias=db2, accumulate=True)
        dy2, gq2, ds2 = H.bn_bwd_pool(dfeat, x, R, mean2, invstd2, gamma, beta, mask2, want_g=True)
        assert feat.dtype == torch.float32 and dfeat.dtype == torch.float32 and dy2.dtype == dt
        for name, a, b in (('mean', mean, mean2), ('invstd', invstd, invstd2), ('mask', mask, mask2), ('flat', flat, flat2),
                           ('feat', flat.view(rows, C), feat), ('part', part, part2), ('logits', logits, logits2),
                           ('loss', loss, loss2), ('dw', dw, dw2), ('dbias', db, db2), ('dy', dy, dy2), ('g', gq, gq2), ('ds', ds, ds2)):
            assert torch.equal(a, b), name
        # forward only: logits and loss complete on return
        _, _, lg3, ls3 = H.head_flat_fwd(feat, w, bias, target, R, finish=True)
        assert torch.equal(lg3, logits) and torch.equal(ls3, loss)
    assert not H.bn_pool_ok(torch.empty(40, 56, 64, device='cuda'), 20)        # a window too long for the pooled form


@pytest.mark.parametrize('C,L,R,W', [(64, 56, 20, 4), (128, 28, 20, 3), (512, 7, 20, 5), (64, 128, 40, 2), (64, 112, 20, 2)])
def test_batchnorm_kernels_bf16_storage(H, C, L, R, W):
    """bn_fwd (+ReLU, +residual, +mask) and bn_bwd (all mask modes) -- single-pass and two-stage geometries."""
    rows = R * W
    x, res, dout = rnd((rows, L, C), 1, 2.0), rnd((rows, L, C), 2), rnd((rows, L, C), 3)
    gamma = (torch.rand(C, generator=torch.Generator().manual_seed(4)) + 0.5).cuda()
    beta = (torch.randn(C, generator=torch.Generator().manual_seed(5)) * 0.3).cuda()
    for relu, use_res in ((True, False), (False, False), (True, True)):
        o32, m32, i32 = H.bn_fwd(x, R, gamma, beta, relu=relu, res=res if use_res else None)
        with storage(H, 'bf16'):
            o16, m16, i16 = H.bn_fwd(x.bfloat16(), R, gamma, beta, relu=relu, res=res.bfloat16() if use_res else None)
        assert o16.dtype == torch.bfloat16 and m16.dtype == torch.float32
        assert torch.allclose(m16, m32, rtol=1e-6, atol=1e-7) and torch.allclose(i16, i32, rtol=1e-6)
        one_ulp(o16, o32, 'bn_fwd relu=%s res=%s' % (relu, use_res))
    # backward, mask recomputed (mode 1) / no relu (mode 0) / from the output (mode 2) / from the bit mask
    o32, m32, i32, mask32 = H.bn_fwd(x, R, gamma, beta, relu=True, res=res, want_mask=True)
    with storage(H, 'bf16'):
        o16, m16, i16, mask16 = H.bn_fwd(x.bfloat16(), R, gamma, beta, relu=True, res=res.bfloat16(), want_mask=True)
    for mode in (0, 1, 2):
        kw = dict(out=o32) if mode == 2 else {}
        dx32, dg32, db32, g32, ds32 = H.bn_bwd(dout, x, R, m32, i32, gamma, beta, mode, want_g=True, **kw)
        with storage(H, 'bf16'):
            kw16 = dict(out=o16) if mode == 2 else {}
            dx16, dg16, db16, g16, ds16 = H.bn_bwd(dout.bfloat16(), x.bfloat16(), R, m16, i16, gamma, beta, mode,
                                                   want_g=True, **kw16)
        if mode != 2:                       # mode 2's mask comes from the ROUNDED output: identical unless out == 0 exactly
            assert torch.allclose(ds16, ds32, rtol=2e-5, atol=1e-4), 'sums differ, mode %d' % mode
            one_ulp(dx16, dx32, 'bn_bwd dx mode %d' % mode, slack=1.5)
            one_ulp(g16, g32, 'bn_bwd g mode %d' % mode)
            assert torch.allclose(dg16, dg32, rtol=2e-5, atol=1e-3) and torch.allclose(db16, db32, rtol=2e-5, atol=1e-3)
        else:
            assert float((dx16.float() - dx32).norm() / dx32.norm()) < 1e-2
    if mask32 is not None:
        dx32, _, _, g32, _ = H.bn_bwd(dout, x, R, m32, i32, gamma, beta, 2, want_g=True, mask=mask32)
        with storage(H, 'bf16'):
            dx16, _, _, g16, _ = H.bn_bwd(dout.bfloat16(), x.bfloat16(), R, m16, i16, gamma, beta, 2, want_g=True, mask=mask16)
        one_ulp(dx16, dx32, 'bn_bwd dx bit mask', slack=1.5)
        one_ulp(g16, g32, 'bn_bwd g bit mask')


@pytest.mark.parametrize('rows,lin,R,pool', [(40, 224, 20, 0), (40, 224, 20, 1), (80, 512, 40, 0)])
def test_stem_and_pool_kernels_bf16_storage(H, rows, lin, R, pool):
    g = torch.Generator().manual_seed(rows + lin)
    x2d = torch.randn(rows, lin, generator=g).cuda()                       # the network input stays float32
    w = (torch.randn(64, 1, 7, generator=g) * 0.3).cuda()
    gamma, beta = (torch.rand(64, generator=g) + 0.5).cuda(), (torch.randn(64, generator=g) * 0.3).cuda()
    y32 = H.stem_conv_fwd(x2d, w)
    with storage(H, 'bf16'):
        y16 = H.stem_conv_fwd(x2d, w)
    assert y16.dtype == torch.bfloat16
    one_ulp(y16, y32, 'stem conv')
    yb = y16.float()                                                        # continue both paths from the SAME stored tensor
    m32, i32 = H.bn_stats(yb, R)
    p32 = H.bn_relu_pool_fwd(yb, R, m32, i32, gamma, beta, pool)
    dout = rnd(tuple(p32.shape), 7)
    dz32 = H.pool_bwd(dout, yb, R, m32, i32, gamma, beta, pool)
    dy32, _, _, _, _ = H.bn_bwd(dz32.bfloat16().float(), yb, R, m32, i32, gamma, beta, 1)
    dw32 = H.stem_conv_wgrad(dy32.bfloat16().float(), x2d)
    with storage(H, 'bf16'):
        m16, i16 = H.bn_stats(y16, R)
        p16 = H.bn_relu_pool_fwd(y16, R, m16, i16, gamma, beta, pool)
        dz16 = H.pool_bwd(dout.bfloat16(), y16, R, m16, i16, gamma, beta, pool)
        dy16, _, _, _, _ = H.bn_bwd(dz16, y16, R, m16, i16, gamma, beta, 1)
        dw16 = H.stem_conv_wgrad(dy16, x2d)
    assert torch.allclose(m16, m32, rtol=1e-6, atol=1e-7) and torch.allclose(i16, i32, rtol=1e-6)
    one_ulp(p16, p32, 'bn_relu_pool')
    one_ulp(dz16, dz32, 'pool_bwd')
    one_ulp(dy16, dy32, 'stem bn_bwd', slack=2.0)
    assert float((dw16 - dw32).norm() / dw32.norm()) < 2e-2 and dw16.dtype == torch.float32


@pytest.mark.parametrize('rows,lin,R,pool', [(40, 224, 20, 0), (12, 64, 4, 1)])
def test_recomputing_stem_bf16_storage(H, rows, lin, R, pool):
    """The recomputing stem under bf16 storage: nothing at the stem's resolution is stored, so the pooled map is EXACTLY the
    float-storage one rounded once (same statistics, bit for bit), and the backward from a bf16 dout equals the float-storage
    backward from the same (bf16-representable) values bit for bit."""
    g = torch.Generator().manual_seed(rows * 3 + lin)
    x2d = torch.randn(rows, lin, generator=g).cuda()
    w = (torch.randn(64, 1, 7, generator=g) * 0.3).cuda()
    gamma, beta = (torch.rand(64, generator=g) + 0.5).cuda(), (torch.randn(64, generator=g) * 0.3).cuda()
    assert H.stem_fused_ok(x2d, w, R)
    p32, m32, i32 = H.stem_fused_fwd(x2d, w, R, gamma, beta, pool)
    dout = rnd(tuple(p32.shape), 5).bfloat16()
    dw32, ds32 = H.stem_fused_bwd(dout.float(), x2d, w, R, m32, i32, gamma, beta, pool)
    with storage(H, 'bf16'):
        assert H.stem_fused_ok(x2d, w, R)
        p16, m16, i16 = H.stem_fused_fwd(x2d, w, R, gamma, beta, pool)
        dw16, ds16 = H.stem_fused_bwd(dout, x2d, w, R, m16, i16, gamma, beta, pool)
    assert p16.dtype == torch.bfloat16 and torch.equal(m16, m32) and torch.equal(i16, i32)
    assert torch.equal(p16, p32.bfloat16())
    assert torch.equal(dw16, dw32) and torch.equal(ds16, ds32)


@pytest.mark.parametrize('st', ['f32', 'bf16'])
@pytest.mark.parametrize('C,L,R,W', [(64, 56, 20, 3), (128, 28, 20, 2), (512, 7, 20, 5), (256, 14, 20, 4)])
def test_conv3_bf16_with_batchnorm_folded_in(H, C, L, R, W, st):
    """H.conv3_bf16_bn (resnet.py:27-33 conv1 -> bn1 -> relu -> conv2 with no pass for bn1): (a) the conv output is
    conv3_bf16's, bit for bit, and the statistics the records merge to are the per-window statistics of that STORED tensor
    (np_ref.bn_window_fwd, fp64) to 2e-6 / 2e-5; (b) with the records as input, the published (mean, invstd) are those, and the
    result is conv3_bf16 of relu(norm(y1)) computed by the same fused multiply-add (H.bn_relu_ss form) and rounded to bf16 --
    up to the bf16 roundings that an fp32 last-bit difference in scale / shift moves (checked: <= 1e-2 of the scale, and
    against the fp64 composition); (c) bn_bwd_ss(hout=) rebuilds exactly what conv2 staged, in the storage type."""
    rows = R * W
    g = torch.Generator().manual_seed(C + L)
    x = bf(torch.randn(rows, L, C, generator=g)).cuda()
    w1 = (torch.randn(C, C, 3, generator=g) * (2.0 / (3 * C)) ** 0.5).cuda()
    w2 = (torch.randn(C, C, 3, generator=g) * (2.0 / (3 * C)) ** 0.5).cuda()
    gamma, beta = (torch.rand(C, generator=g) + 0.5).cuda(), (torch.randn(C, generator=g) * 0.3).cuda()
    p1, p2 = H.pack_conv3_bf16(w1)[0], H.pack_conv3_bf16(w2)[0]
    with storage(H, st):
        xs = x.bfloat16() if st == 'bf16' else x
        y_plain = H.conv3_bf16(xs, p1)
        y1, rec = H.conv3_bf16_bn(xs, p1, R, want_records=True)
        assert torch.equal(y1, y_plain)
        mean = torch.full((W, C), float('nan'), device='cuda')
        invstd = torch.full((W, C), float('nan'), device='cuda')
        y2, rec2 = H.conv3_bf16_bn(y1, p2, R, rec=rec, mean=mean, invstd=invstd, gamma=gamma, beta=beta, want_records=True)
        y2b = H.conv3_bf16_bn(y1, p2, R, rec=rec, mean=mean.clone(), invstd=invstd.clone(), gamma=gamma, beta=beta)
        assert torch.equal(y2, y2b)
        # (c) the backward kernel's rebuilt activation
        dout = rnd((rows, L, C), 9)
        dout = dout.bfloat16() if st == 'bf16' else dout
        h = torch.empty_like(y1)
        dx = torch.empty_like(y1)
        ds = H.bn_bwd_ss(dout, y1, R, mean, invstd, gamma, beta, 1, dx, hout=h)
    y1f = y1.float().cpu().numpy().astype(np.float64).transpose(0, 2, 1)
    _, stref = np_ref.bn_window_fwd(y1f, gamma.cpu().numpy().astype(np.float64), beta.cpu().numpy().astype(np.float64), R)
    mref, iref = stref
    assert np.abs(mean.cpu().numpy() - mref.reshape(W, C)).max() < 2e-6 * (1 + np.abs(mref).max())
    assert np.abs(invstd.cpu().numpy() / iref.reshape(W, C) - 1).max() < 2e-5
    # the staged activation, by the same arithmetic on the host (fp32 fma == a double multiply-add rounded once)
    sc = (gamma * invstd)
    sh = torch.from_numpy(np.float32(beta.cpu().numpy().astype(np.float64) - mean.cpu().numpy().astype(np.float64) * sc.cpu().numpy().astype(np.float64))).cuda()
    yv = y1.float().view(W, R * L, C)
    href = torch.clamp((yv.double() * sc.double()[:, None, :] + sh.double()[:, None, :]).float(), min=0).view(rows, L, C)
    hb = href.bfloat16()
    assert float((h.float() - (hb.float() if st == 'bf16' else href)).abs().max()) <= 1e-2 * float(href.abs().max())
    with storage(H, st):
        y2_ref = H.conv3_bf16(hb if st == 'bf16' else hb.float(), p2)
    err = float((y2.float() - y2_ref.float()).abs().max())
    assert err <= 1e-2 * float(y2_ref.float().abs().max()), err
    # dx / ds against the fp64 BatchNorm backward on the same stored tensors
    dref, dgr, dbr = np_ref.bn_window_bwd(y1f, gamma.cpu().numpy().astype(np.float64), stref,
                                          (dout.float() * (h.float() > 0)).cpu().numpy().astype(np.float64).transpose(0, 2, 1), R)
    tol = 2e-2 if st == 'bf16' else 2e-5
    assert np.abs(dx.float().cpu().numpy().transpose(0, 2, 1) - dref).max() <= tol * (1 + np.abs(dref).max())
    # records of the second conv: the statistics of its stored output
    y2f = y2.float().cpu().numpy().astype(np.float64).transpose(0, 2, 1)
    _, st2 = np_ref.bn_window_fwd(y2f, np.ones(C), np.zeros(C), R)
    m2 = torch.empty((W, C), device='cuda'); i2 = torch.empty((W, C), device='cuda')
    with storage(H, st):
        H.conv3_bf16_bn(y2, p1, R, rec=rec2, mean=m2, invstd=i2, gamma=gamma, beta=beta)
    m2r = st2[0]
    assert np.abs(m2.cpu().numpy() - m2r.reshape(W, C)).max() < 2e-6 * (1 + np.abs(m2r).max())


@pytest.mark.parametrize('ci,co,L,rows', [(64, 64, 56, 40), (128, 128, 28, 23), (512, 512, 7, 40), (64, 64, 128, 9)])
def test_conv_kernels_bf16_storage(H, ci, co, L, rows):
    """k3 s1 conv forward / data gradient (+accumulate), the stride-2 pair, and all three weight-gradient forms with bf16
    activations in and out: equal to the float-storage kernels on the same (bf16-representable) inputs, outputs rounded."""
    g = torch.Generator().manual_seed(ci + L)
    x, dy = rnd((rows, L, ci), 11), rnd((rows, L, co), 12)
    w = (torch.randn(co, ci, 3, generator=g) * np.sqrt(2.0 / (3 * co))).cuda()
    wf, wd = H.pack_conv3_bf16(w)
    y32 = H.conv3_bf16(x, wf)
    dx32 = H.conv3_bf16(dy, wd)
    base = rnd((rows, L, ci), 13)
    acc32 = H.conv3_bf16(dy, wd, out=base.clone(), accumulate=True)
    with storage(H, 'bf16'):
        y16 = H.conv3_bf16(x.bfloat16(), wf)
        dx16 = H.conv3_bf16(dy.bfloat16(), wd)
        acc16 = H.conv3_bf16(dy.bfloat16(), wd, out=base.bfloat16(), accumulate=True)
    assert y16.dtype == torch.bfloat16
    one_ulp(y16, y32, 'conv3 fwd')
    one_ulp(dx16, dx32, 'conv3 dgrad')
    one_ulp(acc16, acc32, 'conv3 dgrad accumulate')
    # weight gradients: float slabs either way
    jobs32 = [(dy, x, 3, 1, 1)]
    H.WGRAD_BF16 = True
    try:
        (slab32,) = H.conv_wgrad_multi(jobs32)
        dw32 = torch.zeros(co, ci, 3, device='cuda')
        H.wgrad_reduce_multi([(slab32, dw32)], accumulate=False)
        with storage(H, 'bf16'):
            (slab16,) = H.conv_wgrad_multi([(dy.bfloat16(), x.bfloat16(), 3, 1, 1)])
            dw16 = torch.zeros(co, ci, 3, device='cuda')
            H.wgrad_reduce_multi([(slab16, dw16)], accumulate=False)
    finally:
        H.WGRAD_BF16 = False
    assert torch.allclose(dw16, dw32, rtol=1e-5, atol=1e-4 * float(dw32.abs().max()))
    if L % 2 == 0 and co == 2 * ci or (ci, co) == (64, 64):
        # stride-2 block head (k3 s2 p1) + 1x1 downsample sharing one launch, and their data / weight gradients
        co2 = 2 * ci
        w1 = (torch.randn(co2, ci, 3, generator=g) * 0.05).cuda()
        wdn = (torch.randn(co2, ci, 1, generator=g) * 0.05).cuda()
        (_, _, f1, d1), (_, _, fd, dd) = H.repack_multi([w1, wdn], [16, 16])
        dy2 = rnd((rows, L // 2, co2), 14)
        a32, b32 = H.conv_fwd_bf16_s2(x, f1, fd)
        g32 = H.conv_dgrad_bf16_s2(dy2, d1, L)
        H.conv_dgrad_bf16_s2(dy2, dd, L, out=g32, accumulate=True)
        H.WGRAD_BF16 = True
        try:
            s32 = H.conv_wgrad_multi([(dy2, x, 3, 2, 1), (dy2, x, 1, 2, 0)])
            with storage(H, 'bf16'):
                a16, b16 = H.conv_fwd_bf16_s2(x.bfloat16(), f1, fd)
                g16 = H.conv_dgrad_bf16_s2(dy2.bfloat16(), d1, L)
                g16_first = g16.clone()
                H.conv_dgrad_bf16_s2(dy2.bfloat16(), dd, L, out=g16, accumulate=True)
                s16 = H.conv_wgrad_multi([(dy2.bfloat16(), x.bfloat16(), 3, 2, 1), (dy2.bfloat16(), x.bfloat16(), 1, 2, 0)])
        finally:
            H.WGRAD_BF16 = False
        one_ulp(a16, a32, 'stride-2 conv fwd')
        one_ulp(b16, b32, 'downsample fwd')
        # the accumulate form rounds twice under bf16 storage (the first launch stores bf16, the second adds to it): the
        # error is one ulp of the FIRST term plus one of the sum -- judged against both (the sum may cancel)
        assert g16_first.dtype == torch.bfloat16
        err = (g16.float() - g32).abs()
        tol = 1.5 * 2.0 ** -7 * (g16_first.float().abs() + g32.abs()) + 1e-6 * g32.abs().max()
        assert not bool((err > tol).any()), 'stride-2 dgrad pair: %d elements beyond two roundings' % int((err > tol).sum())
        for (sl16, *_), (sl32, *_) in zip(s16, s32):
            assert torch.allclose(sl16, sl32, rtol=1e-5, atol=1e-4 * float(sl32.abs().max()) + 1e-6)


def test_feature_boundary_and_refusals_bf16_storage(H):
    x = rnd((40, 7, 512), 21)
    f32 = H.global_avgpool_fwd(x)
    d = torch.randn(40, 512, generator=torch.Generator().manual_seed(3)).cuda()
    dx32 = H.global_avgpool_bwd(d, 7)
    xl = rnd((40, 16, 512), 22)
    s32 = H.avgpool_slide_fwd(xl, 7)
    ds = torch.randn(tuple(s32.shape), generator=torch.Generator().manual_seed(4)).cuda()
    dxl32 = H.avgpool_slide_bwd(ds, 16, 7, 512)
    with storage(H, 'bf16'):
        f16 = H.global_avgpool_fwd(x.bfloat16())
        dx16 = H.global_avgpool_bwd(d, 7)
        s16 = H.avgpool_slide_fwd(xl.bfloat16(), 7)
        dxl16 = H.avgpool_slide_bwd(ds, 16, 7, 512)
        assert f16.dtype == torch.float32 and torch.allclose(f16, f32, rtol=1e-6, atol=1e-6)     # features stay float
        assert torch.allclose(s16, s32, rtol=1e-6, atol=1e-6)
        one_ulp(dx16, dx32, 'global pool bwd')
        one_ulp(dxl16, dxl32, 'sliding pool bwd')
        # the float-activation kernels refuse to run on bf16 storage instead of misreading it
        u = H.wino_weights(torch.randn(64, 64, 3).cuda())
        with pytest.raises(H.HipError):
            H.conv3_winograd(rnd((20, 56, 64), 5).bfloat16(), u)
        with pytest.raises(H.HipError):
            H.concat2(rnd((20, 56, 64), 5).bfloat16(), rnd((20, 56, 32), 6).bfloat16())
        with pytest.raises(ValueError):
            H.bn_fwd(rnd((20, 56, 64), 5), 20, torch.ones(64).cuda(), torch.zeros(64).cuda())   # float tensor, bf16 mode
    assert H.act_dtype() == 'f32'


@pytest.mark.parametrize('bn1_fused', [False, True])
def test_resnet18_bf16_storage_vs_rounding_oracle_and_training(H, bn1_fused, monkeypatch):
    """(bn1_fused: the opt-in form that folds bn1 of the stride-1 blocks into conv1's epilogue / conv2's loader,
    functional._BN1_FUSED -- same rounding model: y1 and h1 are rounded where the unfused form stores them.)
    cnn_linear + resnet18 with bf16 convs AND bf16 storage against the oracle with the same rounding model.  bf16 keeps
    8 significant bits and every stored tensor is rounded: an element near a rounding boundary lands on either side
    depending on the last bits of an fp32 sum, so agreement is statistical, not elementwise -- bounds (builder-stated,
    parity unpinned): logits within 3e-2 of the same-rounding oracle and 5e-2 of the exact one, loss within 2e-2, every
    parameter gradient rel-l2 < 0.6 (measured in the log); 12 SGD steps bring the loss down; DenseNet is refused."""
    import deepards_amd.models as M
    from deepards_amd import functional as F_
    from deepards_amd.functional import bce_with_logits
    from deepards_amd.train import HotPathTrainer
    monkeypatch.setattr(F_, '_BN1_FUSED', bn1_fused)
    x, t = seeded_batch(3, 20, 11)
    xt, tt = torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda()
    params = {k: v.astype(np.float64) for k, v in seeded_params('resnet18', 6).items()}
    exact = np_ref.cnn_linear_forward_backward(params, x.astype(np.float64), t.astype(np.float64))
    ref = np_ref.cnn_linear_forward_backward(params, x.astype(np.float64), t.astype(np.float64), bf16_convs=True,
                                             bf16_storage=True)

    def build():
        model = M.CNNLinearNetwork(M.resnet18(), 20, 0)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_params('resnet18', 6).items()}, strict=False)
        return model.cuda().train()
    F_.set_conv_dtype('bf16')
    try:
        F_.set_storage_dtype('bf16')
        assert F_.storage_dtype() == 'bf16'
        model = build()
        out = model(xt, None)
        assert out.dtype == torch.float32
        loss = bce_with_logits(out, tt)
        loss.backward()
        logits = out.detach().cpu().numpy()
        e_same, e_exact = np.abs(logits - ref['logits']).max(), np.abs(logits - exact['logits']).max()
        worst, worst_ratio = 0.0, 0.0
        for n, p in model.named_parameters():
            if n in ref['grads']:
                r = float(np.linalg.norm(p.grad.cpu().numpy() - ref['grads'][n]) / (np.linalg.norm(ref['grads'][n]) + 1e-30))
                # the arithmetic's own noise floor on these inputs: the same-rounding oracle against the exact one
                floor = float(np.linalg.norm(ref['grads'][n] - exact['grads'][n]) / (np.linalg.norm(exact['grads'][n]) + 1e-30))
                worst, worst_ratio = max(worst, r), max(worst_ratio, r / max(floor, 1e-3))
                assert r < 1.25 * floor + 1e-2, (n, r, floor)
        log('resnet18 bf16 storage: logits vs same-rounding oracle %.3e, vs exact %.3e; loss %.5f vs %.5f; worst gradient '
            'rel-l2 vs same-rounding oracle %.3e (worst ratio to the rounding floor %.2f)' %
            (e_same, e_exact, float(loss), ref['loss'], worst, worst_ratio))
        assert e_same < 3e-2 and e_exact < 5e-2 and abs(float(loss) - ref['loss']) < 2e-2 and worst < 0.6
        tr = HotPathTrainer(build(), use_graph=True)
        losses = [float(tr.train_step(xt, tt)) for _ in range(12)]
        assert all(np.isfinite(losses)) and losses[-1] < losses[0]
        loss_t, logits_t, pred = tr.test_step(xt, tt)
        assert np.isfinite(float(loss_t)) and pred.shape == (3,)
        dn = M.CNNLinearNetwork(M.densenet18(drop_rate=0.0), 20, 0).cuda().train()
        with pytest.raises((NotImplementedError, H.HipError)):
            dn(xt, None)                                    # no bf16-storage DenseNet (96-channel convs, concat kernels)
    finally:
        F_.set_conv_dtype('f32')
    assert F_.storage_dtype() == 'f32' and F_.conv_dtype() == 'f32'
    with torch.no_grad():                                   # the fp32 path is untouched by the excursion
        assert np.abs(build()(xt, None).cpu().numpy() - exact['logits']).max() < 1e-4


def _c5_reference(p64, x64, t64, nb, **flags):
    """The stated C5 model (deepards_amd.models.BreathBlockLinear) in the oracle: breath block on (B*NB, 1, L) rows with
    per-window BatchNorm, features flattened per window, Linear(F*NB, 2), BCE (mean)."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'tools'))
    from decision_match import feature_reference
    b = x64.shape[0]
    w, bias = p64['linear_final.weight'], p64['linear_final.bias']

    def head(feat):
        flat = feat.reshape(b, -1)
        logits = np_ref.linear_fwd(flat, w, bias)
        loss, dl = np_ref.bce_with_logits(logits, t64)
        return (dl @ w).reshape(feat.shape), dict(logits=logits, loss=loss,
                                                  grads={'linear_final.weight': dl.T @ flat, 'linear_final.bias': dl.sum(axis=0)})
    return feature_reference(p64, nb, x64.reshape(b * nb, 1, -1), head, 'resnet18', **flags)


def test_c5_tile_shape_at_its_benchmarked_arithmetic(H):
    """BASELINE configs[4] as bench.py --nb 40 --seq-len 512 --dtype bf16 times it: resnet18 breath block on (40, 1, 512)
    windows + the stated Linear(F*NB, 2) head (``BreathBlockLinear``), bf16 MFMA convs AND bf16 activation storage -- the
    two-stage BatchNorm of the long windows (Wn = 40 * 128 = 5 120 > 1 280), the sliding AvgPool1d(7, 1) boundary and the
    bf16 stride-2 heads at L = 512 are all live.  Against the oracle with the same rounding model
    (np_ref bf16_convs + bf16_storage): features, logits, loss, every weight gradient; bounds as in
    test_resnet18_bf16_storage_vs_rounding_oracle_and_training (statistical: 8 significant bits, ~40 roundings deep) plus
    one that is not builder-stated: this path must sit no further from the same-rounding oracle than that oracle sits
    from the exact one (features: 3/4 of it) -- the arithmetic's own noise floor measured on the same inputs.  Parity unpinned by
    construction: the reference has no bf16 path and cannot run this shape."""
    import deepards_amd.models as M
    from deepards_amd import functional as F_
    from deepards_amd.functional import bce_with_logits
    nb, L, B = 40, 512, 2
    p32 = seeded_params('resnet18', 4, n_sub_batches=nb)
    rng = np.random.RandomState(31)
    head_w = (rng.uniform(-1, 1, (2, 5120 * nb)) / np.sqrt(5120 * nb)).astype(np.float32)
    head_b = rng.uniform(-0.01, 0.01, 2).astype(np.float32)
    p32 = dict(p32)
    p32['linear_final.weight'], p32['linear_final.bias'] = head_w, head_b
    x = rng.randn(B, nb, 1, L).astype(np.float32)
    t = np.zeros((B, 2), np.float32)
    t[0, 1] = t[1, 0] = 1
    p64 = {k: v.astype(np.float64) for k, v in p32.items()}
    # (which stem the device takes for this shape decides what the oracle rounds: the recomputing one stores no stem-resolution map)
    recomputed = bool(F_._STEM_FUSED and H.stem_fused_ok(torch.from_numpy(x.reshape(B * nb, L)).cuda(),
                                                         torch.from_numpy(p32['breath_block.conv1.weight']).cuda(), nb))
    ref = _c5_reference(p64, x.astype(np.float64), t.astype(np.float64), nb, bf16_convs=True, bf16_storage=True,
                        stem_recomputed=recomputed)
    exact = _c5_reference(p64, x.astype(np.float64), t.astype(np.float64), nb)
    F_.set_conv_dtype('bf16')
    try:
        F_.set_storage_dtype('bf16')
        model = M.BreathBlockLinear(M.resnet18(), nb, L)
        missing = model.load_state_dict({k: torch.from_numpy(v) for k, v in p32.items()}, strict=False)
        assert not missing.unexpected_keys
        model = model.cuda().train()
        xt, tt = torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda()
        feat = model.breath_block.forward_windows(xt.reshape(B * nb, 1, L), nb)
        assert feat.dtype == torch.float32 and tuple(feat.shape) == (B * nb, 5120)
        got_f = feat.detach().cpu().numpy()
        f_same, f_floor = rel_l2(got_f, ref['feat']), rel_l2(ref['feat'], exact['feat'])
        out = model(xt, None)
        loss = bce_with_logits(out, tt)
        loss.backward()
        logits = out.detach().cpu().numpy()
        e_same, e_exact = np.abs(logits - ref['logits']).max(), np.abs(logits - exact['logits']).max()
        log('C5 bf16 storage (nb 40, L 512): features rel-l2 vs same-rounding oracle %.3e (oracle vs exact: %.3e); logits '
            '%.3e / %.3e vs exact; loss %.5f vs %.5f' % (f_same, f_floor, e_same, e_exact, float(loss), ref['loss']))
        assert f_same < 2.5e-2 and f_same < 0.75 * f_floor          # measured 9.1e-3 against a floor of 1.9e-2
        assert e_same < 3e-2 and e_exact < 5e-2 and abs(float(loss) - ref['loss']) < 2e-2
        worst, worst_ratio = 0.0, 0.0
        for n, p in model.named_parameters():
            if n in ref['grads']:
                g = p.grad.cpu().numpy()
                r = rel_l2(g, ref['grads'][n])
                floor = rel_l2(ref['grads'][n], exact['grads'][n])
                worst, worst_ratio = max(worst, r), max(worst_ratio, r / max(floor, 1e-3))
                log('   grad %-44s rel-l2 vs same-rounding oracle %.3e, oracle vs exact %.3e' % (n, r, floor))
                assert r < 0.6 and r < 1.0 * floor + 1e-2, (n, r, floor)      # measured: worst ratio to the floor 0.73
        log('   worst gradient rel-l2 %.3e, worst ratio to the rounding floor %.2f' % (worst, worst_ratio))
    finally:
        F_.set_conv_dtype('f32')
    assert F_.storage_dtype() == 'f32'


def rel_l2(a, b):
    nb_ = float(np.linalg.norm(b))
    return float(np.linalg.norm(np.asarray(a, dtype=np.float64) - b) / (nb_ if nb_ > 1e-9 else 1.0))


def test_bf16_storage_training_trajectory_tracks_fp32(H):
    """Training quality of BASELINE config C3's arithmetic (bf16 MFMA + bf16 storage), measured instead of asserted from
    12 steps on 3 windows: 200 SGD-Nesterov steps (the reference's defaults: lr 1e-3, momentum .9, wd 1e-4, clamp .01) on
    the reference's 20 fixture windows (normalised like __getitem__), same initialisation, fp32 path vs bf16 path.
    Logged every 10 steps; bounds: both reduce the loss by at least a third, the bf16 loss stays within 6 % (relative;
    measured: at most 3.9 %, at step 40) of the fp32 loss at every logged step, and the final training predictions of the two agree on >= 18 of 20 windows."""
    import deepards_amd.models as M
    from deepards_amd import functional as F_
    from deepards_amd.train import HotPathTrainer
    z = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'test_dataset_windows.npz'))
    x = ((z['x'] - float(z['mu'])) / float(z['std'])).astype(np.float32)
    t = z['target'].astype(np.float32)
    xt, tt = torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda()

    def run(bf16):
        F_.set_conv_dtype('bf16' if bf16 else 'f32')
        try:
            if bf16:
                F_.set_storage_dtype('bf16')
            model = M.CNNLinearNetwork(M.resnet18(), 20, 0)
            model.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_params('resnet18', 6).items()}, strict=False)
            tr = HotPathTrainer(model.cuda().train(), use_graph=True)
            losses = [float(tr.train_step(xt, tt)) for _ in range(200)]
            _, logits, pred = tr.test_step(xt, tt)
            tr.release_graphs()
            return np.array(losses), pred.cpu().numpy()
        finally:
            F_.set_conv_dtype('f32')
    l32, p32 = run(False)
    l16, p16 = run(True)
    for i in range(0, 200, 10):
        log('trajectory step %3d: fp32 loss %.5f   bf16-storage loss %.5f   (rel diff %+.3e)' %
            (i, l32[i], l16[i], (l16[i] - l32[i]) / l32[i]))
    log('trajectory final: fp32 %.5f bf16 %.5f; predictions agree on %d / 20' % (l32[-1], l16[-1], int((p32 == p16).sum())))
    assert np.all(np.isfinite(l16)) and l32[-1] < l32[0] * (2.0 / 3.0) and l16[-1] < l16[0] * (2.0 / 3.0)
    idx = np.arange(0, 200, 10)
    assert np.all(np.abs(l16[idx] - l32[idx]) <= 0.06 * l32[idx] + 1e-4)
    assert int((p32 == p16).sum()) >= 18
