"""Bit-exact conv family: every conv kernel on small-integer operands must EQUAL the float64 convolution.

The kernels accumulate in fp32, and on the operands of tests/tools/exact_conv.py every intermediate they can form is an
integer or a half that fp32 holds exactly (each case proves that first, with bit_budget; tests/test_exact_conv_cpu.py proves
the claim itself in numpy float32).  So there is no tolerance here: a dropped, doubled or misplaced term, a wrong edge mask,
a half tile that meets its partner wrongly changes an integer and fails array_equal.  The one toleranced case is the
F(4,3) weight gradient, whose combination with sixths rounds; its bound is derived from the roundings counted in the
kernel's code (exact_conv.wino4_wgrad_bound), not measured.

Shapes are the smallest that reach each path: L in {1, 2, 3, 5, 6, 7, 9, 57}; less than one tile, a ragged last tile, and
for the kernels with a half-tile last round one launch of more than 256 tiles whose last round is partly filled."""
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

import exact_conv as E  # noqa: E402


@pytest.fixture(scope='module')
def H():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from deepards_amd import hip_ops
    return hip_ops


def rlc(a):
    """numpy (rows, C, L) -> cuda (rows, L, C) float32"""
    return torch.from_numpy(np.ascontiguousarray(a.transpose(0, 2, 1)).astype(np.float32)).cuda()


def ncl(t):
    return t.detach().float().cpu().numpy().astype(np.float64).transpose(0, 2, 1)


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.float32)).cuda()


def host(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def eq(got, ref, name):
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, '%s: shape %s, expected %s' % (name, got.shape, ref.shape)
    if not np.array_equal(got, ref):
        bad = np.argwhere(got != ref)
        raise AssertionError('%s: %d of %d elements differ, largest difference %.6g, first at %s: got %r, expected %r' % (
            name, len(bad), ref.size, np.nanmax(np.abs(got - ref)), tuple(bad[0]), got[tuple(bad[0])], ref[tuple(bad[0])]))


def out_len(l, k, stride, pad):
    return (l + 2 * pad - k) // stride + 1


def int_base(seed, shape, amp=9):
    return np.random.default_rng([seed, 99]).integers(-amp, amp + 1, shape).astype(np.float64)


def reduce_slabs(H, slabs, shapes, accumulate=False, bases=None):
    dws = [torch.full(s, 7.0, device='cuda') if b is None else cu(b) for s, b in zip(shapes, bases or [None] * len(shapes))]
    H.wgrad_reduce_multi(list(zip(slabs, dws)), accumulate=accumulate)
    return dws


# (ci, co, L, rows): one tile and less, ragged last tiles, channel counts on every tile shape; the last one has more than
# 256 64x64 tiles with a partly filled last round in the forward and in both gradients of every (k, stride, pad)
DIRECT_SHAPES = [(32, 32, 1, 3), (32, 64, 2, 5), (96, 32, 3, 7), (64, 96, 5, 9), (128, 64, 6, 4), (64, 128, 7, 33),
                 (32, 32, 9, 2), (64, 64, 57, 40), (128, 128, 57, 300)]
KSP = [(3, 1, 1), (3, 2, 1), (1, 2, 0), (1, 1, 0)]


# ---------------------------------------------------------------------------------------------------------------------------
# direct fp32 kernels (conv_gemm.hip)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ci,co,L,rows', DIRECT_SHAPES)
@pytest.mark.parametrize('k,stride,pad', KSP)
def test_direct_forward_and_data_gradient(H, k, stride, pad, ci, co, L, rows):
    x, w = E.operand(1, rows, ci, L), E.weight(2, co, ci, k)
    lo = out_len(L, k, stride, pad)
    dy = E.operand(3, rows, co, lo)
    base = int_base(4, (rows, ci, L))
    E.bit_budget('direct', x, w, stride=stride, pad=pad)
    E.bit_budget('direct_dgrad', dy, w, base=base, stride=stride, pad=pad, k=k, l=L)
    wf, wd = H.repack_weight(cu(w), True, True)
    eq(ncl(H.conv_fwd(rlc(x), wf, stride, pad)), E.conv_fwd(x, w, stride, pad), 'forward')
    dx_ref = E.conv_dgrad(dy, w, stride, pad, L)
    eq(ncl(H.conv_dgrad(rlc(dy), wd, stride, pad, L)), dx_ref, 'data gradient')
    junk = torch.full((rows, L, ci), 7.0, device='cuda')            # the overwrite form leaves nothing of `out`
    H.conv_dgrad(rlc(dy), wd, stride, pad, L, out=junk)
    eq(ncl(junk), dx_ref, 'data gradient into a given out')
    bt = rlc(base)
    H.conv_dgrad(rlc(dy), wd, stride, pad, L, out=bt, accumulate=True)
    eq(ncl(bt), base + dx_ref, 'data gradient, accumulate')


# the direct weight-gradient kernels exist for 64- / 128-channel output tiles and (128, 32) / (32, 128): both channel counts
# multiples of 64, or one a multiple of 128 and the other of 32 (what the models have; other pairs the entry point refuses)
DIRECT_WGRAD_SHAPES = [(64, 64, 1, 3), (64, 128, 2, 5), (128, 32, 3, 7), (96, 128, 5, 9), (128, 64, 6, 4), (64, 128, 7, 33),
                       (32, 128, 9, 2), (64, 64, 57, 40), (128, 128, 57, 300)]


@pytest.mark.parametrize('ci,co,L,rows', DIRECT_WGRAD_SHAPES)
@pytest.mark.parametrize('k,stride,pad', KSP)
def test_direct_weight_gradient(H, k, stride, pad, ci, co, L, rows):
    x = E.operand(5, rows, ci, L)
    dy = E.operand(6, rows, co, out_len(L, k, stride, pad))
    base = int_base(7, (co, ci, k))
    E.bit_budget('direct_wgrad', x, dy, base=base, stride=stride, pad=pad, k=k)
    dw_ref = E.conv_wgrad(x, dy, k, stride, pad)
    xt, dyt = rlc(x), rlc(dy)
    eq(host(H.conv_wgrad(dyt, xt, k, stride, pad)), dw_ref, 'weight gradient')
    acc = cu(base)
    H.conv_wgrad(dyt, xt, k, stride, pad, out=acc, accumulate=True)
    eq(host(acc), base + dw_ref, 'weight gradient, accumulate')
    slab = H.conv_wgrad(dyt, xt, k, stride, pad, defer=True)
    for accumulate in (False, True):
        dw, = reduce_slabs(H, [slab], [(co, ci, k)], accumulate, [base])
        eq(host(dw), base * accumulate + dw_ref, 'deferred weight gradient, accumulate=%s' % accumulate)


# a stride-2 block entry: (ci, co, L, rows) with co % 64 == 0 (one launch for both forwards), ci % 64 == 0 and L even (the
# paired data gradient); the last: more than 256 tiles over the problems of the launch, partly filled last round
ENTRY_SHAPES = [(64, 64, 2, 3), (64, 128, 6, 9), (128, 64, 56, 5), (128, 128, 56, 300)]


@pytest.mark.parametrize('ci,co,L,rows', ENTRY_SHAPES)
def test_direct_block_entry_shared_launches(H, ci, co, L, rows):
    x = E.operand(8, rows, ci, L)
    w3, w1, ws = E.weight(9, co, ci, 3), E.weight(10, co, ci, 1), E.weight(11, co, ci, 3)
    E.bit_budget('direct', x, w3, stride=1, pad=1)                   # (bounds the stride-2 forms too)
    packs = [H.repack_weight(cu(w), True, True) for w in (w3, w1, ws)]
    xt = rlc(x)
    y3, y1, ys, yp = H.conv_fwd_multi([(xt, packs[0][0], 2, 1), (xt, packs[1][0], 2, 0), (xt, packs[2][0], 1, 1),
                                       (xt, packs[1][0], 1, 0)])
    eq(ncl(y3), E.conv_fwd(x, w3, 2, 1), 'multi forward: k3 s2 p1')
    eq(ncl(y1), E.conv_fwd(x, w1, 2, 0), 'multi forward: k1 s2 p0')
    eq(ncl(ys), E.conv_fwd(x, ws, 1, 1), 'multi forward: k3 s1 p1')
    eq(ncl(yp), E.conv_fwd(x, w1, 1, 0), 'multi forward: k1 s1 p0')
    dy3, dy1 = E.operand(12, rows, co, L // 2), E.operand(13, rows, co, L // 2)
    dx_ref = E.conv_dgrad(dy3, w3, 2, 1, L) + E.conv_dgrad(dy1, w1, 2, 0, L)
    E.bit_budget('direct_dgrad', dy3, w3, base=E.conv_dgrad(np.abs(dy1), np.abs(w1), 2, 0, L), stride=2, pad=1, l=L)
    eq(ncl(H.conv_dgrad_s2_pair(rlc(dy3), packs[0][1], rlc(dy1), packs[1][1], L)), dx_ref, 'paired data gradient')


@pytest.mark.parametrize('rows,lin', [(1, 2), (3, 6), (5, 30), (40, 224), (600, 6)])
@pytest.mark.parametrize('c0', [32, 64])
def test_stem_convs(H, c0, rows, lin):
    for cin, k, stride in H.STEM_SHAPES:
        x, w = E.operand(14, rows, cin, lin), E.weight(15, c0, cin, k)
        E.bit_budget('direct', x, w, stride=stride, pad=k // 2)
        y_ref = E.conv_fwd(x, w, stride, k // 2)
        assert y_ref.shape == (rows, c0, lin // stride)
        xt = cu(x)
        eq(ncl(H.stem_conv_fwd(xt, cu(w), stride=stride)), y_ref, 'stem forward %s' % ((cin, k, stride),))
        dy = E.operand(16, rows, c0, lin // stride)
        base = int_base(17, (c0, cin, k))
        E.bit_budget('direct_wgrad', x, dy, base=base, stride=stride, pad=k // 2, k=k)
        dw_ref = E.conv_wgrad(x, dy, k, stride, k // 2)
        eq(host(H.stem_conv_wgrad(rlc(dy), xt, k=k, stride=stride)), dw_ref, 'stem weight gradient %s' % ((cin, k, stride),))
        acc = cu(base)
        H.stem_conv_wgrad(rlc(dy), xt, out=acc, accumulate=True, k=k, stride=stride)
        eq(host(acc), base + dw_ref, 'stem weight gradient, accumulate %s' % ((cin, k, stride),))


# ---------------------------------------------------------------------------------------------------------------------------
# Winograd F(2,3) (conv_wino.hip)
# ---------------------------------------------------------------------------------------------------------------------------
# (ci, co, L, rows): odd and even last pairs, one pair a row; the last two: more than 256 tiles (272 / 260 forward), partly
# filled last round -> half tiles
WINO2_SHAPES = [(32, 32, 1, 7), (32, 64, 2, 33), (64, 32, 3, 5), (96, 64, 5, 9), (64, 64, 6, 3), (128, 32, 7, 40),
                (32, 96, 9, 5), (64, 64, 57, 300), (64, 128, 7, 1040)]


@pytest.mark.parametrize('ci,co,L,rows', WINO2_SHAPES)
def test_winograd_f23(H, ci, co, L, rows):
    want = H.WINO2 if H.WINOGRAD_WGRAD else H.DIRECT      # (DA_WINOGRAD=0 routes the models elsewhere; the entry point stays)
    assert H.conv_kernel(co, ci, 3, 1, 1, False, L) == want and H.conv_kernel(ci, co, 3, 1, 1, False, L) == want
    x, w = E.operand(20, rows, ci, L), E.weight(21, co, ci, 3)
    dy = E.operand(22, rows, co, L)
    base = int_base(23, (rows, ci, L))
    uf_ref, ud_ref = E.taps_from_weight(w, 4), E.taps_from_weight(w, 4, transpose=True)
    E.bit_budget('wino', x, uf_ref, scale=2.0)
    E.bit_budget('wino', dy, ud_ref, base=base)
    wt = cu(w)
    uf, ud = H.wino_weights(wt), H.wino_weights(wt, transpose=True)
    eq(host(uf), uf_ref, 'forward taps: the exact half-integers')
    eq(host(ud), ud_ref, 'data-gradient taps')
    (_, _, uf2, ud2), = H.repack_multi([wt], [True])
    assert torch.equal(uf2, uf) and torch.equal(ud2, ud)
    y_ref, dx_ref = E.conv_fwd(x, w, 1, 1), E.conv_dgrad(dy, w, 1, 1, L)
    assert np.array_equal(E.wino_fwd(x, uf_ref), y_ref) and np.array_equal(E.wino_fwd(dy, ud_ref), dx_ref)
    xt, dyt = rlc(x), rlc(dy)
    eq(ncl(H.conv3_winograd(xt, uf)), y_ref, 'F(2,3) forward')
    eq(ncl(H.conv3_winograd(dyt, ud)), dx_ref, 'F(2,3) data gradient')
    bt = rlc(base)
    H.conv3_winograd(dyt, ud, out=bt, accumulate=True)
    eq(ncl(bt), base + dx_ref, 'F(2,3) data gradient, accumulate')
    # dropout in the epilogue at p = 0.5: the kept outputs are doubled -- exact
    seed = torch.tensor([1234 + L], dtype=torch.int64, device='cuda')
    keep2 = ncl(H.dropout(torch.ones(rows, L, co, device='cuda'), seed, 5, 0.5))
    assert set(np.unique(keep2)) <= {0.0, 2.0} and (rows * L * co < 64 or 0.3 < (keep2 == 0).mean() < 0.7)
    eq(ncl(H.conv3_winograd(xt, uf, drop=(seed, 5, 0.5))), y_ref * keep2, 'F(2,3) forward with dropout')


# channel counts that are multiples of 64 (what the Winograd weight gradients take); the 300-row case: several splits
WINO2_WGRAD_SHAPES = [(64, 64, 1, 7), (64, 128, 2, 33), (128, 64, 5, 9), (64, 64, 7, 1), (192, 64, 6, 40), (64, 64, 9, 150),
                      (64, 64, 57, 300)]


@pytest.mark.parametrize('ci,co,L,rows', WINO2_WGRAD_SHAPES)
def test_winograd_f23_weight_gradient(H, ci, co, L, rows):
    """M_j over pairs, dW = M0 + (M1 + M2) / 2, (M1 - M2) / 2, (M1 + M2) / 2 + M3: halves only -- exact."""
    assert H.wgrad_kernel(co, ci, 3, 1, 1, L) == (H.WINO2 if H.WINOGRAD_WGRAD else H.DIRECT)
    x, dy = E.operand(24, rows, ci, L), E.operand(25, rows, co, L)
    base = int_base(26, (co, ci, 3))
    E.bit_budget('wino_wgrad', x, dy, base=base, points=4)
    dw_ref = E.conv_wgrad(x, dy, 3, 1, 1)
    assert np.array_equal(E.wino_wgrad(x, dy, 4), dw_ref)
    slabs = H.conv_wgrad_multi([(rlc(dy), rlc(x), 3, 1, 1)])
    for accumulate in (False, True):
        dw, = reduce_slabs(H, slabs, [(co, ci, 3)], accumulate, [base])
        eq(host(dw), base * accumulate + dw_ref, 'F(2,3) weight gradient, accumulate=%s' % accumulate)


# ---------------------------------------------------------------------------------------------------------------------------
# Winograd F(4,3)
# ---------------------------------------------------------------------------------------------------------------------------
# (c, n, L, rows): 1, 2 or 3 outputs in the last quad, one quad a row; the last: 264 tiles forward, partly filled last round
WINO4_SHAPES = [(32, 32, 1, 7), (32, 64, 2, 33), (32, 32, 3, 4), (64, 32, 5, 9), (96, 64, 6, 40), (64, 96, 7, 5),
                (128, 32, 9, 3), (32, 64, 57, 20), (32, 128, 5, 2100)]


@functools.lru_cache(maxsize=None)
def _f43_case(c, n, L, rows):
    """Operands, budget and float64 references of one shape, shared by the two K-step variants (read-only)."""
    x, u = E.operand(30, rows, c, L, amp=1), E.int_taps(31, 6, n, c)
    x2, u2 = E.operand(32, rows, n, L, amp=1), E.int_taps(33, 6, c, n)
    base = int_base(34, (rows, c, L))
    E.bit_budget('wino', x, u)
    E.bit_budget('wino', x2, u2, base=base)
    out = (x, u, x2, u2, base, E.wino_fwd(x, u), E.wino_fwd(x2, u2))
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize('ksteps', [16, 32])
@pytest.mark.parametrize('c,n,L,rows', WINO4_SHAPES)
def test_winograd_f43_on_integer_taps(H, c, n, L, rows, ksteps):
    """The F(4,3) kernel by itself: hand-made integer taps, independent per point (the tap generator's sixths are rounded),
    against the float64 bilinear form; a data gradient is the same kernel on (6, Ci, Co) taps: both channel orders run."""
    from deepards_amd import _lib
    x, u, x2, u2, base, y_ref, y2_ref = _f43_case(c, n, L, rows)
    _lib.lib().da_wino_debug_tail(3 if ksteps == 16 else 2)
    try:
        eq(ncl(H.conv3_winograd(rlc(x), cu(u))), y_ref, 'F(4,3) forward')
        eq(ncl(H.conv3_winograd(rlc(x2), cu(u2))), y2_ref, 'F(4,3) data gradient')
        bt = rlc(base)
        H.conv3_winograd(rlc(x2), cu(u2), out=bt, accumulate=True)
        eq(ncl(bt), base + y2_ref, 'F(4,3) data gradient, accumulate')
    finally:
        _lib.lib().da_wino_debug_tail(3)


def test_winograd_f43_taps_of_a_weight_of_24s(H, record_property):
    """wino_weights(points=6) on w = 24 * {-1, 0, 1}: the exact taps are integers, the generator multiplies by rounded
    1/6, 1/12, 1/24.  Whether they come out exact is RECORDED (pytest -s), not asserted; that they are within one rounding
    per operation is."""
    w = 24.0 * E.weight(35, 64, 32, 3, amp=1)
    for transpose in (False, True):
        u_ref = E.taps_from_weight(w, 6, transpose=transpose)
        assert np.array_equal(u_ref, np.round(u_ref))
        u = host(H.wino_weights(cu(w), transpose=transpose, points=6))
        off = u != u_ref
        print('F(4,3) taps of w = 24 * {-1, 0, 1} (transpose=%s): %s; %d of %d differ, largest difference %.3g, per point %s' % (
            transpose, 'EXACT' if not off.any() else 'NOT exact', off.sum(), off.size, np.abs(u - u_ref).max(),
            off.reshape(6, -1).sum(1).tolist()))
        record_property('wino4_taps_exact_transpose_%s' % transpose, bool(not off.any()))
        g = np.abs(w[:, :, ::-1].transpose(1, 0, 2) if transpose else w)
        assert np.all(np.abs(u - u_ref) <= 8 * 2.0 ** -24 * np.einsum('jt,nct->jnc', np.abs(E.G4), g))     # (a handful of roundings)


WINO4_WGRAD_SHAPES = [(64, 64, 1, 70), (64, 128, 5, 9), (128, 64, 4, 64), (64, 64, 8, 1), (64, 64, 7, 40), (64, 64, 6, 130),
                      (64, 64, 9, 300)]


@pytest.mark.parametrize('ci,co,L,rows', WINO4_WGRAD_SHAPES)
def test_winograd_f43_weight_gradient_within_its_derived_bound(H, ci, co, L, rows):
    """The one toleranced case: the six accumulators are exact integers, dW = G^T M rounds.  Componentwise bound
    (c + slabs) gamma-roundings of T, c counted from the kernel's combination code (exact_conv.WINO4_WGRAD_ROUNDINGS)."""
    x, dy = E.operand(36, rows, ci, L, amp=1), E.operand(37, rows, co, L, amp=1)
    base = int_base(38, (co, ci, 3))
    E.bit_budget('wino_wgrad', x, dy, points=6)
    dw_ref = E.wino_wgrad(x, dy, 6)
    assert np.abs(dw_ref - E.conv_wgrad(x, dy, 3, 1, 1)).max() <= 1e-9
    dw_ref = E.conv_wgrad(x, dy, 3, 1, 1)
    old = H.WINO4_WGRAD_MIN_C
    H.WINO4_WGRAD_MIN_C = 64
    try:
        assert H.wgrad_kernel(co, ci, 3, 1, 1, L) == (H.WINO4 if H.WINOGRAD_WGRAD else H.DIRECT)
        slabs = H.conv_wgrad_multi([(rlc(dy), rlc(x), 3, 1, 1)])
    finally:
        H.WINO4_WGRAD_MIN_C = old
    splits = slabs[0][1]
    for accumulate in (False, True):
        dw, = reduce_slabs(H, slabs, [(co, ci, 3)], accumulate, [base])
        bound = E.wino4_wgrad_bound(x, dy, splits, base=base if accumulate else None)
        err = np.abs(host(dw) - (base * accumulate + dw_ref))
        print('F(4,3) wgrad %s accumulate=%s: %d slabs, largest error / bound %.3f (error %.3g, bound there %.3g)' % (
            (ci, co, L, rows), accumulate, splits, (err / np.maximum(bound, 1e-300)).max(), err.max(), bound.flat[np.argmax(err)]))
        assert np.all(err <= bound), 'F(4,3) weight gradient outside its derived bound'
    # the F(2,3) form of the same job is exact, and the knob is back
    assert H.WINO4_WGRAD_MIN_C == old and H.wgrad_kernel(co, ci, 3, 1, 1, L) != H.WINO4
    dw2, = reduce_slabs(H, H.conv_wgrad_multi([(rlc(dy), rlc(x), 3, 1, 1)]), [(co, ci, 3)])
    eq(host(dw2), dw_ref, 'the F(2,3) form of the same job')


# ---------------------------------------------------------------------------------------------------------------------------
# bf16 operands (conv_bf16.hip): small integers are bf16 numbers, products and fp32 sums exact
# ---------------------------------------------------------------------------------------------------------------------------
BF16_SHAPES = [(32, 64, 1, 7), (64, 64, 2, 33), (64, 128, 3, 5), (128, 64, 5, 9), (96, 64, 7, 40), (64, 64, 9, 3),
               (64, 64, 57, 300)]


@pytest.mark.parametrize('ci,co,L,rows', BF16_SHAPES)
def test_bf16_k3_forward_and_data_gradient(H, ci, co, L, rows):
    x, w = E.operand(40, rows, ci, L), E.weight(41, co, ci, 3)
    dy = E.operand(42, rows, co, L)
    base = int_base(43, (rows, ci, L))
    E.bit_budget('direct', x, w, stride=1, pad=1)
    wf, wd = H.pack_conv3_bf16(cu(w))
    eq(host(wf), w.transpose(2, 0, 1), 'bf16 forward pack')
    eq(host(wd), w[:, :, ::-1].transpose(2, 1, 0), 'bf16 data-gradient pack')
    eq(ncl(H.conv3_bf16(rlc(x), wf)), E.conv_fwd(x, w, 1, 1), 'bf16 forward')
    if ci % 64 == 0:                                  # the data gradient's output channels are the conv's inputs
        E.bit_budget('direct_dgrad', dy, w, base=base, stride=1, pad=1, l=L)
        dx_ref = E.conv_dgrad(dy, w, 1, 1, L)
        eq(ncl(H.conv3_bf16(rlc(dy), wd)), dx_ref, 'bf16 data gradient')
        bt = rlc(base)
        H.conv3_bf16(rlc(dy), wd, out=bt, accumulate=True)
        eq(ncl(bt), base + dx_ref, 'bf16 data gradient, accumulate')


BF16_ENTRY_SHAPES = [(64, 64, 2, 7), (64, 128, 6, 33), (128, 64, 56, 5), (96, 64, 10, 9), (64, 128, 56, 300)]


@pytest.mark.parametrize('ci,co,L,rows', BF16_ENTRY_SHAPES)
def test_bf16_stride2_block_entry(H, ci, co, L, rows):
    x = E.operand(44, rows, ci, L)
    w3, w1 = E.weight(45, co, ci, 3), E.weight(46, co, ci, 1)
    E.bit_budget('direct', x, w3, stride=1, pad=1)
    (_, _, f3, d3), (_, _, f1, d1) = H.repack_multi([cu(w3), cu(w1)], [16, 16])
    xt = rlc(x)
    y3, y1 = H.conv_fwd_bf16_s2(xt, f3, f1)
    eq(ncl(y3), E.conv_fwd(x, w3, 2, 1), 'bf16 k3 s2 forward (pair launch)')
    eq(ncl(y1), E.conv_fwd(x, w1, 2, 0), 'bf16 k1 s2 forward (pair launch)')
    eq(ncl(H.conv_fwd_bf16_s2(xt, f3)), E.conv_fwd(x, w3, 2, 1), 'bf16 k3 s2 forward')
    eq(ncl(H.conv_fwd_bf16_s2(xt, f1)), E.conv_fwd(x, w1, 2, 0), 'bf16 k1 s2 forward')
    if ci % 64:
        return                                       # (the data gradients write ci channels: multiples of 64)
    dy3, dy1 = E.operand(47, rows, co, L // 2), E.operand(48, rows, co, L // 2)
    base = int_base(49, (rows, ci, L))
    dx3, dx1 = E.conv_dgrad(dy3, w3, 2, 1, L), E.conv_dgrad(dy1, w1, 2, 0, L)
    E.bit_budget('direct_dgrad', dy3, w3, base=np.abs(base) + E.conv_dgrad(np.abs(dy1), np.abs(w1), 2, 0, L), stride=2, pad=1, l=L)
    for dy, wd16, dx_ref, name in ((dy3, d3, dx3, 'k3'), (dy1, d1, dx1, 'k1')):
        eq(ncl(H.conv_dgrad_bf16_s2(rlc(dy), wd16, L)), dx_ref, 'bf16 %s s2 data gradient' % name)
        junk = torch.full((rows, L, ci), 7.0, device='cuda')
        H.conv_dgrad_bf16_s2(rlc(dy), wd16, L, out=junk, accumulate=False)
        eq(ncl(junk), dx_ref, 'bf16 %s s2 data gradient into a given out' % name)
        bt = rlc(base)
        H.conv_dgrad_bf16_s2(rlc(dy), wd16, L, out=bt, accumulate=True)
        eq(ncl(bt), base + dx_ref, 'bf16 %s s2 data gradient, accumulate' % name)
    eq(ncl(H.conv_dgrad_bf16_s2_pair(rlc(dy3), d3, rlc(dy1), d1, L)), dx3 + dx1, 'bf16 paired data gradient')


BF16_WGRAD_SHAPES = [(64, 64, 1, 7), (128, 64, 2, 33), (64, 192, 3, 5), (64, 64, 57, 9), (64, 64, 6, 300), (192, 128, 10, 130)]


@pytest.mark.parametrize('ci,co,L,rows', BF16_WGRAD_SHAPES)
def test_bf16_weight_gradients(H, ci, co, L, rows):
    x, dy = E.operand(50, rows, ci, L), E.operand(51, rows, co, L)
    base = int_base(52, (co, ci, 3))
    E.bit_budget('direct_wgrad', x, dy, base=base, stride=1, pad=1, k=3)
    dw_ref = E.conv_wgrad(x, dy, 3, 1, 1)
    xt, dyt = rlc(x), rlc(dy)
    H.WGRAD_BF16 = True
    try:
        assert H.wgrad_kernel(co, ci, 3, 1, 1, L) == H.BF16
        slabs = H.conv_wgrad_multi([(dyt, xt, 3, 1, 1)])
        for accumulate in (False, True):
            dw, = reduce_slabs(H, slabs, [(co, ci, 3)], accumulate, [base])
            eq(host(dw), base * accumulate + dw_ref, 'bf16 weight gradient, accumulate=%s' % accumulate)
        if L % 2 == 0:                                # the mixed batch of a stride-2 block: k3 s1 + k3 s2 + k1 s2, all bf16
            assert H.wgrad_kernel(co, ci, 3, 2, 1, L) == H.BF16 and H.wgrad_kernel(co, ci, 1, 2, 0, L) == H.BF16
            dy2 = E.operand(53, rows, co, L // 2)
            slabs = H.conv_wgrad_multi([(dyt, xt, 3, 1, 1), (rlc(dy2), xt, 3, 2, 1), (rlc(dy2), xt, 1, 2, 0)])
            d1, d2, d3 = reduce_slabs(H, slabs, [(co, ci, 3), (co, ci, 3), (co, ci, 1)])
            eq(host(d1), dw_ref, 'bf16 k3 s1 weight gradient in a mixed batch')
            eq(host(d2), E.conv_wgrad(x, dy2, 3, 2, 1), 'bf16 k3 s2 weight gradient')
            eq(host(d3), E.conv_wgrad(x, dy2, 1, 2, 0), 'bf16 k1 s2 weight gradient')
    finally:
        H.WGRAD_BF16 = False


# ---------------------------------------------------------------------------------------------------------------------------
# one mixed conv_wgrad_multi call
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('accumulate', [False, True])
def test_one_mixed_weight_gradient_call(H, accumulate):
    """More direct jobs than one 24-entry table holds, F(2,3) and F(4,3) jobs (the knob at 128 channels) and a dy_half job
    (position j of the recomputed X reads dy[j / 2] / 2: dyadic) in ONE conv_wgrad_multi call with chained reductions (dws=); every dW
    against its own oracle: equal, the F(4,3) jobs within their derived bound."""
    direct = [(128, 32, 3, 1, 1, 5, 3), (64, 64, 3, 2, 1, 6, 5), (32, 128, 1, 2, 0, 7, 4), (96, 128, 1, 1, 0, 3, 9),
              (128, 96, 3, 2, 1, 9, 2), (64, 64, 1, 1, 0, 2, 7), (64, 64, 3, 2, 1, 1, 6), (128, 32, 3, 1, 1, 7, 3),
              (64, 128, 1, 2, 0, 6, 40)]
    cases = [direct[i % len(direct)] for i in range(26)]
    cases[5:5] = [(64, 64, 3, 1, 1, 5, 9), (128, 128, 3, 1, 1, 6, 9)]                       # F(2,3), F(4,3)
    cases += [(64, 128, 3, 1, 1, 2, 33), (128, 128, 3, 1, 1, 1, 70), (128, 64, 3, 1, 1, 7, 150), (128, 128, 3, 1, 1, 9, 150)]
    old = H.WINO4_WGRAD_MIN_C
    H.WINO4_WGRAD_MIN_C = 128
    try:
        jobs, refs, kinds, data, bases = [], [], [], [], []
        for n, (ci, co, k, stride, pad, L, rows) in enumerate(cases):
            amp = 1 if min(ci, co) >= 128 and (k, stride, pad) == (3, 1, 1) else 2
            x, dy = E.operand(60 + n, rows, ci, L, amp=amp), E.operand(160 + n, rows, co, out_len(L, k, stride, pad), amp=amp)
            kind = H.wgrad_kernel(co, ci, k, stride, pad, L)
            E.bit_budget('direct_wgrad' if kind == H.DIRECT else 'wino_wgrad', x, dy, stride=stride, pad=pad, k=k, points=kind or 4)
            jobs.append((rlc(dy), rlc(x), k, stride, pad))
            refs.append(E.conv_wgrad(x, dy, k, stride, pad))
            kinds.append(kind)
            data.append((x, dy))
            bases.append(int_base(260 + n, (co, ci, k)))
        # the dense-block operand form: a 1x1 job whose dy has half the positions of x and enters halved, on the X the
        # forward never stored, max(fmaf(x, sc, sh), 0): with invstd 2, gamma 1/2, beta 0 that is relu(x - mean) exactly
        R = 9
        xstored, dyh = E.operand(58, 2 * R, 64, 6), E.operand(59, 2 * R, 64, 3)
        mean_v = np.random.default_rng(56).integers(-1, 2, (2, 64)).astype(np.float64)
        x = np.maximum(xstored - np.repeat(mean_v, R, axis=0)[:, :, None], 0)
        up = np.repeat(dyh, 2, axis=2) / 2
        E.bit_budget('direct_wgrad_half', x, up, stride=1, pad=0, k=1)
        xform = (cu(mean_v), torch.full((2, 64), 2.0, device='cuda'), torch.full((64,), 0.5, device='cuda'),
                 torch.zeros(64, device='cuda'), R)
        jobs.append((rlc(dyh), rlc(xstored), 1, 1, 0, {'dy_half': True, 'xform': xform}))
        refs.append(E.conv_wgrad(x, up, 1, 1, 0))
        kinds.append(H.DIRECT)
        data.append(None)
        bases.append(int_base(57, (64, 64, 1)))
        assert kinds.count(H.DIRECT) > 24 and (not H.WINOGRAD_WGRAD or (kinds.count(H.WINO2) >= 3 and kinds.count(H.WINO4) >= 3))
        dws = [cu(b) for b in bases]
        slabs, reduced = H.conv_wgrad_multi(jobs, dws=dws, accumulate=accumulate)
        assert any(reduced) and not all(reduced), reduced           # (chained: the last launch's jobs are the caller's)
        H.wgrad_reduce_multi([(sl, dw) for sl, dw, r in zip(slabs, dws, reduced) if not r], accumulate=accumulate)
    finally:
        H.WINO4_WGRAD_MIN_C = old
    for n, (dw, ref, kind, b, sl) in enumerate(zip(dws, refs, kinds, bases, slabs)):
        want = ref + b * accumulate
        if kind == H.WINO4:
            bound = E.wino4_wgrad_bound(*data[n], sl[1], base=b if accumulate else None)
            err = np.abs(host(dw) - want)
            print('mixed call job %d F(4,3): largest error / bound %.3f' % (n, (err / np.maximum(bound, 1e-300)).max()))
            assert np.all(err <= bound), 'job %d (F(4,3)) outside its derived bound' % n
        else:
            eq(host(dw), want, 'job %d %s kernel %d' % (n, (cases + [(64, 64, 1, 1, 0, 6, 18)])[n], kind))
