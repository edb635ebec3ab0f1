"""The exactness claim behind tests/test_conv_exact_gpu.py, proved without a GPU: on the small-integer operands of
tests/tools/exact_conv.py each conv algorithm, emulated in numpy FLOAT32 with its contraction taken in three differently
shuffled orders (and cut into unequal partial sums, as split-K, slabs and half tiles do), is bit-equal to the float64
convolution -- so a device result that differs from the oracle in any bit has dropped, doubled or misplaced a term.
Also: the bilinear oracles against np_ref, the generators' guarantees, and bit_budget refusing an oversized case."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'tools'))

from oracle import np_ref  # noqa: E402
import exact_conv as E  # noqa: E402

F32 = np.float32
ORDERS = [0, 1, 2]


def contract32(a, b, order_seed):
    """sum_k a[k] (x) b[k] in float32, one rank-1 update after the other in a shuffled order of k, as three partial
    accumulators of unequal length that meet at the end (a (K, P), b (K, Q) -> (P, Q))."""
    a, b = a.astype(F32), b.astype(F32)
    k = a.shape[0]
    order = np.random.default_rng(order_seed).permutation(k)
    cuts = [0, k // 5, k // 5 + k // 2, k]
    parts = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        acc = np.zeros((a.shape[1], b.shape[1]), F32)
        for i in order[lo:hi]:
            acc += np.outer(a[i], b[i])                 # float32 products and sums
        parts.append(acc)
    assert all(p.dtype == F32 for p in parts)
    return (parts[2] + parts[0]) + parts[1]


def padded(x, pad):
    xp = np.zeros(x.shape[:2] + (x.shape[2] + 2 * pad,))
    xp[:, :, pad:pad + x.shape[2]] = x
    return xp


@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('k,stride,pad', [(3, 1, 1), (3, 2, 1), (1, 2, 0), (1, 1, 0)])
def test_direct_conv_in_float32_is_exact(k, stride, pad, order):
    rows, ci, co, l = 3, 32, 32, 7
    x, w = E.operand(1, rows, ci, l), E.weight(2, co, ci, k)
    E.bit_budget('direct', x, w, stride=stride, pad=pad)
    lo = (l + 2 * pad - k) // stride + 1
    xp = padded(x, pad)
    # contraction index = (channel, tap): a[(c, t)][n], b[(c, t)][(row, position)]
    a = np.stack([w[:, c, t] for c in range(ci) for t in range(k)])
    b = np.stack([xp[:, c, t:t + (lo - 1) * stride + 1:stride].reshape(-1) for c in range(ci) for t in range(k)])
    y = contract32(a, b, order).reshape(co, rows, lo).transpose(1, 0, 2)
    assert y.dtype == F32
    assert np.array_equal(y.astype(np.float64), np_ref.conv1d_fwd(x, w, stride, pad))
    # the weight gradient: contraction over (row, position)
    dy = E.operand(3, rows, co, lo)
    E.bit_budget('direct_wgrad', x, dy, stride=stride, pad=pad, k=k)
    dw_ref = np_ref.conv1d_bwd(x, w, dy, stride, pad, need_dx=False)[1]
    for t in range(k):
        xs = xp[:, :, t:t + (lo - 1) * stride + 1:stride]
        dw = contract32(dy.transpose(0, 2, 1).reshape(-1, co), xs.transpose(0, 2, 1).reshape(-1, ci), order)
        assert np.array_equal(dw.astype(np.float64), dw_ref[:, :, t])


def wino_fwd32(x, u, order):
    """The Winograd forward in float32: B^T d, per-point contraction over channels (shuffled, partial sums), A^T m."""
    points = u.shape[0]
    bt, at, _ = E.FORMS[points]
    d, t = E.tiles(x, points)
    rows, c = x.shape[:2]
    dd = np.einsum('ja,rcta->jcrt', bt.astype(F32), d.astype(F32)).astype(F32)          # integer transform, float32
    mm = np.stack([contract32(u[j].T, dd[j].reshape(c, -1), order + 10 * j) for j in range(points)])     # (points, N, rows * T)
    y = np.zeros((at.shape[0],) + mm.shape[1:], F32)
    for o in range(at.shape[0]):
        for j in range(points):
            if at[o, j]:
                y[o] += F32(at[o, j]) * mm[j]
    y = y.reshape(at.shape[0], u.shape[1], rows, t).transpose(2, 1, 3, 0).reshape(rows, u.shape[1], -1)
    assert y.dtype == F32
    return y[:, :, :x.shape[2]].astype(np.float64)


@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('l', [1, 2, 5, 7])
def test_winograd_f23_forward_in_float32_is_exact(l, order):
    rows, ci, co = 3, 32, 64
    x, w = E.operand(4, rows, ci, l), E.weight(5, co, ci, 3)
    u = E.taps_from_weight(w, 4)
    assert np.array_equal(u * 2, np.round(u * 2)) and np.array_equal(u.astype(F32).astype(np.float64), u)     # exact halves
    E.bit_budget('wino', x, u)
    assert np.array_equal(wino_fwd32(x, u, order), np_ref.conv1d_fwd(x, w, 1, 1))
    dy = E.operand(6, rows, co, l)
    ud = E.taps_from_weight(w, 4, transpose=True)
    E.bit_budget('wino', dy, ud)
    assert np.array_equal(wino_fwd32(dy, ud, order), np_ref.conv1d_bwd(x, w, dy, 1, 1)[0])


@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('l', [1, 2, 3, 5, 6, 7, 9])
def test_winograd_f43_forward_on_integer_taps_in_float32_is_exact(l, order):
    rows, c, n = 3, 64, 32
    x, u = E.operand(7, rows, c, l, amp=1), E.int_taps(8, 6, n, c)
    E.bit_budget('wino', x, u)
    assert np.array_equal(wino_fwd32(x, u, order), E.wino_fwd(x, u))


@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('l', [1, 2, 7])
def test_winograd_f23_weight_gradient_in_float32_is_exact(l, order):
    """M_j over pairs in float32 (shuffled, partial sums), then the kernel's combination: only halves, exact."""
    rows, ci, co = 5, 64, 64
    x, dy = E.operand(9, rows, ci, l), E.operand(10, rows, co, l)
    E.bit_budget('wino_wgrad', x, dy, points=4)
    dm, dd = E.wgrad_operands(x, dy, 4)
    m = [contract32(dm[j].reshape(-1, co), dd[j].reshape(-1, ci), order + 10 * j) for j in range(4)]
    h = F32(0.5)
    dw = np.stack([m[0] + (m[1] + m[2]) * h, (m[1] - m[2]) * h, (m[1] + m[2]) * h + m[3]], axis=2)
    assert dw.dtype == F32
    assert np.array_equal(dw.astype(np.float64), np_ref.conv1d_bwd(x, np.zeros((co, ci, 3)), dy, 1, 1, need_dx=False)[1])


@pytest.mark.parametrize('points', [4, 6])
@pytest.mark.parametrize('l', [1, 2, 3, 5, 6, 7, 9, 57])
def test_bilinear_oracles_equal_the_convolution(points, l):
    """On taps derived in float64 from a REAL weight the bilinear forms are the convolution and its gradients (1e-12)."""
    rng = np.random.default_rng([points, l])
    x, w, dy = rng.standard_normal((3, 32, l)), rng.standard_normal((64, 32, 3)), rng.standard_normal((3, 64, l))
    y_ref = np_ref.conv1d_fwd(x, w, 1, 1)
    dx_ref, dw_ref = np_ref.conv1d_bwd(x, w, dy, 1, 1)
    assert np.abs(E.wino_fwd(x, E.taps_from_weight(w, points)) - y_ref).max() <= 1e-12 * (1 + np.abs(y_ref).max())
    assert np.abs(E.wino_fwd(dy, E.taps_from_weight(w, points, True)) - dx_ref).max() <= 1e-12 * (1 + np.abs(dx_ref).max())
    assert np.abs(E.wino_wgrad(x, dy, points) - dw_ref).max() <= 1e-12 * (1 + np.abs(dw_ref).max())
    for s, p in ((1, 1), (2, 1)):                                     # the einsum oracles are np_ref's convolution
        assert np.array_equal(E.conv_fwd(x, w, s, p), np_ref.conv1d_fwd(x, w, s, p))
        dys = rng.standard_normal(np_ref.conv1d_fwd(x, w, s, p).shape)
        dx, dw = np_ref.conv1d_bwd(x, w, dys, s, p)
        assert np.allclose(E.conv_dgrad(dys, w, s, p, l), dx, rtol=0, atol=1e-12)
        assert np.allclose(E.conv_wgrad(x, dys, 3, s, p), dw, rtol=0, atol=1e-12)


def test_generators_are_deterministic_and_keep_their_guarantees():
    for amp in (1, 2):
        x = E.operand(11, 40, 64, 57, amp=amp)
        assert np.array_equal(x, E.operand(11, 40, 64, 57, amp=amp)) and not np.array_equal(x, E.operand(12, 40, 64, 57, amp=amp))
        assert np.array_equal(x, np.round(x)) and np.abs(x).max() == amp
        dead = E.dead_channels(x)
        assert len(dead) == 64 // 8 and all(np.sum((dead >= g) & (dead < g + 8)) == 1 for g in range(0, 64, 8))
        live = np.setdiff1d(np.arange(64), dead)
        assert np.all(x[:, live, 0] != 0) and np.all(x[:, live, -1] != 0) and np.all(x[-1][live] != 0)
        interior = x[:-1, live, 1:-1]
        assert 0.47 <= (interior == 0).mean() <= 0.53                  # about half the entries are exactly 0
        assert 0.5 <= (x == 0).mean() <= 0.6                           # ... a few more with the dead channels
    for l in (1, 2):                                                   # one- and two-position rows: all edge
        x = E.operand(3, 5, 32, l)
        assert np.all(x[:, np.setdiff1d(np.arange(32), E.dead_channels(x))] != 0)
    assert len(E.dead_channels(E.operand(3, 5, 3, 8))) == 0            # (a stem's 1 .. 3 input channels stay live)
    w = E.weight(13, 64, 32, 3)
    assert np.array_equal(w, E.weight(13, 64, 32, 3)) and set(np.unique(w)) == {-2., -1., 0., 1., 2.}
    u = E.int_taps(14, 6, 32, 64)
    assert np.array_equal(u, E.int_taps(14, 6, 32, 64)) and set(np.unique(u)) == {-3., -2., -1., 0., 1., 2., 3.}
    assert not np.array_equal(u[0], u[1])


def test_bit_budget_refuses_what_leaves_exact_territory():
    x, w = E.operand(15, 3, 32, 7), E.weight(16, 32, 32, 3)
    assert E.bit_budget('direct', x, w) < 2 ** 24
    with pytest.raises(E.BudgetExceeded):
        E.bit_budget('direct', x * 2.0 ** 12, w * 2.0 ** 12)           # 2^24 * (a few hundred terms)
    with pytest.raises(E.BudgetExceeded):
        E.bit_budget('direct', x, w, base=np.full((3, 32, 7), 2.0 ** 24))
    u = E.taps_from_weight(w, 4)
    ok = E.bit_budget('wino', x, u)
    up = 2.0 ** np.floor(np.log2(2.0 ** 24 / ok))                      # ok * up in (2^23, 2^24]
    with pytest.raises(E.BudgetExceeded):                              # halves: one bit less
        E.bit_budget('wino', x * up, u)
    assert 2 ** 22 < E.bit_budget('wino', x * up / 2, u) < 2 ** 23
    with pytest.raises(E.BudgetExceeded):                              # sixths are not exact territory at all
        E.bit_budget('wino', x, E.taps_from_weight(w, 6))
    dy = E.operand(17, 3, 32, 7)
    for points in (4, 6):
        assert E.bit_budget('wino_wgrad', x, dy, points=points) < 2 ** 23
        with pytest.raises(E.BudgetExceeded):
            E.bit_budget('wino_wgrad', x * 2.0 ** 12, dy * 2.0 ** 12, points=points)


def test_f43_weight_gradient_bound_is_derived_from_the_counted_roundings():
    """The bound is (c + splits) gamma-style roundings of T; emulating the kernel's combination in float32 stays inside."""
    x, dy = E.operand(18, 9, 64, 7, amp=1), E.operand(19, 9, 64, 7, amp=1)
    E.bit_budget('wino_wgrad', x, dy, points=6)
    assert E.WINO4_WGRAD_ROUNDINGS == (5, 4, 2)
    m = E.wino_wgrad_sums(x, dy, 6).astype(F32)
    assert np.array_equal(m.astype(np.float64), E.wino_wgrad_sums(x, dy, 6))            # the accumulators are exact
    s12, s34 = m[1] + m[2], m[3] + m[4]
    c6, c12, c24 = F32(1) / F32(6), F32(1) / F32(12), F32(1) / F32(24)
    # (numpy has no fmaf: the separate product adds roundings the bound does not count, so allow them here: + 2 each)
    dw = np.stack([F32(0.25) * m[0] + (c24 * s34 - c6 * s12), c6 * (m[2] - m[1]) + c12 * (m[3] - m[4]), c6 * (s34 - s12) + m[5]], axis=2)
    bound = E.wino4_wgrad_bound(x, dy, splits=1, extra=2)
    assert bound.shape == dw.shape and np.all(bound[np.abs(E.wino_wgrad(x, dy, 6)) > 0] > 0)
    assert np.all(np.abs(dw.astype(np.float64) - E.wino_wgrad(x, dy, 6)) <= bound)
    assert np.all(E.wino4_wgrad_bound(x, dy, 1) < 8 * 2.0 ** -24 * np.abs(E.G4).sum(0).max() * E.wino_wgrad_sums(x, dy, 6, True).max())
