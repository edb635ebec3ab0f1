"""skip5: the F(4,3) conv and weight-gradient kernels without the sixth product of half-empty quads.

With exactly two quads a row and L % 4 != 0 (L = 5, 6, 7) the second quad of every row has no fourth output, so its
m5 = D5 . U5 (forward / data gradient) feeds nothing and its dm5 = dy3 (weight gradient) is a zero of the loader.  The
kernels then compute point 5 for first quads only.  No result bit may move: every case here runs the kernel in both forms
(da_debug_set key 11: 0 = six products for every quad) on the same operands and asks for torch.equal, guard rows included;
one probe on integer operands pins where the first quads' point-5 product lands against the direct convolution."""
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

GUARD_ROWS, PATTERN = 3, -12345.0


@pytest.fixture(scope='module')
def H():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from deepards_amd import hip_ops
    return hip_ops


def both_forms(run):
    """run() with the six-product form, then with the default form (skip5 where it applies); the switch is put back."""
    from deepards_amd import _lib
    lib = _lib.lib()
    assert lib.da_debug_set(11, 0) == 0
    try:
        six = run()
        torch.cuda.synchronize()
    finally:
        assert lib.da_debug_set(11, 1) == 0
    new = run()
    torch.cuda.synchronize()
    return six, new


def rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).cuda()


def conv_into_guarded(H, x, u, base, accumulate):
    """conv3_winograd into the first rows of a buffer whose last GUARD_ROWS rows hold PATTERN -> the whole buffer."""
    rows, L, _ = x.shape
    n = u.shape[1]
    buf = torch.full((rows + GUARD_ROWS, L, n), PATTERN, device='cuda')
    buf[:rows] = base                                     # (accumulate off: the kernel must overwrite every element of it)
    H.conv3_winograd(x, u, out=buf[:rows], accumulate=accumulate)
    return buf


# (rows, L, C, N): less than a tile and a ragged last tile at every skip5 length; 264 tiles -> a last round of half tiles
# (two K halves meet in LDS); L = 4, 8, 11: one, two full and three quads a row, where skip5 must stay off
CONV_SHAPES = [(rows, L, 32, 32) for rows in (20, 100) for L in (5, 6, 7)] + [(1040, 7, 32, 256)] + \
              [(20, L, 32, 32) for L in (4, 8, 11)]


@pytest.mark.parametrize('accumulate', [False, True])
@pytest.mark.parametrize('rows,L,C,N', CONV_SHAPES)
def test_conv_is_bit_equal_in_both_forms(H, rows, L, C, N, accumulate):
    x = rnd(1, rows, L, C)
    u = H.wino_weights(rnd(2, N, C, 3) * 0.1, points=6)
    base = rnd(3, rows, L, N)
    six, new = both_forms(lambda: conv_into_guarded(H, x, u, base, accumulate))
    assert torch.equal(six[rows:], torch.full_like(six[rows:], PATTERN)), 'six-product form wrote behind its output'
    assert torch.equal(new[rows:], torch.full_like(new[rows:], PATTERN)), 'the guard rows behind the output changed'
    assert torch.isfinite(new[:rows]).all()
    assert torch.equal(six, new), 'rows %d L %d: %d elements differ between the forms' % (rows, L, int((six != new).sum()))
    if not accumulate:
        assert not torch.equal(new[:rows], base)


def _int_conv(x, w):
    """float64 k3 s1 p1 convolution: x (rows, L, C), w (N, C, 3) -> (rows, L, N)"""
    rows, L, C = x.shape
    xp = np.zeros((rows, L + 2, C))
    xp[:, 1:L + 1] = x
    return sum(np.einsum('rlc,nc->rln', xp[:, t:t + L], w[:, :, t]) for t in range(3))


def _probe(H, x, w, what):
    u = E.taps_from_weight(w, 6)
    assert np.abs(u - np.round(u)).max() < 1e-9           # w = 24 * integers: every transformed tap is an integer
    xt = torch.from_numpy(x.astype(np.float32)).cuda()
    ut = torch.from_numpy(np.round(u).astype(np.float32)).cuda()
    base = torch.zeros((x.shape[0], x.shape[1], w.shape[0]), device='cuda')
    buf = conv_into_guarded(H, xt, ut, base, False)
    rows = x.shape[0]
    assert torch.equal(buf[rows:], torch.full_like(buf[rows:], PATTERN)), what + ': guard rows changed'
    got, ref = buf[:rows].cpu().numpy().astype(np.float64), _int_conv(x, w)
    bad = np.argwhere(got != ref)
    assert not len(bad), '%s: %d elements differ from the direct convolution, first at %s: got %r, expected %r' % (
        what, len(bad), tuple(bad[0]), got[tuple(bad[0])], ref[tuple(bad[0])])


def test_fixed_probe_equals_the_integer_convolution(H):
    """x is zero but for one 1.0, the weights are 24 * {-2 .. 2} (integer transformed taps): every output is an integer the
    kernel holds exactly.  Position 6 (second quad: its outputs must do without m5, and nothing may leak into y3 of the
    first quad) and position 3, in a row of the tile's second 16-row half.  Then a sweep: every position (4 is the one
    whose only trace in the first quad is m5), in rows of both 16-row halves of a tile and of the ragged second tile,
    several input channels, both output channel halves."""
    rows, L, C, N = 40, 7, 32, 32
    w = 24.0 * np.random.default_rng(5).integers(-2, 3, (N, C, 3)).astype(np.float64)
    for pos in (6, 3):
        x = np.zeros((rows, L, C))
        x[9, pos, 5] = 1.0
        _probe(H, x, w, 'single 1.0 at position %d' % pos)
    for pos in range(L):
        x = np.zeros((rows, L, C))
        for r, c in ((0, 0), (9, 5), (17, 18), (30, 31), (39, 7)):
            x[r, pos, c] = 1.0
        _probe(H, x, w, 'sweep, position %d' % pos)


# (rows, L): the conv cases' rows and lengths; 333 rows of 2 quads = 666 quads -> 3 splits of 224, the last one 218 quads
# (no multiple of the 16-quad K step, nor of the split length); L = 4, 8, 11: skip5 off
WGRAD_SHAPES = [(rows, L) for rows in (20, 100) for L in (5, 6, 7)] + [(333, 7)] + [(20, L) for L in (4, 8, 11)]


@pytest.mark.parametrize('rows,L', WGRAD_SHAPES)
def test_weight_gradient_is_bit_equal_in_both_forms(H, rows, L):
    co = ci = 64
    dy, x = rnd(6, rows, L, co), rnd(7, rows, L, ci)
    dy = dy * (rnd(8, rows, L, co) > 0)                     # a ReLU-like gradient: exact zeros among the operands

    def run():
        old = H.WINO4_WGRAD_MIN_C
        H.WINO4_WGRAD_MIN_C = 64
        try:
            assert H.wgrad_kernel(co, ci, 3, 1, 1, L) == H.WINO4
            slabs = H.conv_wgrad_multi([(dy, x, 3, 1, 1)])
        finally:
            H.WINO4_WGRAD_MIN_C = old
        dw = torch.full((co, ci, 3), 7.0, device='cuda')
        H.wgrad_reduce_multi([(slabs[0], dw)], accumulate=True)
        return slabs[0][0], slabs[0][1], dw

    if not H.WINOGRAD_WGRAD:
        raise AssertionError('the Winograd weight gradients are switched off')
    (slab6, sp6, dw6), (slab5, sp5, dw5) = both_forms(run)
    assert sp6 == sp5 and slab6.shape == slab5.shape
    if (rows, L) == (333, 7):
        assert sp5 == 3
    assert torch.isfinite(slab5).all() and float(slab5.abs().max()) > 0
    assert torch.equal(slab6, slab5), '%d slab elements differ between the forms' % int((slab6 != slab5).sum())
    assert torch.equal(dw6, dw5)


def test_two_resnet18_training_steps_are_bit_equal_in_both_forms(H):
    """B = 2 windows of (20, 1, 224): layer 4 runs its k3 s1 convs at 40 rows of L = 7 on the F(4,3) kernels (forward, data
    and weight gradients).  Parameters, gradients and momentum after two steps, and the BatchNorm buffers."""
    import deepards_amd.models as M
    from deepards_amd.train import HotPathTrainer
    from oracle.weights import seeded_params, seeded_batch
    assert H.conv_kernel_wanted(512, 512, 3, 1, 1) == H.WINO4 and H.wgrad_kernel(512, 512, 3, 1, 1, 7) == H.WINO4
    x, t = seeded_batch(2, 20, 0)
    xt, tt = torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda()

    def run():
        model = M.CNNLinearNetwork(M.resnet18(), 20, 0)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_params('resnet18', 0).items()}, strict=False)
        tr = HotPathTrainer(model.cuda(), use_graph=False)
        losses = [float(tr.train_step(xt, tt).detach()) for _ in range(2)]
        return losses, tr.bucket.p.clone(), tr.bucket.g.clone(), tr.state['buf'].clone(), [b.clone() for b in model.buffers()]

    (l6, p6, g6, m6, b6), (l5, p5, g5, m5, b5) = both_forms(run)
    assert l6 == l5 and all(np.isfinite(l5))
    assert torch.equal(p6, p5), 'parameters differ'
    assert torch.equal(g6, g5), 'gradients differ'
    assert torch.equal(m6, m5), 'momentum differs'
    assert len(b6) == len(b5) and all(torch.equal(a, b) for a, b in zip(b6, b5)), 'buffers differ'
    assert float(g5.abs().max()) > 0
