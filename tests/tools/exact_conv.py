"""Exact-arithmetic conv testing on small-integer operands (pure numpy; nothing here touches a GPU).

Every conv kernel of the library accumulates in fp32, and every constant of the F(2,3) transforms and of the F(4,3) input /
output transforms is an integer or a half.  On small-integer operands every intermediate such a kernel can form -- whatever
its tiling, split-K, slab order or half tiles -- is an integer (or a multiple of 1/2) that fp32 holds exactly, so the result
must EQUAL the float64 convolution.  ``bit_budget`` proves the "holds exactly" part for the operands of a case before the
case is run; the oracles below are the float64 bilinear forms taking TRANSFORMED taps, so a kernel can be fed hand-made
integer taps (F(4,3): the tap generator's sixths are rounded, taps of a real weight are not exact).

The one inexact family is the F(4,3) weight gradient: its six accumulators are exact integers, the final combination with
sixths rounds.  ``wino4_wgrad_bound`` derives its componentwise bound from the roundings counted in the kernel's code.

Layout: operands are float64 (rows, C, L) arrays like oracle/np_ref.py's; taps are (points, N, C)."""
import numpy as np

# ---- the transforms, as the header comments of deepards_amd/csrc/conv_wino.hip state them -------------------------------------
# F(2,3): d0..d3 = x[2i-1 .. 2i+2];  D = B^T d;  y[2i], y[2i+1] = A^T m
BT2 = np.array([[1, 0, -1, 0],          # D0 = d0 - d2
                [0, 1, 1, 0],           # D1 = d1 + d2
                [0, -1, 1, 0],          # D2 = d2 - d1
                [0, 1, 0, -1]], float)  # D3 = d1 - d3
AT2 = np.array([[1, 1, 1, 0],           # y0 = m0 + m1 + m2
                [0, 1, -1, -1]], float)  # y1 = m1 - m2 - m3
G2 = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]])           # U = G g
# F(4,3): d0..d5 = x[4i-1 .. 4i+4]
BT4 = np.array([[4, 0, -5, 0, 1, 0],        # D0 = 4 d0 - 5 d2 + d4
                [0, -4, -4, 1, 1, 0],       # D1 = (d4 - 4 d2) + (d3 - 4 d1)
                [0, 4, -4, -1, 1, 0],       # D2 = (d4 - 4 d2) - (d3 - 4 d1)
                [0, -2, -1, 2, 1, 0],       # D3 = (d4 - d2) + 2 (d3 - d1)
                [0, 2, -1, -2, 1, 0],       # D4 = (d4 - d2) - 2 (d3 - d1)
                [0, 4, 0, -5, 0, 1]], float)  # D5 = 4 d1 - 5 d3 + d5
AT4 = np.array([[1, 1, 1, 1, 1, 0],
                [0, 1, -1, 2, -2, 0],
                [0, 1, 1, 4, 4, 0],
                [0, 1, -1, 8, -8, 1]], float)
G4 = np.array([[1 / 4., 0, 0], [-1 / 6., -1 / 6., -1 / 6.], [-1 / 6., 1 / 6., -1 / 6.],
               [1 / 24., 1 / 12., 1 / 6.], [1 / 24., -1 / 12., 1 / 6.], [0, 0, 1]])
# weight gradients: dm = A dy (the transpose of A^T), dW = G^T M
FORMS = {4: (BT2, AT2, G2), 6: (BT4, AT4, G4)}

EXACT_INT = 2.0 ** 24        # integers below this are fp32 numbers
EXACT_HALF = 2.0 ** 23       # multiples of 1/2 below this are


# ---- seeded integer generators ------------------------------------------------------------------------------------------------
def _nonzero(rng, shape, amp):
    return rng.integers(1, amp + 1, shape) * rng.choice([-1, 1], shape)


def operand(seed, rows, c, l, amp=2, zero=0.5):
    """A ReLU-like integer activation / gradient (rows, c, l) in {-amp .. amp}, float64: about ``zero`` of the entries of
    the live channels exactly 0, one whole channel of every 8 all 0 (c // 8 of them); in every live channel the first
    and the last position of every row and every position of the last row are non-zero, so that sequence edges and the last
    tile always carry data.  F(4,3) cases take amp = 1."""
    rng = np.random.default_rng([int(seed), rows, c, l, amp])
    x = _nonzero(rng, (rows, c, l), amp) * (rng.random((rows, c, l)) >= zero)
    edge = _nonzero(rng, (rows, c, l), amp)
    x[:, :, 0], x[:, :, -1], x[-1] = edge[:, :, 0], edge[:, :, -1], edge[-1]
    dead = [8 * g + int(rng.integers(8)) for g in range(c // 8)]      # one channel of every 8 (none below 8 channels)
    x[:, dead, :] = 0
    return x.astype(np.float64)


def dead_channels(x):
    return np.flatnonzero(~np.any(x != 0, axis=(0, 2)))


def weight(seed, co, ci, k, amp=2):
    """An integer conv weight (co, ci, k), uniform on {-amp .. amp}, float64."""
    rng = np.random.default_rng([int(seed), co, ci, k, amp, 7])
    return rng.integers(-amp, amp + 1, (co, ci, k)).astype(np.float64)


def int_taps(seed, points, n, c, amp=3):
    """Hand-made integer transformed taps (points, n, c), independent per point, uniform on {-amp .. amp}."""
    rng = np.random.default_rng([int(seed), points, n, c, amp, 11])
    return rng.integers(-amp, amp + 1, (points, n, c)).astype(np.float64)


def taps_from_weight(w, points, transpose=False):
    """U = G g in float64 from a (Co, Ci, 3) weight: (points, Co, Ci), or -- transpose -- the data gradient's
    (points, Ci, Co) with the taps reversed."""
    g = w[:, :, ::-1].transpose(1, 0, 2) if transpose else w
    return np.einsum('jt,nct->jnc', FORMS[points][2], g)


# ---- float64 oracles ----------------------------------------------------------------------------------------------------------
def tiles(x, points):
    """(rows, C, L) -> (rows, C, T, points): the inputs d_a = x[m i - 1 + a] of every output tile, zero outside the row."""
    m = points - 2
    rows, c, l = x.shape
    t = -(-l // m)
    xp = np.zeros((rows, c, m * t + 2))
    xp[:, :, 1:1 + l] = x
    return np.stack([xp[:, :, a:a + m * t:m] for a in range(points)], axis=3), t


def wino_fwd(x, u):
    """y = A^T [(U . B^T d)] of x (rows, C, L) with transformed taps u (points, N, C) -> (rows, N, L), float64."""
    points = u.shape[0]
    bt, at, _ = FORMS[points]
    d, t = tiles(x, points)
    dd = np.einsum('ja,rcta->jrtc', bt, d, optimize=True)
    mm = np.einsum('jnc,jrtc->jrtn', u, dd, optimize=True)
    y = np.einsum('oj,jrtn->rnto', at, mm, optimize=True)
    y = y.reshape(y.shape[0], y.shape[1], -1)[:, :, :x.shape[2]]
    return np.ascontiguousarray(y)


def wgrad_operands(x, dy, points, absolute=False):
    """dm = A dy (points, rows, T, N) and D = B^T d (points, rows, T, C) of a k3 s1 p1 weight-gradient job; absolute: the
    same with |A|, |B^T| on |dy|, |x| (upper bounds of |dm|, |D|)."""
    bt, at, _ = FORMS[points]
    m = points - 2
    if absolute:
        bt, at, x, dy = np.abs(bt), np.abs(at), np.abs(x), np.abs(dy)
    d, t = tiles(x, points)
    rows, n, l = dy.shape
    dyp = np.zeros((rows, n, m * t))
    dyp[:, :, :l] = dy
    dm = np.einsum('oj,rnto->jrtn', at, dyp.reshape(rows, n, t, m), optimize=True)
    dd = np.einsum('ja,rcta->jrtc', bt, d, optimize=True)
    return dm, dd


def wino_wgrad_sums(x, dy, points, absolute=False):
    """M_j[n][c] = sum over tiles dm_j[n] D_j[c] (points, N, C); absolute: sum |dm_j| |D_j| >= sum |dm_j D_j|."""
    dm, dd = wgrad_operands(x, dy, points, absolute)
    return np.einsum('jrtn,jrtc->jnc', dm, dd, optimize=True)


def wino_wgrad(x, dy, points):
    """dW (N, C, 3) = G^T M in float64."""
    return np.einsum('jt,jnc->nct', FORMS[points][2], wino_wgrad_sums(x, dy, points))


def conv_fwd(x, w, stride, pad):
    """float64 conv1d (rows, Ci, L) * (Co, Ci, k) with einsum (oracle/np_ref.conv1d_fwd's definition)."""
    rows, ci, l = x.shape
    co, _, k = w.shape
    lo = (l + 2 * pad - k) // stride + 1
    xp = np.zeros((rows, ci, l + 2 * pad))
    xp[:, :, pad:pad + l] = x
    y = np.zeros((rows, co, lo))
    for t in range(k):
        y += np.einsum('oc,rcl->rol', w[:, :, t], xp[:, :, t:t + (lo - 1) * stride + 1:stride], optimize=True)
    return y


def conv_dgrad(dy, w, stride, pad, l):
    rows, co, lo = dy.shape
    _, ci, k = w.shape
    dxp = np.zeros((rows, ci, l + 2 * pad))
    for t in range(k):
        dxp[:, :, t:t + (lo - 1) * stride + 1:stride] += np.einsum('oc,rol->rcl', w[:, :, t], dy, optimize=True)
    return np.ascontiguousarray(dxp[:, :, pad:pad + l])


def conv_wgrad(x, dy, k, stride, pad):
    rows, ci, l = x.shape
    _, co, lo = dy.shape
    xp = np.zeros((rows, ci, l + 2 * pad))
    xp[:, :, pad:pad + l] = x
    dw = np.zeros((co, ci, k))
    for t in range(k):
        dw[:, :, t] = np.einsum('rol,rcl->oc', dy, xp[:, :, t:t + (lo - 1) * stride + 1:stride], optimize=True)
    return dw


# ---- the exactness budget -----------------------------------------------------------------------------------------------------
class BudgetExceeded(AssertionError):
    pass


def bit_budget(kind, a, b, base=None, stride=1, pad=1, k=3, points=4, scale=1.0, l=None):
    """The largest intermediate the algorithm ``kind`` can form on these operands, computed in float64 from ABSOLUTE values
    (so it bounds every partial sum in every order); raises BudgetExceeded unless fp32 holds every such value exactly:
    below 2^24 where all intermediates are integers, below 2^23 where halves occur.  ``base``: what an accumulate form adds
    onto; ``scale``: a final exact power-of-two factor (dropout's 2).  -> the figure.

    kind 'direct' (a = x or dy, b = the (Co, Ci, k) weight as the conv reads it): sum |x| |w|
         'direct_dgrad' (a = dy, b = w, l = the input length): the transposed conv
         'direct_wgrad' (a = x, b = dy): sum |dy| |x|; 'direct_wgrad_half': dy holds halves (the dy_half operand form)
         'wino' (a = x, b = transformed taps (points, N, C)): |B^T| |d|, sum |U| |B^T d|, |A^T| |m|
         'wino_wgrad' (a = x, b = dy): |A| |dy|, |B^T| |d|, sum |dm_j| |D_j|, and -- F(2,3), whose combination is exact --
                      the combination |G^T| M (F(4,3): M only; the combination is what wino4_wgrad_bound bounds)."""
    a, b = np.abs(np.asarray(a, np.float64)), np.abs(np.asarray(b, np.float64))
    halves = False
    if kind == 'direct':
        peak = conv_fwd(a, b, stride, pad).max(initial=0)
    elif kind == 'direct_dgrad':
        peak = conv_dgrad(a, b, stride, pad, l).max(initial=0)
    elif kind in ('direct_wgrad', 'direct_wgrad_half'):
        peak = conv_wgrad(a, b, k, stride, pad).max(initial=0)
        halves = kind.endswith('half')
    elif kind == 'wino':
        bt, at, _ = FORMS[b.shape[0]]
        d, _ = tiles(a, b.shape[0])
        dd = np.einsum('ja,rcta->jrtc', np.abs(bt), d, optimize=True)
        mm = np.einsum('jnc,jrtc->jrtn', b, dd, optimize=True)
        y = np.einsum('oj,jrtn->rnto', np.abs(at), mm, optimize=True)
        peak = max(dd.max(initial=0), mm.max(initial=0), y.max(initial=0))
        halves = bool(np.any(b != np.floor(b)))
        if np.any(2 * b != np.floor(2 * b)):
            raise BudgetExceeded('taps that are not multiples of 1/2 are not exact territory')
    elif kind == 'wino_wgrad':
        dm, dd = wgrad_operands(a, b, points, absolute=True)
        ms = np.einsum('jrtn,jrtc->jnc', dm, dd, optimize=True)
        peak = max(dm.max(initial=0), dd.max(initial=0), ms.max(initial=0))
        if points == 4:
            peak = max(peak, np.einsum('jt,jnc->nct', np.abs(G2), ms).max(initial=0), (ms[1] + ms[2]).max(initial=0))
            halves = True
        else:
            peak = max(peak, (ms[1] + ms[2] + ms[3] + ms[4]).max(initial=0))      # s34 - s12 of the combination
    else:
        raise ValueError(kind)
    peak = float(peak) * scale
    if base is not None:
        peak += float(np.abs(base).max(initial=0))
        halves = halves or bool(np.any(base != np.floor(base)))
    limit = EXACT_HALF if halves else EXACT_INT
    if not peak < limit:
        raise BudgetExceeded('%s: intermediates up to %.4g leave exact fp32 territory (limit 2^%d)' %
                             (kind, peak, 23 if halves else 24))
    return peak


# ---- the one derived tolerance: the F(4,3) weight gradient --------------------------------------------------------------------
# Roundings of the combination, counted from the epilogue of wino4_wgrad_body (deepards_amd/csrc/conv_wino.hip).  acc[j] and
# s12 = acc[1] + acc[2], s34 = acc[3] + acc[4], acc[2] - acc[1], acc[3] - acc[4], s34 - s12 are exact integers (bit_budget).
#   o[0] = fmaf(0.25f, acc[0], fmaf(1.0f / 24.0f, s34, -(1.0f / 6.0f) * s12));
#          the constant 1/6 (1), the product with s12 (2), the constant 1/24 (3), the inner fmaf (4), the outer fmaf (5);
#          0.25f * acc[0] is exact inside the fmaf
#   o[plane] = fmaf(1.0f / 6.0f, acc[2] - acc[1], (1.0f / 12.0f) * (acc[3] - acc[4]));
#          the constant 1/12 (1), its product (2), the constant 1/6 (3), the fmaf (4)
#   o[2 * plane] = fmaf(1.0f / 6.0f, s34 - s12, acc[5]);
#          the constant 1/6 (1), the fmaf (2)
WINO4_WGRAD_ROUNDINGS = (5, 4, 2)
U32 = 2.0 ** -24


def wino4_wgrad_bound(x, dy, splits, base=None, extra=0):
    """Componentwise bound (N, C, 3) of |device dW - float64 dW| for the F(4,3) weight gradient on integer operands:
    n = c_t + splits (+ 1 with an accumulate ``base``) + extra roundings, each of at most 2^-24 of a partial result that
    T (+ |base|) bounds; T = |G^T| sum_quads |dm_j| |D_j| is the combination with every term taken positive, so it bounds
    every slab's partial combination (the slabs' T add up to it) and every partial sum of the slab reduction in any order.
    ``splits``: the slabs the reduction adds, one rounding each.  gamma_n = n u / (1 - n u) keeps it rigorous beyond first
    order."""
    t = np.einsum('jt,jnc->nct', np.abs(G4), wino_wgrad_sums(x, dy, 6, absolute=True))
    n = np.array(WINO4_WGRAD_ROUNDINGS, float) + splits + extra
    if base is not None:
        t, n = t + np.abs(base), n + 1
    return t * (n * U32 / (1 - n * U32))[None, None, :]
