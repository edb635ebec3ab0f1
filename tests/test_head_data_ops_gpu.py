"""GPU parity of the kernels AROUND the convolutions and BatchNorms -- the fused head, the feature-boundary pools, the
device-resident data path, the test-epoch votes, reduce_rows and the two optimisers -- against the float64 oracle
(oracle/np_ref.py; its helpers are pinned to CPU torch in tests/test_small_ops_oracle_cpu.py).

Every test takes seeded numpy inputs whose values are exactly representable in the type the device holds them in, so the
reference sees the same numbers as the kernel.  The shapes are the smallest at which each code path of the kernels is
taken; none is the workload's own.  References are computed once per shape (lru_cache) and never modified.

Bounds.  fp32 kernels against float64: ``2e-6 * (1 + max|ref|)`` and the loss to ``2e-6``, as test_head_and_loss and
test_fused_head_chain_against_the_oracle_and_the_six_launch_chain (tests/test_hip_ops_gpu.py).  bf16 storage: float
outputs to the same bound on the bf16-rounded input; bf16 outputs within one bf16 ulp of the float64 value -- the inputs
of those tests are chosen so that no sum cancels (see the tests), otherwise the fp32 rounding of a nearly cancelled sum
would be judged by the ulp of its tiny result.  Gathers and votes: exact.  Each test prints the figure it achieved."""
import functools

import numpy as np
import pytest
import torch

from oracle import np_ref

pytestmark = pytest.mark.gpu
TOL = 2e-6


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


def f32r(a):
    """float64 array of float32-representable values (what the device holds exactly), read-only."""
    a = np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)
    a.setflags(write=False)
    return a


def cu(a, dtype=torch.float32):
    return torch.from_numpy(np.array(a, order='C')).to(dtype).cuda()       # (a copy: the cached inputs are read-only)


def host(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def close(got, ref, name, tol=TOL, scale=None):
    """max|got - ref| <= tol * scale, scale = 1 + max|ref| unless given; prints the figure."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, '%s: shape %s vs %s' % (name, got.shape, ref.shape)
    scale = 1.0 + np.abs(ref).max() if scale is None else scale
    err = np.abs(got - ref).max()
    assert np.isfinite(got).all(), '%s: non-finite values' % name
    print('%-58s max err %.3e  bound %.3e' % (name, err, tol * scale))
    assert err <= tol * scale, '%s: max err %.3e > %.3e' % (name, err, tol * scale)
    return err


def bf16_ulp(r):
    """One unit in the last place of bfloat16 (8 significand bits) at the magnitude of r."""
    return 2.0 ** (np.floor(np.log2(np.maximum(np.abs(r), 2.0 ** -126))) - 7)


def within_one_bf16_ulp(got16, ref, name):
    assert got16.dtype == torch.bfloat16, name
    got, ref = host(got16), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, name
    ratio = np.abs(got - ref) / bf16_ulp(ref)
    print('%-58s worst %.3f bf16 ulp' % (name, ratio.max()))
    assert ratio.max() <= 1.0, '%s: %d of %d elements beyond one bf16 ulp, worst %.3f ulp' % (
        name, int((ratio > 1.0).sum()), ratio.size, ratio.max())


# ----------------------------------------------------------------------------------------------------------------------
# fused head: head_fwd(finish=False) -> head_bwd, head_fwd(finish=True), head_flat_fwd / head_flat_bwd
# ----------------------------------------------------------------------------------------------------------------------
HEAD_SHAPES = [
    # B, R, L, F
    (3, 7, 5, 36),        # 63 (row, 4 features) items: one partly filled 256-item group; K/4 = 63: a partly filled last
                          # 16-quad weight block; F/4 = 9
    (2, 20, 9, 64),       # a second trip of the 8-deep load loop, 7 of its 8 reads clamped
    (2, 3, 16, 32),       # a second trip with no clamped read
    (512, 2, 3, 8),       # the last batch of the one-launch backward; head_finish_kernel strides over > 256 windows
    (513, 2, 3, 8),       # the first batch of the two-launch backward (HEAD_MAXB = 512)
    (1, 20, 7, 1024),     # DenseNet's feature width: 20 groups, 320 weight blocks for one window
]


@functools.lru_cache(maxsize=None)
def head_case(b, r, l, f, bias_mag=0.1, bf16=False):
    """-> xmap (B*R, L, F) in the device layout, w, bias, target, the oracle's results (dx in the device layout).
    bias_mag = 30: logits of about (+30, -30); all but a few windows have the target (1, 0) that agrees with them, so the
    loss stays O(1) (its 2e-6 bound is an absolute one) while log1p(exp(-|v|)) and the sigmoid run saturated; the few
    disagreeing windows keep the gradients away from zero.
    bf16: the map is bf16-representable, and w[1] has the sign opposite to w[0]: with one-hot targets dlogits[:, 0] and
    dlogits[:, 1] have opposite signs, so dx = (dl0 w0 + dl1 w1) / L never cancels and one bf16 ulp of dx is far above
    the fp32 rounding of the sum."""
    rng = np.random.default_rng(1000 + 131 * b + 17 * r + 5 * l + f)
    xmap = rng.standard_normal((b * r, l, f))
    xmap = np_ref.round_bf16(xmap) if bf16 else f32r(xmap)
    w = rng.standard_normal((2, r * f)) / np.sqrt(r * f)
    if bf16:
        w[1] = -np.sign(w[0]) * np.abs(w[1])
    w = f32r(w)
    bias = f32r([bias_mag, -bias_mag])
    if bias_mag > 1:
        cls = (rng.random(b) < 0.02).astype(np.int64)
        cls[b // 2] = 1
    else:
        cls = rng.integers(0, 2, b)
    target = f32r(np.eye(2)[cls])
    ref = np_ref.head_chain(xmap.transpose(0, 2, 1), w, bias, target, r)
    ref['dx'] = ref['dx'].transpose(0, 2, 1)
    for a in [xmap] + list(ref.values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return xmap, w, bias, target, ref


def run_head_checks(tag, fwd, bwd, w, ref, seed):
    """Every property the issue lists for one shape and one form (fwd / bwd: closures over the map or the features)."""
    rng = np.random.default_rng(seed)
    flat, part, logits, loss = fwd(False)
    dx, dw, db = bwd(part, flat, logits, loss)
    close(host(flat), ref['flat'], tag + ' flat')
    close(host(logits), ref['logits'], tag + ' logits')
    close(host(loss), [ref['loss']], tag + ' loss', scale=1.0)
    close(host(dx), ref['dx'], tag + ' dx')
    close(host(dw), ref['dw'], tag + ' dW')
    close(host(db), ref['dbias'], tag + ' dbias')
    # gscale = 0.5: the gradients scale, the loss and the logits do not
    lg2, ls2 = torch.empty_like(logits), torch.empty_like(loss)
    dx2, dw2, db2 = bwd(part, flat, lg2, ls2, gscale=0.5)
    close(host(dx2), 0.5 * ref['dx'], tag + ' gscale dx')
    close(host(dw2), 0.5 * ref['dw'], tag + ' gscale dW')
    close(host(db2), 0.5 * ref['dbias'], tag + ' gscale dbias')
    close(host(ls2), [ref['loss']], tag + ' gscale loss', scale=1.0)
    assert torch.equal(lg2, logits), tag + ': gscale moved the logits'
    # accumulate onto non-zero dW / dbias
    dw0, db0 = f32r(rng.standard_normal(w.shape) * 0.05), f32r(rng.standard_normal(2) * 0.05)
    dw3, db3 = cu(dw0), cu(db0)
    lg3, ls3 = torch.empty_like(logits), torch.empty_like(loss)
    dx3, dw3b, db3b = bwd(part, flat, lg3, ls3, dw=dw3, dbias=db3, accumulate=True)
    assert dw3b.data_ptr() == dw3.data_ptr() and db3b.data_ptr() == db3.data_ptr()
    close(host(dw3), dw0 + ref['dw'], tag + ' accumulate dW')
    close(host(db3), db0 + ref['dbias'], tag + ' accumulate dbias')
    close(host(dx3), ref['dx'], tag + ' accumulate dx')
    # the forward-only form: the same logits and loss
    flat4, _, lg4, ls4 = fwd(True)
    assert torch.equal(flat4, flat), tag + ': finish=True pooled other features'
    close(host(lg4), ref['logits'], tag + ' finish logits')
    close(host(ls4), [ref['loss']], tag + ' finish loss', scale=1.0)
    assert torch.equal(lg4, logits), tag + ': head_finish_kernel and head_bwd_kernel disagree about the logits'


@pytest.mark.parametrize('b,r,l,f,bias_mag', [s + (0.1,) for s in HEAD_SHAPES] + [(512, 2, 3, 8, 30.0)])
def test_fused_head_against_the_oracle(H, b, r, l, f, bias_mag):
    """head_fwd -> head_bwd and head_fwd(finish=True) on the map, head_flat_fwd -> head_flat_bwd on feat = map.mean(L):
    flat, logits, loss, dx, dW, dbias; gscale = 0.5; accumulate; the forward-only form.  The row with a bias of +-30
    runs log1p(exp(-|v|)) and the sigmoid saturated."""
    xmap, w, bias, target, ref = head_case(b, r, l, f, bias_mag)
    wt, bt, tt = cu(w), cu(bias), cu(target)
    xt = cu(xmap)
    tag = 'head (%d,%d,%d,%d)%s' % (b, r, l, f, ' bias 30' if bias_mag > 1 else '')
    run_head_checks(tag,
                    lambda finish: H.head_fwd(xt, wt, bt, tt, r, finish=finish),
                    lambda part, flat, lg, ls, **kw: H.head_bwd(part, bt, tt, flat, wt, lg, ls, r, l, **kw),
                    w, ref, seed=b + l)
    # the pair on pooled features: a map of ONE position, the pool is the identity
    feat = f32r(ref['flat'].reshape(b * r, f))
    ref1 = np_ref.head_chain(feat[:, :, None], w, bias, target, r)
    ref1['dx'] = ref1['dx'][:, :, 0]
    ft = cu(feat)
    run_head_checks(tag + ' flat form',
                    lambda finish: H.head_flat_fwd(ft, wt, bt, tt, r, finish=finish),
                    lambda part, flat, lg, ls, **kw: H.head_flat_bwd(part, bt, tt, flat, wt, lg, ls, r, **kw),
                    w, ref1, seed=b + l + 1)
    assert torch.equal(H.head_flat_fwd(ft, wt, bt, tt, r)[0].reshape(b * r, f), ft), 'the pool of one position is not the identity'


@pytest.mark.parametrize('b,r,l,f', [(3, 7, 5, 36), (2, 20, 9, 64)])
def test_fused_head_bf16_storage(H, b, r, l, f):
    """bf16 map and bf16 dx: the reference is computed on the bf16-rounded map; flat and logits (float) to the fp32
    bound, dx within one bf16 ulp of the float64 dx (head_case explains why its sums cannot cancel)."""
    xmap, w, bias, target, ref = head_case(b, r, l, f, 0.1, True)
    wt, bt, tt = cu(w), cu(bias), cu(target)
    tag = 'head bf16 (%d,%d,%d,%d)' % (b, r, l, f)
    with storage(H, 'bf16'):
        xt = cu(xmap, torch.bfloat16)
        assert np.array_equal(host(xt), xmap)
        flat, part, logits, loss = H.head_fwd(xt, wt, bt, tt, r)
        dx, dw, db = H.head_bwd(part, bt, tt, flat, wt, logits, loss, r, l)
        _, _, lgf, lsf = H.head_fwd(xt, wt, bt, tt, r, finish=True)
    assert H.act_dtype() == 'f32'
    assert flat.dtype == torch.float32 and logits.dtype == torch.float32
    close(host(flat), ref['flat'], tag + ' flat')
    close(host(logits), ref['logits'], tag + ' logits')
    close(host(lgf), ref['logits'], tag + ' finish logits')
    close(host(loss), [ref['loss']], tag + ' loss', scale=1.0)
    close(host(lsf), [ref['loss']], tag + ' finish loss', scale=1.0)
    close(host(dw), ref['dw'], tag + ' dW')
    close(host(db), ref['dbias'], tag + ' dbias')
    assert np.abs(ref['dx']).min() > 0
    within_one_bf16_ulp(dx, ref['dx'], tag + ' dx')


# ----------------------------------------------------------------------------------------------------------------------
# feature-boundary pools
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pool_case(rows, lin, k, c, bf16=False):
    """-> x (rows, L, C) device layout, dfeat (rows, C * Lout), feat and dx (device layout) of the oracle.  bf16: x is
    bf16-representable and the entries of dfeat that meet in one sum (one row, one channel) share a sign, |.| in
    [0.5, 1.5]: no sum of the backward cancels, so one bf16 ulp of dx is far above the fp32 rounding of the sum."""
    rng = np.random.default_rng(2000 + 97 * rows + 13 * lin + 3 * k + c)
    x = rng.standard_normal((rows, lin, c))
    x = np_ref.round_bf16(x) if bf16 else f32r(x)
    lo = lin - k + 1
    if bf16:
        d = rng.uniform(0.5, 1.5, (rows, c, lo)) * rng.choice([-1.0, 1.0], (rows, c, 1))
    else:
        d = rng.standard_normal((rows, c, lo))
    dfeat = f32r(d.reshape(rows, c * lo))
    feat = np_ref.avgpool_fwd(x.transpose(0, 2, 1), k, 1).reshape(rows, c * lo)       # feat[row][c * Lout + j]
    dx = np_ref.avgpool_slide_bwd(dfeat, k, lin, c).transpose(0, 2, 1)
    for a in (x, feat, dx):
        a.setflags(write=False)
    return x, dfeat, feat, dx


@pytest.mark.parametrize('rows,lin,c', [(3, 7, 32), (5, 1, 64), (2, 9, 36)])
def test_global_avgpool_against_the_oracle(H, rows, lin, c):
    x, dfeat, feat, dx = pool_case(rows, lin, lin, c)
    tag = 'global pool (%d,%d,%d)' % (rows, lin, c)
    got = H.global_avgpool_fwd(cu(x))
    assert tuple(got.shape) == (rows, c)
    close(host(got), feat, tag + ' feat')
    gdx = H.global_avgpool_bwd(cu(dfeat), lin)
    assert tuple(gdx.shape) == (rows, lin, c)
    close(host(gdx), dx, tag + ' dx')
    close(host(gdx), np.repeat(dfeat[:, None, :] / lin, lin, axis=1), tag + ' dx = dfeat / L')


@pytest.mark.parametrize('rows,lin,k,c', [(5, 7, 7, 64), (3, 8, 7, 32), (2, 16, 7, 512), (1, 14, 7, 1024)])
def test_sliding_avgpool_against_the_oracle(H, rows, lin, k, c):
    """feat[row][c * Lout + j] (the order of view() on (N, C, Lout)) and the overlap count of the backward: position l
    receives sum_{j = max(0, l-k+1)}^{min(l, Lout-1)} dfeat[c * Lout + j] / k.  Lout = 1 must equal the global pool."""
    x, dfeat, feat, dx = pool_case(rows, lin, k, c)
    tag = 'sliding pool (%d,%d,%d,%d)' % (rows, lin, k, c)
    xt, dt = cu(x), cu(dfeat)
    got = H.avgpool_slide_fwd(xt, k)
    assert tuple(got.shape) == (rows, c * (lin - k + 1))
    close(host(got), feat, tag + ' feat')
    gdx = H.avgpool_slide_bwd(dt, lin, k, c)
    assert tuple(gdx.shape) == (rows, lin, c)
    close(host(gdx), dx, tag + ' dx')
    if lin == k:
        assert torch.equal(got, H.global_avgpool_fwd(xt)), tag + ': Lout = 1 differs from the global pool'
        assert torch.equal(gdx, H.global_avgpool_bwd(dt, lin)), tag + ': Lout = 1 backward differs from the global pool'
    with pytest.raises(ValueError):
        H.avgpool_slide_bwd(dt[:, :-1].contiguous(), lin, k, c)


@pytest.mark.parametrize('rows,lin,k,c', [(3, 8, 7, 32), (2, 16, 7, 512)])
def test_pools_bf16_storage(H, rows, lin, k, c):
    """bf16 maps: features (float) to the fp32 bound on the rounded input, dx within one bf16 ulp of the float64 dx."""
    x, dfeat, feat, dx = pool_case(rows, lin, k, c, True)
    gfeat = np_ref.avgpool_fwd(x.transpose(0, 2, 1), lin, 1)[:, :, 0]
    gd = dfeat[:, :c]
    tag = 'pools bf16 (%d,%d,%d,%d)' % (rows, lin, k, c)
    with storage(H, 'bf16'):
        xt = cu(x, torch.bfloat16)
        assert np.array_equal(host(xt), x)
        s = H.avgpool_slide_fwd(xt, k)
        sdx = H.avgpool_slide_bwd(cu(dfeat), lin, k, c)
        g = H.global_avgpool_fwd(xt)
        gdx = H.global_avgpool_bwd(cu(gd), lin)
    assert H.act_dtype() == 'f32'
    assert s.dtype == torch.float32 and g.dtype == torch.float32
    close(host(s), feat, tag + ' sliding feat')
    close(host(g), gfeat, tag + ' global feat')
    within_one_bf16_ulp(sdx, dx, tag + ' sliding dx')
    within_one_bf16_ulp(gdx, np.repeat(gd[:, None, :] / lin, lin, axis=1), tag + ' global dx')


# ----------------------------------------------------------------------------------------------------------------------
# data path
# ----------------------------------------------------------------------------------------------------------------------
def flow_tiles(rng, shape):
    """float64 windows with flow-like magnitudes (|x| up to about 1e2), full float64 mantissas."""
    return np.clip(rng.standard_normal(shape) * 35.0, -120.0, 120.0)


def gather_indices(rng, n):
    """B = 1, and B > N: unsorted, with repeats, tile 0 and the last tile included."""
    many = np.concatenate([[n - 1, 0, 0, n - 1], rng.integers(0, n, 2 * n + 3)])
    rng.shuffle(many)
    return [np.array([n // 2]), np.array([n - 1]), many.astype(np.int64)]


@pytest.mark.parametrize('nb,l', [(3, 37), (20, 224)])
def test_gather_normalize_scalar_is_bit_identical_to_float64_numpy(H, nb, l):
    """tile_elems = 111 (less than a block) and 4480.  The kernel claims the bits of
    ``((tiles[idx] - mu) / std).astype(np.float32)`` in float64: exact equality, no tolerance."""
    rng = np.random.default_rng(31 + nb)
    n, mu, std = 6, -3.7, 23.4
    tiles = flow_tiles(rng, (n, nb, l))
    tt = torch.from_numpy(tiles).cuda()
    for idx in gather_indices(rng, n):
        ref = np_ref.gather_normalize(tiles, idx, mu, std)
        assert ref.dtype == np.float32 and ref.shape == (len(idx), nb, l)
        it = torch.from_numpy(idx).cuda()
        got = H.gather_normalize(tt, it, mu, std)
        assert got.dtype == torch.float32
        diff = int((got.cpu().numpy() != ref).sum())
        print('gather_normalize scalar tile %d B %d: %d elements differ' % (nb * l, len(idx), diff))
        assert diff == 0
        out = torch.full((len(idx), nb, l), float('nan'), device='cuda')
        assert H.gather_normalize(tt, it, mu, std, out=out) is out
        assert np.array_equal(out.cpu().numpy(), ref)
    with pytest.raises(ValueError):
        H.gather_normalize(tt, it, mu, std, out=torch.empty((len(idx), nb, l + 1), device='cuda'))
    with pytest.raises(ValueError):
        H.gather_normalize(tt.float(), it, mu, std)


@pytest.mark.parametrize('c', [2, 3, 4])
def test_gather_normalize_per_channel_is_bit_identical_to_float64_numpy(H, c):
    """(N, NB, C, L = 37) tiles: (i / L) % C crosses channel and breath boundaries inside a block of 256."""
    rng = np.random.default_rng(41 + c)
    n, nb, l = 5, 3, 37
    mu = [-3.7, 0.5, 12.0, -0.25][:c]
    std = [23.4, 7.0, 0.3, 110.0][:c]
    tiles = flow_tiles(rng, (n, nb, c, l))
    tt = torch.from_numpy(tiles).cuda()
    for idx in gather_indices(rng, n):
        ref = np_ref.gather_normalize(tiles, idx, mu, std)
        it = torch.from_numpy(idx).cuda()
        got = H.gather_normalize(tt, it, mu, std)
        diff = int((got.cpu().numpy() != ref).sum())
        print('gather_normalize C %d B %d: %d elements differ' % (c, len(idx), diff))
        assert diff == 0
        out = torch.full(tuple(ref.shape), float('nan'), device='cuda')
        assert H.gather_normalize(tt, it, mu, std, out=out) is out
        assert np.array_equal(out.cpu().numpy(), ref)
    with pytest.raises(ValueError):
        H.gather_normalize(tt, it, mu[:-1], std[:-1])


@pytest.mark.parametrize('width,b', [(2, 131), (32, 13), (2, 1)])
def test_gather_rows_is_exact(H, width, b):
    """Targets (width 2) and the [hx | cx] carry row (width 32); B * width = 262 / 416 is no multiple of the block."""
    rng = np.random.default_rng(51 + width + b)
    n = 9
    src = rng.standard_normal((n, width)).astype(np.float32)
    idx = rng.integers(0, n, b)
    idx[:2] = (n - 1, 0)[:min(b, 2)]
    if b > 2:
        idx[2] = idx[0]
    st, it = torch.from_numpy(src).cuda(), torch.from_numpy(idx.astype(np.int64)).cuda()
    got = H.gather_rows(st, it)
    assert np.array_equal(got.cpu().numpy(), src[idx])
    out = torch.full((b, width), float('nan'), device='cuda')
    assert H.gather_rows(st, it, out=out) is out
    assert np.array_equal(out.cpu().numpy(), src[idx])


# ----------------------------------------------------------------------------------------------------------------------
# test-epoch votes
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('b', [1, 257, 5000])
def test_vote_counts_against_argmax_and_add_at(H, b):
    """pred = torch.argmax on the CPU (first maximum: class 0 on an exact tie, -0.0 against 0.0 is a tie), votes =
    np.add.at; 3 groups, so thousands of integer atomics meet on six counters; two calls add into the same table; group
    ids outside [0, n_groups) pass the wrapper and must add nothing (the table is a slice of a larger zeroed buffer,
    whose other rows must stay zero).  Exact.  NaN logits are out of scope: argmax's NaN rule is not reproduced."""
    rng = np.random.default_rng(61 + b)
    n_groups = 3
    buf = torch.zeros((n_groups + 2, 2), dtype=torch.int32, device='cuda')
    votes = buf[1:1 + n_groups]
    ref_votes = None
    for call in range(2):
        logits = rng.standard_normal((b, 2)).astype(np.float32)
        logits[::5, 1] = logits[::5, 0]
        for i, pair in enumerate([(0.0, -0.0), (-0.0, 0.0), (0.0, 0.0), (-0.0, -0.0)]):
            if 1 + 5 * i < b:
                logits[1 + 5 * i] = pair
        if b == 1:
            logits[0] = [(0.0, -0.0), (-0.0, 0.0)][call]
        group = rng.integers(-1, n_groups + 1, b)                          # -1 and n_groups: outside
        if b == 1:
            group[0] = call * 2
        pred = H.vote_counts(cu(logits), torch.from_numpy(group).cuda(), votes)
        ref_pred, ref_votes = np_ref.vote_table(logits.astype(np.float64), group, n_groups, votes=ref_votes)
        tp = torch.argmax(torch.from_numpy(logits), dim=1).numpy()
        assert np.array_equal(ref_pred, tp)
        assert pred.dtype == torch.int32 and np.array_equal(pred.cpu().numpy(), tp)
        assert np.array_equal(votes.cpu().numpy(), ref_votes), 'call %d' % call
        assert H.vote_counts(cu(logits), torch.from_numpy(group).cuda(), torch.zeros_like(votes), want_pred=False) is None
    got = buf.cpu().numpy()
    assert not got[0].any() and not got[-1].any(), 'a group id outside the table was counted'
    print('vote_counts B %d: table %s' % (b, got[1:-1].tolist()))


# ----------------------------------------------------------------------------------------------------------------------
# reduce_rows
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows,n', [(1, 8), (31, 7), (33, 9), (5, 64), (1280, 64)])
def test_reduce_rows_against_a_float64_column_sum(H, rows, n):
    rng = np.random.default_rng(71 + rows + n)
    m = f32r(rng.standard_normal((rows, n)))
    scale = 1.0 + np.abs(m).sum(axis=0).max()
    mt = cu(m)
    out = H.reduce_rows(mt)
    assert tuple(out.shape) == (n,)
    close(host(out), m.sum(axis=0), 'reduce_rows (%d,%d)' % (rows, n), scale=scale)
    assert torch.equal(out, H.reduce_rows(mt)), 'two runs differ'
    o0 = f32r(rng.standard_normal(n))
    acc = cu(o0)
    assert H.reduce_rows(mt, out=acc, accumulate=True) is acc
    close(host(acc), o0 + m.sum(axis=0), 'reduce_rows (%d,%d) accumulate' % (rows, n), scale=scale)
    acc2 = cu(o0)
    H.reduce_rows(mt, out=acc2, accumulate=True)
    assert torch.equal(acc, acc2), 'two accumulating runs differ'
    H.reduce_rows(mt, out=acc2)                                              # without accumulate: overwritten
    assert torch.equal(acc2, out)


# ----------------------------------------------------------------------------------------------------------------------
# optimisers, judged by the update (p_after - p_before) / lr and by the state
# ----------------------------------------------------------------------------------------------------------------------
LR = 0.1          # with |p| <= 1e-2 one ulp of p, divided by lr, is below 1e-6 of a typical update
OPT_SIZES = [3, 4, 100003]


def dev_vec(a, off):
    """a on the device as elements [off:] of a fresh allocation: off = 1 is 4 bytes past a 16-byte boundary."""
    t = torch.empty(len(a) + off, device='cuda')
    t[off:] = cu(a)
    v = t[off:]
    assert v.data_ptr() % 16 == (4 * off) % 16
    return v


def rel_max(got, ref):
    return np.abs(np.asarray(got) - ref).max() / np.abs(ref).max()


@pytest.mark.parametrize('variant', ['clip_wd', 'noclip_nowd_gscale'])
@pytest.mark.parametrize('off', [0, 1])
@pytest.mark.parametrize('n', OPT_SIZES)
def test_sgd_nesterov_update_and_momentum_buffer(H, n, off, variant):
    """Three steps of clamp + weight decay + SGD(momentum .9, nesterov) against np_ref.sgd_nesterov_step in float64:
    the update (p_after - p_before) / lr and buf after every step, 2e-6 relative to the largest reference value.
    first=True runs on a buf full of NaN, which must not leak.  off = 1: p, g and buf start 4 bytes past a 16-byte
    boundary, the kernel's scalar path.  The second variant: clip = 0, weight_decay = 0, gscale = 0.25."""
    rng = np.random.default_rng(81 + n + off)
    clip, wd, gscale = (0.01, 1e-4, 1.0) if variant == 'clip_wd' else (0.0, 0.0, 0.25)
    p_ref = f32r(rng.uniform(-1e-2, 1e-2, n))
    buf_ref = None
    p = dev_vec(p_ref, off)
    buf = dev_vec(np.full(n, np.nan), off)
    worst_u = worst_b = 0.0
    for step in range(3):
        g = f32r(rng.standard_normal(n) * 0.02 / gscale)                     # about a third beyond the clip
        ge = g * gscale
        ge = np_ref.clamp_grad(ge, clip) if clip else ge
        p_new, buf_ref = np_ref.sgd_nesterov_step(p_ref, ge, buf_ref, lr=LR, momentum=0.9, wd=wd, first=(step == 0))
        before = host(p)
        H.clamp_sgd_nesterov_(p, dev_vec(g, off), buf, LR, 0.9, wd, clip, step == 0, gscale=gscale)
        upd, upd_ref = (host(p) - before) / LR, (p_new - p_ref) / LR
        assert np.isfinite(host(p)).all() and np.isfinite(host(buf)).all(), 'step %d: the NaN of buf leaked' % step
        worst_u, worst_b = max(worst_u, rel_max(upd, upd_ref)), max(worst_b, rel_max(host(buf), buf_ref))
        p_ref = p_new
    print('sgd n %d off %d %s: update %.3e  buf %.3e  (relative to the largest reference value, bound %.1e)' % (
        n, off, variant, worst_u, worst_b, TOL))
    assert worst_u <= TOL and worst_b <= TOL


def adam_state(rng, n, t0):
    """m, v as t0 - 1 steps would have left them (zeros before the first step)."""
    if t0 == 1:
        return np.zeros(n), np.zeros(n)
    return f32r(rng.standard_normal(n) * 0.005), f32r(rng.uniform(2e-5, 1e-4, n))


@pytest.mark.parametrize('off', [0, 1])
@pytest.mark.parametrize('n', OPT_SIZES)
def test_adam_host_step_update_and_moments(H, n, off):
    """clamp_adam_ at t = 1, 2, 10 (and the two steps after each) against np_ref.adam_step in float64 with torch's
    betas (0.9, 0.999) as doubles: the update, m and v after every step, 2e-6 relative to the largest reference value."""
    for t0 in (1, 2, 10):
        rng = np.random.default_rng(91 + n + off + t0)
        p_ref = f32r(rng.uniform(-1e-2, 1e-2, n))
        m_ref, v_ref = adam_state(rng, n, t0)
        p, m, v = dev_vec(p_ref, off), dev_vec(m_ref, off), dev_vec(v_ref, off)
        for t in range(t0, t0 + 3):
            g = f32r(rng.standard_normal(n) * 0.02)
            p_new, m_ref, v_ref = np_ref.adam_step(p_ref, np_ref.clamp_grad(g, 0.01), m_ref, v_ref, t, lr=LR)
            before = host(p)
            H.clamp_adam_(p, dev_vec(g, off), m, v, LR, t, 0.01)
            fig = (rel_max((host(p) - before) / LR, (p_new - p_ref) / LR), rel_max(host(m), m_ref), rel_max(host(v), v_ref))
            print('adam host n %d off %d t %d: update %.3e  m %.3e  v %.3e  (bound %.1e)' % ((n, off, t) + fig + (TOL,)))
            assert max(fig) <= TOL, 't = %d' % t
            p_ref = p_new


@pytest.mark.parametrize('n', OPT_SIZES)
@pytest.mark.parametrize('preset', [0, 999])
def test_adam_device_step_counter_and_update(H, n, preset):
    """clamp_adam_dev_ with its counter preset to 0 and to 999: the counter reads 1, 2, 3 / 1000, 1001, 1002 after the
    calls, and every step agrees with the float64 reference at that t and with the host-step form at the same t.
    Bound: the kernel forms 1 - beta^t in double from double betas, like the host form, so the host form's 2e-6 holds
    (an fp32 ``1 - powf(b2, t)`` would lose 2^-24 b2 / (1 - b2) = 6e-5 of bc2 at t = 1, 3e-5 of the step)."""
    rng = np.random.default_rng(101 + n + preset)
    p_ref = f32r(rng.uniform(-1e-2, 1e-2, n))
    m_ref, v_ref = adam_state(rng, n, preset + 1)
    p, m, v = cu(p_ref), cu(m_ref), cu(v_ref)
    ph, mh, vh = cu(p_ref), cu(m_ref), cu(v_ref)
    counter = torch.tensor([preset], dtype=torch.int64, device='cuda')
    for k in range(1, 4):
        t = preset + k
        g = f32r(rng.standard_normal(n) * 0.02)
        p_new, m_ref, v_ref = np_ref.adam_step(p_ref, np_ref.clamp_grad(g, 0.01), m_ref, v_ref, t, lr=LR)
        before, before_h = host(p), host(ph)
        H.clamp_adam_dev_(p, cu(g), m, v, LR, counter, 0.01)
        H.clamp_adam_(ph, cu(g), mh, vh, LR, t, 0.01)
        assert int(counter.item()) == t
        upd, upd_h, upd_ref = (host(p) - before) / LR, (host(ph) - before_h) / LR, (p_new - p_ref) / LR
        fig = (rel_max(upd, upd_ref), rel_max(host(m), m_ref), rel_max(host(v), v_ref), rel_max(upd, upd_h))
        print('adam dev n %d t %d: update %.3e  m %.3e  v %.3e  against the host form %.3e  (bound %.1e)' % ((n, t) + fig + (TOL,)))
        assert max(fig) <= TOL, 't = %d' % t
        assert torch.equal(m, mh) and torch.equal(v, vh), 'the moments do not depend on t'
        p_ref = p_new
    with pytest.raises(ValueError):
        H.clamp_adam_dev_(p, cu(g), m, v, LR, counter.int(), 0.01)
