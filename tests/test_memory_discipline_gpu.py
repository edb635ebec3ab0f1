"""Memory discipline of every kernel-launching wrapper of deepards_amd/hip_ops.py (tests/tools/poison.py): one table of op
cases, five checks over it, each against a second run of the same op BIT FOR BIT (no tolerances):

  1 uninitialised   under poisoned_allocations() (torch.empty & co. return a NaN pattern) the public results keep their bits
  2 guards          every tensor operand inside pattern-filled guard bands: same bits, guards untouched
  3 dirty_out       out / dx / dw of an overwriting call pre-filled with the pattern: same bits
  4 isolation       one input row (conv, pool, stem, gather, median, LSTM) or BatchNorm window set to NaN: the others keep theirs
  5 repeat          the op again after a different-shaped case of its family: same bits (plans / workspaces of another shape)

and the whole step (model construction, one eager training step, a forward-only step, three captured steps) under the patch.
Parity with the oracle is the business of the other GPU files; nothing here provokes a fault -- an overrun lands in a guard
band this file allocated."""
import contextlib
import inspect
import os
import sys
import zlib

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

from tools import poison as P  # noqa: E402

if torch.cuda.is_available():
    from deepards_amd import hip_ops as H, _lib
else:                                   # collected without a GPU (-m "not gpu" deselects every test of this file)
    H = _lib = None

CASES = []
COVERED = {}


class Rng(object):
    def __init__(self, name):
        self.g = torch.Generator().manual_seed(zlib.crc32(name.encode()))

    def n(self, *shape):
        return torch.randn(*shape, generator=self.g).cuda()

    def u(self, *shape):                # in [0.5, 1.5): gammas, variances
        return (torch.rand(*shape, generator=self.g) + 0.5).cuda()


def zeros(*shape, **kw):
    return torch.zeros(*shape, device='cuda', **kw)


def case(name, family, ops, build, call, dests=(), rows=None, note='', setup=None):
    """A table row; ``ops``: the hip_ops wrappers the row stands for in the completeness test.  build(r) gets the row's
    seeded generator.  A row of one window has no neighbour: it takes no isolation spec, and its note says so."""
    if rows is not None and rows['windows'] < 2:
        rows, note = None, (note + '; ' if note else '') + 'one row / window: nothing to isolate it from, exempt from check 4'
    CASES.append(P.OpCase(name, family, lambda: build(Rng(name)), call, dests=dests, rows=rows, note=note, setup=setup))
    for op in ops.split():
        COVERED.setdefault(op, []).append(name)


def tile_mid(rows, l, tile=64):
    """A middle row that starts on a 64-position tile boundary when there is one, else the middle."""
    for r in range(max(1, rows // 2), rows - 1):
        if (r * l) % tile == 0:
            return r
    for r in range(1, rows - 1):
        if (r * l) % tile == 0:
            return r
    return rows // 2


def iso(names, rows, l=1, R=1, axis=None):
    return dict(inputs=tuple(names.split()), R=R, windows=rows // R, mid=tile_mid(rows // R, l * R), axis=axis or {})


# ---- debug knobs, restored on the way out -----------------------------------------------------------------------------------
@contextlib.contextmanager
def wino4_ksteps(k):
    _lib.lib().da_wino_debug_tail(3 if k == 16 else 2)
    try:
        yield
    finally:
        _lib.lib().da_wino_debug_tail(3)


@contextlib.contextmanager
def wino_half_tiles(on):
    _lib.lib().da_wino_debug_tail(1 if on else 0)
    try:
        yield
    finally:
        _lib.lib().da_wino_debug_tail(1)


@contextlib.contextmanager
def bn_two_stage():
    H.bn_debug_two_stage(True)
    try:
        yield
    finally:
        H.bn_debug_two_stage(False)


@contextlib.contextmanager
def bn_blocks8():
    _lib.lib().da_bn_debug_target_blocks(1 << 20)
    try:
        yield
    finally:
        _lib.lib().da_bn_debug_target_blocks(256)


@contextlib.contextmanager
def direct_only():
    old = H.WINOGRAD_WGRAD
    H.WINOGRAD_WGRAD = False
    try:
        yield
    finally:
        H.WINOGRAD_WGRAD = old


@contextlib.contextmanager
def bf16_storage():
    H.set_act_dtype('bf16')
    try:
        yield
    finally:
        H.set_act_dtype('f32')


# ================================================================================================================================
# the table
# ================================================================================================================================
def _table():
    # ---- direct convs: k1 / k3, stride 1 / 2, C = 32, one row, the short lengths, > 256 tiles with a part-filled last round ----
    def wgrad_channels(ci, co):
        """The weight-gradient tiles are 128x128 ... 64x64, 128x32 and 32x128: a side of 32 channels needs 128 on the other."""
        if min(ci, co) == 32 and max(ci, co) % 128:
            return (ci, 128) if ci == 32 else (128, co)
        return ci, co

    def conv_rows(tag, ci, co, k, stride, pad, l, rows):
        lo = H.conv_out_len(l, k, stride, pad)
        if lo < 1:
            return
        name = '%s_c%d_n%d_k%d_s%d_l%d_r%d' % (tag, ci, co, k, stride, l, rows)

        def b_fwd(r):
            w = r.n(co, ci, k) * 0.1
            wf, _ = H.repack_weight(w, True, False)
            return dict(x=r.n(rows, l, ci), wf=wf, out=zeros(rows, lo, co))
        case('conv_fwd_' + name, 'direct', 'conv_fwd', b_fwd,
             lambda x, wf, out: H.conv_fwd(x, wf, stride, pad, out=out), dests=('out',), rows=iso('x', rows, l))

        def b_dg(r):
            w = r.n(co, ci, k) * 0.1
            _, wd = H.repack_weight(w, False, True)
            return dict(dy=r.n(rows, lo, co), wd=wd, out=zeros(rows, l, ci))
        case('conv_dgrad_' + name, 'direct', 'conv_dgrad', b_dg,
             lambda dy, wd, out: H.conv_dgrad(dy, wd, stride, pad, l, out=out), dests=('out',), rows=iso('dy', rows, lo))

        wci, wco = wgrad_channels(ci, co)

        def b_wg(r):
            return dict(dy=r.n(rows, lo, wco), x=r.n(rows, l, wci), out=zeros(wco, wci, k))
        case('conv_wgrad_%s_c%d_n%d_k%d_s%d_l%d_r%d' % (tag, wci, wco, k, stride, l, rows), 'wgrad', 'conv_wgrad', b_wg,
             lambda dy, x, out: H.conv_wgrad(dy, x, k, stride, pad, out=out), dests=('out',),
             note='reduces over rows: exempt from the isolation check; C = 32 against 32 / 64 channels has no weight-gradient '
                  'tile (the library refuses it): the other side is 128, the nearest shape it takes')

    for l in (1, 2, 7, 9, 56, 57):
        conv_rows('edge', 32, 32, 3, 1, 1, l, 1)
        conv_rows('edge', 32, 64, 1, 1, 0, l, 3)
        conv_rows('edge', 32, 32, 3, 2, 1, l, 5)
        conv_rows('edge', 64, 32, 1, 2, 0, l, 5)
    conv_rows('tail', 64, 64, 3, 1, 1, 56, 300)
    conv_rows('tail', 64, 128, 3, 2, 1, 56, 300)
    conv_rows('tail', 128, 64, 1, 1, 0, 14, 1200)
    conv_rows('k7', 32, 32, 7, 1, 3, 28, 5)          # three launches of at most three taps

    def b_allocs(r):
        return dict(x=r.n(7, 9, 32), wf=H.repack_weight(r.n(128, 32, 3) * 0.1)[0], dy=r.n(7, 9, 128),
                    wd=H.repack_weight(r.n(128, 32, 3) * 0.1, False, True)[1])
    case('conv_own_outputs', 'direct', 'conv_fwd conv_dgrad conv_wgrad', b_allocs,
         lambda x, wf, dy, wd: (H.conv_fwd(x, wf, 1, 1), H.conv_dgrad(dy, wd, 1, 1, 9), H.conv_wgrad(dy, x, 3, 1, 1),
                                H.conv_dgrad(dy, wd, 2, 1, 18)),
         note='the wrappers allocate their own outputs (check 1 is the one that matters here)')

    for rows, l in ((5, 56), (300, 14), (3, 2)):
        def b_multi(r, rows=rows, l=l):
            w1, wd_ = r.n(128, 64, 3) * 0.1, r.n(128, 64, 1) * 0.1
            return dict(x=r.n(rows, l, 64), w1=H.repack_weight(w1)[0], w2=H.repack_weight(wd_)[0])
        case('conv_fwd_multi_l%d_r%d' % (l, rows), 'direct', 'conv_fwd_multi', b_multi,
             lambda x, w1, w2: H.conv_fwd_multi([(x, w1, 2, 1), (x, w2, 2, 0)]), rows=iso('x', rows, l))

        def b_pair(r, rows=rows, l=l):
            w1, wd_ = r.n(128, 64, 3) * 0.1, r.n(128, 64, 1) * 0.1
            return dict(dy1=r.n(rows, l // 2, 128), dyd=r.n(rows, l // 2, 128), wd1=H.repack_weight(w1, False, True)[1],
                        wdd=H.repack_weight(wd_, False, True)[1])
        case('conv_dgrad_s2_pair_l%d_r%d' % (l, rows), 'direct', 'conv_dgrad_s2_pair', b_pair,
             lambda dy1, dyd, wd1, wdd, l=l: H.conv_dgrad_s2_pair(dy1, wd1, dyd, wdd, l), rows=iso('dy1 dyd', rows, l // 2))

    # ---- Winograd F(2,3) / F(4,3): 1, 2, 3 outputs in the last quad, both K steps, half-tile tails ------------------------------
    def wino_rows(points, ci, co, l, rows, setup=None, tag=''):
        name = 'f%d3_c%d_n%d_l%d_r%d%s' % (2 if points == 4 else 4, ci, co, l, rows, tag)

        def b_f(r):
            w = r.n(co, ci, 3) * 0.1
            return dict(x=r.n(rows, l, ci), u=H.wino_weights(w, points=points), out=zeros(rows, l, co))
        case('wino_fwd_' + name, 'winograd', 'conv3_winograd', b_f,
             lambda x, u, out: H.conv3_winograd(x, u, out=out), dests=('out',), rows=iso('x', rows, l), setup=setup)

        def b_d(r):
            w = r.n(co, ci, 3) * 0.1
            return dict(dy=r.n(rows, l, co), u=H.wino_weights(w, transpose=True, points=points), base=r.n(rows, l, ci))
        case('wino_dgrad_acc_' + name, 'winograd', 'conv3_winograd', b_d,
             lambda dy, u, base: (H.conv3_winograd(dy, u), H.conv3_winograd(dy, u, out=base, accumulate=True)),
             rows=iso('dy base', rows, l), setup=setup)

    for l in (1, 2, 3, 5, 6, 7, 57):
        wino_rows(4, 32, 64, l, 7)
        wino_rows(6, 32, 32, l, 7, setup=lambda: wino4_ksteps(16), tag='_k16')
        wino_rows(6, 64, 32, l, 9, setup=lambda: wino4_ksteps(32), tag='_k32')
    wino_rows(4, 64, 64, 56, 300)                               # the last round runs as half tiles
    wino_rows(4, 64, 64, 56, 300, setup=lambda: wino_half_tiles(False), tag='_nohalf')
    wino_rows(6, 512, 512, 7, 300, setup=lambda: wino4_ksteps(16), tag='_k16')
    wino_rows(6, 512, 512, 7, 300, setup=lambda: wino4_ksteps(32), tag='_k32')
    wino_rows(6, 96, 64, 6, 1040, setup=lambda: wino4_ksteps(16), tag='_k16')

    def b_wt(r):
        return dict(w=r.n(64, 32, 3))
    case('wino_weights_all', 'pack', 'wino_weights pack_conv3_bf16 repack_weight', b_wt,
         lambda w: (H.wino_weights(w), H.wino_weights(w, True), H.wino_weights(w, points=6), H.wino_weights(w, True, 6),
                    H.pack_conv3_bf16(w), H.repack_weight(w, True, True)))

    for rows, l, R in ((40, 56, 20), (40, 7, 20), (60, 28, 20)):
        def b_drop(r, rows=rows, l=l):
            return dict(x=r.n(rows, l, 64), u=H.wino_weights(r.n(32, 64, 3) * 0.1), out=zeros(rows, l, 32),
                        seed=torch.tensor([99], dtype=torch.int64, device='cuda'))
        case('wino_drop_l%d_r%d' % (l, rows), 'winograd', 'conv3_winograd', b_drop,
             lambda x, u, out, seed: H.conv3_winograd(x, u, out=out, drop=(seed, 4, 0.2)), dests=('out',), rows=iso('x', rows, l))
        case('wino_stats_l%d_r%d' % (l, rows), 'winograd', 'conv3_winograd', b_drop,
             lambda x, u, out, seed, R=R: H.conv3_winograd(x, u, out=out, drop=(seed, 4, 0.2), stats_R=R), dests=('out',),
             rows=iso('x', rows, l, axis={'[1]': None}),
             note='records: every float of da_stat_records_floats is compared (include/deepards_hip.h "Statistics records"); '
                  'check 4: out row by row; the records are per output pair in an opaque layout, not a row-indexed result')

    # ---- the dense block: statistics slices, conv1x1_bn (+ pool, records, pending records), the growth conv, bn_bwd_ss ---------
    for rows, l, c, n, pool in ((40, 56, 96, 128, False), (60, 28, 128, 64, True), (40, 7, 96, 128, False)):
        R, cb = 20, 160

        def b_c1(r, rows=rows, l=l, c=c, n=n, pool=pool):
            x = r.n(rows, l, cb)
            xv = x[:, :, :c]
            tab = zeros(2, rows // R, cb)
            H.bn_stats_fused(xv, R, tab[0][:, :c], tab[1][:, :c])
            lo = l // 2 if pool else l
            return dict(xv=xv, w=r.n(n, c, 1) * 0.1, mean=tab[0][:, :c], invstd=tab[1][:, :c], gamma=r.u(c), beta=r.n(c) * 0.3,
                        out=zeros(rows, lo, n + 32)[:, :, :n])
        case('conv1x1_bn_l%d_c%d%s' % (l, c, '_pool' if pool else ''), 'dense', 'conv1x1_bn', b_c1,
             lambda xv, w, mean, invstd, gamma, beta, out, pool=pool: H.conv1x1_bn(xv, w, R, mean, invstd, gamma, beta, out, pool=pool,
                                                                                  want_records=True),
             dests=('out',), rows=iso('xv', rows, l, R=R, axis={'[1]': None}),
             note='operands are channel slices: the guard covers the channels beside them; check 4: out per window of R rows '
                  '(the statistics tables are operands here); the records are per tile, not a row-indexed result')

        def b_ss(r, rows=rows, l=l, c=c):
            x = r.n(rows, l, cb)
            xv = x[:, :, :c]
            return dict(xv=xv, mean=zeros(rows // R, cb)[:, :c], invstd=zeros(rows // R, cb)[:, :c], gamma=r.u(c), beta=r.n(c) * 0.3)
        case('bn_stats_fused_relu_ss_l%d_c%d' % (l, c), 'dense', 'bn_stats_fused bn_relu_ss', b_ss,
             lambda xv, mean, invstd, gamma, beta: (H.bn_stats_fused(xv, R, mean, invstd), mean, invstd,
                                                    H.bn_relu_ss(xv, R, mean, invstd, gamma, beta))[1:],
             dests=('mean', 'invstd'), rows=iso('xv', rows, l, R=R))

        for relu, half, with_add in ((1, False, True), (0, False, False), (2, False, False), (1, True, False)):
            if half and l % 2:
                continue

            def b_bss(r, rows=rows, l=l, c=c, relu=relu, half=half, with_add=with_add):
                xv = r.n(rows, l, cb)[:, :, :c]
                tab = zeros(2, rows // R, cb)
                mean, invstd = tab[0][:, :c], tab[1][:, :c]
                H.bn_stats_fused(xv, R, mean, invstd)
                gamma, beta = r.u(c), r.n(c) * 0.3
                d = dict(dout=r.n(rows, l // 2 if half else l, cb)[:, :, :c], xv=xv, mean=mean, invstd=invstd, gamma=gamma, beta=beta,
                         dx=zeros(rows, l, cb)[:, :, :c], seed=torch.tensor([5], dtype=torch.int64, device='cuda'),
                         add=r.n(rows, l, cb)[:, :, :c] if with_add else None, out=None, hout=None)
                if relu == 2:
                    d['out'] = H.bn_relu_ss(xv, R, mean, invstd, gamma, beta)
                if relu == 1:
                    d['hout'] = zeros(rows, l, c)
                return d
            case('bn_bwd_ss_l%d_c%d_relu%d%s%s' % (l, c, relu, '_half' if half else '', '_add' if with_add else ''), 'dense',
                 'bn_bwd_ss', b_bss,
                 lambda dout, xv, mean, invstd, gamma, beta, dx, seed, add, out, hout, relu=relu, half=half:
                 (H.bn_bwd_ss(dout, xv, R, mean, invstd, gamma, beta, relu, dx, add=add, half_dout=half,
                              drop=(seed, 3, 0.2, 32) if relu else None, out=out, hout=hout), dx, hout),
                 dests=('dx', 'hout') if relu == 1 else ('dx',),
                 rows=iso('dout xv add out' if (with_add and relu == 2) else 'dout xv add' if with_add else 'dout xv out' if relu == 2
                          else 'dout xv', rows, l, R=R, axis={'[0]': 1}))

    for rows, l, drop in ((40, 56, 0.2), (60, 28, 0.0), (40, 7, 0.2)):
        R = 20

        def b_grow(r, rows=rows, l=l):
            c0, mid, g, cb = 64, 128, 32, 128
            x0 = r.n(rows, l, cb)[:, :, :c0]
            tab = zeros(2, rows // R, cb)
            H.bn_stats_fused(x0, R, tab[0][:, :c0], tab[1][:, :c0])
            y1 = zeros(rows, l, mid)
            _, rec1 = H.conv1x1_bn(x0, r.n(mid, c0, 1) * 0.1, R, tab[0][:, :c0], tab[1][:, :c0], r.u(c0), r.n(c0) * 0.3, y1,
                                   want_records=True)
            return dict(y1=y1, u=H.wino_weights(r.n(g, mid, 3) * 0.08), rec=rec1, mean=zeros(rows // R, mid), invstd=zeros(rows // R, mid),
                        gamma=r.u(mid), beta=r.n(mid) * 0.3, out=zeros(rows, l, cb)[:, :, c0:c0 + g],
                        seed=torch.tensor([99], dtype=torch.int64, device='cuda'))
        case('conv3_winograd_bn_l%d_r%d' % (l, rows), 'dense', 'conv3_winograd_bn', b_grow,
             lambda y1, u, rec, mean, invstd, gamma, beta, out, seed, drop=drop:
             (H.conv3_winograd_bn(y1, u, R, rec, mean, invstd, gamma, beta, out, drop=(seed, 4, drop) if drop else None,
                                  want_records=True), mean, invstd),
             dests=('out', 'mean', 'invstd'), rows=iso('y1', rows, l, R=R, axis={'[0][1]': None}),
             note='check 4: out and the published mean / invstd per window (the statistics come from rec, which stays clean); the '
                  'records of the output are per tile, not a row-indexed result')

        def b_pend(r, rows=rows, l=l):
            c0, g, cb = 64, 32, 128
            buf = r.n(rows, l, cb)
            tab = zeros(2, rows // R, cb)
            H.bn_stats_fused(buf[:, :, :c0], R, tab[0][:, :c0], tab[1][:, :c0])
            _, rec = H.conv3_winograd(r.n(rows, l, 64), H.wino_weights(r.n(g, 64, 3) * 0.1), out=buf[:, :, c0:c0 + g], stats_R=R)
            c = c0 + g
            return dict(xv=buf[:, :, :c], w=r.n(128, c, 1) * 0.1, mean=tab[0][:, :c], invstd=tab[1][:, :c], gamma=r.u(c), beta=r.n(c) * 0.3,
                        out=zeros(rows, l, 128), rec=rec)
        pl = (l + 1) // 2
        case('conv1x1_bn_pend_l%d_r%d' % (l, rows), 'dense', 'conv1x1_bn', b_pend,
             lambda xv, w, mean, invstd, gamma, beta, out, rec, rows=rows, pl=pl:
             (H.conv1x1_bn(xv, w, R, mean, invstd, gamma, beta, out, pend=(rec, 64, rows * pl, R * pl)), mean, invstd),
             dests=('out',), rows=iso('xv', rows, l, R=R),
             note='publishes the statistics of the pending channels into the tables (in place); check 4: out and both tables per '
                  'window (the pending statistics come from rec, which stays clean)')

    # ---- weight gradients: more jobs than one table holds, the chained reduce, the reduce launch, the step tail ---------------
    WG = [(64, 64, 3, 1, 1, 56, 40), (64, 128, 3, 2, 1, 56, 40), (64, 128, 1, 2, 0, 56, 40), (128, 128, 3, 1, 1, 28, 23),
          (96, 128, 1, 1, 0, 56, 20), (128, 32, 3, 1, 1, 28, 20), (64, 64, 3, 1, 1, 56, 1), (128, 32, 3, 1, 1, 9, 5),
          (512, 512, 3, 1, 1, 7, 40), (64, 64, 3, 1, 1, 57, 9), (32, 128, 3, 1, 1, 1, 7), (128, 32, 1, 1, 0, 2, 1)]

    def wg_jobs(r, cases):
        jobs, dws = [], []
        for ci, co, k, stride, pad, l, rows in cases:
            lo = H.conv_out_len(l, k, stride, pad)
            jobs.append((r.n(rows, lo, co), r.n(rows, l, ci), k, stride, pad))
            dws.append(zeros(co, ci, k))
        return jobs, dws

    def run_wgrad_multi(jobs, dws, chained):
        if chained:
            slabs, reduced = H.conv_wgrad_multi(jobs, dws=dws, accumulate=False)
            H.wgrad_reduce_multi([(s, d) for s, d, red in zip(slabs, dws, reduced) if not red], accumulate=False)
        else:
            H.wgrad_reduce_multi(list(zip(H.conv_wgrad_multi(jobs), dws)), accumulate=False)
        return dws

    for tag, cases_, setup in (('mixed_30_jobs', WG * 2 + WG[:6], None), ('direct_only_30_jobs', WG * 2 + WG[:6], 'nowino'),
                               ('f43_and_f23', [WG[8]] * 2 + [WG[0]] * 17 + WG[1:6], None),
                               ('resnet18_b64', [(c, c, 3, 1, 1, l, 1280) for c, l in [(256, 14)] * 3 + [(128, 28)] * 3 + [(64, 56)] * 4],
                                None)):
        for chained in (False, True):
            def b_wgm(r, cases_=cases_):
                jobs, dws = wg_jobs(r, cases_)
                return dict(jobs=jobs, dws=dws)
            case('conv_wgrad_multi_%s%s' % (tag, '_chained' if chained else ''), 'wgrad',
                 'conv_wgrad_multi wgrad_reduce_multi', b_wgm,
                 lambda jobs, dws, chained=chained: run_wgrad_multi(jobs, dws, chained),
                 dests=('dws',), setup=direct_only if setup else None,
                 note='weight gradients reduce over rows: exempt from check 4; dws are the dirty destinations of check 3')

    def b_x3w(r):
        return dict(dy=H.x3_split(r.n(40, 28, 128)), xs=H.x3_split(r.n(40, 28, 128)), x=H.x3_split(r.n(40, 28, 64)),
                    dy2=H.x3_split(r.n(40, 14, 128)), dws=[zeros(128, 128, 3), zeros(128, 64, 3), zeros(128, 64, 1)])
    case('conv_wgrad_multi_x3', 'wgrad', 'conv_wgrad_multi wgrad_reduce_multi', b_x3w,
         lambda dy, xs, x, dy2, dws: run_wgrad_multi([(dy, xs, 3, 1, 1), (dy2, x, 3, 2, 1), (dy2, x, 1, 2, 0)], dws, False),
         dests=('dws',), note='x3 operands: the k3 s1 p1 job and the two jobs of a stride-2 block entry')

    def b_tail(r, n_red, n_bn, with_stem):
        red, dws = [], []
        for i in range(n_red):
            co, ci, k, splits = (64, 32, 3, 5) if i % 2 else (32, 64, 1, 9)
            red.append((r.n(splits * k * co * ci), splits, k, co, ci))
            dws.append(zeros(co, ci, k))
        pg, run = [], []
        for i in range(n_bn):
            c, w = (64, 7) if i % 2 else (96, 64)
            pg.append((r.n(2, w, c), zeros(c), zeros(c)))
            run.append((r.n(w, c), r.u(w, c), 140, r.n(c), r.u(c), torch.zeros((), dtype=torch.int64, device='cuda'), 0.1, 1e-5))
        stem = (r.n(40, 448), 40, 448, zeros(64, 1, 7)) if with_stem else None
        return dict(red=red, dws=dws, pg=pg, run=run, stem=stem)

    def run_tail(red, dws, pg, run, stem):
        H.step_tail_multi(list(zip(red, dws)), pg, run, accumulate=False, stem=stem)
        return (dws, [(g, b) for _, g, b in pg], [(t[3], t[4], t[5]) for t in run], stem[3] if stem is not None else None)
    for n_red, n_bn, with_stem in ((3, 4, True), (33, 4, True), (3, 25, False), (0, 3, True)):
        case('step_tail_multi_%d_%d_%d' % (n_red, n_bn, with_stem), 'tail',
             'step_tail_multi',
             lambda r, a=n_red, b=n_bn, c=with_stem: b_tail(r, a, b, c), run_tail, dests=('dws',),
             note='33 reductions / 25 BatchNorms / no reductions: the fallback counts')

    def b_rep(r):
        return dict(ws=[r.n(64, 32, 3), r.n(128, 64, 3), r.n(512, 512, 3), r.n(128, 64, 3), r.n(128, 64, 1), r.n(64, 64, 3), r.n(128, 64, 1)] +
                    [r.n(32, 32, 1) for _ in range(30)])
    def run_rep(ws):
        packs = [list(t) for t in H.repack_multi(ws, [H.WINO2, H.BF16, H.WINO4, H.X3, H.X3, H.DIRECT, H.BF16] + [H.DIRECT] * 30)]
        packs[4][2], packs[4][3] = packs[4][2][:, :, 6:12], packs[4][3][:, :, 6:12]
        return packs
    case('repack_multi_37', 'pack', 'repack_multi', b_rep, run_rep,
         note='a 1x1 weight in the chunked split-bf16 form fills tap 1 of its chunks only (include/deepards_hip.h, '
              'da_conv_x3p_s2_fwd: "1x1 weights pack with K = 1 into tap 1 of the chunks"): rows [6, 12) of the 18 are compared')

    # ---- bf16-operand and x3p forms ------------------------------------------------------------------------------------------
    for rows, l, ci, co in ((9, 57, 64, 64), (33, 2, 96, 128), (1280, 56, 64, 64)):
        def b_b16(r, rows=rows, l=l, ci=ci, co=co):
            wf, wd = H.pack_conv3_bf16(r.n(co, ci, 3) * 0.1)
            return dict(x=r.n(rows, l, ci), wf=wf, out=zeros(rows, l, co))
        case('conv3_bf16_l%d_r%d' % (l, rows), 'bf16', 'conv3_bf16', b_b16,
             lambda x, wf, out: H.conv3_bf16(x, wf, out=out), dests=('out',), rows=iso('x', rows, l))
    for rows, l in ((40, 56), (60, 7)):
        def b_b16bn(r, rows=rows, l=l):
            p1, _ = H.pack_conv3_bf16(r.n(64, 64, 3) * 0.1)
            y1, rec = H.conv3_bf16_bn(r.n(rows, l, 64), p1, 20, want_records=True)
            return dict(y1=y1, p=p1, rec=rec, mean=zeros(rows // 20, 64), invstd=zeros(rows // 20, 64), gamma=r.u(64), beta=r.n(64) * 0.3)
        case('conv3_bf16_bn_l%d_r%d' % (l, rows), 'bf16', 'conv3_bf16_bn', b_b16bn,
             lambda y1, p, rec, mean, invstd, gamma, beta: (H.conv3_bf16_bn(y1, p, 20, rec=rec, mean=mean, invstd=invstd, gamma=gamma,
                                                                              beta=beta, want_records=True), mean, invstd),
             dests=('mean', 'invstd'), rows=iso('y1', rows, l, R=20, axis={'[0][1]': None}),
             note='check 4: out and the published mean / invstd per window (the statistics come from rec, which stays clean); the '
                  'records of the output are per tile, not a row-indexed result')
    for rows, l in ((5, 56), (300, 14)):
        def b_bs2(r, rows=rows, l=l):
            (_, _, f1, d1), (_, _, fd, dd) = H.repack_multi([r.n(128, 64, 3) * 0.1, r.n(128, 64, 1) * 0.1], [H.BF16, H.BF16])
            return dict(x=r.n(rows, l, 64), f1=f1, fd=fd, d1=d1, dd=dd, dy1=r.n(rows, l // 2, 128), dyd=r.n(rows, l // 2, 128),
                        o1=zeros(rows, l, 64), od=zeros(rows, l, 64))
        case('conv_bf16_s2_l%d_r%d' % (l, rows), 'bf16', 'conv_fwd_bf16_s2 conv_dgrad_bf16_s2 conv_dgrad_bf16_s2_pair', b_bs2,
             lambda x, f1, fd, d1, dd, dy1, dyd, o1, od, l=l:
             (H.conv_fwd_bf16_s2(x, f1, fd), H.conv_fwd_bf16_s2(x, f1), H.conv_dgrad_bf16_s2(dy1, d1, l, out=o1),
              H.conv_dgrad_bf16_s2(dyd, dd, l, out=od), H.conv_dgrad_bf16_s2(dyd, dd, l), H.conv_dgrad_bf16_s2_pair(dy1, d1, dyd, dd, l)),
             dests=('o1', 'od'), rows=iso('x dy1 dyd', rows, l // 2))
    for rows, l, ci, co in ((37, 7, 128, 64), (3, 1, 64, 128), (1281, 14, 64, 64)):
        def b_x3(r, rows=rows, l=l, ci=ci, co=co):
            (_, _, uf, ud), = H.repack_multi([r.n(co, ci, 3) * 0.1], [H.X3])
            return dict(x=r.n(rows, l, ci), uf=uf, out=zeros(rows, l, co))
        case('conv3_x3p_l%d_r%d' % (l, rows), 'x3p', 'conv3_x3p x3_split x3_merge', b_x3,
             lambda x, uf, out: (H.conv3_x3p(H.x3_split(x), uf, out=out), H.conv3_x3p(H.x3_split(x), uf),
                                 H.x3_merge(H.x3_split(x))), dests=('out',), rows=iso('x', rows, l))
    for rows, l in ((5, 56), (300, 14)):
        def b_x3s2(r, rows=rows, l=l):
            return dict(x=r.n(rows, l, 64), w1=r.n(128, 64, 3) * 0.1, wd=r.n(128, 64, 1) * 0.1, dy1=r.n(rows, l // 2, 128),
                        dyd=r.n(rows, l // 2, 128), out=zeros(rows, l, 64))

        def run_x3s2(x, w1, wd, dy1, dyd, out):
            (_, _, f1, d1), (_, _, fd, dd) = H.repack_multi([w1, wd], [H.X3, H.X3])
            return (H.conv_x3p_s2_fwd(H.x3_split(x), f1, fd), H.conv_x3p_s2_dgrad(H.x3_split(dy1), d1, H.x3_split(dyd), dd, out=out))
        case('conv_x3p_s2_l%d_r%d' % (l, rows), 'x3p', 'conv_x3p_s2_fwd conv_x3p_s2_dgrad repack_multi x3_split', b_x3s2, run_x3s2,
             dests=('out',), rows=iso('x dy1 dyd', rows, l // 2),
             note='the packs are made inside the call: under check 1 the 1x1 pack keeps the pattern outside tap 1 of its chunks '
                  '(repack_multi_37), which the kernels must never stage')

    # ---- BatchNorm: single pass, forced two-stage, 8-channel blocks; C in {32, 96, 512}, W in {1, 5, 64} ----------------------
    def bn_rows(c, l, R, w, setup=None, tag=''):
        rows = R * w
        name = 'c%d_l%d_w%d%s' % (c, l, w, tag)
        fam = 'bn'

        def b_f(r):
            return dict(x=r.n(rows, l, c) * 2 + 0.3, res=r.n(rows, l, c), gamma=r.u(c), beta=r.n(c) * 0.3, out=zeros(rows, l, c))
        case('bn_fwd_' + name, fam, 'bn_fwd', b_f,
             lambda x, res, gamma, beta, out: (H.bn_fwd(x, R, gamma, beta, relu=True, res=res, out=out, want_mask=True),
                                               H.bn_fwd(x, R, gamma, beta, relu=False)),
             dests=('out',), rows=iso('x res', rows, l, R=R, axis={'[0][3]': None}), setup=setup,
             note='the mask is one word per thread of the window blocks: not a row-indexed result')
        case('bn_stats_apply_' + name, fam, 'bn_stats bn_stats_partial bn_apply bn_running_multi',
             lambda r: dict(b_f(r), rm=r.n(c), rv=r.u(c), nbt=torch.zeros((), dtype=torch.int64, device='cuda'),
                            mean=zeros(w, c), invstd=zeros(w, c)),
             lambda x, res, gamma, beta, out, rm, rv, nbt, mean, invstd:
             (H.bn_stats(x, R, running_mean=rm, running_var=rv, num_batches_tracked=nbt), rm, rv, nbt,
              H.bn_apply(x, R, mean, invstd, gamma, beta, res=res, out=out, part=H.bn_stats_partial(x, R)), mean, invstd),
             dests=('out', 'mean', 'invstd'), setup=setup,
             rows=iso('x res', rows, l, R=R, axis={'[1]': None, '[2]': None, '[3]': None}),
             note='check 4: statistics and out per window; the running buffers fold every window: exempt')

        def b_b(r):
            d = b_f(r)
            with (setup() if setup else contextlib.nullcontext()):
                out, mean, invstd, mask = H.bn_fwd(d['x'], R, d['gamma'], d['beta'], relu=True, res=d['res'], want_mask=True)
            return dict(dout=r.n(rows, l, c), x=d['x'], mean=mean, invstd=invstd, gamma=d['gamma'], beta=d['beta'], out=out, mask=mask,
                        dx=zeros(rows, l, c), dg=zeros(c), db=zeros(c), add=r.n(rows, l, c + 32))

        def run_b(dout, x, mean, invstd, gamma, beta, out, mask, dx, dg, db, add):
            res = [H.bn_bwd(dout, x, R, mean, invstd, gamma, beta, m, out=out, want_g=True, dx=dx.clone() if m else dx, dgamma=dg.clone(),
                            dbeta=db.clone()) for m in (0, 1, 2)]
            res.append(H.bn_bwd(dout, x, R, mean, invstd, gamma, beta, 2, out=out, add=(add, 32), defer_param_grads=True))
            if mask is not None:
                res.append(H.bn_bwd(dout, x, R, mean, invstd, gamma, beta, 2, mask=mask, want_g=True, defer_param_grads=True))
            ip = dout.clone()
            res.append(H.bn_bwd(ip, x, R, mean, invstd, gamma, beta, 1, out=out, dx=ip))          # in place: dx is dout
            return res
        axis = {}
        for i in range(6):
            axis.update({'[%d][1]' % i: None, '[%d][2]' % i: None, '[%d][4]' % i: 1})
        case('bn_bwd_' + name, fam, 'bn_bwd', b_b, run_b, dests=('dx',), setup=setup,
             rows=iso('dout x out add', rows, l, R=R, axis=axis), note='dgamma / dbeta reduce over windows: exempt; ds is (2, W, C)')

    for c in (32, 96, 512):
        for w in (1, 5, 64):
            bn_rows(c, 7, 20, w)
    bn_rows(64, 56, 20, 5)
    bn_rows(64, 112, 20, 3, tag='_long')                        # Wn = 2240: the two-stage kernels by geometry
    bn_rows(96, 28, 20, 5, setup=bn_two_stage, tag='_twostage')
    bn_rows(512, 7, 20, 64, setup=bn_two_stage, tag='_twostage')
    bn_rows(32, 7, 20, 1, setup=bn_two_stage, tag='_twostage')
    bn_rows(96, 28, 20, 5, setup=bn_blocks8, tag='_blocks8')
    bn_rows(512, 7, 20, 5, setup=bn_blocks8, tag='_blocks8')

    for c, l, w in ((128, 28, 64), (512, 7, 5), (64, 56, 2)):
        R = 20
        rows = R * w

        def b_pair(r, c=c, l=l, rows=rows):
            mk = lambda: r.n(rows, l, c)
            y1, yd, y2 = mk(), mk(), mk()
            g = [r.u(c) for _ in range(6)]
            (res, md, idd, _), (h1, m1, i1, _) = H.bn_fwd_pair([(yd, g[0], g[1], False, None, False), (y1, g[2], g[3], True, None, False)], R)
            out, m2, i2, mask = H.bn_fwd(y2, R, g[4], g[5], relu=True, res=res, want_mask=True)
            return dict(y1=y1, yd=yd, y2=y2, g=g, res=res, md=md, idd=idd, m2=m2, i2=i2, mask=mask, dout=mk(), dout2=mk(),
                        dxa=zeros(rows, l, c), dxb=zeros(rows, l, c), dxt=zeros(rows, l, c))
        case('bn_pair_two_c%d_l%d_w%d' % (c, l, w), 'bn', 'bn_fwd_pair bn_bwd_pair bn_bwd_two', b_pair,
             lambda y1, yd, y2, g, res, md, idd, m2, i2, mask, dout, dout2, dxa, dxb, dxt:
             (H.bn_fwd_pair([(yd, g[0], g[1], False, None, False), (y1, g[2], g[3], True, yd, True)], R),
              H.bn_bwd_pair(dout, [(y2, m2, i2, g[4], g[5], dxa), (yd, md, idd, g[0], g[1], dxb)], R, mask),
              H.bn_bwd_pair(dout, [(y2, m2, i2, g[4], g[5], None), (yd, md, idd, g[0], g[1], None)], R, mask, dout2=dout2),
              H.bn_bwd_two(dout, dout2, y2, R, m2, i2, g[4], g[5], mask, want_g=True, dx=dxt)),
             dests=('dxa', 'dxb', 'dxt'),
             rows=iso('y1 yd y2 dout dout2', rows, l, R=R,
                      axis={'[0][0][3]': None, '[0][1][3]': None, '[1][0][1]': 1, '[1][1][1]': 1, '[2][0][1]': 1, '[2][1][1]': 1,
                            '[3][2]': 1}))

    for c, l, w in ((512, 7, 5), (64, 7, 64), (96, 7, 1)):
        R = 20
        rows = R * w

        def b_pool(r, c=c, l=l, rows=rows):
            x, res, gamma, beta = r.n(rows, l, c), r.n(rows, l, c), r.u(c), r.n(c) * 0.3
            flat, mean, invstd, mask = H.bn_fwd_pool(x, R, gamma, beta, res=res)
            return dict(x=x, res=res, gamma=gamma, beta=beta, mean=mean, invstd=invstd, mask=mask, dflat=r.n(rows, c), dx=zeros(rows, l, c))
        case('bn_pool_c%d_w%d' % (c, w), 'bn', 'bn_fwd_pool bn_bwd_pool', b_pool,
             lambda x, res, gamma, beta, mean, invstd, mask, dflat, dx:
             (H.bn_fwd_pool(x, R, gamma, beta, res=res), H.bn_bwd_pool(dflat, x, R, mean, invstd, gamma, beta, mask, want_g=True, dx=dx)),
             dests=('dx',), rows=iso('x res dflat', rows, l, R=R, axis={'[0][3]': None, '[1][2]': 1}))

    for c, l, w in ((64, 56, 3), (512, 7, 5)):
        R = 20
        rows = R * w

        def b_x(r, c=c, l=l, rows=rows):
            x, res, gamma, beta = r.n(rows, l, c), r.n(rows, l, c), r.u(c), r.n(c) * 0.3
            out, mean, invstd, mask = H.bn_fwd(x, R, gamma, beta, relu=True, res=res, want_mask=True)
            return dict(x=x, res=res, res3=H.x3_split(res), gamma=gamma, beta=beta, mean=mean, invstd=invstd, mask=mask, dout=r.n(rows, l, c))
        case('bn_x3_c%d_l%d' % (c, l), 'bn', 'bn_fwd_x bn_bwd_x', b_x,
             lambda x, res, res3, gamma, beta, mean, invstd, mask, dout:
             (H.bn_fwd_x(x, R, gamma, beta, relu=True, res=res3, want_mask=True, out_x3=True),
              H.bn_fwd_x(x, R, gamma, beta, relu=False, res=res, out_x3=False),
              H.bn_bwd_x(dout, x, R, mean, invstd, gamma, beta, 3, want_g=True, mask=mask, dx_x3=True),
              H.bn_bwd_x(dout, x, R, mean, invstd, gamma, beta, 0, dx_x3=False)),
             rows=iso('x res res3 dout', rows, l, R=R, axis={'[0][3]': None, '[2][2]': 1, '[3][2]': 1}))

    def b_pg(r):
        return dict(ds=[r.n(2, w, c) for w, c in [(7, 64), (64, 96)] * 17], dg=[zeros(c) for _, c in [(7, 64), (64, 96)] * 17],
                    db=[zeros(c) for _, c in [(7, 64), (64, 96)] * 17])
    case('bn_param_grad_multi_34', 'bn', 'bn_param_grad_multi', b_pg,
         lambda ds, dg, db: (H.bn_param_grad_multi(list(zip(ds, dg, db)), accumulate=False), dg, db)[1:], dests=('dg', 'db'))

    def b_run(r):
        return dict(items=[(r.n(w, c), r.u(w, c), 140, r.n(c), r.u(c), torch.zeros((), dtype=torch.int64, device='cuda'), 0.1, 1e-5)
                           for w, c in [(7, 64), (64, 96), (1, 32)] * 12])
    case('bn_running_multi_36', 'bn', 'bn_running_multi', b_run,
         lambda items: (H.bn_running_multi(items), [(t[3], t[4], t[5]) for t in items])[1], note='in place: checks 2 and 5 are the ones that bite')

    # ---- bf16 storage: one conv and one BatchNorm ---------------------------------------------------------------------------
    def b_s16(r):
        p1, _ = H.pack_conv3_bf16(r.n(64, 64, 3) * 0.1)
        return dict(x=r.n(40, 28, 64).bfloat16(), p=p1, res=r.n(40, 28, 64).bfloat16(), gamma=r.u(64), beta=r.n(64) * 0.3,
                    dout=r.n(40, 28, 64).bfloat16())

    def run_s16(x, p, res, gamma, beta, dout):
        y = H.conv3_bf16(x, p)
        out, mean, invstd, mask = H.bn_fwd(y, 20, gamma, beta, relu=True, res=res, want_mask=True)
        return y, out, mean, invstd, mask, H.bn_bwd(dout, y, 20, mean, invstd, gamma, beta, 2, mask=mask, want_g=True, defer_param_grads=True)
    case('bf16_storage_conv_bn', 'bf16', 'conv3_bf16 bn_fwd bn_bwd', b_s16, run_s16, setup=bf16_storage,
         rows=iso('x res dout', 40, 28, R=20, axis={'[4]': None, '[5][1]': None, '[5][2]': None, '[5][4]': 1}))

    # ---- stem, pools ---------------------------------------------------------------------------------------------------------
    for rows, lin, c0 in ((40, 224, 64), (5, 14, 32)):
        def b_stem(r, rows=rows, lin=lin, c0=c0):
            return dict(x=r.n(rows, lin), w=r.n(c0, 1, 7) * 0.2, dy=r.n(rows, lin // 2, c0), out=zeros(c0, 1, 7))
        case('stem_conv_l%d_c%d' % (lin, c0), 'stem', 'stem_conv_fwd stem_conv_wgrad', b_stem,
             lambda x, w, dy, out: (H.stem_conv_fwd(x, w), H.stem_conv_wgrad(dy, x, out=out), H.stem_conv_wgrad(dy, x)),
             dests=('out',), rows=iso('x dy', rows, lin // 2, axis={'[1]': None, '[2]': None}))

    def b_stem3(r):
        return dict(x=r.n(20, 3, 224), w=r.n(64, 3, 7) * 0.2, x1=r.n(20, 1, 56), w1=r.n(32, 1, 3))
    case('stem_conv_other_shapes', 'stem', 'stem_conv_fwd', b_stem3,
         lambda x, w, x1, w1: (H.stem_conv_fwd(x, w), H.stem_conv_fwd(x1, w1, stride=1)), rows=iso('x x1', 20, 112))

    for rows, R, lin, c, mode in ((40, 20, 224, 64, 0), (40, 20, 224, 64, 1), (80, 40, 512, 64, 0), (60, 20, 224, 128, 1), (12, 4, 30, 32, 0)):
        def b_sf(r, rows=rows, R=R, lin=lin, c=c, mode=mode):
            x, w, gamma, beta = r.n(rows, lin), r.n(c, 1, 7) * 0.2, r.u(c), r.n(c) * 0.3
            lp = (lin // 2 - 1) // 2 + 1
            assert H.stem_fused_ok(x, w, R), 'the fused stem refuses %s' % ((rows, R, lin, c),)
            _, mean, invstd = H.stem_fused_fwd(x, w, R, gamma, beta, mode)
            return dict(x=x, w=w, gamma=gamma, beta=beta, mean=mean, invstd=invstd, dout=r.n(rows, lp, c), out=zeros(rows, lp, c),
                        dw=zeros(c, 1, 7))
        case('stem_fused_%d_%d_%d_c%d_pool%d' % (rows, R, lin, c, mode), 'stem', 'stem_fused_fwd stem_fused_bwd', b_sf,
             lambda x, w, gamma, beta, mean, invstd, dout, out, dw, R=R, mode=mode:
             (H.stem_fused_fwd(x, w, R, gamma, beta, mode, out=out), H.stem_fused_fwd(x, w, R, gamma, beta, mode, out_x3=True),
              H.stem_fused_bwd(dout, x, w, R, mean, invstd, gamma, beta, mode, dw=dw)),
             dests=('out', 'dw'), rows=iso('x dout', rows, lin // 4, R=R, axis={'[2][0]': None, '[2][1]': 1}),
             note='(80, 40, 512): the shape of nb 40 x L 512 the fused stem still takes')

        def b_pool(r, rows=rows, R=R, lin=lin, c=c):
            lc = lin // 2
            y = r.n(rows, lc, c)
            mean, invstd = H.bn_stats(y, R)
            return dict(y=y, mean=mean, invstd=invstd, gamma=r.u(c), beta=r.n(c) * 0.3, dout=r.n(rows, (lc - 1) // 2 + 1, c),
                        out=zeros(rows, (lc - 1) // 2 + 1, c + 32)[:, :, :c])
        case('bn_relu_pool_%d_%d_c%d_pool%d' % (rows, lin, c, mode), 'pool', 'bn_relu_pool_fwd pool_bwd', b_pool,
             lambda y, mean, invstd, gamma, beta, dout, out, R=R, mode=mode:
             (H.bn_relu_pool_fwd(y, R, mean, invstd, gamma, beta, mode), H.bn_relu_pool_fwd(y, R, mean, invstd, gamma, beta, mode, out=out),
              H.bn_relu_pool_fwd(y, R, mean, invstd, gamma, beta, mode, out_x3=True), H.pool_bwd(dout, y, R, mean, invstd, gamma, beta, mode)),
             dests=('out',), rows=iso('y dout', rows, lin // 2))

    for rows, l, c in ((40, 7, 512), (3, 1, 32), (1280, 14, 96)):
        def b_ap(r, rows=rows, l=l, c=c):
            return dict(x=r.n(rows, l, c), dfeat=r.n(rows, c), x2=r.n(rows, 2 * l, c), dout=r.n(rows, l, c),
                        dslide=r.n(rows, c * (l - (l + 1) // 2 + 1)))
        k = (l + 1) // 2
        case('avgpools_l%d_c%d_r%d' % (l, c, rows), 'pool',
             'global_avgpool_fwd global_avgpool_bwd avgpool_fwd avgpool_bwd avgpool_slide_fwd avgpool_slide_bwd', b_ap,
             lambda x, dfeat, x2, dout, dslide, l=l, c=c, k=k:
             (H.global_avgpool_fwd(x), H.global_avgpool_bwd(dfeat, l), H.avgpool_fwd(x2, 2), H.avgpool_bwd(dout, 2 * l, 2),
              H.avgpool_slide_fwd(x, k), H.avgpool_slide_bwd(dslide, l, k, c)), rows=iso('x dfeat x2 dout dslide', rows, l))

    # ---- head, loss, optimisers ----------------------------------------------------------------------------------------------
    for b, R, l, f in ((4, 20, 7, 512), (1, 20, 1, 64), (64, 20, 7, 512)):
        def b_head(r, b=b, R=R, l=l, f=f):
            t = zeros(b, 2)
            t[: (b + 1) // 2, 0] = 1
            t[(b + 1) // 2:, 1] = 1
            d = dict(xmap=r.n(b * R, l, f), w=r.n(2, R * f) * 0.01, bias=r.n(2) * 0.1, target=t, dw=zeros(2, R * f), dbias=zeros(2))
            d['feat'] = H.global_avgpool_fwd(d['xmap'])
            return d

        def run_head(xmap, w, bias, target, dw, dbias, feat, R=R, l=l):
            flat, part, logits, loss = H.head_fwd(xmap, w, bias, target, R, finish=False)
            bwd = H.head_bwd(part, bias, target, flat, w, logits, loss, R, l, dw=dw, dbias=dbias)
            fin = H.head_fwd(xmap, w, bias, target, R, finish=True)
            flat2, part2, logits2, loss2 = H.head_flat_fwd(feat, w, bias, target, R, finish=False)
            bwd2 = H.head_flat_bwd(part2, bias, target, flat2, w, logits2, loss2, R)
            fin2 = H.head_flat_fwd(feat, w, bias, target, R, finish=True)
            lin = H.linear2_fwd(flat, w, bias)
            return (flat, part, logits, loss, bwd, fin, flat2, part2, logits2, loss2, bwd2, fin2, lin,
                    H.linear2_bwd(lin, flat, w, dw=dw.clone(), dbias=dbias.clone()), H.linear2_bwd(lin, flat, w), H.bce_logits(lin, target))
        case('head_b%d_l%d_f%d' % (b, l, f), 'head',
             'head_fwd head_bwd head_flat_fwd head_flat_bwd linear2_fwd linear2_bwd bce_logits', b_head, run_head, dests=('dw', 'dbias'),
             note='logits / loss of a head_fwd without finish are filled by head_bwd (hip_ops.head_fwd): compared after it; '
                  'losses and dW reduce over the batch: exempt from check 4')

    for n in (1, 7, 4096 + 3, 1 << 20):
        def b_opt(r, n=n):
            return dict(p=r.n(n), g=r.n(n), buf=r.n(n), m=r.n(n) * 0.1, v=r.u(n) * 0.01, p2=r.n(n), p3=r.n(n), m3=r.n(n) * 0.1, v3=r.u(n) * 0.01,
                        step=torch.full((1,), 3, dtype=torch.int64, device='cuda'))

        def run_opt(p, g, buf, m, v, p2, p3, m3, v3, step):
            H.clamp_sgd_nesterov_(p, g, buf, 1e-3, 0.9, 1e-4, 0.01, False)
            H.clamp_adam_(p2, g, m, v, 1e-3, 4, 0.01)
            H.clamp_adam_dev_(p3, g, m3, v3, 1e-3, step, 0.01)
            return p, buf, p2, m, v, p3, m3, v3, step
        case('optimisers_n%d' % n, 'optim', 'clamp_sgd_nesterov_ clamp_adam_ clamp_adam_dev_', b_opt, run_opt,
             note='in place: checks 2 and 5 only have something to find')

    # ---- the rest ------------------------------------------------------------------------------------------------------------
    for rows, l in ((40, 56), (3, 1), (1280, 7)):
        def b_cat(r, rows=rows, l=l):
            return dict(a=r.n(rows, l, 64), b=r.n(rows, l, 32), seed=torch.tensor([7], dtype=torch.int64, device='cuda'), out=zeros(rows, l, 32),
                        out2=zeros(rows, l, 32))
        case('concat_slice_dropout_l%d_r%d' % (l, rows), 'misc', 'concat2 slice_channels dropout', b_cat,
             lambda a, b, seed, out, out2: (H.concat2(a, b), H.concat2(a, b, drop=(seed, 2, 0.2)), H.slice_channels(a, 32, 32, out=out),
                                            H.slice_channels(a, 16, 32, out=out2, drop=(seed, 2, 0.2)), H.slice_channels(a, 0, 32),
                                            H.dropout(b, seed, 2, 0.2)),
             dests=('out', 'out2'), rows=iso('a b', rows, l))

    def b_gather(r):
        idx = torch.tensor([5, 0, 11, 11, 3, 7, 1], dtype=torch.int64, device='cuda')
        return dict(tiles=r.n(12, 20, 1, 224).double(), tiles4=r.n(12, 20, 3, 224).double(), src=r.n(12, 37), idx=idx, o1=zeros(7, 20, 1, 224),
                    o2=zeros(7, 20, 3, 224), o3=zeros(7, 37))
    case('gather', 'misc', 'gather_normalize gather_rows', b_gather,
         lambda tiles, tiles4, src, idx, o1, o2, o3: (H.gather_normalize(tiles, idx, 0.25, 1.5, out=o1), H.gather_normalize(tiles, idx, 0.25, 1.5),
                                                      H.gather_normalize(tiles4, idx, (0.1, 0.2, 0.3), (1.0, 2.0, 3.0), out=o2),
                                                      H.gather_rows(src, idx, out=o3), H.gather_rows(src, idx)),
         dests=('o1', 'o2', 'o3'), note='rows are picked through idx: isolation is checked by gather_source_rows')

    def b_gather_id(r):
        return dict(tiles=r.n(9, 20, 1, 224).double(), src=r.n(9, 37))
    case('gather_source_rows', 'misc', 'gather_normalize gather_rows', b_gather_id,
         lambda tiles, src: (H.gather_normalize(tiles, torch.arange(9, device='cuda'), 0.25, 1.5), H.gather_rows(src, torch.arange(9, device='cuda'))),
         rows=iso('tiles src', 9))

    for b, nb, f in ((4, 20, 512), (1, 1, 32), (64, 64, 96)):
        def b_med(r, b=b, nb=nb, f=f):
            feat = r.n(b * nb, f)
            return dict(feat=feat, dout=r.n(b, f), idx=H.window_median_fwd(feat, nb)[1])
        case('window_median_b%d_nb%d_f%d' % (b, nb, f), 'misc', 'window_median_fwd window_median_bwd', b_med,
             lambda feat, dout, idx, nb=nb: (H.window_median_fwd(feat, nb), H.window_median_bwd(dout, idx, nb)),
             rows=dict(inputs=('feat',), R=nb, windows=b, mid=b // 2, axis={'[1]': None}),
             note='window_median_bwd scatters dout through idx: its isolation is per window of dout, not of feat')

    for b, t, h in ((4, 20, 16), (1, 1, 16), (33, 7, 32)):
        def b_lstm(r, b=b, t=t, h=h):
            gx, whh, bih, bhh, h0, c0 = r.n(b, t, 4 * h), r.n(4 * h, h) * 0.2, r.n(4 * h) * 0.1, r.n(4 * h) * 0.1, r.n(b, h), r.n(b, h)
            hs, cs, gates, _, _ = H.lstm_fwd(gx, whh, bih, bhh, h0, c0)
            return dict(gx=gx, whh=whh, bih=bih, bhh=bhh, h0=h0, c0=c0, hs=hs, cs=cs, gates=gates, dh=r.n(b, t, h))
        case('lstm_b%d_t%d_h%d' % (b, t, h), 'misc', 'lstm_fwd lstm_bwd', b_lstm,
             lambda gx, whh, bih, bhh, h0, c0, hs, cs, gates, dh: (H.lstm_fwd(gx, whh, bih, bhh, h0, c0), H.lstm_fwd(gx, whh, bih, bhh),
                                                                  H.lstm_bwd(dh, whh, hs, cs, gates, h0, c0)),
             rows=iso('gx h0 c0 hs cs gates dh', b))

    def b_red(r):
        return dict(m=r.n(33, 4 * 16, 16), out=zeros(64, 16), logits=r.n(9, 2), group=torch.tensor([0, 1, 1, 2, 0, 2, 2, 1, 0], device='cuda'),
                    votes=torch.zeros(3, 2, dtype=torch.int32, device='cuda'))
    case('reduce_rows_vote_counts', 'misc', 'reduce_rows vote_counts', b_red,
         lambda m, out, logits, group, votes: (H.reduce_rows(m, out=out), H.reduce_rows(m), H.vote_counts(logits, group, votes), votes),
         dests=('out',), note='both reduce over rows: exempt from check 4')


if H is not None:
    _table()

# Public names of hip_ops that launch no kernel: host-only queries, debug setters and predicates.
EXCLUDED = {
    'set_act_dtype': 'process-wide storage switch (exercised by the bf16_storage rows)',
    'act_dtype': 'host query',
    'conv_out_len': 'host arithmetic',
    'stat_records': 'allocates a record buffer, launches nothing',
    'is_x3': 'predicate',
    'x3_empty': 'allocation only',
    'conv_kernel_wanted': 'kernel choice, host only',
    'conv_kernel': 'kernel choice, host only',
    'step_pack_form': 'kernel choice, host only',
    'wgrad_kernel': 'kernel choice, host only',
    's2_entry_kernel': 'kernel choice, host only',
    'x3_block_ok': 'predicate',
    'bn_single_pass': 'predicate',
    'bn_x3_ok': 'predicate',
    'dense_fused_ok': 'predicate',
    'bn_two_ok': 'predicate',
    'bn_pool_ok': 'predicate',
    'bn_debug_two_stage': 'debug setter (used by the _twostage rows)',
    'stem_fused_ok': 'predicate (host geometry query)',
}


def _ids(cases):
    return [c.name for c in cases]


_SIGNATURES = {}


def _signature(case):
    if case.name not in _SIGNATURES:
        _SIGNATURES[case.name] = P.shape_signature(case)
    return _SIGNATURES[case.name]


def _other(case):
    """The next case of the table (wrapping round) whose operands have other shapes than this one's: of the same family if
    it has one, else of any family.  A forward and the data gradient of one conv, or one shape under two debug settings,
    are the SAME shape and are passed over."""
    at = CASES.index(case)
    order = CASES[at + 1:] + CASES[:at]
    for pool in ([c for c in order if c.family == case.family], order):
        for c in pool:
            if _signature(c) != _signature(case):
                return c
    raise AssertionError('%s: no case of another shape in the table' % case.name)


def test_every_kernel_launching_wrapper_has_a_row():
    public = {n for n, f in vars(H).items() if inspect.isfunction(f) and f.__module__ == H.__name__ and not n.startswith('_')}
    assert not set(EXCLUDED) - public, 'exclusions that no longer exist: %s' % sorted(set(EXCLUDED) - public)
    assert not set(COVERED) - public, 'rows for wrappers that no longer exist: %s' % sorted(set(COVERED) - public)
    assert not set(COVERED) & set(EXCLUDED)
    missing = public - set(COVERED) - set(EXCLUDED)
    assert not missing, 'public hip_ops functions without an op case or a commented exclusion: %s' % sorted(missing)
    assert len(set(_ids(CASES))) == len(CASES)
    print('%d op cases, %d wrappers, %d excluded' % (len(CASES), len(COVERED), len(EXCLUDED)))


def test_every_row_calls_the_wrappers_it_stands_for():
    """COVERED is written by hand: one clean run of every row with each public hip_ops function wrapped by a recorder shows
    that call() -- not build() -- reaches every wrapper the row is credited with."""
    public = sorted(n for n, f in vars(H).items() if inspect.isfunction(f) and f.__module__ == H.__name__ and not n.startswith('_'))
    credited = {}
    for op, names in COVERED.items():
        for name in names:
            credited.setdefault(name, set()).add(op)
    problems = []
    for c in CASES:
        missing = credited.get(c.name, set()) - P.called_wrappers(c, H, public)
        if missing:
            problems.append('%s is credited with %s, which its call never reaches' % (c.name, sorted(missing)))
    assert not problems, '\n'.join(problems)


@pytest.mark.parametrize('case', CASES, ids=_ids(CASES))
def test_uninitialised_memory(case):
    problems = P.check_uninitialised(case)
    assert not problems, '\n'.join(problems)


@pytest.mark.parametrize('case', CASES, ids=_ids(CASES))
def test_guard_bands(case):
    problems = P.check_guards(case)
    assert not problems, '\n'.join(problems)


@pytest.mark.parametrize('case', [c for c in CASES if c.dests], ids=_ids([c for c in CASES if c.dests]))
def test_dirty_destination(case):
    problems = P.check_dirty_out(case)
    assert not problems, '\n'.join(problems)


@pytest.mark.parametrize('case', [c for c in CASES if c.rows], ids=_ids([c for c in CASES if c.rows]))
def test_row_and_window_isolation(case):
    problems = P.check_isolation(case)
    assert not problems, '\n'.join(problems)


@pytest.mark.parametrize('case', CASES, ids=_ids(CASES))
def test_repeat_after_another_shape(case):
    other = _other(case)
    assert other is not case and _signature(other) != _signature(case), (case.name, other.name)
    problems = P.check_repeat(case, other)
    assert not problems, '\n'.join(problems)


def test_the_patch_reaches_the_wrappers():
    """hip_ops resolves torch.empty at call time: an op that allocates its own output does so through the patch."""
    x = torch.randn(3, 7, 32, device='cuda')
    with P.poisoned_allocations() as stats:
        H.global_avgpool_fwd(x)
    assert stats.filled >= 1


# ================================================================================================================================
# the whole step
# ================================================================================================================================
def _build_model(backbone, seed, drop, head='cnn_linear'):
    """The seeded models of the suites that own them: oracle.weights.seeded_params (test_model_gpu, with head='lstm'
    test_lstm_losses_trainer_gpu), se_ref.seeded_se_params (test_se_gpu); the transformer's own parameters keep torch's
    default initialisation under the torch seed the caller set (1234 for the clean and the poisoned run alike; as
    test_transformer_gpu.build_model without a golden does under its seed 11), over the seeded backbone."""
    import deepards_amd.models as M
    from oracle.weights import seeded_params
    if backbone == 'se_resnet18':
        from tools import se_ref
        bb, params = M.se_resnet18(), se_ref.seeded_se_params(seed, 20)
    else:
        bb = M.resnet18() if backbone == 'resnet18' else M.densenet18(drop_rate=drop)
        params = seeded_params(backbone, seed, head={'cnn_linear': 'linear', 'cnn_lstm': 'lstm', 'cnn_transformer': 'single_breath'}[head])
    if head == 'cnn_linear':
        model = M.CNNLinearNetwork(bb, 20, 0)
    elif head == 'cnn_lstm':
        model = M.CNNLSTMNetwork(bb, 0, False, 16)
    else:
        model = M.CNNTransformerNetwork(bb, 0, False, 16, 2)
        params = {k: v for k, v in params.items() if k.startswith('breath_block.')}
    sd = {k: torch.from_numpy(v) for k, v in params.items()}
    assert not model.load_state_dict(sd, strict=False).unexpected_keys
    return model.cuda().train()


def _step_results(backbone, drop, batch, use_graph, steps, patched, head='cnn_linear'):
    """Model construction, ``steps`` training steps and one forward-only step -> every tensor the step leaves behind."""
    from deepards_amd.train import HotPathTrainer
    g = torch.Generator().manual_seed(batch * 7 + 1)
    x = torch.randn(batch, 20, 1, 224, generator=g).cuda()
    t = torch.zeros(batch, 2, device='cuda')
    t[: batch // 2, 0] = 1
    t[batch // 2:, 1] = 1
    torch.manual_seed(1234)
    torch.cuda.manual_seed(1234)
    ctx = P.poisoned_allocations() if patched else contextlib.nullcontext()
    with ctx as stats:
        model = _build_model(backbone, 3, drop, head)
        tr = HotPathTrainer(model, use_graph=use_graph)
        out = {}
        for n in range(steps):
            out['loss%d' % n] = tr.train_step(x, t).clone()
            out['logits%d' % n] = tr.last_logits.clone() if tr.last_logits is not None else None
        out['grad'] = tr.bucket.g.clone()
        out['param'] = tr.bucket.p.clone()
        out['momentum'] = tr.state['buf'].clone()
        tl, tlog, pred = tr.test_step(x, t)
        out['test_loss'], out['test_logits'], out['test_pred'] = tl.clone(), tlog.clone(), pred.clone() if pred is not None else None
        for name, b in model.named_buffers():
            out['buffer.' + name] = b.detach().clone()
        torch.cuda.synchronize()
        tr.release_graphs()
    if patched:
        assert stats.filled > 50, 'the patch reached only %d allocations of a whole step' % stats.filled
    return out


@contextlib.contextmanager
def _config(conv, storage):
    import deepards_amd.functional as F_
    F_.set_conv_dtype(conv)
    if storage == 'bf16':
        F_.set_storage_dtype('bf16')
    try:
        yield
    finally:
        F_.set_conv_dtype('f32')
        F_.set_storage_dtype('f32')


# (backbone, head, drop, conv, storage, batch, use_graph): the linear head at batch 2 and 64 (ids without the head: the rows'
# ids from before the other heads were added), then se_resnet18 and the cnn_lstm / cnn_transformer heads at batch 2
_WHOLE_STEP = [(bb, 'cnn_linear', drop, conv, storage, batch, graph)
               for graph in (False, True) for batch in (2, 64)
               for bb, drop, conv, storage in (('resnet18', 0.0, 'f32', 'f32'), ('densenet18', 0.2, 'f32', 'f32'),
                                               ('resnet18', 0.0, 'bf16', 'bf16'), ('resnet18', 0.0, 'f32x3p', 'f32'))]
_WHOLE_STEP += [(bb, head, 0.0, 'f32', 'f32', 2, graph) for graph in (False, True)
                for bb, head in (('se_resnet18', 'cnn_linear'), ('resnet18', 'cnn_lstm'), ('resnet18', 'cnn_transformer'))]


def _whole_step_id(row):
    bb, head, drop, conv, storage, batch, graph = row
    return '%s-%s-%s-%s-%d-%s' % (bb if head == 'cnn_linear' else bb + '+' + head, drop, conv, storage, batch, 'graph' if graph else 'eager')


@pytest.mark.parametrize('backbone,head,drop,conv,storage,batch,use_graph', _WHOLE_STEP, ids=[_whole_step_id(r) for r in _WHOLE_STEP])
def test_whole_step_under_poisoned_allocations(backbone, head, drop, conv, storage, batch, use_graph):
    """Loss, logits, gradient bucket, parameters and momentum after the update, the forward-only step and every module
    buffer: bit for bit those of the clean run, none holding the pattern.  With use_graph the patch is active during warm-up
    and capture, so the captured fills poison the step's buffers again on every one of the three replayed steps."""
    steps = 3 if use_graph else 1
    with _config(conv, storage):
        clean = _step_results(backbone, drop, batch, use_graph, steps, False, head)
        dirty = _step_results(backbone, drop, batch, use_graph, steps, True, head)
    problems = []
    for k in clean:
        msg = P.diff_report(dirty[k], clean[k])
        if msg:
            problems.append('%s: %s' % (k, msg))
        if dirty[k] is not None and dirty[k].dtype != torch.int64 and P.has_poison(dirty[k]):
            problems.append('%s holds the pattern in %d elements' % (k, P.count_poison(dirty[k])))
    assert not problems, '\n'.join(problems)
