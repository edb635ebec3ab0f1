"""The se_resnet50 / 101 / 152 backbones on the GPU: the wide SE-tail kernels (csrc/se_wide.hip), the chained
SEBlockFunction on the bottleneck, the whole model, the trainer and the driver.

Bound per tensor (the one of tests/test_se_gpu.py): rel-l2 against the float64 oracle <= min(max(4 err32, 16 2^-23), 1e-4),
err32 = the reference's own fp32-against-fp64 rel-l2 from the golden where the shape has one, else tests/tools/sebn_ref.py
evaluated in float32 on the CPU.  The kernel and block cases keep every ReLU pre-activation of the oracle at least 1e-3 from
zero (asserted here, on the CPU): no element is left out of a comparison and the ReLU masks must be the oracle's.
Figures: pytest -s."""
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
import sebn_ref as R  # noqa: E402
import poison as P  # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
FLOOR, CEIL = 16 * 2.0 ** -23, 1e-4
CHUNK = 256                           # rows per chunk of the gate backward's parameter-gradient partials (asserted below)
# (rows, R, L, C, Cr): the four stage shapes of the bottleneck nets; a row tile (32) with one row left and windows that change
# inside a tile; L = 1 with more than two row tiles; 129 rows at the narrowest gate; an odd L in one window; rows past one
# chunk of the partials.  Every case has one negative gamma (tail_case).
SHAPES = [(5, 5, 7, 2048, 128), (6, 3, 14, 1024, 64), (6, 3, 28, 512, 32), (4, 2, 56, 256, 16), (33, 3, 3, 1024, 64),
          (66, 2, 1, 2048, 128), (129, 3, 1, 256, 16), (7, 7, 5, 512, 32), (CHUNK + 2, 2, 1, 256, 16)]
MULTI_CHUNK = SHAPES[-1]


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
    return np.unpackbits(mask.cpu().view(torch.uint8).numpy(), bitorder='little').astype(bool).reshape(shape)


def sid(s):
    return 'x'.join(map(str, s))


# ---- the kernels, each alone ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tail_ref(shape):
    """(case, float64 oracle, err32 per tensor) of one kernel shape, computed once; y2 of se_ref's tail is y3 here."""
    case = R.tail_case(*shape)
    r64 = {k: v.numpy() for k, v in R.se_tail(R=shape[1], **case).items()}
    r64['rowsum'] = case['y2'].astype(np.float64).sum(1)
    r32 = {k: v.double().numpy() for k, v in R.se_tail(R=shape[1], dtype=torch.float32, **case).items() if k != 'mask'}
    r32['rowsum'] = torch.from_numpy(case['y2']).sum(1).double().numpy()
    err = {k: R.rel_l2(r32[k], r64[k]) for k in r32}
    return case, r64, err


@pytest.mark.parametrize('shape', SHAPES, ids=sid)
def test_each_kernel_alone_against_the_oracle(H, shape):
    """Every kernel on the ORACLE's operands (rounded to float32), so that one kernel's error is not another's input."""
    rows, R_, l, c, cr = shape
    assert H.se_wide_chunk_rows() == CHUNK and H.se_wide_ok(c, cr)
    case, ref, err = tail_ref(shape)
    assert case['w1'].shape == (cr, c, 1) and float(case['gamma'].min()) < 0
    hm, om = R.tail_margins(case, R_)
    assert hm >= R.MARGIN and om >= R.MARGIN, (hm, om)
    tag = sid(shape)
    g = {k: cu(v) for k, v in case.items()}
    o = {k: cu(v) for k, v in ref.items() if k != 'mask'}
    bad = []
    mean, invstd, rowsum = H.se_wide_stats(g['y2'], R_)
    for k, v in (('mean', mean), ('invstd', invstd), ('rowsum', rowsum)):
        check(tag, k, v, ref[k], err[k], bad)
    bn = (o['mean'], o['invstd'], g['gamma'], g['beta'])
    pool, hid, s = H.se_wide_gate_fwd(o['rowsum'], R_, l, *bn, g['w1'], g['b1'], g['w2'], g['b2'])
    for k, v in (('pool', pool), ('hid', hid), ('s', s)):
        check(tag, k, v, ref[k], err[k], bad)
    assert np.array_equal(host(hid) > 0, ref['pre1'] > 0), 'hidden ReLU decisions differ from the oracle\'s'
    out, mask = H.se_wide_scale_fwd(g['y2'], R_, *bn, o['s'], g['res'])
    check(tag, 'out', out, ref['out'], err['out'], bad)
    assert mask.dtype == torch.int64 and mask.numel() * 64 == out.numel()
    assert np.array_equal(mask_bits(mask, ref['mask'].shape), ref['mask']), 'ReLU mask differs from the oracle\'s'
    assert np.array_equal(host(out) > 0, ref['mask'])
    gg, dsum = H.se_wide_bwd_reduce(g['dout'], mask, g['y2'], R_, *bn)
    assert torch.equal(gg, g['dout'] * cu(ref['mask']))                # g is a masked copy of dout, not arithmetic
    check(tag, 'dsum', dsum, ref['dsum'], err['dsum'], bad)
    dpool, (dw1, db1, dw2, db2) = H.se_wide_gate_bwd(o['dsum'], o['s'], o['hid'], o['pool'], g['w1'], g['w2'])
    assert dw1.shape == g['w1'].shape and dw2.shape == g['w2'].shape
    for k, v in (('dpool', dpool), ('dw1', dw1), ('db1', db1), ('dw2', dw2), ('db2', db2)):
        check(tag, k, v, ref[k], err[k], bad)
    dz = H.se_wide_bwd_scale(gg, o['s'], o['dpool'])
    check(tag, 'dz', dz, ref['dz'], err['dz'], bad)
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('shape', [(256, 16), (512, 32)], ids=sid)
def test_both_families_agree_on_the_shared_shapes(H, shape):
    """(256, 16) and (512, 32) run on either family; whichever se_gate_family names, the other computes the same tail at
    the bound (the narrow kernels on the map, the wide ones on its row sums)."""
    c, cr = shape
    assert H.se_narrow_ok(c, cr) and H.se_wide_ok(c, cr) and H.se_gate_family(c, cr) in (H.SE_NARROW, H.SE_WIDE)
    full = [s for s in SHAPES if s[3:] == shape][0]
    case, ref, err = tail_ref(full)
    g = {k: cu(v) for k, v in case.items()}
    o = {k: cu(v) for k, v in ref.items() if k != 'mask'}
    bad = []
    pool, hid, s = H.se_gate_fwd(g['y2'], full[1], o['mean'], o['invstd'], g['gamma'], g['beta'], g['w1'], g['b1'], g['w2'], g['b2'])
    for k, v in (('pool', pool), ('hid', hid), ('s', s)):
        check('narrow ' + sid(full), k, v, ref[k], err[k], bad)
    dpool, grads = H.se_gate_bwd(o['dsum'], o['s'], o['hid'], o['pool'], g['w1'], g['w2'])
    for k, v in zip(('dpool', 'dw1', 'db1', 'dw2', 'db2'), (dpool,) + grads):
        check('narrow ' + sid(full), k, v, ref[k], err[k], bad)
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('shape', [SHAPES[0], SHAPES[3], MULTI_CHUNK], ids=sid)
def test_gate_bwd_accumulates_and_is_deterministic(H, shape):
    """(258, 2, 1, 256, 16): two chunks of parameter-gradient partials, the last of two rows."""
    case, ref, _ = tail_ref(shape)
    g = {k: cu(v) for k, v in case.items()}
    o = {k: cu(ref[k]) for k in ('dsum', 's', 'hid', 'pool')}
    run = lambda **kw: H.se_wide_gate_bwd(o['dsum'], o['s'], o['hid'], o['pool'], g['w1'], g['w2'], **kw)
    dpool, fresh = run()
    torch.manual_seed(1)
    fill = [torch.randn_like(t) for t in fresh]
    acc = [t.clone() for t in fill]
    dpool2, got = run(grads=acc, accumulate=True)
    assert all(a is b for a, b in zip(got, acc)) and torch.equal(dpool, dpool2)
    for a, f, t in zip(acc, fill, fresh):
        assert torch.equal(a, f + t)                                    # accumulate == overwrite + the fill, bit for bit
    over = [torch.full_like(t, float('nan')) for t in fresh]
    run(grads=over)                                                     # the overwrite form ignores poisoned destinations
    assert all(torch.equal(a, b) for a, b in zip(over, fresh))
    again = run()[1]
    assert all(torch.equal(a, b) for a, b in zip(again, fresh))         # the same bits twice ...
    oc, oref, _ = tail_ref(SHAPES[2])                                   # ... and again after a call on another shape
    H.se_wide_gate_bwd(cu(oref['dsum']), cu(oref['s']), cu(oref['hid']), cu(oref['pool']), cu(oc['w1']), cu(oc['w2']))
    after = run()[1]
    assert all(torch.equal(a, b) for a, b in zip(after, fresh))
    with pytest.raises(ValueError):
        run(accumulate=True)


def test_forward_kernels_are_deterministic(H):
    shape = SHAPES[4]
    case, ref, _ = tail_ref(shape)
    g = {k: cu(v) for k, v in case.items()}
    a = H.se_wide_stats(g['y2'], shape[1])
    b = H.se_wide_stats(g['y2'], shape[1])
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    f = lambda: H.se_wide_gate_fwd(a[2], shape[1], shape[2], a[0], a[1], g['gamma'], g['beta'], g['w1'], g['b1'], g['w2'], g['b2'])
    assert all(torch.equal(p, q) for p, q in zip(f(), f()))


# ---- refusals -------------------------------------------------------------------------------------------------------------
def _refusal_args(rows, R_, l, c, cr, wc=None):
    """Every operand of the C entry points at (rows, R, L, C, Cr); the outputs sit in poisoned guard bands.  wc: the width of
    the statistics (another width than C: refused by the wrappers)."""
    z = lambda *sh: torch.zeros(*sh, device='cuda')
    ins = dict(y=z(rows, l, c), res=z(rows, l, c), rowsum=z(rows, c), mean=z(rows // R_, wc or c), invstd=z(rows // R_, wc or c),
               gamma=z(c), beta=z(c), w1=z(cr, c, 1), b1=z(cr), w2=z(c, cr, 1), b2=z(c), s=z(rows, c), hid=z(rows, cr))
    outs, handles = {}, []
    for k, sh in (('o_rc', (rows, c)), ('o_rc2', (rows, c)), ('o_rcr', (rows, cr)), ('o_map', (rows, l, c)), ('o_w', (rows // R_, c)),
                  ('o_w2', (rows // R_, c)), ('o_mask', (rows * l * c // 8 + 8,)), ('o_w1', (cr, c, 1)), ('o_b1', (cr,)),
                  ('o_w2g', (c, cr, 1)), ('o_b2', (c,)), ('o_ws', (4 * rows * c + 4 * c * cr,))):
        t = P.fill_poison(torch.empty(sh, device='cuda'))
        outs[k], h = P.guarded(t, name=k)
        handles.append(h)
    return ins, outs, handles


def _untouched(outs, handles):
    P.assert_guards_intact(handles)
    for k, t in outs.items():
        assert P.count_poison(t) == t.numel(), '%s was written by a refused call' % k


@pytest.mark.parametrize('c,cr', [(96, 16), (4096, 128), (384, 24)], ids=['C=96', 'C=4096', 'Cr=24'])
def test_unsupported_shapes_are_refused(H, c, cr):
    """The library refuses the shape with its error before any launch: every entry point of the family, called on the C ABI
    with its destinations inside poisoned guard bands, returns non-zero and writes nothing; the wrappers raise."""
    from deepards_amd import _lib
    rows, R_, l = 4, 2, 3
    assert not H.se_wide_ok(c, cr)
    i, o, handles = _refusal_args(rows, R_, l, c, cr)
    L, p, st = _lib.lib(), H._p, H._stream()
    bn = [p(i[k]) for k in ('mean', 'invstd', 'gamma', 'beta')]
    rcs = [
        L.da_se_wide_gate_fwd(p(i['rowsum']), rows, R_, l, c, cr, *bn, p(i['w1']), p(i['b1']), p(i['w2']), p(i['b2']), p(o['o_rc']),
                              p(o['o_rcr']), p(o['o_rc2']), st),
        L.da_se_wide_gate_bwd(p(i['rowsum']), p(i['s']), p(i['hid']), p(i['s']), p(i['w1']), p(i['w2']), p(o['o_rc']), p(o['o_w1']),
                              p(o['o_b1']), p(o['o_w2g']), p(o['o_b2']), 0, p(o['o_ws']), rows, c, cr, st)]
    if cr != 24:                       # (the three elementwise / reduce entry points do not see Cr)
        rcs += [L.da_se_wide_stats(p(i['y']), rows, R_, l, c, 1e-5, p(o['o_w']), p(o['o_w2']), p(o['o_rc']), p(o['o_ws']), st),
                L.da_se_wide_scale_fwd(p(i['y']), p(i['res']), p(o['o_map']), p(o['o_mask']), rows, R_, l, c, *bn, p(i['s']), st),
                L.da_se_wide_bwd_reduce(p(i['y']), p(o['o_mask']), p(i['y']), p(o['o_map']), p(o['o_rc']), rows, R_, l, c, *bn, st),
                L.da_se_wide_bwd_scale(p(i['y']), p(i['s']), p(i['s']), p(o['o_map']), rows, l, c, st)]
    torch.cuda.synchronize()
    assert all(rc != 0 for rc in rcs), rcs
    _untouched(o, handles)
    with pytest.raises((H.HipError, ValueError)):
        H.se_wide_gate_fwd(i['rowsum'], R_, l, i['mean'], i['invstd'], i['gamma'], i['beta'], i['w1'], i['b1'], i['w2'], i['b2'])
    with pytest.raises((H.HipError, ValueError)):
        H.se_wide_gate_bwd(i['rowsum'], i['s'], i['hid'], i['s'], i['w1'], i['w2'],
                           grads=[o['o_w1'], o['o_b1'], o['o_w2g'], o['o_b2']])
    if cr != 24:
        with pytest.raises((H.HipError, ValueError)):
            H.se_wide_stats(i['y'], R_)
    torch.cuda.synchronize()
    _untouched(o, handles)
    with pytest.raises(NotImplementedError):
        H.se_gate_family(c, cr)


def test_statistics_of_another_width_are_refused(H):
    rows, R_, l, c, cr = 4, 2, 3, 256, 16
    i, o, handles = _refusal_args(rows, R_, l, c, cr, wc=128)
    for call in (lambda: H.se_wide_gate_fwd(i['rowsum'], R_, l, i['mean'], i['invstd'], i['gamma'], i['beta'], i['w1'], i['b1'], i['w2'], i['b2']),
                 lambda: H.se_wide_scale_fwd(i['y'], R_, i['mean'], i['invstd'], i['gamma'], i['beta'], i['s'], i['res'], out=o['o_map']),
                 lambda: H.se_wide_bwd_reduce(i['y'], torch.zeros(rows * l * c // 64, dtype=torch.int64, device='cuda'), i['y'], R_,
                                              i['mean'], i['invstd'], i['gamma'], i['beta'])):
        with pytest.raises(ValueError):
            call()
    torch.cuda.synchronize()
    _untouched(o, handles)


def test_shape_predicates_are_the_library_s(H):
    """se_ops.se_narrow_ok / se_wide_ok restate the C predicates (se.hip se_shape_ok, se_wide.hip sew_shape_ok) so that
    se_gate_family is a pure function; swept over (C, Cr) against the library's own answers -- da_se_wide_shape_ok, and for the
    narrow family da_se_gate_fwd on zero rows, which checks the shape and launches nothing."""
    from deepards_amd import _lib, se_ops
    L, st = _lib.lib(), H._stream()
    d = H._p(torch.zeros(8, device='cuda'))
    for c in list(range(32, 2304, 32)) + [4096]:
        for cr in range(8, 296, 8):
            assert H.se_wide_ok(c, cr) == bool(L.da_se_wide_shape_ok(c, cr)), (c, cr)
            narrow = L.da_se_gate_fwd(d, 0, 1, 1, c, cr, d, d, d, d, d, d, d, d, d, d, d, st) == 0
            assert H.se_narrow_ok(c, cr) == narrow, (c, cr)
            if narrow or H.se_wide_ok(c, cr):
                assert H.se_gate_family(c, cr) == (H.SE_WIDE if not narrow or (c, cr) in se_ops.WIDE_SHARED else H.SE_NARROW)


# ---- memory discipline -----------------------------------------------------------------------------------------------------
def _tail_inputs(shape):
    case, ref, _ = tail_ref(shape)
    return {k: cu(v) for k, v in case.items()}, {k: cu(v) for k, v in ref.items() if k != 'mask'}


def _op_cases(H):
    cases = []
    zg = lambda g: [torch.zeros_like(g['w1']), torch.zeros_like(g['b1']), torch.zeros_like(g['w2']), torch.zeros_like(g['b2'])]
    pg_axis = {'[1][0]': None, '[1][1]': None, '[1][2]': None, '[1][3]': None}     # the parameter gradients sum over all rows
    for shape in (SHAPES[1], SHAPES[4], SHAPES[3]):
        rows, R_, l, c, cr = shape
        tag = sid(shape)

        def b_stats(shape=shape):
            return dict(y=_tail_inputs(shape)[0]['y2'])
        cases.append(P.OpCase('se_wide_stats_' + tag, 'se_wide', b_stats, lambda y, R_=R_: H.se_wide_stats(y, R_),
                              rows=dict(inputs=('y',), R=R_, axis={})))

        def b_gate(shape=shape):
            g, o = _tail_inputs(shape)
            return dict(rowsum=o['rowsum'], mean=o['mean'], invstd=o['invstd'], gamma=g['gamma'], beta=g['beta'], w1=g['w1'], b1=g['b1'],
                        w2=g['w2'], b2=g['b2'])
        cases.append(P.OpCase('se_wide_gate_fwd_' + tag, 'se_wide', b_gate,
                              lambda rowsum, mean, invstd, gamma, beta, w1, b1, w2, b2, R_=R_, l=l:
                              H.se_wide_gate_fwd(rowsum, R_, l, mean, invstd, gamma, beta, w1, b1, w2, b2),
                              rows=dict(inputs=('rowsum',), R=R_, axis={})))

        def b_scale(shape=shape):
            g, o = _tail_inputs(shape)
            return dict(y=g['y2'], res=g['res'], mean=o['mean'], invstd=o['invstd'], gamma=g['gamma'], beta=g['beta'], s=o['s'],
                        out=torch.zeros_like(g['y2']))
        cases.append(P.OpCase('se_wide_scale_fwd_' + tag, 'se_wide', b_scale,
                              lambda y, res, mean, invstd, gamma, beta, s, out, R_=R_:
                              H.se_wide_scale_fwd(y, R_, mean, invstd, gamma, beta, s, res, out=out),
                              dests=('out',), rows=dict(inputs=('y', 'res', 's'), R=1, axis={})))

        def b_red(shape=shape):
            g, o = _tail_inputs(shape)
            _, mask = H.se_wide_scale_fwd(g['y2'], shape[1], o['mean'], o['invstd'], g['gamma'], g['beta'], o['s'], g['res'])
            return dict(dout=g['dout'], mask=mask, y=g['y2'], mean=o['mean'], invstd=o['invstd'], gamma=g['gamma'], beta=g['beta'])
        cases.append(P.OpCase('se_wide_bwd_reduce_' + tag, 'se_wide', b_red,
                              lambda dout, mask, y, mean, invstd, gamma, beta, R_=R_: H.se_wide_bwd_reduce(dout, mask, y, R_, mean, invstd, gamma, beta),
                              rows=dict(inputs=('dout', 'y'), R=R_, axis={})))

        def b_gbw(shape=shape):
            g, o = _tail_inputs(shape)
            return dict(dsum=o['dsum'], s=o['s'], hid=o['hid'], pool=o['pool'], w1=g['w1'], w2=g['w2'], grads=zg(g))
        cases.append(P.OpCase('se_wide_gate_bwd_' + tag, 'se_wide', b_gbw,
                              lambda dsum, s, hid, pool, w1, w2, grads: H.se_wide_gate_bwd(dsum, s, hid, pool, w1, w2, grads=grads),
                              dests=('grads',), rows=dict(inputs=('dsum', 's', 'hid', 'pool'), R=1, axis=pg_axis)))

        def b_bsc(shape=shape):
            g, o = _tail_inputs(shape)
            return dict(g=o['g'], s=o['s'], dpool=o['dpool'], out=torch.zeros_like(o['g']))
        cases.append(P.OpCase('se_wide_bwd_scale_' + tag, 'se_wide', b_bsc, lambda g, s, dpool, out: H.se_wide_bwd_scale(g, s, dpool, out=out),
                              dests=('out',), rows=dict(inputs=('g', 's', 'dpool'), R=1, axis={})))

    def b_gbw2():                      # two chunks of partials: every partial written and folded, none twice
        g, o = _tail_inputs(MULTI_CHUNK)
        return dict(dsum=o['dsum'], s=o['s'], hid=o['hid'], pool=o['pool'], w1=g['w1'], w2=g['w2'], grads=zg(g))
    cases.append(P.OpCase('se_wide_gate_bwd_' + sid(MULTI_CHUNK), 'se_wide', b_gbw2,
                          lambda dsum, s, hid, pool, w1, w2, grads: H.se_wide_gate_bwd(dsum, s, hid, pool, w1, w2, grads=grads),
                          dests=('grads',), rows=dict(inputs=('dsum', 's', 'hid', 'pool'), R=1, axis=pg_axis)))
    return cases


CHECKS = {'uninitialised': P.check_uninitialised, 'guards': P.check_guards, 'dirty_out': P.check_dirty_out, 'isolation': P.check_isolation}
N_OP_CASES = 19
WRAPPERS = ('se_wide_stats', 'se_wide_gate_fwd', 'se_wide_scale_fwd', 'se_wide_bwd_reduce', 'se_wide_gate_bwd', 'se_wide_bwd_scale')


@pytest.mark.parametrize('check', sorted(CHECKS))
@pytest.mark.parametrize('i', range(N_OP_CASES))
def test_memory_discipline(H, i, check):
    cases = _op_cases(H)
    assert len(cases) == N_OP_CASES
    problems = CHECKS[check](cases[i])
    assert not problems, '\n'.join(problems)


def test_every_new_wrapper_has_a_memory_discipline_row(H):
    from deepards_amd import se_ops
    names = {c.name for c in _op_cases(H)}
    launching = sorted(n for n, f in vars(se_ops).items() if callable(f) and n.startswith('se_wide_') and n not in ('se_wide_ok', 'se_wide_chunk_rows'))
    assert launching == sorted(WRAPPERS)
    assert all(any(n.startswith(w + '_') for n in names) for w in WRAPPERS)


# ---- the chained block ----------------------------------------------------------------------------------------------------
BLOCK_TAGS = ['id_4x2x56x256', 'id_6x3x5x1024', 'id_5x5x7x2048', 'e1_4x2x56x256', 's2_6x3x28x512', 's2_6x3x14x1024', 's2_5x5x7x2048']


@functools.lru_cache(maxsize=None)
def block_ref(tag):
    g = _gold('sebn_block_%s.npz' % tag)
    rows, R_, l_out, cin, planes, stride, ds, seed = (int(v) for v in g['cfg'])
    _, params, dout = R.block_draws(rows, R_, l_out, cin, planes, stride, bool(ds), seed)
    x = g['x']
    r = {k: v.numpy() for k, v in R.block_case(x, params, stride, R_, dout).items()}
    return g, x, params, dout, (cin, planes, stride, bool(ds), R_), r


@pytest.mark.parametrize('winograd', [True, False], ids=['default', 'DA_WINOGRAD=0'])
@pytest.mark.parametrize('tag', BLOCK_TAGS)
def test_chained_block_function(H, M, tag, winograd):
    """SEBlockFunction on an SEResNetBottleneck (identity blocks, the stride-1 entry of layer1 and the stride-2 entries) through the module, forward
    and backward, against the oracle at the golden's err32; the output's ReLU decisions must be the oracle's.  Then the same
    block inside a training step with gradient destinations on every parameter (the batched weight-gradient launch, the queued
    folds, the SE parameters written in place): the destinations hold the same gradients at the same bound."""
    g, x, params, dout, (cin, planes, stride, has_ds, R_), ref = block_ref(tag)
    m = {k: float(np.abs(ref['pre/' + k]).min()) for k in ('h1', 'h2', 'hid', 'out')}
    assert min(m.values()) >= R.MARGIN, m
    ds = None
    if has_ds:
        ds = torch.nn.Sequential(torch.nn.Conv1d(cin, planes * 4, kernel_size=1, stride=stride, bias=False), torch.nn.BatchNorm1d(planes * 4))
    blk = M.SEResNetBottleneck(cin, planes, 1, 16, stride, ds)
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
    check(name, 'out', out, ref['out'], float(g['err32/out']), bad)
    assert np.array_equal(host(out) > 0, ref['pre/out'] > 0), 'output ReLU decisions differ from the oracle\'s'
    check(name, 'dx', xt.grad, ref['dx'], float(g['err32/dx']), bad)
    for n, q in blk.named_parameters():
        check(name, 'grad/' + n, q.grad, ref['grad/' + n], float(g['err32/grad/' + n]), bad)
    assert not bad, '\n'.join(bad)
    from deepards_amd import functional as F_
    for n, q in blk.named_parameters():
        q.grad = None
        q._da_grad = torch.zeros_like(q)
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
    check(name + ' step', 'dx', xs.grad, ref['dx'], float(g['err32/dx']), bad)
    for n in dests:
        check(name + ' step', 'grad/' + n, dests[n], ref['grad/' + n], float(g['err32/grad/' + n]), bad)
    assert not bad, '\n'.join(bad)
    # running statistics: one momentum update per window (the reference's loop), two forwards
    w = x.shape[0] // R_
    bns = [blk.bn1, blk.bn2, blk.bn3] + ([blk.downsample[1]] if has_ds else [])
    assert all(int(b.num_batches_tracked) == 2 * w for b in bns)
    assert torch.isfinite(blk.bn3.running_var).all() and float((blk.bn3.running_mean != 0).float().mean()) > 0.9


# ---- the whole model -----------------------------------------------------------------------------------------------------
def build_model(M, g, net='se_resnet50', head='linear'):
    nb = int(g['nb'])
    bb = M.base_networks[net]()
    model = M.CNNLinearNetwork(bb, nb, 0) if head == 'linear' else M.CNNSingleBreathLinearNetwork(bb)
    params = R.seeded_params(net, int(g['seed']), nb, bn_bias_shift=float(g['bn_bias_shift']), fc1_bias_shift=float(g['fc1_bias_shift']))
    sd = {k: torch.from_numpy(v) for k, v in params.items() if head == 'linear' or k.startswith('breath_block.')}
    assert not model.load_state_dict(sd, strict=False).unexpected_keys
    return model.cuda().train()


def test_whole_model_gradients_against_the_golden(M):
    """CNNLinearNetwork(se_resnet50(), 2, 0) at B = 2 with the shifted biases on the decided input: logits, loss and every
    parameter gradient.  A tensor the golden lists as unpinned (err32 > 2.5e-5: its exact gradient is ~ 0) is held to an
    absolute l2 error of 1e-4 x the norm of the same module's weight gradient."""
    from deepards_amd import functional as F_
    g = _gold('sebn_model_se_resnet50_b2_grads.npz')
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
    unpinned = {str(n) for n in g['unpinned']}
    assert len(unpinned) <= 4 and len(list(model.named_parameters())) == 225
    for n, q in model.named_parameters():
        assert q.grad is not None, n
        key = 'grad/' + n
        ref = g['dig/' + key] if 'dig/' + key in g else g[key]
        got = digest(host(q.grad)) if 'dig/' + key in g else host(q.grad)
        if key in unpinned:
            e, bd = float(np.linalg.norm(got.reshape(ref.shape) - ref)), 1e-4 * float(g['wnorm/' + key])
        else:
            e, bd = R.rel_l2(got.reshape(ref.shape), ref), bound(float(g['err32/' + key]))
        log('model %-60s %s %.3e  reference fp32 %.3e  bound %.3e' % (key, 'abs l2' if key in unpinned else 'digest rel-l2', e,
                                                                       float(g['err32/' + key]), bd))
        if not e <= bd:
            bad.append('%s: %.3e > bound %.3e' % (key, e, bd))
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('name,net', [('sebn_model_se_resnet50_nb20.npz', 'se_resnet50'), ('sebn_model_se_resnet50_nb20_shifted.npz', 'se_resnet50'),
                                      ('sebn_model_se_resnet101_nb2_shifted.npz', 'se_resnet101'),
                                      ('sebn_model_se_resnet152_nb2_shifted.npz', 'se_resnet152')])
def test_whole_model_logits_and_loss(M, name, net):
    from deepards_amd import functional as F_
    g = _gold(name)
    model = build_model(M, g, net)
    assert list(model.state_dict().keys()) == [str(n) for n in g['names']]
    with torch.no_grad():
        out = model(torch.from_numpy(g['x']).cuda(), None)
        loss = F_.bce_with_logits(out, torch.from_numpy(g['target']).cuda())
    bad = []
    check(name, 'logits', out, g['logits'], float(g['err32/logits']), bad)
    check(name, 'loss', loss, g['loss'], float(g['err32/loss']), bad)
    assert not bad, '\n'.join(bad)
    if int(g['nb']) == 20 and float(g['bn_bias_shift']) == 0:
        bb = model.breath_block                  # forward_windows(pooled=True) and features() agree with the head's path
        with torch.no_grad():
            x = torch.from_numpy(g['x'][0]).cuda()
            feat, fmap = bb(x), bb.features(x)
        assert tuple(feat.shape) == (20, 2048) and tuple(fmap.shape) == (20, 2048, 7)
        assert torch.allclose(bb.logits(fmap).squeeze(-1), feat, rtol=1e-5, atol=1e-6)


# ---- trainer and driver --------------------------------------------------------------------------------------------------
def test_trainer_eager_and_captured_steps_are_bit_equal(M):
    """se_resnet50 at B = 2, NB = 2: four eager steps against the eager first step plus THREE replays of the captured step
    leave the same losses, parameters and optimiser state, bit for bit; every SE parameter moved.  The capture took the
    overwrite form of the gradient bucket (no zero-fill: every writer of the block, the wide gate backward among them, has
    one), and the graph was captured once."""
    from deepards_amd.train import HotPathTrainer
    g = _gold('sebn_model_se_resnet50_b2_grads.npz')
    x, t = torch.from_numpy(g['x']).cuda(), torch.from_numpy(g['target']).cuda()
    runs = []
    for use_graph in (False, True):
        model = build_model(M, g)
        start = {n: q.detach().clone() for n, q in model.named_parameters()}
        tr = HotPathTrainer(model, optimizer='sgd', use_graph=use_graph)
        losses = []
        for step in range(4):
            losses.append(tr.train_step(x, t).detach().clone().reshape(-1))
            assert len(tr._graphs) == (1 if use_graph and step >= 1 else 0)      # step 0 is the eager first step, then replays
        losses = torch.cat(losses)
        if use_graph:
            assert tr.grad_overwrite, 'a gradient writer without an overwrite form ran: the capture fell back to the zero-fill'
            assert tr.last_loss is tr._graph[2][0]                              # the replay's own output buffer
        runs.append((losses, tr.bucket.p.clone(), {k: v.clone() for k, v in tr.state.items()}))
        moved = {n: float((q.detach() - start[n]).abs().max()) for n, q in model.named_parameters() if 'se_module' in n}
        assert len(moved) == 64 and min(moved.values()) > 0, 'SE parameters that did not move: %s' % [n for n, v in moved.items() if v == 0]
        if use_graph:
            tr.release_graphs()
    assert torch.isfinite(runs[0][0]).all()
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert set(runs[0][2]) == set(runs[1][2]) and 'buf' in runs[0][2]
    assert all(torch.equal(runs[0][2][k], runs[1][2][k]) for k in runs[0][2])


def test_one_captured_step_on_se_resnet152(M):
    """The deepest net (50 blocks) in one graph: with learning rate and weight decay 0 the eager first step leaves the golden's
    parameters where they are (asserted), the second call captures and replays, and the REPLAY's own logits and loss are held to
    the bound; a second replay gives the same bits."""
    from deepards_amd.train import HotPathTrainer
    g = _gold('sebn_model_se_resnet152_nb2_shifted.npz')
    x, t = torch.from_numpy(g['x']).cuda(), torch.from_numpy(g['target']).cuda()
    model = build_model(M, g, 'se_resnet152')
    tr = HotPathTrainer(model, optimizer='sgd', learning_rate=0.0, weight_decay=0.0, use_graph=True)
    tr.train_step(x, t)                                                 # eager: discovers the live parameters
    assert not tr._graphs
    p0 = tr.bucket.p.clone()
    bad = []
    for replay in (1, 2):
        loss = tr.train_step(x, t)
        assert len(tr._graphs) == 1 and tr.grad_overwrite
        assert loss is tr._graph[2][0] and tr.last_logits is tr._graph[2][1]     # the captured step's output buffers
        assert torch.equal(tr.bucket.p, p0)
        check('se_resnet152 replay %d' % replay, 'logits', tr.last_logits, g['logits'], float(g['err32/logits']), bad)
        check('se_resnet152 replay %d' % replay, 'loss', loss, g['loss'], float(g['err32/loss']), bad)
        if replay == 1:
            first = (loss.detach().clone(), tr.last_logits.detach().clone(), tr.bucket.g.clone())
    assert not bad, '\n'.join(bad)
    assert torch.equal(first[0], loss) and torch.equal(first[1], tr.last_logits) and torch.equal(first[2], tr.bucket.g)
    assert torch.isfinite(tr.bucket.g).all() and float(tr.bucket.g.abs().max()) > 0
    tr.release_graphs()


def test_per_breath_head_with_the_confidence_loss(M):
    from deepards_amd.train import HotPathTrainer
    g = _gold('sebn_model_se_resnet50_b2_grads.npz')
    x, t = torch.from_numpy(g['x']).cuda(), torch.from_numpy(g['target']).cuda()
    tr = HotPathTrainer(build_model(M, g, head='single_breath'), use_graph=False, loss='confidence', loss_param=0.5)
    assert torch.isfinite(tr.train_step(x, t)).all()


def test_driver_trains_and_tests_on_the_fixture():
    from deepards_amd import train_ards_detector as T
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    cls = T.network_map['cnn_linear'](T.make_args(train_from_pickle=os.path.join(GOLD, 'test_dataset.npz'), kfolds=2, epochs=1,
                                                  batch_size=4, seed=3, base_network='se_resnet50', cuda=False, cuda_no_dp=True))
    res = cls.train_and_test()
    assert cls.model.breath_block.network_name == 'se_resnet50'
    for fold in (0, 1):
        assert len(res.get_meter('loss', fold)) > 0
        assert np.isfinite(res.get_meter('loss', fold)).all() and np.isfinite(res.get_meter('test_loss', fold)).all()
        assert np.isfinite(res.patient_results[(fold, 1)]['mean_loss'])
