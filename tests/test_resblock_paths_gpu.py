"""functional.BasicBlockFunction, every path against float64 at the edges of its predicates.

One forward / backward of the block Function chooses among an entry form, fuse1, the x3 flags, the BatchNorm pair forms, the
two-term upstream gradient (or its host-side sum), pool_out, mask or sign of ``out``, queued or immediate folds, accumulate or
overwrite -- each a predicate on (W, Wn, C, L) and the arithmetic.  tests/tools/resblock_ref.py holds the table of chains with
the path each must take (as literals; tests/test_resblock_ref_cpu.py holds it to the library's predicates), and
tests/tools/resblock_chain.py runs them the way ResNet._map does, eager and inside a training step.  Here:

  a. fp32 and f32x3p arithmetic against the float64 chain UNDER THE DEVICE'S ReLU DECISIONS: output (or loss and logits), dx,
     every parameter gradient, every running statistic, num_batches_tracked.  Bound per tensor: 8 x the reference chain's own
     float32 error on the same inputs, clamped to [16 * 2^-23, 1e-4] of 1 + max|ref| (resblock_ref.bound).  A mask may differ
     from the sign of the reference's z on at most 1e-4 of an activation, only where |z| <= 1e-5 (1 + max|z|); those elements
     are left out of the forward comparison only.  The launches are counted and must be the path the table names.
  b. fast path == plain path bit for bit, switch by switch (every arithmetic), and a step that overwrites NaN-filled
     destinations == a step that accumulates into zero-filled ones.
"""
import hashlib

import numpy as np
import pytest
import torch

from tools import resblock_chain as RC
from tools import resblock_ref as RR

pytestmark = pytest.mark.gpu


def log(*a):
    print(*a, flush=True)


@pytest.fixture(scope='module')
def Fn():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    import deepards_amd.functional as fn
    return fn


class arithmetic(object):
    """Conv dtype, storage dtype and switches for the duration of a test; everything is put back on exit."""

    def __init__(self, conv='f32', storage='f32', **switches):
        self.conv, self.storage, self.switches = conv, storage, switches

    def __enter__(self):
        from deepards_amd import functional as F_
        from deepards_amd.models import resnet as R_
        self.F_, self.R_ = F_, R_
        self.old = (F_.conv_dtype(), F_.storage_dtype())
        self.old_sw = {}
        F_.set_conv_dtype(self.conv)
        F_.set_storage_dtype(self.storage)
        for k, v in self.switches.items():
            mod = R_ if hasattr(R_, k) else F_
            self.old_sw[k] = (mod, getattr(mod, k))
            setattr(mod, k, v)
        return self

    def __exit__(self, *exc):
        for k, (mod, v) in self.old_sw.items():
            setattr(mod, k, v)
        self.F_.set_storage_dtype('f32')
        self.F_.set_conv_dtype(self.old[0])
        if self.old[1] != 'f32':
            self.F_.set_storage_dtype(self.old[1])


# ---- the reference, once per case and set of decisions ---------------------------------------------------------------------------
_DATA, _REF = {}, {}


def case_data(name):
    if name not in _DATA:
        _DATA[name] = RR.make_data(RR.ALL_CASES[name])
    return _DATA[name]


def reference(name, masks):
    """(float64 chain under ``masks``, its own float32 error per compared tensor, the elements of the last activation whose
    decision differs from the sign of the reference's z) -- after holding the masks to the decision rule."""
    case, data = RR.ALL_CASES[name], case_data(name)
    key = (name, hashlib.sha1(b''.join(np.packbits(m).tobytes() for m in masks)).hexdigest())
    if key not in _REF:
        ref = RR.run_ref(case, data, masks=masks)
        twin = RR.run_ref(case, data, dtype=torch.float32, masks=masks)
        a, b = RR.compared(ref), RR.compared(twin)
        _REF[key] = (ref, {n: RR.rel_err(b[n], a[n]) for n in a})
    ref, err32 = _REF[key]
    assert len(masks) == len(ref['z'])
    flipped = None
    for i, (m, z) in enumerate(zip(masks, ref['z'])):
        assert m.shape == z.shape, (i, m.shape, z.shape)
        flipped = m != (z > 0)
        n = int(flipped.sum())
        assert n <= RR.NEAR_SHARE * z.size, 'activation %d: %d of %d decisions differ from the reference' % (i, n, z.size)
        if n:
            far, lim = float(np.abs(z[flipped]).max()), RR.NEAR * (1 + float(np.abs(z).max()))
            assert far <= lim, 'activation %d: a decision differs where the float64 pre-activation is %.2e (> %.2e) from zero' % (i, far, lim)
    return ref, err32, flipped


def _group(n):
    return 'param grads' if n.startswith('d ') else 'running' if 'running' in n else n


def assert_against_fp64(tag, name, mode, res):
    """Assertion (a) on one run; logs the device's and the reference's own error per group of tensors."""
    case = RR.ALL_CASES[name]
    ref, err32, flipped = reference(name, res['masks'])
    got, want = RC.as_compared(res['raw'], mode), RR.compared(ref)
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    bad, worst = [], {}
    for n in want:
        g, w = got[n], want[n]
        assert g.shape == w.shape, (n, g.shape, w.shape)
        if n == 'out':                                  # undecidable elements: out of the forward comparison only
            g, w = np.where(flipped, 0.0, g), np.where(flipped, 0.0, w)
        e, b = RR.rel_err(g, w), RR.bound(err32[n])
        k = _group(n)
        if k not in worst or e / b > worst[k][0] / worst[k][2]:
            worst[k] = (e, err32[n], b)
        if not e <= b:
            bad.append('%s: err %.3e, reference fp32 %.3e, bound %.3e' % (n, e, err32[n], b))
    log('RESBLOCK %s %s %s | ' % (tag, name, mode) + ' | '.join('%s dev %.2e ref32 %.2e bound %.2e' % ((k,) + v) for k, v in sorted(worst.items())))
    assert not bad, bad
    for n in RR.bn_names(case):
        assert int(res['raw'][n + '.num_batches_tracked']) == case.W, n
    if mode == 'step-overwrite':
        assert all(bool(torch.isfinite(t).all()) for k, t in res['raw'].items() if k.startswith('dest ')), 'a NaN survived'
    if mode != 'eager':
        assert res['ov_ok'], 'a gradient writer without an overwrite form ran'


# ---- the path, from the counted launches -----------------------------------------------------------------------------------------
def summary(res):
    c = res['calls']
    n = lambda k: len(c[k])
    return dict(flags=list(res['flags']), left=res['left'], taken=res['taken'], bn_bwd_two=n('bn_bwd_two'),
                bn_bwd_pair=list(c['bn_bwd_pair']), bn_fwd_pair=n('bn_fwd_pair'), bn_bwd=sorted(c['bn_bwd']),
                pool=(n('bn_fwd_pool'), n('bn_bwd_pool')), head=(n('head_fwd'), n('head_flat_fwd')),
                entry=(n('conv_fwd_multi'), n('conv_dgrad_s2_pair')), kernels=frozenset(c['conv_kernel']),
                running=(list(c['bn_running_multi']), list(c['step_tail_multi'])))


def expected_f32(case, mode):
    """What ``summary`` must say for a two-block chain of the table under fp32 arithmetic, from the case's literals."""
    step, entry = mode != 'eager', RR.has_ds(case.blocks[0])
    assert len(case.blocks) == 2 and not RR.has_ds(case.blocks[1])
    two = step and case.two                             # the two-term forms need the step's hand-over
    pair = entry and case.pair
    bwd = [(1, False), (1, False)]                      # the two bn1 backwards
    if not case.pool:                                   # bn2 of the block behind (pooled: bn_bwd_pool)
        bwd.append((2, case.single))
    if not pair and not two:                            # bn2 of the block in front: mask form, or the sign of ``out``
        bwd.append((2, case.single))
    if entry and not pair:                              # the downsample BatchNorm's backward on g
        bwd.append((0, False))
    n_bn = len(RR.bn_names(case))
    return dict(flags=[(False, False, False), (False, case.pool, True)], left=int(step), taken=int(step),
                bn_bwd_two=int(two and not pair), bn_bwd_pair=[two] if pair else [], bn_fwd_pair=int(pair), bn_bwd=sorted(bwd),
                pool=(1, 1) if case.pool else (0, 0), head=(0, 1) if case.pool else (1, 0) if case.head else (0, 0),
                entry=(1, 1) if entry else (0, 0), kernels=frozenset([case.wino]),
                running=([], [n_bn]) if step else ([1] * n_bn, []))


F32_CASES = [n for n, c in RR.CASES.items() if c.raises is None]


@pytest.mark.parametrize('mode', RC.MODES)
@pytest.mark.parametrize('name', F32_CASES)
def test_f32_chain_against_float64_on_the_path_the_table_names(Fn, name, mode):
    """Every row of the table, fp32 arithmetic, eager / step / step-overwrite: the counted launches are the row's path
    (the second gradient term left and taken, bn_bwd_two or bn_bwd_pair(dout2=) or the host-side sum, the pair and pooled
    forms, mask or sign of ``out``, immediate or queued running statistics), and everything the chain computes is within
    the bound of the float64 chain under the device's decisions.  In a step the destinations start at 0.375 (NaN when
    overwriting) and must end at 0.375 + gradient; nothing comes back through .grad."""
    case = RR.CASES[name]
    with arithmetic('f32', 'f32'):
        res = RC.run_chain(case, case_data(name), mode, tap=True)
    got, want = summary(res), expected_f32(case, mode)
    assert got == want, {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    host_sum = res['taken'] - got['bn_bwd_two'] - sum(got['bn_bwd_pair'])
    assert host_sum == int(mode != 'eager' and not case.two)
    assert_against_fp64('f32', name, mode, res)


def test_cases_that_end_in_an_error(Fn):
    """pool_out on a map without the pooled form (Wn 180): ValueError from the Function; a split block with nobody in front:
    flush_backward refuses to drop the second term."""
    with arithmetic('f32', 'f32'):
        case = RR.CASES['pool_L9']
        with pytest.raises(ValueError, match='pool_out'):
            RC.run_chain(case, case_data('pool_L9'), 'eager')
        case = RR.CASES['lone_split_L14']
        with pytest.raises(RuntimeError, match='two-term input gradient'):
            RC.run_chain(case, case_data('lone_split_L14'), 'step')
        assert not Fn._STEP['on'] and not Fn._STEP.get('dout2')          # (the step closed behind the error)
        res = RC.run_chain(case, case_data('lone_split_L14'), 'eager', tap=True)      # outside a step there is nothing to hand over
        assert res['left'] == 0
        assert_against_fp64('f32', 'lone_split_L14', 'eager', res)


def _forms(res):
    c = res['calls']
    n = lambda k: len(c[k])
    return dict(x3=(n('conv_x3p_s2_fwd'), n('conv_x3p_s2_dgrad')), bf16=(n('conv_fwd_bf16_s2'), n('conv_dgrad_bf16_s2_pair')),
                direct=(n('conv_fwd_multi'), n('conv_dgrad_s2_pair')))


def assert_arith_path(case, exp, res):
    """The arithmetic-specific part of a path: takes3 per block, the entry form, the conv kernels, the fused bn1."""
    assert tuple(f[0] for f in res['flags']) == exp.takes3, res['flags']
    forms = _forms(res)
    want = dict(x3=(0, 0), bf16=(0, 0), direct=(0, 0))
    if exp.entry is not None:
        want[{RR.X3: 'x3', RR.BF16: 'bf16', RR.DIRECT: 'direct'}[exp.entry]] = (1, 1)
    assert forms == want, (forms, want)
    c = res['calls']
    assert frozenset(c['conv_kernel']) == exp.kernels, (set(c['conv_kernel']), exp.kernels)
    assert (len(c['bn_fwd_x']) > 0) == any(exp.takes3) and (len(c['bn_bwd_x']) > 0) == any(exp.takes3)
    assert (len(c['conv3_x3p']) > 0) == (RR.X3 in exp.kernels)
    assert len(c['conv3_bf16_bn']) == 2 * exp.fused and len(c['bn_bwd_ss']) == exp.fused
    assert res['taken'] == res['left']


@pytest.mark.parametrize('mode', ['eager', 'step'])
@pytest.mark.parametrize('name', list(RR.ARITH[('f32x3p', 'f32')]))
def test_x3_chain_against_float64(Fn, name, mode):
    """Conv arithmetic 'f32x3p': the x3 flow (in3, mid3, want_out3) at L = 128, the fall to the fp32 kernels at L = 129 (no
    store forms), a front block on x3 in front of an odd DIRECT entry, an X3 entry -- against float64 as the fp32 cases."""
    case, exp = RR.ALL_CASES[name], RR.ARITH[('f32x3p', 'f32')][name]
    with arithmetic('f32x3p', 'f32'):
        res = RC.run_chain(case, case_data(name), mode, tap=True)
    assert_arith_path(case, exp, res)
    if name == 'id2_L129':                              # plain fp32 blocks: the whole path of the fp32 row
        got, want = summary(res), expected_f32(case, mode)
        assert got == want, {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    else:
        assert res['left'] == 0                         # no two-term hand-over next to an x3 edge
    assert_against_fp64('f32x3p', name, mode, res)


# ---- b. fast path == plain path, bit for bit ---------------------------------------------------------------------------------
def assert_same_bits(a, b, what):
    assert list(a['raw']) == list(b['raw']), what
    diff = [n for n in a['raw'] if not torch.equal(a['raw'][n], b['raw'][n])]
    assert not diff, '%s: %s differ' % (what, diff)


def relevant_switches(case, conv, storage, exp):
    """switch -> the counter that must go to zero with it (None: nothing to count), as the case's literals say."""
    sw = {'_WGRAD_CHAIN': None}
    if len(case.blocks) == 2 and not RR.has_ds(case.blocks[1]) and not any(exp.takes3) and storage == 'f32':
        sw['_SPLIT_DX'] = 'left'
    # (bf16 storage with the two-term hand-over in front of the pair: the tests of their own below)
    if exp.entry is not None and case.pair and not any(exp.takes3[1:]) and not (conv == 'f32x3p') and not (storage == 'bf16' and case.two):
        sw['_BN_PAIR'] = 'bn_fwd_pair'
    if case.pool:
        sw['_FUSED_TAIL'] = 'bn_fwd_pool'
    return sw


def _count(res, key):
    return res[key] if key in ('left', 'taken') else len(res['calls'][key])


def equalities(case, name, conv, storage, exp, fused=False):
    data = case_data(name)
    extra = {'_BN1_FUSED': True} if fused else {}
    with arithmetic(conv, storage, **extra):
        base = RC.run_chain(case, data, 'step', dest_fill=0.0)
        assert base['ov_ok']
    for sw, counter in sorted(relevant_switches(case, conv, storage, exp).items()):
        with arithmetic(conv, storage, **dict(extra, **{sw: False})):
            off = RC.run_chain(case, data, 'step', dest_fill=0.0)
        if counter is not None:
            assert _count(base, counter) > 0 and _count(off, counter) == 0, (sw, counter, _count(base, counter), _count(off, counter))
        assert_same_bits(base, off, '%s %s/%s with %s off' % (name, conv, storage, sw))
    with arithmetic(conv, storage, **extra):
        ov = RC.run_chain(case, data, 'step-overwrite')
    assert ov['ov_ok'], 'a gradient writer without an overwrite form ran'
    assert all(bool(torch.isfinite(t).all()) for k, t in ov['raw'].items() if k.startswith('dest ')), 'a NaN survived'
    assert_same_bits(base, ov, '%s %s/%s overwrite vs accumulate from zero' % (name, conv, storage))
    return base


@pytest.mark.parametrize('name', F32_CASES)
def test_f32_fast_paths_equal_the_plain_ones_bit_for_bit(Fn, name):
    """split_dx, _BN_PAIR, _WGRAD_CHAIN, pool_out off one at a time, and overwrite against accumulate-from-zero: torch.equal
    on the output, dx, every destination and every running statistic."""
    case = RR.CASES[name]
    equalities(case, name, 'f32', 'f32', RR.arith_f32(case))


@pytest.mark.parametrize('name', ['id2_L128', 'idE_L128'])
def test_x3_fast_paths_equal_the_plain_ones_bit_for_bit(Fn, name):
    equalities(RR.ALL_CASES[name], name, 'f32x3p', 'f32', RR.ARITH[('f32x3p', 'f32')][name])


@pytest.mark.parametrize('storage', ['f32', 'bf16'])
@pytest.mark.parametrize('name', list(RR.ARITH[('bf16', 'f32')]))
def test_bf16_paths_and_equalities(Fn, name, storage):
    """bf16 arithmetic with fp32 and with bf16 storage: the entry form, the kernels and the fused bn1 (_BN1_FUSED on at
    R L = 120: not fused, 140: fused) the table names; the odd-length entry runs DIRECT with fp32 storage and raises with
    bf16 storage; the same switches bit for bit (bf16 storage: all but split_dx, whose in-kernel sum is unrounded where
    the stored one is not; _BF16_DGRAD_PAIR has the two tests below).  The arithmetic itself is pinned by the exact and
    rounding-model tests."""
    case, exp = RR.ALL_CASES[name], RR.ARITH[('bf16', storage)][name]
    fused = name in ('id2_L6', 'id2_L7')
    if exp.raises is not None:
        with arithmetic('bf16', storage):
            with pytest.raises(exp.raises):
                RC.run_chain(case, case_data(name), 'eager')
        return
    base = equalities(case, name, 'bf16', storage, exp, fused=fused)
    assert_arith_path(case, exp, base)
    for k, t in base['raw'].items():
        assert bool(torch.isfinite(t.float()).all()), k
    if case.pool:
        assert (len(base['calls']['bn_fwd_pool']), len(base['calls']['head_flat_fwd'])) == (1, 1)


# _BF16_DGRAD_PAIR: a bf16 entry's two data gradients in one launch contract the even input positions over TWO sources; the
# first source's sums are kept apart and added at the end, as the second of the two launches adds onto the first's stored
# result: bit for bit with float storage.  With bf16 storage the two launches round the stored sum once more.
BF16_ENTRIES = [n for n, e in RR.ARITH[('bf16', 'f32')].items() if e.entry == RR.BF16]
_PAIR_RUNS = {}


def toggle_runs(name, storage, switch, counter, **both):
    """(a bf16 step, the same step with ``switch`` off), once per case, storage and switch; ``both``: switches set in both."""
    key = (name, storage, switch, tuple(sorted(both.items())))
    if key not in _PAIR_RUNS:
        case, data = RR.ALL_CASES[name], case_data(name)
        with arithmetic('bf16', storage, **both):
            base = RC.run_chain(case, data, 'step', dest_fill=0.0)
        with arithmetic('bf16', storage, **dict(both, **{switch: False})):
            off = RC.run_chain(case, data, 'step', dest_fill=0.0)
        assert (_count(base, counter), _count(off, counter)) == (1, 0)
        for n in base['raw']:
            a, b = base['raw'][n].double(), off['raw'][n].double()
            if not torch.equal(a, b):
                log('RESBLOCK bf16/%s %s %s off%s: %s differs on %d of %d elements, max %.3e of max|.| %.3e' %
                    (storage, name, switch, ' (%s)' % both if both else '', n, int((a != b).sum()), a.numel(),
                     float((a - b).abs().max()) / float(b.abs().max()), float(b.abs().max())))
        _PAIR_RUNS[key] = (base, off)
    return _PAIR_RUNS[key]


def dgrad_pair_runs(name, storage):
    base, off = toggle_runs(name, storage, '_BF16_DGRAD_PAIR', 'conv_dgrad_bf16_s2_pair')
    assert _count(off, 'conv_dgrad_bf16_s2') == 2                       # conv1's, then the downsample's accumulating
    return base, off


@pytest.mark.parametrize('name', BF16_ENTRIES)
def test_bf16_entry_dgrad_in_one_launch_equals_its_two_launches_bit_for_bit(Fn, name):
    """_BF16_DGRAD_PAIR off with float storage, compared with torch.equal like the other switches.  (It was not, until this
    test: one accumulator over both sources summed in another order than the two launches -- a third of dx's elements
    differed, by 2.3e-7 of max|dx|; DESIGN_APPENDIX.md "BasicBlockFunction: every path".)"""
    base, off = dgrad_pair_runs(name, 'f32')
    assert_same_bits(base, off, '%s bf16/f32 with _BF16_DGRAD_PAIR off' % name)


@pytest.mark.parametrize('name', BF16_ENTRIES)
def test_bf16_storage_entry_dgrad_in_one_launch_against_its_two_launches(Fn, name):
    """_BF16_DGRAD_PAIR off with bf16 storage: everything but dx bit for bit (nothing else is computed from it), dx within
    2^-6 of max|dx|, what tests/test_bf16_storage_gpu.py holds conv_dgrad_bf16_s2_pair to against its two launches there (the
    first launch's stored sum is rounded to bf16 once more; bit for bit is asked of float storage)."""
    base, off = dgrad_pair_runs(name, 'bf16')
    diff = [n for n in base['raw'] if n != 'dx' and not torch.equal(base['raw'][n], off['raw'][n])]
    assert not diff, diff
    a, b = base['raw']['dx'].double(), off['raw']['dx'].double()
    assert float((a - b).abs().max()) <= 2.0 ** -6 * float(b.abs().max())


# _BN_PAIR with bf16 storage behind a two-term gradient: bn_bwd_pair(dout2=) hands the downsample's BatchNorm the sum
# dout + d2 as the kernel formed it; with _BN_PAIR off bn_bwd_two stores that masked sum as the tensor g, rounded to bf16,
# and the downsample's backward reads g.  The rounding split_dx is left out for, met through another switch: bit for bit
# (asked of float storage, where it holds on every row) is held here once split_dx is off on both sides, and a bf16 ulp as
# the step runs.
BF16_TWO_TERM_PAIRS = [n for n, e in RR.ARITH[('bf16', 'bf16')].items() if e.entry == RR.BF16 and RR.ALL_CASES[n].two]
_G_ROUNDED = ('dx', 'dest 0.downsample.0.weight', 'dest 0.downsample.1.weight', 'dest 0.downsample.1.bias')   # what g feeds


@pytest.mark.parametrize('name', BF16_TWO_TERM_PAIRS)
def test_bf16_storage_bn_pair_off_without_the_two_term_gradient_bit_for_bit(Fn, name):
    """_BN_PAIR off with split_dx off on both sides (the upstream gradient is one stored tensor either way): torch.equal."""
    base, off = toggle_runs(name, 'bf16', '_BN_PAIR', 'bn_fwd_pair', _SPLIT_DX=False)
    assert base['left'] == 0
    assert_same_bits(base, off, '%s bf16/bf16 with _BN_PAIR off, split_dx off in both' % name)


@pytest.mark.parametrize('name', BF16_TWO_TERM_PAIRS)
def test_bf16_storage_bn_pair_off_behind_a_two_term_gradient_to_a_bf16_ulp(Fn, name):
    """_BN_PAIR off as the step runs (split_dx on): everything the tensor g does not feed bit for bit; what it feeds (the
    downsample branch: its three parameter gradients and dx) to 2^-6 of the tensor's scale, the bound
    tests/test_bf16_storage_gpu.py holds the two-term kernels to with bf16 storage."""
    base, off = toggle_runs(name, 'bf16', '_BN_PAIR', 'bn_fwd_pair')
    assert base['left'] == 1 and base['calls']['bn_bwd_pair'] == [True] and len(off['calls']['bn_bwd_two']) == 1
    diff = [n for n in base['raw'] if n not in _G_ROUNDED and not torch.equal(base['raw'][n], off['raw'][n])]
    assert not diff, diff
    for n in _G_ROUNDED:
        a, b = base['raw'][n].double(), off['raw'][n].double()
        assert float((a - b).abs().max()) <= 2.0 ** -6 * float(b.abs().max()), n


# ---- the driver against the model ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nb,seq_len', [(40, 512), (8, 224)])
def test_the_drivers_flag_expressions_are_the_models(Fn, nb, seq_len):
    """A real resnet18() through breath_block (and, at seq_len 224, through head_operand): the flags ResNet._map passes to
    BasicBlockFunction.apply are the ones the driver's expressions give for those lengths."""
    import deepards_amd.models as M
    bb = M.resnet18().cuda().train()
    blocks, lens = bb._blocks(), bb._lengths(seq_len)
    x = torch.randn(nb, 1, seq_len, generator=torch.Generator().manual_seed(0)).cuda()
    seen = []
    orig = Fn.BasicBlockFunction.apply

    def spy(*a):
        seen.append((tuple(a[0].shape), a[10], a[11], a[15] is not None, bool(a[16]), bool(a[17]), bool(a[18])))
        return orig(*a)

    def drivers(fused):
        takes3 = [blk.takes_x3(nb, li, nb) for blk, li in zip(blocks, lens)] + [False]
        out = []
        for i, blk in enumerate(blocks):
            shape = (nb, lens[i], blk.conv1.in_channels)
            pool_out, split_dx = RC.flags(blocks, takes3, i, fused, lens[i] == 7, torch.empty(shape, device='meta'), nb)
            out.append((shape, blk.stride, nb, takes3[i], takes3[i + 1], pool_out and not takes3[i], split_dx and not takes3[i]))
        return out

    Fn.BasicBlockFunction.apply = spy
    try:
        with torch.no_grad():
            bb(x)
            assert seen == drivers(False), (seen, drivers(False))
            assert [s[6] for s in seen] == [False, True, False, True, False, True, False, True] and not any(s[5] for s in seen)
            if seq_len == 224:
                del seen[:]
                bb.head_operand(x, nb)
                assert seen == drivers(True), (seen, drivers(True))
                assert [s[5] for s in seen] == [False] * 7 + [True]         # R = 8, L = 7: Wn 56 has the pooled form
    finally:
        del Fn.BasicBlockFunction.apply
    assert 'apply' not in vars(Fn.BasicBlockFunction)
