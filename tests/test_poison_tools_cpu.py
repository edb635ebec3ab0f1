"""tests/tools/poison.py would fail on a wrong kernel: planted faults, written in plain torch on CPU tensors, each caught by
exactly the check meant for it, and the correct op passing all five.  The checks other than the poisoned one run on
deterministic all-zero "fresh" memory (poisoned_allocations(fill=0)): the accident a test process usually provides, and
the reason the faults below are invisible to parity tests."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from tools import poison as P  # noqa: E402

ROWS, L = 6, 5


def _slack(t):
    """t with zero-filled allocator slack on both sides: where an exact-size tensor's overrun lands unnoticed."""
    big = torch.zeros(t.numel() + 16)
    v = big[8:8 + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def _inputs(with_out=True):
    def build():
        g = torch.Generator().manual_seed(3)
        d = {'x': _slack(torch.randn(ROWS, L, generator=g)), 'w': torch.randn(L, generator=g)}
        if with_out:
            d['out'] = _slack(torch.zeros(ROWS, L))
        return d
    return build


def _flat(t, extra_front=0, extra_back=0):
    """The elements of t with some in front of / behind it in its storage (what a kernel's pointer arithmetic reaches)."""
    assert t.is_contiguous()
    return torch.as_strided(t, (t.numel() + extra_front + extra_back,), (1,), t.storage_offset() - extra_front)


def op_good(x, w, out):
    out.copy_(x * w)
    return out


def op_writes_past(x, w, out):
    out.copy_(x * w)
    _flat(out, 0, 1)[-1] = 1.0
    return out


def op_writes_before(x, w, out):
    out.copy_(x * w)
    _flat(out, 1, 0)[0] = 1.0
    return out


def op_last_unwritten(x, w):
    out = torch.empty(x.shape)
    out.view(-1)[:-1] = (x * w).view(-1)[:-1]
    return out


def op_good_alloc(x, w):
    out = torch.empty(x.shape)
    out.copy_(x * w)
    return out


def op_adds_into_out(x, w, out):
    out += x * w                     # "out was zeroed" -- it was, by build(); not by a caller that recycles memory
    return out


def op_folds_unwritten_scratch(x, w):
    scratch = torch.empty((ROWS + 1, L))         # one slab more than the splits write
    scratch[:ROWS] = x * w
    return scratch.sum(0)


def op_good_fold(x, w):
    scratch = torch.empty((ROWS, L))
    scratch[:ROWS] = x * w
    return scratch.sum(0)


def op_reads_past_input(x, w, out):
    beyond = _flat(x, 0, 1)[-1]                   # one element past the input, times zero
    out.copy_(x * w + 0.0 * beyond)
    return out


def op_reads_neighbour_row(x, w, out):
    out.copy_(x * w + 0.0 * torch.roll(x, -1, 0))  # the next row, times zero
    return out


_PLANS = {}


def op_caches_plan_by_rank(x, w, out):
    n = _PLANS.get(x.dim(), x.shape[0])           # a "plan" keyed by too little: the row count of the call before
    _PLANS[x.dim()] = x.shape[0]
    out.zero_()
    out[:n] = (x * w)[:n]
    return out


ISO = dict(inputs=('x',), R=1)


def _case(name, fn, with_out=True, rows=ISO, build=None):
    return P.OpCase(name, 'fake', build or _inputs(with_out), fn, dests=('out',) if with_out else (), rows=rows)


def _other():
    def build():
        return {'x': torch.ones(2, L), 'w': torch.ones(L), 'out': torch.zeros(2, L)}
    return P.OpCase('other_shape', 'fake', build, op_caches_plan_by_rank, dests=('out',))


def _run_all(case, other=None):
    failed = set()
    report = {}
    for check in P.CHECKS:
        if check == 'uninitialised':
            problems = P.run_check(check, case, other)
        else:
            with P.poisoned_allocations(fill=0):              # deterministic "fresh memory is zero"
                problems = P.run_check(check, case, other)
        report[check] = problems
        if problems:
            failed.add(check)
    return failed, report


@pytest.mark.parametrize('fn,with_out', [(op_good, True), (op_good_alloc, False), (op_good_fold, False)])
def test_correct_ops_pass_every_check(fn, with_out):
    rows = None if fn is op_good_fold else ISO
    failed, report = _run_all(_case(fn.__name__, fn, with_out, rows), _case('again', op_good))
    assert not failed, report


@pytest.mark.parametrize('fn,with_out,rows,meant', [
    (op_writes_past, True, ISO, 'guards'),
    (op_writes_before, True, ISO, 'guards'),
    (op_last_unwritten, False, ISO, 'uninitialised'),
    (op_adds_into_out, True, ISO, 'dirty_out'),
    (op_folds_unwritten_scratch, False, None, 'uninitialised'),
    (op_reads_past_input, True, ISO, 'guards'),
    (op_reads_neighbour_row, True, ISO, 'isolation'),
])
def test_each_planted_fault_is_caught_by_exactly_its_check(fn, with_out, rows, meant):
    failed, report = _run_all(_case(fn.__name__, fn, with_out, rows), _case('again', op_good))
    assert failed == {meant}, report
    text = ' '.join(report[meant])
    assert fn.__name__ in text and ('differ' in text or 'guard' in text or 'pattern' in text), text


def test_a_plan_cached_from_another_shape_is_caught_by_the_repeat_check():
    _PLANS.clear()
    case = _case('op_caches_plan_by_rank', op_caches_plan_by_rank)
    _PLANS.clear()
    assert not P.check_repeat(case, None)
    _PLANS.clear()
    problems = P.check_repeat(case, _other())
    assert problems and 'repeat after other_shape' in problems[0], problems


def test_shape_signature_tells_shapes_apart_and_nothing_else():
    """Check 5 picks its in-between case by this: the same operand shapes under another name or in another order are the
    same shape, another row count is not."""
    a, b = _case('a', op_good), _case('b', op_adds_into_out)
    assert P.shape_signature(a) == P.shape_signature(b)
    assert P.shape_signature(a) != P.shape_signature(_other())
    swapped = P.OpCase('swapped', 'fake', lambda: {'w': torch.ones(L), 'out': torch.zeros(ROWS, L), 'x': torch.ones(ROWS, L)}, op_good)
    assert P.shape_signature(swapped) == P.shape_signature(a)


def test_called_wrappers_sees_what_the_call_reaches_and_restores_the_module():
    import types
    mod = types.ModuleType('fake_ops')
    mod.inner = lambda x: x * 2
    mod.outer = lambda x: mod.inner(x) + 1                    # reaches inner through the module, as hip_ops does
    mod.unused = lambda x: x
    before = dict(vars(mod))
    case = P.OpCase('c', 'fake', lambda: {'x': mod.unused(torch.ones(3))}, lambda x: mod.outer(x))    # build() does not count
    assert P.called_wrappers(case, mod, ['inner', 'outer', 'unused']) == {'inner', 'outer'}
    assert dict(vars(mod)) == before
    boom = P.OpCase('boom', 'fake', lambda: {'x': torch.ones(3)}, lambda x: mod.outer(None))
    with pytest.raises(TypeError):
        P.called_wrappers(boom, mod, ['inner', 'outer'])
    assert dict(vars(mod)) == before


def test_isolation_refuses_a_case_of_one_window():
    """One window has no neighbour: a row that asks for the check anyway is a mistake in the table, not a pass."""
    one = P.OpCase('one', 'fake', lambda: {'x': torch.ones(1, L), 'w': torch.ones(L), 'out': torch.zeros(1, L)}, op_good, rows=ISO)
    with pytest.raises(AssertionError, match='one window'):
        P.check_isolation(one)


def test_guard_messages_name_the_side_and_the_first_word():
    t = torch.arange(12.).view(3, 4)
    v, h = P.guarded(t, name='t')
    assert P.same_bits(v, t) and v.stride() == t.stride() and v.data_ptr() % 256 == 0
    assert (h.offset * 4) >= 4096 and (h.buf.numel() - h.offset - h.span) * 4 >= 4096
    P.assert_guards_intact(h)
    h.buf[h.offset - 2] = float('nan')              # *a* NaN is not the pattern
    msg = P.guard_report(h)
    assert 'in front of' in msg and 'first 2 elements' in msg and '1 elements changed' in msg, msg
    with pytest.raises(AssertionError):
        P.assert_guards_intact(h)
    v, h = P.guarded(t)
    h.buf[h.offset + h.span] = 0.0
    assert 'behind' in P.guard_report(h) and 'first 1 elements' in P.guard_report(h)


def test_guard_is_at_least_one_full_row():
    t = torch.zeros(2, 700, 32)                     # a row of 700 x 32 floats = 89600 bytes > 4 KiB
    v, h = P.guarded(t)
    assert h.offset >= 700 * 32 and h.buf.numel() - h.offset - h.span >= 700 * 32
    assert v.is_contiguous() and v.data_ptr() % 256 == 0


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float64, torch.int64, torch.int32, torch.float16])
def test_patterns_per_dtype(dtype):
    t = P.fill_poison(torch.empty((7,), dtype=dtype))
    assert P.has_poison(t) and P.count_poison(t) == 7 and P.same_bits(t, t.clone())
    if dtype.is_floating_point:
        assert torch.isnan(t.float()).all()
        other = torch.full((7,), float('nan'), dtype=dtype)
        assert not P.has_poison(other) and not P.same_bits(t, other)       # a NaN, not the pattern
        assert P.diff_report(t, other).startswith('7 of 7 elements differ, first at flat index 0')
    else:
        assert bytes(t.view(torch.uint8).tolist()) == bytes([P.POISON_BYTE]) * (7 * t.element_size())
    v, h = P.guarded(torch.zeros((3, 5), dtype=dtype))
    assert not P.has_poison(v) and P.has_poison(h.buf)
    P.assert_guards_intact(h)


def test_float32_pattern_is_written_through_the_int32_view():
    t = P.fill_poison(torch.empty((4,)))
    assert t.view(torch.int32).tolist() == [P.POISON] * 4 and P.POISON == 0x7fc0dead


def test_pitched_slice_sits_in_a_poisoned_buffer():
    t = torch.arange(2 * 3 * 4.).view(2, 3, 4)
    v, h = P.pitched(t, 12, off=4)
    assert P.same_bits(v.contiguous(), t) and v.stride() == (36, 12, 1) and (v.data_ptr() - 16) % 256 == 0
    P.assert_guards_intact(h)
    h.buf[h.offset + 4] = 0.0                       # the channel right of the slice, first position
    assert 'between the rows' in P.guard_report(h)


def test_patch_reaches_the_three_allocators_and_nothing_else():
    base = torch.ones(3)
    with P.poisoned_allocations() as stats:
        a, b, c = torch.empty((2, 3)), torch.empty_like(base), base.new_empty((4,))
        d = torch.empty((2, 3), dtype=torch.bfloat16)
        e = torch.empty((3,), dtype=torch.int64)
        z, o = torch.zeros(3), torch.ones(3)
        n = torch.empty((0,))
    assert stats.filled == 5 and n.numel() == 0
    assert all(P.count_poison(t) == t.numel() for t in (a, b, c, d, e))
    assert d.view(torch.int16)[0, 0].item() == P.POISON_BF16 and e[0].item() == 0x5A5A5A5A5A5A5A5A
    assert not P.has_poison(z) and not P.has_poison(o) and float(o.sum()) == 3.0


def test_patch_is_restored_after_an_exception():
    before = (torch.empty, torch.empty_like, torch.Tensor.new_empty, 'new_empty' in torch.Tensor.__dict__)
    with pytest.raises(RuntimeError):
        with P.poisoned_allocations():
            assert torch.empty is not before[0]
            raise RuntimeError('inside')
    after = (torch.empty, torch.empty_like, torch.Tensor.new_empty, 'new_empty' in torch.Tensor.__dict__)
    assert after == before
    assert torch.ones(2).new_empty((3,)).shape == (3,)


def test_module_level_references_are_resolved_at_call_time():
    """hip_ops calls ``torch.empty(...)`` through the module attribute, so the patch reaches it."""
    import inspect
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from deepards_amd import hip_ops, functional, train
    for mod in (hip_ops, functional, train):
        src = inspect.getsource(mod)
        assert 'from torch import' not in src, mod.__name__
