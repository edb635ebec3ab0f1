"""Memory-discipline helpers: poisoned allocations, guard bands and the five checks that use them.

A kernel that depends on what a fresh ``torch.empty`` happens to hold, writes beside its output, reads beside its operands
into arithmetic, adds into a destination it assumed was zero, or lets one row leak into another computes the right numbers
in a test process, where fresh memory is mostly zero and operands sit in exact-size tensors.  The helpers here take those
accidents away; every comparison is bit for bit through integer views, so a NaN equals itself and *a* NaN is not *the*
pattern.

    POISON                    the quiet-NaN bit pattern of float32 words (bf16: POISON_BF16; integers: POISON_BYTE bytes)
    poisoned_allocations()    context manager: torch.empty / torch.empty_like / Tensor.new_empty return pattern-filled memory
    guarded(t) / pitched(t)   t inside a larger pattern-filled allocation (+ a handle for assert_guards_intact)
    has_poison / same_bits    integer-view comparisons
    OpCase, check_*           one table row of an op and the five checks over it (tests/test_memory_discipline_gpu.py on
                              the HIP wrappers, tests/test_poison_tools_cpu.py on planted faults in plain torch)
"""
import contextlib

import torch

POISON = 0x7fc0dead          # float32: a quiet NaN with a payload no arithmetic produces
POISON_BF16 = 0x7fc1         # bfloat16: a quiet NaN
POISON_F16 = 0x7e01          # float16: a quiet NaN
POISON_F64 = 0x7ff8dead7fc0dead
POISON_BYTE = 0x5A           # integer / bool tensors: every byte

_MIN_GUARD_BYTES = 4096
_ALIGN = 256


def _pattern(dtype):
    """-> (integer view dtype, the pattern as a value of it)."""
    if dtype == torch.float32:
        return torch.int32, POISON
    if dtype == torch.bfloat16:
        return torch.int16, POISON_BF16
    if dtype == torch.float16:
        return torch.int16, POISON_F16
    if dtype == torch.float64:
        return torch.int64, POISON_F64
    size = dtype.itemsize
    view = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[size]
    return view, int.from_bytes(bytes([POISON_BYTE]) * size, 'little')


def _bits(t):
    """An integer view (or, for a non-contiguous tensor, an integer copy) of t's elements."""
    view, _ = _pattern(t.dtype)
    if not t.is_contiguous():
        t = t.contiguous()
    return t.view(view) if t.dtype != view else t


def fill_poison(t):
    """Fill a contiguous tensor with the pattern of its dtype, in place."""
    view, value = _pattern(t.dtype)
    (t.view(view) if t.dtype != view else t).fill_(value)
    return t


def has_poison(t):
    if t is None or t.numel() == 0:
        return False
    _, value = _pattern(t.dtype)
    return bool((_bits(t) == value).any())


def count_poison(t):
    _, value = _pattern(t.dtype)
    return int((_bits(t) == value).sum())


def same_bits(a, b):
    if (a is None) != (b is None):
        return False
    if a is None:
        return True
    return a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape) and a.device == b.device and bool((_bits(a) == _bits(b)).all())


def diff_report(a, b):
    """'' when a and b have the same bits, else a line with the first differing flat index, the count and the two values."""
    if (a is None) != (b is None):
        return 'one is None: %s vs %s' % (type(a).__name__, type(b).__name__)
    if a is None:
        return ''
    if a.dtype != b.dtype or tuple(a.shape) != tuple(b.shape):
        return 'dtype / shape %s %s vs %s %s' % (a.dtype, tuple(a.shape), b.dtype, tuple(b.shape))
    if a.numel() == 0:
        return ''
    ne = (_bits(a) != _bits(b)).reshape(-1)
    n = int(ne.sum())
    if n == 0:
        return ''
    first = int(torch.nonzero(ne)[0])
    av, bv = a.contiguous().reshape(-1)[first].item(), b.contiguous().reshape(-1)[first].item()
    return '%d of %d elements differ, first at flat index %d (shape %s): %r vs %r' % (n, ne.numel(), first, tuple(a.shape), av, bv)


# ---- poisoned allocations --------------------------------------------------------------------------------------------------
class _Stats(object):
    def __init__(self):
        self.filled = 0         # allocations the patch filled


@contextlib.contextmanager
def poisoned_allocations(fill=None):
    """Replace torch.empty, torch.empty_like and Tensor.new_empty for the duration: every contiguous non-empty result comes
    back filled with the pattern of its dtype.  torch.zeros and the rest of torch are untouched; the originals are restored
    in ``finally``.  -> an object whose ``filled`` counts the allocations the patch reached.
    ``fill`` (tests of this module only): a plain value instead of the pattern -- fill=0 models the all-zero fresh memory of
    a test process deterministically."""
    stats = _Stats()
    o_empty, o_like = torch.empty, torch.empty_like
    had_new = 'new_empty' in torch.Tensor.__dict__
    o_new = torch.Tensor.new_empty

    def _fill(t):
        if isinstance(t, torch.Tensor) and t.numel() > 0 and t.is_contiguous() and t.layout == torch.strided:
            if fill is None:
                fill_poison(t)
            else:
                t.fill_(fill)
            stats.filled += 1
        return t

    def p_empty(*a, **k):
        return _fill(o_empty(*a, **k))

    def p_like(*a, **k):
        return _fill(o_like(*a, **k))

    def p_new(self, *a, **k):
        return _fill(o_new(self, *a, **k))

    torch.empty, torch.empty_like, torch.Tensor.new_empty = p_empty, p_like, p_new
    try:
        yield stats
    finally:
        torch.empty, torch.empty_like = o_empty, o_like
        if had_new:
            torch.Tensor.new_empty = o_new
        else:
            del torch.Tensor.new_empty


# ---- guard bands -----------------------------------------------------------------------------------------------------------
class Guard(object):
    """What guarded() made: ``buf`` the whole 1-D allocation, ``view`` the tensor inside it, ``offset`` (elements) where
    the view starts, ``span`` (elements) its extent."""

    def __init__(self, buf, view, offset, span, name):
        self.buf, self.view, self.offset, self.span, self.name = buf, view, offset, span, name


def _span(shape, strides):
    return 1 + sum((n - 1) * s for n, s in zip(shape, strides)) if all(n > 0 for n in shape) else 0


def _guard_elems(t, strides, want, esize):
    """Elements of one guard: at least one full row (the extent of t[0]) and 4 KiB, a multiple of the alignment."""
    row = _span(tuple(t.shape[1:]), tuple(strides[1:])) if t.dim() >= 2 else _span(tuple(t.shape), tuple(strides))
    if t.dim() >= 2 and t.shape[0] > 1:
        row = max(row, strides[0])
    nbytes = max(row * esize, _MIN_GUARD_BYTES, (want or 0) * esize)
    nbytes = (nbytes + _ALIGN - 1) // _ALIGN * _ALIGN
    return nbytes // esize


def _place(t, shape, strides, inner_off, front, back, name):
    esize = t.element_size()
    span = _span(shape, strides) + inner_off
    gf, gb = _guard_elems(t, strides, front, esize), _guard_elems(t, strides, back, esize)
    pad = _ALIGN // esize
    buf = fill_poison(torch.empty((gf + span + gb + pad,), dtype=t.dtype, device=t.device))
    base = buf.data_ptr()
    shift = (-(base + gf * esize)) % _ALIGN
    assert shift % esize == 0
    start = gf + shift // esize                   # the (pitched) buffer starts here, 256-byte aligned
    view = buf.as_strided(shape, strides, start + inner_off)
    view.copy_(t)
    assert (buf.data_ptr() + start * esize) % _ALIGN == 0
    return view, Guard(buf, view, start + inner_off, _span(shape, strides), name)


def guarded(t, front=None, back=None, name=''):
    """-> (view, handle): a tensor equal to ``t`` -- same shape, same strides, 256-byte aligned data pointer -- inside a
    larger 1-D allocation filled with the pattern.  Each guard is at least the larger of one full row of t (L x pitch), 4 KiB
    and ``front`` / ``back`` elements, so an overrun by a tile row still lands inside this allocation.  For a strided ``t``
    (a channel slice) the elements between its rows belong to the guard as well."""
    assert t.numel() > 0, 'guarded: empty tensor'
    strides = tuple(t.stride())
    if t.is_contiguous():                         # normalise the strides of size-1 dimensions
        strides = tuple(torch.empty(t.shape, dtype=t.dtype, device='meta').stride())
    return _place(t, tuple(t.shape), strides, 0, front, back, name)


def pitched(t, ld, off=0, front=None, back=None, name=''):
    """-> (view, handle): contiguous (rows, L, C) ``t`` as the channel slice [off, off + C) of a pattern-filled
    (rows, L, ld) buffer inside guard bands: whatever a kernel reads beside its slice poisons its result, whatever it writes
    beside it breaks the guard."""
    rows, l, c = t.shape
    assert off >= 0 and off + c <= ld
    return _place(t.contiguous(), (rows, l, c), (l * ld, ld, 1), off, front, back, name)


def guard_report(handle):
    """'' when every element of the allocation outside the view still holds the pattern, else which words changed."""
    view, value = _pattern(handle.buf.dtype)
    bits = (handle.buf.view(view) if handle.buf.dtype != view else handle.buf).clone()
    bits.as_strided(tuple(handle.view.shape), tuple(handle.view.stride()), handle.offset).fill_(value)
    bad = bits != value
    n = int(bad.sum())
    if n == 0:
        return ''
    idx = torch.nonzero(bad).reshape(-1)
    first, last = int(idx[0]), int(idx[-1])
    lo, hi = handle.offset, handle.offset + handle.span
    where = 'in front of' if first < lo else 'behind' if first >= hi else 'between the rows of'
    return 'guard of %s: %d elements changed, first %d elements %s the tensor (buffer index %d, last %d; tensor at [%d, %d))' % (
        handle.name or 'tensor', n, (lo - first) if first < lo else (first - hi + 1) if first >= hi else first - lo, where,
        first, last, lo, hi)


def assert_guards_intact(handle):
    for h in (handle if isinstance(handle, (list, tuple)) else [handle]):
        msg = guard_report(h)
        assert not msg, msg


# ---- op cases and the five checks ------------------------------------------------------------------------------------------
def map_tensors(obj, fn, path=''):
    """obj with fn(tensor, path) applied to every tensor inside lists / tuples / dicts; one result per distinct tensor
    object, so an operand passed twice stays one operand."""
    memo = {}

    def go(o, p):
        if isinstance(o, torch.Tensor):
            if id(o) not in memo:
                memo[id(o)] = fn(o, p)
            return memo[id(o)]
        if isinstance(o, dict):
            return {k: go(v, '%s.%s' % (p, k) if p else str(k)) for k, v in o.items()}
        if isinstance(o, (list, tuple)):
            return type(o)(go(v, '%s[%d]' % (p, i)) for i, v in enumerate(o))
        return o

    return go(obj, path)


def flatten(obj, path=''):
    """[(path, tensor or None)] of every tensor (and None leaf) inside lists / tuples / dicts."""
    if isinstance(obj, torch.Tensor) or obj is None:
        return [(path, obj)]
    if isinstance(obj, dict):
        return [kv for k, v in obj.items() for kv in flatten(v, '%s.%s' % (path, k) if path else str(k))]
    if isinstance(obj, (list, tuple)):
        return [kv for i, v in enumerate(obj) for kv in flatten(v, '%s[%d]' % (path, i))]
    return []


class OpCase(object):
    """One row of an op table.

    name, family   the id of the case and the kernel family it belongs to (check 5 runs a different-shaped case of the
                   family in between)
    build()        -> dict of seeded inputs (tensors, lists / tuples of them, plain values); fresh on every call
    call(**inputs) -> the PUBLIC results: a tensor, or a tuple / list / dict of tensors (None entries allowed).  Padding a
                   header documents as unwritten is sliced off here; in-place operands are returned here
    dests          names of inputs (tensors or lists of tensors) the op overwrites completely (out / dx / dw with
                   accumulate=False): check 3 pre-fills them with the pattern; build() hands them over zero-filled
    rows           None (the op reduces over rows: exempt from check 4) or dict(inputs=names of inputs with a row axis 0,
                   R=rows per independent window, axis={result path: window axis, or None for a result that reduces over rows},
                   mid=the middle window to try (default: the window count // 2)); a case of one window has no neighbour
                   and takes None
    note           why a row is shaped as it is (replaced shapes, documented padding)"""

    def __init__(self, name, family, build, call, dests=(), rows=None, note='', setup=None):
        self.name, self.family, self.build, self.call = name, family, build, call
        self.dests, self.rows, self.note, self.setup = tuple(dests), rows, note, setup

    def run(self, inputs):
        if self.setup is None:
            return self.call(**inputs)
        with self.setup():
            return self.call(**inputs)

    def __repr__(self):
        return 'OpCase(%s)' % self.name


def _sync(obj):
    for _, t in flatten(obj):
        if t is not None and t.is_cuda:
            torch.cuda.synchronize()
            return


def compare(case, what, got, clean, skip=None):
    """-> problems: every public result of ``got`` against ``clean``, bit for bit."""
    problems = []
    g, c = flatten(got), flatten(clean)
    if [p for p, _ in g] != [p for p, _ in c]:
        return ['%s / %s: result structure %s vs %s' % (case.name, what, [p for p, _ in g], [p for p, _ in c])]
    for (path, a), (_, b) in zip(g, c):
        if skip is not None:
            a, b = skip(path, a, b)
        msg = diff_report(a, b)
        if msg:
            problems.append('%s / %s: result %s: %s' % (case.name, what, path or '0', msg))
    return problems


def clean_run(case):
    out = case.run(case.build())
    _sync(out)
    return out


def check_uninitialised(case, clean=None):
    """Check 1: under poisoned_allocations() every public result has the bits of the clean run and none holds the pattern."""
    clean = clean_run(case) if clean is None else clean
    inputs = case.build()
    with poisoned_allocations():
        got = case.run(inputs)
        _sync(got)
    problems = compare(case, 'poisoned allocations', got, clean)
    for path, t in flatten(got):
        if t is not None and has_poison(t):
            problems.append('%s / poisoned allocations: result %s holds the pattern in %d of %d elements' %
                            (case.name, path or '0', count_poison(t), t.numel()))
    return problems


def check_guards(case, clean=None):
    """Check 2: every tensor operand inside guard bands (destinations included, zero-filled as build() made them): same
    bits as clean, every guard intact."""
    clean = clean_run(case) if clean is None else clean
    handles = []

    def wrap(t, path):
        if t.numel() == 0:
            return t
        v, h = guarded(t, name=path)
        handles.append(h)
        return v

    inputs = map_tensors(case.build(), wrap)
    got = case.run(inputs)
    _sync(got)
    problems = compare(case, 'guard bands', got, clean)
    for h in handles:
        msg = guard_report(h)
        if msg:
            problems.append('%s / guard bands: %s' % (case.name, msg))
    return problems


def check_dirty_out(case, clean=None):
    """Check 3: every destination pre-filled with the pattern: the result has the bits of the clean run."""
    if not case.dests:
        return []
    clean = clean_run(case) if clean is None else clean
    inputs = case.build()
    for name in case.dests:
        for _, t in flatten(inputs[name]):          # a destination, or a list of them
            if t is None:
                continue
            if t.is_contiguous():
                fill_poison(t)
            else:
                t.copy_(fill_poison(torch.empty(t.shape, dtype=t.dtype, device=t.device)))
    got = case.run(inputs)
    _sync(got)
    return compare(case, 'dirty destination', got, clean)


def isolation_windows(case, inputs):
    spec = case.rows
    rows = inputs[spec['inputs'][0]].shape[0]
    w = rows // spec.get('R', 1)
    mid = spec.get('mid', w // 2)
    return w, sorted(set([0, min(mid, w - 1), w - 1]))


def check_isolation(case, clean=None):
    """Check 4: one window of R input rows overwritten with NaN (the first, a middle and the last one): every other window
    of every result has the bits of the clean run."""
    spec = case.rows
    if spec is None:
        return []
    clean = clean_run(case) if clean is None else clean
    R = spec.get('R', 1)
    axes = spec.get('axis', {})
    w, victims = isolation_windows(case, case.build())
    assert w >= 2, '%s: one window has no neighbour to isolate it from -- such a row takes rows=None' % case.name
    problems = []
    for victim in victims:
        inputs = case.build()
        for name in spec['inputs']:
            t = inputs[name]
            assert t.shape[0] == w * R, '%s: input %s has %d rows, not %d windows of %d' % (case.name, name, t.shape[0], w, R)
            if t.is_floating_point():
                t[victim * R:(victim + 1) * R] = float('nan')
            else:
                raise AssertionError('%s: isolation input %s is not floating point' % (case.name, name))
        got = case.run(inputs)
        _sync(got)

        def others(path, a, b):
            ax = axes.get(path, 0)
            if a is None or ax is None:
                return None, None
            assert a.shape[ax] % w == 0, '%s: result %s axis %d (%d) is not a multiple of %d windows' % (case.name, path, ax, a.shape[ax], w)
            per = a.shape[ax] // w
            keep = [i for i in range(a.shape[ax]) if i // per != victim]
            idx = torch.tensor(keep, device=a.device, dtype=torch.long)
            return a.index_select(ax, idx), b.index_select(ax, idx)

        problems += compare(case, 'NaN in window %d of %d' % (victim, w), got, clean, skip=others)
    return problems


def shape_signature(case):
    """The shapes and types of every tensor operand build() makes, in any order: two cases with the same signature run the
    same shape (a forward and the data gradient of one conv, one shape under two debug settings)."""
    return tuple(sorted((tuple(t.shape), str(t.dtype)) for _, t in flatten(case.build()) if t is not None))


def called_wrappers(case, module, names):
    """-> the ``names`` of ``module`` that one clean run of case.call() reaches (build() does not count), found by wrapping
    each with a recorder for the duration; calls the module makes through its own globals are seen as well."""
    seen, saved = set(), {n: getattr(module, n) for n in names}

    def recorder(n, fn):
        def wrapped(*a, **k):
            seen.add(n)
            return fn(*a, **k)
        return wrapped

    inputs = case.build()
    for n, fn in saved.items():
        setattr(module, n, recorder(n, fn))
    try:
        _sync(case.run(inputs))
    finally:
        for n, fn in saved.items():
            setattr(module, n, fn)
    return seen


def check_repeat(case, other, clean=None):
    """Check 5: the op again after a different-shaped case of its family ran: the bits of its first call."""
    first = clean_run(case) if clean is None else clean
    if other is not None:
        _sync(other.run(other.build()))
    again = clean_run(case)
    return compare(case, 'repeat after %s' % (other.name if other is not None else 'nothing'), again, first)


CHECKS = ('uninitialised', 'guards', 'dirty_out', 'isolation', 'repeat')


def run_check(check, case, other=None):
    if check == 'uninitialised':
        return check_uninitialised(case)
    if check == 'guards':
        return check_guards(case)
    if check == 'dirty_out':
        return check_dirty_out(case)
    if check == 'isolation':
        return check_isolation(case)
    if check == 'repeat':
        return check_repeat(case, other)
    raise ValueError(check)
