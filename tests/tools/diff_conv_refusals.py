"""Differential check of the convolution entry points' refusals between two builds of the library.

    python -m tests.tools.diff_conv_refusals --other /path/to/other/libdeepards_hip.so

Loads this tree's build (deepards_amd._lib, DA_LIB_PATH honoured) and ``--other`` side by side and calls da_conv3_winograd,
da_conv3_winograd4, da_conv3_winograd_drop, da_conv3_winograd_bn, da_conv3_bf16, da_conv3_bf16_bn, da_conv_gemm,
da_conv_gemm_multi and da_conv_bf16_multi with an argument grid of calls that are REFUSED (DA_EINVAL) or empty (rows == 0,
DA_OK): every operand is a dummy non-null address and every call returns before a launch, so no GPU is needed.  The
return codes must agree call by call; any code other than DA_EINVAL / DA_OK means a call got through to a launch and is
an error of the grid.  Prints the call count.

The grid reaches every ``return DA_EINVAL`` of those functions but three that no argument list reaches: the F(4,3) refusal
of dropout / statistics / a folded BatchNorm in conv3_winograd_impl (no entry point asks for them), its ``in_Wu < 64``
(R * L < 64 has R * ceil(L / 2) < 64, refused in front of it) and the ``default:`` of conv_gemm_dispatch's tile choice (a
channel count that is a multiple of 32 always has a candidate).
"""
import argparse
import ctypes
import itertools
import sys

P = 4096            # a dummy non-null device address; never dereferenced
BIG = 1 << 30


def _grid(base, singles, pairs=()):
    """base: {name: value}; singles: {name: [values]} -- one field changed at a time; pairs: [(name, name)] -- every
    combination of the two fields' values as well."""
    yield dict(base)
    for k, vals in singles.items():
        for v in vals:
            yield dict(base, **{k: v})
    for a, b in pairs:
        for va, vb in itertools.product(singles[a], singles[b]):
            yield dict(base, **{a: va, b: vb})


_SHAPE = {'x': [None], 'u': [None], 'y': [None], 'rows': [-1, 0, -40], 'L': [0, -3], 'C': [0, 16, 33, 48, 96 + 1, -32],
          'N': [0, 16, 32 + 1, 65, 100, -64], 'ldx': [32, 60, 66, 67, 63], 'ldy': [0, 32, 63]}
_SHAPE_PAIRS = [('rows', 'C'), ('rows', 'N'), ('rows', 'ldx'), ('rows', 'L'), ('C', 'ldx'), ('N', 'ldy'), ('C', 'N'), ('x', 'rows')]


def wino_calls():
    """da_conv3_winograd / da_conv3_winograd4: (x, u, y, rows, L, ldx, C, ldy, N, accumulate, stream)."""
    base = dict(x=P, u=P, y=P, rows=40, L=56, ldx=64, C=64, ldy=64, N=64, acc=0)
    limits = [dict(base, rows=1 << 16, L=1 << 10), dict(base, rows=1 << 20, L=56), dict(base, rows=1, L=1 << 18, ldx=64),
              dict(base, rows=1, L=1 << 19), dict(base, rows=2, L=1 << 18), dict(base, rows=1 << 10, L=1 << 10, ldx=4096, C=64),
              dict(base, rows=4, L=(1 << 18) + 8, ldx=32, C=32, ldy=32, N=32), dict(base, rows=1, L=1 << 18, ldx=32, C=32, ldy=32, N=32)]
    for name in ('da_conv3_winograd', 'da_conv3_winograd4'):
        for act in (0, 1):
            for a in itertools.chain(_grid(base, dict(_SHAPE, acc=[1]), _SHAPE_PAIRS), limits):
                if act == 0 and a == base:
                    continue                                  # the one valid call: it would launch
                if act == 0 and a['acc'] == 1 and all(a[k] == base[k] for k in base if k != 'acc'):
                    continue
                yield name, act, (a['x'], a['u'], a['y'], a['rows'], a['L'], a['ldx'], a['C'], a['ldy'], a['N'], a['acc'], None)


def wino_drop_calls():
    """da_conv3_winograd_drop: (x, u, y, rows, L, ldx, C, ldy, N, drop_seed, drop_salt, drop_p, stat_part, R, stream)."""
    base = dict(x=P, u=P, y=P, rows=40, L=56, ldx=64, C=64, ldy=64, N=64, seed=P, salt=7, p=0.2, part=P, R=20)
    more = {'seed': [None], 'p': [-0.1, 1.0, 1.5], 'R': [0, -1, 3, 7, 1], 'part': [None]}
    pairs = _SHAPE_PAIRS + [('R', 'rows'), ('p', 'rows'), ('R', 'L'), ('seed', 'p'), ('R', 'C')]
    for act in (0, 1):
        for a in _grid(base, dict(_SHAPE, **more), pairs):
            valid = all(a[k] == base[k] for k in base if k not in ('part', 'R')) and (a['part'] is None or a['R'] == 20)
            if act == 0 and valid:
                continue                                      # (no records: R is not looked at)
            yield 'da_conv3_winograd_drop', act, (a['x'], a['u'], a['y'], a['rows'], a['L'], a['ldx'], a['C'], a['ldy'], a['N'],
                                                  a['seed'], a['salt'], a['p'], a['part'], a['R'], None)
        # windows shorter than a tile of 64 pairs: R * ceil(L / 2) < 64
        for R, L in [(1, 56), (2, 56), (2, 62), (1, 126), (4, 30), (1, 1)]:
            yield 'da_conv3_winograd_drop', act, (P, P, P, 40, L, 64, 64, 64, 64, P, 7, 0.2, P, R, None)


def wino_bn_calls():
    """da_conv3_winograd_bn: (x, u, y, rows, L, C, ldy, N, R, in_pend, in_mean, in_invstd, gamma, beta, eps, drop_seed,
    drop_salt, drop_p, stat_part, stream)."""
    base = dict(x=P, u=P, y=P, rows=40, L=56, C=64, ldy=64, N=64, R=20, pend=P, mean=P, invstd=P, gamma=P, beta=P, seed=P, p=0.2, part=P)
    shape = {k: v for k, v in _SHAPE.items() if k != 'ldx'}
    more = {'R': [0, -1, 3, 7, 1], 'pend': [None], 'mean': [None], 'invstd': [None], 'gamma': [None], 'beta': [None],
            'seed': [None], 'p': [-0.1, 1.0], 'part': [None], 'C': shape['C'] + [160, 256]}
    pairs = [('rows', 'C'), ('rows', 'N'), ('R', 'rows'), ('R', 'L'), ('C', 'N'), ('pend', 'rows'), ('mean', 'R'), ('part', 'R'), ('part', 'C')]
    for act in (0, 1):
        for a in _grid(base, dict(shape, **more), pairs):
            if act == 0 and all(a[k] == base[k] for k in base if k != 'part'):
                continue
            yield 'da_conv3_winograd_bn', act, (a['x'], a['u'], a['y'], a['rows'], a['L'], a['C'], a['ldy'], a['N'], a['R'], a['pend'],
                                                a['mean'], a['invstd'], a['gamma'], a['beta'], 1e-5, a['seed'], 7, a['p'], a['part'], None)
        for R, L in [(1, 56), (2, 56), (1, 126), (1, 63), (4, 15)]:     # R * L < 64 or R * ceil(L / 2) < 64
            yield 'da_conv3_winograd_bn', act, (P, P, P, 40, L, 64, 64, 64, R, P, P, P, P, P, 1e-5, P, 7, 0.2, P, None)


def bf16_calls():
    """da_conv3_bf16: (x, wpk, y, rows, L, ldx, C, ldy, N, accumulate, stream); da_conv3_bf16_bn: (..., N, R, in_pend,
    in_mean, in_invstd, gamma, beta, eps, stat_part, stream)."""
    base = dict(x=P, u=P, y=P, rows=40, L=56, ldx=64, C=64, ldy=64, N=64, acc=0)
    shape = dict(_SHAPE, N=[0, 16, 32, 65, 96, -64])
    limits = [dict(base, rows=1 << 16, L=1 << 15), dict(base, rows=1 << 20, L=1 << 11), dict(base, rows=(1 << 21) - 1, L=1 << 10, ldy=64 * 200, N=64 * 200),
              dict(base, rows=1 << 15, L=1 << 15, ldy=64 * 1024, N=64 * 1024)]
    for act in (0, 1):
        for a in itertools.chain(_grid(base, dict(shape, acc=[1]), _SHAPE_PAIRS), limits):
            if all(a[k] == base[k] for k in base if k != 'acc'):
                continue                                      # valid with either activation type: it would launch
            yield 'da_conv3_bf16', act, (a['x'], a['u'], a['y'], a['rows'], a['L'], a['ldx'], a['C'], a['ldy'], a['N'], a['acc'], None)
    bn = dict(base, R=20, pend=P, mean=P, invstd=P, gamma=P, beta=P, part=P)
    more = {'R': [0, -1, 3, 7, 1, 2], 'pend': [None], 'mean': [None], 'invstd': [None], 'gamma': [None], 'beta': [None], 'part': [None],
            'C': shape['C'] + [1056, 2048]}
    pairs = _SHAPE_PAIRS + [('R', 'rows'), ('R', 'L'), ('pend', 'part'), ('pend', 'mean'), ('pend', 'C'), ('part', 'R'), ('mean', 'rows')]
    for act in (0, 1):
        for a in itertools.chain(_grid(bn, dict(shape, **more), pairs), [dict(bn, **{k: v for k, v in l.items() if k != 'acc'}) for l in limits]):
            free = ('part',) if a['pend'] else ('pend', 'mean', 'invstd', 'gamma', 'beta')
            if all(a[k] == bn[k] for k in bn if k not in free) and (a['pend'] or a['part']):
                continue                                      # valid: it would launch
            yield 'da_conv3_bf16_bn', act, (a['x'], a['u'], a['y'], a['rows'], a['L'], a['ldx'], a['C'], a['ldy'], a['N'], a['R'], a['pend'],
                                            a['mean'], a['invstd'], a['gamma'], a['beta'], 1e-5, a['part'], None)
        for R, L in [(1, 56), (2, 56), (2, 64), (1, 129), (3, 43)]:         # a window shorter than a tile and its halo: R * L < 130
            yield 'da_conv3_bf16_bn', act, (P, P, P, 12 * R, L, 64, 64, 64, 64, R, P, P, P, P, P, 1e-5, P, None)


def _job(ConvJob, **kw):
    j = ConvJob()
    vals = dict(x=P, w=P, y=P, rows=40, Lm=28, Lsrc=56, ldx=64, C=64, Ldst=28, ldy=64, N=64, dst_stride=1, dst_off=0, src_stride=2,
                ntaps=3, src_off=(-1, 0, 1), wtap=(0, 1, 2), accumulate=0, x2=None, w2=None, tap_split=0)
    vals.update(kw)
    for k, v in vals.items():
        if k in ('src_off', 'wtap'):
            for t in range(3):
                getattr(j, k)[t] = v[t] if t < len(v) else 0
        else:
            setattr(j, k, v)
    return j


_JOB = {'x': [None], 'w': [None], 'y': [None], 'rows': [-1, 0], 'Lm': [0, -2], 'ntaps': [0, 4, -1], 'C': [16, 48, 65], 'N': [32, 96, 65, 16],
        'ldx': [62, 66, 65], 'x2': [P]}                       # (x2 without w2)
_JOB_BF = {'C': [16, 48, 65, 0], 'ldx': [62, 66, 65, 32], 'ldy': [32, 0], 'src_stride': [0, 3, 1], 'Lsrc': [55, 28, 57], 'dst_stride': [0, -1, 2],
           'dst_off': [-1, 1, 28], 'Ldst': [27, 0], 'wtap': [(0, 1, 3), (-1, 1, 2), (3, 0, 0)], 'src_off': [(-2, 0, 1), (0, 1, 3), (-1, 0, 2)]}
_SPLIT = [dict(x2=P, w2=P, tap_split=0), dict(x2=P, w2=P, tap_split=3), dict(x2=P, w2=P, tap_split=-1),
          dict(x2=P, w2=P, tap_split=2, ntaps=2), dict(x2=P, w2=P, tap_split=1, ntaps=1)]
# the 32-bit limits: rows * Lm * Lm (fp32), rows * Lm, rows * Lsrc, rows * Ldst (bf16)
_LIMITS_GEMM = [dict(rows=1 << 8, Lm=1 << 12, Lsrc=1 << 13, Ldst=1 << 12), dict(rows=1, Lm=1 << 16, Lsrc=1 << 17, Ldst=1 << 16),
                dict(rows=1 << 16, Lm=1 << 15, Lsrc=1 << 16, Ldst=1 << 15)]
_LIMITS_BF = [dict(rows=1 << 16, Lm=1 << 15, Lsrc=1 << 16, Ldst=1 << 15), dict(rows=1 << 12, Lm=1 << 10, Lsrc=1 << 11, Ldst=BIG),
              dict(rows=1 << 20, Lm=1 << 10, Lsrc=1 << 11, Ldst=1 << 10), dict(rows=1 << 14, Lm=1 << 16, Lsrc=1 << 17, Ldst=1 << 16)]


def multi_calls(ConvJob):
    """da_conv_gemm_multi / da_conv_bf16_multi: (jobs, n, stream).  -> (name, act, jobs-or-None, n)."""
    empty = dict(rows=0)
    for act in (0, 1):
        for name in ('da_conv_gemm_multi', 'da_conv_bf16_multi'):
            gemm = name == 'da_conv_gemm_multi'
            yield name, act, None, 1
            yield name, act, None, 3
            yield name, act, [_job(ConvJob)], -1
            if gemm:
                yield name, act, [_job(ConvJob)], 0
                for n in (5, 6, 9):                           # more than 4 jobs
                    yield name, act, [_job(ConvJob, rows=0) for _ in range(n)], n
            fields = _JOB if gemm else dict(_JOB, **_JOB_BF)
            bad = [{k: v} for k, vals in fields.items() for v in vals] + _SPLIT + (_LIMITS_GEMM if gemm else _LIMITS_BF)
            for kw in bad:        # the bad job alone, behind and in front of empty ones: a refusal does not depend on its place
                for jobs in ([kw], [empty, kw], [kw, empty, empty], [empty, empty, empty, kw]):
                    yield name, act, [_job(ConvJob, **j) for j in jobs], len(jobs)
        # da_conv_bf16_multi takes more than 4 jobs, in launches of 4: a refusal in a later group, behind empty jobs
        for n in (5, 8, 9):
            yield 'da_conv_bf16_multi', act, [_job(ConvJob, rows=0) for _ in range(n - 1)] + [_job(ConvJob, C=48)], n
            yield 'da_conv_bf16_multi', act, [_job(ConvJob, rows=0) for _ in range(n)], n
        # all jobs of one launch share src_stride
        yield 'da_conv_bf16_multi', act, [_job(ConvJob, rows=0), _job(ConvJob, rows=0, src_stride=1, Lsrc=28)], 2


def gemm_calls():
    """da_conv_gemm: (x, w, y, rows, Lm, Lsrc, ldx, C, Ldst, ldy, N, dst_stride, dst_off, src_stride, ntaps, src_off, wtap,
    accumulate, stream)."""
    base = dict(x=P, w=P, y=P, rows=40, Lm=28, Lsrc=56, ldx=64, C=64, Ldst=28, ldy=64, N=64, ntaps=3)
    singles = {'x': [None], 'w': [None], 'y': [None], 'rows': [-1, 0], 'Lm': [0, -2], 'ntaps': [0, 4, -1], 'C': [16, 48, 65], 'N': [16, 48, 65],
               'ldx': [62, 66, 65]}
    pairs = [('rows', 'C'), ('rows', 'N'), ('rows', 'ldx'), ('C', 'N'), ('x', 'C'), ('ntaps', 'C'), ('Lm', 'rows')]
    limits = [dict(base, rows=1 << 8, Lm=1 << 12), dict(base, rows=1, Lm=1 << 16), dict(base, rows=1 << 4, Lm=1 << 14)]
    so, wt = (ctypes.c_int * 3)(-1, 0, 1), (ctypes.c_int * 3)(0, 1, 2)
    for act in (0, 1):
        for a in itertools.chain(_grid(base, singles, pairs), limits):
            if act == 0 and a == base:
                continue
            yield 'da_conv_gemm', act, (a['x'], a['w'], a['y'], a['rows'], a['Lm'], a['Lsrc'], a['ldx'], a['C'], a['Ldst'], a['ldy'], a['N'],
                                        1, 0, 2, a['ntaps'], so, wt, 0, None)


def run(lib, other, ConvJob):
    """-> (calls, [(name, act, args, rc, rc_other)] of the calls whose codes differ or are neither DA_EINVAL nor DA_OK)."""
    calls, bad = 0, []
    flat = itertools.chain(wino_calls(), wino_drop_calls(), wino_bn_calls(), bf16_calls(), gemm_calls())
    todo = [(n, act, args, None) for n, act, args in flat] + [(n, act, jobs, cnt) for n, act, jobs, cnt in multi_calls(ConvJob)]
    for act in (0, 1):
        for l in (lib, other):
            assert l.da_set_act_dtype(act) == 0
        for name, a, args, cnt in todo:
            if a != act:
                continue
            rcs = []
            for l in (lib, other):
                if cnt is None:
                    rcs.append(getattr(l, name)(*args))
                else:
                    arr = None if args is None else (ConvJob * len(args))(*args)
                    rcs.append(getattr(l, name)(arr, cnt, None))
            calls += 1
            if rcs[0] != rcs[1] or rcs[0] not in (0, -1):
                bad.append((name, act, args if cnt is None else cnt, rcs[0], rcs[1]))
    for l in (lib, other):
        l.da_set_act_dtype(0)
    return calls, bad


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--other', required=True, help='the library to compare with (for instance the parent commit\'s build)')
    args = ap.parse_args()
    from deepards_amd import _lib
    lib = _lib.lib()
    other = ctypes.CDLL(args.other)
    for name, (res, argt) in _lib.SIGNATURES.items():
        fn = getattr(other, name)
        fn.restype, fn.argtypes = res, argt
    calls, bad = run(lib, other, _lib.ConvJob)
    for b in bad[:40]:
        print('DIFFERENT' if b[3] != b[4] else 'LAUNCHED ', *b)
    print('%d validation calls, %d differences, %d calls that got past validation' %
          (calls, sum(b[3] != b[4] for b in bad), sum(b[3] == b[4] for b in bad)))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
