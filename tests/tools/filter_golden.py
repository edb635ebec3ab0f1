"""The filter goldens (tests/golden/filter_*.npz, written by make_golden_filters.py) and the bound the filter tests hold
results to, shared by tests/test_filters_cpu.py and tests/test_filters_gpu.py.

Bound, per element, derived and not tuned:

    |got - float32(ref)| <= ulp32(ref) + 2 L 2^-52 A

``ref`` is the reference's float64 item, ``got`` a float32 result.  The first term is the one rounding of the final cast (a
float64 value that differs from ref in its last bits may round to the neighbouring float32).  The second is the standard
bound of a length-L dot product evaluated in float64 in any order, |fl(sum a_i b_i) - sum a_i b_i| <= L u sum |a_i| |b_i|
with u = 2^-53, applied to the causal sum and again to the circular sum over its result: A is the same two sums taken over
|x|, |h| and |g|.  As a condition on top, at most 0.1 % of a case's elements may differ from float32(ref) at all: the
reference against the float64 restatement stays at or below 2 of 89 600 on these inputs."""
import glob
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'golden')
KEYS = ('butter_low', 'butter_high', 'fft_filtering_low', 'fft_filtering_high')
BTYPES = {0: None, 1: 'lowpass', 2: 'highpass', 3: 'bandpass'}
MAX_DIFFERING_FRACTION = 1e-3


class Case(object):
    def __init__(self, path):
        z = np.load(path)
        self.name = os.path.basename(path)[len('filter_'):-len('.npz')]
        self.x, self.expected = z['x'], z['expected']
        self.mu, self.std, self.window = float(z['mu']), float(z['std']), int(z['window'])
        self.keys = {k: (None if np.isnan(z[k]) else float(z[k])) for k in KEYS}
        self.btype = BTYPES[int(z['btype'])]
        self.sos = z['sos'] if z['sos'].shape[0] else None
        self.h = z['h'] if z['h'].size else None
        self.g = z['g'] if z['g'].size else None

    def __repr__(self):
        return self.name


_CASES = []


def cases():
    """Every golden case, loaded once."""
    if not _CASES:
        _CASES.extend(Case(p) for p in sorted(glob.glob(os.path.join(GOLD, 'filter_*.npz'))))
    return _CASES


def case(name):
    return {c.name: c for c in cases()}[name]


def ulp32(ref):
    return np.spacing(np.abs(np.asarray(ref).astype(np.float32))).astype(np.float64)


def bound(ref, x_normalised, h, g, apply_host):
    """The per-element bound of the module docstring for rows x_normalised (..., L) filtered by h / g (either None)."""
    L = x_normalised.shape[-1]
    a = apply_host(np.abs(x_normalised), None if h is None else np.abs(h), None if g is None else np.abs(g))
    return ulp32(ref) + 2.0 * L * 2.0 ** -52 * a


def check(what, got32, ref64, limit):
    """Assert the bound and the cap; print the achieved figures first (visible under -s).  got32: float32 array."""
    got32 = np.asarray(got32)
    assert got32.dtype == np.float32 and got32.shape == ref64.shape, (got32.dtype, got32.shape, ref64.shape)
    r32 = ref64.astype(np.float32)
    err = np.abs(got32.astype(np.float64) - r32.astype(np.float64))
    differ = int((got32 != r32).sum())
    worst = float((err / limit).max())
    print('%s: max |got - float32(ref)| %.3e, worst error / bound %.3f, %d of %d elements differ from float32(ref)'
          % (what, err.max(), worst, differ, got32.size))
    assert np.isfinite(got32).all(), what
    assert (err <= limit).all(), '%s: %d elements over the bound, worst at %.3f of it' % (what, int((err > limit).sum()), worst)
    assert differ <= MAX_DIFFERING_FRACTION * got32.size, '%s: %d of %d elements differ from float32(ref)' % (what, differ, got32.size)
