"""The padded / downsampling goldens (tests/golden/padded_*.npz, written by make_golden_padded.py) and the bound the tests
hold results to, shared by tests/test_padded_cpu.py and tests/test_padded_gpu.py.

Bound, per element, derived and not tuned -- in the spirit of filter_golden.py, but NORM-wise:

    |got - float32(ref)| <= ulp32(ref) + 2 S L 2^-52 ||x_norm row||_1 prod_stages max|M_stage|

``ref`` is the reference's float64 item, ``got`` a float32 result.  The first term is the one rounding of the final cast.  The
reference computes two of its stages by FFT (resample, the band mask), whose rounding error scales with the NORM of the row
and not with the element, so an element-wise bound of the sums (filter_golden.py) does not cover the reference's own error
where the result is small.  Every stage is a matrix M on the row (h as a lower-triangular Toeplitz matrix, R, g as a
circulant): |(M y)[n]| <= max|M| ||y||_1 and ||M y||_1 <= L max|M| ||y||_1 bound what a stage can make of its input, and a
length-L dot product in float64 (any order, or an FFT) errs by at most L 2^-53 sum|a_i||b_i| per stage; both sides (the
reference and the code under test) get that allowance for each of the S active stages.  S = 0: the cast alone.

Cap: among the SIGNIFICANT elements of a case -- |ref| >= 2^-16 x the row's max|ref| -- at most 0.1 % may differ from
float32(ref) at all.  Below that floor the reference's own FFT noise decides the last bits; those elements are held by the
bound only.  Measured on the committed lowpass 10 + 1.2x golden (4480 elements, all differences below the floor): the float64
numpy restatement on the CPU (numpy 2, scipy 1.15.3) differs from float32(ref) in 371 elements, the MI355X kernel in 372."""
import glob
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'golden')
KEYS = ('butter_low', 'butter_high', 'fft_filtering_low', 'fft_filtering_high')
MAX_DIFFERING_FRACTION = 1e-3
SIGNIFICANCE_FLOOR = 2.0 ** -16


class Case(object):
    def __init__(self, path):
        z = np.load(path)
        self.name = os.path.basename(path)[len('padded_'):-len('.npz')]
        self.x, self.expected, self.lengths = z['x'], z['expected'], z['lengths']
        self.mu, self.std, self.window = float(z['mu']), float(z['std']), int(z['window'])
        self.padded = bool(z['padded'])
        self.keys = {k: (None if np.isnan(z[k]) else float(z[k])) for k in KEYS}
        self.factor = None if np.isnan(z['post_hoc_downsampling']) else float(z['post_hoc_downsampling'])
        self.new_len = int(z['new_len'])

    def __repr__(self):
        return self.name


_CASES = []


def cases():
    """Every golden case, loaded once."""
    if not _CASES:
        _CASES.extend(Case(p) for p in sorted(glob.glob(os.path.join(GOLD, 'padded_*.npz'))))
    return _CASES


def case(name):
    return {c.name: c for c in cases()}[name]


def ulp32(ref):
    return np.spacing(np.abs(np.asarray(ref).astype(np.float32))).astype(np.float64)


def bound(ref, x_normalised, h=None, r=None, g=None):
    """The per-element bound of the module docstring for rows x_normalised (..., L) through the stages h / r / g (each the
    stage's kernel or matrix, or None)."""
    L = x_normalised.shape[-1]
    stages = [np.abs(m).max() for m in (h, r, g) if m is not None]
    norm1 = np.abs(x_normalised).sum(axis=-1, keepdims=True)
    return ulp32(ref) + 2.0 * len(stages) * L * 2.0 ** -52 * norm1 * float(np.prod(stages))


def check(what, got32, ref64, limit):
    """Assert the bound and the cap; print the achieved figures first (visible under -s).  got32: float32 array."""
    got32 = np.asarray(got32)
    assert got32.dtype == np.float32 and got32.shape == ref64.shape, (got32.dtype, got32.shape, ref64.shape)
    r32 = ref64.astype(np.float32)
    err = np.abs(got32.astype(np.float64) - r32.astype(np.float64))
    significant = np.abs(ref64) >= SIGNIFICANCE_FLOOR * np.abs(ref64).max(axis=-1, keepdims=True)
    differ = got32 != r32
    n_sig, d_sig = int(significant.sum()), int((differ & significant).sum())
    worst = float((err / limit).max())
    print('%s: max |got - float32(ref)| %.3e, worst error / bound %.3e, %d of %d significant elements differ from float32(ref) '
          '(%d of all %d)' % (what, err.max(), worst, d_sig, n_sig, int(differ.sum()), got32.size))
    assert np.isfinite(got32).all(), what
    assert (err <= limit).all(), '%s: %d elements over the bound, worst at %.3f of it' % (what, int((err > limit).sum()), worst)
    assert d_sig <= MAX_DIFFERING_FRACTION * n_sig, '%s: %d of %d significant elements differ from float32(ref)' % (what, d_sig, n_sig)
