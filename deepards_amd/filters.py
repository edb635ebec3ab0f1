"""Host side of the frequency filters of the batch path -- ingest-time numpy, no GPU work.

The reference filters every item in ``ARDSRawDataset.__getitem__`` behind ``(data - mu) / std`` (dataset.py:1381-1400):

* ``sosfilt(self.sos, data, axis=-1)`` with the 10th-order Butterworth cascade ``setup_butter_filter`` chose from
  ``butter_low`` / ``butter_high`` (dataset.py:546-557, fs = 50 Hz);
* an FFT band mask ``|f| > fft_filtering_low and |f| < fft_filtering_high`` over ``fftfreq(224, d=0.02)`` -- active only
  when BOTH values are given (:1393).

Both are linear maps on one row of L samples, and that is how the device applies them (csrc/filters.hip):

    y[n] = sum_{m <= n} h[n - m] x[m]            h = the first L samples of the cascade's impulse response: ``sosfilt``
                                                 starts every call from a zero state, so over a finite row it IS this sum
    z[n] = sum_m g[(n - m) mod 224] y[m]         g = real(ifft(mask)): the mask is symmetric in |f|, so the circular
                                                 convolution is exactly real and dropping ``.imag`` loses nothing

Two more steps of the item complete the chain, in the reference's order: normalise, ``sosfilt``, DOWNSAMPLE, FFT mask.

* padded datasets (every ``dataset_type`` that contains ``padded_breath_by_breath``, :1375-1377, 1406-1409): ``mu`` is
  subtracted only where the raw sample is non-zero, so padding stays exactly 0 (``normalize_host``);
* ``post_hoc_downsampling`` (:1384-1391): ``scipy.signal.resample(data, int(L / factor), axis=-1)``, zero-padded at the end
  back to L samples.  Fourier resampling of a real row is linear as well: r = R y with ``R = resample_matrix(L, new_len)``.

This module chooses the filter, designs it (``scipy.signal.butter``, the reference's own designer, imported lazily),
turns it into ``h`` / ``g`` and restates the two sums in numpy (``apply_host``) for the CPU tests.  ``dataset.py`` itself
does not import here; parity is pinned to the library calls it makes (tests/tools/make_golden_filters.py).
"""
import numpy as np

BUTTER_ORDER = 10                # dataset.py:548-557
SAMPLE_RATE_HZ = 50
FFT_FILTER_LEN = 224             # dataset.py:1394: np.fft.fftfreq(224, d=0.02)
MAX_BUTTER_LEN = 512             # the device kernel's row limit for h (the C5 tile shape)


def butter_choice(low, high):
    """The five branches of ``setup_butter_filter`` (dataset.py:546-557), in the reference's order ->
    (btype, Wn) or None (no filter)."""
    if low is not None and high is None:
        return 'lowpass', low
    elif low == 0:
        return 'lowpass', high
    elif low is None and high is not None:
        return 'highpass', high
    elif high == 25:
        return 'highpass', low
    elif low is not None and high is not None:
        return 'bandpass', (low, high)
    return None


def butter_sos(low, high):
    """The cascade ``setup_butter_filter`` builds: (n_sections, 6) float64 second-order sections, or None."""
    choice = butter_choice(low, high)
    if choice is None:
        return None
    from scipy.signal import butter                       # the reference's own designer (dataset.py:548)
    btype, wn = choice
    return np.asarray(butter(BUTTER_ORDER, wn, fs=SAMPLE_RATE_HZ, output='sos', btype=btype), dtype=np.float64)


def impulse_response(sos, L):
    """First L samples of the impulse response of a second-order-section cascade, float64: every section in direct form II
    transposed from a zero state, sample by sample through the cascade -- the recurrence ``sosfilt`` runs."""
    sos = np.asarray(sos, dtype=np.float64)
    if sos.ndim != 2 or sos.shape[1] != 6:
        raise ValueError('sos must be (n_sections, 6)')
    sos = sos / sos[:, 3:4]                                # a0 = 1
    z = np.zeros((sos.shape[0], 2), dtype=np.float64)
    h = np.zeros(int(L), dtype=np.float64)
    for n in range(int(L)):
        x = 1.0 if n == 0 else 0.0
        for s, (b0, b1, b2, _, a1, a2) in enumerate(sos):
            y = b0 * x + z[s, 0]
            z[s, 0] = b1 * x - a1 * y + z[s, 1]
            z[s, 1] = b2 * x - a2 * y
            x = y
        h[n] = x
    return h


def fft_band_kernel(low, high):
    """g = real(ifft(mask)) of the band mask of dataset.py:1393-1400, (224,) float64; None unless BOTH bounds are given.
    The inequalities are strict: low = 0 removes DC.  The reference builds the mask on the shifted axis and shifts the
    spectrum there and back; on the unshifted axis that is the same mask over ``fftfreq`` itself."""
    if low is None or high is None:
        return None
    freqs = np.fft.fftfreq(FFT_FILTER_LEN, d=0.02)
    mask = np.logical_and(np.abs(freqs) > low, np.abs(freqs) < high)
    return np.ascontiguousarray(np.fft.ifft(mask.astype(np.float64)).real)


def filter_kernels(butter_low=None, butter_high=None, fft_filtering_low=None, fft_filtering_high=None, L=FFT_FILTER_LEN):
    """(h, g) for rows of L samples; each (L,) float64 or None."""
    sos = butter_sos(butter_low, butter_high)
    g = fft_band_kernel(fft_filtering_low, fft_filtering_high)
    if g is not None and int(L) != FFT_FILTER_LEN:
        raise ValueError('the FFT band filter is defined on windows of %d samples (dataset.py:1394), not %d' % (FFT_FILTER_LEN, L))
    if sos is not None and int(L) > MAX_BUTTER_LEN:
        raise ValueError('the Butterworth filter runs on rows of up to %d samples, not %d' % (MAX_BUTTER_LEN, L))
    return (None if sos is None else impulse_response(sos, L)), g


def post_hoc_new_len(L, factor):
    """``int(L / factor)`` (dataset.py:1386).  ValueError unless 1 <= new_len <= L: in the reference a factor below 1 makes
    ``np.pad`` raise (a negative pad length) and a factor above L resamples the row to nothing."""
    if not float(factor) > 0:
        raise ValueError('post_hoc_downsampling must be a positive factor, got %r' % (factor,))
    new_len = int(int(L) / float(factor))
    if not 1 <= new_len <= int(L):
        raise ValueError('post_hoc_downsampling %r turns rows of %d samples into %d: 1 <= int(L / factor) <= L is needed' % (factor, L, new_len))
    return new_len


def resample_matrix(L, new_len):
    """R (new_len, L) float64 with ``scipy.signal.resample(x, new_len, axis=-1) == x @ R.T`` for real rows x of L samples: the
    routine's own steps on the unit vectors -- rfft, keep min(new_len, L) // 2 + 1 bins, double the Nyquist bin when new_len
    is even and smaller than L (halve it when larger: unreachable here), irfft to new_len samples, scale by new_len / L."""
    L, new_len = int(L), int(new_len)
    if not 1 <= new_len <= L:
        raise ValueError('1 <= new_len <= L expected, got new_len %d, L %d' % (new_len, L))
    spectrum = np.fft.rfft(np.eye(L, dtype=np.float64), axis=0)          # column j: the spectrum of the unit vector e_j
    n = min(new_len, L)
    kept = np.zeros((new_len // 2 + 1, L), dtype=spectrum.dtype)
    kept[:n // 2 + 1] = spectrum[:n // 2 + 1]
    if n % 2 == 0 and new_len < L:
        kept[n // 2] *= 2.0                                              # the bin stands for +Nyquist and -Nyquist of the new grid
    return np.ascontiguousarray(np.fft.irfft(kept, new_len, axis=0) * (float(new_len) / float(L)))


def normalize_host(x, mu, std, padded=False):
    """The first step of the item on raw rows x (..., C, L), float64; mu / std scalars or one per channel.  padded:
    ``(x - where(x != 0, mu, 0)) / std`` (dataset.py:1375-1377, 1406-1409; a NaN is non-zero), else ``(x - mu) / std``."""
    x = np.asarray(x, dtype=np.float64)
    mu = np.asarray(mu, dtype=np.float64).reshape(-1, 1)
    std = np.asarray(std, dtype=np.float64).reshape(-1, 1)
    if not padded:
        return (x - mu) / std
    return np.where(x != 0, (x - mu) / std, x / std)


def apply_host(x, h=None, g=None, r=None):
    """The device's sums in numpy on rows x (..., L), float64, in the item's order: y = causal convolution with h,
    r-stage = R y zero-padded at the end back to L samples (r: the (new_len, L) matrix of ``resample_matrix``),
    z = circular convolution with g.  A stage that is None is skipped."""
    y = np.asarray(x, dtype=np.float64)
    L = y.shape[-1]
    n, m = np.arange(L)[:, None], np.arange(L)[None, :]
    if h is not None:
        h = np.asarray(h, dtype=np.float64)
        if h.shape != (L,):
            raise ValueError('h must hold one sample per sample of a row')
        y = y @ np.where(m <= n, h[(n - m) % L], 0.0).T
    if r is not None:
        r = np.asarray(r, dtype=np.float64)
        if r.ndim != 2 or r.shape[1] != L or not 1 <= r.shape[0] <= L:
            raise ValueError('r must be (new_len <= L, L)')
        y = np.concatenate([y @ r.T, np.zeros(y.shape[:-1] + (L - r.shape[0],))], axis=-1)
    if g is not None:
        g = np.asarray(g, dtype=np.float64)
        if g.shape != (L,):
            raise ValueError('g must hold one sample per sample of a row')
        y = y @ g[(n - m) % L].T
    return y
