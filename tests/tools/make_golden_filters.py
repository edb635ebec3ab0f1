"""Write tests/golden/filter_*.npz: the reference's frequency filters on windows of the ingested fixture.

    python tests/tools/make_golden_filters.py [<output dir, default tests/golden>]

The reference applies the filters in ``ARDSRawDataset.__getitem__`` (deepards/dataset.py:1381-1400) with the cascade chosen
by ``setup_butter_filter`` (:546-557).  ``dataset.py`` itself does not import on a machine without ventmap / imblearn, so
PARITY IS PINNED TO THE LIBRARY CALLS IT MAKES, with its arguments: ``scipy.signal.butter(10, Wn, fs=50, output='sos',
btype=...)``, ``scipy.signal.sosfilt(sos, data, axis=-1)`` on the (NB, C, L) item behind ``(data - mu) / std``, and the
mask ``|f| > low and |f| < high`` over ``fftshift(fftfreq(224, d=0.02))`` applied to ``fftshift(fft(data, axis=-1))`` and
undone by ``ifft(ifftshift(.), axis=-1).real`` -- float64 throughout.  Nothing of ``deepards_amd`` is imported: the files
are an independent record the package's own filter design, impulse response and sums are tested against.

Each file holds arrays only, for ONE window (20 rows x 224) of tests/golden/test_dataset.npz:

    x (20, 1, 224) float64    the raw window;  window: its index in the fixture;  mu, std: the fixture's scaling factors
    butter_low, butter_high, fft_filtering_low, fft_filtering_high    the dataset keywords (NaN: None)
    btype                     the branch the choice rule took: 0 none, 1 lowpass, 2 highpass, 3 bandpass
    sos (n, 6)                the designed cascade ((0, 6): no Butterworth filter)
    h (224,)                  sosfilt(sos, unit impulse) ((0,): none)
    g (224,)                  real(ifft(mask)) on the unshifted axis ((0,): no FFT filter)
    expected (20, 1, 224)     the reference's item, float64

Cases: every branch of the choice rule (low alone; low == 0; high alone; high == 25; both), lowpass 0.25 Hz, bandpass
(1e-8, 5), FFT (0, 0.25) and (0, 20), and lowpass 10 combined with FFT (0, 6)."""
import os
import sys

import numpy as np
from scipy.signal import butter, sosfilt

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(os.path.dirname(HERE), 'golden')

# name, fixture window, butter_low, butter_high, fft_filtering_low, fft_filtering_high
CASES = [
    ('lowpass_0p25', 0, 0.25, None, None, None),              # low alone -> lowpass(low)
    ('low0_lowpass_0p03125', 3, 0, 0.03125, None, None),      # low == 0 -> lowpass(high)
    ('highpass_15', 5, None, 15, None, None),                 # high alone -> HIGHPASS(high)
    ('high25_highpass_24', 7, 24, 25, None, None),            # high == 25 -> highpass(low)
    ('bandpass_2_3', 9, 2, 3, None, None),                    # both -> bandpass
    ('bandpass_1em8_5', 11, 1e-8, 5, None, None),
    ('fft_0_0p25', 13, None, None, 0, 0.25),
    ('fft_0_20', 15, None, None, 0, 20),
    ('lowpass_10_fft_0_6', 17, 0, 10, 0, 6),
]
BTYPES = {None: 0, 'lowpass': 1, 'highpass': 2, 'bandpass': 3}


def reference_cascade(low, high):
    """(btype, sos) as setup_butter_filter would leave them; (None, None) without a filter.  The rule is first match in the
    reference's order: low alone, low == 0, high alone, high == 25, both."""
    rule = [(low is not None and high is None, 'lowpass', low),
            (low == 0, 'lowpass', high),
            (low is None and high is not None, 'highpass', high),
            (high == 25, 'highpass', low),
            (low is not None and high is not None, 'bandpass', (low, high))]
    for applies, btype, wn in rule:
        if applies:
            return btype, butter(10, wn, fs=50, output='sos', btype=btype)
    return None, None


def reference_item(window, mu, std, sos, fft_low, fft_high):
    """The item from the normalisation on (unpadded dataset, no transforms, no post-hoc downsampling): the same library
    calls on the same (NB, C, L) array, in the same order."""
    item = (window - mu) / std
    if sos is not None:
        item = sosfilt(sos, item, axis=-1).copy()
    if fft_low is not None and fft_high is not None:
        shifted_hz = np.abs(np.fft.fftshift(np.fft.fftfreq(224, d=0.02)))
        keep = np.logical_and(shifted_hz > fft_low, shifted_hz < fft_high)
        spectrum = np.fft.fftshift(np.fft.fft(item, axis=-1))          # (no axes: every axis is shifted, and shifted back)
        spectrum[:, :, ~keep] = 0
        item = np.fft.ifft(np.fft.ifftshift(spectrum), axis=-1).real
    return item


def main(out_dir=GOLD):
    z = np.load(os.path.join(GOLD, 'test_dataset.npz'))
    mu, std = float(z['mu']), float(z['std'])
    nan = lambda v: np.float64(np.nan if v is None else v)
    for name, window, low, high, fft_low, fft_high in CASES:
        x = np.ascontiguousarray(z['x'][window], dtype=np.float64)
        assert x.shape == (20, 1, 224)
        btype, sos = reference_cascade(low, high)
        impulse = np.zeros(224)
        impulse[0] = 1.0
        h = np.zeros((0,)) if sos is None else sosfilt(sos, impulse)
        if fft_low is not None and fft_high is not None:
            freqs = np.fft.fftfreq(224, d=0.02)
            g = np.fft.ifft(np.logical_and(np.abs(freqs) > fft_low, np.abs(freqs) < fft_high).astype(np.float64)).real
        else:
            g = np.zeros((0,))
        expected = reference_item(x, mu, std, sos, fft_low, fft_high)
        assert expected.shape == x.shape and expected.dtype == np.float64 and np.isfinite(expected).all()
        path = os.path.join(out_dir, 'filter_%s.npz' % name)
        np.savez_compressed(path, x=x, window=np.int64(window), mu=np.float64(mu), std=np.float64(std), butter_low=nan(low),
                            butter_high=nan(high), fft_filtering_low=nan(fft_low), fft_filtering_high=nan(fft_high),
                            btype=np.int64(BTYPES[btype]), sos=np.zeros((0, 6)) if sos is None else np.asarray(sos, dtype=np.float64),
                            h=h, g=g, expected=expected)
        print('%-28s window %2d  %s  max |expected| %.3e  %d bytes' % (name, window, btype, np.abs(expected).max(), os.path.getsize(path)))


if __name__ == '__main__':
    main(*sys.argv[1:2])
