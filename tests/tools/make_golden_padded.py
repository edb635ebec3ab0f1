"""Write tests/golden/padded_*.npz: the reference's item chain on PADDED windows, with post-hoc downsampling.

    python tests/tools/make_golden_padded.py [<output dir, default tests/golden>]

``ARDSRawDataset.__getitem__`` (deepards/dataset.py:1375-1400) does five things to an item of a ``padded_breath_by_breath``
dataset, in this order, float64 throughout.  ``dataset.py`` itself does not import on a machine without ventmap / imblearn, so
PARITY IS PINNED TO THE LIBRARY CALLS IT MAKES, with its arguments:

1. the padded normalisation: an array of zeros gets ``mu`` written with ``np.put`` at the flat positions of the non-zero
   raw samples, is subtracted, and the difference is divided by ``std`` (:1375-1377, 1406-1409); an unpadded dataset type:
   ``(data - mu) / std``;
2. ``scipy.signal.sosfilt(sos, data, axis=-1)`` with the cascade of ``setup_butter_filter`` (:546-557);
3. ``scipy.signal.resample(data, int(L / post_hoc_downsampling), axis=-1)`` (:1384-1388);
4. ``np.pad`` of the last axis only, at its end, back to L samples (:1391);
5. the FFT band mask over ``fftshift(fftfreq(224, d=0.02))`` (:1393-1400).

Nothing of ``deepards_amd`` is imported: the files are an independent record the package's normalisation, resampling matrix
and sums are tested against.

Each case is ONE window (20 rows x 224) of tests/golden/test_dataset.npz made padded: every row's tail is zeroed behind a
seeded length in [30, 224], row 0 keeps all 224 samples, and one interior sample of row 3 is set to exactly 0 (the rule is
``!= 0``, not "behind the breath's end": that sample stays 0 too).  The last case leaves its window unpadded and uses the
unpadded normalisation -- the reference resamples whatever the dataset type.  Arrays only:

    x (20, 1, 224) float64    the raw (padded) window;  window: its index in the fixture;  lengths (20,): samples kept per row
    mu, std                   the fixture's scaling factors;  padded: 1 when the padded normalisation applies
    butter_low, butter_high, fft_filtering_low, fft_filtering_high, post_hoc_downsampling    the dataset keywords (NaN: None)
    new_len                   int(224 / post_hoc_downsampling) (0: no downsampling)
    expected (20, 1, 224)     the reference's item, float64"""
import os
import sys

import numpy as np
from scipy.signal import resample

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_filters import reference_cascade, reference_item as filter_item  # noqa: E402
GOLD = os.path.join(os.path.dirname(HERE), 'golden')

# name, fixture window, padded, butter_low, butter_high, post_hoc_downsampling, fft_filtering_low, fft_filtering_high
CASES = [
    ('only', 1, True, None, None, None, None, None),
    ('down_2', 2, True, None, None, 2.0, None, None),                    # 112
    ('down_2p5', 4, True, None, None, 2.5, None, None),                  # 89: an odd length
    ('down_25', 6, True, None, None, 25.0, None, None),                  # 8: the smallest of the reference's experiments
    ('down_1p2', 8, True, None, None, 1.2, None, None),                  # 186: the largest
    ('bandpass_5_10', 10, True, 5, 10, None, None, None),
    ('lowpass_10_down_4', 12, True, 0, 10, 4.0, None, None),
    ('down_3_fft_0_6', 14, True, None, None, 3.0, 0, 6),
    ('highpass_15_down_1p4_fft_0_20', 16, True, None, 15, 1.4, 0, 20),
    ('lowpass_10_down_1p2', 18, True, 0, 10, 1.2, None, None),
    ('unpadded_down_2', 19, False, None, None, 2.0, None, None),
]


def reference_item(window, mu, std, padded, sos, factor, fft_low, fft_high):
    """The item from the normalisation on: the same library calls on the same (NB, C, L) array, in the same order.  The
    Butterworth and FFT steps are those of make_golden_filters.reference_item, reached with mu = 0 and std = 1 (x - 0 and
    x / 1 return x bit for bit), so both sets of goldens share one statement of them."""
    if padded:
        offset = np.zeros(window.shape)
        np.put(offset, np.flatnonzero(window.ravel() != 0), mu)       # mu where the raw sample is non-zero, 0 on padding
        item = (window - offset) / std
    else:
        item = (window - mu) / std
    item = filter_item(item, 0.0, 1.0, sos, None, None)                # sosfilt (nothing without a cascade)
    if factor is not None:
        L = item.shape[-1]
        shorter = resample(item, int(L / factor), axis=-1)
        item = np.pad(shorter, [(0, 0)] * (item.ndim - 1) + [(0, L - shorter.shape[-1])])
    return filter_item(item, 0.0, 1.0, None, fft_low, fft_high)        # the FFT band mask (nothing without both bounds)


def padded_window(x, seed):
    """Zero every row's tail behind a seeded length in [30, 224]; row 0 keeps its full length; one interior zero in row 3."""
    rng = np.random.RandomState(seed)
    lengths = rng.randint(30, 225, size=x.shape[0])
    lengths[0] = x.shape[-1]
    x = x.copy()
    for row, n in enumerate(lengths):
        x[row, :, n:] = 0.0
    x[3, 0, lengths[3] // 2] = 0.0
    return x, lengths.astype(np.int64)


def main(out_dir=GOLD):
    z = np.load(os.path.join(GOLD, 'test_dataset.npz'))
    mu, std = float(z['mu']), float(z['std'])
    nan = lambda v: np.float64(np.nan if v is None else v)
    for name, window, padded, low, high, factor, fft_low, fft_high in CASES:
        x = np.ascontiguousarray(z['x'][window], dtype=np.float64)
        assert x.shape == (20, 1, 224)
        lengths = np.full(20, 224, dtype=np.int64)
        if padded:
            x, lengths = padded_window(x, 1000 + window)
        expected = reference_item(x, mu, std, padded, reference_cascade(low, high)[1], factor, fft_low, fft_high)
        assert expected.shape == x.shape and expected.dtype == np.float64 and np.isfinite(expected).all()
        new_len = 0 if factor is None else int(224 / factor)
        path = os.path.join(out_dir, 'padded_%s.npz' % name)
        np.savez_compressed(path, x=x, window=np.int64(window), lengths=lengths, mu=np.float64(mu), std=np.float64(std),
                            padded=np.int64(padded), butter_low=nan(low), butter_high=nan(high), fft_filtering_low=nan(fft_low),
                            fft_filtering_high=nan(fft_high), post_hoc_downsampling=nan(factor), new_len=np.int64(new_len),
                            expected=expected)
        print('%-32s window %2d  new_len %3d  max |expected| %.3e  %d bytes' % (name, window, new_len, np.abs(expected).max(),
                                                                              os.path.getsize(path)))


if __name__ == '__main__':
    main(*sys.argv[1:2])
