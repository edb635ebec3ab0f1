"""CPU tests of the frequency filters of the batch path (reference dataset.py:546-557 setup_butter_filter, :1381-1400
__getitem__): the choice rule, the filter design and the impulse response against the goldens, the two float64 sums against
the reference's items under the derived bound (tests/tools/filter_golden.py), and the plumbing from an experiment file /
the command line to the stores.  Figures: pytest -s."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'tools'))

import filter_golden as G  # noqa: E402
from deepards_amd import filters as F  # noqa: E402

CASE_NAMES = ['lowpass_0p25', 'low0_lowpass_0p03125', 'highpass_15', 'high25_highpass_24', 'bandpass_2_3', 'bandpass_1em8_5',
              'fft_0_0p25', 'fft_0_20', 'lowpass_10_fft_0_6']


def test_the_goldens_are_the_cases_the_tests_name():
    assert sorted(c.name for c in G.cases()) == sorted(CASE_NAMES)
    for c in G.cases():
        assert c.x.shape == c.expected.shape == (20, 1, 224) and c.x.dtype == c.expected.dtype == np.float64


def test_choice_rule_restates_the_five_branches_in_the_reference_order():
    table = [
        ((0.25, None), ('lowpass', 0.25)),          # low alone
        ((0, None), ('lowpass', 0)),                # ... also for low == 0: the first branch wins
        ((0, 10), ('lowpass', 10)),                 # low == 0 -> lowpass(high)
        ((0, 25), ('lowpass', 25)),                 # ... before the high == 25 branch
        ((None, 15), ('highpass', 15)),             # high alone -> HIGHPASS(high)
        ((None, 25), ('highpass', 25)),
        ((24, 25), ('highpass', 24)),               # high == 25 -> highpass(low)
        ((2, 3), ('bandpass', (2, 3))),             # both
        ((1e-8, 5), ('bandpass', (1e-8, 5))),
        ((None, None), None),                       # neither: no filter
    ]
    for (low, high), want in table:
        assert F.butter_choice(low, high) == want, (low, high)
    assert F.butter_sos(None, None) is None
    seen = set()
    for c in G.cases():
        choice = F.butter_choice(c.keys['butter_low'], c.keys['butter_high'])
        assert (None if choice is None else choice[0]) == c.btype, c
        sos = F.butter_sos(c.keys['butter_low'], c.keys['butter_high'])
        if c.sos is None:
            assert sos is None, c
        else:
            assert sos.dtype == np.float64 and np.array_equal(sos, c.sos), c        # the same designer, the same arguments
            seen.add((c.btype, c.keys['butter_low'] is None, c.keys['butter_high'] is None, c.keys['butter_low'] == 0,
                      c.keys['butter_high'] == 25))
    assert len(seen) >= 5                            # the goldens reach every branch


@pytest.mark.parametrize('name', [n for n in CASE_NAMES if not n.startswith('fft')])
def test_impulse_response_equals_sosfilt_on_a_unit_impulse(name):
    """The numpy cascade runs sosfilt's recurrence -- the same IEEE operations in the same order -- so it normally has the
    golden's bits.  Held to |dh| <= 2^-36 max|h|: an error of that size moves an output by at most L 2^-36 max|h| max|x|,
    a twentieth of a float32 ulp of that product at L = 224."""
    c = G.case(name)
    h = F.impulse_response(c.sos, 224)
    assert h.dtype == np.float64 and h.shape == (224,)
    err = np.abs(h - c.h).max()
    print('%s: max |h - golden| %.3e (max |h| %.3e), bit-equal: %s' % (name, err, np.abs(c.h).max(), np.array_equal(h, c.h)))
    assert err <= 2.0 ** -36 * np.abs(c.h).max()
    assert np.array_equal(F.impulse_response(c.sos, 100), h[:100])          # a shorter row: the same leading samples


def test_impulse_response_does_not_need_scipy(monkeypatch):
    c = G.case('bandpass_2_3')
    want = F.impulse_response(c.sos, 64)
    for mod in [m for m in sys.modules if m == 'scipy' or m.startswith('scipy.')]:
        monkeypatch.setitem(sys.modules, mod, None)                          # any import of scipy now raises
    monkeypatch.setitem(sys.modules, 'scipy', None)
    assert np.array_equal(F.impulse_response(c.sos, 64), want)
    assert F.filter_kernels() == (None, None)
    with pytest.raises(ValueError):
        F.impulse_response(np.zeros((2, 5)), 8)


def test_fft_band_kernel_is_the_mask_of_the_reference():
    for c in G.cases():
        g = F.fft_band_kernel(c.keys['fft_filtering_low'], c.keys['fft_filtering_high'])
        if c.g is None:
            assert g is None, c
        else:
            assert g.shape == (224,) and g.dtype == np.float64 and np.array_equal(g, c.g), c
    # strict inequalities: low = 0 removes DC, and the bounds themselves are out
    spectrum = np.fft.fft(F.fft_band_kernel(0, 0.5)).real.round(12)
    freqs = np.abs(np.fft.fftfreq(224, d=0.02))
    assert spectrum[0] == 0 and np.array_equal(spectrum != 0, (freqs > 0) & (freqs < 0.5))
    edge = freqs[1]                                                           # the first bin: < is strict
    assert not np.fft.fft(F.fft_band_kernel(0, edge)).real.round(12).any()
    assert abs(np.fft.ifft(np.ones(224)).real - F.fft_band_kernel(-1, 26)).max() == 0          # everything passes: delta


def test_only_one_of_the_fft_pair_means_no_filter():
    assert F.fft_band_kernel(0, None) is None and F.fft_band_kernel(None, 6) is None
    assert F.filter_kernels(fft_filtering_low=0) == (None, None)
    assert F.filter_kernels(fft_filtering_high=6) == (None, None)
    h, g = F.filter_kernels(butter_low=1, fft_filtering_high=6)
    assert h is not None and g is None


@pytest.mark.parametrize('name', CASE_NAMES)
def test_apply_host_reproduces_the_reference_item_under_the_bound(name):
    c = G.case(name)
    h, g = F.filter_kernels(L=224, **c.keys)
    assert (h is None) == (c.h is None) and (g is None) == (c.g is None)
    xn = (c.x - c.mu) / c.std
    got = F.apply_host(xn, h, g)
    assert got.dtype == np.float64 and got.shape == c.expected.shape
    print('%s: float64 max |got - ref| %.3e' % (name, np.abs(got - c.expected).max()))
    G.check(name, got.astype(np.float32), c.expected, G.bound(c.expected, xn, h, g, F.apply_host))


def test_apply_host_identities():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((3, 2, 224))
    delta = np.zeros(224)
    delta[0] = 1.0
    assert np.array_equal(F.apply_host(x), x)
    assert np.array_equal(F.apply_host(x, delta, delta), x)
    shift = np.roll(delta, 5)
    assert np.array_equal(F.apply_host(x, None, shift), np.roll(x, 5, axis=-1))            # circular
    causal = F.apply_host(x, shift, None)
    assert np.array_equal(causal[..., 5:], x[..., :-5]) and not causal[..., :5].any()      # causal, zero state
    with pytest.raises(ValueError):
        F.apply_host(x, delta[:10])


# ---- plumbing -------------------------------------------------------------------------------------------------------------
class FakeStore(object):
    def __init__(self):
        self.filters = 'never set'

    def set_filters(self, **kw):
        self.filters = kw
        return self


def _driver(args):
    """A CNNLinearModel around ``args`` without its constructor (which wants a GPU): get_base_datasets only reads args."""
    from deepards_amd import train_ards_detector as T
    obj = object.__new__(T.CNNLinearModel)
    obj.args = args
    return obj


def test_experiment_file_keys_reach_the_stores(tmp_path):
    from deepards_amd import train_ards_detector as T
    from deepards_amd.config import Configuration
    over = tmp_path / 'butter.yml'
    over.write_text('butter_low: 0\nbutter_high: 10\nfft_filtering_low: 0\nfft_filtering_high: 6.5\n')
    args = Configuration(T.build_parser().parse_args(['-co', str(over)]), T.BUILD_DEFAULTS)
    assert (args.butter_low, args.butter_high, args.fft_filtering_low, args.fft_filtering_high) == (0, 10, 0, 6.5)
    args.train_store, args.test_store = FakeStore(), FakeStore()
    train, test = _driver(args).get_base_datasets()
    want = dict(butter_low=0, butter_high=10, fft_filtering_low=0, fft_filtering_high=6.5)
    assert train.filters == want and test.filters == want
    # the command line beats the file; a key nobody gives is None
    args = Configuration(T.build_parser().parse_args(['-co', str(over), '--butter-high', '3', '--fft-filtering-high', '20']),
                         T.BUILD_DEFAULTS)
    assert (args.butter_low, args.butter_high, args.fft_filtering_low, args.fft_filtering_high) == (0, 3.0, 0, 20.0)
    bare = Configuration(T.build_parser().parse_args([]), T.BUILD_DEFAULTS)
    assert (bare.butter_low, bare.butter_high, bare.fft_filtering_low, bare.fft_filtering_high) == (None,) * 4
    # make_args: absent keys are None and leave handed-in stores alone; given keys reach them
    a = T.make_args(train_store=FakeStore(), test_store=FakeStore())
    assert (a.butter_low, a.butter_high, a.fft_filtering_low, a.fft_filtering_high) == (None,) * 4
    train, test = _driver(a).get_base_datasets()
    assert train.filters == test.filters == 'never set'
    a = T.make_args(train_store=FakeStore(), test_store=FakeStore(), butter_high=15)
    train, test = _driver(a).get_base_datasets()
    assert train.filters == test.filters == dict(butter_low=None, butter_high=15, fft_filtering_low=None, fft_filtering_high=None)


def test_the_pickle_path_sets_the_filters_on_train_and_holdout_test_stores(monkeypatch):
    """--train-from-pickle / --test-from-pickle (the fixture, on the CPU): both stores carry the kernels of the keys."""
    from deepards_amd import train_ards_detector as T
    fixture = os.path.join(G.GOLD, 'test_dataset.npz')
    a = T.make_args(train_from_pickle=fixture, test_from_pickle=fixture, butter_low=0, butter_high=10, fft_filtering_low=0,
                    fft_filtering_high=6)
    obj = _driver(a)
    obj.device = 'cpu'
    train, test = obj.get_base_datasets()
    c = G.case('lowpass_10_fft_0_6')
    for store in (train, test):
        assert (store.butter_low, store.butter_high, store.fft_filtering_low, store.fft_filtering_high) == (0, 10, 0, 6)
        assert store.filter_h.dtype == torch.float64 and np.array_equal(store.filter_g.numpy(), c.g)
        assert np.abs(store.filter_h.numpy() - c.h).max() <= 2.0 ** -36 * np.abs(c.h).max()
    # a k-fold run: the test store is made from the train store and inherits them
    a = T.make_args(train_from_pickle=fixture, kfolds=2, butter_high=15)
    obj = _driver(a)
    obj.device = 'cpu'
    train, test = obj.get_base_datasets()
    assert test is not train and test.filter_h is train.filter_h and test.filter_g is None and test.butter_high == 15


def test_the_three_new_flags_parse_and_the_two_old_refusals_stand():
    from deepards_amd import train_ards_detector as T
    ns = T.build_parser().parse_args(['--butter-high', '15', '--fft-filtering-low', '0', '--fft-filtering-high', '0.25'])
    assert (ns.butter_high, ns.fft_filtering_low, ns.fft_filtering_high) == (15.0, 0.0, 0.25)
    assert all(isinstance(v, float) for v in (ns.butter_high, ns.fft_filtering_low, ns.fft_filtering_high))
    assert all(v is None for v in vars(T.build_parser().parse_args([])).values())
    for flag in ('--butter-high', '--fft-filtering-low', '--fft-filtering-high'):
        assert flag not in T.OUT_OF_SCOPE_FLAGS
    for flag in ('--butter-low', '--post-hoc-downsampling'):
        assert flag in T.OUT_OF_SCOPE_FLAGS
        with pytest.raises(SystemExit, match='outside the accelerated'):
            T.main([flag, '1'])
        with pytest.raises(SystemExit, match='outside the accelerated'):
            T.main([flag + '=1'])


def _cpu_store(n=6, nb=2, c=1, l=224):
    from deepards_amd.data import DeviceTileStore
    rng = np.random.default_rng(0)
    tg = np.eye(2, dtype=np.float32)[np.arange(n) % 2]
    return DeviceTileStore(rng.standard_normal((n, nb, c, l)), tg, [0.0] * c, [1.0] * c, device='cpu')


def test_set_filters_on_the_store():
    store = _cpu_store()
    assert store.filter_h is None and store.filter_g is None and store.butter_low is None         # a fresh store: none
    assert store.set_filters(butter_low=0.25, fft_filtering_low=0, fft_filtering_high=20) is store
    c, f = G.case('lowpass_0p25'), G.case('fft_0_20')
    assert store.filter_h.dtype == store.filter_g.dtype == torch.float64
    assert np.array_equal(store.filter_h.numpy(), F.impulse_response(c.sos, 224)) and np.array_equal(store.filter_g.numpy(), f.g)
    store.set_filters(fft_filtering_low=0)                                                        # half a pair: no filter
    assert store.filter_h is None and store.filter_g is None
    store.set_filters(butter_high=15)
    store.set_filters()
    assert store.filter_h is None and store.filter_g is None and store.butter_high is None


def test_an_fft_filter_on_512_sample_windows_raises_and_a_butter_filter_does_not():
    store = _cpu_store(n=2, l=512)
    with pytest.raises(ValueError, match='224'):
        store.set_filters(fft_filtering_low=0, fft_filtering_high=6)
    assert store.filter_g is None and store.filter_h is None                                      # nothing half-set
    store.set_filters(butter_low=1, butter_high=3)
    assert store.filter_h.shape == (512,) and store.filter_g is None
    store.set_filters(fft_filtering_low=0)                                                        # inactive: fine at any L
    with pytest.raises(ValueError, match='512'):
        _cpu_store(n=2, l=600).set_filters(butter_low=1)


def test_the_kfold_test_store_inherits_the_filters():
    store = _cpu_store(n=8).enable_kfolds(np.arange(8), 2)
    store.set_filters(butter_low=2, butter_high=3, fft_filtering_low=0, fft_filtering_high=6)
    test = store.make_test_store_if_kfold()
    assert test.filter_h is store.filter_h and test.filter_g is store.filter_g
    assert (test.butter_low, test.butter_high, test.fft_filtering_low, test.fft_filtering_high) == (2, 3, 0, 6)
    assert test.train is False and store.train is True
