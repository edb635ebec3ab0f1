"""CPU tests of padded breath-by-breath datasets and post-hoc downsampling in the batch path (reference dataset.py:1375-1391):
the resampling matrix against scipy, the padded normalisation, the host chain against the goldens under the derived bound
and cap (tests/tools/padded_golden.py), and the plumbing from a dataset's type / an experiment file to the stores.
Figures: pytest -s."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'tools'))

import padded_golden as G  # noqa: E402
from deepards_amd import filters as F  # noqa: E402

CASE_NAMES = ['only', 'down_2', 'down_2p5', 'down_25', 'down_1p2', 'bandpass_5_10', 'lowpass_10_down_4', 'down_3_fft_0_6',
              'highpass_15_down_1p4_fft_0_20', 'lowpass_10_down_1p2', 'unpadded_down_2']
REFERENCE_FACTORS = (1.2, 1.4, 1.6, 1.8, 2.0, 2.5, 3.0, 3.5, 4.0, 6.0, 8.0, 10.0, 15.0, 20.0, 25.0)     # its 15 experiment files
FIXTURE = os.path.join(G.GOLD, 'test_dataset.npz')


def stages(c):
    """(h, r, g) of a golden case, from the package's own design."""
    h, g = F.filter_kernels(L=224, **c.keys)
    r = None if c.factor is None else F.resample_matrix(224, F.post_hoc_new_len(224, c.factor))
    return h, r, g


def test_the_goldens_are_the_cases_the_tests_name():
    assert sorted(c.name for c in G.cases()) == sorted(CASE_NAMES)
    for c in G.cases():
        assert c.x.shape == c.expected.shape == (20, 1, 224) and c.x.dtype == c.expected.dtype == np.float64
        assert c.lengths[0] == 224 and c.lengths.min() >= 30 and c.lengths.max() <= 224
        assert c.padded == (c.name != 'unpadded_down_2')
        if c.padded:
            for row, n in enumerate(c.lengths):
                assert not c.x[row, 0, n:].any()
            assert c.x[3, 0, c.lengths[3] // 2] == 0.0 and c.lengths[3] // 2 < c.lengths[3] - 1      # the interior zero
            assert (c.lengths < 224).sum() >= 10
    assert {c.new_len for c in G.cases()} == {0, 112, 89, 8, 186, 56, 74, 160}


@pytest.mark.parametrize('L', [224, 512])
def test_resample_matrix_is_scipy_resample_on_the_unit_vectors(L):
    """Every new_len the reference's 15 factors give, at both row lengths, and new_len = 1 / L.  Both sides run the same
    steps on exact 0/1 inputs; held to 4 ulp of the largest entry (which is <= 1)."""
    from scipy.signal import resample
    lens = sorted({F.post_hoc_new_len(L, f) for f in REFERENCE_FACTORS} | {1, 2, L - 1, L})
    for n in lens:
        r = F.resample_matrix(L, n)
        assert r.shape == (n, L) and r.dtype == np.float64 and r.flags['C_CONTIGUOUS']
        want = resample(np.eye(L), n, axis=0)
        err = np.abs(r - want).max()
        assert err <= 4 * 2.0 ** -52, (L, n, err)
    x = np.random.default_rng(L).standard_normal((3, L))
    n = F.post_hoc_new_len(L, 2.5)
    assert np.abs(x @ F.resample_matrix(L, n).T - resample(x, n, axis=-1)).max() <= 1e-13
    assert np.abs(F.resample_matrix(L, L) - np.eye(L)).max() <= 4 * 2.0 ** -52          # new_len == L: the identity
    for bad in (0, L + 1, -3):
        with pytest.raises(ValueError):
            F.resample_matrix(L, bad)


def test_post_hoc_new_len_values_and_refusals():
    want = dict(zip(REFERENCE_FACTORS, (186, 160, 140, 124, 112, 89, 74, 64, 56, 37, 28, 22, 14, 11, 8)))
    for f, n in want.items():
        assert F.post_hoc_new_len(224, f) == n and isinstance(F.post_hoc_new_len(224, f), int)
    assert F.post_hoc_new_len(224, 1) == 224 and F.post_hoc_new_len(224, 224) == 1 and F.post_hoc_new_len(512, 1.5) == 341
    for bad in (0.99, 0.5, 224.5, 1000, 0, -2.0, float('nan')):    # below 1: np.pad raises in the reference; above L: nothing is left
        with pytest.raises(ValueError):
            F.post_hoc_new_len(224, bad)


@pytest.mark.parametrize('name', CASE_NAMES)
def test_host_chain_reproduces_the_reference_item_under_the_bound(name):
    """Measured (numpy 2, scipy 1.15.3): 0 significant elements differ in every case; lowpass_10_down_1p2 differs in 371
    elements below the floor, worst error 6.3e-3 of the bound; every other case equals float32(ref) in every element."""
    c = G.case(name)
    h, r, g = stages(c)
    assert (r is None) == (c.new_len == 0) and (r is None or r.shape == (c.new_len, 224))
    xn = F.normalize_host(c.x, c.mu, c.std, c.padded)
    got = F.apply_host(xn, h, g, r)
    assert got.dtype == np.float64 and got.shape == c.expected.shape
    if c.new_len:
        assert not got[..., c.new_len:].any() or g is not None            # zeros behind new_len (until the FFT stage mixes them)
    G.check(name, got.astype(np.float32), c.expected, G.bound(c.expected, xn, h, r, g))


def test_padded_normalisation_keeps_zeros_and_is_the_plain_expression_elsewhere():
    c = G.case('only')
    got = F.normalize_host(c.x, c.mu, c.std, padded=True)
    plain = (c.x - c.mu) / c.std
    zero = c.x == 0
    assert zero.sum() > 100 and (~zero).sum() > 100
    assert np.array_equal(got[zero], np.zeros(zero.sum())) and not np.signbit(got[zero]).any()
    assert np.array_equal(got[~zero].view(np.int64), plain[~zero].view(np.int64))
    assert np.array_equal(got, c.expected)                                 # no stage: the reference's item itself
    assert np.array_equal(F.normalize_host(c.x, c.mu, c.std).view(np.int64), plain.view(np.int64))
    # a NaN is non-zero (np.put(..., data.ravel() != 0, ...)); per-channel factors
    x = np.array([[[0.0, 2.0, np.nan]], [[4.0, 0.0, -0.0]]]).transpose(1, 0, 2)          # (1, C = 2, 3)
    got = F.normalize_host(x, (1.0, 2.0), (2.0, 4.0), padded=True)
    assert np.array_equal(got[0, 0, :2], [0.0, 0.5]) and np.isnan(got[0, 0, 2])
    assert np.array_equal(got[0, 1], [0.5, 0.0, -0.0])


def test_apply_host_resample_stage():
    x = np.random.default_rng(5).standard_normal((2, 3, 224))
    top = np.eye(224)[:100]                                                # R = [I; 0]: the first 100 samples, zeros behind
    got = F.apply_host(x, r=top)
    assert np.array_equal(got[..., :100], x[..., :100]) and not got[..., 100:].any()
    assert np.array_equal(F.apply_host(x), x)
    for bad in (np.eye(224)[:, :100], np.eye(225), np.zeros((0, 224))):
        with pytest.raises(ValueError):
            F.apply_host(x, r=bad)


# ---- plumbing -------------------------------------------------------------------------------------------------------------
class FakeStore(object):
    def __init__(self):
        self.filters = 'never set'

    def set_filters(self, **kw):
        self.filters = kw
        return self


def _driver(args, device=None):
    """A CNNLinearModel around ``args`` without its constructor (which wants a GPU): get_base_datasets only reads args."""
    from deepards_amd import train_ards_detector as T
    obj = object.__new__(T.CNNLinearModel)
    obj.args = args
    if device:
        obj.device = device
    return obj


def test_experiment_file_key_and_make_args_reach_the_stores(tmp_path):
    from deepards_amd import train_ards_detector as T
    from deepards_amd.config import Configuration
    over = tmp_path / 'downsamp.yml'
    over.write_text('dataset_type: padded_breath_by_breath\npost_hoc_downsampling: 2.5\nbutter_high: 15\n')
    args = Configuration(T.build_parser().parse_args(['-co', str(over)]), T.BUILD_DEFAULTS)
    assert args.post_hoc_downsampling == 2.5 and args.dataset_type == 'padded_breath_by_breath'
    args.train_store, args.test_store = FakeStore(), FakeStore()
    train, test = _driver(args).get_base_datasets()
    want = dict(butter_low=None, butter_high=15, fft_filtering_low=None, fft_filtering_high=None, post_hoc_downsampling=2.5)
    assert train.filters == want and test.filters == want
    assert Configuration(T.build_parser().parse_args([]), T.BUILD_DEFAULTS).post_hoc_downsampling is None
    assert T.build_parser().parse_args(['-dt', 'padded_breath_by_breath']).dataset_type == 'padded_breath_by_breath'
    a = T.make_args(train_store=FakeStore(), test_store=FakeStore())
    assert a.post_hoc_downsampling is None
    train, test = _driver(a).get_base_datasets()
    assert train.filters == test.filters == 'never set'
    a = T.make_args(train_store=FakeStore(), test_store=FakeStore(), post_hoc_downsampling=4.0)
    train, test = _driver(a).get_base_datasets()
    assert train.filters == test.filters == dict(butter_low=None, butter_high=None, fft_filtering_low=None,
                                                 fft_filtering_high=None, post_hoc_downsampling=4.0)


def test_the_pickle_path_sets_downsampling_on_train_kfold_test_and_holdout_test_stores():
    from deepards_amd import train_ards_detector as T
    want = F.resample_matrix(224, 112)
    a = T.make_args(train_from_pickle=FIXTURE, test_from_pickle=FIXTURE, post_hoc_downsampling=2.0, butter_low=0, butter_high=10)
    train, test = _driver(a, 'cpu').get_base_datasets()
    for store in (train, test):
        assert store.post_hoc_downsampling == 2.0 and store.butter_high == 10 and store.filter_h is not None
        assert store.filter_r.dtype == torch.float64 and tuple(store.filter_r.shape) == (112, 224)
        assert store.filter_r.t().is_contiguous()                          # consecutive outputs lie side by side in memory
        assert np.array_equal(store.filter_r.numpy(), want)
        assert store.padded is False                                        # the fixture is unpadded_centered_sequences
    a = T.make_args(train_from_pickle=FIXTURE, kfolds=2, post_hoc_downsampling=25.0)
    train, test = _driver(a, 'cpu').get_base_datasets()
    assert test is not train and test.filter_r is train.filter_r and tuple(test.filter_r.shape) == (8, 224)
    assert test.post_hoc_downsampling == 25.0 and test.train is False
    # without the key: no R, and the store keeps today's paths
    train, test = _driver(T.make_args(train_from_pickle=FIXTURE, kfolds=2), 'cpu').get_base_datasets()
    assert train.filter_r is None and test.filter_r is None and train.post_hoc_downsampling is None


def test_a_padded_dataset_type_yields_a_padded_store_also_through_the_npz_round_trip(tmp_path):
    from deepards_amd import train_ards_detector as T
    from deepards_amd.ingest import load_dataset
    ds = load_dataset(FIXTURE)
    assert ds.dataset_type == 'unpadded_centered_sequences' and ds.to_store('cpu').padded is False
    for kind, padded in (('padded_breath_by_breath', True), ('padded_breath_by_breath_with_flow_time_features', True),
                         ('unpadded_centered_sequences', False), ('unpadded_downsampled_sequences', False)):
        ds.dataset_type = kind
        assert ds.to_store('cpu').padded is padded, kind
        path = str(tmp_path / (kind + '.npz'))
        ds.save_npz(path)
        back = load_dataset(path)
        assert back.dataset_type == kind and back.to_store('cpu').padded is padded, kind
        # ... and through the driver: train, k-fold test and holdout test stores
        train, test = _driver(T.make_args(train_from_pickle=path, test_from_pickle=path), 'cpu').get_base_datasets()
        assert train.padded is padded and test.padded is padded, kind
        train, test = _driver(T.make_args(train_from_pickle=path, kfolds=2), 'cpu').get_base_datasets()
        assert train.padded is padded and test.padded is padded, kind


def _cpu_store(n=6, nb=2, c=1, l=224):
    from deepards_amd.data import DeviceTileStore
    rng = np.random.default_rng(0)
    tg = np.eye(2, dtype=np.float32)[np.arange(n) % 2]
    return DeviceTileStore(rng.standard_normal((n, nb, c, l)), tg, [0.0] * c, [1.0] * c, device='cpu')


def test_set_filters_keeps_r_and_a_constructed_store_has_neither():
    store = _cpu_store()
    assert store.padded is False and store.filter_r is None and store.post_hoc_downsampling is None
    assert store.set_filters(post_hoc_downsampling=1.2) is store
    assert tuple(store.filter_r.shape) == (186, 224) and store.filter_h is None and store.filter_g is None
    store.set_filters(butter_high=15)                                      # the key is a keyword like the others: absent, gone
    assert store.filter_r is None and store.post_hoc_downsampling is None and store.filter_h is not None
    for bad in (0.5, 300, 0):
        with pytest.raises(ValueError):
            store.set_filters(post_hoc_downsampling=bad)
    big = _cpu_store(n=2, l=512).set_filters(post_hoc_downsampling=1.5)
    assert tuple(big.filter_r.shape) == (341, 512)
    with pytest.raises(ValueError, match='512'):
        _cpu_store(n=2, l=600).set_filters(post_hoc_downsampling=2.0)
    kf = _cpu_store(n=8).enable_kfolds(np.arange(8), 2).set_filters(post_hoc_downsampling=2.0)
    kf.padded = True
    test = kf.make_test_store_if_kfold()
    assert test.padded is True and test.filter_r is kf.filter_r and test.train is False


def test_post_hoc_downsampling_is_still_refused_on_the_command_line():
    from deepards_amd import train_ards_detector as T
    assert '--post-hoc-downsampling' in T.OUT_OF_SCOPE_FLAGS
    for argv in (['--post-hoc-downsampling', '2.0'], ['--post-hoc-downsampling=2.0']):
        with pytest.raises(SystemExit, match='experiment file'):
            T.main(argv)
    with pytest.raises(SystemExit):
        T.build_parser().parse_args(['--post-hoc-downsampling', '2.0'])     # the parser does not know it either
