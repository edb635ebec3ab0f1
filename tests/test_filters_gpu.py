"""GPU tests of ``da_gather_normalize_filter`` (csrc/filters.hip): the batch gather with the reference's Butterworth and FFT
band filters behind the normalisation (dataset.py:546-557, 1381-1400).  Results are held to the reference's items in
tests/golden/filter_*.npz under the derived bound of tests/tools/filter_golden.py; identities, repeats and the store are
held bit for bit.  Figures: pytest -s."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'tools'))
pytestmark = pytest.mark.gpu

import filter_golden as G  # noqa: E402
import poison as P  # noqa: E402
from deepards_amd import filters as F  # noqa: E402

CASE_NAMES = ['lowpass_0p25', 'low0_lowpass_0p03125', 'highpass_15', 'high25_highpass_24', 'bandpass_2_3', 'bandpass_1em8_5',
              'fft_0_0p25', 'fft_0_20', 'lowpass_10_fft_0_6']
FIXTURE = os.path.join(G.GOLD, 'test_dataset.npz')


@pytest.fixture(scope='module')
def H():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from deepards_amd import hip_ops
    return hip_ops


def dev(a, dtype=torch.float64):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def delta(l):
    d = np.zeros(l)
    d[0] = 1.0
    return d


# ---- 1. the goldens ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('idx', [[2, 0, 2], [0]], ids=['idx202', 'B1'])
@pytest.mark.parametrize('name', CASE_NAMES)
def test_golden_cases_through_the_wrapper(H, name, idx):
    """tiles[2] is the golden's window, tiles[0] the same window with its rows in reverse order (rows are filtered one by
    one, so its item is the golden's with the rows reversed), tiles[1] is NaN and never picked.
    Measured on an MI355X: eight cases equal float32(ref) in every element; bandpass_1em8_5 differs in 1 of 4480 elements per
    window by one float32 ulp (2.98e-8, error / bound 1.000)."""
    c = G.case(name)
    tiles = np.stack([c.x[::-1], np.full_like(c.x, np.nan), c.x])
    item = {0: c.expected[::-1], 2: c.expected}
    xn = {0: ((c.x - c.mu) / c.std)[::-1], 2: (c.x - c.mu) / c.std}
    h, g = F.filter_kernels(L=224, **c.keys)
    got = H.gather_normalize_filter(dev(tiles), dev(idx, torch.int64), c.mu, c.std, dev(h), dev(g))
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(idx), 20, 1, 224)
    ref = np.stack([item[i] for i in idx])
    limit = G.bound(ref, np.stack([xn[i] for i in idx]), h, g, F.apply_host)
    G.check('%s idx %s' % (name, idx), got.cpu().numpy(), ref, limit)


# ---- 2. identity filters ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('chans', [1, 3])
def test_identity_filters_are_bit_identical_to_gather_normalize(H, chans):
    rng = np.random.default_rng(chans)
    tiles = dev(rng.standard_normal((5, 4, chans, 224)) * 30 + 2)
    idx = dev([3, 0, 3, 4], torch.int64)
    mu, std = (2.05, 28.3) if chans == 1 else ((2.05, -0.4, 11.0), (28.3, 3.5, 0.75))
    plain = H.gather_normalize(tiles, idx, mu, std)
    d = dev(delta(224))
    for h, g in ((d, d), (d, None), (None, d)):
        got = H.gather_normalize_filter(tiles, idx, mu, std, h, g)
        assert P.same_bits(got, plain), P.diff_report(got, plain)
    if chans == 3:                                            # per-channel factors really are per channel
        swapped = H.gather_normalize_filter(tiles, idx, mu[::-1], std[::-1], d, d)
        assert not P.same_bits(swapped, plain)


# ---- 3. more outputs than threads -------------------------------------------------------------------------------------------
def test_butter_only_on_512_sample_rows(H):
    """L = 512 (the C5 tile shape), NB = 2, two channels: every thread owns two outputs; against apply_host in float64."""
    rng = np.random.default_rng(512)
    tiles = rng.standard_normal((4, 2, 2, 512)) * 25 + 1.5
    idx = [1, 3, 1]
    mu, std = np.array([1.5, -2.0]), np.array([25.0, 19.0])
    h = F.filter_kernels(butter_low=2, butter_high=3, L=512)[0]
    assert h.shape == (512,)
    xn = (tiles[idx] - mu.reshape(1, 1, 2, 1)) / std.reshape(1, 1, 2, 1)
    ref = F.apply_host(xn, h, None)
    got = H.gather_normalize_filter(dev(tiles), dev(idx, torch.int64), tuple(mu), tuple(std), dev(h), None)
    assert tuple(got.shape) == (3, 2, 2, 512)
    G.check('butter L 512', got.cpu().numpy(), ref, G.bound(ref, xn, h, None, F.apply_host))
    assert P.same_bits(got[0], got[2])


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_leave_out_untouched(H):
    from deepards_amd import _lib
    rng = np.random.default_rng(4)
    t224, t512 = dev(rng.standard_normal((3, 2, 1, 224))), dev(rng.standard_normal((3, 2, 1, 512)))
    idx = dev([2, 0], torch.int64)
    k224, k512 = dev(delta(224)), dev(delta(512))
    poisoned = lambda *shape, dtype=torch.float32: P.fill_poison(torch.empty(shape, dtype=dtype, device='cuda'))
    o224, o512 = poisoned(2, 2, 1, 224), poisoned(2, 2, 1, 512)
    calls = [
        ('g on rows of 512 samples', lambda: H.gather_normalize_filter(t512, idx, 0.0, 1.0, None, k512, out=o512)),
        ('g of 224 samples on rows of 512', lambda: H.gather_normalize_filter(t512, idx, 0.0, 1.0, k512, k224, out=o512)),
        ('no filter at all', lambda: H.gather_normalize_filter(t224, idx, 0.0, 1.0, None, None, out=o224)),
        ('h of the wrong length', lambda: H.gather_normalize_filter(t224, idx, 0.0, 1.0, k512, None, out=o224)),
        ('float32 h', lambda: H.gather_normalize_filter(t224, idx, 0.0, 1.0, k224.float(), None, out=o224)),
        ('out of the wrong shape', lambda: H.gather_normalize_filter(t224, idx, 0.0, 1.0, k224, k224, out=o512)),
        ('out with a window too many', lambda: H.gather_normalize_filter(t224, idx, 0.0, 1.0, k224, k224, out=poisoned(3, 2, 1, 224))),
        ('one factor for one channel', lambda: H.gather_normalize_filter(t224, idx, (0.0, 1.0), (1.0, 2.0), k224, None, out=o224)),
    ]
    for what, call in calls:
        with pytest.raises(ValueError):
            call()
        assert P.count_poison(o224) == o224.numel() and P.count_poison(o512) == o512.numel(), what
    o64 = poisoned(2, 2, 1, 224, dtype=torch.float64)
    with pytest.raises(ValueError):
        H.gather_normalize_filter(t224, idx, 0.0, 1.0, k224, k224, out=o64)
    assert P.count_poison(o64) == o64.numel()
    # the entry point itself: an error code before any launch
    entry = _lib.lib().da_gather_normalize_filter
    one = lambda v: (ctypes.c_double * 1)(v)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for what, tiles, h, g, out, l, std in (('g, L 512', t512, None, k512, o512, 512, 1.0), ('both null', t224, None, None, o224, 224, 1.0),
                                           ('h, L 513', t512, k512, None, o512, 513, 1.0), ('std 0', t224, k224, None, o224, 224, 0.0)):
        assert entry(p(tiles), p(idx), one(0.0), one(std), p(h), p(g), p(out), 2, 2, 1, l, stream) == -1, what
    assert entry(p(t224), p(idx), one(0.0), one(1.0), p(k224), None, p(o224), 2, 2, 5, 224, stream) == -1        # C > 4
    assert entry(p(t224), p(idx), one(0.0), one(1.0), p(k224), None, None, 2, 2, 1, 224, stream) == -1          # no out
    torch.cuda.synchronize()
    assert P.count_poison(o224) == o224.numel() and P.count_poison(o512) == o512.numel()
    assert tuple(H.gather_normalize_filter(t224, idx[:0], 0.0, 1.0, k224, None).shape) == (0, 2, 1, 224)          # B = 0: nothing to do


# ---- 5. memory discipline ---------------------------------------------------------------------------------------------------
def _rows(n, nb, c, l, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((n, nb, c, l), generator=g, dtype=torch.float64) * 20 + 1).cuda()


def _cases(H):
    zeros = lambda *s: torch.zeros(s, dtype=torch.float32, device='cuda')
    c17 = G.case('lowpass_10_fft_0_6')
    h224, g224 = F.filter_kernels(L=224, **c17.keys)
    h512 = F.filter_kernels(butter_high=15, L=512)[0]

    def b_both():
        return dict(tiles=_rows(6, 20, 1, 224, 1), idx=dev([5, 0, 3, 3, 1], torch.int64), h=dev(h224), g=dev(g224), o1=zeros(5, 20, 1, 224))

    def b_c3():
        return dict(tiles=_rows(4, 3, 3, 512, 2), idx=dev([3, 3, 0], torch.int64), h=dev(h512), o1=zeros(3, 3, 3, 512))

    def b_g():
        return dict(tiles=_rows(3, 1, 2, 224, 3), idx=dev([1], torch.int64), g=dev(g224), o1=zeros(1, 1, 2, 224))

    def b_src():
        return dict(tiles=_rows(7, 2, 1, 224, 4), h=dev(h224), g=dev(g224))
    return [
        P.OpCase('filter_both_c1', 'filter', b_both,
                 lambda tiles, idx, h, g, o1: (H.gather_normalize_filter(tiles, idx, 0.25, 1.5, h, g, out=o1),
                                               H.gather_normalize_filter(tiles, idx, 0.25, 1.5, h, g)), dests=('o1',),
                 note='rows are picked through idx: isolation is checked by filter_source_rows'),
        P.OpCase('filter_h_l512_c3', 'filter', b_c3,
                 lambda tiles, idx, h, o1: (H.gather_normalize_filter(tiles, idx, (0.1, 0.2, 0.3), (1.0, 2.0, 3.0), h, None, out=o1),
                                            H.gather_normalize_filter(tiles, idx, (0.1, 0.2, 0.3), (1.0, 2.0, 3.0), h)), dests=('o1',)),
        P.OpCase('filter_g_b1_c2', 'filter', b_g,
                 lambda tiles, idx, g, o1: (H.gather_normalize_filter(tiles, idx, (0.1, 0.2), (1.0, 2.0), None, g, out=o1),
                                            H.gather_normalize_filter(tiles, idx, (0.1, 0.2), (1.0, 2.0), g=g)), dests=('o1',)),
        P.OpCase('filter_source_rows', 'filter', b_src,
                 lambda tiles, h, g: H.gather_normalize_filter(tiles, torch.arange(7, device='cuda'), 0.25, 1.5, h, g),
                 rows=dict(inputs=('tiles',), R=1)),
    ]


@pytest.mark.parametrize('check', P.CHECKS)
def test_memory_discipline_rows(H, check):
    """The five checks of tests/tools/poison.py on the wrapper: poisoned allocations, guard bands around every operand and
    around out, a dirty out, a NaN window staying in its own rows, a repeat after another shape."""
    cases = _cases(H)
    problems = []
    for i, case in enumerate(cases):
        problems += P.run_check(check, case, other=cases[(i + 1) % len(cases)])
    assert not problems, '\n'.join(problems)


def test_out_form_returns_out_and_inputs_stay_as_they_were(H):
    for case in _cases(H)[:3]:
        inputs = case.build()
        keep = {k: v.clone() for k, v in inputs.items() if k != 'o1'}
        handles = []

        def wrap(t, path):
            v, hd = P.guarded(t, name=path)
            handles.append(hd)
            return v
        guarded = P.map_tensors(inputs, wrap)
        P.fill_poison(guarded['o1'])
        with_out, fresh = case.call(**guarded)
        torch.cuda.synchronize()
        assert with_out is guarded['o1'] and fresh is not guarded['o1'], case.name
        assert P.same_bits(with_out.contiguous(), fresh) and not P.has_poison(with_out), case.name
        P.assert_guards_intact(handles)
        for k, v in keep.items():
            assert P.same_bits(guarded[k].contiguous(), v), '%s: input %s changed' % (case.name, k)


# ---- 6. repeats -------------------------------------------------------------------------------------------------------------
def test_two_calls_on_equal_inputs_are_bit_equal(H):
    c = G.case('lowpass_10_fft_0_6')
    h, g = F.filter_kernels(L=224, **c.keys)
    z = np.load(FIXTURE)
    idx = dev(np.arange(20)[::-1].copy(), torch.int64)
    first = H.gather_normalize_filter(dev(z['x']), idx, c.mu, c.std, dev(h), dev(g))
    again = H.gather_normalize_filter(dev(z['x']), idx.clone(), c.mu, c.std, dev(h), dev(g))
    assert P.same_bits(first, again), P.diff_report(first, again)


# ---- 7. the store -----------------------------------------------------------------------------------------------------------
def test_store_batches_equal_the_wrapper_bit_for_bit(H):
    from deepards_amd.data import DeviceTileStore
    z = np.load(FIXTURE)
    mu, std = float(z['mu']), float(z['std'])
    store = DeviceTileStore(z['x'], z['target'], mu, std)
    rel = [7, 0, 19, 7]
    plain = H.gather_normalize(store.tiles, dev(rel, torch.int64), mu, std)
    x, t = store.batch(rel)                                                     # no filter set: today's output
    assert P.same_bits(x, plain) and torch.equal(t, store.targets[rel])
    d = store.device_indices(rel)
    assert P.same_bits(store.batch_from_device(d)[0], plain)
    keys = dict(butter_low=0, butter_high=10, fft_filtering_low=0, fft_filtering_high=6)
    h, g = F.filter_kernels(L=224, **keys)
    for kw, hh, gg in ((keys, h, g), (dict(butter_low=0, butter_high=10), h, None), (dict(fft_filtering_low=0, fft_filtering_high=6), None, g)):
        store.set_filters(**kw)
        want = H.gather_normalize_filter(store.tiles, dev(rel, torch.int64), mu, std, dev(hh), dev(gg))
        assert not P.same_bits(want, plain)
        x, t = store.batch(rel)
        assert P.same_bits(x, want) and torch.equal(t, store.targets[rel])
        x, t = store.batch_from_device(d)
        assert P.same_bits(x, want) and torch.equal(t, store.targets[rel])
        ox, ot = P.fill_poison(torch.empty_like(want)), torch.empty((4, 2), device='cuda')
        x, t = store.batch(rel, out=(ox, ot))                                   # out= buffers keep working
        assert x is ox and t is ot and P.same_bits(ox, want)
        x, t = store.batch_from_device(d[1:3], out=(ox[:2], ot[:2]))
        assert P.same_bits(x, want[1:3])
    # fold-relative indices and the k-fold test store
    store.set_filters(**keys)
    want = H.gather_normalize_filter(store.tiles, dev([19, 3], torch.int64), mu, std, dev(h), dev(g))
    store.set_kfold_indexes([3, 19])
    assert P.same_bits(store.batch([1, 0])[0], want)
    store.set_filters()
    store.set_kfold_indexes(None)
    assert P.same_bits(store.batch(rel)[0], plain)                              # cleared: today's output again


# ---- 8. the driver ----------------------------------------------------------------------------------------------------------
def test_driver_trains_and_tests_on_filtered_batches(H):
    """One train and one test epoch of CNNLinearModel with the four keys, on the ingested fixture (train and holdout test
    set), B = 2, resnet18, eager and captured: the same losses, and the first batch the model receives is the golden's
    item.  Both stores are narrowed to the golden's window (the fixture's window 17, three batches of it) so that the
    first batch is known whatever the shuffle does."""
    from deepards_amd import train_ards_detector as T
    c = G.case('lowpass_10_fft_0_6')
    assert c.window == 17
    runs = {}
    for use_graph in (False, True):
        args = T.make_args(base_network='resnet18', epochs=1, batch_size=2, seed=3, use_graph=use_graph, train_from_pickle=FIXTURE,
                           test_from_pickle=FIXTURE, **c.keys)
        cls = T.CNNLinearModel(args)
        made, seen = cls.get_base_datasets, []

        def narrowed():
            train, test = made()
            for store in (train, test):
                store.set_kfold_indexes([c.window] * 6)
            gather = train.batch_from_device

            def recording(abs_idx, out=None):
                x, t = gather(abs_idx, out=out)
                seen.append((abs_idx.clone(), x.clone()))
                return x, t
            train.batch_from_device = recording
            return train, test
        cls.get_base_datasets = narrowed
        res = cls.train_and_test()
        losses = res.get_meter('loss', 0)
        print('use_graph %s: train losses %s' % (use_graph, losses))
        assert len(losses) == 3 and np.isfinite(losses).all() and len(seen) == 3
        assert res.patient_results[(0, 1)]['votes'].sum() == 6                    # the test epoch ran on its 6 windows
        runs[use_graph] = (losses, seen)
    assert runs[False][0] == runs[True][0]
    for use_graph in (False, True):
        abs_idx, x = runs[use_graph][1][0]
        assert abs_idx.tolist() == [c.window, c.window] and tuple(x.shape) == (2, 20, 1, 224)
        h, g = F.filter_kernels(L=224, **c.keys)
        xn = np.stack([(c.x - c.mu) / c.std] * 2)
        ref = np.stack([c.expected] * 2)
        G.check('first batch, use_graph %s' % use_graph, x.cpu().numpy(), ref, G.bound(ref, xn, h, g, F.apply_host))
