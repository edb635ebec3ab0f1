"""GPU tests of ``da_gather_normalize_chain`` (csrc/filters.hip): the batch gather with the padded normalisation, the
Butterworth filter, post-hoc downsampling and the FFT band filter of ``ARDSRawDataset.__getitem__`` (dataset.py:1375-1400) in
one launch.  Results are held to the reference's items in tests/golden/padded_*.npz under the derived bound and cap of
tests/tools/padded_golden.py; identities, repeats and the store are held bit for bit.  Figures: pytest -s."""
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

import filter_golden as FG  # noqa: E402
import padded_golden as G  # noqa: E402
import poison as P  # noqa: E402
from deepards_amd import filters as F  # noqa: E402

CASE_NAMES = ['only', 'down_2', 'down_2p5', 'down_25', 'down_1p2', 'bandpass_5_10', 'lowpass_10_down_4', 'down_3_fft_0_6',
              'highpass_15_down_1p4_fft_0_20', 'lowpass_10_down_1p2', 'unpadded_down_2']
FIXTURE = os.path.join(G.GOLD, 'test_dataset.npz')


@pytest.fixture(scope='module')
def H():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from deepards_amd import hip_ops
    return hip_ops


def dev(a, dtype=torch.float64):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def rop(H, r):
    return None if r is None else H.resample_operand(r)


def delta(l):
    d = np.zeros(l)
    d[0] = 1.0
    return d


def stages(c):
    h, g = F.filter_kernels(L=224, **c.keys)
    r = None if c.factor is None else F.resample_matrix(224, F.post_hoc_new_len(224, c.factor))
    return h, r, g


# ---- 1. the goldens ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('idx', [[2, 0, 2], [0]], ids=['idx202', 'B1'])
@pytest.mark.parametrize('name', CASE_NAMES)
def test_golden_cases_through_the_wrapper(H, name, idx):
    """tiles[2] is the golden's window, tiles[0] the same window with its rows in reverse order (rows are processed one by
    one, so its item is the golden's with the rows reversed), tiles[1] is NaN and never picked.
    Measured on an MI355X: ten cases equal float32(ref) in every element; lowpass_10_down_1p2 differs in 372 of 4480 elements
    per window, none of them significant, worst error 6.3e-3 of the bound (2.8e-14)."""
    c = G.case(name)
    tiles = np.stack([c.x[::-1], np.full_like(c.x, np.nan), c.x])
    item = {0: c.expected[::-1], 2: c.expected}
    xn = F.normalize_host(c.x, c.mu, c.std, c.padded)
    xn = {0: xn[::-1], 2: xn}
    h, r, g = stages(c)
    got = H.gather_normalize_chain(dev(tiles), dev(idx, torch.int64), c.mu, c.std, c.padded, dev(h), rop(H, r), dev(g))
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(idx), 20, 1, 224)
    ref = np.stack([item[i] for i in idx])
    got = got.cpu().numpy()
    if c.new_len and g is None:
        assert not got[..., c.new_len:].any()                                  # exact zeros behind new_len
    if c.padded and h is None and r is None and g is None:
        assert not got[np.stack([tiles[i] for i in idx]) == 0].any()           # padding stays exactly 0
    G.check('%s idx %s' % (name, idx), got, ref, G.bound(ref, np.stack([xn[i] for i in idx]), h, r, g))


# ---- 2. identities ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('chans', [1, 3])
def test_unpadded_chain_without_r_has_the_bits_of_the_existing_gathers(H, chans):
    rng = np.random.default_rng(chans)
    tiles = dev(rng.standard_normal((5, 5, chans, 224)) * 30 + 2)              # 5 x 5 x C rows: no multiple of the row group
    idx = dev([3, 0, 3, 4, 1], torch.int64)
    mu, std = (2.05, 28.3) if chans == 1 else ((2.05, -0.4, 11.0), (28.3, 3.5, 0.75))
    plain = H.gather_normalize(tiles, idx, mu, std)
    d = dev(delta(224))
    for h, g in ((None, None), (d, d), (d, None), (None, d)):
        got = H.gather_normalize_chain(tiles, idx, mu, std, False, h, None, g)
        assert P.same_bits(got, plain), P.diff_report(got, plain)
    assert P.same_bits(H.gather_normalize_chain(tiles, idx, mu, std), plain)   # every keyword at its default
    gold = FG.case('lowpass_10_fft_0_6')
    for h, g in ((gold.h, gold.g), (gold.h, None), (None, gold.g)):
        want = H.gather_normalize_filter(tiles, idx, mu, std, dev(h), dev(g))
        got = H.gather_normalize_chain(tiles, idx, mu, std, False, dev(h), None, dev(g))
        assert P.same_bits(got, want), P.diff_report(got, want)
    # padded on tiles without a zero: the same bits again
    assert not (tiles == 0).any()
    got = H.gather_normalize_chain(tiles, idx, mu, std, True, dev(gold.h), None, dev(gold.g))
    assert P.same_bits(got, H.gather_normalize_filter(tiles, idx, mu, std, dev(gold.h), dev(gold.g)))
    assert P.same_bits(H.gather_normalize_chain(tiles, idx, mu, std, True), plain)


def test_padded_normalisation_on_the_device(H):
    """Zeros (of either sign) stay zeros, a NaN counts as non-zero, everything else has the bits of the plain expression."""
    rng = np.random.default_rng(7)
    x = rng.standard_normal((3, 2, 2, 224)) * 20 + 1
    x[:, :, :, 150:] = 0.0
    x[0, 0, 0, 10], x[0, 0, 0, 11], x[1, 1, 1, 5] = 0.0, -0.0, np.nan
    mu, std = (1.5, -2.0), (25.0, 19.0)
    idx = dev([2, 0, 1], torch.int64)
    got = H.gather_normalize_chain(dev(x), idx, mu, std, padded=True).cpu().numpy()
    plain = H.gather_normalize(dev(x), idx, mu, std).cpu().numpy()
    xs = x[[2, 0, 1]]
    zero = xs == 0
    assert not got[zero].any() and np.isnan(got[2, 1, 1, 5]) and np.isnan(xs[2, 1, 1, 5])
    assert np.array_equal(got[~zero].view(np.int32), plain[~zero].view(np.int32))
    assert plain[zero].all()                                                   # the unpadded rule moves them to -mu / std
    want = F.normalize_host(xs, mu, std, padded=True).astype(np.float32)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))


@pytest.mark.parametrize('new_len', [1, 100, 224])
def test_r_of_zeros_and_ones_returns_the_leading_samples_bit_for_bit(H, new_len):
    rng = np.random.default_rng(new_len)
    tiles = dev(rng.standard_normal((4, 3, 2, 224)) * 30 + 2)
    idx = dev([1, 3, 1], torch.int64)
    mu, std = (2.05, -0.4), (28.3, 3.5)
    plain = H.gather_normalize(tiles, idx, mu, std)
    got = H.gather_normalize_chain(tiles, idx, mu, std, False, None, rop(H, np.eye(224)[:new_len]), None)
    assert P.same_bits(got[..., :new_len].contiguous(), plain[..., :new_len].contiguous())
    assert not got[..., new_len:].any()
    d = dev(delta(224))
    again = H.gather_normalize_chain(tiles, idx, mu, std, False, d, rop(H, np.eye(224)[:new_len]), d)
    assert P.same_bits(again, got)


# ---- 3. edge shapes ---------------------------------------------------------------------------------------------------------
def _against_host(H, what, tiles, idx, mu, std, padded, h, r, g):
    mu_a, std_a = np.atleast_1d(mu), np.atleast_1d(std)
    xn = F.normalize_host(tiles[idx], mu_a, std_a, padded)
    ref = F.apply_host(xn, h, g, r)
    got = H.gather_normalize_chain(dev(tiles), dev(idx, torch.int64), mu, std, padded, dev(h), rop(H, r), dev(g))
    assert tuple(got.shape) == ref.shape
    G.check(what, got.cpu().numpy(), ref, G.bound(ref, xn, h, r, g))
    return got


def test_three_channels_with_per_channel_factors(H):
    rng = np.random.default_rng(33)
    tiles = rng.standard_normal((4, 2, 3, 224)) * np.array([25.0, 3.0, 0.5]).reshape(1, 1, 3, 1) + 1.5
    tiles[:, :, :, 170:] = 0.0
    mu, std = (1.5, -0.4, 11.0), (25.0, 3.5, 0.75)
    h, g = F.filter_kernels(butter_low=0, butter_high=10, fft_filtering_low=0, fft_filtering_high=6)
    r = F.resample_matrix(224, 89)
    got = _against_host(H, 'C 3, all stages', tiles, [3, 0, 3], mu, std, True, h, r, g)
    assert P.same_bits(got[0], got[2])
    swapped = H.gather_normalize_chain(dev(tiles), dev([3, 0, 3], torch.int64), mu[::-1], std[::-1], True, dev(h), rop(H, r), dev(g))
    assert not P.same_bits(swapped, got)                                       # per-channel factors really are per channel
    _against_host(H, 'C 3, r only', tiles, [1], mu, std, True, None, r, None)


@pytest.mark.parametrize('new_len', [341, 256, 257, 1, 512])
def test_rows_of_512_samples(H, new_len):
    """L = 512 (the C5 tile shape), NB = 2, two channels: more than one output per thread, new_len on both sides of the
    thread count, and the two ends of its range."""
    rng = np.random.default_rng(new_len)
    tiles = rng.standard_normal((4, 2, 2, 512)) * 25 + 1.5
    tiles[:, 1, :, 400:] = 0.0
    mu, std = (1.5, -2.0), (25.0, 19.0)
    h = F.filter_kernels(butter_low=2, butter_high=3, L=512)[0]
    r = F.resample_matrix(512, new_len)
    got = _against_host(H, 'L 512 new_len %d' % new_len, tiles, [1, 3, 1], mu, std, True, h, r, None)
    assert not got[..., new_len:].any()
    _against_host(H, 'L 512 new_len %d, r only' % new_len, tiles, [2], mu, std, False, None, r, None)


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_leave_out_untouched(H):
    from deepards_amd import _lib
    rng = np.random.default_rng(4)
    t224, t512 = dev(rng.standard_normal((3, 2, 1, 224))), dev(rng.standard_normal((3, 2, 1, 512)))
    idx = dev([2, 0], torch.int64)
    k224, k512 = dev(delta(224)), dev(delta(512))
    r224, r512 = rop(H, np.eye(224)[:100]), rop(H, np.eye(512)[:100])
    poisoned = lambda *shape, dtype=torch.float32: P.fill_poison(torch.empty(shape, dtype=dtype, device='cuda'))
    o224, o512 = poisoned(2, 2, 1, 224), poisoned(2, 2, 1, 512)
    C = H.gather_normalize_chain
    calls = [
        ('g on rows of 512 samples', lambda: C(t512, idx, 0.0, 1.0, False, None, None, k512, out=o512)),
        ('g of 224 samples on rows of 512', lambda: C(t512, idx, 0.0, 1.0, False, k512, r512, k224, out=o512)),
        ('h of the wrong length', lambda: C(t224, idx, 0.0, 1.0, True, k512, None, None, out=o224)),
        ('float32 h', lambda: C(t224, idx, 0.0, 1.0, False, k224.float(), None, None, out=o224)),
        ('r for rows of another length', lambda: C(t224, idx, 0.0, 1.0, False, None, r512, None, out=o224)),
        ('r with more outputs than samples', lambda: C(t224, idx, 0.0, 1.0, False, None, rop(H, np.zeros((225, 224))), None, out=o224)),
        ('r without an output', lambda: C(t224, idx, 0.0, 1.0, False, None, rop(H, np.zeros((0, 224))), None, out=o224)),
        ('r in row-major memory', lambda: C(t224, idx, 0.0, 1.0, False, None, dev(np.eye(224)[:100]), None, out=o224)),
        ('float32 r', lambda: C(t224, idx, 0.0, 1.0, False, None, r224.float(), None, out=o224)),
        ('out of the wrong shape', lambda: C(t224, idx, 0.0, 1.0, True, k224, r224, k224, out=o512)),
        ('out with a window too many', lambda: C(t224, idx, 0.0, 1.0, True, None, r224, None, out=poisoned(3, 2, 1, 224))),
        ('one factor for one channel', lambda: C(t224, idx, (0.0, 1.0), (1.0, 2.0), True, None, None, None, out=o224)),
        ('rows of more than 512 samples', lambda: C(dev(np.zeros((3, 2, 1, 513))), idx, 0.0, 1.0, True, out=poisoned(2, 2, 1, 513))),
    ]
    for what, call in calls:
        with pytest.raises(ValueError, match='gather_normalize_chain'):          # ... and names the wrapper that was called
            call()
        assert P.count_poison(o224) == o224.numel() and P.count_poison(o512) == o512.numel(), what
    o64 = poisoned(2, 2, 1, 224, dtype=torch.float64)
    with pytest.raises(ValueError):
        C(t224, idx, 0.0, 1.0, True, out=o64)
    assert P.count_poison(o64) == o64.numel()
    # the entry point itself: an error code before any launch
    entry = _lib.lib().da_gather_normalize_chain
    one = lambda v: (ctypes.c_double * 1)(v)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    table = (  # what, tiles, h, r, new_len, g, out, L, std
        ('new_len 0 with R', t224, None, r224, 0, None, o224, 224, 1.0),
        ('new_len -1 with R', t224, None, r224, -1, None, o224, 224, 1.0),
        ('new_len L + 1', t224, None, r224, 225, None, o224, 224, 1.0),
        ('null R, new_len 100', t224, k224, None, 100, None, o224, 224, 1.0),
        ('null R, new_len -1', t224, None, None, -1, None, o224, 224, 1.0),
        ('L 513', t512, None, None, 0, None, o512, 513, 1.0),
        ('L 513 with R', t512, k512, r512, 100, None, o512, 513, 1.0),
        ('g, L 512', t512, None, None, 0, k512, o512, 512, 1.0),
        ('g, L 512, with R', t512, None, r512, 100, k512, o512, 512, 1.0),
        ('std 0', t224, None, r224, 100, None, o224, 224, 0.0),
    )
    for what, tiles, h, r, new_len, g, out, l, std in table:
        for padded in (0, 1):
            assert entry(p(tiles), p(idx), one(0.0), one(std), padded, p(h), p(r), new_len, p(g), p(out), 2, 2, 1, l, stream) == -1, what
    assert entry(p(t224), p(idx), one(0.0), one(1.0), 1, None, p(r224), 100, None, p(o224), 2, 2, 5, 224, stream) == -1      # C > 4
    assert entry(p(t224), p(idx), one(0.0), one(1.0), 1, None, p(r224), 100, None, None, 2, 2, 1, 224, stream) == -1         # no out
    assert entry(None, p(idx), one(0.0), one(1.0), 1, None, None, 0, None, p(o224), 2, 2, 1, 224, stream) == -1              # no tiles
    assert entry(p(t224), p(idx), one(0.0), one(1.0), 1, None, None, 0, None, p(o224), -1, 2, 1, 224, stream) == -1          # B < 0
    torch.cuda.synchronize()
    assert P.count_poison(o224) == o224.numel() and P.count_poison(o512) == o512.numel()
    assert tuple(C(t224, idx[:0], 0.0, 1.0, True, None, r224, None).shape) == (0, 2, 1, 224)                                # B = 0


# ---- 5. memory discipline ---------------------------------------------------------------------------------------------------
def _rows(n, nb, c, l, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn((n, nb, c, l), generator=g, dtype=torch.float64) * 20 + 1
    t[..., l - l // 4:] = 0.0                                                    # padded tails
    return t.cuda()


def _cases(H):
    zeros = lambda *s: torch.zeros(s, dtype=torch.float32, device='cuda')
    h224, g224 = F.filter_kernels(butter_low=0, butter_high=10, fft_filtering_low=0, fft_filtering_high=6)
    h512 = F.filter_kernels(butter_high=15, L=512)[0]
    r224, r512 = F.resample_matrix(224, 186), F.resample_matrix(512, 257)
    C = H.gather_normalize_chain

    def b_all():
        return dict(tiles=_rows(6, 20, 1, 224, 1), idx=dev([5, 0, 3, 3, 1], torch.int64), h=dev(h224), r=rop(H, r224), g=dev(g224),
                    o1=zeros(5, 20, 1, 224))

    def b_c3():
        return dict(tiles=_rows(4, 3, 3, 512, 2), idx=dev([3, 3, 0], torch.int64), h=dev(h512), r=rop(H, r512), o1=zeros(3, 3, 3, 512))

    def b_r():
        return dict(tiles=_rows(3, 1, 2, 224, 3), idx=dev([1], torch.int64), r=rop(H, r224), o1=zeros(1, 1, 2, 224))

    def b_pad():
        return dict(tiles=_rows(5, 3, 1, 224, 5), idx=dev([4, 2, 2], torch.int64), o1=zeros(3, 3, 1, 224))

    def b_src():
        return dict(tiles=_rows(7, 2, 1, 224, 4), h=dev(h224), r=rop(H, r224), g=dev(g224))
    f3 = ((0.1, 0.2, 0.3), (1.0, 2.0, 3.0))
    return [
        P.OpCase('chain_all_c1', 'chain', b_all,
                 lambda tiles, idx, h, r, g, o1: (C(tiles, idx, 0.25, 1.5, True, h, r, g, out=o1), C(tiles, idx, 0.25, 1.5, True, h, r, g)),
                 dests=('o1',), note='rows are picked through idx: isolation is checked by chain_source_rows'),
        P.OpCase('chain_h_r_l512_c3', 'chain', b_c3,
                 lambda tiles, idx, h, r, o1: (C(tiles, idx, f3[0], f3[1], True, h, r, None, out=o1), C(tiles, idx, f3[0], f3[1], True, h, r)),
                 dests=('o1',)),
        P.OpCase('chain_r_b1_c2', 'chain', b_r,
                 lambda tiles, idx, r, o1: (C(tiles, idx, (0.1, 0.2), (1.0, 2.0), False, None, r, None, out=o1),
                                            C(tiles, idx, (0.1, 0.2), (1.0, 2.0), r=r)), dests=('o1',)),
        P.OpCase('chain_padded_only', 'chain', b_pad,
                 lambda tiles, idx, o1: (C(tiles, idx, 0.25, 1.5, True, out=o1), C(tiles, idx, 0.25, 1.5, True)), dests=('o1',)),
        P.OpCase('chain_source_rows', 'chain', b_src,
                 lambda tiles, h, r, g: C(tiles, torch.arange(7, device='cuda'), 0.25, 1.5, True, h, r, g),
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
    for case in _cases(H)[:4]:
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
            assert P.same_bits(guarded[k].contiguous(), v.contiguous()), '%s: input %s changed' % (case.name, k)


def test_a_nan_tile_that_is_never_picked_stays_out_of_the_result(H):
    c = G.case('highpass_15_down_1p4_fft_0_20')
    h, r, g = stages(c)
    tiles = np.stack([np.full_like(c.x, np.nan), c.x, np.full_like(c.x, np.nan)])
    got = H.gather_normalize_chain(dev(tiles), dev([1, 1], torch.int64), c.mu, c.std, True, dev(h), rop(H, r), dev(g))
    assert torch.isfinite(got).all() and P.same_bits(got[0], got[1])


# ---- 6. repeats -------------------------------------------------------------------------------------------------------------
def test_two_calls_on_equal_inputs_are_bit_equal(H):
    c = G.case('highpass_15_down_1p4_fft_0_20')
    h, r, g = stages(c)
    z = np.load(FIXTURE)
    x = z['x'].copy()
    x[:, :, :, 180:] = 0.0
    idx = dev(np.arange(20)[::-1].copy(), torch.int64)
    first = H.gather_normalize_chain(dev(x), idx, c.mu, c.std, True, dev(h), rop(H, r), dev(g))
    again = H.gather_normalize_chain(dev(x), idx.clone(), c.mu, c.std, True, dev(h), rop(H, r), dev(g))
    assert P.same_bits(first, again), P.diff_report(first, again)


# ---- 7. the store -----------------------------------------------------------------------------------------------------------
def _padded_dataset(tmp_path, case):
    """The fixture as a padded_breath_by_breath dataset file: the golden's padded window in place of its own, every other
    window with a zeroed tail."""
    from deepards_amd.ingest import load_dataset
    ds = load_dataset(FIXTURE)
    ds.windows[:, :, :, 200:] = 0.0
    ds.windows[case.window] = case.x
    ds.dataset_type = 'padded_breath_by_breath'
    path = str(tmp_path / 'padded.npz')
    ds.save_npz(path)
    return path


def test_a_padded_dataset_gives_batches_whose_padding_is_exactly_zero(H, tmp_path):
    """(Before the padded normalisation existed every padding sample came out as -mu / std.)"""
    from deepards_amd.ingest import load_dataset
    c = G.case('only')
    store = load_dataset(_padded_dataset(tmp_path, c)).to_store('cuda')
    assert store.padded is True and (store.mu, store.std) == (c.mu, c.std)
    rel = [c.window, 0, 19]
    x, t = store.batch(rel)
    raw = store.tiles[rel]
    assert (raw == 0).sum() > 1000 and not x[raw == 0].any()
    assert (x[raw != 0] != 0).all()
    G.check('padded store', x[:1].cpu().numpy(), c.expected[None], G.bound(c.expected[None], c.expected[None]))
    want = H.gather_normalize_chain(store.tiles, dev(rel, torch.int64), c.mu, c.std, True)
    assert P.same_bits(x, want) and torch.equal(t, store.targets[rel])
    assert P.same_bits(store.batch_from_device(store.device_indices(rel))[0], want)


def test_store_batches_equal_the_wrapper_bit_for_bit(H):
    from deepards_amd.data import DeviceTileStore
    z = np.load(FIXTURE)
    mu, std = float(z['mu']), float(z['std'])
    x = z['x'].copy()
    x[:, :, :, 190:] = 0.0
    store = DeviceTileStore(x, z['target'], mu, std)
    rel = [7, 0, 19, 7]
    plain = H.gather_normalize(store.tiles, dev(rel, torch.int64), mu, std)
    assert store.padded is False and store.filter_r is None
    assert P.same_bits(store.batch(rel)[0], plain)                              # a constructed store: today's output
    d = store.device_indices(rel)
    keys = dict(butter_low=0, butter_high=10, fft_filtering_low=0, fft_filtering_high=6)
    h, g = F.filter_kernels(L=224, **keys)
    r = F.resample_matrix(224, 160)
    for padded in (False, True):
        store.padded = padded
        for kw, hh, rr, gg in ((dict(keys, post_hoc_downsampling=1.4), h, r, g), (dict(post_hoc_downsampling=1.4), None, r, None),
                               (keys, h, None, g), ({}, None, None, None)):
            store.set_filters(**kw)
            if padded or rr is not None:
                want = H.gather_normalize_chain(store.tiles, dev(rel, torch.int64), mu, std, padded, dev(hh), rop(H, rr), dev(gg))
            elif hh is not None:
                want = H.gather_normalize_filter(store.tiles, dev(rel, torch.int64), mu, std, dev(hh), dev(gg))
            else:
                want = plain
            x_, t = store.batch(rel)
            assert P.same_bits(x_, want) and torch.equal(t, store.targets[rel]), (padded, kw)
            x_, t = store.batch_from_device(d)
            assert P.same_bits(x_, want) and torch.equal(t, store.targets[rel]), (padded, kw)
            ox, ot = P.fill_poison(torch.empty_like(want)), torch.empty((4, 2), device='cuda')
            x_, t = store.batch(rel, out=(ox, ot))                              # out= buffers keep working
            assert x_ is ox and t is ot and P.same_bits(ox, want)
            x_, t = store.batch_from_device(d[1:3], out=(ox[:2], ot[:2]))
            assert P.same_bits(x_, want[1:3])
        assert not P.same_bits(store.batch(rel)[0], plain) or not padded       # padded, no stage: zeros instead of -mu / std
    # the k-fold test store inherits both
    store.set_filters(post_hoc_downsampling=1.4)
    store.enable_kfolds(np.arange(20) // 2, 2)
    test = store.make_test_store_if_kfold()
    assert test.padded is True and test.filter_r is store.filter_r
    test.set_kfold_indexes_for_fold(0)
    absolute = test.kfold_indexes[:3]
    want = H.gather_normalize_chain(store.tiles, absolute.contiguous(), test.mu, test.std, True, None, rop(H, r), None)
    assert P.same_bits(test.batch([0, 1, 2])[0], want)


# ---- 8. the driver ----------------------------------------------------------------------------------------------------------
def test_post_hoc_downsampling_from_an_experiment_file_reaches_the_batches(H, tmp_path):
    """``post_hoc_downsampling: 2.0`` in the -co file, a padded dataset file: samples 112..223 of every row are 0.0 and the
    first 112 are the golden's."""
    from deepards_amd import train_ards_detector as T
    from deepards_amd.config import Configuration
    c = G.case('down_2')
    path = _padded_dataset(tmp_path, c)
    over = tmp_path / 'downsamp.yml'
    over.write_text('dataset_type: padded_breath_by_breath\npost_hoc_downsampling: 2.0\n')
    args = Configuration(T.build_parser().parse_args(['-co', str(over), '--train-from-pickle', path, '--test-from-pickle', path]),
                         T.BUILD_DEFAULTS)
    obj = object.__new__(T.CNNLinearModel)
    obj.args, obj.device = args, torch.device('cuda')
    r = F.resample_matrix(224, 112)
    for store in obj.get_base_datasets():
        assert store.padded is True and store.post_hoc_downsampling == 2.0
        x, _ = store.batch([c.window, 3])
        assert tuple(x.shape) == (2, 20, 1, 224) and not x[..., 112:].any() and x[..., :112].any()
        ref = c.expected[None]
        G.check('experiment file, 2.0x', x[:1].cpu().numpy(), ref, G.bound(ref, F.normalize_host(c.x, c.mu, c.std, True)[None], None, r, None))


def test_driver_trains_and_tests_on_padded_downsampled_batches(H, tmp_path):
    """One train and one test epoch of CNNLinearModel on a padded dataset file with the Butterworth filter and 4x
    downsampling, B = 2, resnet18: finite losses, and the first batch the model receives is the wrapper's output (and the
    golden's item).  Both stores are narrowed to the golden's window so that the first batch is known whatever the shuffle
    does."""
    from deepards_amd import train_ards_detector as T
    c = G.case('lowpass_10_down_4')
    path = _padded_dataset(tmp_path, c)
    h, r, g = stages(c)
    args = T.make_args(base_network='resnet18', epochs=1, batch_size=2, seed=3, train_from_pickle=path, test_from_pickle=path,
                       dataset_type='padded_breath_by_breath', post_hoc_downsampling=c.factor, **c.keys)
    cls = T.CNNLinearModel(args)
    made, seen = cls.get_base_datasets, []

    def narrowed():
        train, test = made()
        for store in (train, test):
            assert store.padded is True and store.filter_r is not None
            store.set_kfold_indexes([c.window] * 6)
        gather = train.batch_from_device

        def recording(abs_idx, out=None):
            x, t = gather(abs_idx, out=out)
            seen.append((abs_idx.clone(), x.clone(), train.tiles))
            return x, t
        train.batch_from_device = recording
        return train, test
    cls.get_base_datasets = narrowed
    res = cls.train_and_test()
    losses = res.get_meter('loss', 0)
    print('train losses %s' % losses)
    assert len(losses) == 3 and np.isfinite(losses).all() and len(seen) == 3
    assert res.patient_results[(0, 1)]['votes'].sum() == 6                      # the test epoch ran on its 6 windows
    abs_idx, x, tiles = seen[0]
    assert abs_idx.tolist() == [c.window, c.window] and tuple(x.shape) == (2, 20, 1, 224)
    want = H.gather_normalize_chain(tiles, abs_idx, c.mu, c.std, True, dev(h), rop(H, r), None)
    assert P.same_bits(x, want) and not x[..., c.new_len:].any()
    ref = np.stack([c.expected] * 2)
    xn = np.stack([F.normalize_host(c.x, c.mu, c.std, True)] * 2)
    G.check('first batch', x.cpu().numpy(), ref, G.bound(ref, xn, h, r, None))
