"""Host-side tests of the DTW feature (no GPU): the numpy oracle against itself and against the properties the definition
implies, the shape / plan twins against the built library, the pair lists of find_patient_similarity against a restatement of
dtw_lib.py:185-249, the segments of dtw_analyze, and every refusal with its reason."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'tools'))

import dtw_ref as R                                                       # noqa: E402
from deepards_amd import _lib, dtw as D, dtw_ops as O, ingest             # noqa: E402
from deepards_amd import train_ards_detector as T                         # noqa: E402

NEW_SYMBOLS = ('da_dtw_max_len', 'da_dtw_shape_ok', 'da_dtw_plan', 'da_dtw_pairs', 'da_dtw_segment_mean')
ORACLE_SHAPES = [(1, 1), (1, 7), (5, 1), (63, 64), (65, 257), (224, 224)]
DTYPES = (np.float32, np.float64)


def _bits(v):
    return np.asarray(v).tobytes()


def _seqs(n, m, seed=0, scale=30.0):
    rng = np.random.RandomState(seed + 1000 * n + m)
    return rng.randn(n) * scale, rng.randn(m) * scale


# ---- the oracle -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,m', ORACLE_SHAPES)
def test_the_two_cell_orders_agree_bit_for_bit(n, m):
    x, y = _seqs(n, m)
    for dt in DTYPES:
        for metric in ('euclidean', 'sqeuclidean'):
            for band in (None, 0, 2, abs(n - m), max(n, m)):
                a, b = R.dtw_rows(x, y, dt, metric, band), R.dtw_diagonals(x, y, dt, metric, band)
                assert a.dtype == np.dtype(dt) and b.dtype == np.dtype(dt)
                assert _bits(a) == _bits(b), (n, m, dt, metric, band, a, b)


@pytest.mark.parametrize('dt', DTYPES)
def test_oracle_properties(dt):
    for n, m in [(1, 1), (3, 9), (40, 37), (64, 65)]:
        x, y = _seqs(n, m, seed=3)
        for metric in ('euclidean', 'sqeuclidean'):
            d = R.dtw(x, y, dt, metric)
            assert np.isfinite(d) and d >= 0
            assert _bits(d) == _bits(R.dtw(y, x, dt, metric))                           # symmetry
            same = R.dtw(x, x, dt, metric)
            assert same == 0 and not np.signbit(same)                                   # dtw(x, x) is +0
            assert _bits(R.dtw(x, y, dt, metric, band=max(n, m))) == _bits(d)           # a band that holds every cell
            assert _bits(R.dtw(x, y, dt, metric, band=max(n, m) + 5)) == _bits(d)
            if n != m:
                assert R.dtw(x, y, dt, metric, band=abs(n - m) - 1) == np.inf           # the corner is outside the band
                assert np.isfinite(R.dtw(x, y, dt, metric, band=abs(n - m)))
        # k = 0 on equal lengths: the left-to-right sum of c(i, i)
        x, y = _seqs(50, 50, seed=4)
        xs, ys = np.asarray(x, dt), np.asarray(y, dt)
        for metric in ('euclidean', 'sqeuclidean'):
            s = None
            for i in range(50):
                d = xs[i] - ys[i]
                c = abs(d) if metric == 'euclidean' else d * d
                s = c if s is None else s + c
            assert _bits(R.dtw(x, y, dt, metric, band=0)) == _bits(dt(s))


def test_float32_oracle_is_within_the_derived_bound_of_float64():
    for n, m in [(63, 64), (224, 224), (224, 129)]:
        x, y = _seqs(n, m, seed=5)
        x, y = x.astype(np.float32), y.astype(np.float32)
        lo, hi = float(R.dtw(x, y, np.float32)), float(R.dtw(x, y, np.float64))
        assert abs(lo - hi) <= (n + m + 1) * 2.0 ** -24 * 1.01 * hi


def test_ordered_mean():
    assert np.isnan(R.ordered_mean([]))
    v = [0.1, 0.2, 0.3]
    assert R.ordered_mean(v) == ((0.0 + 0.1) + 0.2 + 0.3) / 3.0


# ---- ABI and twins ----------------------------------------------------------------------------------------------------------
def test_header_declares_and_binds_the_new_symbols():
    declared = set(_lib.header_symbols())
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES
    assert set(_lib.SIGNATURES) == declared
    assert 'dtw.hip' in _lib.SOURCES and os.path.exists(os.path.join(_lib.CSRC, 'dtw.hip'))
    assert D.dtw_shape_ok is O.dtw_shape_ok and D.dtw_plan is O.dtw_plan


LENGTHS = [-1, 0, 1, 2, 63, 64, 65, 128, 129, 224, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 3072, 3073, 4256, 4480, 4607, 4608,
           4609, 10000]


def test_shape_and_plan_twins_match_the_library():
    lib = _lib.lib()
    assert lib.da_dtw_max_len() == O.MAX_LEN == D.MAX_LEN == 4608
    refused = planned = 0
    for n in LENGTHS:
        for m in LENGTHS:
            for acc in ('f32', 'f64'):
                for a64, b64 in ((0, 0), (1, 0), (0, 1), (1, 1)):
                    ok = O.dtw_shape_ok(n, m, acc, bool(a64), bool(b64))
                    assert bool(lib.da_dtw_shape_ok(n, m, O.ACC[acc], a64, b64)) == ok, (n, m, acc, a64, b64)
                    assert (O.dtw_refusal(n, m, acc, bool(a64), bool(b64)) is None) == ok
                    if not ok:
                        refused += 1
                        # a refused shape answers before any launch: null pointers, no device touched
                        assert lib.da_dtw_pairs(None, a64, max(n, 1), 1, n, None, b64, max(m, 1), 1, m, None, None, 1, O.ACC[acc],
                                                0, -1, None, None) == -1
                for p in (0, 1, 3, 4, 5, 1000):
                    got = O.dtw_plan_lib(n, m, p, acc)
                    if O.dtw_shape_ok(n, m, acc) and p >= 1:
                        assert got == O.dtw_plan(n, m, p, acc), (n, m, p, acc)
                        planned += 1
                        w = got['cols_per_lane']
                        assert w in O.CLASSES and 64 * w >= m and got['lanes'] == -(-m // w) <= 64
                        assert got['steps'] == n + got['lanes'] - 1 and got['grid'] * got['waves_per_block'] >= p
                        assert got['block'] == 64 * got['waves_per_block'] and got['lds'] == 0
                    else:
                        assert got is None
                        with pytest.raises(ValueError):
                            O.dtw_plan(n, m, p, acc)
    assert refused and planned
    assert lib.da_dtw_shape_ok(4, 4, 2, 0, 0) == 0 and lib.da_dtw_shape_ok(4, 4, -1, 0, 0) == 0
    out = (ctypes.c_int * 7)()
    assert lib.da_dtw_plan(4, 4, 1, 2, out) == -1


def test_class_edges_follow_the_plan():
    for last, first in O.class_edges():
        assert O.dtw_shape_ok(3, last)
        w = O.dtw_plan(3, last, 1)['cols_per_lane']
        assert last == 64 * w
        if first <= O.MAX_LEN:
            assert O.dtw_plan(3, first, 1)['cols_per_lane'] > w
        else:
            assert not O.dtw_shape_ok(3, first)


# ---- pair lists of find_patient_similarity ----------------------------------------------------------------------------------
def _toy_patients():
    # windows interleaved across patients, with patients of 1, 3, 7 and 60 windows; absolute indices with gaps, as a fold has
    rng = np.random.RandomState(7)
    pat = np.array(['d'] * 60 + ['a'] * 1 + ['c'] * 7 + ['b'] * 3)
    rng.shuffle(pat)
    idx = np.sort(rng.choice(500, len(pat), replace=False))
    return pat, idx


@pytest.mark.parametrize('method', ['random', 'same_ordered'])
@pytest.mark.parametrize('n', [50, 5, 2])
def test_pair_lists_equal_the_restated_reference(method, n):
    pat, idx = _toy_patients()
    pts_ref, pairs_ref = R.reference_pairs(pat, idx, method, np.random.RandomState(11), n=n)
    pts, ia, ib, offsets, segments = D.similarity_pairs(pat, idx, method, n=n, rng=np.random.RandomState(11))
    assert pts == pts_ref and len(segments) == len(pts) * (len(pts) - 1) // 2 == len(pairs_ref)
    assert offsets[0] == 0 and offsets[-1] == len(ia) == len(ib) and (np.diff(offsets) >= 1).all()
    for s, (i, j) in enumerate(segments):
        assert i < j
        got = list(zip(ia[offsets[s]:offsets[s + 1]].tolist(), ib[offsets[s]:offsets[s + 1]].tolist()))
        assert got == [(int(p), int(q)) for p, q in pairs_ref[(pts[i], pts[j])]], (pts[i], pts[j])
    counts = {p: int((pat == p).sum()) for p in pts}
    for s, (i, j) in enumerate(segments):
        k = offsets[s + 1] - offsets[s]
        lim = min(counts[pts[i]], counts[pts[j]])
        assert k == (min(lim, n) if method == 'random' else lim)
    # every pair joins a window of the first patient to one of the second
    where = dict(zip(idx.tolist(), pat.tolist()))
    for s, (i, j) in enumerate(segments):
        for p, q in zip(ia[offsets[s]:offsets[s + 1]].tolist(), ib[offsets[s]:offsets[s + 1]].tolist()):
            assert where[p] == pts[i] and where[q] == pts[j]


def test_pair_lists_of_one_patient_and_bad_method():
    pts, ia, ib, offsets, segments = D.similarity_pairs(np.zeros(4, dtype=np.int64), np.arange(4), 'random', rng=np.random.RandomState(0))
    assert pts == [0] and len(ia) == 0 and segments == [] and offsets.tolist() == [0]
    with pytest.raises(ValueError, match='random'):
        D.similarity_pairs([0, 1], [0, 1], 'nearest')


# ---- segments of dtw_analyze ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nb', [1, 3])
def test_analyze_segments(nb):
    t = 12
    ia, ib, offsets = D.analyze_index_arrays(t, nb, device='cpu')
    assert ia.dtype == ib.dtype == offsets.dtype == torch.int32
    assert offsets.tolist() == [nb * g for g in range(t - nb + 1)]
    want = [(cur - j, cur) for cur in range(nb, t) for j in range(nb, 0, -1)]           # oldest breath first
    assert list(zip(ia.tolist(), ib.tolist())) == want
    assert D.analyze_index_arrays(nb, nb, device='cpu') is None and D.analyze_index_arrays(1, nb, device='cpu') is None
    with pytest.raises(ValueError, match='n_breaths'):
        D.analyze_index_arrays(5, 0, device='cpu')


def test_rolling_average_is_the_references_convolution():
    s = np.array([np.nan, np.nan, np.nan, 1.0, 2.0, 4.0, 8.0])
    assert _bits(D.rolling_average(s, 1)) == _bits(np.append([], np.convolve(s, np.ones(1), mode='valid')))
    got = D.rolling_average(s, 2)
    want = np.append([np.nan], np.convolve(s, np.ones((2,)) / 2, mode='valid'))
    assert len(got) == len(s) and _bits(got) == _bits(want)


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_carry_their_reason():
    x = np.zeros(8)
    with pytest.raises(ValueError, match='CPU tensor'):
        D.dtw(torch.zeros(8), x)
    with pytest.raises(ValueError, match='CPU tensor'):
        D.dtw_pairs(torch.zeros(2, 8), [0], [1])
    with pytest.raises(ValueError, match='CPU tensor'):
        D.dtw_analyze(torch.zeros(4, 8))
    with pytest.raises(ValueError, match='4608'):
        D.dtw(np.zeros(4609), x)
    with pytest.raises(ValueError, match='4608'):
        D.dtw(x, np.zeros(4609))
    with pytest.raises(ValueError, match='at least one sample'):
        D.dtw(np.zeros(0), x)
    with pytest.raises(ValueError, match="acc='f32'"):
        D.dtw(x, x.astype(np.float32), acc='f32')
    with pytest.raises(ValueError, match='acc must be'):
        D.dtw(x, x, acc='f16')
    with pytest.raises(ValueError, match='metric'):
        D.dtw(x, x, metric='cosine')
    with pytest.raises(ValueError, match='1-D'):
        D.dtw(np.zeros((2, 8)), x)
    with pytest.raises(ValueError, match='channels'):
        D.dtw_analyze(np.zeros((3, 4, 2, 8)))
    assert '4608' in O.dtw_refusal(5000, 8) and 'float32 tables only' in O.dtw_refusal(8, 8, 'f32', True, False)
    assert O.dtw_refusal(4608, 1) is None and O.dtw_refusal(8, 8, 'f64', True, False) is None


def _toy_dataset(chans=1, nb=2, l=8, n=6):
    rng = np.random.RandomState(2)
    x = rng.randn(n, nb, chans, l)
    tgt = np.eye(2, dtype=np.float32)[rng.randint(0, 2, n)]
    return ingest.IngestedDataset(x, tgt, np.array(['p%d' % (i % 3) for i in range(n)]), np.zeros((n, nb)),
                                  {None: (np.zeros(chans), np.ones(chans))}, nb, 'unpadded_centered_sequences')


def test_similarity_refusals_come_before_any_upload():
    with pytest.raises(ValueError, match='channels'):
        D.find_patient_similarity(_toy_dataset(chans=2))
    with pytest.raises(ValueError, match='4608'):
        D.find_patient_similarity(_toy_dataset(nb=20, l=231, n=3))
    with pytest.raises(ValueError, match="acc='f32'"):
        D.find_patient_similarity(_toy_dataset(), acc='f32')
    with pytest.raises(ValueError, match='random'):
        D.find_patient_similarity(_toy_dataset(), dist_method='nearest')
    with pytest.raises(ValueError, match='expected'):
        D.find_patient_similarity(np.zeros((3, 2, 1, 8)))


def test_the_training_parser_still_refuses_the_dtw_flags():
    for flag in ('--perform-dtw-preprocessing', '--plot-dtw-with-disease'):
        with pytest.raises(SystemExit, match='outside the accelerated'):
            T.main([flag, '1'])
    args = D.build_parser().parse_args(['similarity', '-p', 'a.npz', '-o', 'b.pkl', '--seed', '3'])
    assert args.command == 'similarity' and args.dist_method == 'random' and args.n == 50 and args.seed == 3
    args = D.build_parser().parse_args(['analyze', '-p', 'a.npz', '-o', 'b.npz', '--patient', '2'])
    assert args.n_breaths == 3 and args.rolling_av_len == 1 and args.patient == '2'
