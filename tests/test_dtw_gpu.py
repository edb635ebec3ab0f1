"""GPU tests of the DTW kernels and of the dtw_lib surface on them.  The distance is defined bit for bit (one IEEE operation per
step of the recurrence), so every comparison with the numpy oracle (tests/tools/dtw_ref.py) is for EQUALITY, through the raw
bytes.  Shapes sit at the edges the launch plan reports (``dtw_plan``): lane counts around 64, every columns-per-lane class
boundary, pair counts around the pairs per block."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'tools'))

import dtw_ref as R                                                       # noqa: E402
from tools import poison as P                                             # noqa: E402

pytestmark = pytest.mark.gpu

NP = {'f32': np.float32, 'f64': np.float64}
TT = {'f32': torch.float32, 'f64': torch.float64}
N_SET = (1, 2, 63, 64, 65, 224)
M_SET = (1, 2, 63, 64, 65, 127, 128, 129, 224, 255, 256, 257)
# (accumulation, type of table a, type of table b)
TYPE_CASES = [('f32', 'f32', 'f32'), ('f64', 'f32', 'f32'), ('f64', 'f64', 'f64'), ('f64', 'f32', 'f64')]


@pytest.fixture(scope='module')
def D():
    from deepards_amd import dtw
    return dtw


@pytest.fixture(scope='module')
def O():
    from deepards_amd import dtw_ops
    return dtw_ops


def cuda(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def bits(v):
    return np.asarray(v).tobytes()


_DATA = {}


def seq(length, which, kind='f32', scale=30.0):
    """A seeded sequence, the same for every test that asks: float32-representable values (kind 'f32': what a float32 table and
    its float64 widening hold) or full doubles (kind 'f64')."""
    key = (length, which, kind, scale)
    if key not in _DATA:
        v = np.random.RandomState(977 * length + 31 * which + 5).randn(length) * scale
        _DATA[key] = v.astype(np.float32).astype(np.float64) if kind == 'f32' else v
    return _DATA[key]


_ORACLE = {}


def oracle(x, y, acc, metric='euclidean', band=None):
    """The oracle's value for one pair, computed once per distinct request and shared between the tests."""
    key = (bits(x), bits(y), acc, metric, band)
    if key not in _ORACLE:
        _ORACLE[key] = R.dtw(x, y, NP[acc], metric, band)
    return _ORACLE[key]


def run_pair(D, x, y, acc, ta='f32', tb='f32', metric='euclidean', band=None):
    out = D.dtw_pairs(cuda(x.astype(NP[ta]))[None, :], [0], [0], cuda(y.astype(NP[tb]))[None, :], metric=metric, band=band, acc=acc)
    assert out.dtype == TT[acc] and tuple(out.shape) == (1,)
    return out.cpu().numpy()[0]


# ---- bit equality with the oracle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('metric', ['euclidean', 'sqeuclidean'])
@pytest.mark.parametrize('acc,ta,tb', TYPE_CASES)
def test_grid_of_small_shapes_equals_the_oracle(D, acc, ta, tb, metric):
    bad = []
    for n in N_SET:                                             # n < m, n == m and n > m all occur
        for m in M_SET:
            x, y = seq(n, 0, ta), seq(m, 1, tb)
            got, want = run_pair(D, x, y, acc, ta, tb, metric), oracle(x, y, acc, metric)
            if bits(got) != bits(want):
                bad.append((n, m, got, want))
    assert not bad, bad[:8]


def class_edge_lengths(O):
    """m at and one past every change of the columns per lane that dtw_plan reports, and the longest row."""
    edges, prev = [], O.dtw_plan(3, 1, 1)['cols_per_lane']
    for m in range(2, O.MAX_LEN + 1):
        w = O.dtw_plan(3, m, 1)['cols_per_lane']
        if w != prev:
            edges += [m - 1, m]
            prev = w
    return edges + [O.MAX_LEN]


@pytest.mark.parametrize('metric', ['euclidean', 'sqeuclidean'])
@pytest.mark.parametrize('acc,ta,tb', TYPE_CASES)
def test_every_columns_per_lane_class_boundary(D, O, acc, ta, tb, metric):
    edges = class_edge_lengths(O)
    assert len(edges) == 2 * (len(O.CLASSES) - 1) + 1 and edges[-1] == 4608
    bad = []
    for m in edges:
        x, y = seq(3, 2, ta), seq(m, 3, tb)
        got, want = run_pair(D, x, y, acc, ta, tb, metric), oracle(x, y, acc, metric)
        if bits(got) != bits(want):
            bad.append((m, got, want))
    # the long side as x: n > m, 64 lanes' worth of rows and more through a one-lane strip
    for n in (edges[3], edges[-1]):
        x, y = seq(n, 3, ta), seq(3, 2, tb)
        got, want = run_pair(D, x, y, acc, ta, tb, metric), oracle(x, y, acc, metric)
        if bits(got) != bits(want):
            bad.append((n, 'as x', got, want))
    assert not bad, bad


@pytest.mark.parametrize('n,m', [(4480, 4480), (4480, 4256)])
def test_full_windows(D, n, m):
    """One pair of flattened windows (20 x 224 samples): bit equal in both accumulation types, and float32 within
    (n + m + 1) 2^-24 1.01 relative of float64 -- at most n + m - 1 cells on the path, one rounding for the cost and one for the
    add per cell, and min is monotone.  (Measured on the CPU oracle: 18.6 2^-24 at 4480 x 4480.)"""
    x, y = seq(n, 4, scale=25.0), seq(m, 5, scale=25.0)
    lo, hi = run_pair(D, x, y, 'f32'), run_pair(D, x, y, 'f64')
    print('dtw(%d, %d): f32 %r f64 %r, relative difference %.2f x 2^-24' % (n, m, lo, hi, abs(float(lo) - hi) / hi * 2.0 ** 24))
    assert bits(lo) == bits(oracle(x, y, 'f32')) and bits(hi) == bits(oracle(x, y, 'f64'))
    assert abs(float(lo) - float(hi)) <= (n + m + 1) * 2.0 ** -24 * 1.01 * float(hi)


@pytest.mark.parametrize('acc', ['f32', 'f64'])
@pytest.mark.parametrize('n,m', [(40, 37), (224, 224), (37, 40)])
def test_band(D, acc, n, m):
    x, y = seq(n, 6), seq(m, 7)
    free = run_pair(D, x, y, acc)
    for metric in ('euclidean', 'sqeuclidean'):
        for k in sorted(set(k for k in (0, 1, abs(n - m) - 1, abs(n - m), max(n, m)) if k >= 0)):
            got = run_pair(D, x, y, acc, metric=metric, band=k)
            assert bits(got) == bits(oracle(x, y, acc, metric, k)), (metric, k, got)
            if k < abs(n - m):
                assert got == np.inf
    assert bits(run_pair(D, x, y, acc, band=max(n, m))) == bits(free) == bits(run_pair(D, x, y, acc, band=4000))
    if n == m:                                                  # k = 0: the left-to-right sum of the diagonal's costs
        xs, ys = x.astype(NP[acc]), y.astype(NP[acc])
        s = NP[acc](0)
        for i in range(n):
            s = s + abs(xs[i] - ys[i])
        assert bits(run_pair(D, x, y, acc, band=0)) == bits(NP[acc](s))


@pytest.mark.parametrize('acc', ['f32', 'f64'])
def test_hard_inputs(D, acc):
    rng = np.random.RandomState(12)
    n, m = 224, 193
    flow = lambda k: (np.clip(rng.randn(k) * 60, -100, 100)).astype(np.float32).astype(np.float64)   # raw-flow magnitudes
    cases = {
        'raw flow': (flow(n), flow(m)),
        'constant rows (every min a tie)': (np.full(n, 3.5), np.full(m, -1.25)),
        'equal constants': (np.full(n, 7.0), np.full(m, 7.0)),
        'all-zero rows (padded breaths)': (np.zeros(n), np.zeros(m)),
        'zero against flow': (np.zeros(n), flow(m)),
        'equal up to a shift': (np.roll(flow(224), 9), None),
        'large accumulations': (flow(n) * 1000, flow(m) * 1000),
    }
    # (every operand a float32 value: the tables are float32, the oracle takes the same numbers)
    cases = {k: tuple(None if v is None else v.astype(np.float32).astype(np.float64) for v in xy) for k, xy in cases.items()}
    shifted = cases['equal up to a shift'][0]
    cases['equal up to a shift'] = (shifted, np.roll(shifted, -9))
    for name, (x, y) in cases.items():
        for metric in ('euclidean', 'sqeuclidean'):
            got = run_pair(D, x, y, acc, metric=metric)
            assert bits(got) == bits(oracle(x, y, acc, metric)), (name, metric, got)
    assert run_pair(D, np.zeros(n), np.zeros(m), acc) == 0 and run_pair(D, np.full(n, 7.0), np.full(m, 7.0), acc) == 0
    x = flow(n)
    same = run_pair(D, x, x, acc)
    assert same == 0 and not np.signbit(same)
    assert float(run_pair(D, cases['large accumulations'][0], cases['large accumulations'][1], 'f32')) > 1e5


# ---- batches ----------------------------------------------------------------------------------------------------------------
def test_batches_do_not_depend_on_size_or_position(D, O):
    rows, n, m = 6, 65, 129
    a = np.stack([seq(n, 20 + r) for r in range(rows)]).astype(np.float32)
    b = np.stack([seq(m, 40 + r) for r in range(rows)]).astype(np.float32)
    ta, tb = cuda(a), cuda(b)
    wpb = O.dtw_plan(n, m, 1)['waves_per_block']
    for acc in ('f32', 'f64'):
        alone = {}
        for i in range(rows):
            for j in range(rows):
                alone[(i, j)] = D.dtw_pairs(ta, [i], [j], tb, acc=acc).cpu().numpy()[0]
                assert bits(alone[(i, j)]) == bits(oracle(a[i].astype(np.float64), b[j].astype(np.float64), acc))
        rng = np.random.RandomState(3)
        for p in (1, wpb - 1, wpb, wpb + 1, 1000):
            ia, ib = rng.randint(0, rows, p), rng.randint(0, rows, p)
            ia[p // 2], ib[p // 2] = ia[0], ib[0]                                        # a repeated pair
            got = D.dtw_pairs(ta, ia, ib, tb, acc=acc).cpu().numpy()
            want = np.array([alone[(i, j)] for i, j in zip(ia.tolist(), ib.tolist())])
            assert bits(got) == bits(want), (acc, p)
            back = D.dtw_pairs(ta, ia[::-1].copy(), ib[::-1].copy(), tb, acc=acc).cpu().numpy()   # every pair at another position
            assert bits(back[::-1].copy()) == bits(want)
            swapped = D.dtw_pairs(tb, ib, ia, ta, acc=acc).cpu().numpy()                 # dtw(y, x) through the kernel
            assert bits(swapped) == bits(want), (acc, p)
            dev_idx = D.dtw_pairs(ta, cuda(ia.astype(np.int64)), cuda(ib.astype(np.int32)), tb, acc=acc).cpu().numpy()
            assert bits(dev_idx) == bits(want)
        # one table against itself, with ia == ib entries: exactly +0 there
        ia, ib = np.array([0, 1, 2, 2, 5, 3, 0]), np.array([0, 4, 2, 1, 5, 3, 1])
        got = D.dtw_pairs(ta, ia, ib, acc=acc).cpu().numpy()
        for q, (i, j) in enumerate(zip(ia.tolist(), ib.tolist())):
            if i == j:
                assert got[q] == 0 and not np.signbit(got[q])
            else:
                assert bits(got[q]) == bits(oracle(a[i].astype(np.float64), a[j].astype(np.float64), acc))
        assert bits(got[3]) == bits(D.dtw_pairs(ta, [1], [2], acc=acc).cpu().numpy()[0])


# ---- memory discipline ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('acc,tt', [('f32', 'f32'), ('f64', 'f32'), ('f64', 'f64')])
def test_memory_discipline(D, acc, tt):
    rows, n, m = 5, 65, 130
    a = np.stack([seq(n, 60 + r, tt) for r in range(rows)])
    b = np.stack([seq(m, 70 + r, tt) for r in range(rows)])
    ia, ib = np.array([0, 2, 4, 2, 0]), np.array([1, 1, 4, 0, 1])                        # rows 1, 3 of a and 2, 3 of b: unselected
    clean = D.dtw_pairs(cuda(a.astype(NP[tt])), ia, ib, cuda(b.astype(NP[tt])), acc=acc)
    assert not torch.isnan(clean).any()

    def in_slack(t, lead, trail):                                # the table as a column slice of a wider, pattern-filled buffer
        buf = P.fill_poison(torch.empty((t.shape[0] + 2, lead + t.shape[1] + trail), dtype=t.dtype, device='cuda'))
        view = buf[1:-1, lead:lead + t.shape[1]]
        view.copy_(t)
        return view

    wa, wb = in_slack(cuda(a.astype(NP[tt])), 3, 11), in_slack(cuda(b.astype(NP[tt])), 2, 1)
    for t, used in ((wa, set(ia.tolist())), (wb, set(ib.tolist()))):
        for r in range(rows):
            if r not in used:
                t[r] = float('nan')                                                      # unselected rows poisoned
    out, guard = P.guarded(torch.zeros_like(clean), name='out')
    P.fill_poison(out)                                                                   # a dirty destination
    with P.poisoned_allocations():
        got = D.dtw_pairs(wa, ia, ib, wb, acc=acc, out=out)
        torch.cuda.synchronize()
    assert got is out and P.same_bits(out, clean), P.diff_report(out, clean)
    P.assert_guards_intact(guard)
    # an index outside its table, in a device tensor (not read back): NaN for that pair alone, nothing read
    bad_a = cuda(np.array([0, rows, 4, -1, 0], dtype=np.int32))
    got = D.dtw_pairs(wa, bad_a, cuda(ib.astype(np.int32)), wb, acc=acc).cpu().numpy()
    c = clean.cpu().numpy()
    assert np.isnan(got[1]) and np.isnan(got[3]) and bits(got[[0, 2, 4]]) == bits(c[[0, 2, 4]])
    with pytest.raises(IndexError):
        D.dtw_pairs(wa, [0, rows], [0, 0], wb, acc=acc)                                  # a host list is checked on the host
    with pytest.raises(ValueError, match='out must be'):
        D.dtw_pairs(wa, ia, ib, wb, acc=acc, out=torch.zeros(4, device='cuda', dtype=TT[acc]))
    with pytest.raises(ValueError, match='pitch'):
        D.dtw_pairs(wa.t(), [0], [0], acc=acc)
    if tt == 'f64':
        with pytest.raises(ValueError, match="acc='f32'"):
            D.dtw_pairs(wa, ia, ib, wb, acc='f32')


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_segment_mean(D, dt):
    rng = np.random.RandomState(5)
    lens = [1, 3, 50, 0, 2, 0]
    d = (rng.rand(sum(lens)) * 1e4).astype(NP[dt])
    offsets = np.concatenate([[0], np.cumsum(lens)])
    want = np.array([R.ordered_mean(d[offsets[g]:offsets[g + 1]]) for g in range(len(lens))])
    assert np.isnan(want[3]) and np.isnan(want[5])
    out, guard = P.guarded(torch.zeros(len(lens), dtype=torch.float64, device='cuda'), name='means')
    P.fill_poison(out)
    got = D.segment_mean(cuda(d), offsets, out=out)
    assert got is out and bits(out.cpu().numpy()) == bits(want)
    P.assert_guards_intact(guard)
    again = D.segment_mean(cuda(d), cuda(offsets.astype(np.int32))).cpu().numpy()
    assert bits(again) == bits(want)
    # offsets that leave the distances: NaN for that segment, nothing read (device offsets are not read back)
    wild = cuda(np.array([0, 1, len(d) + 5], dtype=np.int32))
    got = D.segment_mean(cuda(d), wild).cpu().numpy()
    assert bits(got[0]) == bits(want[0]) and np.isnan(got[1])
    with pytest.raises(IndexError):
        D.segment_mean(cuda(d), [0, len(d) + 1])


# ---- dtw_analyze ------------------------------------------------------------------------------------------------------------
def _analyze_store(padded=False, filters=None):
    from deepards_amd.data import DeviceTileStore
    rng = np.random.RandomState(21)
    w = rng.randn(3, 4, 1, 224) * 20 + 3
    if padded:
        for i in range(3):
            for j in range(4):
                w[i, j, 0, 120 + 17 * j + i:] = 0.0
    tgt = np.eye(2, dtype=np.float32)[[0, 1, 1]]
    store = DeviceTileStore(w, tgt, 2.5, 17.0)
    store.padded = padded
    store.hours = np.arange(12, dtype=np.float64).reshape(3, 4) / 4
    if filters:
        store.set_filters(**filters)
    return store


@pytest.mark.parametrize('variant', ['plain', 'padded', 'butterworth'])
def test_dtw_analyze_equals_the_reference_loop(D, variant):
    store = _analyze_store(padded=variant == 'padded', filters=dict(butter_low=0, butter_high=10) if variant == 'butterworth' else None)
    served = store.batch(torch.arange(3))[0].cpu().numpy().astype(np.float64)              # breaths as the dataset serves them
    for nb in (3, 1):
        want = R.reference_analyze([served[i, :, 0, :] for i in range(3)], nb)
        df = D.dtw_analyze(store, n_breaths=nb)
        got = df['dtw'].values
        assert len(got) == 12 and np.isnan(got[:nb]).all() and not np.isnan(got[nb:]).any()
        assert bits(got[nb:]) == bits(want[nb:]), (variant, nb)
        assert list(df.index) == [0] * 4 + [1] * 4 + [2] * 4
        hours = df['hour'].values
        assert np.isnan(hours[:nb]).all() and bits(hours[nb:]) == bits(store.hours.reshape(-1)[nb:])
    # a subset of windows in another order, and the rolling average behind its NaN prefix
    want = R.reference_analyze([served[2, :, 0, :], served[0, :, 0, :]], 3)
    df = D.dtw_analyze(store, n_breaths=3, rolling_av_len=2, indices=[2, 0])
    rolled = np.append([np.nan], np.convolve(want, np.ones((2,)) / 2, mode='valid'))
    assert bits(df['dtw'].values[4:]) == bits(rolled[4:]) and np.isnan(df['dtw'].values[:4]).all()
    # rows given directly, and too few breaths for any score
    rows = cuda(served[:, :, 0, :].reshape(12, 224).astype(np.float32))
    assert bits(D.dtw_analyze(rows, n_breaths=3)['dtw'].values[3:]) == bits(R.reference_analyze([served[i, :, 0, :] for i in range(3)], 3)[3:])
    assert np.isnan(D.dtw_analyze(rows[:3], n_breaths=3)['dtw'].values).all()


def test_analyze_patient_takes_the_patients_windows(D):
    store = _analyze_store()
    store.patient_slot = np.array([1, 0, 1])
    served = store.batch(torch.arange(3))[0].cpu().numpy().astype(np.float64)
    df = D.analyze_patient(1, store)
    want = R.reference_analyze([served[0, :, 0, :], served[2, :, 0, :]], 3)
    assert list(df.index) == [0] * 4 + [2] * 4 and bits(df['dtw'].values[3:]) == bits(want[3:])
    with pytest.raises(ValueError, match='no window'):
        D.analyze_patient(5, store)


# ---- find_patient_similarity ------------------------------------------------------------------------------------------------
def _similarity_dataset():
    from deepards_amd import ingest
    rng = np.random.RandomState(31)
    counts = {'w': 1, 'x': 2, 'y': 5, 'z': 60}
    pat = np.array([p for p, c in counts.items() for _ in range(c)])
    rng.shuffle(pat)
    n = len(pat)
    windows = rng.randn(n, 2, 1, 32) * 40
    tgt = np.eye(2, dtype=np.float32)[rng.randint(0, 2, n)]
    return ingest.IngestedDataset(windows, tgt, pat, np.zeros((n, 2)), {None: (np.zeros(1), np.ones(1))}, 2,
                                  'unpadded_centered_sequences')


def test_find_patient_similarity_equals_the_restated_reference(D):
    ds = _similarity_dataset()
    n = len(ds)
    for method in ('random', 'same_ordered'):
        pts, want = R.reference_similarity(ds.windows, ds.patients, np.arange(n), method, np.random.RandomState(17))
        df = D.find_patient_similarity(ds, method, seed=17)
        assert list(df.index) == list(df.columns) == pts
        assert bits(df.values) == bits(want), (method, df.values, want)
        assert (np.diag(df.values) == 0).all() and bits(df.values) == bits(df.values.T.copy())
        assert not np.isnan(df.values).any() and (df.values[~np.eye(4, dtype=bool)] > 0).all()
        few = D.find_patient_similarity(ds, method, seed=17, byte_budget=16 * 5)          # many launches: the same matrix
        assert bits(few.values) == bits(want)
        store = ds.to_store()                                                             # a store: indexed by slot number
        by_slot = D.find_patient_similarity(store, method, seed=17)
        assert list(by_slot.index) == [0, 1, 2, 3] and bits(by_slot.values) == bits(want)
    none = D.find_patient_similarity(ds, 'random', n=0, seed=17)                          # no window pair anywhere: NaN
    off = ~np.eye(4, dtype=bool)
    assert np.isnan(none.values[off]).all() and (np.diag(none.values) == 0).all()


# ---- command line -----------------------------------------------------------------------------------------------------------
def test_command_lines_in_a_child_process(D, tmp_path):
    import pandas as pd
    ds = _similarity_dataset()
    path = str(tmp_path / 'toy.npz')
    ds.save_npz(path, anonymise=False)
    env = dict(os.environ, PYTHONPATH=ROOT)
    pkl = str(tmp_path / 'sim.pkl')
    run = subprocess.run([sys.executable, '-m', 'deepards_amd.dtw', 'similarity', '-p', path, '--dist-method', 'random', '--seed', '17',
                          '-o', pkl], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-2000:])
    df = pd.read_pickle(pkl)
    pts, want = R.reference_similarity(ds.windows, ds.patients, np.arange(len(ds)), 'random', np.random.RandomState(17))
    assert list(df.index) == pts and bits(df.values) == bits(want)
    out = str(tmp_path / 'scores.npz')
    run = subprocess.run([sys.executable, '-m', 'deepards_amd.dtw', 'analyze', '-p', path, '--patient', 'y', '--n-breaths', '3',
                          '-o', out], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-2000:])
    z = np.load(out)
    store = ds.to_store()
    store.patient_ids = ds.patients
    want = D.analyze_patient('y', store)
    assert len(z['dtw']) == 5 * 2 and bits(z['dtw']) == bits(want['dtw'].values) and np.isnan(z['dtw'][:3]).all()
    assert list(z['window']) == list(want.index) and (z['patient_slot'] == z['patient_slot'][0]).all()
