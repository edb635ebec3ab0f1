"""Numpy oracle of the DTW distance (include/deepards_hip.h, section dynamic time warping) in two cell orders, and restatements
of what dtw_lib.py does with it (the pair lists of find_patient_similarity, the per-breath score loop of dtw_analyze).

    c(i,j) = |x[i] - y[j]| or (x[i] - y[j])^2;  +inf where |i - j| > band
    D(0,0) = c(0,0);  D(i,j) = c(i,j) + min(of the neighbours (i-1,j), (i,j-1), (i-1,j-1) that exist);  dtw = D(n-1,m-1)

Every operation is one numpy operation on ``dtype`` scalars or arrays, so float32 rounds after each one exactly as the float32
kernel does.  ``dtw_rows`` walks the cells row by row in plain Python (slow, obviously the definition); ``dtw_diagonals`` walks
anti-diagonals with one vector operation per step of the recurrence (fast enough for 4480 x 4480).  min of non-NaN values is
exact, so the two agree bit for bit -- tests/test_dtw_cpu.py holds them to that."""
import numpy as np


def _operands(x, y, dtype):
    dtype = np.dtype(dtype).type
    x, y = np.asarray(x, dtype=dtype).reshape(-1), np.asarray(y, dtype=dtype).reshape(-1)
    assert x.size >= 1 and y.size >= 1
    return x, y, dtype


def dtw_rows(x, y, dtype=np.float64, metric='euclidean', band=None):
    x, y, dtype = _operands(x, y, dtype)
    inf = dtype(np.inf)
    above = None
    for i in range(x.size):
        row = []
        for j in range(y.size):
            d = x[i] - y[j]
            c = abs(d) if metric == 'euclidean' else d * d
            if band is not None and abs(i - j) > band:
                c = inf
            near = []
            if i > 0:
                near.append(above[j])
            if j > 0:
                near.append(row[j - 1])
            if i > 0 and j > 0:
                near.append(above[j - 1])
            row.append(dtype(c + min(near)) if near else dtype(c))
        above = row
    return above[-1]


def dtw_diagonals(x, y, dtype=np.float64, metric='euclidean', band=None):
    x, y, dtype = _operands(x, y, dtype)
    n, m = x.size, y.size
    inf = dtype(np.inf)
    # diagonals d - 1 and d - 2, slot i + 1 holds row i (slot 0: row -1); D(-1,-1) = 0 stands in for "no neighbour" at (0,0)
    one_back = np.full(n + 1, inf, dtype=dtype)
    two_back = np.full(n + 1, inf, dtype=dtype)
    two_back[0] = dtype(0)
    for d in range(n + m - 1):
        i = np.arange(max(0, d - m + 1), min(n - 1, d) + 1)
        j = d - i
        diff = x[i] - y[j]
        cost = np.abs(diff) if metric == 'euclidean' else diff * diff
        if band is not None:
            cost = np.where(np.abs(i - j) > band, inf, cost)
        best = np.minimum(np.minimum(one_back[i], two_back[i]), one_back[i + 1])
        cur = np.full(n + 1, inf, dtype=dtype)
        cur[i + 1] = cost + best
        two_back, one_back = one_back, cur
    return one_back[n]


def dtw(x, y, dtype=np.float64, metric='euclidean', band=None):
    return dtw_diagonals(x, y, dtype, metric, band)


def ordered_mean(values):
    """((0 + v0) + v1) + ... in float64, over the count; NaN for none: ``score / len(prev_flow_waves)``."""
    if len(values) == 0:
        return np.float64(np.nan)
    s = np.float64(0.0)
    for v in values:
        s = s + np.float64(v)
    return s / np.float64(len(values))


# ---- find_patient_similarity's pair lists (dtw_lib.py:185-249), over a pandas frame as the reference holds its ground truth ----
def reference_pairs(window_patient, window_index, dist_method, rng, n=50):
    """-> {(pt, other_pt): [(window of pt, window of other_pt), ...]} in the reference's order, patients in the order of
    ``gt.patient.unique()``; the draws come from ``rng`` where the reference calls ``np.random.choice``."""
    import pandas as pd
    gt = pd.DataFrame({'patient': list(window_patient)}, index=list(window_index)).sort_index()
    pts = list(gt.patient.unique())
    by_pt = {pt: gt[gt.patient == pt] for pt in pts}
    out = {}
    for pos, pt in enumerate(pts):
        later = pts[pos + 1:]
        for other in later:
            out[(pt, other)] = []
        if dist_method == 'same_ordered':
            for iloc, (idx, _) in enumerate(by_pt[pt].iterrows()):
                for other in later:
                    if iloc >= len(by_pt[other]):
                        continue
                    out[(pt, other)].append((idx, by_pt[other].iloc[iloc].name))
        else:
            own = by_pt[pt].index
            mine = rng.choice(own, min(n, len(own)), replace=False)
            for other in later:
                theirs_all = by_pt[other].index
                theirs = rng.choice(theirs_all, min(len(mine), len(theirs_all)), replace=False)
                for q, idx in enumerate(theirs):
                    out[(pt, other)].append((mine[q], idx))
    return pts, out


def reference_similarity(windows, window_patient, window_index, dist_method, rng, n=50, dtype=np.float64):
    """The matrix of dtw_lib.py:295-306 over the oracle: windows (N, ...) raw, ravelled per window."""
    pts, pairs = reference_pairs(window_patient, window_index, dist_method, rng, n)
    mat = np.zeros((len(pts), len(pts)))
    for (a, b), lst in pairs.items():
        ds = [dtw(np.ravel(windows[p]), np.ravel(windows[q]), dtype) for p, q in lst]
        v = ordered_mean(ds)
        mat[pts.index(a), pts.index(b)] = mat[pts.index(b), pts.index(a)] = v
    return pts, mat


# ---- dtw_analyze's score loop (dtw_lib.py:330-370) --------------------------------------------------------------------------
def reference_analyze(windows, n_breaths, dtype=np.float64):
    """windows: list of (NB, L) arrays of one patient in order -> the scores before the rolling average, NaN for the first
    n_breaths breaths; a sliding list of the last n_breaths breaths, the current one scored against them oldest first."""
    recent, scores = [], [np.nan] * n_breaths
    for seq in windows:
        for breath in seq:
            breath = np.ravel(breath)
            if len(recent) == n_breaths + 1:
                recent.pop(0)
            if len(recent) < n_breaths:
                recent.append(breath)
                continue
            scores.append(ordered_mean([dtw(old, breath, dtype) for old in recent]))
            recent.append(breath)
    return np.asarray(scores, dtype=np.float64)
