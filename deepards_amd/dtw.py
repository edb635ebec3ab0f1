"""Dynamic time warping on the device: the reference's ``dtw_lib`` surface over csrc/dtw.hip.

The distance (this definition governs; include/deepards_hip.h states it in full): for 1-D x (n >= 1) and y (m >= 1)

    c(i,j) = |x[i] - y[j]|  ('euclidean')  |  (x[i] - y[j])^2  ('sqeuclidean')
    D(i,j) = c(i,j) + min(D(i-1,j), D(i,j-1), D(i-1,j-1)),   D(0,0) = c(0,0),   dtw(x,y) = D(n-1,m-1)

with an optional Sakoe-Chiba band, one IEEE operation per step in the accumulation type -- so the result is defined bit for
bit.  This is ``dtwco.warping.core.dtw(x, y)`` with its defaults AS ITS DOCUMENTATION DESCRIBES THEM (unnormalised accumulated
cost, metric 'euclidean' on scalars, the symmetric step pattern); dtwco is not installed where this was written and that
reading was never checked against dtwco itself.

    dtw(x, y)                        one pair -> float
    dtw_pairs(table, ia, ib)         P pairs in one launch -> device tensor
    dtw_analyze / analyze_patient    dtw_lib.py:330-409: every breath against the n_breaths before it
    find_patient_similarity[_for_kfold]   dtw_lib.py:185-327: the patient x patient matrix of mean window distances

acc='f64' is the default because the reference computes in double; acc='f32' (float32 tables only) is the fast opt-in, within
(n + m + 1) 2^-24 relative of the double result.  Refused with a reason: lengths above 4608, windows of more than one channel
(the reference ravels them into one sequence; that is not built), CPU tensors, acc='f32' on float64 data.  Not built:
``pick_similar_pts`` / ``pick_dissimilar_pts``, ``KMedoids`` / ``mediod_process``, plots, ``lstm_dtw.py``, Grad-CAM's
``dtw_clust``, warping paths (``dist_only=False``) and ``warping_penalty``; there is no cache directory.

Command line:
    python -m deepards_amd.dtw similarity -p dataset.pkl|.npz [--fold K] [--dist-method random|same_ordered] [-n 50]
        [--seed S] -o out.npz|out.pkl        (.pkl: the DataFrame through pd.to_pickle, what sim_dissim_experiments_script.py reads)
    python -m deepards_amd.dtw analyze -p dataset.pkl|.npz [--fold K] [--patient SLOT|ID] [--n-breaths 3] [--rolling-av-len 1]
        -o out.npz
"""
import argparse
import sys

import numpy as np
import torch

from . import dtw_ops as O
from .dtw_ops import MAX_LEN, dtw_plan, dtw_shape_ok, segment_mean  # noqa: F401  (part of this module's surface)

PAIR_BYTES = 16                        # device bytes one pair costs beside the tables: two int32 indices and a float64 distance
DEFAULT_BYTE_BUDGET = 256 << 20


# ---- single pairs and tables ------------------------------------------------------------------------------------------------
def _row(v, name):
    """A 1-D sequence before any upload: arrays and lists become float32 (if they are) or float64 host arrays, device tensors
    are taken as they are, CPU tensors are refused -> (array or tensor, length, whether float64)."""
    if isinstance(v, torch.Tensor):
        if not v.is_cuda:
            raise ValueError('dtw: %s is a CPU tensor; pass an array, or move it to the device' % name)
        if v.dtype not in (torch.float32, torch.float64):
            raise ValueError('dtw: %s must be float32 or float64, got %s' % (name, v.dtype))
        t, is64 = v, v.dtype == torch.float64
    else:
        t = np.asarray(v)
        t = np.ascontiguousarray(t if t.dtype == np.float32 else t.astype(np.float64))
        is64 = t.dtype == np.float64
    if t.ndim != 1:
        raise ValueError('dtw: %s must be one 1-D sequence, got shape %s (a multi-channel breath is not ravelled here)'
                         % (name, tuple(t.shape)))
    return t, t.shape[0], is64


def dtw(x, y, metric='euclidean', band=None, acc='f64', device='cuda'):
    """``dtwco``'s ``dtw(x, y)`` (see the module docstring for the caveat) for one pair -> Python float.  Refusals come before
    anything is uploaded."""
    (x, n, x64), (y, m, y64) = _row(x, 'x'), _row(y, 'y')
    why = O.dtw_refusal(n, m, acc, x64, y64)
    if why:
        raise ValueError('dtw: ' + why)
    if metric not in O.METRICS:
        raise ValueError("dtw: metric must be 'euclidean' or 'sqeuclidean', got %r" % (metric,))
    dev = x.device if isinstance(x, torch.Tensor) else y.device if isinstance(y, torch.Tensor) else device
    ta, tb = (t if isinstance(t, torch.Tensor) else torch.as_tensor(t).to(dev) for t in (x, y))
    return float(O.dtw_pairs(ta.contiguous().reshape(1, -1), [0], [0], tb.contiguous().reshape(1, -1), metric=metric, band=band,
                             acc=acc)[0])


def dtw_pairs(table_a, ia, ib, table_b=None, metric='euclidean', band=None, acc='f64', out=None):
    """out[p] = dtw(table_a[ia[p]], table_b[ib[p]]) for all P pairs in one launch -> (P,) device tensor of the accumulation
    type (``dtw_ops.dtw_pairs``: the operand rules are there)."""
    return O.dtw_pairs(table_a, ia, ib, table_b, metric=metric, band=band, acc=acc, out=out)


# ---- dtw_analyze (dtw_lib.py:330-372) ---------------------------------------------------------------------------------------
def analyze_index_arrays(n_rows, n_breaths, device='cuda'):
    """The pairs and segments of ``dtw_analyze`` over ``n_rows`` breaths in order, built on ``device``: breath t >= n_breaths is
    segment t - n_breaths and holds the pairs (t - n_breaths, t), ..., (t - 1, t), oldest first, as
    ``_find_per_breath_dtw_score`` walks ``prev_flow_waves``.  -> (ia, ib, offsets) int32, or None when no breath has
    n_breaths predecessors."""
    nb = int(n_breaths)
    if nb < 1:
        raise ValueError('dtw_analyze: n_breaths must be at least 1, got %r' % (n_breaths,))
    g = int(n_rows) - nb
    if g < 1:
        return None
    seg = torch.arange(g, device=device, dtype=torch.int32)
    ia = (seg[:, None] + torch.arange(nb, device=device, dtype=torch.int32)[None, :]).reshape(-1)
    ib = (seg + nb).repeat_interleave(nb)
    offsets = torch.arange(g + 1, device=device, dtype=torch.int32) * nb
    return ia.contiguous(), ib.contiguous(), offsets.contiguous()


def _is_store(obj):
    return hasattr(obj, 'tiles') and hasattr(obj, 'batch')


def _breath_rows(src, indices):
    """-> (rows (T, L) device table, hours (T,) or None, window index per row (T,) or None)."""
    if _is_store(src):
        if src.tiles.shape[2] != 1:
            raise ValueError('dtw: windows of %d channels: the reference ravels a multi-channel breath into one sequence '
                             '(dtw_lib.py:362); that is not built, only C = 1 is' % src.tiles.shape[2])
        rel = np.arange(len(src)) if indices is None else np.asarray(indices, dtype=np.int64).reshape(-1)
        if rel.size == 0:
            raise ValueError('dtw_analyze: no windows')
        x, _ = src.batch(torch.as_tensor(rel))                # normalised and filtered, as the dataset serves them
        b, nb, _, l = x.shape
        absidx = rel if src.kfold_indexes is None else src.kfold_indexes.cpu().numpy()[rel]
        hours = None
        if src.hours is not None:
            hours = np.asarray(src.hours, dtype=np.float64)[absidx].reshape(-1)
        return x.reshape(b * nb, l), hours, np.repeat(absidx, nb)
    if indices is not None:
        raise ValueError('dtw_analyze: indices select windows of a store; rows are taken as they are')
    t = src if isinstance(src, torch.Tensor) else None
    if t is None:
        a = np.asarray(src)
        if a.ndim == 4 and a.shape[2] != 1:
            raise ValueError('dtw: windows of %d channels are not built, only C = 1 is (the reference ravels them)' % a.shape[2])
        if a.ndim not in (2, 3, 4):
            raise ValueError('dtw_analyze: breaths (T, L), windows (B, NB, L) or (B, NB, 1, L) expected, got %s' % (a.shape,))
        t = torch.as_tensor(np.ascontiguousarray(a if a.dtype == np.float32 else a.astype(np.float64))).cuda()
    elif not t.is_cuda:
        raise ValueError('dtw: the breaths are a CPU tensor; pass an array, or move it to the device')
    if t.dim() == 4:
        if t.shape[2] != 1:
            raise ValueError('dtw: windows of %d channels are not built, only C = 1 is (the reference ravels them)' % t.shape[2])
        t = t.reshape(t.shape[0] * t.shape[1], t.shape[3])
    elif t.dim() == 3:
        t = t.reshape(t.shape[0] * t.shape[1], t.shape[2])
    if t.dim() != 2:
        raise ValueError('dtw_analyze: breaths (T, L), windows (B, NB, L) or (B, NB, 1, L) expected, got %s' % (tuple(t.shape),))
    return t, None, None


def rolling_average(scores, rolling_av_len):
    """dtw_lib.py:371-372: ``np.convolve(scores, ones / len, 'valid')`` behind its NaN prefix."""
    k = int(rolling_av_len)
    if k < 1:
        raise ValueError('dtw_analyze: rolling_av_len must be at least 1, got %r' % (rolling_av_len,))
    scores = np.asarray(scores, dtype=np.float64)
    if k > len(scores):
        return np.full(len(scores), np.nan)
    return np.append([np.nan] * (k - 1), np.convolve(scores, np.ones((k,)) / k, mode='valid'))


def dtw_analyze(store_or_rows, n_breaths=3, rolling_av_len=1, indices=None, metric='euclidean', band=None, acc='f64'):
    """``dtw_lib.dtw_analyze`` for one patient's windows in order: breath t >= n_breaths scores the mean of
    dtw(breath[t - j], breath[t]), j = n_breaths .. 1, across window boundaries; the first n_breaths scores are NaN.
    ``store_or_rows``: a DeviceTileStore (``indices``: its fold-relative windows, in order; None: all) whose breaths are taken
    through the store's gather -- normalised and filtered --, or the breaths themselves, (T, L) / (B, NB, L) / (B, NB, 1, L).
    One pairs launch and one segment-mean launch; the index arithmetic runs on the device.
    -> pandas.DataFrame with column 'dtw' (after the rolling average) and, for a store with hours, 'hour' (NaN for the first
    n_breaths rows, as the reference leaves them); indexed by window for a store."""
    import pandas as pd
    rows, hours, widx = _breath_rows(store_or_rows, indices)
    t = rows.shape[0]
    scores = torch.full((t,), float('nan'), device=rows.device, dtype=torch.float64)
    arrays = analyze_index_arrays(t, n_breaths, rows.device)
    if arrays is not None:
        ia, ib, offsets = arrays
        dist = O.dtw_pairs(rows, ia, ib, metric=metric, band=band, acc=acc)
        O.segment_mean(dist, offsets, out=scores[int(n_breaths):])
    cols = {'dtw': rolling_average(scores.cpu().numpy(), rolling_av_len)}
    if hours is not None:
        hours = hours.copy()
        hours[:int(n_breaths)] = np.nan
        cols['hour'] = hours
    return pd.DataFrame(cols, index=widx)


def _fold_windows(store):
    """Absolute window indices the store serves, ascending, WITHOUT oversampling (dtw_lib.py:277 switches it off)."""
    if store.kfold_num is not None and store.total_kfolds is not None:
        idx = np.asarray(store.get_kfold_indexes_for_fold(store.kfold_num), dtype=np.int64)
    elif store.kfold_indexes is not None:
        idx = np.unique(store.kfold_indexes.cpu().numpy())
    else:
        idx = np.arange(store.tiles.shape[0], dtype=np.int64)
    return np.sort(idx)


def _slot_of(store, slot_or_id):
    ids = getattr(store, 'patient_ids', None)
    if isinstance(slot_or_id, str) and not slot_or_id.lstrip('-').isdigit():
        if ids is None:
            raise ValueError('dtw: the dataset file carries no patient identifiers; name the patient by slot number')
        hit = np.nonzero(np.asarray(ids).astype(str) == slot_or_id)[0]
        if hit.size == 0:
            raise ValueError('dtw: no patient %r in this dataset' % slot_or_id)
        return int(np.asarray(store.patient_slot)[hit[0]])
    return int(slot_or_id)


def analyze_patient(slot_or_id, store, n_breaths=3, rolling_av_len=1, **kw):
    """``dtw_lib.analyze_patient`` without its cache directory: ``dtw_analyze`` over the windows of one patient (slot number,
    or identifier where the store carries ``patient_ids``) that the store's current fold serves, in the store's order."""
    if store.patient_slot is None:
        raise ValueError('dtw: this store carries no patient information')
    slot = _slot_of(store, slot_or_id)
    served = np.arange(store.tiles.shape[0]) if store.kfold_indexes is None else store.kfold_indexes.cpu().numpy()
    rel = np.nonzero(np.asarray(store.patient_slot)[served] == slot)[0]
    if rel.size == 0:
        raise ValueError('dtw: patient %r has no window in what the store serves' % (slot_or_id,))
    return dtw_analyze(store, n_breaths, rolling_av_len, indices=rel, **kw)


# ---- find_patient_similarity (dtw_lib.py:185-327) ---------------------------------------------------------------------------
def similarity_pairs(window_patient, window_index, dist_method='random', n=50, rng=None):
    """The window pairs of ``find_patient_similarity``, on the host.  window_patient / window_index: patient and absolute
    index of every served window, index ascending (``gt.sort_index()``).  Patients in order of first appearance; 'random'
    (``random_compare_seqs``): per patient one ``choice(pt_seqs, min(n, len), replace=False)``, then per later patient one
    ``choice(other_seqs, n_o, replace=False)``, pair i = (rand_seqs[i], other_rand[i]) -- drawn from ``rng`` in that call
    order; 'same_ordered' (``compare_by_same_ordered_seqs``): the iloc-th windows of both while both exist.
    -> (patients, ia, ib, offsets, segments): segment s = patients pair ``segments[s]`` = (i, j), i < j, holds the pairs
    offsets[s]:offsets[s + 1]."""
    if dist_method not in ('random', 'same_ordered'):
        raise ValueError('Inputs to this function only accept "random" or "same_ordered" choices for dist_method.')
    window_patient, window_index = np.asarray(window_patient), np.asarray(window_index, dtype=np.int64)
    pts, seen = [], set()
    for p in window_patient.tolist():
        if p not in seen:
            seen.add(p)
            pts.append(p)
    seqs = {p: window_index[window_patient == p] for p in pts}
    rng = np.random.RandomState() if rng is None else rng
    ia, ib, offsets, segments = [], [], [0], []
    for i, pt in enumerate(pts):
        pt_seqs = seqs[pt]
        if dist_method == 'random':
            rand_seqs = rng.choice(pt_seqs, min(int(n), len(pt_seqs)), replace=False)
        for j in range(i + 1, len(pts)):
            other = seqs[pts[j]]
            if dist_method == 'random':
                n_o = min(len(rand_seqs), len(other))
                other_rand = rng.choice(other, n_o, replace=False)
                ia.extend(rand_seqs[:n_o].tolist())
                ib.extend(other_rand.tolist())
            else:
                k = min(len(pt_seqs), len(other))
                ia.extend(pt_seqs[:k].tolist())
                ib.extend(other[:k].tolist())
            offsets.append(len(ia))
            segments.append((i, j))
    return pts, np.asarray(ia, dtype=np.int64), np.asarray(ib, dtype=np.int64), np.asarray(offsets, dtype=np.int64), segments


def _check_windows(shape, acc):
    """Refuse, before anything is uploaded or launched, windows (N, NB, C, L) that the comparison of flattened windows does not
    take."""
    if len(shape) != 4:
        raise ValueError('dtw: windows (N, NB, C, L) expected, got shape %s' % (tuple(shape),))
    if shape[2] != 1:
        raise ValueError('dtw: windows of %d channels: the reference ravels them into one sequence; that is not built, only '
                         'C = 1 is' % shape[2])
    length = shape[1] * shape[3]
    why = O.dtw_refusal(length, length, acc, True, True)
    if why:
        raise ValueError('dtw: windows flatten to NB L = %d samples: %s' % (length, why))
    return length


def _similarity_source(src, device, acc):
    """-> (tiles (N, NB, C, L) float64 on the device, patient slot per window, identifiers per slot or None, served windows)."""
    if _is_store(src):
        if src.patient_slot is None:
            raise ValueError('dtw: this store carries no patient information')
        return src.tiles, np.asarray(src.patient_slot), getattr(src, 'patient_ids', None), _fold_windows(src)
    if hasattr(src, 'windows') and hasattr(src, 'patient_slot'):                 # ingest.IngestedDataset
        if src.patient_slot is None:
            raise ValueError('dtw: this dataset file carries no patient information')
        if getattr(src, 'breath_level', False):
            raise ValueError('dtw: a breath-level dataset has no windows to compare')
        _check_windows(src.windows.shape, acc)
        tiles = torch.as_tensor(src.windows, dtype=torch.float64).to(device)
        return tiles, np.asarray(src.patient_slot), src.patients, np.arange(tiles.shape[0], dtype=np.int64)
    raise ValueError('dtw: a DeviceTileStore or an ingested dataset expected, got %s' % type(src).__name__)


def find_patient_similarity(dataset_or_store, dist_method='random', n=50, seed=None, metric='euclidean', band=None, acc='f64',
                            byte_budget=DEFAULT_BYTE_BUDGET, device='cuda'):
    """``dtw_lib.find_patient_similarity`` on the device: the symmetric patient x patient DataFrame of mean DTW distances
    between RAW (un-normalised) windows flattened to NB L samples -- ``all_sequences[idx][1].ravel()`` --, zero on the
    diagonal, NaN for a patient pair without a window pair; indexed by patient identifier (by slot number when the file
    carries none).  The pairs are drawn on the host by ``similarity_pairs`` from ``np.random.RandomState(seed)``; all of them
    go to the device in ceil(16 P / byte_budget) pairs launches plus one segment-mean launch.  The mean is the float64 sum
    in pair order over the count (``np.mean`` sums pairwise from 8 values on: the last bits may differ).  Oversampling
    indices are ignored, as the reference switches oversampling off."""
    import pandas as pd
    if dist_method not in ('random', 'same_ordered'):
        raise ValueError('Inputs to this function only accept "random" or "same_ordered" choices for dist_method.')
    tiles, slots, ids, served = _similarity_source(dataset_or_store, device, acc)
    length = _check_windows(tiles.shape, acc)
    pts, ia, ib, offsets, segments = similarity_pairs(slots[served], served, dist_method, n, np.random.RandomState(seed))
    mat = np.zeros((len(pts), len(pts)), dtype=np.float64)
    if segments:
        table = tiles.reshape(tiles.shape[0], length)
        total = len(ia)
        means = np.full(len(segments), np.nan)
        if total:
            dist = torch.empty((total,), device=table.device, dtype=torch.float32 if acc == 'f32' else torch.float64)
            chunk = max(1, int(byte_budget) // PAIR_BYTES)
            for s in range(0, total, chunk):
                e = min(total, s + chunk)
                O.dtw_pairs(table, ia[s:e], ib[s:e], metric=metric, band=band, acc=acc, out=dist[s:e])
            means = O.segment_mean(dist, offsets).cpu().numpy()
        for (i, j), v in zip(segments, means):
            mat[i, j] = mat[j, i] = v
    names = pts
    if ids is not None:
        first = {}
        for s_, id_ in zip(slots.tolist(), np.asarray(ids).astype(str).tolist()):
            first.setdefault(s_, id_)
        names = [first[p] for p in pts]
    return pd.DataFrame(mat, index=names, columns=names)


def find_patient_similarity_for_kfold(store, fold_num, dist_method='random', **kw):
    """``dtw_lib.find_patient_similarity_for_kfold``: ``set_kfold_indexes_for_fold(fold_num)`` first."""
    store.set_kfold_indexes_for_fold(fold_num)
    return find_patient_similarity(store, dist_method, **kw)


# ---- command line -----------------------------------------------------------------------------------------------------------
def build_parser():
    parser = argparse.ArgumentParser(prog='python -m deepards_amd.dtw', description='DTW analyses of dtw_lib.py on the device '
                                     '(arrays and DataFrames, no plots)')
    sub = parser.add_subparsers(dest='command', required=True)
    for name in ('similarity', 'analyze'):
        p = sub.add_parser(name)
        p.add_argument('-p', '--pickled-data-path', required=True,
                       help='ARDSRawDataset pickle (read without unpickling) or its .npz export')
        p.add_argument('--fold', type=int, default=None, help='k-fold whose windows are analysed (default: every window)')
        p.add_argument('--test', action='store_true', help="with --fold: the fold's test patients instead of its train patients")
        p.add_argument('--metric', choices=sorted(O.METRICS), default='euclidean')
        p.add_argument('--band', type=int, default=None, help='Sakoe-Chiba radius (default: none)')
        p.add_argument('--acc', choices=sorted(O.ACC), default='f64')
        p.add_argument('-o', '--output', required=True)
    p = sub.choices['similarity']
    p.add_argument('--dist-method', choices=['random', 'same_ordered'], default='random')
    p.add_argument('-n', type=int, default=50, help="windows drawn per patient by 'random'")
    p.add_argument('--seed', type=int, default=None)
    p = sub.choices['analyze']
    p.add_argument('--patient', default=None, help='slot number or identifier (default: every patient)')
    p.add_argument('--n-breaths', type=int, default=3)
    p.add_argument('--rolling-av-len', type=int, default=1)
    return parser


def _load_store(args):
    from . import ingest
    ds = ingest.load_dataset(args.pickled_data_path)
    store = ds.to_store(device='cuda', fold=args.fold)
    store.patient_ids = ds.patients
    if args.fold is not None:
        if store.total_kfolds is None:
            raise SystemExit('--fold: %s is not a k-fold dataset' % args.pickled_data_path)
        store.train = not args.test
        store.set_kfold_indexes_for_fold(args.fold)
    return store


def main(argv=None):
    args = build_parser().parse_args(argv)
    store = _load_store(args)
    kw = dict(metric=args.metric, band=args.band, acc=args.acc)
    if args.command == 'similarity':
        if not (args.output.endswith('.npz') or args.output.endswith('.pkl')):
            raise SystemExit('-o must end in .npz or .pkl')
        df = find_patient_similarity(store, args.dist_method, n=args.n, seed=args.seed, **kw)
        if args.output.endswith('.pkl'):
            import pandas as pd
            pd.to_pickle(df, args.output)
        else:
            np.savez(args.output, distance=df.values, patients=np.asarray(df.index).astype(str))
        print('%d patients, %s -> %s' % (len(df), args.dist_method, args.output))
        return 0
    if store.patient_slot is None:
        raise SystemExit('analyze: this dataset file carries no patient information')
    if args.patient is not None:
        slots = [_slot_of(store, args.patient)]
    else:
        slots = []
        for s in np.asarray(store.patient_slot)[_fold_windows(store)].tolist():
            if s not in slots:
                slots.append(s)
    parts = [analyze_patient(s, store, args.n_breaths, args.rolling_av_len, **kw) for s in slots]
    out = dict(dtw=np.concatenate([p['dtw'].values for p in parts]),
               window=np.concatenate([np.asarray(p.index, dtype=np.int64) for p in parts]),
               patient_slot=np.concatenate([np.full(len(p), s, dtype=np.int64) for s, p in zip(slots, parts)]),
               n_breaths=args.n_breaths, rolling_av_len=args.rolling_av_len)
    if all('hour' in p for p in parts):
        out['hour'] = np.concatenate([p['hour'].values for p in parts])
    np.savez(args.output, **out)
    print('%d patients, %d breaths -> %s' % (len(slots), len(out['dtw']), args.output))
    return 0


if __name__ == '__main__':
    sys.exit(main())
