"""Cost of the frequency filters in the device batch path (reported, not gated; bench.py measures the flagship):

    python scripts/bench_batch_filters.py [--batch 64] [--calls 200] [--rounds 7] [--out FILE.json]

``DeviceTileStore.batch_from_device`` at B windows of (20, 1, 224), written into fixed ``out=`` buffers the way the captured
step is fed, in four forms: plain (no filter: ``da_gather_normalize``, the only path before the filters existed), butter
(lowpass 10 Hz), fft (band (0, 6) Hz) and both (``da_gather_normalize_filter``); and, on windows whose rows are zero behind a
random length (a padded_breath_by_breath dataset), in the forms of ``da_gather_normalize_chain``: padded (the padded
normalisation alone), down_2 and down_1p2 (post-hoc downsampling by 2.0 and by 1.2: new_len 112 and 186) and chain
(Butterworth + downsampling by 1.2 + FFT band).  Two figures per form:

* ``us_per_batch``   a host clock around ``calls`` batches (gather launch + ``gather_rows`` + the Python around them) ending in
                     a device synchronise: what a training loop pays per step when nothing else hides it;
* ``us_per_gather``  the gather launch alone, ``calls`` of them captured into one hipGraph on one stream and replayed, timed
                     with device events: the kernel with its launch gap, without the host.

Per form: a warm-up, then ``rounds`` timed windows, the forms ALTERNATING round by round so that drift of a shared machine
lands on all of them; median, minimum and maximum are printed, one JSON line per form.  No GPU, no number: the script fails."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BOTH = dict(butter_low=0, butter_high=10, fft_filtering_low=0, fft_filtering_high=6)
# name, set_filters keywords, padded dataset
FORMS = (('plain', {}, False), ('butter', dict(butter_low=0, butter_high=10), False),
         ('fft', dict(fft_filtering_low=0, fft_filtering_high=6), False), ('both', BOTH, False),
         ('padded', {}, True), ('down_2', dict(post_hoc_downsampling=2.0), True), ('down_1p2', dict(post_hoc_downsampling=1.2), True),
         ('chain', dict(BOTH, post_hoc_downsampling=1.2), True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--windows', type=int, default=4096, help='windows in the store (4096 x 20 x 224 float64 = 147 MB)')
    ap.add_argument('--out')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_batch_filters needs an MI355X: there is no CPU timing')
    from deepards_amd.data import DeviceTileStore
    rng = np.random.default_rng(0)
    windows = rng.standard_normal((a.windows, 20, 1, 224)) * 28 + 2
    lengths = rng.integers(30, 225, (a.windows, 20, 1, 1))
    padded_windows = np.where(np.arange(224).reshape(1, 1, 1, 224) < lengths, windows, 0.0)
    targets = np.eye(2, dtype=np.float32)[rng.integers(0, 2, a.windows)]
    stores, graphs = {}, {}
    perm = torch.from_numpy(rng.permutation(a.windows))
    n_batches = a.windows // a.batch
    for name, kw, padded in FORMS:
        store = DeviceTileStore(padded_windows if padded else windows, targets, 2.0, 28.0).set_filters(**kw)
        store.padded = padded
        dev = store.device_indices(perm)
        out = (torch.empty((a.batch, 20, 1, 224), device='cuda'), torch.empty((a.batch, 2), device='cuda'))
        stores[name] = (store, dev, out)
        for i in range(3):                                           # warm-up: code objects loaded, allocations made
            store.batch_from_device(dev[i * a.batch:(i + 1) * a.batch], out=out)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):                                # (captures on a side stream of its own: one linear chain)
            for i in range(a.calls):
                s = (i % n_batches) * a.batch
                store._gather(dev[s:s + a.batch], out[0])
        graph.replay()
        torch.cuda.synchronize()
        graphs[name] = graph
    host = {f[0]: [] for f in FORMS}
    kern = {f[0]: [] for f in FORMS}
    for _ in range(a.rounds):
        for name in host:
            store, dev, out = stores[name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(a.calls):
                s = (i % n_batches) * a.batch
                store.batch_from_device(dev[s:s + a.batch], out=out)
            torch.cuda.synchronize()
            host[name].append(1e6 * (time.perf_counter() - t0) / a.calls)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            graphs[name].replay()
            e1.record()
            e1.synchronize()
            kern[name].append(1e3 * e0.elapsed_time(e1) / a.calls)
    lines = []
    for name in host:
        med = lambda v: round(statistics.median(v), 2)
        rec = dict(form=name, batch=a.batch, calls=a.calls, rounds=a.rounds,
                   us_per_batch=med(host[name]), us_per_batch_min=round(min(host[name]), 2), us_per_batch_max=round(max(host[name]), 2),
                   us_per_gather=med(kern[name]), us_per_gather_min=round(min(kern[name]), 2), us_per_gather_max=round(max(kern[name]), 2),
                   us_per_gather_over_plain=round(statistics.median(kern[name]) - statistics.median(kern['plain']), 2))
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
