"""Cost of the vgg11 backbone in the captured training step (reported, not gated; bench.py measures the flagship):

    python scripts/bench_vgg.py [--batch 64] [--steps 30] [--rounds 7] [--out FILE.json]

1. cnn_linear + vgg11 and cnn_linear + resnet18 at B windows of (20, 1, 224), graph replay, in ONE process: two warm steps
   each (the eager one and the capture), then ``rounds`` windows of ``steps`` replays timed with device events, the two
   networks ALTERNATING round by round so that drift of a shared machine lands on both; the median round, the spread and
   the ratio to resnet18 are printed.
2. The two pool kernels alone at the five pooled stage shapes of that batch -- bn_relu_maxpool2_fwd (reads y, writes half as
   much) and bn_relu_maxpool2_bwd (two passes over y and dout, writes dy) -- each captured in a graph and replayed the same
   way, with the bytes they must move and the rate that makes, as a fraction of the 8 TB/s HBM peak.
One JSON line per measurement.  No GPU, no number: the script fails."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed_rounds(runners, steps, rounds):
    """runners: name -> callable running ONE step; -> name -> [ms per step of every round], the runners alternating."""
    times = {k: [] for k in runners}
    for _ in range(rounds):
        for key, fn in runners.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                fn()
            e1.record()
            e1.synchronize()
            times[key].append(e0.elapsed_time(e1) / steps)
    return times


def captured(fn):
    """fn() captured in a graph after a warm-up on a side stream -> the replay callable (and the graph, kept alive)."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        keep = fn()
    return g.replay, (g, keep)


HBM_PEAK = 8e12                    # bytes / s


def pool_runners(rows, R, l, c):
    from deepards_amd import hip_ops as H
    torch.manual_seed(c)
    y = torch.randn(rows, l, c, device='cuda')
    dout = torch.randn(rows, l // 2, c, device='cuda')
    gamma, beta = torch.rand(c, device='cuda') + 0.5, torch.randn(c, device='cuda') * 0.1
    mean, invstd = H.vgg_stats(y, R)
    out, dy = torch.empty_like(dout), torch.empty_like(y)
    return {'fwd': captured(lambda: H.bn_relu_maxpool2_fwd(y, R, mean, invstd, gamma, beta, out=out)),
            'bwd': captured(lambda: H.bn_relu_maxpool2_bwd(dout, y, R, mean, invstd, gamma, beta, out=dy))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_vgg needs an MI355X: there is no CPU timing')
    import deepards_amd.models as M
    from deepards_amd.train import HotPathTrainer
    from oracle.weights import seeded_batch
    x, t = seeded_batch(a.batch, 20, 0)
    x, t = torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda()
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    trainers = {}
    for name, mk in (('resnet18', M.resnet18), ('vgg11', M.vgg11_bn)):
        torch.manual_seed(0)
        tr = HotPathTrainer(M.CNNLinearNetwork(mk(), 20, 0).cuda().train(), use_graph=True)
        for _ in range(3):                                   # eager step, capture + replay, replay
            tr.train_step(x, t)
        trainers[name] = tr
    torch.cuda.synchronize()
    statics = {k: tr.static_batch() for k, tr in trainers.items()}
    times = timed_rounds({k: (lambda tr=tr, s=statics[k]: tr.train_step(s[0], s[1])) for k, tr in trainers.items()}, a.steps, a.rounds)
    base = statistics.median(times['resnet18'])
    for name, ts in times.items():
        emit(dict(what='train_step', network='cnn_linear+' + name, batch=a.batch, steps=a.steps, rounds=a.rounds,
                  ms_per_step_median=round(statistics.median(ts), 4), ms_per_step_min=round(min(ts), 4),
                  ms_per_step_max=round(max(ts), 4), ratio_to_resnet18=round(statistics.median(ts) / base, 4),
                  final_loss=float(trainers[name].last_loss.detach())))
    for tr in trainers.values():
        tr.release_graphs()
    rows = a.batch * 20
    for l, c in ((224, 64), (112, 128), (56, 256), (28, 512), (14, 512)):
        pairs = pool_runners(rows, 20, l, c)
        ts = timed_rounds({k: v[0] for k, v in pairs.items()}, a.steps, a.rounds)
        full = rows * l * c * 4
        for k, nbytes in (('fwd', full * 3 // 2), ('bwd', full * 4)):       # bwd: (y + dout) twice, dy once
            med = statistics.median(ts[k])
            emit(dict(what='bn_relu_maxpool2_' + k, rows=rows, L=l, C=c, steps=a.steps, rounds=a.rounds, us_median=round(1000 * med, 1),
                      us_min=round(1000 * min(ts[k]), 1), us_max=round(1000 * max(ts[k]), 1), mbytes=round(nbytes / 1e6, 1),
                      tbytes_per_s=round(nbytes / (med * 1e-3) / 1e12, 3), of_hbm_peak=round(nbytes / (med * 1e-3) / HBM_PEAK, 3)))
        del pairs
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
