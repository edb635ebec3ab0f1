"""Cost of the se_resnet18 backbone in the captured training step (reported, not gated; bench.py measures the flagship):

    python scripts/bench_se_resnet.py [--batch 64] [--steps 50] [--rounds 7] [--out FILE.json]

1. cnn_linear + se_resnet18 and cnn_linear + resnet18 at B windows of (20, 1, 224), graph replay, in ONE process: two warm
   steps each (the eager one and the capture), then ``rounds`` windows of ``steps`` replays timed with device events, the two
   networks ALTERNATING round by round so that drift of a shared machine lands on both; the median round, the spread and
   the ratio to resnet18 are printed.
2. The SE tail alone at the four stage shapes of that batch -- forward [statistics -> gate -> scale + residual + ReLU] and
   backward [reduce -> gate -> scale -> bn2's BatchNorm backward] through the HIP kernels, against the same arithmetic from
   stock torch ops (autograd backward), each captured in a graph and replayed the same way.
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


def tail_runners(rows, R, l, c):
    from deepards_amd import hip_ops as H
    torch.manual_seed(c)
    dev = 'cuda'
    cr = c // 4
    y2, res, dout = (torch.randn(rows, l, c, device=dev) for _ in range(3))
    gamma, beta = torch.rand(c, device=dev) + 0.5, torch.randn(c, device=dev) * 0.1
    w1, b1 = torch.randn(cr, c, 1, device=dev) / c ** 0.5, torch.zeros(cr, device=dev)
    w2, b2 = torch.randn(c, cr, 1, device=dev) / cr ** 0.5, torch.zeros(c, device=dev)

    def hip():
        mean, invstd = H.se_stats(y2, R)
        pool, hid, s = H.se_gate_fwd(y2, R, mean, invstd, gamma, beta, w1, b1, w2, b2)
        out, mask = H.se_scale_fwd(y2, R, mean, invstd, gamma, beta, s, res)
        g, dsum = H.se_bwd_reduce(dout, mask, y2, R, mean, invstd, gamma, beta)
        dpool, grads = H.se_gate_bwd(dsum, s, hid, pool, w1, w2)
        dz = H.se_bwd_scale(g, s, dpool)
        dy2 = H.bn_bwd(dz, y2, R, mean, invstd, gamma, beta, 0, dx=dz)
        return out, g, dy2, grads

    leaves = [t.clone().requires_grad_(True) for t in (y2, res, gamma, beta, w1, b1, w2, b2)]

    def stock():
        y, r, ga, be, a1, c1, a2, c2 = leaves
        yw = y.reshape(rows // R, R * l, c)
        var, mean = torch.var_mean(yw, 1, unbiased=False, keepdim=True)
        z = ((yw - mean) * torch.rsqrt(var + 1e-5) * ga + be).reshape(rows, l, c)
        hid = torch.relu(torch.addmm(c1, z.mean(1), a1.reshape(cr, c).t()))
        s = torch.sigmoid(torch.addmm(c2, hid, a2.reshape(c, cr).t()))
        out = torch.relu(z * s[:, None, :] + r)
        return out, torch.autograd.grad(out, leaves, dout)

    return {'hip': captured(hip), 'torch': captured(stock)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_se_resnet needs an MI355X: there is no CPU timing')
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
    for name, mk in (('resnet18', M.resnet18), ('se_resnet18', M.se_resnet18)):
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
                  final_loss=float(trainers[name].last_loss)))
    for tr in trainers.values():
        tr.release_graphs()
    rows = a.batch * 20
    for l, c in ((56, 64), (28, 128), (14, 256), (7, 512)):
        pairs = tail_runners(rows, 20, l, c)
        ts = timed_rounds({k: v[0] for k, v in pairs.items()}, a.steps, a.rounds)
        hip, stock = statistics.median(ts['hip']), statistics.median(ts['torch'])
        emit(dict(what='se_tail_fwd_bwd', rows=rows, L=l, C=c, steps=a.steps, rounds=a.rounds, hip_us_median=round(1000 * hip, 1),
                  hip_us_min=round(1000 * min(ts['hip']), 1), hip_us_max=round(1000 * max(ts['hip']), 1),
                  torch_us_median=round(1000 * stock, 1), torch_us_min=round(1000 * min(ts['torch']), 1),
                  torch_us_max=round(1000 * max(ts['torch']), 1), torch_over_hip=round(stock / hip, 2)))
        del pairs
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
