"""Cost of the se_resnet50 backbone and of the wide SE-tail kernels (reported, not gated; bench.py measures the flagship):

    python scripts/bench_se_bottleneck.py [--batch 64] [--steps 20] [--rounds 7] [--out FILE.json] [--skip-steps]

1. cnn_linear + se_resnet50 / se_resnet18 / resnet18 at B windows of (20, 1, 224) in ONE process: the captured step (graph
   replay) of all three and the eager step of se_resnet50, ``rounds`` windows of ``steps`` steps timed with device events, the
   runners ALTERNATING round by round so that drift of a shared machine lands on all; median round, spread, ratio to resnet18.
2. Each kernel of csrc/se_wide.hip alone at the four stage shapes of that batch -- (L, C, Cr) = (56, 256, 16), (28, 512, 32),
   (14, 1024, 64), (7, 2048, 128) -- captured in a graph and replayed the same way, with the bytes it has to move (operands
   read once, results written once) or the FLOPs of its GEMMs and the rate that makes.
3. Both gate families (csrc/se.hip on the map, csrc/se_wide.hip on the row sums) at the two shapes both take, (256, 16) and
   (512, 32): forward [statistics -> gate] and backward [gate backward], what ``se_ops.se_gate_family`` chooses between.
One JSON line per measurement.  No GPU, no number: the script fails."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_se_resnet import timed_rounds, captured      # noqa: E402

STAGES = ((56, 256, 16), (28, 512, 32), (14, 1024, 64), (7, 2048, 128))


def tail_operands(rows, l, c, cr):
    torch.manual_seed(c)
    dev = 'cuda'
    y, res, dout = (torch.randn(rows, l, c, device=dev) for _ in range(3))
    gamma, beta = torch.rand(c, device=dev) + 0.5, torch.randn(c, device=dev) * 0.1
    w1, b1 = torch.randn(cr, c, 1, device=dev) / c ** 0.5, torch.zeros(cr, device=dev)
    w2, b2 = torch.randn(c, cr, 1, device=dev) / cr ** 0.5, torch.zeros(c, device=dev)
    return y, res, dout, gamma, beta, w1, b1, w2, b2


def kernel_runners(rows, R, l, c, cr):
    """name -> (callable, bytes moved, FLOPs) of every wide kernel on operands the kernels in front of it produced."""
    from deepards_amd import hip_ops as H
    y, res, dout, gamma, beta, w1, b1, w2, b2 = tail_operands(rows, l, c, cr)
    mean, invstd, rowsum = H.se_wide_stats(y, R)
    pool, hid, s = H.se_wide_gate_fwd(rowsum, R, l, mean, invstd, gamma, beta, w1, b1, w2, b2)
    out, mask = H.se_wide_scale_fwd(y, R, mean, invstd, gamma, beta, s, res)
    g, dsum = H.se_wide_bwd_reduce(dout, mask, y, R, mean, invstd, gamma, beta)
    dpool, grads = H.se_wide_gate_bwd(dsum, s, hid, pool, w1, w2)
    m, rc, rcr, wts = 4 * rows * l * c, 4 * rows * c, 4 * rows * cr, 4 * 2 * c * cr
    gemm = 2 * rows * c * cr
    return {
        'stats': (lambda: H.se_wide_stats(y, R), m + 2 * rc, 0),
        'gate_fwd': (lambda: H.se_wide_gate_fwd(rowsum, R, l, mean, invstd, gamma, beta, w1, b1, w2, b2), 3 * rc + rcr + wts, 2 * gemm),
        'scale_fwd': (lambda: H.se_wide_scale_fwd(y, R, mean, invstd, gamma, beta, s, res), 3 * m + m // 32 + rc, 0),
        'bwd_reduce': (lambda: H.se_wide_bwd_reduce(dout, mask, y, R, mean, invstd, gamma, beta), 3 * m + m // 32 + rc, 0),
        'gate_bwd': (lambda: H.se_wide_gate_bwd(dsum, s, hid, pool, w1, w2, grads=grads), 6 * rc + 2 * rcr + 2 * wts, 4 * gemm),
        'bwd_scale': (lambda: H.se_wide_bwd_scale(g, s, dpool), 2 * m + 2 * rc, 0),
    }


def family_runners(rows, R, l, c, cr):
    from deepards_amd import hip_ops as H
    y, res, dout, gamma, beta, w1, b1, w2, b2 = tail_operands(rows, l, c, cr)

    def narrow_fwd():
        mean, invstd = H.se_stats(y, R)
        return H.se_gate_fwd(y, R, mean, invstd, gamma, beta, w1, b1, w2, b2)

    def wide_fwd():
        mean, invstd, rowsum = H.se_wide_stats(y, R)
        return H.se_wide_gate_fwd(rowsum, R, l, mean, invstd, gamma, beta, w1, b1, w2, b2)
    pool, hid, s = wide_fwd()
    dsum = torch.randn(rows, c, device='cuda')
    gn = tuple(torch.empty_like(t) for t in (w1, b1, w2, b2))
    gw = tuple(torch.empty_like(t) for t in (w1, b1, w2, b2))
    return {'narrow_fwd': narrow_fwd, 'wide_fwd': wide_fwd,
            'narrow_bwd': lambda: H.se_gate_bwd(dsum, s, hid, pool, w1, w2, grads=gn),
            'wide_bwd': lambda: H.se_wide_gate_bwd(dsum, s, hid, pool, w1, w2, grads=gw)}


def med(ts):
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out')
    ap.add_argument('--skip-steps', action='store_true', help='kernels and families only')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_se_bottleneck needs an MI355X: there is no CPU timing')
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    if not a.skip_steps:
        import deepards_amd.models as M
        from deepards_amd.train import HotPathTrainer
        from oracle.weights import seeded_batch
        x, t = seeded_batch(a.batch, 20, 0)
        x, t = torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda()
        trainers = {}
        for name, mk, graph in (('resnet18', M.resnet18, True), ('se_resnet18', M.se_resnet18, True), ('se_resnet50', M.se_resnet50, True),
                                ('se_resnet50 eager', M.se_resnet50, False)):
            torch.manual_seed(0)
            tr = HotPathTrainer(M.CNNLinearNetwork(mk(), 20, 0).cuda().train(), use_graph=graph)
            for _ in range(3):                                   # eager step, capture + replay, replay
                tr.train_step(x, t)
            trainers[name] = tr
        torch.cuda.synchronize()
        runners = {}
        for k, tr in trainers.items():
            sx, st = tr.static_batch() if tr.use_graph else (x, t)
            runners[k] = (lambda tr=tr, sx=sx, st=st: tr.train_step(sx, st))
        times = timed_rounds(runners, a.steps, a.rounds)
        base = med(times['resnet18'])
        for name, ts in times.items():
            emit(dict(what='train_step', network='cnn_linear+' + name, batch=a.batch, steps=a.steps, rounds=a.rounds,
                      ms_per_step_median=round(med(ts), 4), ms_per_step_min=round(min(ts), 4), ms_per_step_max=round(max(ts), 4),
                      ratio_to_resnet18=round(med(ts) / base, 4), final_loss=float(trainers[name].last_loss)))
        for tr in trainers.values():
            if tr.use_graph:
                tr.release_graphs()
        del trainers, runners
        torch.cuda.empty_cache()
    rows = a.batch * 20
    for l, c, cr in STAGES:
        ks = kernel_runners(rows, 20, l, c, cr)
        reps = {k: captured(v[0]) for k, v in ks.items()}
        ts = timed_rounds({k: v[0] for k, v in reps.items()}, a.steps, a.rounds)
        for k, (_, nbytes, flops) in ks.items():
            us = 1000 * med(ts[k])
            emit(dict(what='se_wide_kernel', kernel=k, rows=rows, L=l, C=c, Cr=cr, us_median=round(us, 1), us_min=round(1000 * min(ts[k]), 1),
                      us_max=round(1000 * max(ts[k]), 1), mbytes=round(nbytes / 1e6, 2), gbytes_per_s=round(nbytes / us / 1e3, 1),
                      gflop=round(flops / 1e9, 3), tflops=round(flops / us / 1e6, 2)))
        del ks, reps
    for l, c, cr in STAGES[:2]:
        fr = family_runners(rows, 20, l, c, cr)
        reps = {k: captured(v) for k, v in fr.items()}
        ts = timed_rounds({k: v[0] for k, v in reps.items()}, a.steps, a.rounds)
        rec = dict(what='se_gate_families', rows=rows, L=l, C=c, Cr=cr)
        for k in fr:
            rec[k + '_us_median'] = round(1000 * med(ts[k]), 1)
            rec[k + '_us_min'] = round(1000 * min(ts[k]), 1)
            rec[k + '_us_max'] = round(1000 * max(ts[k]), 1)
        rec['narrow_over_wide'] = round((med(ts['narrow_fwd']) + med(ts['narrow_bwd'])) / (med(ts['wide_fwd']) + med(ts['wide_bwd'])), 3)
        emit(rec)
        del fr, reps
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
