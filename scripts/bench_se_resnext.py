"""Cost of the se_resnext50_32x4d backbone and of the grouped k3 kernels (reported, not gated; bench.py measures the flagship):

    python scripts/bench_se_resnext.py [--batches 16,64] [--steps 20] [--rounds 7] [--out FILE.json] [--skip-steps]

1. cnn_linear + se_resnext50_32x4d beside cnn_linear + se_resnet50 at B windows of (20, 1, 224) in ONE process: the captured
   step (graph replay) of both, ``rounds`` windows of ``steps`` steps timed with device events, the runners ALTERNATING round
   by round so that drift of a shared machine lands on both; median round, spread, ratio to se_resnet50.
2. Each kernel of csrc/conv_grouped.hip alone (forward, data gradient, weight gradient) at conv2's shapes in the four stages
   at the largest batch -- (L, C, stride) = (56, 128, 1), (56, 256, 2), (28, 256, 1), (28, 512, 2), (14, 512, 1), (14, 1024, 2),
   (7, 1024, 1) -- captured in a graph and replayed the same way.  In the SAME run, alternating with it: a float4 copy
   (``y.copy_(x)``, as scripts/bw_probe.py measures it) that moves the kernel's bytes (its maps read once, written once) -- the
   kernel's bound --, and stock ``torch.nn.functional.conv1d(groups=32)`` forward / ``aten.convolution_backward`` on the same
   operands in torch's (N, C, L) layout, the route the reference takes (eager launches, the same event timing).  Each kernel's
   time is reported as a ratio to the copy and to stock torch.
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

STAGES = ((56, 128, 1), (56, 256, 2), (28, 256, 1), (28, 512, 2), (14, 512, 1), (14, 1024, 2), (7, 1024, 1))


def med(ts):
    return statistics.median(ts)


def stage_runners(rows, l, c, stride):
    """name -> (callable, graph-capturable) for the three kernels, the copies of their bytes and stock torch."""
    from deepards_amd import hip_ops as H
    torch.manual_seed(c + stride)
    lo = (l - 1) // stride + 1
    x, dy = torch.randn(rows, l, c, device='cuda'), torch.randn(rows, lo, c, device='cuda')
    w = torch.randn(c, c // 32, 3, device='cuda') / (3 * c // 32) ** 0.5
    y, dx, dw = torch.empty_like(dy), torch.empty_like(x), torch.empty_like(w)
    n = (x.numel() + dy.numel()) // 2                                   # a copy of n floats moves the bytes of both maps
    src, dst = torch.randn(n, device='cuda'), torch.empty(n, device='cuda')
    xn, dyn = x.permute(0, 2, 1).contiguous(), dy.permute(0, 2, 1).contiguous()    # torch's own layout: no transposes timed
    conv_bwd = torch.ops.aten.convolution_backward
    run = {'fwd': (lambda: H.gconv3_fwd(x, w, stride, out=y), True),
           'dgrad': (lambda: H.gconv3_dgrad(dy, w, stride, l, out=dx), True),
           'wgrad': (lambda: H.gconv3_wgrad(dy, x, stride, out=dw), True),
           'copy': (lambda: dst.copy_(src), True),
           'torch_fwd': (lambda: torch.nn.functional.conv1d(xn, w, stride=stride, padding=1, groups=32), False),
           'torch_bwd': (lambda: conv_bwd(dyn, xn, w, None, [stride], [1], [1], False, [0], 32, [True, True, False]), False)}
    return run, 4 * (x.numel() + dy.numel())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='16,64')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out')
    ap.add_argument('--skip-steps', action='store_true', help='kernels only')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_se_resnext needs an MI355X: there is no CPU timing')
    batches = [int(b) for b in a.batches.split(',')]
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    if not a.skip_steps:
        import deepards_amd.models as M
        from deepards_amd.train import HotPathTrainer
        from oracle.weights import seeded_batch
        for batch in batches:
            x, t = seeded_batch(batch, 20, 0)
            x, t = torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda()
            trainers = {}
            for name, mk in (('se_resnet50', M.se_resnet50), ('se_resnext50_32x4d', M.se_resnext50_32x4d)):
                torch.manual_seed(0)
                tr = HotPathTrainer(M.CNNLinearNetwork(mk(), 20, 0).cuda().train(), use_graph=True)
                for _ in range(3):                                   # eager step, capture + replay, replay
                    tr.train_step(x, t)
                trainers[name] = tr
            torch.cuda.synchronize()
            runners = {}
            for k, tr in trainers.items():
                sx, st = tr.static_batch()
                runners[k] = (lambda tr=tr, sx=sx, st=st: tr.train_step(sx, st))
            times = timed_rounds(runners, a.steps, a.rounds)
            base = med(times['se_resnet50'])
            for name, ts in times.items():
                emit(dict(what='train_step', network='cnn_linear+' + name, batch=batch, steps=a.steps, rounds=a.rounds,
                          ms_per_step_median=round(med(ts), 4), ms_per_step_min=round(min(ts), 4), ms_per_step_max=round(max(ts), 4),
                          ratio_to_se_resnet50=round(med(ts) / base, 4), final_loss=float(trainers[name].last_loss)))
            for tr in trainers.values():
                tr.release_graphs()
            del trainers, runners
            torch.cuda.empty_cache()
    rows = max(batches) * 20
    for l, c, stride in STAGES:
        run, nbytes = stage_runners(rows, l, c, stride)
        keep, fns = [], {}
        for k, (fn, graph) in run.items():
            if graph:
                fns[k], kept = captured(fn)
                keep.append(kept)
            else:
                for _ in range(3):                                      # (the library picks and compiles its kernel here)
                    fn()
                fns[k] = fn
        torch.cuda.synchronize()
        ts = {k: [1000 * v for v in vs] for k, vs in timed_rounds(fns, a.steps, a.rounds).items()}      # us
        copy_us = med(ts['copy'])
        stock = {'fwd': med(ts['torch_fwd']), 'dgrad+wgrad': med(ts['torch_bwd'])}
        emit(dict(what='gconv3_reference', rows=rows, L=l, C=c, stride=stride, mbytes=round(nbytes / 1e6, 2), copy_us_median=round(copy_us, 1),
                  copy_tbytes_per_s=round(nbytes / copy_us / 1e6, 2), torch_fwd_us_median=round(stock['fwd'], 1),
                  torch_bwd_us_median=round(stock['dgrad+wgrad'], 1)))
        for k in ('fwd', 'dgrad', 'wgrad'):
            us = med(ts[k])
            emit(dict(what='gconv3_kernel', kernel=k, rows=rows, L=l, C=c, stride=stride, us_median=round(us, 1), us_min=round(min(ts[k]), 1),
                      us_max=round(max(ts[k]), 1), tbytes_per_s=round(nbytes / us / 1e6, 2), ratio_to_copy=round(us / copy_us, 2),
                      gflop=round(2 * 3 * (c // 32) * rows * ((l - 1) // stride + 1) * c / 1e9, 3)))
        bwd = med(ts['dgrad']) + med(ts['wgrad'])
        emit(dict(what='gconv3_vs_torch', rows=rows, L=l, C=c, stride=stride, fwd_ratio_to_torch=round(med(ts['fwd']) / stock['fwd'], 2),
                  bwd_ratio_to_torch=round(bwd / stock['dgrad+wgrad'], 2)))
        del run, fns, keep
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
