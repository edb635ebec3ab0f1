"""Cost of the per-breath losses in the captured training step (reported, not gated; bench.py measures the flagship):

    python scripts/bench_losses.py [--batch 64] [--steps 200] [--rounds 5] [--out FILE.json]

cnn_single_breath_linear + resnet18 and cnn_lstm + densenet18 at B windows of (20, 1, 224), graph replay, each with bce
(the path of the commit before the losses existed: per-breath BCE kernel behind the model's forward), vacillating (alpha 2)
and confidence (beta 1).  Per configuration: two warm steps (the eager one and the capture), then ``rounds`` windows of
``steps`` replays timed with device events, the configurations ALTERNATING round by round so that drift of a shared
machine lands on all of them; the median round and the spread are printed, one JSON line per configuration.  No GPU, no
number: the script fails."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_losses needs an MI355X: there is no CPU timing')
    import deepards_amd.models as M
    from deepards_amd.train import HotPathTrainer
    from oracle.weights import seeded_batch
    x, t = seeded_batch(a.batch, 20, 0)
    x, t = torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda()
    nets = {'cnn_single_breath_linear+resnet18': lambda: M.CNNSingleBreathLinearNetwork(M.resnet18()),
            'cnn_lstm+densenet18': lambda: M.CNNLSTMNetwork(M.densenet18(), 0, False, 16)}
    losses = (('bce', None), ('vacillating', 2.0), ('confidence', 1.0))
    trainers = {}
    for net, mk in nets.items():
        for loss, param in losses:
            torch.manual_seed(0)
            tr = HotPathTrainer(mk().cuda().train(), use_graph=True, loss=loss, loss_param=param)
            for _ in range(3):                                   # eager step, capture + replay, replay
                tr.train_step(x, t)
            trainers[(net, loss)] = tr
    torch.cuda.synchronize()
    times = {k: [] for k in trainers}
    for _ in range(a.rounds):
        for key, tr in trainers.items():
            static = tr.static_batch()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                tr.train_step(static[0], static[1])
            e1.record()
            e1.synchronize()
            times[key].append(e0.elapsed_time(e1) / a.steps)
    lines = []
    for (net, loss), ts in times.items():
        base = statistics.median(times[(net, 'bce')])
        rec = dict(network=net, loss=loss, batch=a.batch, steps=a.steps, rounds=a.rounds, ms_per_step_median=round(statistics.median(ts), 4),
                   ms_per_step_min=round(min(ts), 4), ms_per_step_max=round(max(ts), 4),
                   us_over_bce=round(1000 * (statistics.median(ts) - base), 1), final_loss=float(trainers[(net, loss)].last_loss))
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    for tr in trainers.values():
        tr.release_graphs()


if __name__ == '__main__':
    main()
