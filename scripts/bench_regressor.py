"""Cost of the breath-metadata pretraining step and of its head kernels (reported, not gated; bench.py measures the flagship):

    python scripts/bench_regressor.py [--batches 16,128] [--bases resnet18,densenet18] [--m 9] [--rounds 7] [--reps 5] [--out F.json]

In ONE process, every captured runner a graph replayed between device events (the launches' host cost stays out), the runners
ALTERNATING round by round so that drift of a shared machine lands on all; medians over the rounds, with the spread:

  step           ``RegressorTrainer.train_step`` on (B, 1, 224) breaths, ALL B rows one BatchNorm window (captured replay)
  test_step      ``RegressorTrainer.test_step`` (captured replay, with its two input copies and two output clones)
  torch_step     the same network from stock ``torch.nn`` modules (Conv1d / BatchNorm1d / ... assembled below like the reference's
                 models), MSELoss, autograd backward, torch.optim SGD-Nesterov with the +-clip clamp: eager, and captured where
                 torch's capture takes it (``captured`` says which)
  cnn_linear     for context: ``HotPathTrainer.train_step`` of cnn_linear on the same number of breath rows (B / 8 windows of
                 8 breaths: BatchNorm per window, the single-pass geometry); only where B is a multiple of 16
  head_hip       da_regress_fwd + da_regress_bwd alone on the (B, 7, F) map
  head_torch     the same arithmetic from stock torch ops (mean over the positions, linear, mse_loss, autograd.grad), captured
                 where the capture takes it
  head_copy      a float4 copy of the head's bytes (map read, pooled features written and read, map gradient written): one
                 ``copy_`` of that many floats
One JSON line per measurement.  No GPU, no number: the script fails."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def events_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def captured(fn, reps):
    """``reps`` calls of fn in one graph -> a runner whose call is one replay (its time / reps is one call's device time)."""
    from deepards_amd.train import _capture_graph
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    graph, held = torch.cuda.CUDAGraph(), []
    with _capture_graph(graph):
        for _ in range(reps):
            held.append(fn())
    graph.replay()
    torch.cuda.synchronize()
    graph._held = held
    return graph.replay


def try_captured(fn, reps):
    """(runner, calls per timing, calls per runner call, captured?)"""
    try:
        return captured(fn, reps), 1, reps, True
    except Exception:                                      # noqa: BLE001 -- a library under the stock ops refused the capture
        torch.cuda.synchronize()
        return fn, reps, 1, False


def measure(runners, rounds, tag, lines):
    """runners: {name: (fn, calls per timing, calls per fn, captured?)}."""
    for fn, calls, _, _ in runners.values():
        events_ms(fn, 2)
    times = {k: [] for k in runners}
    for _ in range(rounds):
        for k, (fn, calls, per, _) in runners.items():
            times[k].append(events_ms(fn, calls) / per)
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, v in times.items():
        lines.append(dict(tag, runner=k, ms_median=round(med[k], 4), ms_min=round(min(v), 4), ms_max=round(max(v), 4), rounds=rounds,
                          captured=bool(runners[k][3])))
    return med


# ---- the networks from stock torch.nn modules (the structure of the reference's models/resnet.py and models/densenet.py) ----------
class _StockBasicBlock(nn.Module):
    def __init__(self, cin, planes, stride):
        super(_StockBasicBlock, self).__init__()
        self.conv1, self.bn1 = nn.Conv1d(cin, planes, 3, stride, 1, bias=False), nn.BatchNorm1d(planes)
        self.conv2, self.bn2 = nn.Conv1d(planes, planes, 3, 1, 1, bias=False), nn.BatchNorm1d(planes)
        self.shortcut = None
        if stride != 1 or cin != planes:
            self.shortcut = nn.Sequential(nn.Conv1d(cin, planes, 1, stride, bias=False), nn.BatchNorm1d(planes))

    def forward(self, x):
        out = self.bn2(self.conv2(torch.relu(self.bn1(self.conv1(x)))))
        return torch.relu(out + (x if self.shortcut is None else self.shortcut(x)))


def stock_resnet18():
    layers, cin = [nn.Conv1d(1, 64, 7, 2, 3, bias=False), nn.BatchNorm1d(64), nn.ReLU(inplace=True), nn.MaxPool1d(3, 2, 1)], 64
    for i, planes in enumerate((64, 128, 256, 512)):
        for b in range(2):
            layers.append(_StockBasicBlock(cin, planes, 2 if (i > 0 and b == 0) else 1))
            cin = planes
    return nn.Sequential(*layers, nn.AvgPool1d(7, stride=1), nn.Flatten()), 512


class _StockDenseLayer(nn.Module):
    def __init__(self, cin, growth, bn_size, drop):
        super(_StockDenseLayer, self).__init__()
        bn = lambda c: nn.BatchNorm1d(c, track_running_stats=False)
        self.body = nn.Sequential(bn(cin), nn.ReLU(inplace=True), nn.Conv1d(cin, bn_size * growth, 1, bias=False), bn(bn_size * growth),
                                  nn.ReLU(inplace=True), nn.Conv1d(bn_size * growth, growth, 3, 1, 1, bias=False), nn.Dropout(drop))

    def forward(self, x):
        return torch.cat([x, self.body(x)], dim=1)


def stock_densenet18(growth=32, bn_size=4, drop=0.2):
    bn = lambda c: nn.BatchNorm1d(c, track_running_stats=False)
    layers, c = [nn.Conv1d(1, 64, 7, 2, 3, bias=False), bn(64), nn.ReLU(inplace=True), nn.MaxPool1d(3, 2, 1)], 64
    for i in range(4):
        for _ in range(2):
            layers.append(_StockDenseLayer(c, growth, bn_size, drop))
            c += growth
        if i < 3:
            layers += [bn(c), nn.ReLU(inplace=True), nn.Conv1d(c, c // 2, 1, bias=False), nn.AvgPool1d(2, 2)]
            c //= 2
    return nn.Sequential(*layers, bn(c), nn.ReLU(inplace=True), nn.AvgPool1d(7, stride=1), nn.Flatten()), c


class StockRegressor(nn.Module):
    def __init__(self, base, m):
        super(StockRegressor, self).__init__()
        self.breath_block, width = stock_resnet18() if base == 'resnet18' else stock_densenet18()
        self.linear_final = nn.Linear(width, m)

    def forward(self, x):
        return self.linear_final(self.breath_block(x))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='16,128')
    ap.add_argument('--bases', default='resnet18,densenet18')
    ap.add_argument('--m', type=int, default=9)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('bench_regressor.py measures on the GPU: none here')
    import deepards_amd.models as M
    from deepards_amd import regress_ops as RO
    from deepards_amd.regressor import RegressorTrainer
    from deepards_amd.train import HotPathTrainer
    m, lines = args.m, []
    batches = [int(v) for v in args.batches.split(',')]
    crit = nn.MSELoss()
    for base in args.bases.split(','):
        for batch in batches:
            torch.manual_seed(0)
            x, t = torch.randn(batch, 1, 224, device='cuda'), torch.randn(batch, m, device='cuda')
            runners, trainers = {}, []
            model = M.CNNRegressor(M.base_networks[base](), m).cuda()
            assert model.breath_block.n_out_filters == StockRegressor(base, m).linear_final.in_features
            tr = RegressorTrainer(model, use_graph=True)
            for _ in range(3):
                tr.train_step(x, t)
            sx, st = tr.static_batch(batch)
            runners['step'] = ((lambda tr=tr, sx=sx, st=st: tr.train_step(sx, st)), args.reps, 1, True)
            tr.test_step(x, t)
            runners['test_step'] = ((lambda tr=tr: tr.test_step(x, t)), args.reps, 1, True)
            trainers.append(tr)
            stock = StockRegressor(base, m).cuda().train()
            opt = torch.optim.SGD(stock.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4, nesterov=True)

            def torch_step(stock=stock, opt=opt):
                opt.zero_grad(set_to_none=False)
                loss = crit(stock(x), t)
                loss.backward()
                for p in stock.parameters():
                    p.grad.clamp_(-0.01, 0.01)
                opt.step()
                return loss
            runners['torch_step_eager'] = (torch_step, args.reps, 1, False)
            stock2 = StockRegressor(base, m).cuda().train()
            opt2 = torch.optim.SGD(stock2.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4, nesterov=True)
            cap = try_captured(lambda: torch_step(stock2, opt2), args.reps)
            if cap[3]:
                runners['torch_step_captured'] = cap
            if batch % 16 == 0:
                clf = HotPathTrainer(M.CNNLinearNetwork(M.base_networks[base](), 8, 0).cuda(), use_graph=True)
                xw = torch.randn(batch // 8, 8, 1, 224, device='cuda')
                tw = torch.zeros(batch // 8, 2, device='cuda')
                tw[:, 0] = 1.0
                for _ in range(3):
                    clf.train_step(xw, tw)
                cx, ct = clf.static_batch(batch // 8)
                runners['cnn_linear'] = ((lambda clf=clf, cx=cx, ct=ct: clf.train_step(cx, ct)), args.reps, 1, True)
                trainers.append(clf)
            med = measure(runners, args.rounds, dict(bench='regressor_step', base=base, batch=batch, m=m), lines)
            for rec in lines[-len(runners):]:
                if rec['runner'] != 'step':
                    rec['ratio_to_step'] = round(med[rec['runner']] / med['step'], 3)
                print(json.dumps(rec), flush=True)
            for tr in trainers:
                tr.release_graphs()
            del runners, trainers, stock, stock2
    for f in (512, 128):
        for batch in batches:
            torch.manual_seed(1)
            xmap = torch.relu(torch.randn(batch, 7, f, device='cuda'))
            w, b = torch.randn(m, f, device='cuda') / f ** 0.5, torch.randn(m, device='cuda')
            t = torch.randn(batch, m, device='cuda')
            work = torch.empty(max(RO.regress_workspace(batch, f, m) // 4, 1), device='cuda')

            def head_hip():
                feat, out, loss = RO.regress_fwd(xmap, w, b, t)
                return RO.regress_bwd(feat, w, out, t, RO.MAP, workspace=work), loss
            leaves = [v.clone().requires_grad_(True) for v in (xmap, w, b)]

            def head_torch():
                loss = torch.nn.functional.mse_loss(torch.nn.functional.linear(leaves[0].mean(dim=1), leaves[1], leaves[2]), t)
                return torch.autograd.grad(loss, leaves), loss
            n_copy = (2 * 7 * batch * f + 2 * batch * f) // 2           # floats moved one way by a copy_ of this many
            src, dst = torch.randn(n_copy, device='cuda'), torch.empty(n_copy, device='cuda')
            runners = {'head_hip': (captured(head_hip, args.reps), 1, args.reps, True), 'head_torch': try_captured(head_torch, args.reps),
                       'head_copy': (captured(lambda: dst.copy_(src), args.reps), 1, args.reps, True)}
            med = measure(runners, args.rounds, dict(bench='regressor_head', f=f, batch=batch, m=m), lines)
            for rec in lines[-len(runners):]:
                if rec['runner'] == 'head_hip':
                    rec['ratio_to_torch'] = round(med['head_hip'] / med['head_torch'], 3)
                    rec['ratio_to_copy'] = round(med['head_hip'] / med['head_copy'], 3)
                    rec['traffic_mb'] = round(2 * n_copy * 4 / 1e6, 3)
                print(json.dumps(rec), flush=True)
            del runners
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + '\n')
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
