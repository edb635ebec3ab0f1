"""Cost of the siamese pretraining step and of its head kernels (reported, not gated; bench.py measures the flagship):

    python scripts/bench_siamese.py [--batches 16,64] [--nb 20] [--bases resnet18,densenet18] [--rounds 7] [--reps 5] [--out F.json]

In ONE process, every captured runner a graph replayed between device events (the launches' host cost stays out), the runners
ALTERNATING round by round so that drift of a shared machine lands on all; medians over the rounds, with the spread:

  step_literal   ``SiameseTrainer.train_step`` on [anchor | pos | anchor | neg] (4 B windows: the reference's four tower passes)
  step_shared    the same on [anchor | pos | neg] (3 B windows, share_anchor=True); expectation: about 3/4 of step_literal
  eager_compose  ``model(seq, pos)``, ``model(seq, neg)``, stock BCEWithLogitsLoss, autograd backward -- no optimiser, eager (the
                 composition a user would write without forward_triplet); ``captured: false``; densenet18 with dropout OFF (two
                 forwards in front of one backward cannot share the in-place dropout seed)
  head_hip       da_siamese_head_fwd + da_siamese_head_bwd at D = 512 and D = 16 (B NB rows), shared and separate anchor
  head_torch     the same arithmetic from stock torch ops (abs, linear, binary_cross_entropy_with_logits, autograd backward),
                 captured too where the graph capture takes it (``captured`` says which)
One JSON line per measurement.  No GPU, no number: the script fails."""
import argparse
import json
import os
import statistics
import sys

import torch

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
        rec = dict(tag, runner=k, ms_median=round(med[k], 4), ms_min=round(min(v), 4), ms_max=round(max(v), 4), rounds=rounds,
                   captured=bool(runners[k][3]))
        lines.append(rec)
    return med


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='16,64')
    ap.add_argument('--nb', type=int, default=20)
    ap.add_argument('--bases', default='resnet18,densenet18')
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('bench_siamese.py measures on the GPU: none here')
    import deepards_amd.models as M
    from deepards_amd import siamese_ops as SO
    from deepards_amd.siamese import SiameseTrainer
    nb, lines = args.nb, []
    crit = torch.nn.BCEWithLogitsLoss()
    for base in args.bases.split(','):
        for batch in [int(v) for v in args.batches.split(',')]:
            torch.manual_seed(0)
            seq, pos, neg = (torch.randn(batch, nb, 1, 224, device='cuda') for _ in range(3))
            t_pos = torch.tensor([[0.0, 1.0]], device='cuda').repeat(batch, 1)
            t_neg = torch.tensor([[1.0, 0.0]], device='cuda').repeat(batch, 1)
            runners, trainers = {}, []
            for name, share in (('step_literal', False), ('step_shared', True)):
                tr = SiameseTrainer(M.SiameseCNNLinearNetwork(M.base_networks[base](), nb).cuda(), share_anchor=share, use_graph=True)
                x = torch.cat([seq, pos, neg] if share else [seq, pos, seq, neg], dim=0)
                for _ in range(3):
                    tr.train_step(x)
                sx = tr.static_batch(x.shape[0])[0]
                runners[name] = ((lambda tr=tr, sx=sx: tr.train_step(sx)), args.reps, 1, True)
                trainers.append(tr)
            # (a DenseNet's dropout seed is bumped in place by every forward and saved for its backward: two calls in front of
            # one backward need dropout off -- the eager composition is timed without the dropout kernels' work)
            eager_bb = M.densenet18(drop_rate=0) if base == 'densenet18' else M.base_networks[base]()
            eager_model = M.SiameseCNNLinearNetwork(eager_bb, nb).cuda().train()

            def eager_compose():
                for p in eager_model.parameters():
                    p.grad = None
                loss = crit(eager_model(seq, pos), t_pos) + crit(eager_model(seq, neg), t_neg)
                loss.backward()
                return loss
            runners['eager_compose'] = (eager_compose, args.reps, 1, False)
            med = measure(runners, args.rounds, dict(bench='siamese_step', base=base, batch=batch, nb=nb), lines)
            for rec in lines[-len(runners):]:
                if rec['runner'] != 'step_literal':
                    rec['ratio_to_step_literal'] = round(med[rec['runner']] / med['step_literal'], 3)
                print(json.dumps(rec), flush=True)
            for tr in trainers:
                tr.release_graphs()
            del runners, trainers, eager_model
    for d in (512, 16):
        for batch in [int(v) for v in args.batches.split(',')]:
            rows = batch * nb
            torch.manual_seed(1)
            feats = torch.randn(4 * rows, d, device='cuda')
            w1, b1 = torch.randn(2, d, device='cuda') / d ** 0.5, torch.randn(2, device='cuda')
            w2, b2 = torch.randn(2, 2 * nb, device='cuda') / (2 * nb) ** 0.5, torch.randn(2, device='cuda')
            t_pos = torch.tensor([[0.0, 1.0]], device='cuda').repeat(batch, 1)
            t_neg = torch.tensor([[1.0, 0.0]], device='cuda').repeat(batch, 1)
            runners = {}
            for share in (False, True):
                ops = SO.triplet_slices(feats if not share else feats[:3 * rows], batch, nb, not share)

                def head_hip(ops=ops):
                    u, z, loss = SO.siamese_head_fwd(*ops, w1, b1, w2, b2, batch, nb)
                    return SO.siamese_head_bwd(*ops, w1, b1, w2, b2, u, z, batch, nb), loss
                leaves = [t.clone().requires_grad_(True) for t in ((feats if not share else feats[:3 * rows]), w1, b1, w2, b2)]

                def head_torch(leaves=leaves, share=share):
                    f, a, c, e, g = leaves
                    fa, fp, fa2, fn = SO.triplet_slices(f, batch, nb, not share)
                    lin = torch.nn.functional.linear
                    zp = lin(lin(torch.abs(fp - fa), a, c).view(batch, -1), e, g)
                    zn = lin(lin(torch.abs(fn - fa2), a, c).view(batch, -1), e, g)
                    loss = crit(zp, t_pos) + crit(zn, t_neg)
                    return torch.autograd.grad(loss, leaves), loss
                tag = 'shared' if share else 'literal'
                runners['head_hip_' + tag] = (captured(head_hip, args.reps), 1, args.reps, True)
                try:
                    runners['head_torch_' + tag] = (captured(head_torch, args.reps), 1, args.reps, True)
                except Exception:                              # noqa: BLE001 -- a library under the stock ops refused the capture
                    torch.cuda.synchronize()
                    runners['head_torch_' + tag] = (head_torch, args.reps, 1, False)
            med = measure(runners, args.rounds, dict(bench='siamese_head', d=d, batch=batch, nb=nb, rows=rows), lines)
            for rec in lines[-len(runners):]:
                if rec['runner'].startswith('head_hip_'):
                    rec['ratio_to_torch'] = round(med[rec['runner']] / med[rec['runner'].replace('hip', 'torch')], 3)
                    k = 3 if rec['runner'].endswith('shared') else 4
                    rec['traffic_mb'] = round(2 * k * rows * d * 4 / 1e6, 3)          # operands read twice + gradients written
                    rec['gb_per_s'] = round(3 * k * rows * d * 4 / 1e6 / med[rec['runner']], 1)
                print(json.dumps(rec), flush=True)
            del runners
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            for rec in lines:
                f.write(json.dumps(rec) + '\n')
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
