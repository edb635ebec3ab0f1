"""Cost of the 1-D ProtoPNet step and of its head (reported, not gated; bench.py measures the flagship):

    python scripts/bench_protopnet.py [--batches 16,64] [--rounds 7] [--reps 20] [--out FILE.json]

On densenet18 at B windows of (20, 1, 224), in ONE process, every runner a captured graph replayed ``reps`` times between device
events (the launches' host cost stays out), the runners ALTERNATING round by round so that drift of a shared machine lands on
all; medians over the rounds, with the spread:

  step_joint / step_warm / step_last_layer   ``ProtoPNetTrainer.train_step`` in the three phases (SGD; forward, loss,
                                             the phase's backward, the phase's update)
  step_cnn_linear                            ``HotPathTrainer.train_step`` of cnn_linear + densenet18: the step the project is
                                             measured by, in the same run
  head_hip                                   the head alone, forward and backward, on a fixed (B * 20, 7, 128) map: add-on layers
                                             (GEMM conv + bias / activation kernels), prototype layer, last layer
  head_torch                                 the same arithmetic from stock torch ops in the reference's layout (conv1d, relu,
                                             sigmoid, the expanded-form L2 layer, max_pool1d, log, linear) and autograd
One JSON line per measurement.  No GPU, no number: the script fails."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as Fn

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
    graph._held = held                                       # (the outputs live as long as the graph)
    return graph.replay


def torch_head(h, convs, protos, w_last, g_logits, g_min, b):
    """Forward and backward of the head from stock torch ops, h (rows, C, L)."""
    z = h
    for i, (w, bias) in enumerate(convs):
        z = Fn.conv1d(z, w, bias)
        z = torch.sigmoid(z) if i == len(convs) - 1 else torch.relu(z)
    x2 = Fn.conv1d(z ** 2, torch.ones_like(protos))
    p2 = (protos ** 2).sum(dim=(1, 2)).view(-1, 1)
    dist = torch.relu(x2 + (-2 * Fn.conv1d(z, protos) + p2))
    min_d = (-Fn.max_pool1d(-dist, kernel_size=dist.shape[2])).view(-1, protos.shape[0])
    sim = torch.log((min_d + 1) / (min_d + 1e-4))
    logits = Fn.linear(sim.view(b, -1), w_last)
    torch.autograd.backward([logits, min_d.view(b, -1)], [g_logits, g_min])
    return logits


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='16,64')
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('bench_protopnet.py measures on the GPU: none here')
    import deepards_amd.models as M
    from deepards_amd import functional as F_, protopnet_ops as PO
    from deepards_amd.protopnet import ProtoPNetTrainer
    from deepards_amd.train import HotPathTrainer
    nb, lines = 20, []
    for batch in [int(v) for v in args.batches.split(',')]:
        torch.manual_seed(0)
        x = torch.randn(batch, nb, 1, 224, device='cuda')
        t = torch.eye(2, device='cuda')[torch.arange(batch, device='cuda') % 2].contiguous()
        runners, keep = {}, []
        # the steps: each trainer's own captured graph, fed from its static buffers (no input copies)
        pp = ProtoPNetTrainer(M.construct_PPNet(M.densenet18(), nb).cuda(), use_graph=True)
        cl = HotPathTrainer(M.CNNLinearNetwork(M.densenet18(), nb, 0).cuda(), use_graph=True)
        keep += [pp, cl]
        for _ in range(3):
            cl.train_step(x, t)
        sx, st = cl.static_batch(batch)
        runners['step_cnn_linear'] = lambda sx=sx, st=st: cl.train_step(sx, st)
        for phase in ('joint', 'warm', 'last_layer'):
            pp.set_phase(phase)
            for _ in range(3):
                pp.train_step(x, t)
            px, pt = pp.static_batch(batch)

            def step(phase=phase, px=px, pt=pt):
                if pp.phase != phase:
                    pp.set_phase(phase)
                return pp.train_step(px, pt)
            runners['step_' + phase] = step
        # the head alone on a fixed map
        model = pp.model
        hmap = torch.relu(torch.randn(batch * nb, 7, 128, device='cuda')).requires_grad_(True)
        g_logits = torch.randn(batch, 2, device='cuda')
        g_min = torch.randn(batch, nb * 20, device='cuda') * 0.1
        head_w = [q.detach().clone().requires_grad_(True) for q in
                  list(model.add_on_layers.parameters()) + [model.prototype_vectors, model.last_layer.weight]]

        def head_hip():
            with F_.training_step():                         # (as inside a trainer's step: a conv weight is packed once)
                z = hmap
                for i in (0, 2):
                    z = PO.BiasActFunction.apply(PO.PointwiseConvFunction.apply(z, head_w[i]), head_w[i + 1],
                                                 PO.SIGMOID if i == 2 else PO.RELU)
                sim, min_d = PO.PrototypeLayerFunction.apply(z, head_w[4])
                logits = PO.LastLayerFunction.apply(sim.view(batch, -1), head_w[5])
                torch.autograd.backward([logits, min_d.view(batch, -1)], [g_logits, g_min])
            return logits
        h_ncl = hmap.detach().permute(0, 2, 1).contiguous().requires_grad_(True)
        tw = [q.detach().clone().requires_grad_(True) for q in head_w]

        def head_torch():
            return torch_head(h_ncl, [(tw[0], tw[1]), (tw[2], tw[3])], tw[4], tw[5], g_logits, g_min, batch)
        head_runners = {'head_hip': captured(head_hip, args.reps), 'head_torch': captured(head_torch, args.reps)}
        for fn in runners.values():
            events_ms(fn, 2)
        times = {k: [] for k in list(runners) + list(head_runners)}
        for _ in range(args.rounds):
            for k, fn in runners.items():
                times[k].append(events_ms(fn, args.reps))
            for k, fn in head_runners.items():
                times[k].append(events_ms(fn, 1) / args.reps)
        med = {k: statistics.median(v) for k, v in times.items()}
        for k, v in times.items():
            rec = dict(bench='protopnet', network='densenet18', batch=batch, nb=nb, runner=k, ms_median=round(med[k], 4),
                       ms_min=round(min(v), 4), ms_max=round(max(v), 4), rounds=args.rounds, reps=args.reps)
            if k.startswith('step_') and k != 'step_cnn_linear':
                rec['ratio_to_cnn_linear'] = round(med[k] / med['step_cnn_linear'], 3)
            if k == 'head_hip':
                rec['ratio_to_head_torch'] = round(med[k] / med['head_torch'], 3)
            lines.append(rec)
            print(json.dumps(rec), flush=True)
        pp.release_graphs()
        cl.release_graphs()
        del head_runners, runners, keep
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            for rec in lines:
                f.write(json.dumps(rec) + '\n')
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
