"""Cost of the lstm_only step and of its waveform-LSTM kernels (reported, not gated; bench.py measures the flagship):

    python scripts/bench_lstm_only.py [--shapes 64x20,16x20,16x100] [--hidden 16] [--rounds 7] [--reps 10] [--out FILE.json]

At (B, NB) windows of (NB, 1, 224), N = B NB sequences of T = 224 steps, in ONE process, every runner a captured graph
replayed between device events (the launches' host cost stays out), the runners ALTERNATING round by round so that drift of a
shared machine lands on all; medians over the rounds, with the spread (min, max):

  step_lstm_only   ``HotPathTrainer.train_step`` of LSTMOnlyNetwork (SGD; forward, bce, backward, update)
  rec_hip          the recurrence alone, forward and backward: da_lstm_seq_fwd + da_lstm_seq_bwd (with its folds)
  rec_existing     the same recurrence through the cnn_lstm head's kernels: gx (N, T, 4H) = x (outer) w_ih built by one
                   broadcast multiply, da_lstm_fwd, da_lstm_bwd, the da_reduce_rows folds of dw_hh and db and the dw_ih
                   product (one multiply-sum) -- what the lstm_only networks would cost without kernels of their own
  head_hip         recurrence + breath projection Linear(224 H -> 16), forward and backward, through the autograd Functions
  head_torch       stock ``torch.nn.LSTM`` + ``nn.Linear`` on the same GPU, forward and backward; ``captured: false``: the
                   BLAS library under them refuses a graph capture, so this one runner is timed eagerly between the same
                   device events, ``reps`` calls queued back to back
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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='64x20,16x20,16x100')
    ap.add_argument('--hidden', type=int, default=16)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('bench_lstm_only.py measures on the GPU: none here')
    import deepards_amd.models as M
    from deepards_amd import hip_ops as H, lstm_seq_ops as S
    from deepards_amd.train import HotPathTrainer
    hd, t_len, feat, lines = args.hidden, 224, 16, []
    for shape in args.shapes.split(','):
        batch, nb = [int(v) for v in shape.split('x')]
        n = batch * nb
        torch.manual_seed(0)
        x = torch.randn(batch, nb, 1, t_len, device='cuda')
        tgt = torch.eye(2, device='cuda')[torch.arange(batch, device='cuda') % 2].contiguous()
        model = M.LSTMOnlyNetwork(hd, nb).cuda()
        lstm, lin = model.lstm_breath_block, model.linear_breath_inst
        tr = HotPathTrainer(model, use_graph=True)
        for _ in range(3):
            tr.train_step(x, tgt)
        sx, st = tr.static_batch(batch)
        step = lambda: tr.train_step(sx, st)
        rows = x.view(n, t_len).contiguous()
        ws = [p.detach().clone() for p in (lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0)]
        dhs = torch.randn(n, t_len, hd, device='cuda')
        dy = torch.randn(n, feat, device='cuda')

        def rec_hip():
            hs, cs, lens = S.lstm_seq_fwd(rows, *ws)
            return S.lstm_seq_bwd(dhs, rows, *ws, hs, cs, lens)

        def rec_existing():
            gx = rows.unsqueeze(-1) * ws[0].view(1, 1, -1)                       # the outer product, materialised
            hs, cs, gates, _, _ = H.lstm_fwd(gx, ws[1], ws[2], ws[3])
            dgates, part = H.lstm_bwd(dhs, ws[1], hs, cs, gates)
            dw_hh, db = H.reduce_rows(part), H.reduce_rows(dgates.view(n * t_len, 4 * hd))
            dw_ih = (dgates * rows.unsqueeze(-1)).sum(dim=(0, 1))
            return dw_ih, dw_hh, db
        hw = [w.clone().requires_grad_(True) for w in ws] + [lin.weight.detach().clone().requires_grad_(True),
                                                            lin.bias.detach().clone().requires_grad_(True)]

        def head_hip():
            hs = S.WaveformLSTMFunction.apply(rows, hw[0], hw[1], hw[2], hw[3], False)
            y = S.BreathProjectionFunction.apply(hs.view(n, -1), hw[4], hw[5])
            y.backward(dy)
            return y
        t_lstm = torch.nn.LSTM(1, hd, batch_first=True).cuda()
        t_lin = torch.nn.Linear(hd * t_len, feat).cuda()
        x3 = rows.unsqueeze(-1).contiguous()

        def head_torch():
            y = t_lin(t_lstm(x3)[0].reshape(n, -1))
            y.backward(dy)
            return y
        runners = {'step_lstm_only': (step, args.reps, 1)}
        for name, fn in (('rec_hip', rec_hip), ('rec_existing', rec_existing), ('head_hip', head_hip)):
            runners[name] = (captured(fn, args.reps), 1, args.reps)
        runners['head_torch'] = (head_torch, args.reps, 1)         # eager: the BLAS library under nn.LSTM / nn.Linear refuses a capture
        for fn, calls, _ in runners.values():
            events_ms(fn, 2)
        times = {k: [] for k in runners}
        for _ in range(args.rounds):
            for k, (fn, calls, per) in runners.items():
                times[k].append(events_ms(fn, calls) / per)
        med = {k: statistics.median(v) for k, v in times.items()}
        for k, v in times.items():
            rec = dict(bench='lstm_only', batch=batch, nb=nb, n=n, t=t_len, hidden=hd, runner=k, ms_median=round(med[k], 4),
                       ms_min=round(min(v), 4), ms_max=round(max(v), 4), rounds=args.rounds, reps=args.reps)
            if k == 'head_torch':
                rec['captured'] = False
            if k == 'rec_hip':
                rec['ratio_to_rec_existing'] = round(med[k] / med['rec_existing'], 3)
            if k == 'head_hip':
                rec['ratio_to_head_torch'] = round(med[k] / med['head_torch'], 3)
            lines.append(rec)
            print(json.dumps(rec), flush=True)
        tr.release_graphs()
        del runners, tr
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            for rec in lines:
                f.write(json.dumps(rec) + '\n')
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
