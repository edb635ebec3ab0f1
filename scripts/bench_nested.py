"""Cost of the whole-patient recurrence kernels and of the nested networks' step (reported, not gated; bench.py measures the
flagship):

    python scripts/bench_nested.py [--steps 64,512,2048] [--windows 64,512] [--rounds 7] [--reps 10] [--out FILE.json]

S = 1 sequence, H = 128, T steps, in ONE process; the kernel runners are captured graphs replayed between device events (the
launches' host cost stays out), ALTERNATING round by round so that drift of a shared machine lands on all; medians over the
rounds with the spread (min, max):

  <kind>_fwd / <kind>_bwd   da_seqw_<kind>_fwd / _bwd alone (kind = rnn, lstm); us_per_step = the dependent step's latency
  lstm_fwd_existing         da_lstm_fwd (the cnn_lstm head's kernel, built for many short sequences) at B = 1, H = 128: it reads
                            w_hh from memory on every step.  Forward only: its backward stops at H = 64
  torch_<kind>_fwd / _fwdbwd stock torch.nn.RNN / nn.LSTM on the same GPU; ``captured: false``: the libraries under them refuse
                            a graph capture, so they are timed eagerly, ``reps`` calls queued back to back
  step_<kind>               HotPathTrainer.train_step of CNNToNested<kind>Network on densenet18, NB = 20, W windows, eager (the
                            driver's default: W changes from patient to patient) with the peak memory of the step
One JSON line per measurement.  No GPU, no number: the script fails."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_lstm_only import events_ms, captured                                       # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', default='64,512,2048')
    ap.add_argument('--windows', default='64,512')
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('bench_nested.py measures on the GPU: none here')
    import deepards_amd.models as M
    from deepards_amd import hip_ops as H, seq_wide_ops as SW
    from deepards_amd.train import HotPathTrainer
    hd, lines = SW.HIDDEN, []

    def emit(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    for t in [int(v) for v in args.steps.split(',') if v]:
        torch.manual_seed(0)
        runners = {}
        for kind, g in (('rnn', hd), ('lstm', 4 * hd)):
            mod = (torch.nn.LSTM if kind == 'lstm' else torch.nn.RNN)(hd, hd, batch_first=True).cuda()
            ws = [p.detach().clone() for p in (mod.weight_hh_l0, mod.bias_ih_l0, mod.bias_hh_l0)]
            gx, dhs, x = torch.randn(1, t, g, device='cuda'), torch.randn(1, t, hd, device='cuda'), torch.rand(1, t, hd, device='cuda')
            if kind == 'lstm':
                hs, cs, gates = SW.lstm_fwd(gx, *ws)
                runners['lstm_fwd'] = (captured(lambda gx=gx, ws=ws: SW.lstm_fwd(gx, *ws), args.reps), 1, args.reps, True)
                runners['lstm_bwd'] = (captured(lambda d=dhs, w=ws[0], c=cs, a=gates: SW.lstm_bwd(d, w, c, a), args.reps), 1, args.reps, True)
                runners['lstm_fwd_existing'] = (captured(lambda gx=gx, ws=ws: H.lstm_fwd(gx, *ws), args.reps), 1, args.reps, True)
            else:
                hs = SW.rnn_fwd(gx, *ws)
                runners['rnn_fwd'] = (captured(lambda gx=gx, ws=ws: SW.rnn_fwd(gx, *ws), args.reps), 1, args.reps, True)
                runners['rnn_bwd'] = (captured(lambda d=dhs, w=ws[0], h=hs: SW.rnn_bwd(d, w, h), args.reps), 1, args.reps, True)

            def t_fwd(mod=mod, x=x):
                with torch.no_grad():
                    return mod(x)[0]

            def t_fwdbwd(mod=mod, x=x, dhs=dhs):
                y = mod(x)[0]
                y.backward(dhs)
                return y
            runners['torch_%s_fwd' % kind] = (t_fwd, args.reps, 1, False)
            runners['torch_%s_fwdbwd' % kind] = (t_fwdbwd, args.reps, 1, False)
        for fn, calls, _, _ in runners.values():
            events_ms(fn, 2)
        times = {k: [] for k in runners}
        for _ in range(args.rounds):
            for k, (fn, calls, per, _) in runners.items():
                times[k].append(events_ms(fn, calls) / per)
        for k, v in times.items():
            med = statistics.median(v)
            emit(dict(bench='nested', runner=k, s=1, t=t, hidden=hd, ms_median=round(med, 4), ms_min=round(min(v), 4),
                      ms_max=round(max(v), 4), us_per_step=round(1e3 * med / t, 4), rounds=args.rounds, reps=args.reps,
                      captured=runners[k][3]))
        del runners
    nb = 20
    for w in [int(v) for v in args.windows.split(',') if v]:
        for kind, cls in (('rnn', M.CNNToNestedRNNNetwork), ('lstm', M.CNNToNestedLSTMNetwork)):
            torch.manual_seed(0)
            model = cls(M.densenet18(), nb, True).cuda()
            tr = HotPathTrainer(model, use_graph=False)
            x = torch.randn(1, w, nb, 1, 224, device='cuda')
            tgt = torch.tensor([[0.0, 1.0]], device='cuda')
            for _ in range(2):
                tr.train_step(x, tgt)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            v = [events_ms(lambda: tr.train_step(x, tgt), max(1, args.reps // 2)) for _ in range(args.rounds)]
            emit(dict(bench='nested', runner='step_' + kind, windows=w, nb=nb, base_network='densenet18', use_graph=False,
                      ms_median=round(statistics.median(v), 4), ms_min=round(min(v), 4), ms_max=round(max(v), 4),
                      peak_mib=round(torch.cuda.max_memory_allocated() / 2.0 ** 20, 1), rounds=args.rounds))
            tr.release_graphs()
            del tr, model
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            for rec in lines:
                f.write(json.dumps(rec) + '\n')
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
