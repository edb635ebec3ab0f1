"""Cost of the autoencoder and of its own kernels (reported, not gated; bench.py measures the flagship):

    python scripts/bench_autoencoder.py [--batches 16,64] [--steps 20] [--rounds 7] [--out FILE.json] [--skip-steps]

1. The whole training step of ``AutoencoderTrainer`` (graph replay) at B windows of (20, 1, 224) beside the SAME network from stock
   torch modules on the same GPU -- Conv1d / BatchNorm1d / MaxPool1d(2, return_indices) / MaxUnpool1d / ConvTranspose1d / MSELoss,
   SGD with Nesterov momentum, eager and, if torch captures it, as a graph -- in ONE process: ``rounds`` windows of ``steps`` steps
   timed with device events, the runners ALTERNATING round by round so that drift of a shared machine lands on all of them;
   median round, spread, ratios.  The forward-only ``test_step`` (``model.eval()``) the same way beside stock torch in eval mode.
2. Each kernel of csrc/autoencoder.hip alone at the largest batch, captured in a graph and replayed the same way: the pool
   forward and backward and the unpool pair at the four stages' shapes, the output stage at L = 224.  In the SAME run,
   alternating with it: a float4 copy (``y.copy_(x)``) that moves the bytes the kernel must move (each map it reads or writes,
   once) -- its bound.  Each kernel's time is reported as a ratio to that copy.
One JSON line per measurement.  No GPU, no number: the script fails."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_se_resnet import timed_rounds, captured      # noqa: E402

NB, L = 20, 224
CHANNELS = (1, 64, 128, 256, 512)


def med(ts):
    return statistics.median(ts)


class StockAutoencoder(nn.Module):
    """The same network from stock torch modules (its own text: the layer list of the issue, not the reference's file)."""

    def __init__(self):
        super(StockAutoencoder, self).__init__()
        self.down = nn.ModuleList(nn.Conv1d(CHANNELS[k], CHANNELS[k + 1], 3, padding=1) for k in range(4))
        self.bn = nn.ModuleList(nn.BatchNorm1d(CHANNELS[k + 1]) for k in range(4))
        self.up = nn.ModuleList(nn.ConvTranspose1d(CHANNELS[4 - k], CHANNELS[3 - k], 3, padding=1) for k in range(4))
        self.pool, self.unpool = nn.MaxPool1d(2, return_indices=True), nn.MaxUnpool1d(2)

    def forward(self, x):
        idx = []
        for conv, bn in zip(self.down, self.bn):
            x, i = self.pool(bn(conv(x)))
            idx.append(i)
        for k, conv in enumerate(self.up):
            x = conv(self.unpool(x, idx[3 - k]))
        return x


def stock_runners(rows_x):
    """name -> one-step callable of the stock network: eager step, captured step (None if torch refuses), eval forward."""
    torch.manual_seed(0)
    net = StockAutoencoder().cuda().train()
    opt = torch.optim.SGD(net.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4, nesterov=True)
    crit = nn.MSELoss()

    def step():
        opt.zero_grad(set_to_none=False)
        loss = crit(net(rows_x), rows_x)
        loss.backward()
        opt.step()
        return loss

    for _ in range(3):
        step()

    def graph():
        """The captured step's replay callable, or the reason torch refused the capture (tried last: a refused capture may
        leave the process unable to capture again)."""
        try:
            return captured(step)[0], None
        except Exception as e:                           # noqa: BLE001 -- reported, not hidden
            return None, '%s: %s' % (type(e).__name__, str(e)[:200])
    ev = StockAutoencoder().cuda().eval()

    def fwd():
        with torch.no_grad():
            return ev(rows_x)
    for _ in range(3):
        fwd()
    return step, graph, fwd


def kernel_runners(rows):
    """[(name, shape, callable, bytes the kernel must move)] of the new kernels at the four stages' shapes."""
    from deepards_amd import hip_ops as H
    out = []
    for k in range(1, 5):
        lin, c = L >> (k - 1), CHANNELS[k]
        lo = lin // 2
        torch.manual_seed(k)
        y, dout = torch.randn(rows, lin, c, device='cuda'), torch.randn(rows, lo, c, device='cuda')
        mean, invstd = H.vgg_stats(y, rows)
        gamma, beta = torch.rand(c, device='cuda') + 0.5, torch.randn(c, device='cuda') * 0.1
        pooled, sel = H.bn_maxpool2_idx_fwd(y, rows, mean, invstd, gamma, beta)
        dy, up = torch.empty_like(y), torch.empty_like(y)
        full, half, bits = 4 * y.numel(), 4 * dout.numel(), 4 * sel.numel()
        shape = (rows, lin, c)
        out += [('bn_maxpool2_idx_fwd', shape, lambda y=y, m=mean, i=invstd, g=gamma, b=beta, o=pooled, s=sel:
                 H.bn_maxpool2_idx_fwd(y, rows, m, i, g, b, out=o, sel=s), full + half + bits),
                # (the backward reads y and dout in both of its passes: the bytes it MUST move count them once)
                ('bn_maxpool2_idx_bwd', shape, lambda y=y, d=dout, s=sel, m=mean, i=invstd, g=gamma, b=beta, o=dy:
                 H.bn_maxpool2_idx_bwd(d, s, y, rows, m, i, g, b, out=o), 2 * full + half + bits),
                ('unpool2_fwd', shape, lambda v=dout, s=sel, b=beta, o=up: H.unpool2_fwd(v, s, b, out=o), full + half + bits),
                ('unpool2_bwd', shape, lambda d=y, s=sel, o=pooled: H.unpool2_bwd(d, s, out=o), full + half + bits)]
    torch.manual_seed(9)
    v, x = torch.randn(rows, L // 2, 64, device='cuda'), torch.randn(rows, L, device='cuda')
    sel1 = torch.randint(-2 ** 31, 2 ** 31 - 1, (rows, L // 2, 2), device='cuda', dtype=torch.int64).to(torch.int32)
    b3, w4, b4 = torch.randn(64, device='cuda') * 0.1, torch.randn(64, 1, 3, device='cuda') / 14.0, torch.zeros(1, device='cuda')
    recon, dr, _ = H.ae_out_fwd(v, b3, sel1, w4, b4, x)
    vb, xb, sb = 4 * v.numel(), 4 * x.numel(), 4 * sel1.numel()
    out += [('ae_out_fwd', (rows, L), lambda: H.ae_out_fwd(v, b3, sel1, w4, b4, x), vb + sb + 3 * xb),
            ('ae_out_bwd', (rows, L), lambda: H.ae_out_bwd(dr, v, b3, sel1, w4), 2 * vb + sb + xb)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='16,64')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out')
    ap.add_argument('--skip-steps', action='store_true', help='kernels only')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_autoencoder needs an MI355X: there is no CPU timing')
    batches = [int(b) for b in a.batches.split(',')]
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    if not a.skip_steps:
        import deepards_amd.models as M
        from deepards_amd.autoencoder import AutoencoderTrainer
        for batch in batches:
            torch.manual_seed(1)
            x = torch.randn(batch, NB, 1, L, device='cuda')
            torch.manual_seed(0)
            tr = AutoencoderTrainer(M.AutoencoderNetwork(M.AutoencoderCNN()).cuda().train(), use_graph=True, clip_grad=False)
            for _ in range(3):                                       # eager step, capture + replay, replay
                tr.train_step(x)
            tr.test_step(x)
            tr.test_step(x)
            sx = tr.static_batch()[0]
            step, graph, fwd = stock_runners(x.view(batch * NB, 1, L))
            runners = {'hip_train_step': lambda: tr.train_step(sx), 'torch_eager_train_step': step}
            times = timed_rounds(runners, a.steps, a.rounds)
            # the captured test step, without the copies test_step makes of its results for the caller
            tg, tstatic, _ = next(iter(tr._test_graphs.values()))
            times.update(timed_rounds({'hip_test_step': tg.replay, 'torch_eager_eval_forward': fwd}, a.steps, a.rounds))
            for name, ts in times.items():
                base = med(times['torch_eager_eval_forward' if 'test' in name or 'eval' in name else 'torch_eager_train_step'])
                emit(dict(what='autoencoder_step', runner=name, batch=batch, rows=batch * NB, L=L, steps=a.steps, rounds=a.rounds,
                          ms_median=round(med(ts), 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4),
                          ratio_to_torch_eager=round(med(ts) / base, 3)))
            emit(dict(what='autoencoder_loss', batch=batch, hip_last_loss=float(tr.last_loss)))
            replay, why = graph()
            if replay is None:
                emit(dict(what='torch_capture_refused', batch=batch, error=why))
                torch.cuda.synchronize()
            else:
                ts = timed_rounds({'torch_captured_train_step': replay, 'hip_train_step': runners['hip_train_step']}, a.steps, a.rounds)
                emit(dict(what='autoencoder_step', runner='torch_captured_train_step', batch=batch, rows=batch * NB, L=L, steps=a.steps,
                          rounds=a.rounds, ms_median=round(med(ts['torch_captured_train_step']), 4),
                          ms_min=round(min(ts['torch_captured_train_step']), 4), ms_max=round(max(ts['torch_captured_train_step']), 4),
                          hip_ms_median_same_rounds=round(med(ts['hip_train_step']), 4),
                          hip_ratio_to_torch_captured=round(med(ts['hip_train_step']) / med(ts['torch_captured_train_step']), 3)))
            tr.release_graphs()
            del tr, runners, step, graph, fwd, replay
            torch.cuda.empty_cache()
    rows = max(batches) * NB
    for name, shape, fn, nbytes in kernel_runners(rows):
        n = nbytes // 8                                              # a copy of n floats reads and writes nbytes in all
        src, dst = torch.randn(n, device='cuda'), torch.empty(n, device='cuda')
        kfn, keep = captured(fn)
        cfn, keep2 = captured(lambda: dst.copy_(src))
        ts = {k: [1000 * v for v in vs] for k, vs in timed_rounds({'kernel': kfn, 'copy': cfn}, a.steps, a.rounds).items()}      # us
        emit(dict(what='autoencoder_kernel', kernel=name, shape=list(shape), mbytes=round(nbytes / 1e6, 2),
                  us_median=round(med(ts['kernel']), 1), us_min=round(min(ts['kernel']), 1), us_max=round(max(ts['kernel']), 1),
                  copy_us_median=round(med(ts['copy']), 1), tbytes_per_s=round(nbytes / med(ts['kernel']) / 1e6, 2),
                  ratio_to_copy=round(med(ts['kernel']) / med(ts['copy']), 2)))
        del src, dst, kfn, cfn, keep, keep2
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
