"""Cost of the UNet autoencoder and of its own kernels (reported, not gated; bench.py measures the flagship):

    python scripts/bench_unet.py [--batches 16,64] [--steps 20] [--rounds 7] [--out FILE.json] [--skip-steps]

1. The training step of ``AutoencoderTrainer`` on ``AutoencoderNetwork(UNet(1))`` -- captured (graph replay) and eager -- at B
   windows of (20, 1, 224) beside the SAME network from stock torch modules on the same GPU -- Conv1d / ReLU / MaxPool1d(2) /
   Upsample(x2, linear, align_corners=True) / cat / MSELoss, SGD with Nesterov momentum, eager and, if torch captures it, as a graph
   -- in ONE process: ``rounds`` windows of ``steps`` steps timed with device events, the runners ALTERNATING round by round so that
   drift of a shared machine lands on all of them; median round, spread, ratios.  The forward-only ``test_step`` the same way.
2. Each kernel of csrc/unet.hip alone at the largest batch and the shapes the network gives it (slices of the concat buffers where
   the network passes slices), captured in a graph and replayed the same way.  In the SAME run, alternating with it: a float4 copy
   (``y.copy_(x)``) that moves the bytes the kernel must move (each map it reads or writes, once) -- its bound.  Each kernel's time
   is reported as a ratio to that copy.
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
CHANNELS = (64, 128, 256, 512)


def med(ts):
    return statistics.median(ts)


def _dc(a, b):
    return nn.Sequential(nn.Conv1d(a, b, 3, padding=1), nn.ReLU(inplace=True), nn.Conv1d(b, b, 3, padding=1), nn.ReLU(inplace=True))


class StockUNet(nn.Module):
    """The same network from stock torch modules (its own text: the layer list of DESIGN.md 5l, not the reference's file)."""

    def __init__(self):
        super(StockUNet, self).__init__()
        self.down = nn.ModuleList(_dc(a, b) for a, b in zip((1,) + CHANNELS[:3], CHANNELS))
        self.up = nn.ModuleList(_dc(3 * c, c) for c in CHANNELS[2::-1])
        self.pool, self.ups = nn.MaxPool1d(2), nn.Upsample(scale_factor=2, mode='linear', align_corners=True)
        self.last = nn.Conv1d(64, 1, 1)

    def forward(self, x):
        skips = []
        for k, dc in enumerate(self.down):
            x = dc(x)
            if k < 3:
                skips.append(x)
                x = self.pool(x)
        for k, dc in enumerate(self.up):
            x = dc(torch.cat([self.ups(x), skips[2 - k]], dim=1))
        return self.last(x)


def stock_runners(rows_x):
    """one-step callables of the stock network: eager step, captured step (None + the reason if torch refuses), eval forward."""
    torch.manual_seed(0)
    net = StockUNet().cuda().train()
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
        try:
            return captured(step)[0], None
        except Exception as e:                           # noqa: BLE001 -- reported, not hidden
            return None, '%s: %s' % (type(e).__name__, str(e)[:200])
    ev = StockUNet().cuda().eval()

    def fwd():
        with torch.no_grad():
            return ev(rows_x)
    for _ in range(3):
        fwd()
    return step, graph, fwd


def kernel_runners(rows):
    """[(name, shape, callable, bytes the kernel must move)] of the new kernels at the shapes the network gives them."""
    from deepards_amd import hip_ops as H
    out = []
    for k, c in enumerate(CHANNELS):
        l = L >> k
        torch.manual_seed(k)
        full = 4 * rows * l * c
        y, bias = torch.randn(rows, l, c, device='cuda'), torch.randn(c, device='cuda') * 0.1
        d = torch.randn(rows, l, c, device='cuda')
        out += [('bias_relu', (rows, l, c), lambda y=y, b=bias: H.unet_bias_relu(y, b), 2 * full),
                ('relu_bwd', (rows, l, c), lambda d=d, a=y: H.unet_relu_bwd(d, a, out=d), 3 * full)]
        if k == 3:
            break
        cat, dcat = torch.randn(rows, l, 3 * c, device='cuda'), torch.randn(rows, l, 3 * c, device='cuda')
        skip, pooled, dy = cat[:, :, 2 * c:], torch.empty(rows, l // 2, c, device='cuda'), torch.empty(rows, l, c, device='cuda')
        low = torch.randn(rows, l // 2, 2 * c, device='cuda')                       # the map the level's upsample reads
        b2, dlow = torch.randn(2 * c, device='cuda') * 0.1, torch.empty(rows, l // 2, 2 * c, device='cuda')
        lowb = 4 * low.numel()
        out += [('bias_relu_pool2_fwd', (rows, l, c), lambda s=skip, b=bias, o=pooled: H.unet_bias_relu_pool2_fwd(s, b, out=o),
                 2 * full + full // 2),
                ('pool2_skip_bwd', (rows, l, c), lambda p=pooled, ds=dcat[:, :, 2 * c:], a=skip, o=dy: H.unet_pool2_skip_bwd(p, ds, a, out=o),
                 3 * full + full // 2),
                ('relu_upsample2_fwd', (rows, l // 2, 2 * c), lambda y=low, b=b2, o=cat[:, :, :2 * c]: H.unet_relu_upsample2_fwd(y, b, o),
                 3 * lowb),
                ('relu_upsample2_bwd', (rows, l // 2, 2 * c), lambda d=dcat[:, :, :2 * c], y=low, b=b2, o=dlow:
                 H.unet_relu_upsample2_bwd(d, y, b, out=o), 4 * lowb)]
    torch.manual_seed(9)
    a, x = torch.relu(torch.randn(rows, L, 64, device='cuda')), torch.randn(rows, L, device='cuda')
    w, b = torch.randn(1, 64, 1, device='cuda') / 8.0, torch.zeros(1, device='cuda')
    recon, dr, _ = H.unet_out_fwd(a, w, b, x)
    ab, xb = 4 * a.numel(), 4 * x.numel()
    out += [('out_fwd', (rows, L, 64), lambda: H.unet_out_fwd(a, w, b, x), ab + 3 * xb),
            ('out_bwd', (rows, L, 64), lambda: H.unet_out_bwd(dr, a, w), 2 * ab + xb)]
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
        raise SystemExit('bench_unet needs an MI355X: there is no CPU timing')
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
            tr = AutoencoderTrainer(M.AutoencoderNetwork(M.UNet(1)).cuda().train(), use_graph=True, clip_grad=False)
            torch.manual_seed(0)
            te = AutoencoderTrainer(M.AutoencoderNetwork(M.UNet(1)).cuda().train(), use_graph=False, clip_grad=False)
            for _ in range(3):                                       # eager step, capture + replay, replay
                tr.train_step(x)
                te.train_step(x)
            tr.test_step(x)
            tr.test_step(x)
            sx = tr.static_batch()[0]
            step, graph, fwd = stock_runners(x.view(batch * NB, 1, L))
            runners = {'hip_train_step': lambda: tr.train_step(sx), 'hip_eager_train_step': lambda: te.train_step(x),
                       'torch_eager_train_step': step}
            times = timed_rounds(runners, a.steps, a.rounds)
            # the captured test step, without the copies test_step makes of its results for the caller
            tg, tstatic, _ = next(iter(tr._test_graphs.values()))
            times.update(timed_rounds({'hip_test_step': tg.replay, 'torch_eager_eval_forward': fwd}, a.steps, a.rounds))
            for name, ts in times.items():
                base = med(times['torch_eager_eval_forward' if 'test' in name or 'eval' in name else 'torch_eager_train_step'])
                emit(dict(what='unet_step', runner=name, batch=batch, rows=batch * NB, L=L, steps=a.steps, rounds=a.rounds,
                          ms_median=round(med(ts), 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4),
                          ratio_to_torch_eager=round(med(ts) / base, 3)))
            emit(dict(what='unet_loss', batch=batch, hip_last_loss=float(tr.last_loss)))
            replay, why = graph()
            if replay is None:
                emit(dict(what='torch_capture_refused', batch=batch, error=why))
                torch.cuda.synchronize()
            else:
                ts = timed_rounds({'torch_captured_train_step': replay, 'hip_train_step': runners['hip_train_step']}, a.steps, a.rounds)
                emit(dict(what='unet_step', runner='torch_captured_train_step', batch=batch, rows=batch * NB, L=L, steps=a.steps,
                          rounds=a.rounds, ms_median=round(med(ts['torch_captured_train_step']), 4),
                          ms_min=round(min(ts['torch_captured_train_step']), 4), ms_max=round(max(ts['torch_captured_train_step']), 4),
                          hip_ms_median_same_rounds=round(med(ts['hip_train_step']), 4),
                          hip_ratio_to_torch_captured=round(med(ts['hip_train_step']) / med(ts['torch_captured_train_step']), 3)))
            tr.release_graphs()
            del tr, te, runners, step, graph, fwd, replay
            torch.cuda.empty_cache()
    rows = max(batches) * NB
    for name, shape, fn, nbytes in kernel_runners(rows):
        n = nbytes // 8                                              # a copy of n floats reads and writes nbytes in all
        src, dst = torch.randn(n, device='cuda'), torch.empty(n, device='cuda')
        kfn, keep = captured(fn)
        cfn, keep2 = captured(lambda: dst.copy_(src))
        ts = {k: [1000 * v for v in vs] for k, vs in timed_rounds({'kernel': kfn, 'copy': cfn}, a.steps, a.rounds).items()}      # us
        emit(dict(what='unet_kernel', kernel=name, shape=list(shape), mbytes=round(nbytes / 1e6, 2),
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
