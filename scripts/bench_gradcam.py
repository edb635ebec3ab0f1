"""Cost of the batched Grad-CAM path against the route a user had before it (reported, not gated; bench.py measures the flagship):

    python scripts/bench_gradcam.py [--batch 64] [--rounds 7] [--reps 10] [--loop-windows 2] [--out FILE.json]

For cnn_linear + densenet18 and + densenet201 at B windows of (20, 1, 224), in ONE process, the three runners ALTERNATING round
by round so that drift of a shared machine lands on all; medians over the rounds, with the spread:

  kernel      ``hip_ops.gradcam`` alone (its two launches) on the map of the batch: ``reps`` calls captured in one graph and
              replayed between device events, so that the launches' host cost stays out; with the bytes it has to move (the map
              read once) and the rate that makes
  call        the same call eager, ``reps`` times between device events: the host's share (two launches, eleven allocations)
  cams        ``GradCam.cams``: one batched forward + the kernel, the same way
  cams_pw     ``GradCam.cams(per_window_forward=True)``: B forwards of one window + the kernel (what ``PatientCams`` runs, for
              the bits of the single-window methods), the same way with ``reps`` / 5 calls
  loop        the per-window route: ``features`` -> register_hook -> relu -> avgpool -> view(-1) -> linear_final -> backward of the
              one-hot score (the calls of tests/test_model_gpu.py::test_gradcam_surface_on_densenet), both arrays copied to the
              host, then the reference's numpy loops over the channels for the max-min window CAM (gradcam.py:138-162);
              ``loop-windows`` windows per round on a host clock around work that ends in a synchronise, scaled to B windows
One JSON line per measurement.  No GPU, no number: the script fails."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def loop_window(model, x, target):
    """One window through the hook-and-backward route and the reference's numpy loops -> the uint8 window CAM."""
    import torch.nn.functional as Fn
    grads = {}
    conv = model.breath_block.features(x)
    conv.register_hook(lambda gr: grads.__setitem__('g', gr))
    out = model.linear_final(model.breath_block.avgpool(Fn.relu(conv)).view(-1)).unsqueeze(0)
    if target is None:
        target = int(np.argmax(out.detach().cpu().numpy()))
    one_hot = torch.zeros((1, 2), device=x.device)
    one_hot[0, target] = 1
    model.zero_grad()
    torch.sum(one_hot * out).backward()
    grad = grads['g'].cpu().numpy()
    conv_output = conv.detach().cpu().numpy()
    weights = np.mean(grad, axis=(0, 2))
    conv_output = np.mean(conv_output, axis=0)
    cam = np.zeros(conv_output.shape[1:], dtype=np.float32)
    for i, w in enumerate(weights):
        cam += w * conv_output[i, :]
    cam = np.maximum(cam, 0)
    with np.errstate(invalid='ignore', divide='ignore'):
        cam = (cam - np.min(cam)) / (np.max(cam) - np.min(cam))
        return np.uint8(np.nan_to_num(cam) * 255)


def events_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--loop-windows', type=int, default=2)
    ap.add_argument('--networks', default='densenet18,densenet201')
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('bench_gradcam.py measures on the GPU: none here')
    import deepards_amd.models as M
    from deepards_amd import gradcam as GC, hip_ops as H
    from deepards_amd.train import _capture_graph
    nb, lines = 20, []
    for name in args.networks.split(','):
        torch.manual_seed(0)
        model = M.CNNLinearNetwork(M.base_networks[name](drop_rate=0), nb, 0).cuda().train()
        x = torch.randn(args.batch, nb, 1, 224, device='cuda')
        gc = GC.GradCam(model)
        fmap = gc.extractor.forward_map(x)
        lin = model.linear_final
        w, bias = lin.weight.detach(), lin.bias.detach()
        tin = torch.full((args.batch,), -1, dtype=torch.int32, device='cuda')
        ws = torch.empty((H.gradcam_workspace(args.batch, nb, fmap.shape[2]) // 4,), device='cuda')
        call = lambda: H.gradcam(fmap, w, bias, tin, nb, workspace=ws)
        runners = {'call': call, 'cams': lambda: gc.cams(x, tin), 'cams_pw': lambda: gc.cams(x, tin, per_window_forward=True)}
        for fn in runners.values():                                  # warm-up: code objects, allocator pools
            events_ms(fn, 2)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            call()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with _capture_graph(graph):
            held = [call() for _ in range(args.reps)]                # (held: the outputs live as long as the graph)
        graph.replay()
        loop_window(model, x[0], None)
        times = {'kernel': [], 'call': [], 'cams': [], 'cams_pw': [], 'loop': []}
        for _ in range(args.rounds):
            times['kernel'].append(events_ms(graph.replay, 1) / args.reps)
            for k, fn in runners.items():
                times[k].append(events_ms(fn, max(args.reps // 5, 1) if k == 'cams_pw' else args.reps))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.loop_windows):
                loop_window(model, x[i % args.batch], None)
            torch.cuda.synchronize()
            times['loop'].append((time.perf_counter() - t0) * 1e3 / args.loop_windows * args.batch)
        map_bytes = fmap.numel() * 4
        med = {k: statistics.median(v) for k, v in times.items()}
        for k, v in times.items():
            rec = dict(bench='gradcam', network=name, batch=args.batch, nb=nb, channels=int(fmap.shape[2]), runner=k,
                       ms_median=round(med[k], 4), ms_min=round(min(v), 4), ms_max=round(max(v), 4), rounds=args.rounds)
            if k == 'kernel':
                rec.update(map_mbytes=round(map_bytes / 1e6, 3), gbytes_per_s=round(map_bytes / med[k] / 1e6, 1))
            if k == 'loop':
                rec.update(windows_timed_per_round=args.loop_windows, ms_per_window=round(med[k] / args.batch, 4),
                           ratio_to_cams=round(med[k] / med['cams'], 1), ratio_to_cams_pw=round(med[k] / med['cams_pw'], 1))
            lines.append(rec)
            print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            for rec in lines:
                f.write(json.dumps(rec) + '\n')
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
