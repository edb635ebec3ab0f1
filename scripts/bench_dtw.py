"""Cell rate of the DTW pairs kernel (reported, not gated; bench.py measures the flagship):

    python scripts/bench_dtw.py [--cases breaths,windows] [--rounds 5] [--window-s 0.3] [--clock-mhz 2400] [--out F.json]

  breaths   224 x 224 at P = 30000: the pairs of one patient's ``dtw_analyze`` (3 predecessors x 20 breaths x 500 windows)
  windows   4480 x 4480 at P = 2048: flattened windows of ``find_patient_similarity`` (the 'random' matrix of an 80-patient fold
            is about 158 k such pairs)
each with float32 accumulation (float32 table), float64 accumulation of a float32 table and float64 accumulation of a float64
table.  One launch is timed between device events, repeated until a window of ``--window-s`` seconds is filled, after a warm-up
of the same shape; the configurations ALTERNATE round by round so that drift of a shared machine lands on all; medians over
the rounds, with the spread.

Per case: ``cells_per_s`` = P n m / time (the cells of the matrices, not the lane slots of the wavefront), and
``valu_bound_fraction`` = cells_per_s x VALU instructions per cell / (CUs x 4 SIMDs x 16 lanes x clock): the share of the
vector-issue rate the kernel's own instruction mix would need at that cell rate.  The instructions per cell are counted in the
main loop of the gfx950 ISA of csrc/dtw.hip (``hipcc -O3 --offload-arch=gfx950 -save-temps``; DESIGN_APPENDIX.md, section DTW,
lists the counts per kernel) -- recount them there when the kernel changes.  The clock is ``--clock-mhz``, by default the
MI355X's maximum of 2400 MHz; a chip that holds its clock lower under load shows as a smaller fraction.
One JSON line per measurement.  No GPU, no number: the script fails."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# VALU instructions per cell in the main loop, (accumulation, columns per lane) -> count; DESIGN_APPENDIX.md section DTW
VALU_PER_CELL = {('f32', 4): 33 / 8.0, ('f64', 4): 53 / 8.0, ('f32', 72): 444 / 144.0, ('f64', 72): 421 / 72.0}
CASES = {'breaths': (224, 224, 30000), 'windows': (4480, 4480, 2048)}
CONFIGS = (('f32', torch.float32), ('f64', torch.float32), ('f64', torch.float64))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='breaths,windows')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--window-s', type=float, default=0.3)
    ap.add_argument('--clock-mhz', type=float, default=2400.0, help="the bound's clock: the MI355X maximum")
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('bench_dtw: no GPU, no number')
    from deepards_amd import dtw_ops as O
    props = torch.cuda.get_device_properties(0)
    clock_hz = args.clock_mhz * 1e6
    issue_rate = props.multi_processor_count * 4 * 16 * clock_hz
    lines = []
    for case in args.cases.split(','):
        n, m, p = CASES[case]
        rng = np.random.RandomState(1)
        rows = 256
        host = (rng.randn(rows, max(n, m)) * 30).astype(np.float32)
        ia = torch.as_tensor(rng.randint(0, rows, p).astype(np.int32)).cuda()
        ib = torch.as_tensor(rng.randint(0, rows, p).astype(np.int32)).cuda()
        plan = O.dtw_plan(n, m, p)
        runs = []
        for acc, dtype in CONFIGS:
            ta = torch.as_tensor(host[:, :n]).to(dtype).cuda().contiguous()
            tb = torch.as_tensor(host[:, :m]).to(dtype).cuda().contiguous()
            out = torch.empty((p,), device='cuda', dtype=torch.float32 if acc == 'f32' else torch.float64)
            fn = (lambda ta=ta, tb=tb, out=out, acc=acc: O.dtw_pairs(ta, ia, ib, tb, acc=acc, out=out))
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            fn()
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            reps = max(1, int(args.window_s * 1e3 / max(a.elapsed_time(b), 1e-3)))
            runs.append((acc, dtype, fn, reps, []))
        for _ in range(args.rounds):
            for acc, dtype, fn, reps, times in runs:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(reps):
                    fn()
                b.record()
                torch.cuda.synchronize()
                times.append(a.elapsed_time(b) / reps)
        for acc, dtype, fn, reps, times in runs:
            ms = statistics.median(times)
            cells = float(p) * n * m / (ms * 1e-3)
            valu = VALU_PER_CELL[(acc, plan['cols_per_lane'])]
            lines.append(dict(case=case, n=n, m=m, pairs=p, acc=acc, table=str(dtype).replace('torch.', ''),
                              cols_per_lane=plan['cols_per_lane'], lanes=plan['lanes'], steps=plan['steps'], reps=reps,
                              ms=round(ms, 4), ms_min=round(min(times), 4), ms_max=round(max(times), 4),
                              cells_per_s=cells, pairs_per_s=p / (ms * 1e-3), valu_per_cell=round(valu, 3),
                              valu_issue_per_s=issue_rate, clock_mhz=clock_hz / 1e6, cus=props.multi_processor_count,
                              valu_bound_fraction=round(cells * valu / issue_rate, 4),
                              lane_slot_use=round(n * m / float(plan['steps'] * 64 * plan['cols_per_lane']), 4)))
            print(json.dumps(lines[-1]), flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            for ln in lines:
                f.write(json.dumps(ln) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
