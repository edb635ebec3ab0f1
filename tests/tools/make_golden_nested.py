"""Goldens of the nested networks from the REAL reference classes (models/cnn_to_nested_layer.py on its densenet18, dropout off),
run where the reference is checked out ($DEEPARDS_REFERENCE, default: a `reference` directory beside this repository); never
imported by a test:

    python tests/tools/make_golden_nested.py

Case: one patient of W = 3 windows of NB = 4 breaths, real rows of tests/golden/test_dataset_windows.npz (normalised with the
file's mu / std).  Writes tests/golden/nested_<rnn|lstm>_w3.p<i>.npz -- one record sharded into parts below the 1 MiB limit
(``nested_ref.load_golden`` merges them):

    keys                      the reference's state_dict keys, in order
    param/<key>               the seeded parameters (float32)
    x (1, 3, 4, 1, 224), r (1, 3, 2)
    logits, grad/<key>        float64 run (under torch.set_default_dtype(float64): the reference's forward writes the features
                              into a torch.rand buffer of the DEFAULT dtype, so .double() alone would round them to float32)
    logits32, err32/<key>     the reference's own float32 run: its logits, and per gradient max |float32 - float64| -- the
                              yardstick for the device
    feat (3, 4, 128)          the breath block's features of the float64 run (pins tests/tools/nested_ref.py)
    idx, idx32 (3, 128)       the breath the median selects, both runs

``window_linear`` never receives a gradient (its call is commented out in the reference): it has no grad/ entry.  The seed is
the first at which both runs select the same breath at every (w, f) whose median is non-zero (a tie at exactly 0 is harmless:
ReLU then passes no gradient), so the golden does not depend on how a near-tie fell."""
import glob
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)

from nested_ref import W, NB                      # noqa: E402  (the case's shape, shared with the tests' loader)

OUT = os.path.join(ROOT, 'tests', 'golden')
LIMIT = 1000 * 1024            # per part, below the 1 MiB limit of a committed file


def case_input():
    z = np.load(os.path.join(OUT, 'test_dataset_windows.npz'))
    x = (z['x'][:W, :NB] - float(z['mu'])) / float(z['std'])
    return np.ascontiguousarray(x.reshape(1, W, NB, 1, 224)).astype(np.float32)


def run(kind, params, x, r, dtype):
    from deepards.models.cnn_to_nested_layer import CNNToNestedRNNNetwork, CNNToNestedLSTMNetwork
    from deepards.models.densenet import densenet18
    torch.set_default_dtype(dtype)
    try:
        torch.manual_seed(0)
        cls = CNNToNestedLSTMNetwork if kind == 'lstm' else CNNToNestedRNNNetwork
        model = cls(densenet18(drop_rate=0), NB, False)
        if params is None:
            return {k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
        model.load_state_dict({k: torch.tensor(v).to(dtype) if np.issubdtype(v.dtype, np.floating) else torch.tensor(v)
                               for k, v in params.items()}, strict=True)
        model.train()
        feats = []
        hook = model.breath_block.register_forward_hook(lambda m, i, o: feats.append(o.detach().clone()))
        logits = model(torch.tensor(x).to(dtype), None)
        hook.remove()
        (logits * torch.tensor(r).to(dtype)).sum().backward()
        feat = torch.stack(feats)
        vals = {'logits': logits.detach().numpy(), 'feat': feat.numpy(), 'idx': feat.median(dim=1)[1].numpy().astype(np.int32)}
        for name, p in model.named_parameters():
            if p.grad is not None:
                vals['grad/' + name] = p.grad.numpy()
            else:
                assert name.startswith('window_linear.'), name
        return vals, list(model.state_dict().keys())
    finally:
        torch.set_default_dtype(torch.float32)


def write_parts(kind, rec):
    for old in glob.glob(os.path.join(OUT, 'nested_%s_w%d.p*.npz' % (kind, W))):
        os.remove(old)
    parts, cur, size = [], {}, 0
    for k, v in rec.items():
        n = np.asarray(v).nbytes + 256
        assert n < LIMIT, k
        if cur and size + n > LIMIT:
            parts.append(cur)
            cur, size = {}, 0
        cur[k] = v
        size += n
    parts.append(cur)
    for i, p in enumerate(parts):
        path = os.path.join(OUT, 'nested_%s_w%d.p%d.npz' % (kind, W, i))
        np.savez(path, **p)
        assert os.path.getsize(path) < 1024 * 1024, path
        print('%s  %d tensors, %.0f KB' % (os.path.basename(path), len(p), os.path.getsize(path) / 1024.0))


def main():
    sys.path.insert(0, os.environ.get('DEEPARDS_REFERENCE', os.path.join(os.path.dirname(ROOT), 'reference')))
    x = case_input()
    for kind in ('rnn', 'lstm'):
        for seed in range(64):
            torch.manual_seed(1000 + seed)
            base = run(kind, None, None, None, torch.float32)
            gen = torch.Generator().manual_seed(seed)
            # the reference's default parameters, every float one re-drawn a little larger so that no gradient is tiny
            params = {k: (v if not np.issubdtype(v.dtype, np.floating) or 'running' in k
                          else (v + 0.05 * torch.randn(v.shape, generator=gen).numpy()).astype(np.float32)) for k, v in base.items()}
            r = torch.randn(1, W, 2, generator=gen).numpy().astype(np.float32)
            v64, keys = run(kind, params, x, r, torch.float64)
            v32, _ = run(kind, params, x, r, torch.float32)
            live = np.take_along_axis(v64['feat'], v64['idx'][:, None, :].astype(np.int64), 1)[:, 0, :] != 0
            if (v64['idx'] == v32['idx'])[live].all():
                break
            print('%s seed %d: the two runs select different breaths at %d live medians, next seed' %
                  (kind, seed, int((v64['idx'] != v32['idx'])[live].sum())))
        else:
            raise SystemExit('no seed found')
        rec = {'keys': np.array(keys), 'seed': np.int64(seed), 'x': x, 'r': r, 'logits': v64['logits'],
               'logits32': v32['logits'].astype(np.float64), 'feat': v64['feat'], 'idx': v64['idx'], 'idx32': v32['idx']}
        for k, v in params.items():
            rec['param/' + k] = v
        worst = 0.0
        for k, v in v64.items():
            if k.startswith('grad/'):
                rec[k] = v
                e, mag = np.abs(v32[k].astype(np.float64) - v).max(), np.abs(v).max()
                rec['err32/' + k[5:]] = np.float64(e)
                worst = max(worst, e / mag)
        print('%s: seed %d, %d live medians of %d, logits err32 %.2e, worst gradient err32 / max %.2e' %
              (kind, seed, int(live.sum()), live.size, np.abs(rec['logits32'] - rec['logits']).max(), worst))
        write_parts(kind, rec)


if __name__ == '__main__':
    main()
