"""Goldens of the cnn_transformer head from the REAL reference classes (models/transformer.py, models/cnn_transformer.py),
run where the reference is checked out ($DEEPARDS_REFERENCE, default: a `reference` directory beside this repository); never
imported by a test:

    python tests/tools/make_golden_transformer.py

The reference's transformer.py is Python 2 text; it runs unmodified with ``builtins.xrange = range`` set before the import
and ``attention.head_size`` made an int on every block after construction.

Writes tests/golden/tfm_block_<B>x<T>x<D>x<H>.npz  (Transformer of 2 blocks + Linear(D, 2) + BCE, dropout p = 0),
       tests/golden/tfm_masked_2x20x128x16.npz     (the two nn.Dropout children of every block replaced by fixed masks, p = 0.2),
       tests/golden/tfm_model_b2_<backbone>.npz    (CNNTransformerNetwork on oracle.weights.seeded_params backbones).
Per tensor: the fp64 value (``<name>``; ``oracle.weights.digest`` of it where the case is large, key ``dig/<name>``) and
``err32/<name>``, the rel-l2 of the reference's own fp32 run against its fp64 run -- the yardstick of the GPU tests."""
import builtins
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.environ.get('DEEPARDS_REFERENCE', os.path.join(os.path.dirname(ROOT), 'reference')))
builtins.xrange = range

from oracle.weights import seeded_params, seeded_batch, digest                              # noqa: E402
from deepards.models.transformer import Transformer                                         # noqa: E402
from deepards.models.cnn_transformer import CNNTransformerNetwork                           # noqa: E402
from deepards.models.resnet import resnet18                                                 # noqa: E402
from deepards.models.densenet import densenet18                                             # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden')
P_DROP = 0.2


def rel_l2(a, b):
    nb = float(np.linalg.norm(b))
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / (nb if nb > 0 else 1.0))


class FixedMask(torch.nn.Module):
    def __init__(self, mask):
        super(FixedMask, self).__init__()
        self.mask = mask

    def forward(self, x):
        return x * self.mask.to(x.dtype) / (1 - P_DROP)


def fix_blocks(tfm, masks=None):
    for i, blk in enumerate(tfm.blocks):
        blk.attention.head_size = int(blk.attention.head_size)
        if masks is None:
            blk.attention_dropout.p = 0.0
            blk.ff[3].p = 0.0
        else:
            blk.attention_dropout = FixedMask(masks[i][0])
            blk.ff[3] = FixedMask(masks[i][1])


def block_case(b, t, d, h, seed, masked=False, big=False):
    torch.manual_seed(seed)
    tfm = Transformer(d, h, 2, 4)
    lin = torch.nn.Linear(d, 2)
    rng = np.random.default_rng([seed, b, t, d, h])
    x = rng.standard_normal((b, t, d)).astype(np.float32)
    target = np.eye(2, dtype=np.float32)[rng.integers(0, 2, b)]
    masks = None
    rec = dict(x=x, target=target, shape=np.array([b, t, d, h]), p=P_DROP if masked else 0.0,
               names=np.array([n for n, _ in tfm.named_parameters()] + ['linear_final.weight', 'linear_final.bias']))
    if masked:
        m = rng.random((2, 2, b, t, d)) >= P_DROP
        rec['masks_packed'] = np.packbits(m)
        masks = [[torch.from_numpy(m[i, s]) for s in range(2)] for i in range(2)]
    fix_blocks(tfm, masks)
    for n, q in list(tfm.named_parameters()) + [('linear_final.' + k, v) for k, v in lin.named_parameters()]:
        rec['param/' + n] = q.detach().numpy().copy()
    vals = {}
    for dt in (torch.float64, torch.float32):
        tfm.to(dt)
        lin.to(dt)
        tfm.zero_grad()
        lin.zero_grad()
        xt = torch.from_numpy(x).to(dt).requires_grad_(True)
        y = tfm(xt)
        logits = lin(y)
        loss = torch.nn.BCEWithLogitsLoss()(logits, torch.from_numpy(target).to(dt).unsqueeze(1).repeat(1, t, 1))
        loss.backward()
        v = dict(y=y, logits=logits, loss=loss, dx=xt.grad)
        for i, blk in enumerate(tfm.blocks):
            v['weights%d' % i] = blk.attention.weights
        for n, q in tfm.named_parameters():
            v['grad/' + n] = q.grad
        for n, q in lin.named_parameters():
            v['grad/linear_final.' + n] = q.grad
        vals[dt] = {k: a.detach().numpy().astype(np.float64) for k, a in v.items()}
    for k, a in vals[torch.float64].items():
        rec[('dig/' if big and a.size > 1024 else '') + k] = digest(a) if big and a.size > 1024 else a
        rec['err32/' + k] = rel_l2(vals[torch.float32][k], a)
    name = 'tfm_%s_%dx%dx%dx%d.npz' % ('masked' if masked else 'block', b, t, d, h)
    save(name, rec)


def model_case(backbone, seed=11, b=2, h=16, blocks=2):
    x, tgt = seeded_batch(b, 20, seed, 'randn')
    rec = dict(x=x, target=tgt, backbone=backbone, seed=seed, b=b, bn_bias_shift=0.0, hidden=h, blocks=blocks,
               first_pool_type='max')
    vals = {}
    for dt in (torch.float64, torch.float32):
        torch.manual_seed(seed)
        bb = resnet18() if backbone == 'resnet18' else densenet18(drop_rate=0)
        model = CNNTransformerNetwork(bb, 0, False, h, blocks)
        fix_blocks(model.transformer)
        sd = {k: torch.from_numpy(v) for k, v in seeded_params(backbone, seed, head='single_breath').items()
              if k.startswith('breath_block.')}
        missing = model.load_state_dict(sd, strict=False)
        assert not missing.unexpected_keys
        if dt == torch.float64:
            rec['names'] = np.array(list(model.state_dict().keys()))
            for n, q in model.named_parameters():
                if not n.startswith('breath_block.'):
                    rec['param/' + n] = q.detach().numpy().copy()
        model = model.to(dt).train()
        xt, tt = torch.from_numpy(x).to(dt), torch.from_numpy(tgt).to(dt)
        out = model(xt, torch.full((b,), float('nan'), dtype=dt))
        loss = torch.nn.BCEWithLogitsLoss()(out, tt.unsqueeze(1).repeat((1, out.shape[1], 1)))
        loss.backward()
        v = dict(logits=out, loss=loss)
        for n, q in model.named_parameters():
            if q.grad is not None:
                v['grad/' + n] = q.grad
        vals[dt] = {k: a.detach().numpy().astype(np.float64) for k, a in v.items()}
    for k, a in vals[torch.float64].items():
        big = k.startswith('grad/')
        rec[('dig/' if big else '') + k] = digest(a) if big else a
        rec['err32/' + k] = rel_l2(vals[torch.float32][k], a)
    save('tfm_model_b2_%s.npz' % backbone, rec)


def save(name, rec):
    path = os.path.join(OUT, name)
    np.savez_compressed(path, **rec)
    size = os.path.getsize(path)
    assert size < (1 << 20), (name, size)
    print(name, size, 'loss', float(rec['loss']), 'err32 y/logits', rec.get('err32/y', rec['err32/logits']))


if __name__ == '__main__':
    if sys.argv[1:] == ['models']:
        model_case('resnet18')
        model_case('densenet18')
        sys.exit(0)
    block_case(2, 20, 128, 16, 3)
    block_case(2, 20, 512, 16, 4, big=True)
    block_case(2, 5, 128, 8, 5)
    block_case(2, 20, 128, 16, 6, masked=True)
    model_case('resnet18')
    model_case('densenet18')
