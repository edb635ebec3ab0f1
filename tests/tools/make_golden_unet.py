"""Goldens of the UNet autoencoder from the REAL reference classes (models/unet.py, models/autoencoder_network.py), run where the
reference is checked out ($DEEPARDS_REFERENCE, default: a `reference` directory beside this repository); never imported by a test:

    python tests/tools/make_golden_unet.py

Writes tests/golden/unet_n{4x16,5x24,3x224}.npz: AutoencoderNetwork(UNet(1)) in train mode on unet_ref.seeded_rows /
seeded_params: the output, the MSELoss against the input, every parameter's gradient (an ``oracle.weights.digest`` where it is
large), the encoder's output (``breath_block``), the state_dict key list, and the decisions of the float64 run as packed bits: the
14 ReLU masks (output > 0, in forward order) and the 3 pool winners (index % 2).  Per tensor the fp64 value and ``err32/<name>``,
the rel-l2 of the reference's own fp32 run against its fp64 run -- the yardstick of the GPU tests.  ``seed``: the first of 0, 1,
2, ... for which the fp32 run takes every decision as the float64 run does; ``near``: the decisions of the float64 run that lie
within 1e-4 of going the other way (unet_ref.near_count: ReLU pre-activations, pool gaps)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.environ.get('DEEPARDS_REFERENCE', os.path.join(os.path.dirname(ROOT), 'reference')))

from oracle.weights import digest                                                           # noqa: E402
import unet_ref as R                                                                        # noqa: E402
from deepards.models.unet import UNet                                                       # noqa: E402
from deepards.models.autoencoder_network import AutoencoderNetwork                          # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden')


def run(n, l, seed, dtype):
    torch.manual_seed(0)
    net = AutoencoderNetwork(UNet(1)).to(dtype)
    sd = net.state_dict()
    ref = R.network_state_dict(R.seeded_params(seed))
    assert list(sd.keys()) == list(ref.keys())
    for k, v in ref.items():
        assert tuple(sd[k].shape) == v.shape, k
        sd[k] = torch.tensor(v, dtype=dtype)
    net.load_state_dict(sd, strict=True)
    net.train()
    relu, pool, hooks = [], [], []
    base = net.base_network
    for name in R.BLOCKS:                                   # (inplace ReLUs: the hook sees the activated output)
        for i in (1, 3):
            hooks.append(getattr(base, name)[i].register_forward_hook(lambda m, i_, o: relu.append((o > 0).numpy().copy())))
    idx_pool = torch.nn.MaxPool1d(2, return_indices=True)
    hooks.append(base.maxpool.register_forward_hook(lambda m, i_, o: pool.append((idx_pool(i_[0])[1] % 2).numpy().astype(bool))))
    x = torch.tensor(R.seeded_rows(n, l, seed), dtype=dtype).view(1, n, 1, l)
    out = net(x, None)
    loss = torch.nn.MSELoss()(out, x.view(n, 1, l))
    loss.backward()
    for h in hooks:
        h.remove()
    vals = {'recon': out.detach().numpy(), 'loss': loss.detach().numpy().reshape(1)}
    for name, p in base.named_parameters():
        vals['grad/' + name] = p.grad.numpy()
    with torch.no_grad():
        vals['encoded'] = net.breath_block(x.view(n, 1, l)).numpy()
    return vals, (relu, pool), list(net.state_dict().keys())


def main():
    for n, l in R.MODEL_SHAPES:
        for seed in range(64):
            v64, dec64, keys = run(n, l, seed, torch.float64)
            v32, dec32, _ = run(n, l, seed, torch.float32)
            if R.decisions_differ(dec64, dec32) == 0:
                break
        else:
            raise RuntimeError('no seed whose fp32 run decides as the fp64 run')
        assert len(dec64[0]) == 14 and len(dec64[1]) == 3
        own = R.forward_backward(R.seeded_rows(n, l, seed), R.seeded_params(seed))
        rec = {'seed': np.array([seed]), 'shape': np.array([n, l]), 'keys': np.array(keys), 'near': np.array([R.near_count(own)])}
        for kind, masks in zip(('relu', 'pool'), dec64):
            for i, m in enumerate(masks):
                rec['%sbits/%d' % (kind, i)] = np.packbits(m.reshape(-1))
                rec['%sshape/%d' % (kind, i)] = np.array(m.shape)
        for k, a in v64.items():
            big = a.size > 1024
            rec[('dig/' if big else '') + k] = digest(a) if big else a
            rec['err32/' + k] = R.rel_l2(v32[k], a)
        rec['full/recon'] = v64['recon']
        if n * l <= 128:
            rec['full/encoded'] = v64['encoded']
        path = os.path.join(OUT, 'unet_n%dx%d.npz' % (n, l))
        np.savez_compressed(path, **rec)
        assert os.path.getsize(path) < (1 << 20), path
        print(path, os.path.getsize(path), 'seed', seed, 'near', int(rec['near'][0]),
              'err32 max', max(float(v) for k, v in rec.items() if k.startswith('err32/')))


if __name__ == '__main__':
    main()
