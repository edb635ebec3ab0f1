"""Goldens of the autoencoder from the REAL reference classes (models/autoencoder_cnn.py, models/autoencoder_network.py), run
where the reference is checked out ($DEEPARDS_REFERENCE, default: a `reference` directory beside this repository); never
imported by a test:

    python tests/tools/make_golden_autoencoder.py

Writes tests/golden/autoencoder_n{4x16,6x32,3x224}.npz: AutoencoderNetwork(AutoencoderCNN()) in train mode on
ae_ref.seeded_rows / seeded_params (BatchNorm weights in [0.5, 1.5], every third negated; biases in [-0.5, 0.5]): the output,
the MSELoss against the input, every parameter's gradient (an ``oracle.weights.digest`` where it is large; for the conv biases
in front of a BatchNorm, whose gradient is exactly 0, only a marker ``exact_zero/<name>``), the running statistics after the step, the state_dict key list, the pool indices of the four stages as packed bits (index % 2), and at
(3, 224) the encoder's output.  Per tensor the fp64 value and ``err32/<name>``, the rel-l2 of the reference's own fp32 run
against its fp64 run -- the yardstick of the GPU tests.  ``seed``: the first of 0, 1, 2, ... for which the fp32 run takes
every pool decision as the float64 run does; ``near/<k>``: the pairs of stage k whose float64 gap is under 1e-4."""
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
import ae_ref as R                                                                          # noqa: E402
from deepards.models.autoencoder_cnn import AutoencoderCNN                                  # noqa: E402
from deepards.models.autoencoder_network import AutoencoderNetwork                          # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden')
SHAPES = ((4, 16), (6, 32), (3, 224))


def run(n, l, seed, dtype):
    torch.manual_seed(0)
    net = AutoencoderNetwork(AutoencoderCNN()).to(dtype)
    params = R.seeded_params(seed)
    sd = net.state_dict()
    for k, v in list(R.full_state_dict(params, 'base_network.').items()) + list(
            {('breath_block.' + k[len('encoder.'):]): v for k, v in R.full_state_dict(params).items() if k.startswith('encoder.')}.items()):
        assert k in sd and tuple(sd[k].shape) == v.shape, k
        sd[k] = torch.tensor(v, dtype=dtype)
    net.load_state_dict(sd)
    net.train()
    idx = []
    hook = net.base_network.maxpool.register_forward_hook(lambda m, i, o: idx.append(o[1].numpy().copy()))
    x = torch.tensor(R.seeded_rows(n, l, seed), dtype=dtype).view(1, n, 1, l)
    out = net(x, None)
    loss = torch.nn.MSELoss()(out, x.view(n, 1, l))
    loss.backward()
    hook.remove()
    vals = {'recon': out.detach().numpy(), 'loss': loss.detach().numpy().reshape(1)}
    for name, p in net.base_network.named_parameters():
        vals['grad/' + name] = p.grad.numpy()
    for k in range(1, 5):
        bn = getattr(net.base_network, 'bn%d' % k)
        vals['running_mean/bn%d' % k], vals['running_var/bn%d' % k] = bn.running_mean.numpy().copy(), bn.running_var.numpy().copy()
    if l // 16 >= 14:
        with torch.no_grad():           # (moves the running statistics again: taken after they were read)
            vals['encoded'] = net.breath_block(x.view(n, 1, l)).numpy()
    return vals, [(i % 2).astype(bool) for i in idx], list(net.state_dict().keys())


def main():
    for n, l in SHAPES:
        for seed in range(64):
            v64, sel64, keys = run(n, l, seed, torch.float64)
            v32, sel32, _ = run(n, l, seed, torch.float32)
            if all(np.array_equal(a, b) for a, b in zip(sel64, sel32)):
                break
        else:
            raise RuntimeError('no seed whose fp32 run decides as the fp64 run')
        gaps = R.model(R.seeded_rows(n, l, seed), R.seeded_params(seed))['gap']
        rec = {'seed': np.array([seed]), 'shape': np.array([n, l]), 'keys': np.array(keys)}
        for k, (s, g) in enumerate(zip(sel64, gaps)):
            rec['selbits/%d' % (k + 1)] = np.packbits(s.reshape(-1))
            rec['selshape/%d' % (k + 1)] = np.array(s.shape)
            rec['near/%d' % (k + 1)] = np.array([int((g < 1e-4).sum())])
        for k, a in v64.items():
            if k.startswith('grad/conv_down') and k.endswith('.bias'):
                # a bias in front of a train-mode BatchNorm: the gradient is exactly 0 and both runs hold rounding noise around
                # it, so there is no value and no err32 to record -- a marker with the largest |noise| of the fp64 run instead
                rec['exact_zero/' + k] = np.array([float(np.abs(a).max())])
                continue
            big = a.size > 1024
            rec[('dig/' if big else '') + k] = digest(a) if big else a
            rec['err32/' + k] = R.rel_l2(v32[k], a)
        rec['full/recon'] = v64['recon']
        path = os.path.join(OUT, 'autoencoder_n%dx%d.npz' % (n, l))
        np.savez_compressed(path, **rec)
        assert os.path.getsize(path) < (1 << 20), path
        print(path, os.path.getsize(path), 'seed', seed)


if __name__ == '__main__':
    main()
