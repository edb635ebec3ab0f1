"""Goldens of the breath-metadata regressor from the REAL reference classes (models/torch_cnn_bm_regressor.py on its resnet18 /
densenet18), run where the reference is checked out ($DEEPARDS_REFERENCE, default: a `reference` directory beside this
repository); never imported by a test:

    python tests/tools/make_golden_regressor.py

Writes tests/golden/regressor_r<R>_<net>.npz (the rows in front: the whole-model tests of cnn_linear collect every
'*net18_*.npz' golden) for R = 6, 5 (odd: the fused stem's row-pair rule does not hold) and 46 (the first
even R whose first residual stage, one window of R * 56 positions at 64 channels, leaves the single-pass BatchNorm geometry:
``hip_ops.bn_single_pass(1, R * 56, 64)`` holds up to R = 44): CNNRegressor(net, 9) in train mode (dropout off) on
``regressor_case``: the (R, 9) output, the MSELoss, every parameter's gradient (an ``oracle.weights.digest`` where it is large) --
per tensor the float64 value and ``err32/<name>``, the rel-l2 of the reference's own float32 run against its float64 run -- and
the ReLU decisions of the float64 run as packed bits (``relu/<k>``: output > 0 of the k-th ReLU call, in forward order)."""
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
from regressor_case import regressor_case, M_OUT                                            # noqa: E402
from regress_ref import rel_l2                                                              # noqa: E402
from deepards.models.torch_cnn_bm_regressor import CNNRegressor                             # noqa: E402
from deepards.models.resnet import resnet18                                                 # noqa: E402
from deepards.models.densenet import densenet18                                             # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden')
CASES = [(net, r) for net in ('resnet18', 'densenet18') for r in (6, 5, 46)]


def run(net, r, dtype):
    case = regressor_case(net, r)
    bb = resnet18() if net == 'resnet18' else densenet18(drop_rate=0)
    model = CNNRegressor(bb, M_OUT).to(dtype)
    missing = model.load_state_dict({k: torch.tensor(v, dtype=dtype) for k, v in case['params'].items()}, strict=False)
    assert not missing.unexpected_keys
    assert all('running_' in k or 'num_batches' in k or k.split('.')[-2] in ('conv1_alt', 'conv2', 'bn2')
               for k in missing.missing_keys), missing
    model.train()
    relu, hooks = [], []
    for mod in model.modules():
        if isinstance(mod, torch.nn.ReLU):                  # (inplace ReLUs: the hook sees the activated output)
            hooks.append(mod.register_forward_hook(lambda m, i_, o: relu.append((o > 0).numpy().copy())))
    out = model(torch.tensor(case['x'], dtype=dtype), None)
    loss = torch.nn.MSELoss()(out, torch.tensor(case['target'], dtype=dtype))
    loss.backward()
    for h in hooks:
        h.remove()
    vals = {'out': out.detach().numpy(), 'loss': loss.detach().numpy().reshape(1)}
    for name, p in model.named_parameters():
        if p.grad is not None:
            vals['grad/' + name] = p.grad.numpy()
    return vals, relu, list(model.state_dict().keys())


def main():
    os.makedirs(OUT, exist_ok=True)
    for net, r in CASES:
        v64, relu, keys = run(net, r, torch.float64)
        v32, _, _ = run(net, r, torch.float32)
        rec = {'net': net, 'rows': r, 'keys': np.array(keys)}
        for k, v in v64.items():
            rec[k] = digest(v) if k.startswith('grad/') else v
            rec['err32/' + k] = np.float64(rel_l2(v32[k], v))
        for i, m in enumerate(relu):
            rec['relu/%d' % i] = np.packbits(m.reshape(-1))
            rec['relu_shape/%d' % i] = np.array(m.shape)
        path = os.path.join(OUT, 'regressor_r%d_%s.npz' % (r, net))
        np.savez_compressed(path, **rec)
        print('%s  %d tensors, %d ReLU calls, %.0f KB; loss %.6f; err32 out %.2e, worst gradient %.2e' %
              (os.path.basename(path), len(v64), len(relu), os.path.getsize(path) / 1024.0, float(v64['loss'][0]),
               rec['err32/out'], max(rec['err32/' + k] for k in v64 if k.startswith('grad/'))))


if __name__ == '__main__':
    main()
