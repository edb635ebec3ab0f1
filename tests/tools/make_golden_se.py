"""Goldens of the se_resnet18 backbone from the REAL reference classes (models/senet.py, models/torch_cnn_linear_network.py),
run where the reference is checked out ($DEEPARDS_REFERENCE, default: a `reference` directory beside this repository); never
imported by a test:

    python tests/tools/make_golden_se.py

Writes tests/golden/se_model_b2.npz            CNNLinearNetwork(se_resnet18(), 20, 0) on se_ref.seeded_se_params with
                                               bn_bias_shift = 2 and the fc1 biases shifted by +2 (no ReLU decision can
                                               flip): fp64 logits, loss, gradient digests, the state_dict key list
       tests/golden/se_model_b2_unshifted.npz  the same without the shifts: logits and loss only
       tests/golden/se_block_cases.npz         one SEBasicBlock (identity and stride-2 entries) and layer0 at small
                                               shapes, inputs from se_ref.block_inputs / stem_inputs
(The file names keep clear of ``*net18_*.npz``, which the resnet18 / densenet18 golden tests collect.)
Per tensor: the fp64 value (``oracle.weights.digest`` of it where it is large, key ``dig/<name>``) and ``err32/<name>``, the
rel-l2 of the reference's own fp32 run against its fp64 run -- the yardstick of the GPU tests."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.environ.get('DEEPARDS_REFERENCE', os.path.join(os.path.dirname(ROOT), 'reference')))

from oracle.weights import seeded_batch, digest                                             # noqa: E402
import se_ref as R                                                                          # noqa: E402
from deepards.models.senet import SEBasicBlock, se_resnet18                                 # noqa: E402
from deepards.models.torch_cnn_linear_network import CNNLinearNetwork                       # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden')
SEED = 7


def save(name, rec):
    path = os.path.join(OUT, name)
    np.savez_compressed(path, **rec)
    size = os.path.getsize(path)
    assert size < (1 << 20), (name, size)
    print(name, size)


def put(rec, vals64, vals32):
    for k, a in vals64.items():
        big = a.size > 1024
        rec[('dig/' if big else '') + k] = digest(a) if big else a
        rec['err32/' + k] = R.rel_l2(vals32[k], a)


def model_case(name, bn_bias_shift, fc1_bias_shift, grads):
    x, tgt = seeded_batch(2, 20, SEED)
    params = R.seeded_se_params(SEED, 20, bn_bias_shift=bn_bias_shift, fc1_bias_shift=fc1_bias_shift)
    rec = dict(x=x, target=tgt, seed=SEED, bn_bias_shift=bn_bias_shift, fc1_bias_shift=fc1_bias_shift)
    vals = {}
    for dt in (torch.float64, torch.float32):
        model = CNNLinearNetwork(se_resnet18(), 20, 0)
        missing = model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=False)
        assert not missing.unexpected_keys and all('running_' in k or 'num_batches' in k for k in missing.missing_keys)
        assert [n for n, _ in model.named_parameters()] == [n for n, _, _ in R.se_param_spec(20)]
        if dt == torch.float64:
            rec['names'] = np.array(list(model.state_dict().keys()))
            rec['shapes'] = np.array(['x'.join(map(str, v.shape)) for v in model.state_dict().values()])
        model = model.to(dt).train()
        out = model(torch.from_numpy(x).to(dt), None)
        loss = torch.nn.BCEWithLogitsLoss()(out, torch.from_numpy(tgt).to(dt))
        v = dict(logits=out, loss=loss)
        if grads:
            loss.backward()
            v.update({'grad/' + n: q.grad for n, q in model.named_parameters()})
        vals[dt] = {k: a.detach().numpy().astype(np.float64) for k, a in v.items()}
    put(rec, vals[torch.float64], vals[torch.float32])
    print(name, 'loss', float(rec['loss']), 'err32 logits', rec['err32/logits'])
    save(name, rec)


def ncl(a):
    return torch.from_numpy(np.ascontiguousarray(np.transpose(a, (0, 2, 1))))


def block_case(rec, tag, rows, R_, l_out, planes, stride, seed):
    """One reference SEBasicBlock, window by window (a window of R_ rows is one BatchNorm batch, as the reference's per-window
    loop feeds it)."""
    x, params, dout = R.block_inputs(rows, R_, l_out, planes, stride, seed)
    rec[tag + '/x'] = x
    rec[tag + '/cfg'] = np.array([rows, R_, l_out, planes, stride, seed])
    vals = {}
    for dt in (torch.float64, torch.float32):
        cin = planes // stride
        ds = None
        if stride != 1:
            ds = torch.nn.Sequential(torch.nn.Conv1d(cin, planes, kernel_size=1, stride=stride, padding=0, bias=False),
                                     torch.nn.BatchNorm1d(planes))
        blk = SEBasicBlock(cin, planes, 1, 4, stride, ds)
        blk.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=False)
        blk = blk.to(dt).train()
        xt = ncl(x).to(dt).requires_grad_(True)
        outs = [blk(xt[w * R_:(w + 1) * R_]) for w in range(rows // R_)]
        out = torch.cat(outs, 0)
        out.backward(ncl(dout).to(dt))
        v = dict(out=out.permute(0, 2, 1), dx=xt.grad.permute(0, 2, 1))
        v.update({'grad/' + n: q.grad for n, q in blk.named_parameters()})
        vals[dt] = {tag + '/' + k: a.detach().numpy().astype(np.float64) for k, a in v.items()}
    put(rec, vals[torch.float64], vals[torch.float32])


def stem_case(rec, tag, rows, R_, lin, seed):
    """The reference's layer0 (conv k7 s2 -> BN -> ReLU -> MaxPool1d(3, 2, ceil_mode=True)) of se_resnet18, per window."""
    x, w, gamma, beta, dout = R.stem_inputs(rows, R_, lin, 64, seed)
    rec[tag + '/cfg'] = np.array([rows, R_, lin, 64, seed])
    vals = {}
    for dt in (torch.float64, torch.float32):
        l0 = se_resnet18().layer0
        l0.load_state_dict({'conv1.weight': torch.from_numpy(w), 'bn1.weight': torch.from_numpy(gamma),
                            'bn1.bias': torch.from_numpy(beta)}, strict=False)
        l0 = l0.to(dt).train()
        xt = torch.from_numpy(x).to(dt)[:, None, :]
        out = torch.cat([l0(xt[k * R_:(k + 1) * R_]) for k in range(rows // R_)], 0)
        out.backward(ncl(dout).to(dt))
        v = dict(out=out.permute(0, 2, 1), dw=l0.conv1.weight.grad, dgamma=l0.bn1.weight.grad, dbeta=l0.bn1.bias.grad)
        vals[dt] = {tag + '/' + k: a.detach().numpy().astype(np.float64) for k, a in v.items()}
    put(rec, vals[torch.float64], vals[torch.float32])


BLOCK_CASES = (('id_6x3x7x64', 6, 3, 7, 64, 1), ('id_4x2x56x64', 4, 2, 56, 64, 1), ('id_5x5x7x512', 5, 5, 7, 512, 1),
               ('id_4x2x5x512', 4, 2, 5, 512, 1), ('s2_6x3x28x128', 6, 3, 28, 128, 2), ('s2_4x2x14x256', 4, 2, 14, 256, 2),
               ('s2_5x5x7x512', 5, 5, 7, 512, 2))
STEM_CASES = (('stem_224', 4, 2, 224), ('stem_30', 6, 2, 30), ('stem_16', 4, 2, 16), ('stem_14', 4, 4, 14))


if __name__ == '__main__':
    rec = dict(blocks=np.array([c[0] for c in BLOCK_CASES]), stems=np.array([c[0] for c in STEM_CASES]))
    for i, (tag, rows, R_, l_out, planes, stride) in enumerate(BLOCK_CASES):
        block_case(rec, tag, rows, R_, l_out, planes, stride, 20 + i)
    for i, (tag, rows, R_, lin) in enumerate(STEM_CASES):
        stem_case(rec, tag, rows, R_, lin, 40 + i)
    save('se_block_cases.npz', rec)
    model_case('se_model_b2.npz', 2.0, 2.0, True)
    model_case('se_model_b2_unshifted.npz', 0.0, 0.0, False)
