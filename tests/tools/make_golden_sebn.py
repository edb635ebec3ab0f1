"""Goldens of the se_resnet50 / 101 / 152 backbones from the REAL reference classes (models/senet.py,
models/torch_cnn_linear_network.py), run where the reference is checked out ($DEEPARDS_REFERENCE, default: a `reference`
directory beside this repository); never imported by a test:

    python tests/tools/make_golden_sebn.py [blocks] [models] [grads]

Writes tests/golden/sebn_block_<tag>.npz       one SEResNetBottleneck, window by window, inputs from sebn_ref.block_inputs
                                               (the nudged x is stored: finding it again takes up to 81 oracle passes)
       tests/golden/sebn_model_<net>_nb<NB>[_shifted].npz   CNNLinearNetwork(<net>(), NB, 0) on sebn_ref.seeded_params (shifted:
                                               BatchNorm and fc1 biases + 2): fp64 logits and loss, the state_dict key list
                                               and shapes; se_resnet50 at NB = 20 both ways, se_resnet101 / 152 at NB = 2 shifted
       tests/golden/sebn_model_se_resnet50_b2_grads.npz     NB = 2, BatchNorm and fc1 biases shifted by +2, the input moved
                                               until every ReLU pre-activation and every stem-pool top-two gap of the fp64 run is
                                               at least 1e-4: logits, loss and a digest of every parameter gradient; ``unpinned``
                                               lists the tensors whose err32 exceeds 2.5e-5 (at most 4)
(The names keep clear of ``*net18_*.npz``, which the resnet18 / densenet18 golden tests collect.)
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
import sebn_ref as R                                                                        # noqa: E402
import se_ref as S                                                                          # noqa: E402
from deepards.models import senet as ref_senet                                              # noqa: E402
from deepards.models.torch_cnn_linear_network import CNNLinearNetwork                       # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden')
SEED = 7
UNPINNED_ABOVE, UNPINNED_MAX = 2.5e-5, 4
# (tag, rows, R, l_out, cin, planes, stride, downsample)
BLOCK_CASES = (('id_4x2x56x256', 4, 2, 56, 256, 64, 1, False), ('id_6x3x5x1024', 6, 3, 5, 1024, 256, 1, False),
               ('id_5x5x7x2048', 5, 5, 7, 2048, 512, 1, False), ('e1_4x2x56x256', 4, 2, 56, 64, 64, 1, True),
               ('s2_6x3x28x512', 6, 3, 28, 256, 128, 2, True), ('s2_6x3x14x1024', 6, 3, 14, 512, 256, 2, True),
               ('s2_5x5x7x2048', 5, 5, 7, 1024, 512, 2, True))


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


def ncl(a):
    return torch.from_numpy(np.ascontiguousarray(np.transpose(a, (0, 2, 1))))


def block_case(i, tag, rows, R_, l_out, cin, planes, stride, ds):
    """One reference SEResNetBottleneck, window by window (a window of R_ rows is one BatchNorm batch)."""
    x, params, dout, steps = R.block_inputs(rows, R_, l_out, cin, planes, stride, ds, 60 + i)
    rec = dict(x=x, cfg=np.array([rows, R_, l_out, cin, planes, stride, int(ds), 60 + i]), steps=steps)
    vals, signs = {}, {}
    for dt in (torch.float64, torch.float32):
        dsm = None
        if ds:
            dsm = torch.nn.Sequential(torch.nn.Conv1d(cin, planes * 4, kernel_size=1, stride=stride, padding=0, bias=False),
                                      torch.nn.BatchNorm1d(planes * 4))
        blk = ref_senet.SEResNetBottleneck(cin, planes, 1, 16, stride, dsm)
        missing = blk.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=False)
        assert not missing.unexpected_keys and all('running_' in k or 'num_batches' in k for k in missing.missing_keys)
        blk = blk.to(dt).train()
        xt = ncl(x).to(dt).requires_grad_(True)
        out = torch.cat([blk(xt[w * R_:(w + 1) * R_]) for w in range(rows // R_)], 0)
        out.backward(ncl(dout).to(dt))
        v = dict(out=out.permute(0, 2, 1), dx=xt.grad.permute(0, 2, 1))
        v.update({'grad/' + n: q.grad for n, q in blk.named_parameters()})
        vals[dt] = {k: a.detach().numpy().astype(np.float64) for k, a in v.items()}
        signs[dt] = vals[dt]['out'] > 0
    assert np.array_equal(signs[torch.float64], signs[torch.float32]), 'the reference\'s fp32 run takes other output decisions'
    # ... and the hidden decisions: the oracle in float32 against float64 at every ReLU site
    for dt in (torch.float64, torch.float32):
        taps = {}
        R.block_forward(R._t(x, dt), {k: R._t(a, dt) for k, a in params.items()}, stride, R_, taps=taps)
        signs[dt] = {k: (a > 0).numpy() for k, a in taps.items()}
    assert all(np.array_equal(signs[torch.float64][k], signs[torch.float32][k]) for k in signs[torch.float64])
    put(rec, vals[torch.float64], vals[torch.float32])
    print(tag, 'steps', steps, 'max err32', max(float(v) for k, v in rec.items() if k.startswith('err32/')))
    save('sebn_block_%s.npz' % tag, rec)


def ref_model(net, nb, params, dt):
    model = CNNLinearNetwork(getattr(ref_senet, net)(), nb, 0)
    missing = model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=False)
    assert not missing.unexpected_keys and all('running_' in k or 'num_batches' in k for k in missing.missing_keys)
    assert [n for n, _ in model.named_parameters()] == [n for n, _, _ in R.param_spec(net, nb)]
    return model.to(dt).train()


def model_case(name, net, nb, shift, x=None, grads=False):
    xs, tgt = seeded_batch(2, nb, SEED)
    x = xs if x is None else x
    params = R.seeded_params(net, SEED, nb, bn_bias_shift=shift, fc1_bias_shift=shift)
    rec = dict(x=x, target=tgt, seed=SEED, bn_bias_shift=shift, fc1_bias_shift=shift, nb=nb)
    vals = {}
    for dt in (torch.float64, torch.float32):
        model = ref_model(net, nb, params, dt)
        if dt == torch.float64:
            rec['names'] = np.array(list(model.state_dict().keys()))
            rec['shapes'] = np.array(['x'.join(map(str, v.shape)) for v in model.state_dict().values()])
        out = model(torch.from_numpy(x).to(dt), None)
        loss = torch.nn.BCEWithLogitsLoss()(out, torch.from_numpy(tgt).to(dt))
        v = dict(logits=out, loss=loss)
        if grads:
            loss.backward()
            v.update({'grad/' + n: q.grad for n, q in model.named_parameters()})
        vals[dt] = {k: a.detach().numpy().astype(np.float64) for k, a in v.items()}
    put(rec, vals[torch.float64], vals[torch.float32])
    if grads:
        errs = {k[6:]: float(v) for k, v in rec.items() if k.startswith('err32/grad/')}
        unpinned = sorted(k for k, v in errs.items() if v > UNPINNED_ABOVE)
        assert len(unpinned) <= UNPINNED_MAX, unpinned
        rec['unpinned'] = np.array(unpinned)
        # the yardstick of an unpinned tensor: the norm of the same module's weight gradient
        for k in unpinned:
            wk = 'grad/' + k[5:].rsplit('.', 1)[0] + '.weight'
            rec['wnorm/' + k] = float(np.linalg.norm(vals[torch.float64][wk]))
            rec['abs32/' + k] = float(np.linalg.norm(vals[torch.float32][k] - vals[torch.float64][k]))
        print(name, 'err32 median', float(np.median(list(errs.values()))), 'unpinned', unpinned)
    print(name, 'loss', float(rec['loss']), 'err32 logits', rec['err32/logits'], 'loss', rec['err32/loss'])
    save(name, rec)


def decided_input(net, nb, shift, margin=1e-4):
    """The seeded batch moved until every ReLU pre-activation and every stem-pool top-two gap (windows whose maximum is
    positive) of the fp64 oracle is at least ``margin``; asserts that the oracle's fp32 run takes the same decisions."""
    x, _ = seeded_batch(2, nb, SEED)
    params = R.seeded_params(net, SEED, nb, bn_bias_shift=shift, fc1_bias_shift=shift)
    b = x.shape[0]

    def sites(xt, dt):
        p = {k: R._t(v, dt) for k, v in params.items()}
        taps = []
        R.backbone_forward(net, xt.reshape(b * nb, 1, -1), p, nb, taps=taps)
        a = torch.relu(taps[0])                                         # the stem's post-ReLU map: pool windows {2j, 2j+1, 2j+2}
        l = a.shape[1]
        lp = S.pool_len_ceil(l)
        idx = torch.arange(lp)[:, None] * 2 + torch.arange(3)[None, :]
        ok = idx < l
        win = torch.where(ok[None, :, :, None], a[:, idx.clamp(max=l - 1), :], torch.full((), -1.0, dtype=dt))
        top = torch.topk(win, 2, dim=2).values
        gap = torch.where(top[:, :, 0] > 0, top[:, :, 0] - top[:, :, 1], torch.ones((), dtype=dt))
        return taps, gap, win.argmax(2)

    for step in range(400):
        xt = torch.tensor(x.astype(np.float32), dtype=torch.float64, requires_grad=True)
        taps, gap, _ = sites(xt, torch.float64)
        hit = None
        for v in taps + [gap]:
            idx = torch.nonzero(v.detach().abs() < margin)
            if idx.numel():
                hit = v[tuple(idx[0].tolist())]
                break
        if hit is None:
            break
        (gr,) = torch.autograd.grad(hit, xt)
        hv = float(hit.detach())
        target = 2 * margin * (1.0 if hv >= 0 else -1.0)
        x = x.astype(np.float32).astype(np.float64) + (gr * ((target - hv) / float((gr * gr).sum()))).numpy() * 1.05
    else:
        raise AssertionError('decided_input: offenders remain')
    x = x.astype(np.float32)
    with torch.no_grad():
        t64, _, a64 = sites(torch.from_numpy(x).double(), torch.float64)
        t32, _, a32 = sites(torch.from_numpy(x), torch.float32)
    assert all(torch.equal(p > 0, q > 0) for p, q in zip(t64, t32)) and torch.equal(a64, a32), 'fp32 takes other decisions'
    print('decided_input', net, 'steps', step)
    return x


if __name__ == '__main__':
    what = set(sys.argv[1:]) or {'blocks', 'models', 'grads'}
    if 'blocks' in what:
        for i, case in enumerate(BLOCK_CASES):
            block_case(i, *case)
    if 'models' in what:
        # (shifted: without the shifts the reference's own fp32 logits of these two are 1.2e-4 / 2.4e-4 from its fp64 ones at
        # NB = 2 -- ReLU decisions flip --, beyond the 1e-4 ceiling of the GPU tests' bound: nothing could be held to them)
        for net in ('se_resnet101', 'se_resnet152'):
            model_case('sebn_model_%s_nb2_shifted.npz' % net, net, 2, 2.0)
        model_case('sebn_model_se_resnet50_nb20.npz', 'se_resnet50', 20, 0.0)
        model_case('sebn_model_se_resnet50_nb20_shifted.npz', 'se_resnet50', 20, 2.0)
    if 'grads' in what:
        model_case('sebn_model_se_resnet50_b2_grads.npz', 'se_resnet50', 2, 2.0, x=decided_input('se_resnet50', 2, 2.0), grads=True)
