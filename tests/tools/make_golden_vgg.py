"""Goldens of the vgg11 / vgg13 backbones from the REAL reference classes (models/vgg.py, models/torch_cnn_linear_network.py),
run where the reference is checked out ($DEEPARDS_REFERENCE, default: a `reference` directory beside this repository); never
imported by a test:

    python tests/tools/make_golden_vgg.py

Writes tests/golden/vgg_stage_cases.npz        slices of the reference's own make_layers (one conv / BatchNorm / ReLU [/ pool]
                                               stage each), window by window, on vgg_ref.stage_inputs / stage_params (NON-zero
                                               conv bias): out, dx, parameter gradients, running statistics after the forward
       tests/golden/vgg_stage_x700.npz         the input of the one long case (it would take the file above past its size)
       tests/golden/vgg_model_vgg11_nb4.npz    CNNLinearNetwork(vgg11_bn(), 4, 0) at B = 2, BN betas + 2: logits, loss, gradient
                                               digests; the first seed 0, 1, 2, ... whose fp32 run takes every ReLU and pool
                                               decision as the float64 run does, with margins 8 x the fp32 error of the tensor
                                               -- or, none of the first 64 having them, the agreeing seed with the largest
                                               margins, which the file records (model_margins below)
       tests/golden/vgg_model_vgg11_nb{2|1}.npz  the same at fewer breaths a window, where the 8 x margins are reached
       tests/golden/vgg_model_vgg1{1,3}_nb20.npz   logits and loss only, the state_dict key list
       tests/golden/vgg_backbone_512.npz       vgg11_bn() on one (20, 1, 512) window: the (20, 3584) features
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
import vgg_ref as R                                                                         # noqa: E402
from deepards.models.vgg import make_layers, cfgs, vgg11_bn, vgg13_bn                       # noqa: E402
from deepards.models.torch_cnn_linear_network import CNNLinearNetwork                       # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden')
NETS = {'vgg11': vgg11_bn, 'vgg13': vgg13_bn}

# (tag, rows, R, Lin, Cin, C, pooled, cfg, first module of the slice): every shape two windows or more
STAGE_CASES = (('s64_64p_2', 4, 2, 2, 64, 64, True, 'B', 3), ('s64_128p_3', 6, 3, 3, 64, 128, True, 'A', 4),
               ('s256_256p_7', 4, 2, 7, 256, 256, True, 'A', 11), ('s128_256_15', 6, 3, 15, 128, 256, False, 'A', 8),
               ('s128_256p_15', 6, 3, 15, 128, 256, True, 'A', 8), ('s512_512p_14', 4, 2, 14, 512, 512, True, 'A', 18),
               ('s512_512_14', 4, 2, 14, 512, 512, False, 'A', 22), ('s64_128p_700', 4, 2, 700, 64, 128, True, 'A', 4),
               ('first_224p', 8, 4, 224, 1, 64, True, 'A', 0), ('first_30p', 6, 3, 30, 1, 64, True, 'A', 0),
               ('first_30', 6, 3, 30, 1, 64, False, 'B', 0))


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


def stage_case(rec, xrec, i, tag, rows, R_, lin, cin, c, pool, cfg, first):
    seed = 60 + i
    x = R.stage_inputs(rows, R_, lin, cin, c, pool, seed)
    p = R.stage_params(cin, c, seed)
    dout = R.stage_dout(rows, lin, c, pool, seed)
    (xrec if x.size > 100000 else rec)[tag + '/x'] = x
    rec[tag + '/cfg'] = np.array([rows, R_, lin, cin, c, int(pool), seed])
    vals = {}
    for dt in (torch.float64, torch.float32):
        layers = make_layers(cfgs[cfg], batch_norm=True)
        mods = list(layers[first:first + 3])
        assert (mods[0].in_channels, mods[0].out_channels) == (cin, c)
        if pool:
            mods.append(next(m for m in layers if isinstance(m, torch.nn.MaxPool1d)))
        seq = torch.nn.Sequential(*mods)
        seq.load_state_dict({'0.weight': torch.from_numpy(p['w']), '0.bias': torch.from_numpy(p['b']),
                             '1.weight': torch.from_numpy(p['gamma']), '1.bias': torch.from_numpy(p['beta'])}, strict=False)
        seq = seq.to(dt).train()
        xt = ncl(x).to(dt).requires_grad_(True)
        out = torch.cat([seq(xt[w * R_:(w + 1) * R_]) for w in range(rows // R_)], 0)
        out.backward(ncl(dout).to(dt))
        v = dict(out=out.permute(0, 2, 1), dx=xt.grad.permute(0, 2, 1), dw=seq[0].weight.grad, db=seq[0].bias.grad,
                 dgamma=seq[1].weight.grad, dbeta=seq[1].bias.grad, running_mean=seq[1].running_mean, running_var=seq[1].running_var)
        assert int(seq[1].num_batches_tracked) == rows // R_
        vals[dt] = {tag + '/' + k: a.detach().numpy().astype(np.float64) for k, a in v.items()}
    mine = R.stage_case(x, p, R_, pool, dout)
    for k, a in vals[torch.float64].items():           # the formulas of vgg_ref against the reference's modules
        e = R.rel_l2(mine[k.split('/')[1]].numpy(), a)
        assert e < 1e-10, (k, e)
    rec[tag + '/margins'] = np.array(R.decision_margins(mine['z'], pool))
    print(tag, 'margins', rec[tag + '/margins'], 'max |db|', float(np.abs(vals[torch.float64][tag + '/db']).max()))
    put(rec, vals[torch.float64], vals[torch.float32])


def run_model(arch, nb, params, x, tgt, dt, grads, taps=None):
    model = CNNLinearNetwork(NETS[arch](), nb, 0)
    missing = model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=False)
    assert not missing.unexpected_keys and all('running_' in k or 'num_batches' in k for k in missing.missing_keys)
    assert [n for n, _ in model.named_parameters()] == [n for n, _, _ in R.vgg_param_spec(arch, nb)]
    sd = model.state_dict()
    names, shapes = np.array(list(sd.keys())), np.array(['x'.join(map(str, v.shape)) for v in sd.values()])
    model = model.to(dt).train()
    if taps is not None:                                # BatchNorm outputs (the ReLU is in place: copied before it runs)
        feats = list(model.breath_block.features)
        for i, m in enumerate(feats):
            if isinstance(m, torch.nn.BatchNorm1d):
                pooled = i + 2 < len(feats) and isinstance(feats[i + 2], torch.nn.MaxPool1d)
                m.register_forward_hook(lambda _m, _i, o, pooled=pooled: taps.append((o.detach().clone().double(), pooled)))
    out = model(torch.from_numpy(x).to(dt), None)
    loss = torch.nn.BCEWithLogitsLoss()(out, torch.from_numpy(tgt).to(dt))
    v = dict(logits=out, loss=loss)
    if grads:
        loss.backward()
        v.update({'grad/' + n: q.grad for n, q in model.named_parameters()})
    return {k: a.detach().numpy().astype(np.float64) for k, a in v.items()}, names, shapes


def decisions_agree(t64, t32):
    """-> (ok, smallest |pre-activation| / fp32 error, smallest pool gap / fp32 error) over all BatchNorm outputs (N, C, L)."""
    ok, rz, rg = True, np.inf, np.inf
    for (a, pooled), (b, _) in zip(t64, t32):
        err = float((a - b).abs().max())
        ok = ok and bool(((a > 0) == (b > 0)).all())
        rz = min(rz, float(a.abs().min()) / err)
        if pooled:
            l2 = a.shape[2] // 2 * 2
            pa, pb = (torch.relu(t[:, :, :l2]).reshape(t.shape[0], t.shape[1], l2 // 2, 2) for t in (a, b))
            ok = ok and bool(((pa[..., 0] >= pa[..., 1]) == (pb[..., 0] >= pb[..., 1])).all())
            live = pa.amax(3) > 0
            rg = min(rg, float((pa[..., 0] - pa[..., 1]).abs()[live].min()) / err)
    return ok, rz, rg


WANT_RATIO, MAX_SEEDS = 8.0, 64


def model_margins(nb):
    """CNNLinearNetwork(vgg11_bn(), nb, 0) at B = 2, betas + 2.  Seeds 0, 1, 2, ...: the first whose fp32 run takes every ReLU
    and pool decision as the float64 run does with both margin ratios (smallest |pre-activation|, smallest pool gap, each over
    the largest fp32-against-float64 difference of its tensor) >= WANT_RATIO.  Measured at nb = 4: over its 802 816 decisions no
    seed below MAX_SEEDS has both (the smallest of ~400 000 pool gaps is ~1e-5, the fp32 error of those tensors ~5e-6); then the
    agreeing seed with the largest smaller ratio is taken and what it has is recorded (``margin_ratio``, ``margin_wanted``,
    ``margin_met``).  A smaller nb has fewer decisions and so larger smallest margins: the 8 x case is made there."""
    seen, walked = [], 0
    for seed in range(MAX_SEEDS):
        x, tgt = seeded_batch(2, nb, seed)
        params = R.seeded_vgg_params('vgg11', seed, nb, bn_bias_shift=2.0)
        t64, t32 = [], []
        with torch.no_grad():
            run_model('vgg11', nb, params, x, tgt, torch.float64, False, t64)
            run_model('vgg11', nb, params, x, tgt, torch.float32, False, t32)
        ok, rz, rg = decisions_agree(t64, t32)
        walked += 1
        n_dec = sum(int(a.numel()) for a, _ in t64)
        print('vgg11 nb%d seed' % nb, seed, 'decisions', n_dec, 'agree', ok, 'margin / fp32 error: pre-activations %.1f pool gaps %.1f' % (rz, rg))
        if ok:
            seen.append((min(rz, rg), -seed, rz, rg))
        if ok and rz >= WANT_RATIO and rg >= WANT_RATIO:
            break
    _, seed, rz, rg = max(seen)
    seed = -seed
    x, tgt = seeded_batch(2, nb, seed)
    params = R.seeded_vgg_params('vgg11', seed, nb, bn_bias_shift=2.0)
    v64, names, shapes = run_model('vgg11', nb, params, x, tgt, torch.float64, True)
    v32, _, _ = run_model('vgg11', nb, params, x, tgt, torch.float32, True)
    met = bool(rz >= WANT_RATIO and rg >= WANT_RATIO)
    print('vgg11 nb%d: seed' % nb, seed, 'ratios', rz, rg, 'met', met)
    rec = dict(x=x, target=tgt, seed=seed, bn_bias_shift=2.0, names=names, shapes=shapes, decisions=n_dec,
               margin_ratio=np.array([rz, rg]), margin_wanted=WANT_RATIO, margin_met=met, seeds_walked=walked,
               seeds_agreeing=len(seen))
    put(rec, v64, v32)
    save('vgg_model_vgg11_nb%d.npz' % nb, rec)
    return met


def model_nb20(arch, seed=7):
    x, tgt = seeded_batch(2, 20, seed)
    params = R.seeded_vgg_params(arch, seed, 20)
    v64, names, shapes = run_model(arch, 20, params, x, tgt, torch.float64, False)
    v32, _, _ = run_model(arch, 20, params, x, tgt, torch.float32, False)
    mine, mloss = R.model_forward(x, tgt, params, arch)
    assert R.rel_l2(mine.numpy(), v64['logits']) < 1e-10 and abs(float(mloss) - float(v64['loss'])) < 1e-10
    rec = dict(x=x, target=tgt, seed=seed, bn_bias_shift=0.0, names=names, shapes=shapes,
               n_params=sum(int(np.prod(s)) for n, s, _ in R.vgg_param_spec(arch, 20) if not n.startswith('linear_final')))
    put(rec, v64, v32)
    print(arch, 'nb20 loss', float(rec['loss']), 'err32 logits', rec['err32/logits'])
    save('vgg_model_%s_nb20.npz' % arch, rec)


def backbone_512(seed=11):
    x = np.random.default_rng([seed, 512]).standard_normal((20, 1, 512)).astype(np.float32)
    params = R.seeded_vgg_params('vgg11', seed, 20)
    vals = {}
    for dt in (torch.float64, torch.float32):
        net = vgg11_bn()
        net.load_state_dict({k[len('breath_block.'):]: torch.from_numpy(v) for k, v in params.items() if k.startswith('breath_block.')},
                            strict=False)
        vals[dt] = dict(feat=net.to(dt).train()(torch.from_numpy(x).to(dt)).detach().numpy().astype(np.float64))
    mine = R.backbone_forward(torch.from_numpy(x).double(), {k: torch.from_numpy(v).double() for k, v in params.items()}, 'vgg11', 20)
    assert R.rel_l2(mine.numpy(), vals[torch.float64]['feat']) < 1e-10
    rec = dict(x=x, seed=seed)
    put(rec, vals[torch.float64], vals[torch.float32])
    save('vgg_backbone_512.npz', rec)


if __name__ == '__main__':
    if 'models-only' not in sys.argv[1:]:
        rec, xrec = dict(stages=np.array([c[0] for c in STAGE_CASES])), {}
        for i, case in enumerate(STAGE_CASES):
            stage_case(rec, xrec, i, *case)
        save('vgg_stage_cases.npz', rec)
        save('vgg_stage_x700.npz', xrec)
    if 'nb4' in sys.argv[1:] or 'models-only' not in sys.argv[1:]:
        model_margins(4)
    if 'nb4-only' in sys.argv[1:]:
        sys.exit(0)
    for nb in (2, 1):                                   # the largest of these that reaches the 8 x margins
        if model_margins(nb):
            break
        os.remove(os.path.join(OUT, 'vgg_model_vgg11_nb%d.npz' % nb))
    if 'margins-only' in sys.argv[1:]:
        sys.exit(0)
    model_nb20('vgg11')
    model_nb20('vgg13')
    backbone_512()
