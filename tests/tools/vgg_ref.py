"""Float64 formulas of the VGG backbones (reference models/vgg.py) on channels-last (rows, L, C) maps with BatchNorm windows of
R rows, the seeded parameters of ``CNNLinearNetwork(vgg11_bn() | vgg13_bn(), nb, 0)`` (3 M values: regenerated from a seed,
never stored) and the seeded stage cases of tests/test_vgg_gpu.py.  torch on the CPU only; nothing of the package under test
and nothing of the reference is imported.  tests/tools/make_golden_vgg.py ties these formulas to the reference's own classes
(the goldens hold digests of the reference's results, which tests/test_vgg_cpu.py compares with what this file computes)."""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

CFGS = {'vgg11': [64, 'M', 128, 'M', 256, 256, 'M', 512, 512, 'M', 512, 512, 'M'],
        'vgg13': [64, 64, 'M', 128, 128, 'M', 256, 256, 'M', 512, 512, 'M', 512, 512, 'M']}
MARGIN = 1e-3
MOMENTUM, EPS = 0.1, 1e-5


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    nb = float(np.linalg.norm(b))
    return float(np.linalg.norm(a - b) / (nb if nb > 1e-9 else 1.0))      # ~zero references: absolute


def _t(a, dtype):
    return a.to(dtype) if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a)).to(dtype)


# ---- the module tree ------------------------------------------------------------------------------------------------------
def stage_list(arch):
    """[(index of the conv in ``features``, cin, cout, pooled)]"""
    out, cin, i, cfg = [], 1, 0, CFGS[arch]
    for k, v in enumerate(cfg):
        if v == 'M':
            i += 1
            continue
        out.append((i, cin, v, k + 1 < len(cfg) and cfg[k + 1] == 'M'))
        cin, i = v, i + 3
    return out


def vgg_param_spec(arch, n_sub_batches=20):
    """(name, shape, kind) in the reference's ``named_parameters()`` order."""
    out = []
    for i, cin, c, _ in stage_list(arch):
        p = 'breath_block.features.'
        out += [(p + '%d.weight' % i, (c, cin, 3), 'conv'), (p + '%d.bias' % i, (c,), 'conv_b'),
                (p + '%d.weight' % (i + 1), (c,), 'bn_w'), (p + '%d.bias' % (i + 1), (c,), 'bn_b')]
    return out + [('linear_final.weight', (2, 3584 * n_sub_batches), 'lin_w'), ('linear_final.bias', (2,), 'lin_b')]


def state_dict_spec(arch, n_sub_batches=20):
    """(key, shape) of the whole state_dict, buffers included, in order."""
    out = []
    for name, shape, kind in vgg_param_spec(arch, n_sub_batches):
        out.append((name, shape))
        if kind == 'bn_b':
            p = name[:-len('bias')]
            out += [(p + 'running_mean', shape), (p + 'running_var', shape), (p + 'num_batches_tracked', ())]
    return out


def seeded_value(name, shape, kind, seed, bn_bias_shift=0.0):
    """One parameter from the name-keyed RNG of oracle/weights.py (float64).  The conv biases are NOT the reference's zeros:
    a bias that is dropped or mishandled must show."""
    rng = np.random.default_rng([seed, zlib.crc32(name.encode())])
    if kind == 'conv':
        return rng.standard_normal(shape) * np.sqrt(2.0 / (shape[2] * shape[0]))
    if kind == 'conv_b':
        return rng.uniform(-0.5, 0.5, shape)
    if kind == 'bn_w':
        return rng.uniform(0.5, 1.5, shape)
    if kind == 'bn_b':
        return rng.standard_normal(shape) * 0.1 + bn_bias_shift
    if kind == 'lin_w':
        bound = 1.0 / np.sqrt(shape[1])
        return rng.uniform(-bound, bound, shape)
    return rng.uniform(-0.01, 0.01, shape)


def seeded_vgg_params(arch, seed=0, n_sub_batches=20, dtype=np.float32, bn_bias_shift=0.0):
    return {name: seeded_value(name, shape, kind, seed, bn_bias_shift).astype(dtype)
            for name, shape, kind in vgg_param_spec(arch, n_sub_batches)}


# ---- one stage: Conv1d(k3, p1, bias) -> BatchNorm1d per window -> ReLU [-> MaxPool1d(2, 2)] -----------------------------------
def window_stats(y, R, eps=EPS):
    rows, l, c = y.shape
    yw = y.reshape(rows // R, R * l, c)
    mean = yw.mean(1)
    var = ((yw - mean[:, None]) ** 2).mean(1)
    return mean, var, 1.0 / torch.sqrt(var + eps)


def running_after(mean, var, n, momentum=MOMENTUM):
    """running_mean / running_var (from 0 / 1) after one momentum update per window, in window order (unbiased variance)."""
    rm, rv = torch.zeros_like(mean[0]), torch.ones_like(var[0])
    for w in range(mean.shape[0]):
        rm = (1 - momentum) * rm + momentum * mean[w]
        rv = (1 - momentum) * rv + momentum * var[w] * (n / (n - 1.0))
    return rm, rv


def maxpool2(a):
    """MaxPool1d(2, 2) of (rows, L, C): floor(L / 2) pairs, an odd last position dropped."""
    rows, l, c = a.shape
    return a[:, :l // 2 * 2].reshape(rows, l // 2, 2, c).amax(2)


def stage_forward(x, w, b, gamma, beta, R, pool, eps=EPS):
    """x (rows, L, Cin) (Cin = 1: the raw rows) -> dict(y = conv + b, z = bn(y), out, mean, var)."""
    y = F.conv1d(x.permute(0, 2, 1), w, b, padding=1).permute(0, 2, 1)
    rows, l, c = y.shape
    mean, var, invstd = window_stats(y, R, eps)
    z = (((y.reshape(rows // R, R * l, c) - mean[:, None]) * invstd[:, None]) * gamma + beta).reshape(rows, l, c)
    a = torch.relu(z)
    return dict(y=y, z=z, out=maxpool2(a) if pool else a, mean=mean, var=var)


def stage_case(x, p, R, pool, dout, dtype=torch.float64):
    """Forward + backward of one stage -> out, dx, dw, db, dgamma, dbeta, running_mean, running_var (after the forward), z."""
    xt = _t(x, dtype).requires_grad_(True)
    q = {k: _t(v, dtype).requires_grad_(True) for k, v in p.items()}
    r = stage_forward(xt, q['w'], q['b'], q['gamma'], q['beta'], R, pool)
    r['out'].backward(_t(dout, dtype))
    rm, rv = running_after(r['mean'].detach(), r['var'].detach(), R * r['y'].shape[1])
    return dict(out=r['out'].detach(), dx=xt.grad, dw=q['w'].grad, db=q['b'].grad, dgamma=q['gamma'].grad, dbeta=q['beta'].grad,
                running_mean=rm, running_var=rv, z=r['z'].detach())


def decision_margins(z, pool):
    """(smallest |pre-activation|, smallest gap between the two members of a pool pair that are not both negative) of z (rows, L, C)."""
    z = _t(z, torch.float64)
    m = float(z.abs().min())
    if not pool:
        return m, float('inf')
    rows, l, c = z.shape
    pr = torch.relu(z[:, :l // 2 * 2]).reshape(rows, l // 2, 2, c)
    gap = (pr[:, :, 0] - pr[:, :, 1]).abs()
    live = pr.amax(2) > 0
    return m, float(gap[live].min()) if bool(live.any()) else float('inf')


def stage_params(cin, c, seed):
    f = np.float32
    p = dict(w=seeded_value('stage.w', (c, cin, 3), 'conv', seed), b=seeded_value('stage.b', (c,), 'conv_b', seed),
             gamma=seeded_value('stage.gamma', (c,), 'bn_w', seed), beta=seeded_value('stage.beta', (c,), 'bn_b', seed))
    p['gamma'][3] = -0.7                                # a negative scale
    return {k: v.astype(f) for k, v in p.items()}


def stage_dout(rows, lin, c, pool, seed):
    rng = np.random.default_rng([seed, rows, lin, c, 5])
    return rng.standard_normal((rows, lin // 2 if pool else lin, c)).astype(np.float32)


def stage_inputs(rows, R, lin, cin, c, pool, seed=0, margin=MARGIN):
    """x (rows, lin, cin) float32 for the seeded stage, moved offender by offender until no ReLU pre-activation of the float64
    oracle, and no gap of a pool pair that is not both negative, lies within ``margin`` of zero: the smallest change of x that
    takes the offender to +-2 margin to first order (along its own gradient), which moves everything else by far less."""
    rng = np.random.default_rng([seed, rows, R, lin, cin, c])
    p64 = {k: _t(v, torch.float64) for k, v in stage_params(cin, c, seed).items()}
    x = rng.standard_normal((rows, lin, cin))
    for _ in range(20000):
        xt = torch.tensor(x.astype(np.float32), dtype=torch.float64, requires_grad=True)
        z = stage_forward(xt, p64['w'], p64['b'], p64['gamma'], p64['beta'], R, pool)['z']
        cands = [z]
        if pool:
            pr = torch.relu(z[:, :lin // 2 * 2]).reshape(rows, lin // 2, 2, c)
            gap = pr[:, :, 0] - pr[:, :, 1]
            cands.append(torch.where(pr.amax(2) > 0, gap, torch.ones_like(gap)))
        hit = None
        for v in cands:
            idx = torch.nonzero(v.detach().abs() < margin)
            if idx.numel():
                hit = v[tuple(idx[0].tolist())]
                break
        if hit is None:
            return x.astype(np.float32)
        (gr,) = torch.autograd.grad(hit, xt)
        hv = float(hit.detach())
        target = 2 * margin * (1.0 if hv >= 0 else -1.0)
        x = x.astype(np.float32).astype(np.float64) + (gr * ((target - hv) / float((gr * gr).sum()))).numpy() * 1.05
    raise AssertionError('stage_inputs: decisions stay within the margin')


# ---- the tail of a pooled stage alone: y -> BatchNorm per window -> ReLU -> MaxPool1d(2, 2) ------------------------------------
def stage_tail(y, gamma, beta, R, pool, dout, dtype=torch.float64, eps=EPS):
    """-> out, dy, dgamma, dbeta, mean, invstd, z, dz and the window sums ds1 = sum dz, ds2 = sum dz xhat (W, C)."""
    yt, g, b = (_t(v, dtype).requires_grad_(True) for v in (y, gamma, beta))
    rows, l, c = yt.shape
    mean, var, invstd = window_stats(yt, R, eps)
    xh = (yt.reshape(rows // R, R * l, c) - mean[:, None]) * invstd[:, None]
    z = (xh * g + b).reshape(rows, l, c)
    z.retain_grad()
    a = torch.relu(z)
    out = maxpool2(a) if pool else a
    out.backward(_t(dout, dtype))
    dz = z.grad.reshape(rows // R, R * l, c)
    return dict(out=out.detach(), dy=yt.grad, dgamma=g.grad, dbeta=b.grad, mean=mean.detach(), invstd=invstd.detach(), z=z.detach(),
                dz=z.grad, ds1=dz.sum(1), ds2=(dz * xh.detach()).sum(1))


def tail_inputs(rows, R, lin, c, seed=0, margin=MARGIN):
    """y, gamma, beta, dout (float32) of a pooled stage's tail at (rows, R, L, C) with every ReLU pre-activation and every gap
    of a pool pair that is not both negative at least ``margin`` from zero in float64: offending elements of y are moved so that
    z lands at +-2 margin (pairs: the second member moves away from the first), repeated until the statistics, which move
    with y by a part in n, leave none."""
    rng = np.random.default_rng([seed, rows, R, lin, c, 9])
    f = np.float32
    y = (rng.standard_normal((rows, lin, c)) * 1.5 + 0.3).astype(f)
    gamma, beta = rng.uniform(0.5, 1.5, c).astype(f), (rng.standard_normal(c) * 0.3).astype(f)
    gamma[3] = f(-0.7)
    dout = rng.standard_normal((rows, lin // 2, c)).astype(f)
    g64, b64 = torch.from_numpy(gamma).double(), torch.from_numpy(beta).double()
    for _ in range(50):
        yt = torch.from_numpy(y).double()
        mean, var, invstd = window_stats(yt, R)
        k = (g64 * invstd).repeat_interleave(R, 0)[:, None, :]                   # dz / dy per row
        z = (yt - mean.repeat_interleave(R, 0)[:, None, :]) * k + b64
        want = torch.where(z.abs() < margin, torch.where(z >= 0, 2 * margin, -2 * margin).to(z.dtype), z)
        l2 = lin // 2 * 2
        pr = torch.relu(want[:, :l2]).reshape(rows, lin // 2, 2, c)
        close = ((pr[:, :, 0] - pr[:, :, 1]).abs() < margin) & (pr.amax(2) > 0)
        w2 = want[:, :l2].reshape(rows, lin // 2, 2, c)
        w2[:, :, 1][close] = w2[:, :, 0][close] + 3 * margin
        want[:, :l2] = w2.reshape(rows, l2, c)
        moved = want != z
        if not bool(moved.any()):
            return dict(y=y, gamma=gamma, beta=beta, dout=dout)
        y = torch.where(moved, yt + (want - z) / k * 1.02, yt).numpy().astype(f)
    raise AssertionError('tail_inputs: decisions stay within the margin')


# ---- AdaptiveAvgPool1d(lout) + view(N, -1) ---------------------------------------------------------------------------------
def adaptive_pool_flat(x, lout):
    """x (rows, L, C) -> (rows, C * lout): feature c * lout + i = mean of x[:, floor(i L / lout) : ceil((i + 1) L / lout), c]."""
    rows, l, c = x.shape
    cols = [x[:, (i * l) // lout: -((-(i + 1) * l) // lout)].mean(1) for i in range(lout)]
    return torch.stack(cols, 2).reshape(rows, c * lout)


def adaptive_pool_case(x, lout, dfeat, dtype=torch.float64):
    xt = _t(x, dtype).requires_grad_(True)
    feat = adaptive_pool_flat(xt, lout)
    feat.backward(_t(dfeat, dtype))
    return dict(feat=feat.detach(), dx=xt.grad)


# ---- the backbone and the model ----------------------------------------------------------------------------------------------
def backbone_forward(x, params, arch, R, prefix='breath_block.'):
    """x (rows, 1, L) -> features (rows, 3584) by the formulas above."""
    h = x.permute(0, 2, 1)
    for i, cin, c, pooled in stage_list(arch):
        f = prefix + 'features.'
        h = stage_forward(h, params[f + '%d.weight' % i], params[f + '%d.bias' % i], params[f + '%d.weight' % (i + 1)],
                          params[f + '%d.bias' % (i + 1)], R, pooled)['out']
    return adaptive_pool_flat(h, 7)


def model_forward(x, target, params, arch, dtype=torch.float64):
    """CNNLinearNetwork + BCEWithLogitsLoss: x (B, NB, 1, L) -> logits (B, 2), loss."""
    b, nb = x.shape[:2]
    p = {k: _t(v, dtype) for k, v in params.items()}
    feat = backbone_forward(_t(x, dtype).reshape(b * nb, 1, -1), p, arch, nb)
    logits = feat.reshape(b, -1) @ p['linear_final.weight'].t() + p['linear_final.bias']
    return logits, F.binary_cross_entropy_with_logits(logits, _t(target, dtype))
