"""Oracle of the SE-ResNet path (TEST INFRASTRUCTURE ONLY): the SE BasicBlock forward and backward, the ceil-mode stem and
the whole ``CNNLinearNetwork(se_resnet18)`` restated in stock torch ops on the CPU, float64 by default (any dtype: the float32
run is the yardstick ``err32`` of the GPU tests where no golden has one).  tests/test_se_cpu.py pins it to the goldens that
tests/tools/make_golden_se.py wrote from the reference's own classes.

Layouts are the kernels': activations (rows, L, C) channels-last, a BatchNorm window = R consecutive rows; parameters in
torch's layouts.  ``se_param_spec`` / ``seeded_se_params`` follow oracle/weights.py: the same name-keyed RNG formula and its
rules for conv / BatchNorm / linear parameters; the SE gate's fc weights ~ U(+-1/sqrt(C_in)), its biases ~ U(+-0.01).
"""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

LAYERS = (2, 2, 2, 2)
PLANES = (64, 128, 256, 512)
REDUCTION = 4


def se_param_spec(n_sub_batches=20):
    """-> [(name, shape, kind)] of CNNLinearNetwork(se_resnet18(), n_sub_batches, 0) in named_parameters() order; kind in
    {'conv', 'bn_w', 'bn_b', 'fc_w', 'fc1_b', 'fc2_b', 'lin_w', 'lin_b'}."""
    out = []

    def conv(name, co, ci, k):
        out.append((name + '.weight', (co, ci, k), 'conv'))

    def bn(name, c):
        out.append((name + '.weight', (c,), 'bn_w'))
        out.append((name + '.bias', (c,), 'bn_b'))

    p = 'breath_block.'
    conv(p + 'layer0.conv1', 64, 1, 7)
    bn(p + 'layer0.bn1', 64)
    inpl = 64
    for li, planes in enumerate(PLANES):
        for bi in range(LAYERS[li]):
            bp = '%slayer%d.%d.' % (p, li + 1, bi)
            stride = 2 if (li > 0 and bi == 0) else 1
            conv(bp + 'conv1', planes, inpl, 3)
            bn(bp + 'bn1', planes)
            conv(bp + 'conv2', planes, planes, 3)
            cr = planes // REDUCTION
            out.append((bp + 'se_module.fc1.weight', (cr, planes, 1), 'fc_w'))
            out.append((bp + 'se_module.fc1.bias', (cr,), 'fc1_b'))
            out.append((bp + 'se_module.fc2.weight', (planes, cr, 1), 'fc_w'))
            out.append((bp + 'se_module.fc2.bias', (planes,), 'fc2_b'))
            bn(bp + 'bn2', planes)
            if stride != 1 or inpl != planes:
                conv(bp + 'downsample.0', planes, inpl, 1)
                bn(bp + 'downsample.1', planes)
            inpl = planes
    out.append(('linear_final.weight', (2, 512 * n_sub_batches), 'lin_w'))
    out.append(('linear_final.bias', (2,), 'lin_b'))
    return out


def seeded_value(name, shape, kind, seed, bn_bias_shift=0.0, fc1_bias_shift=0.0):
    """One parameter from the name-keyed RNG of oracle/weights.py (float64)."""
    rng = np.random.default_rng([seed, zlib.crc32(name.encode())])
    if kind == 'conv':
        return rng.standard_normal(shape) * np.sqrt(2.0 / (shape[2] * shape[0]))
    if kind == 'bn_w':
        return rng.uniform(0.5, 1.5, shape)
    if kind == 'bn_b':
        return rng.standard_normal(shape) * 0.1 + bn_bias_shift
    if kind in ('fc_w', 'lin_w'):
        bound = 1.0 / np.sqrt(shape[1])
        return rng.uniform(-bound, bound, shape)
    return rng.uniform(-0.01, 0.01, shape) + (fc1_bias_shift if kind == 'fc1_b' else 0.0)


def seeded_se_params(seed=0, n_sub_batches=20, dtype=np.float32, bn_bias_shift=0.0, fc1_bias_shift=0.0):
    """Deterministic weights of CNNLinearNetwork(se_resnet18).  bn_bias_shift / fc1_bias_shift > 0 move every BatchNorm beta
    and every fc1 bias up so that no ReLU decision (block outputs, gate hidden units) can flip under fp32 rounding."""
    return {name: seeded_value(name, shape, kind, seed, bn_bias_shift, fc1_bias_shift).astype(dtype)
            for name, shape, kind in se_param_spec(n_sub_batches)}


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    nb = float(np.linalg.norm(b))
    return float(np.linalg.norm(a - b) / (nb if nb > 1e-9 else 1.0))      # ~zero references: absolute


def _t(a, dtype):
    return a.to(dtype) if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a)).to(dtype)


def pool_len_ceil(lc):
    """Output length of MaxPool1d(3, stride 2, ceil_mode=True), no padding, from the rule itself: windows start at 0, 2, 4, ...
    and a window must start inside the row; the last one may be clipped, but a row needs two elements for one window."""
    if lc < 2:
        return 0
    n = -(-(lc - 3) // 2) + 1
    return n - 1 if (n - 1) * 2 >= lc else n


# ---- BatchNorm per window of R rows, (rows, L, C) -----------------------------------------------------------------------
def window_stats(x, R, eps=1e-5):
    rows, l, c = x.shape
    xw = x.reshape(rows // R, R * l, c)
    mean = xw.mean(1)
    var = ((xw - mean[:, None]) ** 2).mean(1)
    return mean, 1.0 / torch.sqrt(var + eps)


def window_bn(x, R, gamma, beta, eps=1e-5):
    rows, l, c = x.shape
    mean, invstd = window_stats(x, R, eps)
    xw = x.reshape(rows // R, R * l, c)
    return (((xw - mean[:, None]) * invstd[:, None]) * gamma + beta).reshape(rows, l, c)


def conv_rlc(x, w, stride):
    """Bias-free Conv1d with padding k // 2 on a (rows, L, C) map."""
    return F.conv1d(x.permute(0, 2, 1), w, stride=stride, padding=w.shape[2] // 2).permute(0, 2, 1)


# ---- the SE tail in closed form: what each of the five kernels computes ------------------------------------------------
def se_tail(y2, res, gamma, beta, w1, b1, w2, b2, R, dout=None, eps=1e-5, dtype=torch.float64):
    """out = relu(z * s + res) with z = bn2(y2), s = sigmoid(fc2(relu(fc1(mean_L z)))), and -- with dout -- its backward,
    every intermediate by name (what the kernels store or return).  w1 (Cr, C[, 1]), w2 (C, Cr[, 1])."""
    y2, res, gamma, beta, b1, b2 = (_t(a, dtype) for a in (y2, res, gamma, beta, b1, b2))
    w1, w2 = _t(w1, dtype).reshape(b1.shape[0], -1), _t(w2, dtype).reshape(b2.shape[0], -1)
    rows, l, c = y2.shape
    w = rows // R
    mean, invstd = window_stats(y2, R, eps)
    xhat = ((y2.reshape(w, R * l, c) - mean[:, None]) * invstd[:, None])
    z = (xhat * gamma + beta).reshape(rows, l, c)
    pool = z.mean(1)
    pre1 = pool @ w1.t() + b1
    hid = torch.relu(pre1)
    s = torch.sigmoid(hid @ w2.t() + b2)
    pre = z * s[:, None, :] + res
    r = dict(mean=mean, invstd=invstd, z=z, pool=pool, pre1=pre1, hid=hid, s=s, pre=pre, out=torch.relu(pre), mask=pre > 0)
    if dout is None:
        return r
    dout = _t(dout, dtype)
    g = dout * r['mask'].to(dtype)
    dsum = (g * z).sum(1)
    dpre2 = dsum * s * (1 - s)
    dhid = (dpre2 @ w2) * (pre1 > 0).to(dtype)
    dpool = dhid @ w1
    dz = g * s[:, None, :] + dpool[:, None, :] / l
    dzw = dz.reshape(w, R * l, c)
    s1, s2 = dzw.sum(1), (dzw * xhat).sum(1)
    n = R * l
    dy2 = ((dzw - s1[:, None] / n - xhat * s2[:, None] / n) * (gamma * invstd)[:, None]).reshape(rows, l, c)
    r.update(g=g, dsum=dsum, dpool=dpool, dz=dz, dy2=dy2, dgamma=s2.sum(0), dbeta=s1.sum(0),
             dw2=dpre2.t() @ hid, db2=dpre2.sum(0), dw1=dhid.t() @ pool, db1=dhid.sum(0))
    return r


def block_forward(x, p, stride, R, eps=1e-5, taps=None):
    """One SEBasicBlock on a (rows, L, C) map; p: the block's parameters by their state_dict names (tensors of x's dtype).
    taps: a dict that receives the ReLU pre-activations (h1, hid, out)."""
    y1 = conv_rlc(x, p['conv1.weight'], stride)
    pre_h1 = window_bn(y1, R, p['bn1.weight'], p['bn1.bias'], eps)
    y2 = conv_rlc(torch.relu(pre_h1), p['conv2.weight'], 1)
    z = window_bn(y2, R, p['bn2.weight'], p['bn2.bias'], eps)
    res = x
    if 'downsample.0.weight' in p:
        res = window_bn(conv_rlc(x, p['downsample.0.weight'], stride), R, p['downsample.1.weight'], p['downsample.1.bias'], eps)
    cr = p['se_module.fc1.bias'].shape[0]
    pre1 = z.mean(1) @ p['se_module.fc1.weight'].reshape(cr, -1).t() + p['se_module.fc1.bias']
    s = torch.sigmoid(torch.relu(pre1) @ p['se_module.fc2.weight'].reshape(-1, cr).t() + p['se_module.fc2.bias'])
    pre = z * s[:, None, :] + res
    if taps is not None:
        taps.update(h1=pre_h1, hid=pre1, out=pre)
    return torch.relu(pre)


def block_case(x, params, stride, R, dout, dtype=torch.float64, eps=1e-5):
    """Forward and backward of one block through autograd: -> dict(out, dx, grad/<name>, pre/<h1|hid|out>)."""
    xt = _t(x, dtype).clone().requires_grad_(True)
    p = {k: _t(v, dtype).clone().requires_grad_(True) for k, v in params.items()}
    taps = {}
    out = block_forward(xt, p, stride, R, eps, taps)
    names = list(p)
    grads = torch.autograd.grad(out, [xt] + [p[k] for k in names], _t(dout, dtype))
    r = dict(out=out.detach(), dx=grads[0])
    r.update({'grad/' + k: g for k, g in zip(names, grads[1:])})
    r.update({'pre/' + k: v.detach() for k, v in taps.items()})
    return r


# ---- layer0: conv k7 s2 p3 -> BatchNorm -> ReLU -> MaxPool1d(3, 2, ceil_mode=True) --------------------------------------
def ceil_pool(a):
    """(rows, L, C) -> (rows, Lp, C): max over {2j, 2j+1, 2j+2} clipped at L."""
    return F.max_pool1d(a.permute(0, 2, 1), 3, stride=2, ceil_mode=True).permute(0, 2, 1)


def ceil_pool_routing(a, dout):
    """The pool's backward alone on the post-ReLU map ``a`` (rows, L, C): every window hands its dout to its FIRST maximum
    (ascending position, strict >), written out as a loop so that the rule is stated here and not borrowed.  -> (rows, L, C)."""
    rows, l, c = a.shape
    lp = pool_len_ceil(l)
    da = torch.zeros_like(a)
    for j in range(lp):
        best = a[:, 2 * j, :].clone()
        arg = torch.full_like(best, 2 * j, dtype=torch.long)
        for t in (1, 2):
            pos = 2 * j + t
            if pos >= l:
                break
            better = a[:, pos, :] > best
            best = torch.where(better, a[:, pos, :], best)
            arg = torch.where(better, torch.full_like(arg, pos), arg)
        da.scatter_add_(1, arg[:, None, :], dout[:, j:j + 1, :])
    return da


def stem_forward(x2d, w, gamma, beta, R, eps=1e-5):
    """x2d (rows, Lin) -> (pooled map (rows, Lp, C), conv output y (rows, Lc, C))."""
    y = conv_rlc(x2d[:, :, None], w, 2)
    return ceil_pool(torch.relu(window_bn(y, R, gamma, beta, eps))), y


def stem_case(x2d, w, gamma, beta, R, dout, dtype=torch.float64, eps=1e-5):
    x2d, dout = _t(x2d, dtype), _t(dout, dtype)
    w, gamma, beta = (_t(a, dtype).clone().requires_grad_(True) for a in (w, gamma, beta))
    out, y = stem_forward(x2d, w, gamma, beta, R, eps)
    dw, dg, db = torch.autograd.grad(out, [w, gamma, beta], dout)
    mean, invstd = window_stats(y.detach(), R, eps)
    a = torch.relu(window_bn(y.detach(), R, gamma.detach(), beta.detach(), eps))
    return dict(out=out.detach(), y=y.detach(), mean=mean, invstd=invstd, dw=dw, dgamma=dg, dbeta=db,
                routed=ceil_pool_routing(a, dout))


def stem_inputs(rows, R, lin, c, seed=0):
    """Raw rows (rows, lin) with tied maxima for the pool -- a silent row (every conv output equal), a row of constant blocks
    of 16 samples (equal conv outputs inside a block), values on a quarter grid elsewhere --, the stem's weights, BatchNorm
    parameters with one negative scale and one channel pushed far below zero (all-negative windows: the ReLU gives 0, 0, 0
    and the first position takes the gradient), and dout for the pooled map.  float32."""
    rng = np.random.default_rng([seed, rows, R, lin, c])
    f = np.float32
    x = np.round(rng.standard_normal((rows, lin)) * 4) / 4
    x[1] = 0.0
    x[2] = np.repeat(np.round(rng.standard_normal((lin + 15) // 16) * 4) / 4, 16)[:lin]
    w = rng.standard_normal((c, 1, 7)) * 0.4
    gamma = rng.uniform(0.5, 1.5, c)
    beta = rng.standard_normal(c) * 0.3
    gamma[3] = -0.7
    beta[5] = -30.0
    dout = rng.standard_normal((rows, pool_len_ceil(lin // 2), c))
    return x.astype(f), w.astype(f), gamma.astype(f), beta.astype(f), dout.astype(f)


# ---- the whole network ---------------------------------------------------------------------------------------------------
def block_params(params, prefix):
    return {k[len(prefix):]: v for k, v in params.items() if k.startswith(prefix)}


def backbone_forward(x, params, R, eps=1e-5, prefix='breath_block.'):
    """x (rows, 1, L) -> the last map (rows, L / 32, 512); params: name -> tensor of x's dtype."""
    h, _ = stem_forward(x[:, 0, :], params[prefix + 'layer0.conv1.weight'], params[prefix + 'layer0.bn1.weight'],
                        params[prefix + 'layer0.bn1.bias'], R, eps)
    for li in range(4):
        for bi in range(LAYERS[li]):
            h = block_forward(h, block_params(params, '%slayer%d.%d.' % (prefix, li + 1, bi)), 2 if (li > 0 and bi == 0) else 1, R, eps)
    return h


def model_case(x, target, params, dtype=torch.float64, want_grads=True):
    """CNNLinearNetwork(se_resnet18) + BCEWithLogitsLoss on x (B, NB, 1, L), target (B, 2): every window is one BatchNorm
    batch; the head flattens a window's NB x 512 pooled features breath-major.  -> dict(logits, loss, grad/<name>)."""
    x, target = _t(x, dtype), _t(target, dtype)
    p = {k: _t(v, dtype).clone().requires_grad_(want_grads) for k, v in params.items()}
    b, nb, _, l = x.shape
    hmap = backbone_forward(x.reshape(b * nb, 1, l), p, nb)
    feat = hmap.mean(1) if hmap.shape[1] == 7 else None
    assert feat is not None, 'the oracle pools the 7-position map (seq_len 224)'
    logits = feat.reshape(b, nb * 512) @ p['linear_final.weight'].t() + p['linear_final.bias']
    loss = F.binary_cross_entropy_with_logits(logits, target)
    r = dict(logits=logits.detach(), loss=loss.detach())
    if want_grads:
        names = list(p)
        for k, g in zip(names, torch.autograd.grad(loss, [p[k] for k in names])):
            r['grad/' + k] = g
    return r


# ---- seeded kernel cases whose ReLU decisions have a margin ------------------------------------------------------------
MARGIN = 1e-3


def tail_case(rows, R, l, c, seed=0, margin=MARGIN, cr=None):
    """Inputs of the SE tail at (rows, R, L, C), float32 arrays, built so that no ReLU pre-activation of the float64 oracle
    (the gate's hidden units, the block output) lies within ``margin`` of zero.  Hidden units: an offender's fc1 bias is
    nudged by 4 margin away from zero (that moves the unit's whole column: repeated until none is left).  Outputs: pre =
    z s + res is moved to +-2 margin through res, element by element (res enters nothing else).  ``cr``: the gate's hidden
    width, c // REDUCTION unless given (the draws before fc1 do not depend on it)."""
    rng = np.random.default_rng([seed, rows, R, l, c])
    cr = c // REDUCTION if cr is None else cr
    f = np.float32
    case = dict(y2=rng.standard_normal((rows, l, c)).astype(f) * 1.5 + 0.3, res=rng.standard_normal((rows, l, c)).astype(f),
                gamma=rng.uniform(0.5, 1.5, c).astype(f), beta=(rng.standard_normal(c) * 0.1).astype(f),
                w1=rng.uniform(-1, 1, (cr, c, 1)).astype(f) / f(np.sqrt(c)), b1=rng.uniform(-0.01, 0.01, cr).astype(f),
                w2=rng.uniform(-1, 1, (c, cr, 1)).astype(f) / f(np.sqrt(cr)), b2=rng.uniform(-0.01, 0.01, c).astype(f),
                dout=rng.standard_normal((rows, l, c)).astype(f))
    case['gamma'][3] = f(-0.7)                       # a negative scale
    fwd = lambda: se_tail(R=R, **{k: v for k, v in case.items() if k != 'dout'})
    for _ in range(400):
        pre1 = fwd()['pre1'].numpy()
        bad = np.argwhere(np.abs(pre1) < margin)
        if bad.size == 0:
            break
        row, j = bad[0]
        case['b1'][j] += f(4 * margin) * (1 if pre1[row, j] >= 0 else -1)
    else:
        raise AssertionError('tail_case: hidden pre-activations stay within the margin')
    pre = fwd()['pre'].numpy()
    bad = np.abs(pre) < margin
    case['res'] = np.where(bad, case['res'] + np.where(pre >= 0, 2 * margin, -2 * margin) - pre, case['res']).astype(f)
    return case


def tail_margins(case, R):
    """(smallest |hidden pre-activation|, smallest |output pre-activation|) of the float64 oracle on the case's inputs."""
    r = se_tail(R=R, **{k: v for k, v in case.items() if k != 'dout'})
    return float(r['pre1'].abs().min()), float(r['pre'].abs().min())


def block_seeded_params(cin, planes, stride, seed):
    """One block's parameters by the rules of seeded_se_params, keyed by (seed, name)."""
    cr = planes // REDUCTION
    spec = [('conv1.weight', (planes, cin, 3), 'conv'), ('bn1.weight', (planes,), 'bn_w'), ('bn1.bias', (planes,), 'bn_b'),
            ('conv2.weight', (planes, planes, 3), 'conv'), ('se_module.fc1.weight', (cr, planes, 1), 'fc_w'),
            ('se_module.fc1.bias', (cr,), 'fc1_b'), ('se_module.fc2.weight', (planes, cr, 1), 'fc_w'),
            ('se_module.fc2.bias', (planes,), 'fc2_b'), ('bn2.weight', (planes,), 'bn_w'), ('bn2.bias', (planes,), 'bn_b')]
    if stride != 1 or cin != planes:
        spec += [('downsample.0.weight', (planes, cin, 1), 'conv'), ('downsample.1.weight', (planes,), 'bn_w'),
                 ('downsample.1.bias', (planes,), 'bn_b')]
    return {n: seeded_value('block.' + n, sh, kind, seed).astype(np.float32) for n, sh, kind in spec}


def block_margins(x, params, stride, R):
    """Smallest |pre-activation| of the three ReLU sites (h1, hid, out) of one block in the float64 oracle."""
    taps = {}
    block_forward(_t(x, torch.float64), {k: _t(v, torch.float64) for k, v in params.items()}, stride, R, taps=taps)
    return {k: float(v.abs().min()) for k, v in taps.items()}


def block_inputs(rows, R, l_out, planes, stride, seed=0, margin=MARGIN):
    """x (rows, l_out * stride, planes / stride) float32, the block's seeded parameters and dout for an SEBasicBlock whose
    output is (rows, l_out, planes) -- an identity block (stride 1) or a stage entry (stride 2, half the channels in).  x is
    then moved, offender by offender, until no ReLU pre-activation of the float64 oracle (h1, the gate's hidden units, the
    block output) lies within ``margin`` of zero: the smallest change of x that takes the offender to +-2 margin to first
    order (along the offender's own gradient with respect to x), which moves everything else by far less."""
    cin, lin = planes // stride, l_out * stride
    rng = np.random.default_rng([seed, rows, R, l_out, planes, stride])
    params = block_seeded_params(cin, planes, stride, seed)
    x = rng.standard_normal((rows, lin, cin))
    dout = rng.standard_normal((rows, l_out, planes)).astype(np.float32)
    p64 = {k: _t(v, torch.float64) for k, v in params.items()}
    for _ in range(2000):
        xt = torch.tensor(x.astype(np.float32), dtype=torch.float64, requires_grad=True)
        taps = {}
        block_forward(xt, p64, stride, R, taps=taps)
        hit = None
        for v in taps.values():
            idx = torch.nonzero(v.detach().abs() < margin)
            if idx.numel():
                hit = v[tuple(idx[0].tolist())]
                break
        if hit is None:
            return x.astype(np.float32), params, dout
        (gr,) = torch.autograd.grad(hit, xt)
        hv = float(hit.detach())
        target = 2 * margin * (1.0 if hv >= 0 else -1.0)
        x = x.astype(np.float32).astype(np.float64) + (gr * ((target - hv) / float((gr * gr).sum()))).numpy() * 1.05
    raise AssertionError('block_inputs: pre-activations stay within the margin')
