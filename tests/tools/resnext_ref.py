"""Oracle of the SE-ResNeXt 32x4d path (TEST INFRASTRUCTURE ONLY): the SEResNeXtBottleneck forward and backward and the whole
``CNNLinearNetwork(se_resnext50_32x4d / se_resnext101_32x4d)`` restated in stock torch ops on the CPU, float64 by default (any
dtype).  tests/test_resnext_cpu.py pins it to the goldens that tests/tools/make_golden_resnext.py wrote from the reference's
own classes.

The block differs from sebn_ref's SEResNetBottleneck in three places (reference models/senet.py:147-168): conv1 is k1 with
stride 1 onto width = 2 planes channels, conv2 is k3 with 32 groups and carries the stride, and the downsample (k1 with the
block's stride) reads the block's input.  The BatchNorm / conv helpers, the stem, the seeded draws and the margin method are
tests/tools/se_ref.py's and sebn_ref.py's.
"""
import numpy as np
import torch
import torch.nn.functional as F

import se_ref as S
from se_ref import rel_l2, seeded_value, MARGIN, _t   # noqa: F401
from sebn_ref import conv_k1

LAYERS = {'se_resnext50_32x4d': (3, 4, 6, 3), 'se_resnext101_32x4d': (3, 4, 23, 3)}
PLANES = (64, 128, 256, 512)
REDUCTION = 16
EXPANSION = 4
GROUPS = 32


def width_of(planes):
    return planes * 4 // 64 * GROUPS          # floor(planes * (base_width / 64)) * groups, base_width 4


def gconv_rlc(x, w, stride):
    """Bias-free grouped Conv1d k3 p1 (32 groups) on a (rows, L, C) map."""
    return F.conv1d(x.permute(0, 2, 1), w, stride=stride, padding=1, groups=GROUPS).permute(0, 2, 1)


def block_spec(cin, planes, downsample):
    """[(name, shape, kind)] of one SEResNeXtBottleneck in named_parameters() order (senet.py:153-168)."""
    c, wd = planes * EXPANSION, width_of(planes)
    cr = c // REDUCTION
    spec = [('conv1.weight', (wd, cin, 1), 'conv'), ('bn1.weight', (wd,), 'bn_w'), ('bn1.bias', (wd,), 'bn_b'),
            ('conv2.weight', (wd, wd // GROUPS, 3), 'conv'), ('bn2.weight', (wd,), 'bn_w'), ('bn2.bias', (wd,), 'bn_b'),
            ('conv3.weight', (c, wd, 1), 'conv'), ('bn3.weight', (c,), 'bn_w'), ('bn3.bias', (c,), 'bn_b'),
            ('se_module.fc1.weight', (cr, c, 1), 'fc_w'), ('se_module.fc1.bias', (cr,), 'fc1_b'),
            ('se_module.fc2.weight', (c, cr, 1), 'fc_w'), ('se_module.fc2.bias', (c,), 'fc2_b')]
    if downsample:
        spec += [('downsample.0.weight', (c, cin, 1), 'conv'), ('downsample.1.weight', (c,), 'bn_w'), ('downsample.1.bias', (c,), 'bn_b')]
    return spec


def param_spec(net, n_sub_batches=20):
    """-> [(name, shape, kind)] of CNNLinearNetwork(<net>(), n_sub_batches, 0) in named_parameters() order."""
    p = 'breath_block.'
    out = [(p + 'layer0.conv1.weight', (64, 1, 7), 'conv'), (p + 'layer0.bn1.weight', (64,), 'bn_w'), (p + 'layer0.bn1.bias', (64,), 'bn_b')]
    inpl = 64
    for li, planes in enumerate(PLANES):
        for bi in range(LAYERS[net][li]):
            out += [('%slayer%d.%d.%s' % (p, li + 1, bi, n), sh, kind) for n, sh, kind in block_spec(inpl, planes, bi == 0)]
            inpl = planes * EXPANSION
    out.append(('linear_final.weight', (2, 2048 * n_sub_batches), 'lin_w'))
    out.append(('linear_final.bias', (2,), 'lin_b'))
    return out


def seeded_params(net, seed=0, n_sub_batches=20, dtype=np.float32, bn_bias_shift=0.0, fc1_bias_shift=0.0):
    """Deterministic weights by se_ref's name-keyed rules, with sebn_ref's bias shifts."""
    return {name: seeded_value(name, shape, kind, seed, bn_bias_shift, fc1_bias_shift).astype(dtype)
            for name, shape, kind in param_spec(net, n_sub_batches)}


def block_seeded_params(cin, planes, downsample, seed):
    return {n: seeded_value('resnext.' + n, sh, kind, seed).astype(np.float32) for n, sh, kind in block_spec(cin, planes, downsample)}


def block_forward(x, p, stride, R, eps=1e-5, taps=None):
    """One SEResNeXtBottleneck on a (rows, L, C) map; p: the block's parameters by their state_dict names.  taps: a dict that
    receives the ReLU pre-activations (h1, h2, hid, out)."""
    pre_h1 = S.window_bn(conv_k1(x, p['conv1.weight'], 1), R, p['bn1.weight'], p['bn1.bias'], eps)
    pre_h2 = S.window_bn(gconv_rlc(torch.relu(pre_h1), p['conv2.weight'], stride), R, p['bn2.weight'], p['bn2.bias'], eps)
    z = S.window_bn(conv_k1(torch.relu(pre_h2), p['conv3.weight'], 1), R, p['bn3.weight'], p['bn3.bias'], eps)
    res = x
    if 'downsample.0.weight' in p:
        res = S.window_bn(conv_k1(x, p['downsample.0.weight'], stride), R, p['downsample.1.weight'], p['downsample.1.bias'], eps)
    cr = p['se_module.fc1.bias'].shape[0]
    pre1 = z.mean(1) @ p['se_module.fc1.weight'].reshape(cr, -1).t() + p['se_module.fc1.bias']
    s = torch.sigmoid(torch.relu(pre1) @ p['se_module.fc2.weight'].reshape(-1, cr).t() + p['se_module.fc2.bias'])
    pre = z * s[:, None, :] + res
    if taps is not None:
        taps.update(h1=pre_h1, h2=pre_h2, hid=pre1, out=pre)
    return torch.relu(pre)


def block_case(x, params, stride, R, dout, dtype=torch.float64, eps=1e-5):
    """Forward and backward of one block through autograd: -> dict(out, dx, grad/<name>, pre/<h1|h2|hid|out>)."""
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


def block_margins(x, params, stride, R):
    """Smallest |pre-activation| of the four ReLU sites (h1, h2, hid, out) of one block in the float64 oracle."""
    taps = {}
    block_forward(_t(x, torch.float64), {k: _t(v, torch.float64) for k, v in params.items()}, stride, R, taps=taps)
    return {k: float(v.abs().min()) for k, v in taps.items()}


def block_draws(rows, R, l_out, cin, planes, stride, downsample, seed=0):
    """The seeded draws of a block case before any nudging: x (float64), the parameters, dout (float32).  A test takes the
    nudged x from the golden and the other two from here.  The input has ``l_out * stride`` positions."""
    rng = np.random.default_rng([seed, rows, R, l_out, cin, planes, stride, GROUPS])
    params = block_seeded_params(cin, planes, downsample, seed)
    x = rng.standard_normal((rows, l_out * stride, cin))
    dout = rng.standard_normal((rows, l_out, planes * EXPANSION)).astype(np.float32)
    return x, params, dout


def block_inputs(rows, R, l_out, cin, planes, stride, downsample, seed=0, margin=MARGIN):
    """x (rows, l_out * stride, cin) float32, the block's seeded parameters and dout.  x is moved, offender by offender
    (sebn_ref.block_inputs' method), until no ReLU pre-activation of the float64 oracle lies within ``margin`` of zero.
    -> x, params, dout, steps."""
    x, params, dout = block_draws(rows, R, l_out, cin, planes, stride, downsample, seed)
    p64 = {k: _t(v, torch.float64) for k, v in params.items()}
    for step in range(4000):
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
            return x.astype(np.float32), params, dout, step
        (gr,) = torch.autograd.grad(hit, xt)
        hv = float(hit.detach())
        target = 2 * margin * (1.0 if hv >= 0 else -1.0)
        x = x.astype(np.float32).astype(np.float64) + (gr * ((target - hv) / float((gr * gr).sum()))).numpy() * 1.05
    raise AssertionError('block_inputs: pre-activations stay within the margin')


# ---- the whole network ---------------------------------------------------------------------------------------------------
def backbone_forward(net, x, params, R, eps=1e-5, prefix='breath_block.', taps=None):
    """x (rows, 1, L) -> the last map (rows, L / 32, 2048); params: name -> tensor of x's dtype.  taps: a list that receives
    every ReLU pre-activation (the stem's, then four a block)."""
    y = S.conv_rlc(x[:, 0, :, None], params[prefix + 'layer0.conv1.weight'], 2)
    pre0 = S.window_bn(y, R, params[prefix + 'layer0.bn1.weight'], params[prefix + 'layer0.bn1.bias'], eps)
    h = S.ceil_pool(torch.relu(pre0))
    if taps is not None:
        taps.append(pre0)
    for li in range(4):
        for bi in range(LAYERS[net][li]):
            t = {} if taps is not None else None
            h = block_forward(h, S.block_params(params, '%slayer%d.%d.' % (prefix, li + 1, bi)), 2 if (li > 0 and bi == 0) else 1, R, eps, t)
            if taps is not None:
                taps.extend(t.values())
    return h


def model_case(net, x, target, params, dtype=torch.float64, want_grads=True):
    """CNNLinearNetwork(<net>) + BCEWithLogitsLoss on x (B, NB, 1, L), target (B, 2): every window is one BatchNorm batch; the
    head flattens a window's NB x 2048 pooled features breath-major.  -> dict(logits, loss, grad/<name>)."""
    x, target = _t(x, dtype), _t(target, dtype)
    p = {k: _t(v, dtype).clone().requires_grad_(want_grads) for k, v in params.items()}
    b, nb, _, l = x.shape
    hmap = backbone_forward(net, x.reshape(b * nb, 1, l), p, nb)
    assert hmap.shape[1] == 7, 'the oracle pools the 7-position map (seq_len 224)'
    logits = hmap.mean(1).reshape(b, nb * 2048) @ p['linear_final.weight'].t() + p['linear_final.bias']
    loss = F.binary_cross_entropy_with_logits(logits, target)
    r = dict(logits=logits.detach(), loss=loss.detach())
    if want_grads:
        names = list(p)
        for k, g in zip(names, torch.autograd.grad(loss, [p[k] for k in names])):
            r['grad/' + k] = g
    return r
