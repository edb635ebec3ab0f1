"""This repository's own restatement of the reference's autoencoder (models/autoencoder_cnn.py, models/autoencoder_network.py:
four Conv1d / BatchNorm1d / MaxPool1d(2, return_indices) stages, then four MaxUnpool1d(2) / ConvTranspose1d stages, NO ReLU, all
N rows one BatchNorm batch, MSE against the input) in plain torch on the CPU, in float64 or float32: the yardstick an
implementation of that network is held to.  Layout here is torch's (N, C, L).

A pool decision is a bool per pooled element, True where the SECOND member of the pair won (strictly greater: torch's index
keeps the first on a tie).  Every function that pools takes ``sel``: None -- decide here -- or the decisions as given
(teacher-forced: the comparison of a GPU run then does not depend on how near-ties fell)."""
import zlib

import numpy as np
import torch
import torch.nn.functional as TF

EPS, MOMENTUM = 1e-5, 0.1
CHANNELS = (1, 64, 128, 256, 512)
BOUND_FLOOR, BOUND_CAP = 16 * 2.0 ** -23, 1e-4


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    d = np.sqrt(np.sum(b * b))
    return float(np.sqrt(np.sum((a - b) ** 2)) / d) if d > 0 else float(np.sqrt(np.sum(a * a)))


def bound(err32):
    """The project's bound per tensor: rel-l2 against float64 <= min(max(4 err32, 16 2^-23), 1e-4)."""
    return min(max(4.0 * float(err32), BOUND_FLOOR), BOUND_CAP)


def _rng(name, seed):
    return np.random.RandomState((zlib.crc32(name.encode()) + 7919 * seed) & 0x7fffffff)


def param_names():
    """(name, shape, kind) of AutoencoderCNN's parameters in named_parameters() order."""
    out = []
    for k in range(1, 5):
        ci, co = CHANNELS[k - 1], CHANNELS[k]
        out += [('conv_down%d.weight' % k, (co, ci, 3), 'w'), ('conv_down%d.bias' % k, (co,), 'b'),
                ('bn%d.weight' % k, (co,), 'g'), ('bn%d.bias' % k, (co,), 'b')]
    for k in range(1, 5):
        ci, co = CHANNELS[5 - k], CHANNELS[4 - k]
        out += [('conv_up%d.weight' % k, (ci, co, 3), 'w'), ('conv_up%d.bias' % k, (co,), 'b')]
    return out


def seeded_params(seed=0):
    """name -> float64 array.  Conv weights uniform with torch's default bound; BatchNorm weights in [0.5, 1.5] with every
    third one negated; every bias in [-0.5, 0.5]."""
    p = {}
    for name, shape, kind in param_names():
        r = _rng(name, seed)
        if kind == 'w':
            fan = shape[1] * shape[2] if 'down' in name else shape[0] * shape[2]
            a = r.uniform(-1.0, 1.0, size=shape) / np.sqrt(fan)
        elif kind == 'g':
            a = r.uniform(0.5, 1.5, size=shape)
            a[::3] *= -1.0
        else:
            a = r.uniform(-0.5, 0.5, size=shape)
        p[name] = a.astype(np.float32).astype(np.float64)           # (exactly representable in float32)
    return p


def seeded_rows(n, l, seed=0):
    return _rng('rows', seed).standard_normal((n, 1, l)).astype(np.float32).astype(np.float64)


def full_state_dict(params, prefix=''):
    """The parameters under every name the reference's state_dict has them (the shared ``encoder.N.*`` too)."""
    sd = {}
    for k in range(1, 5):
        for leaf in ('weight', 'bias'):
            sd['encoder.%d.%s' % (3 * (k - 1), leaf)] = params['conv_down%d.%s' % (k, leaf)]
            sd['encoder.%d.%s' % (3 * (k - 1) + 1, leaf)] = params['bn%d.%s' % (k, leaf)]
    sd.update(params)
    return {prefix + k: v for k, v in sd.items()}


# ---- pieces -------------------------------------------------------------------------------------------------------------
def bn_stats(y, R=None):
    """(mean, var) per window of R rows (all rows when None) and channel of y (N, C, L): (W, C), biased variance."""
    n, c, l = y.shape
    R = n if R is None else R
    yw = y.reshape(n // R, R, c, l)
    mean = yw.mean(dim=(1, 3))
    var = ((yw - mean[:, None, :, None]) ** 2).mean(dim=(1, 3))
    return mean, var


def bn_apply(y, mean, var, gamma, beta, eps=EPS):
    n, c, l = y.shape
    w = mean.shape[0]
    yw = y.reshape(w, n // w, c, l)
    z = (yw - mean[:, None, :, None]) / torch.sqrt(var[:, None, :, None] + eps) * gamma[None, None, :, None] + beta[None, None, :, None]
    return z.reshape(n, c, l)


def pool2(z, sel=None):
    """-> pooled (N, C, L // 2), sel bool, gap |z1 - z0|."""
    lo = z.shape[2] // 2
    z0, z1 = z[:, :, 0:2 * lo:2], z[:, :, 1:2 * lo:2]
    if sel is None:
        sel = (z1 > z0).detach()
    return torch.where(sel, z1, z0), sel, (z1 - z0).detach().abs()


def unpool2(v, sel):
    n, c, l = v.shape
    out = torch.zeros((n, c, 2 * l), dtype=v.dtype)
    zero = torch.zeros((), dtype=v.dtype)
    out[:, :, 0::2] = torch.where(sel, zero, v)
    out[:, :, 1::2] = torch.where(sel, v, zero)
    return out


def _t(a, dtype, grad=False):
    t = torch.tensor(np.asarray(a), dtype=dtype)
    return t.requires_grad_(True) if grad else t


def model(x, params, dtype=torch.float64, sels=None, eps=EPS, encoder_only=False):
    """The whole network on rows x (N, 1, L), all N rows one BatchNorm batch, and the gradient of the MSE loss.
    -> dict: recon, loss, sel (4 bool arrays), gap (the 4 stages' |z1 - z0| per pair), grad/<name>, running_mean/bn<k>,
    running_var/bn<k> (after ONE step from torch's initial buffers); encoder_only: 'encoded' (N, 512, (L // 16) // 14) alone."""
    p = {k: _t(v, dtype, True) for k, v in params.items()}
    h = x_ = _t(x, dtype)
    out = {'sel': [], 'gap': []}
    for k in range(1, 5):
        y = TF.conv1d(h, p['conv_down%d.weight' % k], p['conv_down%d.bias' % k], padding=1)
        mean, var = bn_stats(y)
        cnt = y.shape[0] * y.shape[2]
        out['running_mean/bn%d' % k] = (MOMENTUM * mean[0]).detach().numpy()
        out['running_var/bn%d' % k] = (1.0 - MOMENTUM + MOMENTUM * var[0] * cnt / max(cnt - 1, 1)).detach().numpy()
        z = bn_apply(y, mean, var, p['bn%d.weight' % k], p['bn%d.bias' % k], eps)
        h, s, gap = pool2(z, None if sels is None else torch.as_tensor(sels[k - 1]))
        out['sel'].append(s.numpy())
        out['gap'].append(gap.numpy())
    if encoder_only:
        out['encoded'] = TF.max_pool1d(h, 14).detach().numpy()
        return out
    u = h
    for k in range(1, 5):
        u = TF.conv_transpose1d(unpool2(u, torch.as_tensor(out['sel'][4 - k])), p['conv_up%d.weight' % k], p['conv_up%d.bias' % k],
                                padding=1)
    loss = ((u - x_) ** 2).mean()
    loss.backward()
    out['recon'], out['loss'] = u.detach().numpy(), loss.detach().numpy().reshape(1)
    for name, t in p.items():
        out['grad/' + name] = t.grad.numpy() if t.grad is not None else np.zeros(tuple(t.shape))
    return out


def decision_report(sel_a, sel_b, gap64):
    """Per stage: (pairs, pairs that differ, the largest float64 gap among those, pairs with a gap under 1e-4)."""
    rep = []
    for a, b, g in zip(sel_a, sel_b, gap64):
        d = np.asarray(a) != np.asarray(b)
        rep.append((int(d.size), int(d.sum()), float(g[d].max()) if d.any() else 0.0, int((g < 1e-4).sum())))
    return rep


MODEL_SHAPES = ((4, 16), (6, 32), (3, 224))          # (N, L) of the goldens


def load_golden(n, l):
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'golden', 'autoencoder_n%dx%d.npz' % (n, l)))
    sels = [np.unpackbits(g['selbits/%d' % k])[:int(np.prod(g['selshape/%d' % k]))].reshape(g['selshape/%d' % k]).astype(bool)
            for k in range(1, 5)]
    return g, sels
