"""This repository's own restatement of the reference's UNet autoencoder (models/unet.py under models/autoencoder_network.py:
seven double_convs -- Conv1d(k3, p1, bias) -> ReLU twice --, three MaxPool1d(2), three Upsample(scale_factor=2, 'linear',
align_corners=True) each concatenated IN FRONT of the skip map, Conv1d(64, 1, 1); MSE against the input) in float64 numpy, forward
and backward written out by hand: the yardstick an implementation of that network is held to.  Layout here is torch's (N, C, L).

The x2 align_corners=True upsample is the closed form (D = 2 L - 1, exact in rationals):

    out[2j+1] = ((L + j) / D) x[j] + ((L - 1 - j) / D) x[j+1]        out[0] = x[0]
    out[2j]   = (j / D) x[j-1] + ((D - j) / D) x[j]   (j >= 1)

The network takes 14 ReLU decisions (v > 0; one per double_conv conv, in forward order: down1..4, up3, up2, up1) and 3 pool
decisions (True where the SECOND member of the pair won: strictly greater, torch keeps the first on a tie).  ``forward_backward``
takes ``decisions``: None -- decide here -- or (14 bool masks, 3 bool winners) to take instead (the comparison of a GPU run then
does not depend on how near-zero pre-activations fell).  ``bound`` / ``rel_l2`` are ae_ref's."""
import zlib

import numpy as np

from ae_ref import bound, rel_l2                                                           # noqa: F401

DOWN = ((1, 64), (64, 128), (128, 256), (256, 512))
UP = ((3, 768, 256), (2, 384, 128), (1, 192, 64))
BLOCKS = ['dconv_down%d' % k for k in range(1, 5)] + ['dconv_up%d' % k for k, _, _ in UP]      # forward order
NEAR = 1e-4
MODEL_SHAPES = ((4, 16), (5, 24), (3, 224))          # (N, L) of the goldens


def _rng(name, seed):
    return np.random.RandomState((zlib.crc32(('unet/' + name).encode()) + 7919 * seed) & 0x7fffffff)


def param_names():
    """(name, shape) of UNet(1)'s parameters in named_parameters() order."""
    out = []
    for name, (ci, co) in zip(BLOCKS, list(DOWN) + [(ci, co) for _, ci, co in UP]):
        out += [(name + '.0.weight', (co, ci, 3)), (name + '.0.bias', (co,)), (name + '.2.weight', (co, co, 3)), (name + '.2.bias', (co,))]
    return out + [('conv_last.weight', (1, 64, 1)), ('conv_last.bias', (1,))]


def seeded_params(seed=0):
    """name -> float64 array (exactly representable in float32).  Conv weights uniform in +-sqrt(6 / fan_in) (the variance a ReLU
    network keeps), biases in [-0.1, 0.1]."""
    p = {}
    for name, shape in param_names():
        r = _rng(name, seed)
        a = r.uniform(-1.0, 1.0, size=shape) * (np.sqrt(6.0 / (shape[1] * shape[2])) if len(shape) == 3 else 0.1)
        p[name] = a.astype(np.float32).astype(np.float64)
    return p


def seeded_rows(n, l, seed=0):
    return _rng('rows', seed).standard_normal((n, 1, l)).astype(np.float32).astype(np.float64)


def state_dict_keys(prefix=''):
    """The reference's state_dict key list of UNet(1): the parameters, then ``encoder.{0,2,4,6}.*`` (the same tensors as
    ``dconv_down{1..4}.*``)."""
    names = [n for n, _ in param_names()]
    enc = ['encoder.%d.%s' % (2 * (k - 1), n[len('dconv_down1.'):]) for k in range(1, 5) for n in names if n.startswith('dconv_down%d.' % k)]
    return [prefix + k for k in names + enc]


def network_keys():
    """... of AutoencoderNetwork(UNet(1)): ``base_network.*`` then ``breath_block.*`` (the encoder again)."""
    return state_dict_keys('base_network.') + ['breath_block.' + k[len('encoder.'):] for k in state_dict_keys() if k.startswith('encoder.')]


def full_state_dict(params, prefix=''):
    """The parameters under every name the reference's state_dict of UNet(1) has them (the shared ``encoder.N.*`` too)."""
    sd = {}
    for k in state_dict_keys():
        src = k if not k.startswith('encoder.') else 'dconv_down%d.%s' % (int(k.split('.')[1]) // 2 + 1, k.split('.', 2)[2])
        sd[prefix + k] = params[src]
    return sd


def network_state_dict(params):
    sd = full_state_dict(params, 'base_network.')
    sd.update({'breath_block.' + k[len('encoder.'):]: v for k, v in full_state_dict(params).items() if k.startswith('encoder.')})
    return {k: sd[k] for k in network_keys()}


# ---- pieces -------------------------------------------------------------------------------------------------------------
def conv3(x, w, b):
    l = x.shape[2]
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1)))
    return sum(np.einsum('ncl,oc->nol', xp[:, :, t:t + l], w[:, :, t]) for t in range(3)) + b[None, :, None]


def conv3_bwd(dy, x, w):
    """-> dx, dw, db."""
    l = x.shape[2]
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1)))
    dxp = np.zeros_like(xp)
    dw = np.zeros_like(w)
    for t in range(3):
        dw[:, :, t] = np.einsum('nol,ncl->oc', dy, xp[:, :, t:t + l])
        dxp[:, :, t:t + l] += np.einsum('nol,oc->ncl', dy, w[:, :, t])
    return dxp[:, :, 1:l + 1], dw, dy.sum(axis=(0, 2))


def upsample2(x):
    """Upsample(scale_factor=2, mode='linear', align_corners=True) along the last axis, closed form."""
    l = x.shape[-1]
    d = float(2 * l - 1)
    j = np.arange(l, dtype=np.float64)
    out = np.empty(x.shape[:-1] + (2 * l,), dtype=np.float64)
    xn = np.concatenate([x[..., 1:], np.zeros_like(x[..., :1])], axis=-1)          # x[j + 1] (weight 0 at the end)
    xm = np.concatenate([np.zeros_like(x[..., :1]), x[..., :-1]], axis=-1)         # x[j - 1] (weight 0 at the start)
    out[..., 1::2] = ((l + j) / d) * x + ((l - 1 - j) / d) * xn
    out[..., 0::2] = (j / d) * xm + ((d - j) / d) * x
    return out


def upsample2_t(g):
    """The transpose of upsample2: gradient at the output (..., 2 L) -> at the input (..., L)."""
    l = g.shape[-1] // 2
    d = float(2 * l - 1)
    j = np.arange(l, dtype=np.float64)
    ge, go = g[..., 0::2], g[..., 1::2]
    dx = ((l + j) / d) * go + ((d - j) / d) * ge
    dx[..., 1:] += (((l - j) / d) * np.concatenate([np.zeros_like(go[..., :1]), go[..., :-1]], axis=-1))[..., 1:]     # d[2j - 1]
    dx[..., :-1] += (((j + 1) / d) * np.concatenate([ge[..., 1:], np.zeros_like(ge[..., :1])], axis=-1))[..., :-1]    # d[2j + 2]
    return dx


def upsample_terms(x):
    """sum_i |w_i| |x_i| of every output of upsample2 (the scale of its componentwise rounding bound)."""
    return upsample2(np.abs(x))


def upsample_t_terms(g):
    return upsample2_t(np.abs(g))


def forward_backward(x, params, decisions=None, backward=True):
    """The whole network on rows x (N, 1, L) and the gradient of the MSE loss.  -> dict: recon (N, 1, L), loss (1,), encoded
    (N, 512, L / 8: the activated output of dconv_down4), relu (the 14 masks taken), pool (the 3 winners taken), pre (the 14
    pre-activations), gap (3: |a1 - a0| per pair), live (3: whether a pair's larger pre-activation exceeds -NEAR), grad/<name>."""
    p = params
    x = np.asarray(x, dtype=np.float64)
    relu_in = None if decisions is None else list(decisions[0])
    pool_in = None if decisions is None else list(decisions[1])
    out = {'relu': [], 'pool': [], 'pre': [], 'gap': [], 'live': []}
    tape = []

    def relu(v):
        m = (v > 0) if relu_in is None else np.asarray(relu_in[len(out['relu'])], dtype=bool)
        out['relu'].append(m)
        out['pre'].append(v)
        return np.where(m, v, 0.0), m

    def block(h, name):
        v1 = conv3(h, p[name + '.0.weight'], p[name + '.0.bias'])
        a1, m1 = relu(v1)
        v2 = conv3(a1, p[name + '.2.weight'], p[name + '.2.bias'])
        a2, m2 = relu(v2)
        tape.append((name, h, a1, m1, m2))
        return a2

    h, skips, sels = x, [], []
    for k in range(1, 5):
        a = block(h, 'dconv_down%d' % k)
        if k == 4:
            break
        a0, a1 = a[:, :, 0::2], a[:, :, 1::2]
        s = (a1 > a0) if pool_in is None else np.asarray(pool_in[k - 1], dtype=bool)
        pre = out['pre'][-1]
        out['pool'].append(s)
        out['gap'].append(np.abs(a1 - a0))
        out['live'].append(np.maximum(pre[:, :, 0::2], pre[:, :, 1::2]) > -NEAR)
        skips.append(a)
        sels.append(s)
        h = np.where(s, a1, a0)
    out['encoded'] = a
    h = a
    for k, _, _ in UP:
        h = block(np.concatenate([upsample2(h), skips[k - 1]], axis=1), 'dconv_up%d' % k)
    recon = np.einsum('ncl,oc->nol', h, p['conv_last.weight'][:, :, 0]) + p['conv_last.bias'][None, :, None]
    err = recon - x
    out['recon'], out['loss'] = recon, np.array([np.mean(err ** 2)])
    if not backward:
        return out
    g = {}
    dr = 2.0 * err / err.size
    g['conv_last.weight'] = np.einsum('nol,ncl->oc', dr, h)[:, :, None]
    g['conv_last.bias'] = dr.sum(axis=(0, 2))
    dh = np.einsum('nol,oc->ncl', dr, p['conv_last.weight'][:, :, 0])

    def block_bwd(dh):
        name, hin, a1, m1, m2 = tape.pop()
        dv2 = np.where(m2, dh, 0.0)
        da1, g[name + '.2.weight'], g[name + '.2.bias'] = conv3_bwd(dv2, a1, p[name + '.2.weight'])
        dv1 = np.where(m1, da1, 0.0)
        dx, g[name + '.0.weight'], g[name + '.0.bias'] = conv3_bwd(dv1, hin, p[name + '.0.weight'])
        return dx

    dskips = [None] * 3
    for k in (1, 2, 3):
        dcat = block_bwd(dh)
        c = dcat.shape[1] // 3
        dskips[k - 1] = dcat[:, 2 * c:]
        dh = upsample2_t(dcat[:, :2 * c])
    dp = block_bwd(dh)
    for k in (3, 2, 1):
        s = sels[k - 1]
        dh = dskips[k - 1].copy()
        dh[:, :, 0::2] += np.where(s, 0.0, dp)
        dh[:, :, 1::2] += np.where(s, dp, 0.0)
        dp = block_bwd(dh)
    for name, v in g.items():
        out['grad/' + name] = v
    return out


def near_count(res):
    """Decisions of a float64 run that a float32 run may take the other way: ReLU pre-activations within NEAR of 0, and pool pairs
    with a gap under NEAR that are not safely dead (both pre-activations under -NEAR: the mask kills both whoever wins)."""
    n = sum(int((np.abs(v) < NEAR).sum()) for v in res['pre'])
    return n + sum(int(((g < NEAR) & lv).sum()) for g, lv in zip(res['gap'], res['live']))


def decisions_differ(a, b):
    """The number of decisions (14 masks, 3 winners) that two runs took differently."""
    return sum(int((np.asarray(u, dtype=bool) != np.asarray(v, dtype=bool)).sum()) for u, v in zip(list(a[0]) + list(a[1]), list(b[0]) + list(b[1])))


def load_golden(n, l):
    import os
    return np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'golden', 'unet_n%dx%d.npz' % (n, l)))


def golden_decisions(g):
    """(14 masks, 3 winners) the reference's float64 run took, unpacked from a golden."""
    def un(kind, i):
        shape = g['%sshape/%d' % (kind, i)]
        return np.unpackbits(g['%sbits/%d' % (kind, i)])[:int(np.prod(shape))].reshape(shape).astype(bool)
    return [un('relu', i) for i in range(14)], [un('pool', i) for i in range(3)]
