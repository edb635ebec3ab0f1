"""numpy restatement of the cnn_transformer head (reference models/transformer.py:13-107), forward and backward, in the
dtype of its operands (float64: the oracle; float32: the reference figure for shapes that have no golden).

A block's parameters are the sixteen arrays in named_parameters() order (PARAM_NAMES).  ``masks``: None (no dropout) or
the two keep masks (B, T, D) of the block's dropout sites, applied as ``x * mask / (1 - p)`` like nn.Dropout.
Quirk kept: the second residual adds the block INPUT (:88)."""
import numpy as np

PARAM_NAMES = ('attention.q_linear.weight', 'attention.q_linear.bias', 'attention.k_linear.weight', 'attention.k_linear.bias',
               'attention.v_linear.weight', 'attention.v_linear.bias', 'attention.joint_linear.weight',
               'attention.joint_linear.bias', 'attention_norm.weight', 'attention_norm.bias', 'ff.0.weight', 'ff.0.bias',
               'ff.2.weight', 'ff.2.bias', 'ff_norm.weight', 'ff_norm.bias')
HEADS = 4
EPS = 1e-5


def _ln(a, g, b):
    mean = a.mean(-1, keepdims=True)
    var = np.square(a - mean).mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + a.dtype.type(EPS))
    xh = (a - mean) * rstd
    return xh * g + b, xh, rstd


def _ln_bwd(dy, xh, rstd, g):
    gg = dy * g
    return rstd * (gg - gg.mean(-1, keepdims=True) - xh * (gg * xh).mean(-1, keepdims=True)), (dy * xh).sum((0, 1)), dy.sum((0, 1))


def block_forward(x, P, masks=None, p=0.0):
    """x (B, T, D) -> (y, cache); cache['weights'] (B, 4, T, T)."""
    wq, bq, wk, bk, wv, bv, wj, bj, g1, be1, w0, b0, w2, b2, g2, be2 = P
    B, T, D = x.shape
    Hd = wq.shape[0]
    hs = Hd // HEADS
    one = x.dtype.type(1)
    scale = one / (one - x.dtype.type(p))
    m1, m2 = (None, None) if masks is None else [m.astype(x.dtype) * scale for m in masks]
    split = lambda a: a.reshape(B, T, HEADS, hs).transpose(0, 2, 1, 3)
    q, k, v = split(x @ wq.T + bq), split(x @ wk.T + bk), split(x @ wv.T + bv)
    s = (q @ k.transpose(0, 1, 3, 2)) / np.sqrt(x.dtype.type(hs))
    e = np.exp(s - s.max(-1, keepdims=True))
    w = e / e.sum(-1, keepdims=True)
    wvv = (w @ v).transpose(0, 2, 1, 3).reshape(B, T, Hd)
    joint = wvv @ wj.T + bj
    a1 = (joint if m1 is None else joint * m1) + x
    att, xh1, r1 = _ln(a1, g1, be1)
    pre = att @ w0.T + b0
    hid = np.maximum(pre, 0)
    f = hid @ w2.T + b2
    a2 = (f if m2 is None else f * m2) + x
    y, xh2, r2 = _ln(a2, g2, be2)
    return y, dict(x=x, P=P, q=q, k=k, v=v, weights=w, wv=wvv, m1=m1, m2=m2, xh1=xh1, r1=r1, att=att, hid=hid, xh2=xh2, r2=r2)


def block_backward(dy, c):
    """-> (dx, the sixteen parameter gradients in PARAM_NAMES order)."""
    wq, bq, wk, bk, wv, bv, wj, bj, g1, be1, w0, b0, w2, b2, g2, be2 = c['P']
    x = c['x']
    B, T, D = x.shape
    Hd = wq.shape[0]
    hs = Hd // HEADS
    sum01 = lambda a, b: np.einsum('btm,btn->mn', a, b)
    da2, dg2, dbe2 = _ln_bwd(dy, c['xh2'], c['r2'], g2)
    df = da2 if c['m2'] is None else da2 * c['m2']
    dw2, db2 = sum01(df, c['hid']), df.sum((0, 1))
    dpre = (df @ w2) * (c['hid'] > 0)
    dw0, db0 = sum01(dpre, c['att']), dpre.sum((0, 1))
    datt = dpre @ w0
    da1, dg1, dbe1 = _ln_bwd(datt, c['xh1'], c['r1'], g1)
    dj = da1 if c['m1'] is None else da1 * c['m1']
    dwj, dbj = sum01(dj, c['wv']), dj.sum((0, 1))
    dwv = (dj @ wj).reshape(B, T, HEADS, hs).transpose(0, 2, 1, 3)
    w, q, k, v = c['weights'], c['q'], c['k'], c['v']
    dv = w.transpose(0, 1, 3, 2) @ dwv
    dw = dwv @ v.transpose(0, 1, 3, 2)
    ds = w * (dw - (w * dw).sum(-1, keepdims=True)) / np.sqrt(x.dtype.type(hs))
    dq, dk = ds @ k, ds.transpose(0, 1, 3, 2) @ q
    join = lambda a: a.transpose(0, 2, 1, 3).reshape(B, T, Hd)
    dq, dk, dv = join(dq), join(dk), join(dv)
    dx = da1 + da2 + dq @ wq + dk @ wk + dv @ wv
    grads = [sum01(dq, x), dq.sum((0, 1)), sum01(dk, x), dk.sum((0, 1)), sum01(dv, x), dv.sum((0, 1)), dwj, dbj, dg1, dbe1,
             dw0, db0, dw2, db2, dg2, dbe2]
    return dx, grads


def bce_head(y, wf, bf, target):
    """BCEWithLogitsLoss() (mean) of Linear(D, 2) per breath against the window target repeated over the breaths ->
    (loss, logits, dy, dwf, dbf)."""
    z = y @ wf.T + bf
    t = np.broadcast_to(target[:, None, :], z.shape)
    loss = (np.maximum(z, 0) - z * t + np.log1p(np.exp(-np.abs(z)))).mean()
    dz = (1 / (1 + np.exp(-z)) - t) / z.size
    return loss, z, dz @ wf, np.einsum('btm,btn->mn', dz, y), dz.sum((0, 1))


def transformer_loss(x, blocks, wf, bf, target, masks=None, p=0.0):
    """The whole head: blocks (a list of 16-array lists), linear_final, BCE.  -> dict(y, logits, loss, dx, weights
    [per block], grads [per block: 16 arrays], dwf, dbf) in the dtype of x."""
    dt = x.dtype
    blocks = [[np.asarray(a, dt) for a in P] for P in blocks]
    wf, bf, target = np.asarray(wf, dt), np.asarray(bf, dt), np.asarray(target, dt)
    caches, h = [], x
    for i, P in enumerate(blocks):
        h, c = block_forward(h, P, None if masks is None else masks[i], p)
        caches.append(c)
    loss, logits, dy, dwf, dbf = bce_head(h, wf, bf, target)
    grads = [None] * len(blocks)
    for i in reversed(range(len(blocks))):
        dy, grads[i] = block_backward(dy, caches[i])
    return dict(y=h, logits=logits, loss=loss, dx=dy, weights=[c['weights'] for c in caches], grads=grads, dwf=dwf, dbf=dbf)


def rel_l2(a, b):
    nb = float(np.linalg.norm(np.asarray(b, np.float64)))
    return float(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / (nb if nb > 0 else 1.0))


def model_reference(g, backbone, dtype=np.float64):
    """The whole cnn_transformer model of a tests/golden/tfm_model_* file in the oracle: np_ref's breath block on the
    seeded backbone with this module's head, in the form decision_match wants (grads, tape, rebackward; + logits, loss).
    ``dtype``: the arithmetic of the whole run (float32: the noise figure of decision_match.fp32_noise)."""
    from oracle.weights import seeded_params
    from decision_match import feature_reference
    x64, t64 = g['x'].astype(dtype), g['target'].astype(dtype)
    b, nb = x64.shape[:2]
    p64 = {k: v.astype(dtype) for k, v in seeded_params(backbone, int(g['seed']), bn_bias_shift=float(g['bn_bias_shift']),
                                                             head='single_breath').items() if k.startswith('breath_block.')}
    nblocks = int(g['blocks'])
    blocks = [[g['param/transformer.blocks.%d.%s' % (i, n)].astype(dtype) for n in PARAM_NAMES] for i in range(nblocks)]
    wf, bf = g['param/linear_final.weight'].astype(dtype), g['param/linear_final.bias'].astype(dtype)

    def head(feat):
        o = transformer_loss(feat.reshape(b, nb, -1), blocks, wf, bf, t64)
        grads = {'linear_final.weight': o['dwf'], 'linear_final.bias': o['dbf']}
        for i in range(nblocks):
            for n, a in zip(PARAM_NAMES, o['grads'][i]):
                grads['transformer.blocks.%d.%s' % (i, n)] = a
        return o['dx'].reshape(feat.shape), dict(logits=o['logits'], loss=o['loss'], grads=grads)
    return feature_reference(p64, nb, x64.reshape(b * nb, 1, -1), head, backbone, first_pool_type=str(g['first_pool_type']))
