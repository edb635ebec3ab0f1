"""Stock-torch restatement (float64 by default) of what the nested networks put behind the breath block, and of the bare
recurrences -- the reference of tests/test_nested_gpu.py, pinned to the real reference classes by tests/test_nested_cpu.py
(reference models/cnn_to_nested_layer.py:41-43 / :80-82, train_ards_detector.py:750-755).

    feat (W, NB, 128) --lower median over NB--> (1, W, 128) --nn.RNN / nn.LSTM(128, 128), zero state--> linear_final --> (1, W, 2)
"""
import glob
import os

import numpy as np
import torch

HIDDEN = 128
W, NB = 3, 4                     # the golden case of tests/tools/make_golden_nested.py: one patient of 3 windows of 4 breaths
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'golden')
PARAMS = ('weight_ih_l0', 'weight_hh_l0', 'bias_ih_l0', 'bias_hh_l0')


def load_golden(kind, directory=GOLDEN_DIR):
    """The merged golden record of ``kind`` ('rnn' / 'lstm'), written in parts below the size limit of a committed file, as a
    dict of numpy arrays."""
    parts = sorted(glob.glob(os.path.join(directory, 'nested_%s_w%d.p*.npz' % (kind, W))))
    assert parts, 'no golden parts for %s' % kind
    rec = {}
    for p in parts:
        with np.load(p, allow_pickle=False) as z:
            rec.update({k: z[k] for k in z.files})
    return rec


def _t(a, dtype):
    return torch.as_tensor(np.asarray(a)).to(dtype)


def module(kind, weights, dtype):
    """nn.RNN / nn.LSTM(128, 128, batch_first=True) in ``dtype`` holding ``weights`` = (w_ih, w_hh, b_ih, b_hh)."""
    m = (torch.nn.LSTM if kind == 'lstm' else torch.nn.RNN)(HIDDEN, HIDDEN, batch_first=True).to(dtype)
    with torch.no_grad():
        for name, w in zip(PARAMS, weights):
            getattr(m, name).copy_(_t(w, dtype))
    return m


def default_weights(kind, gen):
    """The four parameters under torch's default initialisation (uniform +- 1 / sqrt(H)), float32 CPU tensors."""
    g = (4 if kind == 'lstm' else 1) * HIDDEN
    k = 1.0 / np.sqrt(HIDDEN)
    u = lambda *s: (torch.rand(*s, generator=gen) * 2 - 1) * k
    return u(g, HIDDEN), u(g, HIDDEN), u(g), u(g)


def recurrence(kind, x, weights, dhs, dtype=torch.float64):
    """x (S, T, 128), dhs (S, T, 128) -> hs and the gradients of sum(hs * dhs) on w_ih, w_hh, b_ih, b_hh and x
    (float64 numpy: hs, [dw_ih, dw_hh, db_ih, db_hh, dx])."""
    m = module(kind, weights, dtype)
    xx = _t(x, dtype).clone().requires_grad_(True)
    hs = m(xx)[0]
    (hs * _t(dhs, dtype)).sum().backward()
    grads = [getattr(m, n).grad for n in PARAMS] + [xx.grad]
    return hs.detach().double().numpy(), [g.double().numpy() for g in grads]


def loss(logits, target, loss_calc):
    """NestedMixin.calc_loss: logits (1, W, 2), target (1, 2); BCEWithLogitsLoss (mean) on every window or on the last."""
    crit = torch.nn.BCEWithLogitsLoss()
    if loss_calc == 'all_breaths':
        return crit(logits, target.view(1, 1, 2).repeat(1, logits.shape[1], 1))
    if loss_calc == 'last_breath':
        return crit(logits[:, -1], target.view(1, 2))
    raise ValueError(loss_calc)


def head(kind, feat, weights, lin_w, lin_b, r=None, dtype=torch.float64):
    """feat (W, NB, 128) breath-block features -> dict: logits (1, W, 2), idx (W, 128) the breath each median selects, and --
    with ``r`` (1, W, 2) -- the gradients of sum(logits * r) on the six head parameters (state_dict names without the
    ``rnn.`` / ``lstm.`` prefix for the four recurrent ones) and on feat.  float64 numpy."""
    m = module(kind, weights, dtype)
    lw, lb = _t(lin_w, dtype).clone().requires_grad_(True), _t(lin_b, dtype).clone().requires_grad_(True)
    f = _t(feat, dtype).clone().requires_grad_(True)
    med, idx = f.median(dim=1)
    logits = torch.nn.functional.linear(m(med.unsqueeze(0))[0], lw, lb)
    out = {'logits': logits.detach().double().numpy(), 'idx': idx.numpy(), 'median': med.detach().double().numpy()}
    if r is not None:
        (logits * _t(r, dtype)).sum().backward()
        for n in PARAMS:
            out['grad/' + n] = getattr(m, n).grad.double().numpy()
        out['grad/linear_final.weight'], out['grad/linear_final.bias'] = lw.grad.double().numpy(), lb.grad.double().numpy()
        out['grad/feat'] = f.grad.double().numpy()
    return out
