"""Capture tests/golden/loss_*.npz from the reference's own ``deepards/loss.py``:

    python tests/tools/make_golden_losses.py <reference checkout> [<output dir, default tests/golden>]

Each file holds, for fixed seeded inputs: ``logits`` (float32 values), ``target`` (W, 2) one-hot, ``alpha`` or ``beta``,
and the reference's loss and d loss / d logits evaluated in float64 (``loss64``, ``grad64``) and in float32 (``loss32``,
``grad32``) -- arrays and scalars only.  The reference module is loaded from its file (nothing else of the reference is
imported); its criteria get the target repeated over the breaths, as PerBreathClassifierMixin.calc_loss hands it over.

Cases: vacillating at alpha in {inf, 2.0, 0.5} on (4, 20, 2) and (1, 20, 2); confidence at beta in {1.0, 0.25} on
(4, 20, 2) and (8, 2); one "decided" case each whose logits are scaled so that some class means exceed 0.99.
Condition on the vacillating inputs, asserted here: every |x - 0.5| >= 1e-3 (x: the class means), and the reference ran
without raising in both precisions (at x == 0.5 its two masks differ in size)."""
import importlib.util
import os
import sys

import numpy as np
import torch


def load_reference_losses(checkout):
    path = os.path.join(checkout, 'deepards', 'loss.py')
    spec = importlib.util.spec_from_file_location('reference_loss', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def inputs(seed, shape, decided=False):
    """Per-window leaning logits with breath-to-breath noise, rounded to float32; one-hot targets."""
    rng = np.random.RandomState(seed)
    w = shape[0]
    lean = rng.choice([-1.0, 1.0], size=(w,) + (1,) * (len(shape) - 1)) * rng.uniform(0.4, 1.6, size=(w,) + (1,) * (len(shape) - 1))
    x = rng.standard_normal(shape)
    x[..., 1] += lean[..., 0]
    x[..., 0] -= lean[..., 0]
    if decided:
        x = 0.5 * x
        x[..., 1] += 5.0 * np.sign(lean[..., 0])
        x[..., 0] -= 5.0 * np.sign(lean[..., 0])
    target = np.zeros((w, 2), dtype=np.float32)
    target[np.arange(w), rng.randint(0, 2, w)] = 1
    return x.astype(np.float32), target


def evaluate(make, logits, target, dtype):
    x = torch.tensor(logits, dtype=dtype, requires_grad=True)
    t = torch.tensor(target, dtype=dtype)
    if x.dim() == 3:
        t = t.unsqueeze(1).repeat(1, x.shape[1], 1)
    loss = make(dtype)(x, t)
    loss.backward()
    return loss.detach().numpy().reshape(()), x.grad.numpy()


def class_means(logits):
    e = np.exp(logits.astype(np.float64) - logits.max(axis=-1, keepdims=True))
    return (e / e.sum(axis=-1, keepdims=True)).mean(axis=1)


def main(argv):
    if len(argv) < 2:
        raise SystemExit(__doc__)
    ref = load_reference_losses(argv[1])
    out_dir = argv[2] if len(argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'golden')
    cases = []
    for ai, alpha in enumerate((float('inf'), 2.0, 0.5)):
        for shape in ((4, 20, 2), (1, 20, 2)):
            cases.append(('vac_a%s_%s' % ('inf' if np.isinf(alpha) else ('%g' % alpha).replace('.', 'p'), 'x'.join(map(str, shape[:-1]))),
                          'vacillating', alpha, shape, 100 + 10 * ai + shape[0], False))
    cases.append(('vac_ainf_4x20_decided', 'vacillating', float('inf'), (4, 20, 2), 171, True))
    for bi, beta in enumerate((1.0, 0.25)):
        for shape in ((4, 20, 2), (8, 2)):
            cases.append(('conf_b%s_%s' % (('%g' % beta).replace('.', 'p'), 'x'.join(map(str, shape[:-1]))),
                          'confidence', beta, shape, 200 + 10 * bi + shape[0], False))
    cases.append(('conf_b1_4x20_decided', 'confidence', 1.0, (4, 20, 2), 271, True))
    for name, kind, param, shape, seed, decided in cases:
        logits, target = inputs(seed, shape, decided)
        if kind == 'vacillating':
            xm = class_means(logits)
            assert np.abs(xm - 0.5).min() >= 1e-3, '%s: a class mean within 1e-3 of 0.5, choose another seed' % name
            make = lambda dt: ref.VacillatingLoss(torch.tensor([param], dtype=dt))
        else:
            xm = class_means(logits) if logits.ndim == 3 else None
            make = lambda dt: ref.ConfidencePenaltyLoss(param)
        if decided:
            assert xm.max() > 0.99, '%s: no class mean above 0.99' % name
        l64, g64 = evaluate(make, logits, target, torch.float64)         # (raises here if the reference raises)
        l32, g32 = evaluate(make, logits, target, torch.float32)
        assert np.isfinite(l64) and np.isfinite(g64).all() and np.isfinite(l32) and np.isfinite(g32).all(), name
        key = 'alpha' if kind == 'vacillating' else 'beta'
        np.savez(os.path.join(out_dir, 'loss_%s.npz' % name), logits=logits, target=target, kind=np.array(kind),
                 loss64=np.float64(l64), grad64=g64.astype(np.float64), loss32=np.float32(l32), grad32=g32.astype(np.float32),
                 **{key: np.float64(param)})
        print('%-28s loss64 %.12f |loss32-loss64| %.2e max|grad32-grad64| %.2e' %
              (name, l64, abs(float(l32) - float(l64)), np.abs(g32 - g64).max()))


if __name__ == '__main__':
    main(sys.argv)
