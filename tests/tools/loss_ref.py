"""numpy restatement (float64, or the ``dtype`` asked for: float32 gives the noise figure of decision_match.fp32_noise)
of the reference's two per-breath losses (deepards/loss.py) and their gradients, written from the formulas, not from the kernels: tests/test_losses_cpu.py pins it to the goldens captured from the reference
(tests/golden/loss_*.npz, 1e-10) and to central finite differences; the GPU tests chain its gradient through the
oracle's model restatement.

    logits (W, NB, 2) or (W, 2) (confidence only), target (W, 2) one-hot, repeated over the breaths.
"""
import numpy as np


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def _softmax(x):
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def _log_softmax(x):
    m = x.max(axis=-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def _repeat(logits, target):
    return np.broadcast_to(target[:, None, :], logits.shape) if logits.ndim == 3 else target


def bce_mean(logits, target, dtype=np.float64):
    """torch.nn.BCEWithLogitsLoss() (mean) with the window target repeated over the breaths -> loss, d loss / d logits."""
    x, t = np.asarray(logits, dtype=dtype), _repeat(logits, np.asarray(target, dtype=dtype))
    loss = (np.maximum(x, 0) - x * t + np.log1p(np.exp(-np.abs(x)))).mean()
    return float(loss), (_sigmoid(x) - t) / x.size


def confidence(logits, target, beta, dtype=np.float64):
    """ConfidencePenaltyLoss(beta), loss.py:32-35: BCE mean + beta * mean over all elements of p log p."""
    x = np.asarray(logits, dtype=dtype)
    beta = x.dtype.type(beta)
    bce, dbce = bce_mean(x, target, dtype)
    p, lp = _softmax(x), _log_softmax(x)
    s = (p * lp).sum(axis=-1, keepdims=True)
    loss = bce + beta * (p * lp).mean()
    return float(loss), dbce + beta * p * (lp - s) / x.size


def class_means(logits):
    """x[w, c]: mean over the breaths of softmax(logits[w, t, :])[c]."""
    return _softmax(np.asarray(logits, dtype=np.float64)).mean(axis=1)


def vacillating(logits, target, alpha, dtype=np.float64):
    """VacillatingLoss(alpha), loss.py:15-23: BCE mean + mean over (W, 2) of v(x); v(x) = -log(2 (e^-alpha - 1) x + 1) for
    x < 0.5, -log(2 e^-alpha (1 - x) + 2 x - 1) for x > 0.5 (x == 0.5 -- the reference raises -- takes the left branch)."""
    x = np.asarray(logits, dtype=dtype)
    if x.ndim != 3:
        raise ValueError('the vacillating loss needs per-breath logits (W, NB, 2)')
    w, nb, _ = x.shape
    ea = np.exp(-x.dtype.type(alpha))
    bce, dbce = bce_mean(x, target, dtype)
    p = _softmax(x)
    xm = p.mean(axis=1)                                               # (W, 2)
    left = xm <= 0.5
    arg = np.where(left, 2 * (ea - 1) * xm + 1, 2 * ea * (1 - xm) + 2 * xm - 1)
    darg = np.where(left, 2 * (ea - 1), 2 - 2 * ea)
    loss = bce + (-np.log(arg)).mean()
    dv = -darg / arg / (2 * w)                                        # d loss / d xm
    dp = np.broadcast_to(dv[:, None, :] / nb, p.shape)                # d loss / d p
    dx = p * (dp - (dp * p).sum(axis=-1, keepdims=True))              # softmax backward
    return float(loss), dbce + dx


def finite_difference(fn, logits, eps=1e-6):
    """Central differences of the scalar fn(logits) over every logit."""
    x = np.array(logits, dtype=np.float64)
    g = np.zeros_like(x)
    for i in np.ndindex(*x.shape):
        old = x[i]
        x[i] = old + eps
        up = fn(x)
        x[i] = old - eps
        dn = fn(x)
        x[i] = old
        g[i] = (up - dn) / (2 * eps)
    return g
