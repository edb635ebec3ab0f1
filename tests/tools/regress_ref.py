"""numpy reference of the regression head (csrc/regress.hip): both operand forms, forward and backward, in the dtype of its
operands -- float64 is the oracle of the GPU tests, float32 the yardstick's own error (``err32``: rel-l2 of the float32 run against
the float64 run on the same operands).  Plain numpy reductions: nothing here mirrors the kernels' summation order."""
import numpy as np

POOL = 7


def rel_l2(a, b):
    """||a - b|| / ||b|| in float64 (0 when both vanish)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    den = np.sqrt((b ** 2).sum())
    num = np.sqrt(((a - b) ** 2).sum())
    return 0.0 if num == 0 else num / den if den > 0 else np.inf


def forward(x, w, bias, target):
    """x: the map (R, 7, F) or flat features (R, F); w (M, F), bias (M,), target (R, M) -> dict(feat, out, loss)."""
    dt = x.dtype
    feat = x.sum(axis=1, dtype=dt) / dt.type(POOL) if x.ndim == 3 else x
    out = (feat @ w.T + bias).astype(dt)
    err = out - target
    loss = ((err * err).sum(dtype=dt) / dt.type(err.size)).astype(dt)
    return dict(feat=feat, out=out, loss=np.reshape(loss, (1,)))


def backward(x, w, out, target, gscale=1.0):
    """-> dict(dx (x's shape), dW (M, F), db (M,)) from the forward's out."""
    dt = x.dtype
    feat = x.sum(axis=1, dtype=dt) / dt.type(POOL) if x.ndim == 3 else x
    d = (dt.type(2.0) * (out - target) * dt.type(gscale) / dt.type(out.size)).astype(dt)
    dfeat = (d @ w).astype(dt)
    dx = np.repeat((dfeat / dt.type(POOL))[:, None, :], POOL, axis=1).astype(dt) if x.ndim == 3 else dfeat
    return dict(dx=dx, dW=(d.T @ feat).astype(dt), db=d.sum(axis=0, dtype=dt))


def run(x, w, bias, target, gscale=1.0, dtype=np.float64):
    """Forward and backward in ``dtype`` on (casts of) the operands -> one dict: feat, out, loss, dx, dW, db."""
    x, w, bias, target = (np.asarray(a, dtype=dtype) for a in (x, w, bias, target))
    res = forward(x, w, bias, target)
    res.update(backward(x, w, res['out'], target, gscale))
    return res


def make_case(r, f, m, form, seed=0):
    """float32 operands of one head call: a non-negative map (it is behind a ReLU) or features, weights of Linear's own scale, and
    target columns of mixed scale, 1e-2 ... 1e3, as raw breath metadata are (a tidal volume beside an I:E ratio)."""
    rng = np.random.RandomState(1000 * seed + 7 * r + 3 * f + m + 100003 * form)
    shape = (r, POOL, f) if form else (r, f)
    x = np.maximum(rng.randn(*shape), 0).astype(np.float32)
    bound = 1.0 / np.sqrt(f)
    w = rng.uniform(-bound, bound, (m, f)).astype(np.float32)
    bias = rng.uniform(-bound, bound, (m,)).astype(np.float32)
    scale = 10.0 ** np.linspace(-2, 3, m) if m > 1 else np.array([30.0])
    target = (rng.randn(r, m) * scale).astype(np.float32)
    return dict(x=x, w=w, bias=bias, target=target)
