"""Host side of csrc/regress.hip: checked wrappers around ``da_regress_*`` and the autograd node of the regression head
(reference models/torch_cnn_bm_regressor.py: ``linear_final(breath_block(x).squeeze())`` and the ``MSELoss`` of its training
loop; the breath block's AvgPool1d(7) is pooled here, from its last map).  PyTorch allocates and orders streams; all arithmetic
is in the kernels."""
import torch
from torch.autograd import Function

from . import _lib
from . import functional as F_
from . import hip_ops as H

FLAT, MAP = 0, 1
POOL = 7
MAX_OUTPUTS = 16
ROWS_PER_BLOCK = 8          # csrc/regress.hip RG_ROWS (tests hold the twin against da_regress_rows_per_block)


def regress_rows_per_block():
    """Rows one block of the head's row kernels takes."""
    return _lib.lib().da_regress_rows_per_block()


def regress_shape_ok(r, f, m, form):
    """Python twin of ``da_regress_shape_ok`` (no library needed)."""
    return form in (FLAT, MAP) and 1 <= r <= 1 << 24 and 1 <= f <= 1 << 20 and 1 <= m <= MAX_OUTPUTS and r * POOL * f < 1 << 40


def regress_workspace(r, f, m):
    """Python twin of ``da_regress_workspace``: bytes of the backward's partial rows, 0 for a refused shape."""
    if not regress_shape_ok(r, f, m, FLAT):
        return 0
    return (r + ROWS_PER_BLOCK - 1) // ROWS_PER_BLOCK * m * f * 4


def _one_pitch(x):
    """Whether the strides of a map (R, 7, F) / of features (R, F) are what the kernels address: unit columns, one pitch >= F
    between positions, rows 7 pitches apart (the flat form: a row pitch >= F)."""
    r, f = x.shape[0], x.shape[-1]
    if x.dim() == 3:
        ld = x.stride(1)
        return x.stride(2) == 1 and ld >= f and (r == 1 or x.stride(0) == POOL * ld)
    return x.stride(1) == 1 and (r == 1 or x.stride(0) >= f)


def _operand(x, name):
    """x: the map (R, 7, F) or flat features (R, F), float32 CUDA, unit column stride, one pitch for positions and rows (a
    channel slice of a wider buffer is fine) -> (form, R, F, pitch)."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() in (2, 3) and x.shape[0] >= 1 and x.shape[-1] >= 1):
        raise ValueError('regression head: %s must be a float32 CUDA map (R, 7, F) or features (R, F), got %s %s'
                         % (name, tuple(x.shape), x.dtype))
    r, f = x.shape[0], x.shape[-1]
    if x.dim() == 3 and x.shape[1] != POOL:
        raise ValueError('regression head: the map must have the %d positions AvgPool1d(7) pools, got %s' % (POOL, tuple(x.shape)))
    if not _one_pitch(x):
        raise ValueError('regression head: %s must have contiguous columns and one pitch, got strides %s' % (name, x.stride()))
    if x.dim() == 3:
        return MAP, r, f, x.stride(1)
    return FLAT, r, f, x.stride(0) if r > 1 else max(f, x.stride(0))


def _check_params(w, bias, target, r, f):
    H._f32(w, 'linear_final.weight')
    H._f32(bias, 'linear_final.bias')
    H._f32(target, 'target')
    m = w.shape[0] if w.dim() == 2 else -1
    if w.dim() != 2 or w.shape[1] != f or tuple(bias.shape) != (m,):
        raise ValueError('regression head: linear_final must be (M, %d) with a bias (M,), got %s and %s' %
                         (f, tuple(w.shape), tuple(bias.shape)))
    if tuple(target.shape) != (r, m):
        raise ValueError('regression head: target must be (%d, %d), got %s' % (r, m, tuple(target.shape)))
    if not regress_shape_ok(r, f, m, FLAT):
        raise ValueError('regression head: R = %d, F = %d, M = %d is outside what the kernels take (1 <= M <= %d)' %
                         (r, f, m, MAX_OUTPUTS))
    return m


def regress_fwd(x, w, bias, target, bufs=None):
    """x: the map (R, 7, F) or features (R, F) -> (feat (R, F) -- the pooled features; x itself in the flat form --, out (R, M),
    loss (1,)).  Two launches.  ``bufs``: the (feat, out, loss) destinations (feat None in the flat form)."""
    form, r, f, ld = _operand(x, 'x')
    m = _check_params(w, bias, target, r, f)
    dev = x.device
    if bufs is not None:
        feat, out, loss = bufs
        for t, shape, name in ((feat, (r, f), 'feat'), (out, (r, m), 'out'), (loss, (1,), 'loss')):
            if t is None and name == 'feat' and form == FLAT:
                continue
            H._f32(t, name)
            if tuple(t.shape) != shape:
                raise ValueError('regress_fwd: %s must be %s, got %s' % (name, shape, tuple(t.shape)))
    else:
        feat = torch.empty((r, f), device=dev, dtype=torch.float32) if form == MAP else None
        out = torch.empty((r, m), device=dev, dtype=torch.float32)
        loss = torch.empty((1,), device=dev, dtype=torch.float32)
    H._chk(_lib.lib().da_regress_fwd(H._p(x), ld, form, H._p(w), H._p(bias), H._p(target), H._p(feat), H._p(out), H._p(loss),
                                     r, f, m, H._stream()), 'da_regress_fwd')
    return (feat if form == MAP else x), out, loss


def regress_bwd(feat, w, out, target, form, dx=None, dparams=None, accumulate=False, gscale=1.0, workspace=None):
    """From the forward's feat and out -> (dx, (dW, db)).  ``dx``: the destination, (R, 7, F) (``form`` MAP) or (R, F), may be a
    channel slice of a wider buffer; ``dparams``: the two parameter-gradient destinations, (+)= with ``accumulate``.  Two
    launches."""
    fform, r, f, ldf = _operand(feat, 'feat')
    if fform != FLAT:
        raise ValueError('regress_bwd: feat must be (R, F)')
    H._f32(w, 'linear_final.weight')
    m = w.shape[0]
    H._f32(out, 'out')
    H._f32(target, 'target')
    if w.dim() != 2 or w.shape[1] != f or tuple(out.shape) != (r, m) or tuple(target.shape) != (r, m):
        raise ValueError('regress_bwd: linear_final (M, %d), out and target (%d, M) expected, got %s, %s, %s' %
                         (f, r, tuple(w.shape), tuple(out.shape), tuple(target.shape)))
    if form not in (FLAT, MAP) or not regress_shape_ok(r, f, m, form):
        raise ValueError('regress_bwd: R = %d, F = %d, M = %d, form %r is outside what the kernels take' % (r, f, m, form))
    dev = feat.device
    if dx is None:
        dx = torch.empty((r, POOL, f) if form == MAP else (r, f), device=dev, dtype=torch.float32)
    dform, dr, df, ldg = _operand(dx, 'dx')
    if (dform, dr, df) != (form, r, f):
        raise ValueError('regress_bwd: dx %s does not match the operand (R = %d, F = %d, form %d)' % (tuple(dx.shape), r, f, form))
    if dparams is None:
        if accumulate:
            raise ValueError('regress_bwd: accumulate needs dparams')
        dparams = (torch.empty_like(w), torch.empty((m,), device=dev, dtype=torch.float32))
    for gp, shape in zip(dparams, ((m, f), (m,))):
        if tuple(gp.shape) != shape or gp.dtype != torch.float32 or not gp.is_contiguous() or not gp.is_cuda:
            raise ValueError('regress_bwd: a gradient destination does not match its parameter')
    need = regress_workspace(r, f, m) // 4
    if workspace is None:
        workspace = torch.empty((need,), device=dev, dtype=torch.float32)
    elif not (workspace.is_cuda and workspace.dtype == torch.float32 and workspace.is_contiguous() and workspace.numel() >= need):
        raise ValueError('regress_bwd: workspace must be a contiguous float32 CUDA tensor of at least %d elements' % need)
    H._chk(_lib.lib().da_regress_bwd(H._p(feat), ldf, H._p(w), H._p(out), H._p(target), H._p(dx), ldg, form, H._p(dparams[0]),
                                     H._p(dparams[1]), H._p(workspace), float(gscale), 1 if accumulate else 0, r, f, m,
                                     H._stream()), 'da_regress_bwd')
    return dx, tuple(dparams)


class RegressHeadFunction(Function):
    """Pool, linear_final and MSELoss of one batch as ONE autograd node over the forward and the backward call: x the breath
    block's last map (R, 7, F) or its flat features (R, F), target (R, M) -> (loss (1,), out (R, M)).  Complete on return.  The
    backward takes no upstream gradient into account beyond d(loss) = 1 -- what the trainer's ``loss.backward()`` means -- and
    writes the parameter gradients straight into a trainer's destinations when both parameters have one (overwriting in a
    step captured without the zero-fill).  Saved: the pooled features (R F floats; the flat operand itself), out, target -- not
    the map."""

    @staticmethod
    def forward(ctx, x, w, bias, target):
        if x.dim() in (2, 3) and not _one_pitch(x):
            x = x.contiguous()
        form = _operand(x, 'x')[0]
        target = target.contiguous()
        feat, out, loss = regress_fwd(x, w, bias, target)
        ctx.save_for_backward(feat, w, out, target)
        ctx.form = form
        ctx.gt = F_._tgt(w, bias)
        ctx.mark_non_differentiable(out)
        ctx.set_materialize_grads(False)
        return loss, out

    @staticmethod
    def backward(ctx, _dloss, _dout=None):
        feat, w, out, target = ctx.saved_tensors
        direct = all(t is not None for t in ctx.gt)
        dx, dparams = regress_bwd(feat, w, out, target, ctx.form, dparams=ctx.gt if direct else None,
                                  accumulate=direct and F_._acc())
        return (dx,) + ((None, None) if direct else dparams) + (None,)


class RegressLinearFunction(Function):
    """``CNNRegressor.forward``: pool + linear_final alone, x -> out (R, M), through the same kernels.  The forward runs against
    a zero target (its loss is dropped); the backward hands the upstream gradient to ``da_regress_bwd`` in the place of ``out``,
    with a zero target and gscale = R M / 2, so that the kernel's d = 2 (dout - 0) (gscale / (R M)) = dout exactly."""

    @staticmethod
    def forward(ctx, x, w, bias, grad_mode):
        if x.dim() in (2, 3) and not _one_pitch(x):
            x = x.contiguous()
        form = _operand(x, 'x')[0]
        zero = torch.zeros((x.shape[0], w.shape[0]), device=x.device, dtype=torch.float32)
        feat, out, _ = regress_fwd(x, w, bias, zero)
        if grad_mode:
            ctx.save_for_backward(feat, w, zero)
            ctx.form = form
            ctx.gt = F_._tgt(w, bias)
        return out

    @staticmethod
    def backward(ctx, dout):
        feat, w, zero = ctx.saved_tensors
        direct = all(t is not None for t in ctx.gt)
        dx, dparams = regress_bwd(feat, w, dout.contiguous(), zero, ctx.form, dparams=ctx.gt if direct else None,
                                  accumulate=direct and F_._acc(), gscale=0.5 * zero.numel())
        return (dx,) + ((None, None) if direct else dparams) + (None,)


def regress_head_loss(x, w, bias, target):
    """(loss (1,), out (R, M)) through RegressHeadFunction."""
    return RegressHeadFunction.apply(x, w, bias, target)
