"""The per-breath losses of the reference's ``deepards/loss.py`` as wrappers of the C ABI (``da_confidence_loss``,
``da_vacillating_loss``; kernels in csrc/head_optim.hip beside ``da_bce_logits``).  Reached as ``hip_ops.confidence_loss`` /
``hip_ops.vacillating_loss``; same conventions as ``hip_ops.bce_logits``: contiguous float32 CUDA operands, the current
stream, no host synchronisation, ``want_grad`` selects the gradient, ``gscale`` multiplies the gradient only."""
import torch

from . import hip_ops as _H


def _breath_loss(entry, name, logits, target, param, want_grad, gscale):
    _H._f32(logits, 'logits')
    _H._f32(target, 'target')
    if logits.dim() not in (2, 3) or logits.shape[-1] != 2 or tuple(target.shape) != (logits.shape[0], 2):
        raise ValueError('%s: logits %s must be (B, 2) or (B, NB, 2) and target %s (B, 2)'
                         % (name, tuple(logits.shape), tuple(target.shape)))
    if logits.numel() == 0:
        raise ValueError('%s: empty logits' % name)
    nb = logits.shape[1] if logits.dim() == 3 else 1
    loss = torch.empty((1,), device=logits.device, dtype=torch.float32)
    d = torch.empty_like(logits) if want_grad else None
    _H._chk(entry(_H._p(logits), _H._p(target), logits.shape[0], nb, param, gscale, _H._p(loss), _H._p(d), _H._stream()), name)
    return loss, d


def confidence_loss(logits, target, beta=1.0, want_grad=True, gscale=1.0):
    """ConfidencePenaltyLoss(beta) (loss.py:26-35) on logits (B, 2) or (B, NB, 2) and window targets (B, 2), repeated
    over the breaths -> loss (1,), dlogits (same shape as logits) or None."""
    return _breath_loss(_H._lib.lib().da_confidence_loss, 'da_confidence_loss', logits, target, float(beta), want_grad, gscale)


def vacillating_loss(logits, target, alpha=float('inf'), want_grad=True, gscale=1.0):
    """VacillatingLoss(alpha) (loss.py:7-23) on per-breath logits (B, NB, 2) and window targets (B, 2) -> loss (1,),
    dlogits or None.  Window-level logits make every class mean 0.5 up to rounding (the reference sums over the class
    axis there): refused."""
    if logits.dim() != 3:
        raise ValueError('the vacillating loss is only defined on per-breath outputs (B, NB, 2): with %s the reference averages '
                         'the softmax over the CLASS axis, every mean is 0.5 and the term is a constant or an exception'
                         % (tuple(logits.shape),))
    if not float(alpha) > 0:
        raise ValueError('vacillating loss: alpha must be > 0 (inf allowed)')
    return _breath_loss(_H._lib.lib().da_vacillating_loss, 'da_vacillating_loss', logits, target, float(alpha), want_grad, gscale)
