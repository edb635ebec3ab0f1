"""Host side of csrc/siamese.hip: checked wrappers around ``da_siamese_*`` and the autograd node of the siamese head
(reference models/siamese.py: ``linear_final(linear_intermediate(|compr - x|).view(B, -1))`` for the (anchor, positive) and the
(anchor, negative) pair of a triplet, and the two ``BCEWithLogitsLoss`` terms of its training loop).  PyTorch allocates and orders
streams; all arithmetic is in the kernels."""
import torch
from torch.autograd import Function

from . import _lib
from . import functional as F_
from . import hip_ops as H


def head_rows_per_block():
    """Rows of (B NB) one block of the head's row kernels takes."""
    return _lib.lib().da_siamese_head_rows_per_block()


def siamese_draw(anchor, pat_start, pat_count, seed, step, literal, out=None):
    """anchor (B,) int64 CUDA absolute indices, pat_start / pat_count (N,) int32 CUDA -> (4B,) [anchor | pos | anchor | neg]
    (``literal``) or (3B,) [anchor | pos | neg] int64: one launch, nothing read back.  ``seed`` and ``step`` are taken modulo
    2^32."""
    for t, dt, name in ((anchor, torch.int64, 'anchor'), (pat_start, torch.int32, 'pat_start'), (pat_count, torch.int32, 'pat_count')):
        if not (t.is_cuda and t.dtype == dt and t.dim() == 1 and t.is_contiguous()):
            raise ValueError('siamese_draw: %s must be a contiguous 1-D %s CUDA tensor' % (name, dt))
    b, n = anchor.numel(), pat_start.numel()
    if pat_count.numel() != n:
        raise ValueError('siamese_draw: pat_start and pat_count must have one entry per window')
    if n < 2 or b < 1:
        raise ValueError('siamese_draw: needs at least two windows and one anchor, got N = %d, B = %d' % (n, b))
    width = (4 if literal else 3) * b
    if out is None:
        out = torch.empty((width,), device=anchor.device, dtype=torch.int64)
    elif not (out.is_cuda and out.dtype == torch.int64 and out.is_contiguous() and tuple(out.shape) == (width,)):
        raise ValueError('siamese_draw: out must be a contiguous int64 CUDA tensor of shape (%d,)' % width)
    H._chk(_lib.lib().da_siamese_draw(H._p(anchor), H._p(pat_start), H._p(pat_count), H._p(out), b, n, int(seed) & 0xffffffff,
                                      int(step) & 0xffffffff, 1 if literal else 0, H._stream()), 'da_siamese_draw')
    return out


def _operand(t, name, rows, d):
    """A (rows, D) float32 CUDA view with unit column stride (a row slice of a wider or longer tensor is fine) -> its pitch."""
    if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and tuple(t.shape) == (rows, d) and t.stride(1) == 1
            and (rows == 1 or t.stride(0) >= d)):
        raise ValueError('siamese head: %s must be a (%d, %d) float32 CUDA tensor with contiguous rows, got %s %s' %
                         (name, rows, d, tuple(t.shape), t.stride()))
    return t.stride(0) if rows > 1 else d


def _check_head(ops, w1, b1, w2, b2, b, nb):
    rows = b * nb
    if b < 1 or nb < 1:
        raise ValueError('siamese head: B and NB must be at least 1')
    d = ops[0].shape[1] if ops[0].dim() == 2 else -1
    if d < 1:
        raise ValueError('siamese head: operands must be (B NB, D) with D >= 1')
    pitches = {_operand(t, n, rows, d) for t, n in zip(ops, ('fa_pos', 'fc_pos', 'fa_neg', 'fc_neg'))}
    if len(pitches) != 1:
        raise ValueError('siamese head: the four operands must share one row pitch')
    for t, shape, name in ((w1, (2, d), 'linear_intermediate.weight'), (b1, (2,), 'linear_intermediate.bias'),
                           (w2, (2, 2 * nb), 'linear_final.weight'), (b2, (2,), 'linear_final.bias')):
        H._f32(t, name)
        if tuple(t.shape) != shape:
            raise ValueError('siamese head: %s must be %s, got %s' % (name, shape, tuple(t.shape)))
    return rows, d, pitches.pop()


def siamese_head_fwd(fa_pos, fc_pos, fa_neg, fc_neg, w1, b1, w2, b2, b, nb):
    """-> u (2, B NB, 2), z (2, B, 2) [pair 0: positive, 1: negative], loss (1,)."""
    rows, d, ld = _check_head((fa_pos, fc_pos, fa_neg, fc_neg), w1, b1, w2, b2, b, nb)
    dev = fa_pos.device
    u = torch.empty((2, rows, 2), device=dev, dtype=torch.float32)
    z = torch.empty((2, b, 2), device=dev, dtype=torch.float32)
    loss = torch.empty((1,), device=dev, dtype=torch.float32)
    H._chk(_lib.lib().da_siamese_head_fwd(H._p(fa_pos), H._p(fc_pos), H._p(fa_neg), H._p(fc_neg), ld, H._p(w1), H._p(b1), H._p(w2),
                                          H._p(b2), H._p(u), H._p(z), H._p(loss), b, nb, d, H._stream()), 'da_siamese_head_fwd')
    return u, z, loss


def siamese_head_bwd(fa_pos, fc_pos, fa_neg, fc_neg, w1, b1, w2, b2, u, z, b, nb, grads=None, dparams=None, accumulate=False,
                     gscale=1.0):
    """-> (dfa_pos, dfc_pos, dfa_neg, dfc_neg), (dW1, db1, dW2, db2).  ``grads``: the four (B NB, D) destinations (row slices of
    one tensor are fine; dfa_neg is None and stays unwritten when fa_neg is fa_pos -- the anchor's gradient is then the sum of
    both pairs, in dfa_pos); ``dparams``: the four parameter-gradient destinations, (+)= with ``accumulate``."""
    rows, d, ld = _check_head((fa_pos, fc_pos, fa_neg, fc_neg), w1, b1, w2, b2, b, nb)
    shared = fa_pos.data_ptr() == fa_neg.data_ptr()
    dev = fa_pos.device
    H._f32(u, 'u')
    H._f32(z, 'z')
    if tuple(u.shape) != (2, rows, 2) or tuple(z.shape) != (2, b, 2):
        raise ValueError('siamese_head_bwd: u must be (2, %d, 2) and z (2, %d, 2)' % (rows, b))
    if grads is None:
        g = torch.empty((3 if shared else 4, rows, d), device=dev, dtype=torch.float32)
        grads = (g[0], g[1], None, g[2]) if shared else (g[0], g[1], g[2], g[3])
    grads = tuple(grads)
    if shared and grads[2] is not None:
        raise ValueError('siamese_head_bwd: with a shared anchor dfa_neg is not written; pass None')
    live = [(t, n) for t, n in zip(grads, ('dfa_pos', 'dfc_pos', 'dfa_neg', 'dfc_neg')) if t is not None]
    if len(live) != (3 if shared else 4):
        raise ValueError('siamese_head_bwd: a gradient destination is missing')
    pitches = {_operand(t, n, rows, d) for t, n in live}
    if len(pitches) != 1:
        raise ValueError('siamese_head_bwd: the gradient destinations must share one row pitch')
    if dparams is None:
        if accumulate:
            raise ValueError('siamese_head_bwd: accumulate needs dparams')
        dparams = (torch.empty_like(w1), torch.empty_like(b1), torch.empty_like(w2), torch.empty_like(b2))
    for gp, p in zip(dparams, (w1, b1, w2, b2)):
        if gp.shape != p.shape or gp.dtype != torch.float32 or not gp.is_contiguous() or not gp.is_cuda:
            raise ValueError('siamese_head_bwd: a gradient destination does not match its parameter')
    ws = _lib.lib().da_siamese_head_bwd_workspace(b, nb, d)
    work = torch.empty((max(ws // 4, 1),), device=dev, dtype=torch.float32)
    H._chk(_lib.lib().da_siamese_head_bwd(H._p(fa_pos), H._p(fc_pos), H._p(fa_neg), H._p(fc_neg), ld, H._p(w1), H._p(w2), H._p(u),
                                          H._p(z), H._p(grads[0]), H._p(grads[1]), H._p(grads[2]), H._p(grads[3]), pitches.pop(),
                                          H._p(dparams[0]), H._p(dparams[1]), H._p(dparams[2]), H._p(dparams[3]), H._p(work),
                                          float(gscale), 1 if accumulate else 0, b, nb, d, H._stream()), 'da_siamese_head_bwd')
    return grads, tuple(dparams)


def triplet_slices(feats, b, nb, literal):
    """The four head operands as row slices of ``feats`` ((4 or 3) B NB, D): [anchor | pos | anchor | neg] or, shared,
    [anchor | pos | neg] (fa_neg is then fa_pos itself)."""
    rows = b * nb
    want = (4 if literal else 3) * rows
    if feats.dim() != 2 or feats.shape[0] != want:
        raise ValueError('siamese head: features must be (%d, D) for B = %d, NB = %d, %s anchor; got %s' %
                         (want, b, nb, 'separate' if literal else 'shared', tuple(feats.shape)))
    if literal:
        return feats[:rows], feats[rows:2 * rows], feats[2 * rows:3 * rows], feats[3 * rows:]
    return feats[:rows], feats[rows:2 * rows], feats[:rows], feats[2 * rows:]


class SiameseHeadFunction(Function):
    """The head and loss of one triplet batch as ONE autograd node over the forward and the backward call: feats ((4 or 3) B NB,
    D) the tower's output for [anchor | pos | anchor | neg] (``literal``) or [anchor | pos | neg] -> (loss (1,), z (2, B, 2)).
    Complete on return.  The backward takes no upstream gradient into account beyond d(loss) = 1 -- what the trainer's
    ``loss.backward()`` means -- and writes the parameter gradients straight into a trainer's destinations when all four
    parameters have one (overwriting in a step captured without the zero-fill)."""

    @staticmethod
    def forward(ctx, feats, w1, b1, w2, b2, b, nb, literal):
        feats = feats.contiguous()
        ops = triplet_slices(feats, b, nb, literal)
        u, z, loss = siamese_head_fwd(*ops, w1, b1, w2, b2, b, nb)
        ctx.save_for_backward(feats, w1, b1, w2, b2, u, z)
        ctx.dims = (b, nb, bool(literal))
        ctx.gt = F_._tgt(w1, b1, w2, b2)
        ctx.mark_non_differentiable(z)
        ctx.set_materialize_grads(False)
        return loss, z

    @staticmethod
    def backward(ctx, _dloss, _dz=None):
        feats, w1, b1, w2, b2, u, z = ctx.saved_tensors
        b, nb, literal = ctx.dims
        ops = triplet_slices(feats, b, nb, literal)
        dfeats = torch.empty_like(feats)
        g = triplet_slices(dfeats, b, nb, literal)
        grads = g if literal else (g[0], g[1], None, g[3])
        direct = all(t is not None for t in ctx.gt)
        _, dparams = siamese_head_bwd(*ops, w1, b1, w2, b2, u, z, b, nb, grads=grads, dparams=ctx.gt if direct else None,
                                      accumulate=direct and F_._acc())
        return (dfeats,) + ((None,) * 4 if direct else dparams) + (None, None, None)


def siamese_head_loss(feats, w1, b1, w2, b2, b, nb, literal):
    """(loss (1,), z_pos (B, 2), z_neg (B, 2)) through SiameseHeadFunction."""
    loss, z = SiameseHeadFunction.apply(feats, w1, b1, w2, b2, b, nb, literal)
    return loss, z[0], z[1]
