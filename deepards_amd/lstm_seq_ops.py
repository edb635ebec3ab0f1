"""Host side of csrc/lstm_seq.hip: checked wrappers around ``da_lstm_seq_*`` and the two autograd Functions of the lstm_only
networks (reference models/lstm_only.py) -- the waveform LSTM over every breath row and the per-breath projection behind it.
PyTorch allocates and orders streams; all arithmetic is in the kernels."""
import torch
from torch.autograd import Function

from . import _lib
from . import functional as F_
from . import hip_ops as H

HIDDEN_SIZES = tuple(range(8, 65, 8))          # what da_lstm_seq_* accept for H
PROJ_FEATURES = (16, 32, 48, 64)               # what da_lstm_seq_proj_* accept for F


def block_seqs(h):
    """Sequences one block of the recurrence kernels works on at hidden size ``h``."""
    n = _lib.lib().da_lstm_seq_block_seqs(int(h))
    if n < 1:
        raise ValueError('hidden size %r is not one of %s' % (h, HIDDEN_SIZES))
    return n


def _check_weights(w_ih, w_hh, b_ih, b_hh):
    h = w_hh.shape[1]
    if h not in HIDDEN_SIZES:
        raise ValueError('lstm_seq: hidden size must be one of %s, got %d' % (HIDDEN_SIZES, h))
    if tuple(w_hh.shape) != (4 * h, h) or w_ih.numel() != 4 * h or tuple(b_ih.shape) != (4 * h,) or tuple(b_hh.shape) != (4 * h,):
        raise ValueError('lstm_seq: weights must be w_ih (4H, 1), w_hh (4H, H), b_ih / b_hh (4H,), got %s %s %s %s' %
                         (tuple(w_ih.shape), tuple(w_hh.shape), tuple(b_ih.shape), tuple(b_hh.shape)))
    for t, name in ((w_ih, 'w_ih'), (w_hh, 'w_hh'), (b_ih, 'b_ih'), (b_hh, 'b_hh')):
        H._f32(t, name)
    return h


def lstm_seq_fwd(x, w_ih, w_hh, b_ih, b_hh, packed=False):
    """x (N, T) -> hs, cs (N, T, H), lens (N,) int32: nn.LSTM(1, H, batch_first=True) from a zero state on every row; with
    ``packed`` the rows stop behind their first exact zero (a row that starts with one runs whole) and hs is +0.0 there."""
    H._f32(x, 'x')
    if x.dim() != 2 or x.shape[1] < 1:
        raise ValueError('lstm_seq: x must be (N, T) with T >= 1, got %s' % (tuple(x.shape),))
    h = _check_weights(w_ih, w_hh, b_ih, b_hh)
    n, t = x.shape
    hs = torch.empty((n, t, h), device=x.device, dtype=torch.float32)
    cs = torch.empty((n, t, h), device=x.device, dtype=torch.float32)
    lens = torch.empty((n,), device=x.device, dtype=torch.int32)
    H._chk(_lib.lib().da_lstm_seq_fwd(H._p(x), H._p(w_ih), H._p(w_hh), H._p(b_ih), H._p(b_hh), 1 if packed else 0, H._p(hs),
                                      H._p(cs), H._p(lens), n, t, h, H._stream()), 'da_lstm_seq_fwd')
    return hs, cs, lens


def lstm_seq_bwd(dhs, x, w_ih, w_hh, b_ih, b_hh, hs, cs, lens, dw_ih=None, dw_hh=None, db=None, db2=None, accumulate=False):
    """dhs (N, T, H) -> dw_ih (4H, 1), dw_hh (4H, H), db (4H,) (for both biases; ``db2``, when given, receives it too); into
    the given tensors, (+)= with ``accumulate``."""
    H._f32(dhs, 'dhs')
    h = _check_weights(w_ih, w_hh, b_ih, b_hh)
    n, t = x.shape
    if tuple(dhs.shape) != (n, t, h) or tuple(hs.shape) != (n, t, h) or tuple(cs.shape) != (n, t, h) or lens.numel() != n:
        raise ValueError('lstm_seq_bwd: dhs / hs / cs must be (%d, %d, %d) and lens (%d,)' % (n, t, h, n))
    if lens.dtype != torch.int32:
        raise ValueError('lstm_seq_bwd: lens must be int32')
    given = [g is not None for g in (dw_ih, dw_hh, db)]
    if any(given) != all(given) or ((accumulate or db2 is not None) and not all(given)):
        raise ValueError('lstm_seq_bwd: pass all of dw_ih, dw_hh, db or none; accumulate and db2 need them')
    if not all(given):
        dw_ih, dw_hh, db = torch.empty_like(w_ih), torch.empty_like(w_hh), torch.empty_like(b_ih)
    for g, w in ((dw_ih, w_ih), (dw_hh, w_hh), (db, b_ih)) + (((db2, b_hh),) if db2 is not None else ()):
        if g.shape != w.shape or g.dtype != torch.float32 or not g.is_contiguous():
            raise ValueError('lstm_seq_bwd: a gradient destination does not match its parameter')
    ws = _lib.lib().da_lstm_seq_bwd_workspace(n, h)
    work = torch.empty((max(ws // 4, 1),), device=x.device, dtype=torch.float32)
    H._chk(_lib.lib().da_lstm_seq_bwd(H._p(dhs), H._p(x), H._p(w_ih), H._p(w_hh), H._p(b_ih), H._p(b_hh), H._p(hs), H._p(cs),
                                      H._p(lens), H._p(dw_ih), H._p(dw_hh), H._p(db), H._p(db2), H._p(work),
                                      1 if accumulate else 0, n, t, h, H._stream()), 'da_lstm_seq_bwd')
    return dw_ih, dw_hh, db


def _check_proj(rows, w, bias):
    H._f32(rows, 'rows')
    H._f32(w, 'weight')
    H._f32(bias, 'bias')
    n, k = rows.shape
    f = w.shape[0]
    if tuple(w.shape) != (f, k) or tuple(bias.shape) != (f,) or f not in PROJ_FEATURES or k % 4 or k < 4:
        raise ValueError('lstm_seq_proj: rows (N, K) with K a multiple of 4, weight (F, K), bias (F,), F one of %s; got %s %s %s'
                         % (PROJ_FEATURES, tuple(rows.shape), tuple(w.shape), tuple(bias.shape)))
    return n, k, f


def proj_fwd(rows, w, bias):
    """rows (N, K) -> (N, F) = rows w^T + bias (linear_breath_inst)."""
    n, k, f = _check_proj(rows, w, bias)
    y = torch.empty((n, f), device=rows.device, dtype=torch.float32)
    H._chk(_lib.lib().da_lstm_seq_proj_fwd(H._p(rows), H._p(w), H._p(bias), H._p(y), n, k, f, H._stream()), 'da_lstm_seq_proj_fwd')
    return y


def proj_bwd(dy, rows, w, bias, dw=None, dbias=None, accumulate=False):
    """dy (N, F) -> drows (N, K), dw (F, K), dbias (F,); the parameter gradients into the given tensors, (+)= with
    ``accumulate``."""
    n, k, f = _check_proj(rows, w, bias)
    H._f32(dy, 'dy')
    if tuple(dy.shape) != (n, f):
        raise ValueError('lstm_seq_proj_bwd: dy must be (%d, %d), got %s' % (n, f, tuple(dy.shape)))
    if (dw is None) != (dbias is None) or (accumulate and dw is None):
        raise ValueError('lstm_seq_proj_bwd: pass both dw and dbias or neither; accumulate needs them')
    if dw is None:
        dw, dbias = torch.empty_like(w), torch.empty_like(bias)
    for g, p in ((dw, w), (dbias, bias)):
        if g.shape != p.shape or g.dtype != torch.float32 or not g.is_contiguous():
            raise ValueError('lstm_seq_proj_bwd: a gradient destination does not match its parameter')
    drows = torch.empty_like(rows)
    ws = _lib.lib().da_lstm_seq_proj_bwd_workspace(n, k, f)
    work = torch.empty((max(ws // 4, 1),), device=rows.device, dtype=torch.float32)
    H._chk(_lib.lib().da_lstm_seq_proj_bwd(H._p(dy), H._p(rows), H._p(w), H._p(drows), H._p(dw), H._p(dbias), H._p(work),
                                           1 if accumulate else 0, n, k, f, H._stream()), 'da_lstm_seq_proj_bwd')
    return drows, dw, dbias


class WaveformLSTMFunction(Function):
    """``nn.LSTM(1, H, batch_first=True)`` from a zero state over the T samples of each of N rows (LSTMOnlyNetwork,
    models/lstm_only.py:57,65-67; with ``packed`` the pack_sequence / pad_packed_sequence round trip of LSTMOnlyWithPacking,
    :18-41): x (N, T) -> hs (N, T, H).  x is data and gets no gradient.  With a trainer's destinations on all four parameters
    the backward writes (or, outside an overwriting capture, accumulates) straight into the flat gradient bucket; db serves
    b_ih and b_hh."""

    @staticmethod
    def forward(ctx, x, w_ih, w_hh, b_ih, b_hh, packed):
        x = x.contiguous()
        hs, cs, lens = lstm_seq_fwd(x, w_ih, w_hh, b_ih, b_hh, packed)
        ctx.save_for_backward(x, w_ih, w_hh, b_ih, b_hh, hs, cs, lens)
        ctx.gt = F_._tgt(w_ih, w_hh, b_ih, b_hh)
        return hs

    @staticmethod
    def backward(ctx, dhs):
        x, w_ih, w_hh, b_ih, b_hh, hs, cs, lens = ctx.saved_tensors
        tih, thh, tbi, tbh = ctx.gt
        direct = all(g is not None for g in ctx.gt)
        if not direct:
            dw_ih, dw_hh, db = lstm_seq_bwd(dhs.contiguous(), x, w_ih, w_hh, b_ih, b_hh, hs, cs, lens)
            return None, dw_ih, dw_hh, db, db.clone(), None
        lstm_seq_bwd(dhs.contiguous(), x, w_ih, w_hh, b_ih, b_hh, hs, cs, lens, dw_ih=tih, dw_hh=thh, db=tbi, db2=tbh,
                     accumulate=F_._acc())
        return None, None, None, None, None, None


class BreathProjectionFunction(Function):
    """``linear_breath_inst`` = Linear(T H -> F) on every breath row (models/lstm_only.py:58,68): rows (N, K) -> (N, F)."""

    @staticmethod
    def forward(ctx, rows, w, bias):
        rows = rows.contiguous()
        ctx.save_for_backward(rows, w, bias)
        ctx.gt = F_._tgt(w, bias)
        return proj_fwd(rows, w, bias)

    @staticmethod
    def backward(ctx, dy):
        rows, w, bias = ctx.saved_tensors
        tw, tb = ctx.gt
        direct = tw is not None and tb is not None
        drows, dw, db = proj_bwd(dy.contiguous(), rows, w, bias, dw=tw if direct else None, dbias=tb if direct else None,
                                 accumulate=direct and F_._acc())
        return drows, None if direct else dw, None if direct else db
