"""Host side of csrc/seq_wide.hip: checked wrappers around ``da_seqw_*``, the whole-patient recurrences of the nested networks
(reference models/cnn_to_nested_layer.py: nn.RNN(128, 128) / nn.LSTM(128, 128) over the W window vectors of one patient).
PyTorch allocates and orders streams; all arithmetic is in the kernels.  The autograd Functions around them
(WideRNNFunction / WideLSTMFunction) are in functional.py."""
import torch

from . import _lib
from . import hip_ops as H

HIDDEN = 128                     # the one hidden size da_seqw_* accept
RNN, LSTM = 0, 1                 # ``kind`` of da_seqw_shape_ok
GATES = {RNN: 1, LSTM: 4}


def shape_ok(kind, h, t):
    """Whether the kernels of ``kind`` ('rnn' / 'lstm' or RNN / LSTM) run hidden size ``h`` over ``t`` steps; launches nothing."""
    kind = {'rnn': RNN, 'lstm': LSTM}.get(kind, kind)
    return bool(_lib.lib().da_seqw_shape_ok(int(kind), int(h), int(t)))


def _check(kind, gx, w_hh, b_ih=None, b_hh=None):
    who = 'seqw_lstm' if kind == LSTM else 'seqw_rnn'
    H._f32(gx, 'gx')
    H._f32(w_hh, 'w_hh')
    g = GATES[kind] * HIDDEN
    if gx.dim() != 3 or gx.shape[2] != g or tuple(w_hh.shape) != (g, HIDDEN):
        raise ValueError('%s: gx must be (S, T, %d) and w_hh (%d, %d) -- the hidden size is %d, nothing else is built; got %s %s'
                         % (who, g, g, HIDDEN, HIDDEN, tuple(gx.shape), tuple(w_hh.shape)))
    s, t, _ = gx.shape
    if not shape_ok(kind, HIDDEN, t):
        raise ValueError('%s: a sequence needs T >= 1 steps, got %d' % (who, t))
    for b, name in ((b_ih, 'b_ih'), (b_hh, 'b_hh')):
        if b is not None:
            H._f32(b, name)
            if tuple(b.shape) != (g,):
                raise ValueError('%s: %s must be (%d,), got %s' % (who, name, g, tuple(b.shape)))
    return s, t


def _like(gx, *shape):
    return torch.empty(shape, device=gx.device, dtype=torch.float32)


def rnn_fwd(gx, w_hh, b_ih, b_hh):
    """gx (S, T, 128) = x W_ih^T -> hs (S, T, 128): h_t = tanh(gx_t + b_ih + b_hh + W_hh h_{t-1}) from a zero state."""
    s, t = _check(RNN, gx, w_hh, b_ih, b_hh)
    hs = _like(gx, s, t, HIDDEN)
    H._chk(_lib.lib().da_seqw_rnn_fwd(H._p(gx), H._p(w_hh), H._p(b_ih), H._p(b_hh), H._p(hs), s, t, HIDDEN, H._stream()),
           'da_seqw_rnn_fwd')
    return hs


def rnn_bwd(dhs, w_hh, hs):
    """dhs (S, T, 128) -> dz (S, T, 128), the gradient on the pre-activations."""
    s, t = _check(RNN, dhs, w_hh)
    H._f32(hs, 'hs')
    if hs.shape != dhs.shape:
        raise ValueError('seqw_rnn_bwd: hs %s does not match dhs %s' % (tuple(hs.shape), tuple(dhs.shape)))
    dz = _like(dhs, s, t, HIDDEN)
    H._chk(_lib.lib().da_seqw_rnn_bwd(H._p(dhs), H._p(w_hh), H._p(hs), H._p(dz), s, t, HIDDEN, H._stream()), 'da_seqw_rnn_bwd')
    return dz


def lstm_fwd(gx, w_hh, b_ih, b_hh):
    """gx (S, T, 512) = x W_ih^T (gate order i, f, g, o) -> hs, cs (S, T, 128) and the activated gates (S, T, 128, 4)
    (unit-major: what the backward reads back, 2 560 bytes per step with cs)."""
    s, t = _check(LSTM, gx, w_hh, b_ih, b_hh)
    hs, cs, gates = _like(gx, s, t, HIDDEN), _like(gx, s, t, HIDDEN), _like(gx, s, t, HIDDEN, 4)
    H._chk(_lib.lib().da_seqw_lstm_fwd(H._p(gx), H._p(w_hh), H._p(b_ih), H._p(b_hh), H._p(hs), H._p(cs), H._p(gates), s, t, HIDDEN,
                                       H._stream()), 'da_seqw_lstm_fwd')
    return hs, cs, gates


def lstm_bwd(dhs, w_hh, cs, gates):
    """dhs (S, T, 128) -> dz (S, T, 512), the gradient on the four pre-activations in torch's row order."""
    H._f32(dhs, 'dhs')
    H._f32(cs, 'cs')
    H._f32(gates, 'gates')
    if dhs.dim() != 3 or dhs.shape[2] != HIDDEN or cs.shape != dhs.shape or tuple(gates.shape) != tuple(dhs.shape) + (4,):
        raise ValueError('seqw_lstm_bwd: dhs / cs must be (S, T, %d) and gates (S, T, %d, 4), got %s %s %s'
                         % (HIDDEN, HIDDEN, tuple(dhs.shape), tuple(cs.shape), tuple(gates.shape)))
    s, t, _ = dhs.shape
    _check(LSTM, gates.view(s, t, 4 * HIDDEN), w_hh)
    dz = _like(dhs, s, t, 4 * HIDDEN)
    H._chk(_lib.lib().da_seqw_lstm_bwd(H._p(dhs), H._p(w_hh), H._p(cs), H._p(gates), H._p(dz), s, t, HIDDEN, H._stream()),
           'da_seqw_lstm_bwd')
    return dz
