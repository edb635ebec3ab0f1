"""The networks that read the raw waveform with an LSTM and no CNN (reference models/lstm_only.py): LSTMOnlyNetwork (:46-69)
and LSTMOnlyWithPacking (:7-43).  Same constructor, class constants, children and ``state_dict`` keys; the modules only hold
the parameters (torch's default initialisation), the arithmetic is csrc/lstm_seq.hip through ``deepards_amd.lstm_seq_ops``.

The reference runs ``nn.LSTM(1, H, batch_first=True)`` window by window on (NB, 224, 1) from a zero state, so every breath row
is an independent sequence: here all B NB rows go through one launch.  Its reshape of (B, NB, 1, 224) to (B, NB, 224, 1)
(:34,:63) moves no data for one feature.  DoubleLSTMNetwork (:72-95) is not built: its second nn.LSTM is not batch_first, so
it recurs over the BATCH axis and couples the windows of a batch."""
import torch.nn as nn

from .. import functional as F_
from .. import lstm_seq_ops as S


class _WaveformLSTMNetwork(nn.Module):
    seq_len = 224
    packed = False

    def __init__(self, lstm_hidden_units, sub_batches):
        super(_WaveformLSTMNetwork, self).__init__()
        if lstm_hidden_units not in S.HIDDEN_SIZES:
            raise ValueError('%s: lstm_hidden_units must be one of %s (the waveform-LSTM kernels keep a row of weight_hh_l0 per '
                             'lane), got %r' % (type(self).__name__, S.HIDDEN_SIZES, lstm_hidden_units))
        self.lstm_breath_block = nn.LSTM(1, lstm_hidden_units, batch_first=True)
        self.linear_breath_inst = nn.Linear(lstm_hidden_units * self.seq_len, self.intermediate_features)
        self.linear_final = nn.Linear(self.intermediate_features * sub_batches, 2)
        self.lstm_hidden_units, self.sub_batches = lstm_hidden_units, sub_batches

    def forward(self, x, metadata):
        if x.dim() != 4:
            raise ValueError('%s takes (B, NB, 1, %d) inputs, got %s' % (type(self).__name__, self.seq_len, tuple(x.shape)))
        batches, sub_batches, n_features, seq_len = x.shape
        if seq_len != self.seq_len:
            raise ValueError('%s: the last dimension must be %d (linear_breath_inst is built for it), got %d'
                             % (type(self).__name__, self.seq_len, seq_len))
        if n_features != 1:
            raise ValueError('%s reads ONE channel (nn.LSTM(1, H)), got %d' % (type(self).__name__, n_features))
        if sub_batches != self.sub_batches:
            raise ValueError('%s was built for %d breaths per window, got %d' % (type(self).__name__, self.sub_batches, sub_batches))
        lstm = self.lstm_breath_block
        hs = S.WaveformLSTMFunction.apply(x.reshape(batches * sub_batches, seq_len), lstm.weight_ih_l0, lstm.weight_hh_l0,
                                          lstm.bias_ih_l0, lstm.bias_hh_l0, self.packed)
        # (NB, 224, H) flattened t-major per breath (outputs.view([batches, sub_batches, -1]), :42,:68)
        feat = S.BreathProjectionFunction.apply(hs.view(batches * sub_batches, seq_len * self.lstm_hidden_units),
                                                self.linear_breath_inst.weight, self.linear_breath_inst.bias)
        return F_.Linear2Function.apply(feat.view(batches, sub_batches * self.intermediate_features), self.linear_final.weight,
                                        self.linear_final.bias)


class LSTMOnlyNetwork(_WaveformLSTMNetwork):
    """One LSTM layer over the samples of every breath, then linear layers (models/lstm_only.py:46-69)."""
    seq_len = 224
    intermediate_features = 16


class LSTMOnlyWithPacking(_WaveformLSTMNetwork):
    """LSTMOnlyNetwork on padded breaths (models/lstm_only.py:7-43): a row runs up to and including its first exact zero
    (``pack_sequence``; a row that starts with a zero, or holds none, runs all 224 steps), the outputs behind it are zero
    (``pad_packed_sequence``).  The lengths are found on the device, inside the recurrence kernel."""
    seq_len = 224
    intermediate_features = 64
    packed = True
