"""The siamese pretraining networks on MI355X.

Operator surface of reference ``deepards/models/siamese.py`` (Identity :8-13, SiameseCNNLinearNetwork :56-83,
SiameseCNNTransformerNetwork :86-116, SiameseCNNLSTMNetwork :119-157): same constructors, children in the same registration
order, ``seq_size`` / ``time_layer_hidden_units`` / ``lstm_layers`` attributes, ``state_dict`` keys and the same exception for a
wrong sequence length.  ``forward(x, compr)`` compares two windows: both go through the breath block (and the LSTM / Transformer
behind it), ``linear_intermediate`` maps |compr - x| to two numbers per breath and ``linear_final`` the 2 NB numbers of a window
to two logits.

Where the reference runs the breath block once per window and once per tower, all windows of both towers go through it in ONE
batched pass here (BatchNorm statistics still per window, the running statistics updated window by window in the reference's
order: x's windows, then compr's), and the LSTM / Transformer runs once on the concatenation -- both treat windows independently.

``forward_triplet`` is the training path: the windows of a whole triplet batch -- [anchor | pos | anchor | neg] (``literal``: the
reference's two calls ``model(seq, pos)``, ``model(seq, neg)``, four tower passes) or [anchor | pos | neg] (the anchor once) --
in one tower pass, then head, both BCE terms and their gradients in the fused head kernels (siamese_ops.SiameseHeadFunction).
In the literal form BatchNorm's running statistics take one update per call the pass stands for (windows [0, 2 B), then
[2 B, 4 B)), so they end with the bits ``model(seq, pos)``, ``model(seq, neg)`` leave.

``SiameseARDSClassifier`` (:16-53) is not built: its only caller (train_ards_detector.py:1153) omits ``sub_batch_size``, so the
reference cannot construct it.  ``network_map`` of the driver keeps its six entries; these classes are reached through
``python -m deepards_amd.siamese``.
"""
import torch
import torch.nn as nn

from .. import functional as F_
from .. import hip_ops as H
from .. import siamese_ops as SO
from .torch_cnn_linear_network import SEQ_LEN
from .transformer import Transformer, NUM_HEADS


class Identity(nn.Module):
    def __init__(self):
        super(Identity, self).__init__()

    def forward(self, x):
        return x


class _SiameseNetwork(nn.Module):
    """What the three networks share: the batched tower pass, the two-Linear head behind the abs-diff, the triplet path.  A
    subclass registers its children (the order is the contract) and gives ``_time_layer``."""

    def _time_layer(self, feat, n_windows, nb):
        """(n_windows * nb, F) breath features -> (n_windows * nb, D) rows the head compares."""
        return feat

    def _towers(self, windows, calls=1):
        """windows (W, NB, C, 224) -> (W * NB, D): every window through the breath block (one pass) and the time layer.
        ``calls``: the pass stands for this many consecutive ``forward`` calls of equal size -- BatchNorm's running statistics
        take one update per call (functional.running_update_groups), the bits separate calls would leave."""
        if windows.shape[-1] != SEQ_LEN:
            raise Exception('input breaths must have sequence length of 224')             # the reference's message (:76-77)
        if windows.dim() != 4 or windows.shape[0] == 0:
            raise ValueError('expected (windows >= 1, NB, C, 224) input, got %s' % (tuple(windows.shape),))
        w, nb, c, l = windows.shape
        if 2 * nb != self.linear_final.in_features:
            raise ValueError('windows of %d breaths do not fit linear_final (sub_batch_size %d)' %
                             (nb, self.linear_final.in_features // 2))
        with F_.running_update_groups(calls):
            feat = self.breath_block.forward_windows(windows.reshape(w * nb, c, l), nb)
        return self._time_layer(feat, w, nb)

    def forward(self, x, compr):
        # (B, NB, C, 224) each -> (B, 2)
        if x.shape[-1] != SEQ_LEN or compr.shape[-1] != SEQ_LEN:
            raise Exception('input breaths must have sequence length of 224')
        if x.shape != compr.shape:
            raise ValueError('x and compr must have one shape, got %s and %s' % (tuple(x.shape), tuple(compr.shape)))
        b, nb = x.shape[0], x.shape[1]
        rows = self._towers(torch.cat([x, compr], dim=0))                               # x's windows first: the reference's order
        li, lf = self.linear_intermediate, self.linear_final
        if not torch.is_grad_enabled():                                                 # the fused head on the one pair, twice
            _, z, _ = SO.siamese_head_fwd(rows[:b * nb], rows[b * nb:], rows[:b * nb], rows[b * nb:], li.weight, li.bias,
                                          lf.weight, lf.bias, b, nb)
            return z[0]
        diff = torch.abs(rows[b * nb:] - rows[:b * nb])
        inter = F_.Linear2Function.apply(diff, li.weight, li.bias)
        return F_.Linear2Function.apply(inter.view(b, 2 * nb), lf.weight, lf.bias)

    def forward_triplet(self, batch, literal=True):
        """batch ((4 or 3) B, NB, C, 224): [anchor | pos | anchor | neg] (``literal``) or [anchor | pos | neg] windows, as
        ``SiameseTileStore.triplet_batch`` gathers them -> (loss (1,), z_pos (B, 2), z_neg (B, 2)); loss = BCE(z_pos, [0, 1]) +
        BCE(z_neg, [1, 0]), the two terms of the reference's training loop."""
        loss, z = self.triplet_head(batch, literal)
        return loss, z[0], z[1]

    def triplet_head(self, batch, literal=True):
        """``forward_triplet`` with the logits as the head kernel leaves them: (loss (1,), z (2, B, 2)), z[0] the positive
        pair's."""
        k = 4 if literal else 3
        if batch.dim() != 4 or batch.shape[0] % k or batch.shape[0] == 0:
            raise ValueError('forward_triplet: expected (%d B, NB, C, 224) windows, got %s' % (k, tuple(batch.shape)))
        b, nb = batch.shape[0] // k, batch.shape[1]
        rows = self._towers(batch, calls=2 if literal else 1)           # literal: model(seq, pos) then model(seq, neg)
        li, lf = self.linear_intermediate, self.linear_final
        return SO.SiameseHeadFunction.apply(rows, li.weight, li.bias, lf.weight, lf.bias, b, nb, bool(literal))


class SiameseCNNLinearNetwork(_SiameseNetwork):
    def __init__(self, breath_block, sub_batch_size):
        super(SiameseCNNLinearNetwork, self).__init__()
        self.seq_size = SEQ_LEN
        self.breath_block = breath_block
        self.linear_intermediate = nn.Linear(breath_block.n_out_filters, 2)
        self.linear_final = nn.Linear(2 * sub_batch_size, 2)


class SiameseCNNTransformerNetwork(_SiameseNetwork):
    def __init__(self, breath_block, hidden_units, sub_batch_size):
        super(SiameseCNNTransformerNetwork, self).__init__()
        d = breath_block.n_out_filters
        try:
            H.tfm_check_shape(1, d, hidden_units, 'SiameseCNNTransformerNetwork')
        except ValueError as e:
            raise NotImplementedError(str(e))
        self.seq_size = SEQ_LEN
        self.breath_block = breath_block
        self.time_layer_hidden_units = hidden_units
        self.transformer = Transformer(d, hidden_units, 2, NUM_HEADS)                   # two blocks, four heads (:92-94)
        self.linear_intermediate = nn.Linear(d, 2)
        self.linear_final = nn.Linear(2 * sub_batch_size, 2)

    def _time_layer(self, feat, n_windows, nb):
        H.tfm_check_shape(nb, feat.shape[1], self.time_layer_hidden_units, 'SiameseCNNTransformerNetwork')
        return self.transformer(feat.view(n_windows, nb, feat.shape[1])).reshape(n_windows * nb, -1)


class SiameseCNNLSTMNetwork(_SiameseNetwork):
    def __init__(self, breath_block, hidden_units, sub_batch_size):
        super(SiameseCNNLSTMNetwork, self).__init__()
        if hidden_units % 8 or not 8 <= hidden_units <= 64:
            raise NotImplementedError('hidden_units must be a multiple of 8 in [8, 64] (the LSTM kernels, as for CNNLSTMNetwork)')
        self.seq_size = SEQ_LEN
        self.breath_block = breath_block
        self.time_layer_hidden_units = hidden_units
        self.lstm_layers = 1
        self.lstm = nn.LSTM(breath_block.n_out_filters, hidden_units, num_layers=self.lstm_layers, batch_first=True)
        self.linear_intermediate = nn.Linear(hidden_units, 2)
        self.linear_final = nn.Linear(2 * sub_batch_size, 2)

    def _time_layer(self, feat, n_windows, nb):
        lstm = self.lstm
        hs, _, _ = F_.LSTMFunction.apply(feat, lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0, nb, None,
                                         None)
        return hs.reshape(n_windows * nb, -1)
