"""The breath-metadata regressor on MI355X.

Operator surface of reference ``deepards/models/torch_cnn_bm_regressor.py`` (CNNRegressor :6-19): same constructor, children in
the same registration order (``breath_block``, ``linear_final``), the ``seq_size`` attribute, ``state_dict`` keys and the same
exception for a wrong sequence length.  ``forward(x, metadata)`` maps single breaths (B, C_in, 224) to (B, M) regressed breath
metadata; ``metadata`` is ignored, as in the reference.

The reference calls ``self.breath_block(x)`` once on the whole batch, so BatchNorm takes its statistics over all B rows: ONE
window of B rows here (``rows_per_window = B``).  The head -- AvgPool1d(7) of the last map, ``linear_final`` and, in
``forward_loss``, ``MSELoss`` with its gradient -- is the fused kernel pair of ``regress_ops`` on the un-pooled map (or on the flat
features a VGG hands over); the pooled map is never stored.

Departure: the reference's ``.squeeze()`` turns a batch of one breath into an (M,) output; here the output is (B, M) for every
B >= 1.
"""
import torch
import torch.nn as nn

from .. import functional as F_
from .. import regress_ops as RO
from .backbone import Backbone
from .torch_cnn_linear_network import SEQ_LEN


def regressor_f32_only():
    if F_.conv_dtype() != 'f32' or F_.storage_dtype() != 'f32':
        raise NotImplementedError("CNNRegressor runs with conv arithmetic 'f32' and float storage only (got %s / %s): the regression "
                                  'head reads float maps only' % (F_.conv_dtype(), F_.storage_dtype()))


class CNNRegressor(nn.Module):
    def __init__(self, breath_block, n_final_features):
        super(CNNRegressor, self).__init__()
        if not isinstance(breath_block, Backbone):
            raise TypeError('CNNRegressor takes a Backbone of this package (ResNet, DenseNet, SENet, VGG) as its breath block, got '
                            '%s: a UNet / AutoencoderCNN has no pooled feature vector to regress from' % type(breath_block).__name__)
        if not 1 <= int(n_final_features) <= RO.MAX_OUTPUTS:
            raise ValueError('n_final_features must be in [1, %d] (the regression head keeps one accumulator per output in '
                             'registers), got %r' % (RO.MAX_OUTPUTS, n_final_features))
        self.seq_size = SEQ_LEN
        self.breath_block = breath_block
        self.linear_final = nn.Linear(breath_block.n_out_filters, int(n_final_features))

    def _operand(self, x):
        """x (B, C_in, 224) -> what the fused head pools: the last map (B, 7, C), or features (B, F); all B rows ONE window."""
        if x.shape[-1] != SEQ_LEN:
            raise Exception('input breaths must have sequence length of 224')             # the reference's message (:16-17)
        if x.dim() != 3 or x.shape[0] == 0:
            raise ValueError('expected (breaths >= 1, C_in, 224) input, got %s' % (tuple(x.shape),))
        regressor_f32_only()
        bb = self.breath_block
        if bb.head_operand_kind(SEQ_LEN) is None:
            raise NotImplementedError('%s hands no operand to a fused head at length %d' % (type(bb).__name__, SEQ_LEN))
        return bb.head_operand(x, x.shape[0])

    def forward(self, x, metadata=None):
        op = self._operand(x)
        return RO.RegressLinearFunction.apply(op, self.linear_final.weight, self.linear_final.bias, torch.is_grad_enabled())

    def forward_loss(self, x, target):
        """(loss (1,), out (B, M)) of MSELoss()(self(x, None), target): pool, linear_final, the loss and -- on ``loss.backward()``
        -- all their gradients as ONE autograd node in two launches each way (regress_ops.RegressHeadFunction)."""
        op = self._operand(x)
        lf = self.linear_final
        if target.dim() != 2 or tuple(target.shape) != (x.shape[0], lf.out_features):
            raise ValueError('target must be (%d, %d), got %s' % (x.shape[0], lf.out_features, tuple(target.shape)))
        return RO.regress_head_loss(op, lf.weight, lf.bias, target)
