"""The nested networks on MI355X: one item is a WHOLE PATIENT, all W windows of it as one sequence.

Operator surface of reference ``deepards/models/cnn_to_nested_layer.py`` (CNNToNestedRNNNetwork :8-44, CNNToNestedLSTMNetwork
:47-83): same constructors, children in the same registration order (``breath_block``, ``window_linear``, ``rnn`` / ``lstm``,
``linear_final``) and the ``is_cuda`` attribute, so ``state_dict`` keys and their order match and a reference ``state_dict``
loads with ``strict=True``.  ``forward(x, metadata)`` maps (1, W, NB, 1, 224) or (W, NB, 1, 224) to (1, W, 2): the breath block
on every window, the per-feature lower median over the NB breaths of a window, nn.RNN(128, 128) / nn.LSTM(128, 128) over the W
window vectors from a zero state, ``linear_final`` per window.

The reference loops over the W windows in Python; BatchNorm is window-grouped here, so it is ONE breath-block pass of B = W
windows (never several: the DenseNet dropout bumps its device-resident seed on every forward and the backward needs the
value).  The median is ``WindowMedianFunction``, the recurrence ``WideRNNFunction`` / ``WideLSTMFunction`` (csrc/seq_wide.hip).

``window_linear`` is what the reference constructs and never uses (its call is commented out, :40): a real parameter in the
``state_dict`` that never receives a gradient.

Refused, each with its reason: more than one patient per item (the reference raises), a breath block whose
``n_out_filters != 128`` (the recurrent input size is hard-wired: the reference's ``nn.RNN(128, ..)`` fails on anything else;
``densenet18`` is the one that fits), ``metadata`` other than None / NaN, CPU tensors, bf16 / f32x3p conv arithmetic and bf16
storage, and ``cnn_to_nested_transformer`` (:86-127), whose attention runs over T = W windows.
"""
import torch
import torch.nn as nn

from .. import functional as F_
from .backbone import Backbone
from .torch_cnn_linear_network import SEQ_LEN

INTERMEDIATE_UNITS = 128        # cnn_to_nested_layer.py:13,52
# The cap on W.  Read from the launch geometry of the densenet18 path: none of its kernels puts rows or windows into a 16-bit
# grid dimension (the 65535 limits of the library sit in the SE, VGG, ProtoPNet and autoencoder families), and every launch
# is checked, so no smaller cap exists there.  What remains is 32-bit element arithmetic: the largest activation of one pass
# is (W NB, 112, 64) = (W NB, 56, 128) -- 7 168 floats per breath row -- and a pass is refused once that tensor would reach
# 2^31 elements (W NB >= 299 593: W = 14 979 at NB = 20, far beyond the memory such a pass needs, about 7.6 MiB per window).
MAX_ROW_ELEMENTS = 7168


def check_windows(w, nb, who='this patient'):
    if w * nb * MAX_ROW_ELEMENTS >= 2 ** 31:
        raise ValueError('%s has W = %d windows of %d breaths: one breath-block pass over them holds an activation of %d x %d '
                         'elements, past the 2^31 the kernels index with 32 bits, and the pass is never chunked (the dropout '
                         "seed's hazard); the cap is W < %d"
                         % (who, w, nb, w * nb, MAX_ROW_ELEMENTS, -(-(2 ** 31) // (nb * MAX_ROW_ELEMENTS))))


TRANSFORMER_REFUSAL = ('cnn_to_nested_transformer is not built: attention over T = W windows needs a long-sequence kernel; the '
                       'block kernels stop at T = 64')


def nested_f32_only():
    if F_.conv_dtype() != 'f32' or F_.storage_dtype() != 'f32':
        raise NotImplementedError("the nested networks run with conv arithmetic 'f32' and float storage only (got %s / %s): the "
                                  'window median and the recurrence kernels read float features only'
                                  % (F_.conv_dtype(), F_.storage_dtype()))


class _NestedNetwork(nn.Module):
    """What the two classes share; ``_recurrent`` names the child that holds the recurrence's parameters."""
    _recurrent = None
    _function = None

    def _build(self, breath_block, window_sequence_size, is_cuda, recurrent):
        nn.Module.__init__(self)
        if not isinstance(breath_block, Backbone):
            raise TypeError('%s takes a Backbone of this package as its breath block, got %s'
                            % (type(self).__name__, type(breath_block).__name__))
        if breath_block.n_out_filters != INTERMEDIATE_UNITS:
            raise NotImplementedError(
                "%s: the recurrent input size is hard-wired to %d (the reference's nn.RNN(128, ..) fails on anything else), "
                'this breath block has n_out_filters = %d; densenet18 is the base network that fits'
                % (type(self).__name__, INTERMEDIATE_UNITS, breath_block.n_out_filters))
        self.breath_block = breath_block
        self.window_linear = nn.Linear(breath_block.n_out_filters * int(window_sequence_size), INTERMEDIATE_UNITS)
        setattr(self, self._recurrent, recurrent(INTERMEDIATE_UNITS, INTERMEDIATE_UNITS, batch_first=True))
        self.linear_final = nn.Linear(INTERMEDIATE_UNITS, 2)
        self.is_cuda = is_cuda
        self.seq_size = SEQ_LEN

    def _windows(self, x, metadata):
        """x -> (W, NB, C, L) of the one patient, after every refusal."""
        if x.dim() not in (4, 5):
            raise ValueError('expected (1, W, NB, 1, %d) or (W, NB, 1, %d) input, got %s' % (SEQ_LEN, SEQ_LEN, tuple(x.shape)))
        if x.dim() == 5:
            if x.shape[0] > 1:
                raise Exception('currently this network only supports patient batch sizes of 1')      # the reference's (:24-25)
            if x.shape[0] == 0:
                raise ValueError('an item is one patient, got an empty batch')
            x = x[0]
        if x.shape[0] == 0:
            raise ValueError('a patient needs at least one window')
        if x.shape[-1] != SEQ_LEN:
            raise Exception('input breaths must have sequence length of 224')
        if metadata is not None and not bool(torch.isnan(torch.as_tensor(metadata, dtype=torch.float32)).all()):
            raise NotImplementedError('%s takes no metadata (None or NaN): the reference ignores the argument'
                                      % type(self).__name__)
        nested_f32_only()
        check_windows(x.shape[0], x.shape[1])
        if not x.is_cuda:
            raise NotImplementedError('%s runs on the GPU only: there is no CPU path' % type(self).__name__)
        return x

    def forward(self, x, metadata):
        x = self._windows(x, metadata)
        w, nb, c, l = x.shape
        feat = self.breath_block.forward_windows(x.reshape(w * nb, c, l), nb)            # ONE pass over the W windows
        med = F_.WindowMedianFunction.apply(feat, nb)                                     # (W, 128)
        r = getattr(self, self._recurrent)
        hs = self._function.apply(med, r.weight_ih_l0, r.weight_hh_l0, r.bias_ih_l0, r.bias_hh_l0, 1)
        out = F_.Linear2Function.apply(hs.view(w, INTERMEDIATE_UNITS), self.linear_final.weight, self.linear_final.bias)
        return out.view(1, w, 2)


class CNNToNestedRNNNetwork(_NestedNetwork):
    _recurrent = 'rnn'
    _function = F_.WideRNNFunction

    def __init__(self, breath_block, window_sequence_size, is_cuda):
        self._build(breath_block, window_sequence_size, is_cuda, nn.RNN)


class CNNToNestedLSTMNetwork(_NestedNetwork):
    _recurrent = 'lstm'
    _function = F_.WideLSTMFunction

    def __init__(self, breath_block, window_sequence_size, is_cuda):
        self._build(breath_block, window_sequence_size, is_cuda, nn.LSTM)


class CNNToNestedTransformerNetwork(object):
    """Not built (its own kernel first): constructing it says why."""

    def __init__(self, *args, **kwargs):
        raise NotImplementedError(TRANSFORMER_REFUSAL)
