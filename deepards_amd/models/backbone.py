"""What a breath-block backbone is to a head, the trainer, the driver and the checkpoint loader: the input check, ``forward``,
the operand a fused head may ask for (known from the shapes, before anything is launched) and the class data that decisions
about a backbone are read from.  ``ResNet``, ``DenseNet``, ``SENet`` and ``VGG`` derive from ``Backbone``; it has no parameters,
buffers or children, so their ``state_dict`` keys are their own.
"""
import torch.nn as nn

from .. import functional as F_

POOL_LEN = 7                          # AvgPool1d(7, stride=1) on the last map: the one length the fused head pools
HEAD_MAP, HEAD_FLAT = 'map', 'flat'   # Backbone.head_operand_kind: the (rows, 7, C) map | (rows, F) features the head takes as they are


def check_windows(what, x, rows_per_window, in_channels):
    """x must be (rows, in_channels, L) on the GPU with rows = windows * rows_per_window."""
    if not x.is_cuda:
        raise RuntimeError('%s: the deepards_amd models run on MI355X only (input is on %s); there is no '
                           'CPU fallback' % (what, x.device))
    if x.dim() != 3 or x.shape[1] != in_channels:
        raise ValueError('expected (rows, %d, L) input, got %s' % (in_channels, tuple(x.shape)))
    if x.shape[0] % rows_per_window:
        raise ValueError('rows not a multiple of rows_per_window')


class Backbone(nn.Module):
    """A subclass gives ``_map(x, rows_per_window)`` -- checked (rows, C_in, L) input -> the last map (rows, L', C) channels-last
    -- and ``final_length(l)``, that map's L' for an input length l."""

    in_channels = 1            # channels of the input rows
    f32_only = None            # kernels for every conv arithmetic / storage; else (family, why): conv arithmetic 'f32' and float storage only
    running_stats = True       # BatchNorm keeps running statistics (eval() would mean inference on them, which is not built)
    bf16_storage = False       # bf16 kernels throughout: conv dtype 'bf16' runs with bf16 storage too

    def check_input(self, x, rows_per_window):
        if self.f32_only is not None and (F_.conv_dtype() != 'f32' or F_.storage_dtype() != 'f32'):
            raise NotImplementedError("the %s run with conv arithmetic 'f32' and float storage only (got %s / %s): %s"
                                      % (self.f32_only[0], F_.conv_dtype(), F_.storage_dtype(), self.f32_only[1]))
        check_windows(type(self).__name__, x, rows_per_window, self.in_channels)

    def head_operand_kind(self, seq_len):
        """What ``head_operand`` hands a fused head for rows of ``seq_len`` samples: HEAD_MAP, HEAD_FLAT, or None (nothing: the
        head then takes ``forward_windows`` and its own kernels)."""
        return HEAD_MAP if self.final_length(seq_len) == POOL_LEN else None

    def head_operand(self, x, rows_per_window):
        return self.forward_windows(x, rows_per_window, pooled=False)

    def forward_windows(self, x, rows_per_window, pooled=True):
        """x: (rows, C_in, L) with rows = windows * rows_per_window; BatchNorm statistics are taken per window, exactly as when
        the reference feeds one (NB, C_in, L) window at a time.  -> the pooled features (rows, C); pooled=False: the last map
        (rows, 7, C) itself, for a head that pools it in its own kernel (TypeError where there is no such map)."""
        self._check(x, rows_per_window, want_map=not pooled)
        h = self._map(x, rows_per_window)
        return F_.GlobalAvgPoolFunction.apply(h) if pooled else h

    def _check(self, x, rows_per_window, want_map):
        """The input check and what the last map's length allows, before anything is launched."""
        self.check_input(x, rows_per_window)
        l = self.final_length(x.shape[2])
        if l < POOL_LEN:
            raise ValueError('AvgPool1d(7, stride=1) needs a final length >= 7 (seq_len >= 224); got %d' % l)
        if want_map and l != POOL_LEN:
            raise TypeError('the un-pooled map is only handed out at the 7-position length the fused head pools')

    def forward(self, x):
        # one call == one BatchNorm batch, like the reference's breath_block(x[i])
        return self.forward_windows(x, x.shape[0])
