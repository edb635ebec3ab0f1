"""1-D VGG-11 / VGG-13 (with BatchNorm) breath blocks on MI355X.

Operator surface of reference ``deepards/models/vgg.py`` (VGG :10-34, make_layers :37-50, cfgs :53-58, vgg11_bn :78-85,
vgg13_bn :98-105), written here in this package's own terms: the same module tree -- ``features`` is a Sequential of Conv1d (WITH bias) / BatchNorm1d / ReLU /
MaxPool1d(2, 2), ``avgpool`` an AdaptiveAvgPool1d(7) -- so ``state_dict`` keys and their order match, the same
``n_out_filters`` (3584) and initialisation.  ``network_name`` ('vgg11' / 'vgg13') is an extra attribute the driver and the
checkpoint code need; the reference's class has none.  As in ``resnet.py`` the torch.nn leaf modules are only parameter
containers: ``forward`` runs the HIP kernels through ``deepards_amd.functional`` on a whole batch of windows.

Built: cfgs A and B with BatchNorm (``vgg11_bn`` / ``vgg13_bn``, the reference's ``base_networks['vgg11' | 'vgg13']``).  The
nets without BatchNorm and cfgs D / E are refused.
"""
import math

import torch.nn as nn

from .. import functional as F_
from .backbone import Backbone, HEAD_FLAT

# (channels, pooled) of every stage, by the reference's configuration letter (vgg.py:53-55): A = vgg11, B = vgg13
STAGES = {
    'A': ((64, True), (128, True), (256, False), (256, True), (512, False), (512, True), (512, False), (512, True)),
    'B': ((64, False), (64, True), (128, False), (128, True), (256, False), (256, True), (512, False), (512, True), (512, False),
          (512, True)),
}
# Stages whose conv has 512 channels on both sides keep off the F(4,3) Winograd kernels, as the SE blocks do (hip_ops._wino,
# DESIGN_APPENDIX.md "vgg11")
PRECISE_MIN_C = 512


def _as_stages(cfg):
    """A stage table, or the reference's flat list of channel counts and 'M' marks -> ((channels, pooled), ...)."""
    cfg = list(cfg)
    if all(isinstance(v, tuple) for v in cfg):
        return tuple(cfg)
    if not cfg or cfg[0] == 'M' or any(a == 'M' and b == 'M' for a, b in zip(cfg, cfg[1:])):
        raise NotImplementedError('a pool must follow a conv stage')
    return tuple((v, nxt == 'M') for v, nxt in zip(cfg, cfg[1:] + [None]) if v != 'M')


def make_layers(cfg, batch_norm=False):
    """The ``features`` Sequential of vgg.py:37-50: per stage Conv1d(k3, p1, with bias), BatchNorm1d, ReLU and, behind a
    pooled stage, MaxPool1d(2, 2) -- in that order, which is the state_dict's numbering.  The first conv reads one channel."""
    if not batch_norm:
        raise NotImplementedError('the VGG nets without BatchNorm (vgg11 / vgg13) are not on the accelerated path')
    mods, cin = [], 1
    for c, pooled in _as_stages(cfg):
        conv = nn.Conv1d(cin, c, 3, stride=1, padding=1, bias=True)
        conv.precise_conv = min(cin, c) >= PRECISE_MIN_C           # (functional.training_step packs its weight for F(2,3))
        mods.extend((conv, nn.BatchNorm1d(c), nn.ReLU(inplace=True)))
        if pooled:
            mods.append(nn.MaxPool1d(2, 2))
        cin = c
    return nn.Sequential(*mods)


def init_like_reference(net):
    """The reference's initialisation (vgg.py:26-34): conv weights N(0, sqrt(2 / (k * C_out))) (kaiming normal, fan_out, relu),
    conv biases 0, BatchNorm weight 1 and bias 0."""
    for m in net.modules():
        if isinstance(m, nn.Conv1d):
            m.weight.data.normal_(0.0, math.sqrt(2.0 / (m.kernel_size[0] * m.out_channels)))
            m.bias.data.zero_()
        elif isinstance(m, nn.BatchNorm1d):
            m.weight.data.fill_(1.0)
            m.bias.data.zero_()


class VGG(Backbone):
    """``features`` -> ``avgpool`` (AdaptiveAvgPool1d(7)) -> view(N, -1) (vgg.py:20-24): (N, 1, L) -> (N, 3584), feature
    c * 7 + i.  ``features``: what make_layers builds."""

    f32_only = ('VGG nets', 'the pooled stages have no bf16 / f32x3p forms')
    POOLED_LEN = 7

    def __init__(self, features, init_weights=True):
        nn.Module.__init__(self)
        self.features, self.avgpool = features, nn.AdaptiveAvgPool1d(self.POOLED_LEN)      # (registered in the reference's order)
        self.n_out_filters = self.stages()[-1][0].out_channels * self.POOLED_LEN
        if init_weights:
            init_like_reference(self)

    def stages(self):
        """[(conv, bn, pooled)] read off ``features``: every Conv1d is followed by BatchNorm1d and ReLU, then maybe a pool."""
        mods, out, i = list(self.features), [], 0
        while i < len(mods):
            conv, bn, relu = mods[i:i + 3] if i + 3 <= len(mods) else (None, None, None)
            if not (isinstance(conv, nn.Conv1d) and isinstance(bn, nn.BatchNorm1d) and isinstance(relu, nn.ReLU)) or \
                    (conv.kernel_size, conv.stride, conv.padding) != ((3,), (1,), (1,)) or conv.bias is None:
                raise NotImplementedError('features must be Conv1d(k3, p1, bias) / BatchNorm1d / ReLU triples and MaxPool1d(2, 2)')
            i += 3
            pooled = i < len(mods) and isinstance(mods[i], nn.MaxPool1d)
            if pooled:
                if (mods[i].kernel_size, mods[i].stride, mods[i].padding, mods[i].ceil_mode) != (2, 2, 0, False):
                    raise NotImplementedError('only MaxPool1d(2, 2) is on the accelerated path')
                i += 1
            out.append((conv, bn, pooled))
        return out

    def _map(self, x, rows_per_window):
        """The last stage's map (rows, L / 32, 512) channels-last."""
        rows, _, l = x.shape
        h = x.contiguous().float().view(rows, l)
        for k, (conv, bn, pooled) in enumerate(self.stages()):
            if pooled and h.shape[1] < 2:
                raise ValueError('MaxPool1d(2, 2) needs a length >= 2 (seq_len >= 32); got %d' % h.shape[1])
            h = F_.VGGStageFunction.apply(h, conv.weight, conv.bias, bn.weight, bn.bias, rows_per_window, F_.BNState(bn), pooled,
                                          k == 0, bool(getattr(conv, 'precise_conv', False)))
        return h

    def head_operand_kind(self, seq_len):
        return HEAD_FLAT

    def head_operand(self, x, rows_per_window):
        return self.forward_windows(x, rows_per_window)

    def forward_windows(self, x, rows_per_window, pooled=True):
        """x: (rows, 1, L) with rows = windows * rows_per_window; BatchNorm statistics are taken per window, exactly as when
        the reference feeds one (NB, 1, L) window at a time.  -> (rows, 3584) features (a fused head's flat form takes them as
        they are); there is no un-pooled map to hand out (pooled=False: TypeError)."""
        if not pooled:
            raise TypeError('VGG has no un-pooled map: its features are the flattened AdaptiveAvgPool1d(7) output')
        self.check_input(x, rows_per_window)
        return F_.AdaptiveAvgPoolFlatFunction.apply(self._map(x, rows_per_window), self.avgpool.output_size)


def _vgg(name, cfg):
    model = VGG(make_layers(STAGES[cfg], batch_norm=True))
    model.network_name = name
    return model


def vgg11_bn():
    return _vgg('vgg11', 'A')


def vgg13_bn():
    return _vgg('vgg13', 'B')
