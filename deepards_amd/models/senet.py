"""1-D SE-ResNet / SE-ResNeXt breath blocks (se_resnet18 / 50 / 101 / 152, se_resnext50_32x4d / 101_32x4d) on MI355X.

Operator surface of reference ``deepards/models/senet.py`` (SEModule :15-34, SEBasicBlock :37-68, Bottleneck :71-95,
SEResNetBottleneck :122-144, SEResNeXtBottleneck :147-168, SENet :171-328, se_resnet18 :343-348, se_resnet50 / 101 / 152
:351-372, se_resnext50_32x4d / se_resnext101_32x4d :375-388): same constructor arguments, sub-module / parameter names and their order (so ``state_dict`` keys
match), ``n_out_filters`` and ``network_name``.  As in ``resnet.py`` the torch.nn leaf modules are only parameter containers:
``forward`` runs the HIP kernels through ``deepards_amd.functional`` on a whole batch of windows.

Built: the BasicBlock and the SE-ResNet Bottleneck variants on the k7 stem (``se_resnet18``, ``se_resnet50`` / ``101`` /
``152`` and other ``layers`` lists), and the ResNeXt 32x4d bottleneck on the same stem (``se_resnext50_32x4d`` /
``se_resnext101_32x4d``: 32 groups, base width 4; its grouped conv2 runs on ``H.gconv3_*``; the block class and the two
factories live in ``models/seresnext.py``).  The 3x3-stem nets (``senet18``,
``senet154``), the SENet-154 bottleneck (``SEBottleneck``, 64 groups) and every other group count are refused in the constructor.  Initialisation is
torch's defaults: the reference's SENet has no init loop.
"""
from collections import OrderedDict

import torch.nn as nn

from .. import functional as F_
from .backbone import Backbone


class SEModule(nn.Module):
    """Parameter container of the gate sigmoid(fc2(relu(fc1(avg_pool(x))))) (senet.py:17-25); fc1 / fc2 are k1 convs WITH bias."""

    def __init__(self, channels, reduction):
        super(SEModule, self).__init__()
        self.avg_pool = nn.AdaptiveAvgPool1d(1)
        self.fc1 = nn.Conv1d(channels, channels // reduction, kernel_size=1, padding=0)
        self.relu = nn.ReLU(inplace=True)
        self.fc2 = nn.Conv1d(channels // reduction, channels, kernel_size=1, padding=0)
        self.sigmoid = nn.Sigmoid()


def _se_block(blk, x, R, units, family, own=False):
    """F_.SEBlockFunction on block ``blk``: ``units`` = its (conv, BatchNorm, precise) in order, ``family`` its gate kernels'.
    own: every unit carries its conv's own stride and group count (the ResNeXt form) instead of the block's stride on the first."""
    ds, se = blk.downsample, blk.se_module
    params = [t for conv, bn, _ in units for t in (conv.weight, bn.weight, bn.bias)]
    params += [se.fc1.weight, se.fc1.bias, se.fc2.weight, se.fc2.bias]
    if ds is not None:
        params += [ds[0].weight, ds[1].weight, ds[1].bias]
    return F_.SEBlockFunction.apply(x, blk.stride, R, family,
                                    [(conv.kernel_size[0], precise, F_.BNState(bn)) + ((conv.stride[0], conv.groups) if own else ())
                                     for conv, bn, precise in units],
                                    None if ds is None else F_.BNState(ds[1]), *params)


class SEBasicBlock(nn.Module):
    """Parameter container of one SE residual block; child names and their order are the state_dict contract
    (conv1, bn1, relu, conv2, se_module, bn2, downsample -- senet.py:43-49)."""
    expansion = 1
    precise_convs = True      # functional.training_step: the block's convs are packed for F(2,3) at every width (H._wino)

    def __init__(self, inplanes, planes, groups, reduction, stride=1, downsample=None):
        super(SEBasicBlock, self).__init__()
        if groups != 1:
            raise NotImplementedError('grouped convolutions (senet18 / senet154, the ResNeXt nets) are not on the accelerated path')
        cr = planes // reduction if reduction >= 1 else 0
        if planes % 64 or planes > 512 or planes & (planes - 1) or cr < 16 or cr % 16 or 256 % cr or planes * cr < 1024:
            raise NotImplementedError('the SE gate kernels take 64 / 128 / 256 / 512 planes with a hidden width that is a '
                                      'multiple of 16 dividing 256 (reduction 4 on the four stages)')
        self.conv1 = nn.Conv1d(inplanes, planes, kernel_size=3, stride=stride, padding=1, bias=False)
        self.bn1 = nn.BatchNorm1d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv1d(planes, planes, kernel_size=3, stride=1, padding=1, bias=False)
        self.se_module = SEModule(planes, reduction=reduction)
        self.bn2 = nn.BatchNorm1d(planes)
        self.downsample = downsample
        self.stride = stride

    def forward_rlc(self, x, R):
        """x: (rows, L, C) channels-last; R rows per BatchNorm window.  The gate stays on the narrow kernels at every width."""
        return _se_block(self, x, R, ((self.conv1, self.bn1, True), (self.conv2, self.bn2, True)), F_.H.SE_NARROW)


class SEResNetBottleneck(nn.Module):
    """Parameter container of one SE-ResNet bottleneck block: conv1 (k1, carries the stride) -> conv2 (k3) -> conv3 (k1, to
    4 planes channels) with the gate on the wide map; child names and their order are the state_dict contract (conv1, bn1,
    conv2, bn2, conv3, bn3, relu, se_module, downsample -- senet.py:132-144)."""
    expansion = 4
    precise_convs = True      # functional.training_step: conv2 is packed for F(2,3) at every width (H._wino)

    def __init__(self, inplanes, planes, groups, reduction, stride=1, downsample=None):
        super(SEResNetBottleneck, self).__init__()
        if groups != 1:
            raise NotImplementedError('grouped convolutions (senet18 / senet154, the ResNeXt nets) are not on the accelerated path')
        c = planes * 4
        cr = c // reduction if reduction >= 1 else 0
        if planes % 32 or inplanes % 32 or not F_.H.se_wide_ok(c, cr) or cr * reduction != c:
            raise NotImplementedError('the SE bottleneck takes planes and inplanes that are multiples of 32 and a gate on 4 planes <= '
                                      '2048 channels whose hidden width is a multiple of 16 up to 128 (reduction 16 on the four stages)')
        self.conv1 = nn.Conv1d(inplanes, planes, kernel_size=1, bias=False, stride=stride)
        self.bn1 = nn.BatchNorm1d(planes)
        self.conv2 = nn.Conv1d(planes, planes, kernel_size=3, padding=1, groups=groups, bias=False)
        self.bn2 = nn.BatchNorm1d(planes)
        self.conv3 = nn.Conv1d(planes, planes * 4, kernel_size=1, bias=False)
        self.bn3 = nn.BatchNorm1d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.se_module = SEModule(planes * 4, reduction=reduction)
        self.downsample = downsample
        self.stride = stride

    def forward_rlc(self, x, R):
        """x: (rows, L, C) channels-last; R rows per BatchNorm window."""
        fc1 = self.se_module.fc1
        return _se_block(self, x, R, ((self.conv1, self.bn1, False), (self.conv2, self.bn2, True), (self.conv3, self.bn3, False)),
                         F_.H.se_gate_family(fc1.in_channels, fc1.out_channels))


class SENet(Backbone):
    """Four stages of SEBasicBlocks, SEResNetBottlenecks or SEResNeXtBottlenecks behind layer0 = conv k7 s2 -> BN -> ReLU -> MaxPool1d(3, 2, ceil_mode=True).  The module
    tree (names, order, shapes) is the reference's (senet.py:219-289)."""

    f32_only = ('SE-ResNets', 'the SE tail has no bf16 / f32x3p forms')

    def __init__(self, block, layers, groups, reduction, dropout_p=0.2, inplanes=128, input_3x3=True, downsample_kernel_size=3,
                 downsample_padding=1):
        super(SENet, self).__init__()
        from .seresnext import SEResNeXtBottleneck      # (imported here: that module builds on this one)
        if block not in (SEBasicBlock, SEResNetBottleneck, SEResNeXtBottleneck):
            raise NotImplementedError('only SEBasicBlock (se_resnet18 style), SEResNetBottleneck (se_resnet50 style) and '
                                      'SEResNeXtBottleneck (se_resnext50_32x4d style) are on the accelerated path')
        if block is SEResNeXtBottleneck:
            if groups != 32:
                raise NotImplementedError('SEResNeXtBottleneck runs with groups = 32 (the 32x4d nets), got groups = %r' % (groups,))
        elif groups != 1:
            raise NotImplementedError('grouped convolutions (senet18 / senet154, the ResNeXt nets) are not on the accelerated path')
        if input_3x3:
            raise NotImplementedError('the three-conv 3x3 stem (senet18 / senet154) is not on the accelerated path')
        if dropout_p is not None:
            raise NotImplementedError('dropout behind the pooled features (senet18 / senet154) is not on the accelerated path')
        if (downsample_kernel_size, downsample_padding) != (1, 0):
            raise NotImplementedError('downsample convolutions other than k1 p0 (senet154) are not on the accelerated path')
        if inplanes != 64:
            raise NotImplementedError('inplanes must be 64 (the SE-ResNets and SE-ResNeXts) on the accelerated path')
        self.inplanes = inplanes
        self.layer0 = nn.Sequential(OrderedDict([
            ('conv1', nn.Conv1d(1, inplanes, kernel_size=7, stride=2, padding=3, bias=False)),
            ('bn1', nn.BatchNorm1d(inplanes)),
            ('relu1', nn.ReLU(inplace=True)),
            # (ceil_mode instead of padding=1, senet.py:243-246: windows {2j, 2j+1, 2j+2} clipped at the end)
            ('pool', nn.MaxPool1d(3, stride=2, ceil_mode=True))]))
        for i, n_blocks in enumerate(layers):
            self.add_module('layer%d' % (i + 1), self._make_layer(block, 64 << i, n_blocks, groups, reduction, 1 if i == 0 else 2))
        self.avg_pool = nn.AvgPool1d(7, stride=1)
        self.dropout = None
        self.n_out_filters = 512 * block.expansion

    def _make_layer(self, block, planes, blocks, groups, reduction, stride=1):
        downsample = None
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(nn.Conv1d(self.inplanes, planes * block.expansion, kernel_size=1, stride=stride, padding=0,
                                                 bias=False),
                                       nn.BatchNorm1d(planes * block.expansion))
        stage = [block(self.inplanes, planes, groups, reduction, stride, downsample)]
        self.inplanes = planes * block.expansion
        stage += [block(self.inplanes, planes, groups, reduction) for _ in range(1, blocks)]
        return nn.Sequential(*stage)

    def final_length(self, l):
        cur = F_.H.pool_out_len(l // 2, F_.POOL_MAX_CEIL)          # layer0: conv s2, then the ceil-mode pool
        for layer in (self.layer1, self.layer2, self.layer3, self.layer4):
            cur = (cur - 1) // layer[0].stride + 1
        return cur

    def _map(self, x, rows_per_window):
        """The last block's map (rows, L / 32, 512 * block.expansion) channels-last."""
        rows, _, l = x.shape
        l0 = self.layer0
        h = F_.StemFunction.apply(x.contiguous().float().view(rows, l), l0.conv1.weight, l0.bn1.weight, l0.bn1.bias,
                                  rows_per_window, F_.POOL_MAX_CEIL, F_.BNState(l0.bn1), False)
        for layer in (self.layer1, self.layer2, self.layer3, self.layer4):
            for blk in layer:
                h = blk.forward_rlc(h, rows_per_window)
        return h

    def features(self, x):
        """layer0 .. layer4 of one BatchNorm batch: the last map in the reference's (N, C, L) layout (senet.py:311-317)."""
        self.check_input(x, x.shape[0])
        return self._map(x, x.shape[0]).permute(0, 2, 1)

    def logits(self, x):
        """AvgPool1d(7, stride=1) of an (N, C, L) map (senet.py:319-323; there is no dropout on this path)."""
        n, c, _ = x.shape
        return F_.GlobalAvgPoolFunction.apply(x.permute(0, 2, 1).contiguous()).view(n, c, -1)


def se_resnet18():
    model = SENet(SEBasicBlock, [2, 2, 2, 2], groups=1, reduction=4, dropout_p=None, inplanes=64, input_3x3=False,
                  downsample_kernel_size=1, downsample_padding=0)
    model.network_name = 'se_resnet18'
    return model


def _se_resnet_bottleneck(name, layers):
    model = SENet(SEResNetBottleneck, layers, groups=1, reduction=16, dropout_p=None, inplanes=64, input_3x3=False,
                  downsample_kernel_size=1, downsample_padding=0)
    model.network_name = name
    return model


def se_resnet50():
    return _se_resnet_bottleneck('se_resnet50', [3, 4, 6, 3])


def se_resnet101():
    return _se_resnet_bottleneck('se_resnet101', [3, 4, 23, 3])


def se_resnet152():
    return _se_resnet_bottleneck('se_resnet152', [3, 8, 36, 3])
