"""The UNet of the reference's autoencoder pretraining route (``--base-network unet``) on MI355X.

Operator surface of reference ``deepards/models/unet.py`` (``UNet(n_class)``), written here in this package's own terms: the same
children and attribute names (``dconv_down1..4``, ``maxpool``, ``upsample``, ``dconv_up3..1``, ``conv_last``, ``n_out_filters`` =
512, ``encoder``), so ``state_dict`` keys and their order match -- the ``encoder.N.*`` entries are the SAME tensors as
``dconv_downK.*`` -- and a reference state_dict loads with ``strict=True``.  As in ``autoencoder.py`` the torch.nn leaf modules are
only parameter containers: ``forward`` runs the HIP kernels through ``deepards_amd.functional`` on all rows at once.

    double_conv(a, b)   Conv1d(a, b, 3, padding=1) -> ReLU -> Conv1d(b, b, 3, padding=1) -> ReLU       (all with bias)
    down                1 -> 64 -> 128 -> 256 -> 512, MaxPool1d(2) between
    up x 3              Upsample(x2, linear, align_corners=True), cat with the skip (upsampled first), double_conv
    conv_last           Conv1d(64, n_class, 1)

There is no BatchNorm and no dropout: ``eval()`` computes the same function as ``train()``.

Refused: ``n_class != 1`` (the output stage and its MSE are built for one reconstructed channel), more than one input channel, a
length that is no multiple of 8 (three pools, three x2 upsamples, a cat at every level), CPU tensors, bf16 / f32x3p arithmetic,
``sels=`` (no pool decision is stored here, so there is none to force), and a gradient through ``encoder`` (the second stage -- a
classifier on the pretrained encoder -- is not built).
"""
import torch
import torch.nn as nn

from .. import functional as F_

DOWN = ((1, 64), (64, 128), (128, 256), (256, 512))
UP = ((256 + 512, 256), (128 + 256, 128), (128 + 64, 64))          # dconv_up3, dconv_up2, dconv_up1


def double_conv(in_channels, out_channels):
    return nn.Sequential(nn.Conv1d(in_channels, out_channels, 3, padding=1), nn.ReLU(inplace=True),
                         nn.Conv1d(out_channels, out_channels, 3, padding=1), nn.ReLU(inplace=True))


def _check_rows(x, sels=None):
    if sels is not None:
        raise NotImplementedError('the UNet takes no sels=: its pools store no decisions (the backward re-derives the winner from '
                                  'the stored activation), so there are none to take instead of deciding')
    if x.dim() != 3:
        raise ValueError('the UNet takes rows (N, 1, L), got %s' % (tuple(x.shape),))
    if x.shape[1] != 1:
        raise NotImplementedError('the UNet reads one channel (dconv_down1 starts with Conv1d(1, 64)), got %d' % x.shape[1])
    if x.shape[2] < 8 or x.shape[2] % 8:
        raise NotImplementedError('the UNet needs a length that is a multiple of 8 -- three MaxPool1d(2) whose x2 upsamples must '
                                  'meet the skip maps again for the cat -- got %d' % x.shape[2])
    if not x.is_cuda:
        raise RuntimeError('the UNet needs CUDA (MI355X) tensors; there is no CPU fallback')
    return x.contiguous().float().view(x.shape[0], x.shape[2])


class _UNetEncoder(nn.Sequential):
    """``UNet.encoder``: dconv_down1..4 with MaxPool1d(2) between -- forward only, (N, 1, L) -> (N, 512, L / 8)."""

    def forward(self, x):
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError(_ENCODER_GRADIENT)
        rows = _check_rows(x)
        owner = self._owner[0]
        with torch.no_grad():
            return F_.unet_encode(rows, owner._double_convs()[:4], owner.precise_convs).permute(0, 2, 1).contiguous()


# (the reason autoencoder._Encoder gives, with this network's name)
_ENCODER_GRADIENT = ('a gradient through the UNet\'s encoder means the second stage (a classifier on the pretrained encoder), which '
                     'is not built; call it under torch.no_grad()')


class UNet(nn.Module):
    """(N, 1, L) -> recon (N, 1, L).  ``forward_loss(x)`` -> (loss (1,), recon): the MSE against x with its gradient, one autograd
    node (``functional.UNetFunction``); under ``eval()`` or ``no_grad`` the forward-only ``functional.unet_forward``."""

    precise_convs = False          # F(4,3) on dconv_down4's 512 -> 512 conv stays: the gradients hold the tests' bound with it

    def __init__(self, n_class):
        super(UNet, self).__init__()
        if n_class != 1:
            raise NotImplementedError('UNet(n_class=%r): the output stage (Conv1d(64, 1, 1) + MSELoss against the one-channel '
                                      'input) is built for n_class = 1 only' % (n_class,))
        for k, (ci, co) in enumerate(DOWN, 1):
            setattr(self, 'dconv_down%d' % k, double_conv(ci, co))
        self.maxpool = nn.MaxPool1d(2)
        self.upsample = nn.Upsample(scale_factor=2, mode='linear', align_corners=True)
        for k, (ci, co) in zip((3, 2, 1), UP):
            setattr(self, 'dconv_up%d' % k, double_conv(ci, co))
        self.conv_last = nn.Conv1d(64, n_class, 1)
        self.n_out_filters = 512
        self.encoder = _UNetEncoder(self.dconv_down1, self.maxpool, self.dconv_down2, self.maxpool, self.dconv_down3, self.maxpool,
                                    self.dconv_down4)
        self.encoder._owner = (self,)                # (a tuple: not a registered child, no reference cycle in the module tree)

    def _double_convs(self):
        """(w1, b1, w2, b2) of down1..4, up3, up2, up1: functional.UNetFunction's order."""
        mods = [getattr(self, 'dconv_down%d' % k) for k in range(1, 5)] + [getattr(self, 'dconv_up%d' % k) for k in (3, 2, 1)]
        return [(m[0].weight, m[0].bias, m[2].weight, m[2].bias) for m in mods]

    def forward_loss(self, x, sels=None):
        rows = _check_rows(x, sels)
        dcs, last = self._double_convs(), (self.conv_last.weight, self.conv_last.bias)
        if self.training and torch.is_grad_enabled():
            recon, loss = F_.UNetFunction.apply(rows, self.precise_convs, *[p for dc in dcs for p in dc], *last)
        else:
            with torch.no_grad():
                recon, loss = F_.unet_forward(rows, dcs, last, self.precise_convs)
        return loss, recon.view(x.shape[0], 1, x.shape[2])

    def forward(self, x, sels=None):
        return self.forward_loss(x, sels)[1]
