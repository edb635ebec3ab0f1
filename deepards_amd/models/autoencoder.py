"""The autoencoder of the reference's pretraining route on MI355X.

Operator surface of reference ``deepards/models/autoencoder_cnn.py`` (AutoencoderCNN) and ``autoencoder_network.py``
(AutoencoderNetwork), written here in this package's own terms: the same constructors, children and attributes
(``n_out_filters`` = 512, ``encoder``, ``breath_block``, ``base_network``), so ``state_dict`` keys and their order match -- the
``encoder.N.*`` / ``breath_block.N.*`` entries are the SAME tensors as ``conv_downK.*`` / ``bnK.*`` -- and a reference state_dict
loads.  As in ``vgg.py`` the torch.nn leaf modules are only parameter containers: ``forward`` runs the HIP kernels through
``deepards_amd.functional`` on all rows at once.

    down x 4    Conv1d(k3, p1, bias) -> BatchNorm1d -> MaxPool1d(2, return_indices)      1 -> 64 -> 128 -> 256 -> 512
    up   x 4    MaxUnpool1d(2) -> ConvTranspose1d(k3, p1, bias)                          512 -> 256 -> 128 -> 64 -> 1

There is NO ReLU (``self.relu`` exists and is never called), and BatchNorm runs over ALL N rows as one batch: one window, unlike
every other model of this package.  ``eval()`` is honoured: BatchNorm becomes the per-channel affine of its running statistics.

Refused: a length that is no multiple of 16 (four pools must unpool to the input's length), more than one channel, bf16 / f32x3p
arithmetic, and a gradient through ``encoder`` (the second stage -- a classifier on the pretrained encoder -- is not built).
"""
import torch
import torch.nn as nn

from .. import functional as F_

CHANNELS = (1, 64, 128, 256, 512)
ENCODED_POOL = 14


def _check_rows(x):
    if x.dim() != 3:
        raise ValueError('the autoencoder takes rows (N, 1, L), got %s' % (tuple(x.shape),))
    if x.shape[1] != 1:
        raise NotImplementedError('the autoencoder reads one channel (conv_down1 is Conv1d(1, 64)), got %d' % x.shape[1])
    if x.shape[2] < 16 or x.shape[2] % 16:
        raise NotImplementedError('the autoencoder needs a length that is a multiple of 16 -- four MaxPool1d(2) whose '
                                  'MaxUnpool1d(2) must give the input length back for the MSE -- got %d' % x.shape[2])
    if not x.is_cuda:
        raise RuntimeError('the autoencoder needs CUDA (MI355X) tensors; there is no CPU fallback')
    return x.contiguous().float().view(x.shape[0], x.shape[2])


class _Encoder(nn.Sequential):
    """``AutoencoderCNN.encoder``: the down stages with plain MaxPool1d(2), then MaxPool1d(14) -- forward only."""

    def forward(self, x):
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError('a gradient through the autoencoder\'s encoder means the second stage (a classifier on the '
                                      'pretrained encoder), which is not built; call it under torch.no_grad()')
        rows = _check_rows(x)
        owner = self._owner[0]
        with torch.no_grad():
            h, _ = F_.ae_encode(rows, owner._down(), owner._bn_states(), self.training)
            if h.shape[1] < ENCODED_POOL:
                raise ValueError('MaxPool1d(14) needs L / 16 >= 14, got %d' % h.shape[1])
            n = h.shape[1] // ENCODED_POOL                                  # (not the trained path: plain torch)
            return h[:, :n * ENCODED_POOL].reshape(h.shape[0], n, ENCODED_POOL, h.shape[2]).amax(dim=2).permute(0, 2, 1).contiguous()


class AutoencoderCNN(nn.Module):
    """(N, 1, L) -> recon (N, 1, L).  ``forward(x, sels=None)``: ``sels`` four decision tensors (``hip_ops.sel_from_bool``) taken
    instead of deciding.  ``forward_loss(x, sels=None)`` -> (loss (1,), recon): the MSE against x with its gradient, one autograd
    node.  ``last_sels``: the decisions of the last train-mode pass."""

    precise_convs = False          # no conv here has 512 channels on both sides: F(4,3) is never chosen (hip_ops._wino)

    def __init__(self):
        super(AutoencoderCNN, self).__init__()
        self.relu = nn.ReLU()
        self.maxpool = nn.MaxPool1d(2, return_indices=True)
        for k in range(1, 5):
            setattr(self, 'conv_down%d' % k, nn.Conv1d(CHANNELS[k - 1], CHANNELS[k], 3, padding=1))
            setattr(self, 'bn%d' % k, nn.BatchNorm1d(CHANNELS[k]))
        self.maxunpool = nn.MaxUnpool1d(2)
        for k in range(1, 5):
            setattr(self, 'conv_up%d' % k, nn.ConvTranspose1d(CHANNELS[5 - k], CHANNELS[4 - k], 3, padding=1))
        self.n_out_filters = 512
        mods = []
        for k in range(1, 5):
            mods += [getattr(self, 'conv_down%d' % k), getattr(self, 'bn%d' % k), nn.MaxPool1d(2)]
        self.encoder = _Encoder(*mods, nn.MaxPool1d(ENCODED_POOL))
        self.encoder._owner = (self,)                # (a tuple: not a registered child, no reference cycle in the module tree)
        self.last_sels = None

    def __getstate__(self):
        state = self.__dict__.copy()
        state['last_sels'] = None                    # (a saved model carries no decisions of some training batch)
        return state

    def _down(self):
        return [(c.weight, c.bias, b.weight, b.bias) for c, b in
                ((getattr(self, 'conv_down%d' % k), getattr(self, 'bn%d' % k)) for k in range(1, 5))]

    def _up(self):
        return [(c.weight, c.bias) for c in (getattr(self, 'conv_up%d' % k) for k in range(1, 5))]

    def _bn_states(self):
        return [F_.BNState(getattr(self, 'bn%d' % k)) for k in range(1, 5)]

    def forward_loss(self, x, sels=None):
        rows = _check_rows(x)
        if sels is not None and len(sels) != 4:
            raise ValueError('sels: the four stages\' decision tensors expected')
        if self.training:
            tap = []
            params = [p for st in self._down() for p in st] + [p for st in self._up() for p in st]
            recon, loss = F_.AutoencoderFunction.apply(rows, self._bn_states(), sels, self.precise_convs, tap, *params)
            self.last_sels = tap
        else:
            with torch.no_grad():
                h, taken = F_.ae_encode(rows, self._down(), self._bn_states(), False, sels, self.precise_convs)
                recon, _, loss, _, _ = F_.ae_decode(h, taken, self._up(), rows, self.precise_convs)
        return loss, recon.view(x.shape[0], 1, x.shape[2])

    def forward(self, x, sels=None):
        return self.forward_loss(x, sels)[1]


class AutoencoderNetwork(nn.Module):
    """(B, NB, 1, L) windows (and the metadata the driver passes) -> recon (B NB, 1, L): all B NB rows one BatchNorm batch.
    ``base_network``: an AutoencoderCNN, or a ``models.unet.UNet`` (no BatchNorm; it takes no ``sels``)."""

    def __init__(self, base_network):
        super(AutoencoderNetwork, self).__init__()
        self.base_network = base_network
        self.breath_block = self.base_network.encoder
        self.breath_block.n_out_filters = self.base_network.n_out_filters

    @staticmethod
    def _rows(x):
        if len(x.shape) != 4:
            raise Exception('Data is not in expected shape. Supply a 4 dimensional input with shape <batches, sub-batches, chans, '
                            'timeseries data>')
        return x.reshape(x.shape[0] * x.shape[1], x.shape[2], x.shape[3])

    def forward_loss(self, x, metadata=None, sels=None):
        return self.base_network.forward_loss(self._rows(x), sels)

    def forward(self, x, metadata=None, sels=None):
        return self.base_network(self._rows(x), sels)
