"""Autoencoder pretraining on MI355X: the trainer and the command line.

The reference's ``network_map['autoencoder']`` (``AutoencoderModel``, train_ards_detector.py:1102-1116): an ``AutoencoderNetwork``
(models/autoencoder_cnn.py, models/autoencoder_network.py) trained to reproduce its input rows under ``MSELoss``; the test epoch
books ``test_mae``, ``r2`` and ``test_mse`` per batch (``RegressorMixin``, :661-677).

    python -m deepards_amd.autoencoder -n autoencoder --base-network basic_cnn_ae | unet --cuda-no-dp -p <dataset.pkl | .npz> \\
           --test-from-pickle <...> --save-model pretrained_ae.pth

* ``AutoencoderTrainer``: one step = the whole network and its loss as one autograd node (``functional.AutoencoderFunction``),
  the batched parameter-gradient folds and the fused optimiser -- eager, or a captured graph per input shape, the loss on the
  device.  ``test_step`` runs under ``model.eval()`` (BatchNorm on its running statistics) and returns the reconstruction.
* any prepared ``ARDSRawDataset`` pickle or ``.npz`` serves; targets are ignored (the reference's ``_autoencoder_target`` is NaN).
* ``--base-network unet``: the same trainer on ``AutoencoderNetwork(UNet(1))`` (models/unet.py, ``functional.UNetFunction``).  It has
  no BatchNorm; more than one GPU and folds in flight are refused for it too -- not built, not run -- as are lengths that are no
  multiple of 8.

Refused: more than one GPU and folds in flight (BatchNorm runs over the WHOLE batch, so a split batch is another function), bf16 /
f32x3p arithmetic, ``--load-base-network`` / ``--freeze-base-network`` (the second stage is not built), lengths that are no
multiple of 16.  A saved autoencoder is not accepted as a base network (``checkpoint.load_autoencoder`` reads it back).
"""
from . import functional as F_
from .models.autoencoder import AutoencoderCNN, AutoencoderNetwork
from .models.unet import UNet
from .train import SelfSupervisedTrainer, epoch_shards_on_device

AUTOENCODER_NETWORKS = ('autoencoder',)
AUTOENCODER_BASE_NETWORK = 'basic_cnn_ae'
AUTOENCODER_BASE_NETWORKS = (AUTOENCODER_BASE_NETWORK, 'unet')       # the reference's two (base_networks of its driver)
AUTOENCODER_DATASET_TYPE = 'unpadded_downsampled_autoencoder_sequences'


class AutoencoderTrainer(SelfSupervisedTrainer):
    """One autoencoder on one GPU.  ``train_step(inputs)``: one iteration of the reference's batch loop on windows (B, NB, 1, L)
    (an ``AutoencoderNetwork``) or rows (N, 1, L) (an ``AutoencoderCNN``) -- eager, or a captured graph per input shape -- with the
    optimiser and clamp of ``HotPathTrainer``; returns the device-resident loss (``last_loss``; ``last_logits`` is the
    reconstruction).  ``test_step(inputs)``: the forward under ``model.eval()`` -> recon (N, 1, L); ``last_test_loss`` its MSE.

    The step scaffold -- the placeholder target (the input is its own), the refusals, forward/backward around
    ``_loss_and_output`` and ``model.eval()`` in the test step -- is ``train.SelfSupervisedTrainer``."""
    batch_alone = 'an autoencoder step takes the batch alone: the input is its own target'

    def __init__(self, model, optimizer='sgd', learning_rate=1e-3, weight_decay=1e-4, momentum=0.9, clip_grad=True, clip_val=0.01,
                 world_size=1, rank=0, process_group=None, use_graph=True, folds_in_flight=None):
        if not isinstance(model, (AutoencoderNetwork, AutoencoderCNN, UNet)):
            raise TypeError('AutoencoderTrainer trains an AutoencoderNetwork / AutoencoderCNN / UNet, got %s' % type(model).__name__)
        unet = isinstance(model.base_network if isinstance(model, AutoencoderNetwork) else model, UNet)
        if unet:
            one_gpu = ('the autoencoder trainer runs on one GPU: a UNet step sharded over %d ranks (the gradient all-reduce of '
                       'this trainer) is not built and was not run')
            no_folds = 'folds in flight with the autoencoder trainer: not built and not run for the UNet'
        else:
            one_gpu = ('the autoencoder trainer runs on one GPU: its BatchNorm takes its statistics over the whole batch, so a '
                       'batch sharded over %d ranks is a different function')
            no_folds = 'folds in flight with the autoencoder trainer: one model, one whole-batch BatchNorm per step'
        super(AutoencoderTrainer, self).__init__(model, one_gpu, no_folds, world_size=world_size, folds_in_flight=folds_in_flight,
                                                 optimizer=optimizer, learning_rate=learning_rate, weight_decay=weight_decay,
                                                 momentum=momentum, clip_grad=clip_grad, clip_val=clip_val, use_graph=use_graph)
        (F_._unet_f32_only if unet else F_._ae_f32_only)()
        self.last_test_loss = None

    def _check_batch(self, batch):
        want = 4 if isinstance(self.model, AutoencoderNetwork) else 3
        if batch.dim() != want or batch.shape[0] == 0:
            raise ValueError('an autoencoder step takes %s, got %s' %
                             ('(B, NB, 1, L) windows' if want == 4 else '(N, 1, L) rows', tuple(batch.shape)))

    def _loss_and_output(self, inputs):
        return self.model.forward_loss(inputs)

    def test_step(self, batch, target=None, reset=None):
        self.last_test_loss, recon = super(AutoencoderTrainer, self).test_step(batch, target, reset)
        return recon


def run_autoencoder_train_epoch(trainer, store, batch_size=16, shuffle=True, generator=None):
    """Yields the (cloned, device-resident) loss of every batch: a gather launch and the step."""
    for idx in epoch_shards_on_device(store, batch_size, shuffle, generator):
        x, _ = store.batch_from_device(idx)
        yield trainer.train_step(x).clone()


def run_autoencoder_test_epoch(trainer, store, batch_size=16, shuffle=True, generator=None):
    """Yields (inputs (B, NB, 1, L), recon (B NB, 1, L), loss (1,)) of every batch, on the device."""
    for idx in epoch_shards_on_device(store, batch_size, shuffle, generator):
        x, _ = store.batch_from_device(idx)
        recon = trainer.test_step(x)
        yield x, recon, trainer.last_test_loss.clone()


def build_parser():
    """The driver's parser with this stage's own ``-n`` / ``--base-network`` choices and its dataset type."""
    from . import train_ards_detector as T
    parser = T.build_parser()
    parser.prog = 'deepards_amd.autoencoder'
    for action in parser._actions:
        if action.dest == 'network':
            action.choices = list(AUTOENCODER_NETWORKS)
        elif action.dest == 'base_network':
            action.choices = list(action.choices) + list(AUTOENCODER_BASE_NETWORKS)
    return parser


def main(argv=None):
    """``python -m deepards_amd.autoencoder -n autoencoder <the driver's flags>``."""
    from . import train_ards_detector as T
    return T.stage_main(argv, build_parser(), AUTOENCODER_NETWORKS, T.autoencoder_network_map, dict(T.BUILD_DEFAULTS))


def __getattr__(name):
    if name == 'autoencoder_network_map':                 # (lives beside the driver's other maps; importing it here would be circular)
        from . import train_ards_detector as T
        return T.autoencoder_network_map
    raise AttributeError(name)


if __name__ == '__main__':
    main()
