"""Breath-metadata pretraining on MI355X: the breath store, the trainer and the command line.

The reference's third pretraining route (``scripts/main/preprocess_breath_meta_models.py``): ``cnn_regressor`` -- a ``CNNRegressor``
(models/torch_cnn_bm_regressor.py) on single breaths -- trained to regress each breath's metadata from its waveform under
``MSELoss`` (``CNNRegressorModel``, train_ards_detector.py:1081-1099); the saved model's ``breath_block`` then seeds a classifier
through ``--load-base-network``.

    python -m deepards_amd.regressor -n cnn_regressor --base-network resnet18 --cuda-no-dp --train-from-pickle <train.pkl | .npz> \\
           --test-from-pickle <test.pkl | .npz> -dt padded_breath_by_breath_with_full_bm_target -b 128 -e 10 --save-model reg.pth

* ``BreathMetaStore``: breath rows (N, 1, L) and an (N, M) float32 target table resident in HBM.  A batch is ONE gather launch
  for the rows (the gather, padding rule and filters of ``DeviceTileStore``) and ONE ``gather_rows`` of the targets: (B, 1, L)
  and (B, M).  ``from_dataset`` reads a breath-level ``ingest.IngestedDataset`` (a ``*_bm_target`` pickle or its .npz);
  ``from_windows`` flattens a window dataset that carries per-breath metadata to N NB breath rows.
* ``RegressorTrainer``: one step = the whole batch through the breath block as ONE BatchNorm window, the fused head (pool,
  linear_final, MSE and their gradients), the fused optimiser -- eager, or a captured graph per batch shape.  ``test_step`` runs
  with train-mode modules under ``no_grad`` (the reference's test epoch never calls ``model.eval()``), so it runs on every
  backbone, ResNets included.

Refused: more than one GPU and folds in flight (BatchNorm over the whole batch is a different function when the batch is split),
k-folds (the dataset's target slot holds ``[nan]``: no class to stratify patients by), ``--freeze-base-network``, any ``-loss``,
bf16 / f32x3p arithmetic.  Not built: the ``*_bm_target`` datasets from raw ventilator files.
"""
import numpy as np
import torch

from . import functional as F_
from . import hip_ops as H
from .data import DeviceTileStore
from .models.regressor import CNNRegressor, regressor_f32_only
from .train import HotPathTrainer

REGRESSOR_NETWORKS = ('cnn_regressor',)
# dataset type -> M, the width of the breath-metadata target (dataset.py:522-529)
BM_TARGET_TYPES = {'padded_breath_by_breath_with_limited_bm_target': 3,
                   'padded_breath_by_breath_with_experimental_bm_target': 7,
                   'padded_breath_by_breath_with_full_bm_target': 9}
WINDOW_METADATA_TYPE = 'padded_breath_by_breath_with_flow_time_features'       # the one window type with per-breath metadata


class BreathMetaStore(object):
    """Breath rows and their metadata targets, for ``(B, 1, L)`` / ``(B, M)`` batches.

    ``rows`` (N, 1, L) RAW flow, ``targets`` (N, M) finite.  ``mu`` / ``std``: one scalar each; when neither is given nor taken
    from ``scaling_from`` (the train store, for a test store) they are the plain mean / std over all samples of the rows.
    ``padded``: mu is subtracted from non-zero samples only (the ``padded_breath_by_breath`` rule, dataset.py:1375-1377).  The
    frequency filters are those of ``DeviceTileStore`` (``set_filters``), through the same gather kernels."""

    def __init__(self, rows, targets, mu=None, std=None, device='cuda', scaling_from=None, padded=True, patient_slot=None,
                 dataset_type=None):
        w = np.asarray(rows, dtype=np.float64)
        if w.ndim != 3 or w.shape[1] != 1 or w.shape[0] < 1:
            raise ValueError('rows must be (N >= 1, 1, L), got %s' % (w.shape,))
        t = np.asarray(targets, dtype=np.float64)
        if t.ndim != 2 or t.shape[0] != w.shape[0] or t.shape[1] < 1:
            raise ValueError('targets must be (N, M) with one row per breath, got %s for %d breaths' % (t.shape, w.shape[0]))
        bad = np.flatnonzero(~np.isfinite(t).all(axis=1))
        if bad.size:
            raise ValueError('breath %d has a non-finite target %s' % (int(bad[0]), t[bad[0]].tolist()))
        w = np.ascontiguousarray(w[:, None])                                   # (N, 1, 1, L): windows of one breath
        if scaling_from is not None:
            mu, std = scaling_from.mu, scaling_from.std
        elif mu is None or std is None:
            from .tiles import scaling_factors_for_indices
            mu, std = scaling_factors_for_indices(w)
        self.store = DeviceTileStore(w, np.zeros((w.shape[0], 2), dtype=np.float32), mu, std, device=device)
        self.store.padded = bool(padded)
        self.targets = torch.from_numpy(t.astype(np.float32)).contiguous().to(self.store.tiles.device)
        self.patient_slot = None if patient_slot is None else np.asarray(patient_slot, dtype=np.int64)
        self.dataset_type = dataset_type

    tiles = property(lambda self: self.store.tiles)
    mu = property(lambda self: self.store.mu)
    std = property(lambda self: self.store.std)
    padded = property(lambda self: self.store.padded)
    n_targets = property(lambda self: int(self.targets.shape[1]))
    seq_len = property(lambda self: int(self.store.tiles.shape[3]))

    def set_filters(self, **kw):
        self.store.set_filters(**kw)
        return self

    def __len__(self):
        return int(self.store.tiles.shape[0])

    def enable_kfolds(self, *a, **k):
        raise ValueError('breath-metadata pretraining is not run with k-folds: the dataset\'s target slot holds [nan], so there '
                         'is no class to stratify patients by')

    # ---- constructors --------------------------------------------------------------------------------------------------
    @staticmethod
    def _holdout_factors(ds, scaling_from):
        if scaling_from is None and ds.scaling_factors and None in ds.scaling_factors:
            return tuple(np.ravel(v)[:1] for v in ds.scaling_factors[None])
        return None, None

    @classmethod
    def from_dataset(cls, ds, device='cuda', scaling_from=None):
        """A breath-level ``ingest.IngestedDataset`` (a ``*_bm_target`` pickle or its .npz).  Holdout factors the file carries are
        kept; a window dataset goes through ``from_windows``."""
        if not getattr(ds, 'breath_level', False):
            return cls.from_windows(ds, device=device, scaling_from=scaling_from)
        if ds.total_kfolds is not None:
            raise ValueError('breath-metadata pretraining is not run with k-folds; got a dataset with %d folds' % ds.total_kfolds)
        mu, std = cls._holdout_factors(ds, scaling_from)
        return cls(ds.windows, ds.targets, mu, std, device=device, scaling_from=scaling_from,
                   padded='padded_breath_by_breath' in str(ds.dataset_type), patient_slot=ds.patient_slot,
                   dataset_type=str(ds.dataset_type))

    @classmethod
    def from_windows(cls, ds, device='cuda', scaling_from=None):
        """Any prepared window dataset that carries per-breath metadata (``padded_breath_by_breath_with_flow_time_features``:
        (NB, 9) per window, STANDARDISED by the reference when it builds the dataset) flattened to N NB breath rows whose
        targets are its metadata rows."""
        if getattr(ds, 'breath_level', False):
            return cls.from_dataset(ds, device=device, scaling_from=scaling_from)
        if ds.metadata is None:
            raise ValueError('a %s dataset carries no per-breath metadata to regress: only %s (5-item sequences with (NB, 9) '
                             'metadata) and the *_bm_target types do' % (ds.dataset_type, WINDOW_METADATA_TYPE))
        if ds.total_kfolds is not None:
            raise ValueError('breath-metadata pretraining is not run with k-folds; got a dataset with %d folds' % ds.total_kfolds)
        n, nb, c, l = ds.windows.shape
        meta = np.asarray(ds.metadata, dtype=np.float64).reshape(n, -1)
        if c != 1 or meta.shape[1] % nb:
            raise ValueError('from_windows takes one-channel windows with one metadata row per breath, got windows %s and '
                             'metadata %s' % (ds.windows.shape, meta.shape))
        mu, std = cls._holdout_factors(ds, scaling_from)
        slot = None if ds.patient_slot is None else np.repeat(ds.patient_slot, nb)
        return cls(ds.windows.reshape(n * nb, 1, l), meta.reshape(n * nb, -1), mu, std, device=device, scaling_from=scaling_from,
                   padded='padded_breath_by_breath' in str(ds.dataset_type), patient_slot=slot, dataset_type=str(ds.dataset_type))

    @classmethod
    def from_pickle(cls, path, device='cuda', scaling_from=None):
        """``--train-from-pickle`` / ``--test-from-pickle``: the reference's dataset pickle (parsed without unpickling) or its
        .npz export."""
        from . import ingest
        return cls.from_dataset(ingest.load_dataset(path), device=device, scaling_from=scaling_from)

    # ---- batches -------------------------------------------------------------------------------------------------------
    def _batch(self, idx, out):
        ox, ot = out if out is not None else (None, None)
        b = idx.numel()
        x = self.store._gather(idx, None if ox is None else ox.view(b, 1, 1, self.seq_len))
        return x.view(b, 1, self.seq_len), H.gather_rows(self.targets, idx, out=ot)

    def batch(self, idx, out=None):
        """(inputs (B, 1, L) float32, targets (B, M) float32) for a host index list: one gather launch each.  ``out``: the
        (x, t) buffers to fill in place (``RegressorTrainer.static_batch``)."""
        idx = torch.as_tensor(idx, dtype=torch.int64)
        if idx.dim() != 1:
            raise ValueError('idx must be a 1-D index list')
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= len(self)):    # the gather reads tiles[idx] unchecked
            raise IndexError('breath index out of range [0, %d)' % len(self))
        return self._batch(idx.to(self.store.tiles.device).contiguous(), out)

    def device_indices(self, idx):
        """``DeviceTileStore.device_indices``: a whole epoch's indices checked and uploaded once."""
        return self.store.device_indices(idx)

    def batch_from_device(self, abs_idx, out=None):
        """``batch`` for (a slice of) a tensor ``device_indices`` returned; anything else is refused, as by the tile store."""
        if not (abs_idx.is_cuda and abs_idx.dtype == torch.int64 and abs_idx.dim() == 1 and abs_idx.is_contiguous()):
            raise ValueError('batch_from_device: a contiguous 1-D int64 device tensor from device_indices() expected')
        if abs_idx.numel() and getattr(self.store, '_checked_idx', {}).get(abs_idx.untyped_storage().data_ptr()) is None:
            raise ValueError('batch_from_device: indices must be (a slice of) a tensor returned by device_indices(), which '
                             'checks them against the store; use batch() for anything else')
        return self._batch(abs_idx, out)

    def epoch(self, batch_size, shuffle=True, generator=None, drop_odd=True):
        """Iterate one epoch like DataLoader(batch_size, shuffle) + clip_odd_batch_sizes: yields (idx, x (B, 1, L), t (B, M))."""
        for idx in epoch_index_batches(self, batch_size, shuffle, generator, drop_odd):
            x, t = self.batch(idx)
            yield idx, x, t


def epoch_index_batches(store, batch_size, shuffle=True, generator=None, drop_odd=True):
    """Host index batches of one epoch: a permutation from ``generator`` (torch's global RNG without one) in ``batch_size``
    slices, the last item of an odd batch dropped (train_ards_detector.py:482-494) when ``drop_odd``."""
    n = len(store)
    order = torch.randperm(n, generator=generator) if shuffle else torch.arange(n)
    out = []
    for s in range(0, n, batch_size):
        idx = order[s:s + batch_size]
        if drop_odd and batch_size != 1 and len(idx) % 2 == 1:
            idx = idx[:-1]
        if len(idx):
            out.append(idx)
    return out


def _device_batches(store, batches):
    """The epoch's batches as slices of ONE device tensor (uploaded once)."""
    if not batches:
        return []
    dev = store.device_indices(torch.cat(batches))
    out, s = [], 0
    for b in batches:
        out.append(dev[s:s + len(b)])
        s += len(b)
    return out


class RegressorTrainer(HotPathTrainer):
    """One ``CNNRegressor`` on one GPU.  ``train_step(inputs (B, 1, 224), target (B, M))``: one iteration of the reference's batch
    loop -- eager, or a captured graph per batch shape -- with the optimiser and clamp of ``HotPathTrainer``; returns the
    device-resident loss (``last_loss``; ``last_logits`` is the (B, M) output).  ``test_step(inputs, target)`` -> (loss (1,), out
    (B, M)): the forward with train-mode modules under ``no_grad``, as ``BaseTraining.run_test_epoch`` runs it.

    The loss is MSE; there is no choice.  One GPU, no folds in flight: BatchNorm takes its statistics over the whole batch, so
    a split batch is a different function."""

    def __init__(self, model, optimizer='sgd', learning_rate=1e-3, weight_decay=1e-4, momentum=0.9, clip_grad=True, clip_val=0.01,
                 world_size=1, rank=0, process_group=None, use_graph=True, folds_in_flight=None, loss=None, carry_state=False):
        if not isinstance(model, CNNRegressor):
            raise TypeError('RegressorTrainer trains a CNNRegressor, got %s' % type(model).__name__)
        if loss not in (None, 'mse'):
            raise ValueError('the regressor\'s loss is MSELoss (train_ards_detector.py:674); loss %r is not taken' % (loss,))
        if carry_state:
            raise ValueError('carry_state needs a CNNLSTMNetwork: a CNNRegressor has no recurrent state')
        if world_size != 1:
            raise NotImplementedError('the regressor trainer runs on one GPU: its BatchNorm takes its statistics over the whole '
                                      'batch, so a batch sharded over %d ranks is a different function' % world_size)
        if folds_in_flight is not None and int(folds_in_flight) > 1:
            raise NotImplementedError('folds in flight with the regressor trainer: its dataset has no folds')
        regressor_f32_only()
        super(RegressorTrainer, self).__init__(model, optimizer=optimizer, learning_rate=learning_rate, weight_decay=weight_decay,
                                               momentum=momentum, clip_grad=clip_grad, clip_val=clip_val, world_size=1, rank=0,
                                               process_group=None, use_graph=use_graph)
        self.loss, self._plain_bce = 'mse', False

    def _check(self, inputs, target):
        m = self.model.linear_final.out_features
        if inputs.dim() != 3 or inputs.shape[0] == 0:
            raise ValueError('a regressor step takes (B, C_in, 224) breaths, got %s' % (tuple(inputs.shape),))
        if target is None or target.dim() != 2 or tuple(target.shape) != (inputs.shape[0], m):
            raise ValueError('a regressor step takes a (%d, %d) target, got %s' %
                             (inputs.shape[0], m, None if target is None else tuple(target.shape)))

    def _forward_backward(self, inputs, target, zero_grad=False):
        if zero_grad:
            self.bucket.zero_grad()
        with F_.training_step(self.model):
            loss, out = self.model.forward_loss(inputs, target)
            F_.flush_forward(defer=True)
            torch.autograd.backward(loss, grad_tensors=self._one(loss))
            F_.flush_backward()
        return loss.detach(), out

    def _test_forward(self, inputs, target):
        with torch.no_grad(), F_.training_step(self.model):
            loss, out = self.model.forward_loss(inputs, target)
            F_.flush_forward()                                    # train-mode forward: BN running statistics do move
        return loss, out

    def train_step(self, inputs, target, reset=None):
        self._check(inputs, target)
        return super(RegressorTrainer, self).train_step(inputs, target.contiguous(), reset)

    def test_step(self, inputs, target, reset=None):
        self._check(inputs, target)
        return super(RegressorTrainer, self).test_step(inputs, target.contiguous(), reset)


def run_regressor_train_epoch(trainer, store, batch_size=128, shuffle=True, generator=None):
    """Yields the (cloned, device-resident) loss of every batch: two gather launches -- into the captured step's own buffers
    once there are some -- and the step.  Odd batches are clipped (train_ards_detector.py:146-147)."""
    for idx in _device_batches(store, epoch_index_batches(store, batch_size, shuffle, generator, drop_odd=True)):
        x, t = store.batch_from_device(idx, out=trainer.static_batch(idx.numel()))
        yield trainer.train_step(x, t).clone()


def run_regressor_test_epoch(trainer, store, batch_size=128, shuffle=True, generator=None):
    """Yields (target (B, M), out (B, M), loss (1,)) of every batch, on the device.  Test batches keep their odd item
    (``BaseTraining.clip_odd_batches`` is False)."""
    for idx in _device_batches(store, epoch_index_batches(store, batch_size, shuffle, generator, drop_odd=False)):
        x, t = store.batch_from_device(idx)
        loss, out = trainer.test_step(x, t)
        yield t, out, loss


def build_parser():
    """The driver's parser with this stage's own ``-n`` choice and the three ``*_bm_target`` dataset types."""
    from . import train_ards_detector as T
    parser = T.build_parser()
    parser.prog = 'deepards_amd.regressor'
    for action in parser._actions:
        if action.dest == 'network':
            action.choices = list(REGRESSOR_NETWORKS)
        elif action.dest == 'dataset_type':
            action.choices = list(action.choices) + sorted(BM_TARGET_TYPES)
    return parser


def main(argv=None):
    """``python -m deepards_amd.regressor -n cnn_regressor <the driver's flags>``."""
    import sys
    from . import train_ards_detector as T
    argv = sys.argv[1:] if argv is None else list(argv)
    given = [a for a in argv if a.split('=')[0] in ('-loss', '--loss-func')]
    if given:                                   # (after the merge with defaults.yml "unset" reads as bce: asked here, before it)
        raise SystemExit('%s with -n cnn_regressor: the regressor\'s loss is MSELoss (train_ards_detector.py:674), there is no '
                         'choice' % given[0])
    return T.stage_main(argv, build_parser(), REGRESSOR_NETWORKS, T.regressor_network_map, dict(T.BUILD_DEFAULTS))


if __name__ == '__main__':
    main()
