"""Siamese pretraining on MI355X: the triplet store, the trainer and the command line.

The reference's first stage (``scripts/main/preprocess_siamese_models.py``): ``siamese_cnn_linear`` / ``siamese_cnn_lstm`` /
``siamese_cnn_transformer`` trained on ``SiameseNetworkDataset`` triplets (dataset.py:1463-1612) by the loops of ``SiameseMixin``
(train_ards_detector.py:558-658); the saved model's ``breath_block`` then seeds a classifier through ``--load-base-network``.

    python -m deepards_amd.siamese -n siamese_cnn_linear --cuda-no-dp -p <dataset.pkl | .npz> --test-from-pickle <...> \\
           --base-network densenet18 --save-model pretrained.pth

* ``SiameseTileStore``: windows resident in HBM, sorted so that a patient's windows are contiguous; a triplet batch is ONE draw
  launch (``da_siamese_draw``: positive = the patient's next window, negative uniform over the other patients' windows, from a
  counter-based hash of (seed, step, slot) -- the reference draws with ``np.random.choice`` on the host per item) and ONE gather
  launch for all (4 or 3) B windows.
* ``SiameseTrainer``: one step = the triplet batch through ONE tower pass, the fused head, backward, the fused optimiser.
  ``share_anchor=False`` (default) keeps the reference's four-pass semantics in a 4 B-window pass: the anchor runs twice, with
  its own dropout masks each time, and BatchNorm's running statistics take its update twice, in the reference's order (seq, pos,
  seq, neg).  ``share_anchor=True`` is a DEPARTURE that saves a quarter of the tower work: a 3 B pass -- one dropout mask and
  one running-statistics update for the anchor, whose gradient is the sum over both pairs.
* the test step runs under ``model.eval()`` as the reference's siamese test epoch does (:635): dropout off on a DenseNet; a
  backbone whose BatchNorm keeps running statistics (ResNet, SE-ResNet, VGG) would mean inference on them, which this package
  does not have -- ``test_step`` raises, and the driver classes train such a network and skip the test epoch with one notice.

Not built: ``SiameseARDSClassifier`` / ``--load-siamese`` (the reference cannot construct it), data parallelism and folds in
flight for these trainers, k-folds (the reference's dataset is not meant for them), datasets from raw ventilator files.
"""
import numpy as np
import torch

from . import siamese_ops as SO
from .data import DeviceTileStore
from .models.siamese import _SiameseNetwork
from .train import SelfSupervisedTrainer

SIAMESE_NETWORKS = ('siamese_cnn_linear', 'siamese_cnn_lstm', 'siamese_cnn_transformer')


def group_patients(patients):
    """patients (N,) ids -> (kept, order): ``kept`` the indices of the windows whose patient has at least two windows
    (dataset.py:1491-1498: no positive example exists for the others), ``order`` a permutation of ``kept`` that makes every
    patient's windows contiguous -- patients in order of first appearance, a patient's windows in their original order."""
    patients = np.asarray(patients)
    if patients.ndim != 1:
        raise ValueError('one patient id per window expected')
    slot, seen = np.empty(len(patients), dtype=np.int64), {}
    for i, p in enumerate(patients.tolist()):
        slot[i] = seen.setdefault(p, len(seen))
    counts = np.bincount(slot, minlength=len(seen)) if len(patients) else np.zeros(0, dtype=np.int64)
    kept = np.flatnonzero(counts[slot] >= 2)
    order = kept[np.argsort(slot[kept], kind='stable')]
    return kept, order, slot


class SiameseTileStore(object):
    """Windows and one patient id per window, for triplet batches.

    Patients with a single window are dropped; the rest are sorted stably by patient (``original_index`` maps a store index
    back to the caller's); ``mu`` / ``std`` come from the WHOLE set (``scaling_factors[None]``: the reference's dataset is not
    meant for k-folds) unless given, or taken from ``scaling_from`` (the train store, for a test store).  The ``padded`` rule and
    the frequency filters are those of ``DeviceTileStore`` (``set_filters``), through the same gather kernels.  Neither a patient
    count of 1 nor one of N can occur: at least two patients with at least two windows each are required (ValueError)."""

    def __init__(self, windows, patients, mu=None, std=None, device='cuda', scaling_from=None, padded=False, seed=0):
        w = np.asarray(windows, dtype=np.float64)
        if w.ndim != 4:
            raise ValueError('windows must be (N, NB, C, L)')
        patients = np.asarray(patients)
        if patients.shape != (w.shape[0],):
            raise ValueError('one patient id per window expected')
        kept, order, slot = group_patients(patients)
        self.dropped = int(w.shape[0] - len(kept))
        slots = slot[order]
        if len(np.unique(slots)) < 2:
            raise ValueError('siamese triplets need at least two patients with two or more windows each (a negative example '
                             'comes from another patient); %d left after dropping single-window patients' % len(np.unique(slots)))
        w = np.ascontiguousarray(w[order])
        self.original_index = order
        self.patients = patients[order]
        change = np.flatnonzero(np.diff(slots)) + 1
        starts = np.concatenate([[0], change])
        counts = np.diff(np.concatenate([starts, [len(slots)]]))
        self.patient_starts, self.patient_counts = starts.astype(np.int64), counts.astype(np.int64)
        if scaling_from is not None:
            mu, std = scaling_from.mu, scaling_from.std
        elif mu is None or std is None:
            from .tiles import scaling_factors_for_indices
            mu, std = scaling_factors_for_indices(w)
        self.store = DeviceTileStore(w, np.zeros((w.shape[0], 2), dtype=np.float32), mu, std, device=device)
        self.store.padded = bool(padded)
        dev = self.store.tiles.device
        self.pat_start = torch.from_numpy(np.repeat(starts, counts).astype(np.int32)).to(dev)
        self.pat_count = torch.from_numpy(np.repeat(counts, counts).astype(np.int32)).to(dev)
        self.seed = int(seed)
        self.draws = 0                                    # triplet batches drawn so far: the default ``step`` of the next one

    # ---- what the gather reads ---------------------------------------------------------------------------------------
    tiles = property(lambda self: self.store.tiles)
    mu = property(lambda self: self.store.mu)
    std = property(lambda self: self.store.std)
    padded = property(lambda self: self.store.padded)
    n_sub_batches = property(lambda self: int(self.store.tiles.shape[1]))

    def set_filters(self, **kw):
        self.store.set_filters(**kw)
        return self

    def __len__(self):
        return int(self.store.tiles.shape[0])

    def enable_kfolds(self, *a, **k):
        raise ValueError('the siamese dataset is not meant to be run with k-folds (dataset.py:1597): triplets are drawn over the '
                         'whole set')

    # ---- constructors --------------------------------------------------------------------------------------------------
    @classmethod
    def from_dataset(cls, ds, device='cuda', scaling_from=None, seed=0):
        """Any prepared ``ingest.IngestedDataset`` (an ARDSRawDataset pickle or its .npz) as a pretraining set: its windows and
        patients, the targets unused.  Holdout factors the dataset carries are kept; a k-fold dataset is refused."""
        if ds.total_kfolds is not None:
            raise ValueError('the siamese dataset is not meant to be run with k-folds (dataset.py:1597); got a dataset with '
                             '%d folds' % ds.total_kfolds)
        patients = ds.patient_slot if ds.patient_slot is not None else ds.patients
        if patients is None:
            raise ValueError('triplets are drawn patient-wise and this dataset file carries no patient information')
        mu = std = None
        if scaling_from is None and ds.scaling_factors and None in ds.scaling_factors:
            chans = ds.windows.shape[2]
            mu, std = (np.ravel(v)[:chans] for v in ds.scaling_factors[None])
        return cls(ds.windows, patients, mu, std, device=device, scaling_from=scaling_from,
                   padded='padded_breath_by_breath' in str(ds.dataset_type), seed=seed)

    @classmethod
    def from_pickle(cls, path, device='cuda', scaling_from=None, seed=0):
        """A ``SiameseNetworkDataset`` pickle (``all_sequences`` entries ``[patient_id, array]``), read through
        ``ingest.parse_pickle``: nothing is unpickled.  A .npz export or an ``ARDSRawDataset`` pickle goes through
        ``from_dataset``."""
        from . import ingest
        if str(path).endswith('.npz'):
            return cls.from_dataset(ingest.load_npz(path), device=device, scaling_from=scaling_from, seed=seed)
        with open(path, 'rb') as f:
            root = ingest.parse_pickle(f.read())
        st = ingest._state_dict(root)
        seqs = st.get('all_sequences')
        if not isinstance(seqs, list) or not seqs:
            raise ValueError('the dataset holds no sequences')
        if len(list(seqs[0])) != 2:
            return cls.from_dataset(ingest.dataset_from_tree(root), device=device, scaling_from=scaling_from, seed=seed)
        if ingest._plain(st.get('total_kfolds')) is not None:
            raise ValueError('the siamese dataset is not meant to be run with k-folds (dataset.py:1597)')
        patients, windows = [], []
        for seq in seqs:
            pt, data = list(seq)
            patients.append(ingest._plain(pt))
            windows.append(np.asarray(ingest.resolve(data), dtype=np.float64))
        mu = std = None
        sf = st.get('scaling_factors')
        if scaling_from is None and isinstance(sf, dict):
            for k, v in sf.items():
                if ingest._plain(k) is None:
                    mu, std = ingest._channel_scalars(v[0]), ingest._channel_scalars(v[1])
        return cls(np.stack(windows), np.asarray(patients), mu, std, device=device, scaling_from=scaling_from,
                   padded='padded_breath_by_breath' in str(ingest._plain(st.get('dataset_type', ''))), seed=seed)

    # ---- batches -------------------------------------------------------------------------------------------------------
    def anchors_on_device(self, idx):
        """Store indices (host list / tensor) checked against the store and uploaded once: slices go to ``triplet_batch``."""
        idx = torch.as_tensor(idx, dtype=torch.int64).reshape(-1)
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= len(self)):
            raise IndexError('window index out of range [0, %d)' % len(self))
        return idx.to(self.store.tiles.device).contiguous()

    def triplet_batch(self, anchor_idx, step=None, literal=True, out=None):
        """-> (windows ((4 or 3) B, NB, C, L) float32, index list int64): [anchor | pos | anchor | neg] (``literal``) or
        [anchor | pos | neg], normalised (and filtered) like every batch of a ``DeviceTileStore``.  One draw launch and one
        gather launch; nothing is read back.  ``anchor_idx``: host indices (checked here) or a contiguous int64 DEVICE tensor
        (``anchors_on_device``; the draw clamps whatever it is given into the store).  ``step``: the draw's counter -- default:
        the number of batches drawn so far; with the store's ``seed`` it fixes the negatives."""
        if not (isinstance(anchor_idx, torch.Tensor) and anchor_idx.is_cuda):
            anchor_idx = self.anchors_on_device(anchor_idx)
        if step is None:
            step = self.draws
        self.draws += 1
        idx = SO.siamese_draw(anchor_idx.contiguous(), self.pat_start, self.pat_count, self.seed, step, literal)
        return self.store._gather(idx, out), idx


class SiameseTrainer(SelfSupervisedTrainer):
    """One siamese network on one GPU.  ``train_step(batch)``: one iteration of SiameseMixin.run_train_epoch (:613-624) on the
    windows ``SiameseTileStore.triplet_batch(..., literal=not share_anchor)`` gathered -- eager, or a captured graph per input
    shape -- with the optimiser and clamp of ``HotPathTrainer``; returns the device-resident loss (``last_loss``; ``last_logits``
    is z (2, B, 2)).  ``test_step(batch)``: the body of run_test_epoch (:636-649) under ``model.eval()`` -> (loss (1,),
    accuracy (1,) of argmax(cat(z_pos, z_neg)) against B ones then B zeros, z (2, B, 2)), all on the device.

    ``share_anchor`` (see the module docstring) departs from the reference; the default does not.  The step scaffold -- the
    placeholder target, the refusals, forward/backward around ``_loss_and_output``, ``model.eval()`` in the test step and its
    refusal on running statistics -- is ``train.SelfSupervisedTrainer``; here is only what is siamese."""
    batch_alone = 'a siamese step takes the triplet batch alone'

    def __init__(self, model, share_anchor=False, optimizer='sgd', learning_rate=1e-3, weight_decay=1e-4, momentum=0.9,
                 clip_grad=True, clip_val=0.01, world_size=1, rank=0, process_group=None, use_graph=True, folds_in_flight=None):
        if not isinstance(model, _SiameseNetwork):
            raise TypeError('SiameseTrainer trains a siamese network, got %s' % type(model).__name__)
        super(SiameseTrainer, self).__init__(
            model, 'the siamese trainer runs on one GPU: the triplet draw and its batch are not sharded over %d ranks',
            'folds in flight with the siamese trainer: its dataset has no folds (dataset.py:1597)', world_size=world_size,
            folds_in_flight=folds_in_flight, optimizer=optimizer, learning_rate=learning_rate, weight_decay=weight_decay,
            momentum=momentum, clip_grad=clip_grad, clip_val=clip_val, use_graph=use_graph)
        self.share_anchor = bool(share_anchor)

    @property
    def windows_per_triplet(self):
        return 3 if self.share_anchor else 4

    def _check_batch(self, batch):
        k = self.windows_per_triplet
        if batch.dim() != 4 or batch.shape[0] == 0 or batch.shape[0] % k:
            raise ValueError('a %s-anchor step takes (%d B, NB, C, 224) windows, got %s' %
                             ('shared' if self.share_anchor else 'separate', k, tuple(batch.shape)))

    def _loss_and_output(self, inputs):
        return self.model.triplet_head(inputs, literal=not self.share_anchor)

    def _test_forward(self, inputs, target):
        loss, z = super(SiameseTrainer, self)._test_forward(inputs, target)
        b = z.shape[1]
        pred = z.argmax(dim=-1).reshape(-1)                                     # cat(z_pos, z_neg).argmax(1)  (:656-657)
        want = (torch.arange(2 * b, device=z.device) < b).to(pred.dtype)       # B ones, then B zeros         (:654-655)
        acc = (pred == want).to(torch.float32).mean().reshape(1)
        return loss, acc, z


def epoch_anchor_batches(store, batch_size, shuffle=True, generator=None):
    """One epoch's anchors: every window of the store once, in ``batch_size`` slices of ONE device tensor (a permutation
    when ``shuffle``)."""
    n = len(store)
    order = torch.randperm(n, generator=generator) if shuffle else torch.arange(n)
    dev = store.anchors_on_device(order)
    return [dev[s:s + batch_size] for s in range(0, n, batch_size)]


def run_siamese_train_epoch(trainer, store, batch_size=16, shuffle=True, generator=None):
    """Yields the (cloned, device-resident) loss of every batch.  Each batch is a draw launch, a gather launch -- into the
    captured step's own input buffer once there is one -- and the step."""
    literal = not trainer.share_anchor
    k = trainer.windows_per_triplet
    for anchors in epoch_anchor_batches(store, batch_size, shuffle, generator):
        static = trainer.static_batch(k * anchors.numel())
        batch, _ = store.triplet_batch(anchors, literal=literal, out=None if static is None else static[0])
        yield trainer.train_step(batch).clone()


def run_siamese_test_epoch(trainer, store, batch_size=16, shuffle=True, generator=None):
    """Yields (loss (1,), accuracy (1,)) of every batch, on the device."""
    literal = not trainer.share_anchor
    for anchors in epoch_anchor_batches(store, batch_size, shuffle, generator):
        batch, _ = store.triplet_batch(anchors, literal=literal)
        loss, acc, _ = trainer.test_step(batch)
        yield loss.clone(), acc.clone()


def build_parser():
    """The driver's parser with this stage's own ``-n`` choices (and ``--share-anchor``)."""
    from . import train_ards_detector as T
    parser = T.build_parser()
    parser.prog = 'deepards_amd.siamese'
    for action in parser._actions:
        if action.dest == 'network':
            action.choices = list(SIAMESE_NETWORKS)
    parser.add_argument('--share-anchor', action='store_true', default=None,
                        help='run the anchor once per triplet (3 B windows a step instead of 4 B): one dropout mask and one '
                             'running-statistics update for it -- a departure from the reference')
    return parser


def main(argv=None):
    """``python -m deepards_amd.siamese -n siamese_cnn_linear|siamese_cnn_lstm|siamese_cnn_transformer <the driver's flags>``."""
    from . import train_ards_detector as T
    return T.stage_main(argv, build_parser(), SIAMESE_NETWORKS, T.siamese_network_map, dict(T.BUILD_DEFAULTS, share_anchor=None))


if __name__ == '__main__':
    main()
