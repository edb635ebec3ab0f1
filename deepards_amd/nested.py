"""Whole-patient batches for the nested networks (models/nested.py): one item is ALL windows of one patient.

The reference builds such items with ``whole_patient_super_batch=True`` (dataset.py:1021-1081: every finished window of a
patient is appended to ``super_batch_tmp_arr`` and the patient becomes one ``[patient, (W, NB, 1, L), target, hours]`` entry).
``PatientSequenceStore.from_windows`` takes any prepared WINDOW dataset instead -- an ``ARDSRawDataset`` pickle or its .npz, as
``ingest`` reads them, or a pickle the reference wrote whole-patient (``ingest`` reads its items back as windows) -- and groups
the windows by patient in dataset order, which is exactly what that accumulation yields.  ``item(p)`` is ONE launch of the
tile store's gather over the patient's windows, so normalisation, the ``padded`` rule and the frequency filters are those of
``DeviceTileStore`` because it is that launch.

Departure: the reference's super-batch path keeps only the hours of a patient's LAST window (``batch_seq_hours`` is reset per
window, the entry gets what is left); here every window keeps its own (``hours(p)`` (W, NB)).

Refused, as the reference does or because nothing is built for it: ``oversample_minority`` (dataset.py:443), ``*_with_bm``
dataset types (:1084-1085), breath-level datasets, more than one input channel (the nested models take flow only).
"""
import sys

import numpy as np
import torch


def group_by_patient(patient_slot):
    """patient_slot (N,) -> list of index arrays, one per patient in order of first appearance, a patient's windows in dataset
    order."""
    slot = np.asarray(patient_slot)
    if slot.ndim != 1:
        raise ValueError('one patient slot per window expected')
    groups, seen = [], {}
    for i, p in enumerate(slot.tolist()):
        if p not in seen:
            seen[p] = len(groups)
            groups.append([])
        groups[seen[p]].append(i)
    return [np.asarray(g, dtype=np.int64) for g in groups]


class PatientSequenceStore(object):
    """Patients of a window store: ``len`` patients, ``item(p)`` -> (x (W_p, NB, 1, L) float32, target (1, 2)) on the device.
    ``store`` is the DeviceTileStore the windows live in (``set_filters`` / ``padded`` / the scaling factors are its own);
    ``select(patients)`` restricts the store to a fold's patients without touching the tiles."""

    def __init__(self, store, patient_slot, hours=None, oversample_minority=False):
        if oversample_minority:
            raise NotImplementedError('currently oversampling with whole patient super batch does not work')     # dataset.py:443
        if store.tiles.shape[2] != 1:
            raise NotImplementedError('the nested networks take one input channel (flow), this dataset has %d'
                                      % store.tiles.shape[2])
        slot = np.asarray(patient_slot, dtype=np.int64)
        if slot.shape != (store.tiles.shape[0],):
            raise ValueError('one patient slot per window expected')
        self.store = store
        self.patient_slot = slot
        self.groups = group_by_patient(slot)
        self.patient_ids = [int(slot[g[0]]) for g in self.groups]
        labels = self._labels = store.targets.argmax(dim=1).cpu().numpy()
        for g in self.groups:
            if len(set(labels[g].tolist())) != 1:
                raise ValueError('patient slot %d has windows of both classes: a patient is one item with one target'
                                 % int(slot[g[0]]))
        self._hours = None if hours is None else np.asarray(hours, dtype=np.float64)
        self.selected = list(range(len(self.groups)))

    @classmethod
    def from_windows(cls, dataset, device='cuda', oversample_minority=False, random_kfold=False):
        """``dataset``: an ``ingest.IngestedDataset`` or the path of a dataset file (``ingest.load_dataset``).  A k-fold
        dataset keeps its patient splits and per-fold scaling factors: ``set_kfold_indexes_for_fold`` selects a fold."""
        from . import ingest
        ds = ingest.load_dataset(dataset) if isinstance(dataset, str) else dataset
        check_dataset(ds)
        if oversample_minority:
            raise NotImplementedError('currently oversampling with whole patient super batch does not work')
        ps = cls(ds.to_store(device=device, random_kfold=random_kfold), ds.patient_slot, ds.hours)
        ps.train = bool(ds.train)
        return ps

    train = True

    # ---- k-folds: patients are split as DeviceTileStore.enable_kfolds splits them ---------------------------------------
    def make_test_store_if_kfold(self):
        """The same windows and splits serving each fold's TEST patients (``make_test_dataset_if_kfold``, dataset.py:672-700);
        the scaling factors stay the fold's TRAIN factors: both views read the one store."""
        if self.store.total_kfolds is None:
            raise ValueError('the dataset has no folds')
        other = object.__new__(PatientSequenceStore)
        other.__dict__.update(self.__dict__)
        other.train, other.selected = False, list(self.selected)
        return other

    def set_kfold_indexes_for_fold(self, kfold_num):
        st = self.store
        if st.total_kfolds is None:
            raise ValueError('the dataset has no folds')
        st.kfold_num = kfold_num
        st.mu, st.std = st.scaling_factors[kfold_num]
        self.select(st.kfold_patient_splits[kfold_num]['train' if self.train else 'test'])

    def __len__(self):
        return len(self.selected)

    def select(self, patient_ids=None):
        """Serve only the patients whose slot is in ``patient_ids`` (None: all), in dataset order."""
        keep = None if patient_ids is None else set(int(p) for p in np.asarray(patient_ids).tolist())
        self.selected = [i for i, p in enumerate(self.patient_ids) if keep is None or p in keep]
        return self

    def windows(self, p):
        """W_p of the p-th selected patient."""
        return int(len(self.groups[self.selected[p]]))

    def indices(self, p):
        return self.groups[self.selected[p]]

    def hours(self, p):
        """(W_p, NB) hours of every window of the patient (NaN where the dataset has none)."""
        idx = self.indices(p)
        if self._hours is None:
            return np.full((len(idx), int(self.store.tiles.shape[1])), np.nan)
        return self._hours[idx]

    def target_label(self, p):
        return int(self._labels[self.indices(p)[0]])

    def item(self, p):
        """(x (W_p, NB, 1, L) float32, target (1, 2)): ONE gather launch over the patient's windows."""
        from .models.nested import check_windows
        idx = self.indices(p)
        check_windows(len(idx), int(self.store.tiles.shape[1]), 'patient slot %d' % int(self.patient_slot[idx[0]]))
        x, t = self.store.batch_absolute(torch.from_numpy(idx))
        return x, t[:1].contiguous()


def check_dataset(ds):
    """The refusals that depend on the dataset file alone, each with its reason."""
    if getattr(ds, 'breath_level', False):
        raise NotImplementedError('a breath-level dataset (%s) has no windows to make a patient sequence of' % ds.dataset_type)
    if 'with_bm' in str(ds.dataset_type) or ds.metadata is not None:
        raise NotImplementedError('whole-patient batches of a %s dataset are refused: the reference refuses '
                                  'whole_patient_super_batch with *_with_bm dataset types (dataset.py:1084-1085)' % ds.dataset_type)
    if ds.windows.shape[2] != 1:
        raise NotImplementedError('the nested networks take one input channel (flow), this dataset has %d' % ds.windows.shape[2])
    if ds.patient_slot is None:
        raise ValueError('whole-patient batches are patient-wise and this dataset file carries no patient information')


def run_nested_train_epoch(trainer, patients, batch_size=1, shuffle=True, generator=None):
    """One step per patient (B = 1, T = W_p), yielding each step's loss (a device tensor) -- the train epoch iterator of the
    driver classes.  ``batch_size`` is what the driver hands every iterator; an item is one patient, so it must be 1."""
    if batch_size != 1:
        raise ValueError('the nested networks take one patient per step (batch size 1), got %r' % (batch_size,))
    n = len(patients)
    order = torch.randperm(n, generator=generator).tolist() if shuffle else list(range(n))
    for p in order:
        x, t = patients.item(p)
        yield trainer.train_step(x.unsqueeze(0), t).clone()


def run_nested_test_epoch(trainer, patients):
    """``BaseTraining.run_test_epoch`` for the nested networks: train-mode modules under no_grad, one patient per step; every
    window's argmax (NestedMixin._process_test_batch_results) is a vote for its patient (``transform_obs_idx`` repeats the
    item's index over the W outputs) -- reduced on the device by the vote kernel.  -> the result dict of
    ``train.test_epoch_steps.result`` (votes (P_all, 2) by patient slot, prediction, window_pred, window_abs_index, mean_loss)
    plus ``patients``, the slots that were served."""
    from . import hip_ops as H
    dev = patients.store.tiles.device
    n_pat = int(patients.patient_slot.max()) + 1
    votes = torch.zeros((n_pat, 2), dtype=torch.int32, device=dev)
    slot = torch.from_numpy(patients.patient_slot).to(dev)
    preds, losses, absolute = [], [], []
    for p in range(len(patients)):
        idx = torch.from_numpy(patients.indices(p)).to(dev)
        x, t = patients.item(p)
        loss, logits, _ = trainer.test_step(x.unsqueeze(0), t)
        preds.append(H.vote_counts(logits.reshape(-1, 2).contiguous(), slot[idx].contiguous(), votes))
        losses.append(loss.reshape(1))
        absolute.append(idx)
    v = votes.cpu().numpy()
    tot = v.sum(axis=1)
    cat = lambda ts, dt: torch.cat(ts).cpu().numpy() if ts else np.zeros(0, dtype=dt)
    return dict(votes=v, pred_frac=v[:, 1] / tot.clip(min=1), prediction=v.argmax(axis=1), window_pred=cat(preds, np.int32),
                window_index=cat(absolute, np.int64), window_abs_index=cat(absolute, np.int64),
                mean_loss=float(torch.cat(losses).mean()) if losses else float('nan'),
                patients=np.asarray([patients.patient_ids[i] for i in patients.selected], dtype=np.int64))


# ---- command line -----------------------------------------------------------------------------------------------------------
NESTED_NETWORKS = ('cnn_to_nested_rnn', 'cnn_to_nested_lstm')


def build_parser():
    """The driver's parser with this stage's own ``-n`` choices and ``--graph``."""
    from . import train_ards_detector as T
    parser = T.build_parser()
    parser.prog = 'deepards_amd.nested'
    for action in parser._actions:
        if action.dest == 'network':
            action.choices = list(NESTED_NETWORKS) + ['cnn_to_nested_transformer']
    parser.add_argument('--graph', dest='nested_graph', action='store_true', default=None,
                        help='capture the step per number of windows W and replay it (default: eager, because W changes from '
                             'patient to patient; only worth it when W values repeat)')
    return parser


def main(argv=None):
    """``python -m deepards_amd.nested -n cnn_to_nested_rnn|cnn_to_nested_lstm --base-network densenet18 --cuda-no-dp -p <dataset>
    [--test-from-pickle ..] [--kfolds K] [-lc all_breaths|last_breath] [--save-model f.pth]``; the batch size is forced to 1."""
    from . import train_ards_detector as T
    from .models.nested import TRANSFORMER_REFUSAL
    args = list(sys.argv[1:] if argv is None else argv)
    for i, a in enumerate(args):
        if (a in ('-n', '--network') and args[i + 1:i + 2] == ['cnn_to_nested_transformer']) or \
                a == '--network=cnn_to_nested_transformer':
            raise SystemExit(TRANSFORMER_REFUSAL)
    return T.stage_main(args, build_parser(), NESTED_NETWORKS, T.nested_network_map, dict(T.BUILD_DEFAULTS, nested_graph=None))


if __name__ == '__main__':
    main()
