"""Host mirror of the reference training driver for the cnn_linear path: same command line, configuration merge,
class / method / argument names as ``deepards/train_ards_detector.py`` (``build_parser`` / ``main`` :1439-1590,
``network_map`` :1410-1436, ``base_networks`` :45-69, ``BaseTraining`` :73-512, ``PatientClassifierMixin`` :514-537,
``CNNLinearModel`` :925-939, values of ``defaults.yml``), so that

    python -m deepards_amd.train_ards_detector -co experiment_files/unpadded_centered_nb20_cnn_linear.yml \\
           --train-from-pickle <dataset.pkl | dataset.npz> [--base-network resnet18] ...

or, from Python,

    cls = network_map[args.network](args)        # train_ards_detector.py:1589-1590
    cls.train_and_test()

runs the hot path on MI355X.  What differs, and why:

* the dataset objects are :class:`deepards_amd.data.DeviceTileStore` (windows resident in HBM) instead of
  ``ARDSRawDataset`` + ``DataLoader``; a "loader" is ``(store, batch_size, shuffle)``.  ``--train-from-pickle`` /
  ``--test-from-pickle`` take the reference's dataset pickle -- read WITHOUT unpickling by ``deepards_amd.ingest`` -- or
  the ``.npz`` that module exports; callers may also hand stores in (``args.train_store`` / ``args.test_store``).
  Building a dataset from raw ventilator files (``-dp``) needs ventmap / the cohort tree and is out of scope;
* ``get_optimizer`` returns a :class:`deepards_amd.train.HotPathTrainer`: the clamp hooks of ``get_model`` (:474-476),
  SGD-Nesterov / Adam (:416-422) and ``zero_grad`` are one fused kernel at the end of the captured step, so
  ``handle_train_optimization`` is a single ``train_step``;
* multi-GPU is one process per GPU under ``torch.distributed`` (launch with ``python -m torch.distributed.run``), not
  ``nn.DataParallel`` (:96): every rank takes its window shard of each batch (``deepards_amd.train``);
* results: the loss meters and the per-patient vote aggregation of ``DeepARDSResults`` (metrics.py:142-153,572-604) are
  kept on the device and read back once per epoch (``self.results`` is a small dict-of-lists recorder, not the
  reference's reporting / plotting class, which is out of scope).

There is no CPU path: constructing a model class with neither ``--cuda`` nor ``--cuda-no-dp`` raises.
"""
import argparse
import contextlib
import os

import torch

from . import models as M
from .config import Configuration
from .train import HotPathTrainer, run_test_epoch, run_train_epoch_from_store, test_epoch_steps

base_networks = M.base_networks
saved_models_default_dir = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'saved_models')

# Knobs this build adds below defaults.yml (the reference has none of them) + the store_true switches of build_parser,
# which must not live in defaults.yml (defaults.yml:9) and read as off / None when nobody set them.
BUILD_DEFAULTS = dict(
    train_store=None, test_store=None, test_patient_slot=None, use_graph=True, seed=None, conv_dtype=None, act_dtype=None,
    cuda=None, cuda_no_dp=None, no_print_progress=None, print_progress=None, no_test_after_epochs=None, debug=None,
    save_model_per_epoch=None, no_train=None, resnet_double_conv=None, bm_to_linear=None, unshuffled=None,
    oversample_minority=None, reshuffle_oversample_per_epoch=None, freeze_base_network=None, stop_on_loss=None,
    clip_grad=None, with_fft=None, only_fft=None, fft_real_only=None, random_kfold=None, bootstrap=None,
    kfolds=None, only_fold=None, load_checkpoint=None, load_base_network=None, save_model=None, saved_models_dir=None,
    train_from_pickle=None, train_to_pickle=None, test_from_pickle=None, test_to_pickle=None,
    experiment_name='deepards_amd', config_override=None, folds_in_flight=None, fold_groups=None, transformer_blocks=2,
    use_l1=None, average_linear_layer=None, share_anchor=None, nested_graph=None,
)

# make_args(): the merged view with every reference default, for callers that build ``args`` in Python
DEFAULTS = dict(
    network='cnn_linear', epochs=10, batch_size=16, base_network='densenet18', loader_threads=0,
    initial_planes=64, resnet_first_pool_type='max', resnet_double_conv=False,
    optimizer='sgd', dataset_type='unpadded_centered_sequences', learning_rate=0.001, n_sub_batches=20,
    weight_decay=0.0001, loss_func='bce', valpha=float('inf'), conf_beta=1.0, loss_calc='all_breaths', bm_to_linear=False,
    clip_grad=False, clip_val=0.01, time_series_hidden_units=16, transformer_blocks=2,
    with_fft=False, only_fft=False, fft_real_only=False, freeze_base_network=False,
    kfolds=None, bootstrap=False, random_kfold=False, only_fold=None, unshuffled=False, no_train=False,
    no_test_after_epochs=False, debug=False, cuda=True, cuda_no_dp=False, cuda_device=0, load_checkpoint=None,
    load_base_network=None, save_model=None, save_model_per_epoch=False, saved_models_dir=None,
    no_print_progress=True, print_progress=False, experiment_name='deepards_amd',
    oversample_minority=False, oversample_all_factor=1.0, reshuffle_oversample_per_epoch=False,
    undersample_factor=-1, train_pt_frac=1.0, train_from_pickle=None, test_from_pickle=None, train_to_pickle=None,
    test_to_pickle=None, stop_on_loss=False, stop_thresh=1.5, stop_after_epoch=1,
    train_store=None, test_store=None, test_patient_slot=None, use_graph=True, seed=None, conv_dtype=None, act_dtype=None,
    butter_low=None, butter_high=None, fft_filtering_low=None, fft_filtering_high=None, post_hoc_downsampling=None,
    n_warm_epochs=3, push_start_epoch=6, push_every_n=6, n_push_iters=5, clust_lambda=0.8, sep_lambda=0.2, n_prototypes=10,
    incorrect_strength=-0.5, use_l1=False, average_linear_layer=False, folds_in_flight=None, share_anchor=False,
    nested_graph=False,
)


def make_args(**overrides):
    """An ``args`` namespace with the reference's attribute names (``Configuration`` of config.py merges CLI,
    overrides file and defaults.yml the same way: later wins)."""
    unknown = set(overrides) - set(DEFAULTS)
    if unknown:
        raise TypeError('unknown arguments: %s' % sorted(unknown))
    d = dict(DEFAULTS)
    d.update(overrides)
    return argparse.Namespace(**d)


class Results(object):
    """The slice of ``DeepARDSResults`` the training loop writes: named meters per fold and the patient vote tables."""

    def __init__(self):
        self.meters = {}
        self.patient_results = {}

    def update_meter(self, name, fold_num, value):
        self.meters.setdefault((name, fold_num), []).append(value)

    def get_meter(self, name, fold_num):
        vals = self.meters.get((name, fold_num), [])
        return [float(v) for v in vals]                       # host sync only when somebody looks


def _flag(args, name, default=False):
    v = getattr(args, name, default)
    return default if v is None else v


def _one_gpu_one_fold_at_a_time(args, one_gpu, no_folds):
    """The refusal of the families whose trainer is neither sharded over ranks nor run with folds in flight (ProtoPNet, the
    siamese and the autoencoder stage), each with its own two reasons; the fold loop then runs the folds one after the other."""
    if int(os.environ.get('WORLD_SIZE', '1')) > 1:
        raise NotImplementedError(one_gpu)
    n_flight = getattr(args, 'folds_in_flight', None)
    if n_flight is not None and int(n_flight) > 1:
        raise NotImplementedError(no_folds)
    args.folds_in_flight = 1


class BaseTraining(object):
    clip_odd_batches = False
    per_breath_outputs = False            # (B, NB, 2) outputs: PerBreathClassifierMixin
    eval_in_test_epoch = False            # only CNNLSTMModel calls model.eval() in its test epoch (:861)
    carries_lstm_state = False

    def __init__(self, args):
        self.args = args
        from .train import check_loss_choice              # (before anything touches the device)
        check_loss_choice(args.loss_func, self.per_breath_outputs and self._loss_calc() == 'all_breaths')
        legacy = getattr(args, 'oversample', None)
        if legacy is not None:
            args.oversample_minority = legacy             # older configuration files say `oversample` (:80-83)
        if not (_flag(args, 'cuda') or _flag(args, 'cuda_no_dp')):
            raise RuntimeError('deepards_amd runs the hot path on an MI355X only: pass --cuda or --cuda-no-dp (no CPU fallback)')
        if not torch.cuda.is_available():
            raise RuntimeError('no HIP device visible; there is no CPU fallback')
        self.device = torch.device('cuda', args.cuda_device if _flag(args, 'cuda_no_dp') else torch.cuda.current_device())
        self.cuda_wrapper = lambda x: x.to(self.device)
        self.model_cuda_wrapper = lambda x: x.to(self.device)   # one process per GPU; nn.DataParallel (:96) is not used
        self.set_loss_criterion()
        self.n_metadata_inputs = 9 if args.dataset_type == 'padded_breath_by_breath_with_flow_time_features' else 0
        if _flag(args, 'unshuffled') and args.batch_size > 1:
            raise Exception('Currently we can only run unshuffled runs with a batch size of 1!')
        if _flag(args, 'bootstrap'):
            raise NotImplementedError('--bootstrap (80/20 patient resampling, dataset.py:792-807) is outside the hot path')
        if _flag(args, 'stop_on_loss'):
            raise NotImplementedError('--stop-on-loss drops into an interactive shell in the reference (:155-157)')
        self.n_kfolds = args.kfolds if args.kfolds else 1
        self._prev_dtypes = None
        if _flag(args, 'conv_dtype', None):
            from . import functional as F_
            # the arithmetic / storage switches are process-wide: remember what was set so that restore_dtypes() (called
            # when train_and_test finishes, and by evaluate.main) leaves a later run in this process what it had before
            self._prev_dtypes = (F_.conv_dtype(), F_.storage_dtype())
            F_.set_conv_dtype(args.conv_dtype)
            # BASELINE's bf16 configs: bf16 storage too where the network has bf16 kernels throughout (the ResNets)
            if args.conv_dtype == 'bf16' and getattr(M.backbone_class(args.base_network), 'bf16_storage', False) and \
                    getattr(args, 'act_dtype', None) != 'f32':
                F_.set_storage_dtype('bf16')
        self.results = Results()
        self.preds, self.pred_idx = [], []

    # ---- model / optimizer ---------------------------------------------------------------------------------------
    def _base_network_kwargs(self):
        a = self.args
        return dict(resnet_kwargs=dict(initial_planes=a.initial_planes, first_pool_type=a.resnet_first_pool_type,
                                       double_conv_first=_flag(a, 'resnet_double_conv')),
                    densenet_kwargs=dict(with_fft=_flag(a, 'with_fft'), only_fft=_flag(a, 'only_fft'),
                                         fft_real_only=_flag(a, 'fft_real_only')),
                    base_network=a.base_network)

    def get_base_network(self):
        """:380-414 for the backbones this package builds.  ``--load-base-network`` takes the ``breath_block`` of a
        saved model -- a whole module pickled by this package, by the reference (read without unpickling) or a
        state_dict (``deepards_amd.checkpoint``).

        A deliberate deviation: ``se_*`` and ``vgg*`` names are built with NO keyword arguments.  The reference's driver falls
        into its DenseNet branch for them (:409-414) and passes ``with_fft`` / ``only_fft`` / ``fft_real_only`` to
        ``se_resnet18()`` / ``VGG.__init__``, which take none and raise ``TypeError`` -- although its experiment scripts sweep
        those networks.  Here the network those scripts ask for is built."""
        a = self.args
        kw = self._base_network_kwargs()
        if a.load_base_network:
            from .checkpoint import load_base_network
            base_network = load_base_network(a.load_base_network, base_networks, kw)
        else:
            base_network = M.build_base_network(a.base_network, kw)
        if _flag(a, 'freeze_base_network'):
            for p in base_network.parameters():
                p.requires_grad = False
        return base_network

    def get_model(self):
        """:467-477.  The +-clip_val clamp the reference registers as a hook on every trainable parameter is applied by
        the fused optimizer kernel of the trainer ``get_optimizer`` returns (after the gradient all-reduce when data
        parallel), so no hooks are registered here.  Under data parallelism the replicas are made identical by the
        trainer's rank-0 broadcast before the first update, whatever each rank's seed was."""
        if self.args.load_checkpoint:
            from .checkpoint import load_model_weights
            model = load_model_weights(self.args.load_checkpoint, lambda: self.get_network(self.get_base_network()))
        else:
            if self.args.seed is not None:
                torch.manual_seed(self.args.seed)
            model = self.get_network(self.get_base_network())
        return self.model_cuda_wrapper(model)

    def get_optimizer(self, model, world_size=1, rank=0, process_group=None):
        """:416-422: Adam(lr) or SGD(lr, momentum .9, weight_decay, nesterov) + the clamp of get_model, as the trainer
        that owns the captured step."""
        return HotPathTrainer(model, **self._trainer_kwargs(world_size, rank, process_group), **self._loss_kwargs())

    def _trainer_kwargs(self, world_size, rank, process_group):
        """The keywords every family's trainer takes from the command line (its own ``get_optimizer`` adds the rest)."""
        a = self.args
        if a.optimizer not in ('adam', 'sgd'):
            raise ValueError('optimizer must be adam or sgd')
        return dict(optimizer=a.optimizer, learning_rate=a.learning_rate, weight_decay=a.weight_decay,
                    clip_grad=bool(_flag(a, 'clip_grad')), clip_val=a.clip_val, world_size=world_size, rank=rank,
                    process_group=process_group, use_graph=_flag(a, 'use_graph', True))

    def _loss_kwargs(self):
        """What set_loss_criterion chose, as the trainer's keywords (the criterion runs inside its captured step)."""
        a = self.args
        param = {'bce': None, 'vacillating': getattr(a, 'valpha', None), 'confidence': getattr(a, 'conf_beta', None)}[a.loss_func]
        return dict(loss=a.loss_func, loss_param=param, loss_calc=self._loss_calc(), eval_test=self.eval_in_test_epoch,
                    carry_state=self.carries_lstm_state and bool(_flag(a, 'unshuffled')))

    def _loss_calc(self):
        return 'all_breaths'              # only CNNLSTMModel.calc_loss reads --loss-calc (:815-821)

    # ---- data ----------------------------------------------------------------------------------------------------
    def get_base_datasets(self):
        """:189-315 for prepared datasets: stores handed in by the caller, or ``--train-from-pickle`` (+ optional
        ``--test-from-pickle``) read by ``deepards_amd.ingest`` (the reference's pickle, parsed without executing it, or
        its .npz export).  K-fold runs take the test patients of each fold from the train dataset
        (``make_test_dataset_if_kfold`` :272-273); a holdout test pickle gets the TRAIN set's scaling factors (:285)."""
        a = self.args
        if a.train_store is not None and a.test_store is not None:
            if any(v is not None for v in self._filter_kwargs().values()):
                a.train_store.set_filters(**self._filter_kwargs())    # (all None: stores handed in keep what they carry)
                a.test_store.set_filters(**self._filter_kwargs())
            return a.train_store, a.test_store
        if not a.train_from_pickle:
            raise ValueError('no dataset: pass --train-from-pickle <dataset.pkl|.npz> (or args.train_store / args.test_store); '
                             'building one from raw ventilator files (--data-path) is outside the accelerated path')
        from .ingest import load_dataset
        fft = dict(add_fft=bool(_flag(a, 'with_fft')), only_fft=bool(_flag(a, 'only_fft')),
                   fft_real_only=bool(_flag(a, 'fft_real_only')))
        ds = load_dataset(a.train_from_pickle).with_fft(**fft)            # dataset.py:743-762
        if a.kfolds is not None and ds.total_kfolds is None:
            ds.total_kfolds = a.kfolds                            # an unfolded pickle split now (:126-133 reads args.kfolds)
        ds.train = True
        train = ds.to_store(self.device, random_kfold=bool(_flag(a, 'random_kfold')))
        train.oversample_minority = bool(_flag(a, 'oversample_minority'))
        train.oversample_all_factor = float(getattr(a, 'oversample_all_factor', 1.0) or 1.0)
        train.undersample_factor = getattr(a, 'undersample_factor', -1)
        train.train_patient_fraction = getattr(a, 'train_pt_frac', 1.0)
        if a.seed is not None:
            import numpy as np
            train.sampling_rng = np.random.RandomState(a.seed)
        train.set_filters(**self._filter_kwargs())                # before the k-fold test store is made: it inherits them
        self.n_sub_batches = ds.n_sub_batches
        if a.train_to_pickle:
            ds.save_npz(a.train_to_pickle)
        if not a.test_from_pickle and a.kfolds is not None:
            test = train.make_test_store_if_kfold()
        elif a.test_from_pickle:
            tds = load_dataset(a.test_from_pickle).with_fft(**fft)
            tds.train = False
            test = tds.to_store(self.device)
            test.mu, test.std = train.mu, train.std               # test_dataset.scaling_factors = train_dataset's (:285)
            test.scaling_factors = train.scaling_factors
            test.set_filters(**self._filter_kwargs())             # the holdout test dataset gets the same keywords (:266-272)
            if a.test_to_pickle:
                tds.save_npz(a.test_to_pickle)
        else:
            raise ValueError('a holdout run needs --test-from-pickle (or --kfolds)')
        if a.test_patient_slot is None and test.patient_slot is not None:
            a.test_patient_slot = torch.as_tensor(test.patient_slot, dtype=torch.int64)
        return train, test

    def _filter_kwargs(self):
        """The four filter keys of the dataset constructors (:246-255); a key nobody set reads as None.  The fifth,
        post_hoc_downsampling, is passed on only when it is set."""
        kw = {k: getattr(self.args, k, None) for k in ('butter_low', 'butter_high', 'fft_filtering_low', 'fft_filtering_high')}
        if getattr(self.args, 'post_hoc_downsampling', None) is not None:
            kw['post_hoc_downsampling'] = self.args.post_hoc_downsampling
        return kw

    def get_splits(self):
        """:317-338: per fold, (train_dataset, train_loader, test_dataset, test_loader); a loader is the tuple
        (store, batch_size, shuffle) the epoch functions iterate on the device."""
        train_dataset, test_dataset = self.get_base_datasets()
        for i in range(self.n_kfolds):
            if self.args.kfolds is not None:
                self._seed_fold_sampler(train_dataset, i)
                for ds in (train_dataset, test_dataset):
                    if hasattr(ds, 'set_kfold_indexes_for_fold'):
                        ds.set_kfold_indexes_for_fold(i)
            shuffle = not _flag(self.args, 'unshuffled')
            yield (train_dataset, (train_dataset, self.args.batch_size, shuffle),
                   test_dataset, (test_dataset, self.args.batch_size, shuffle))

    def _seed_fold_sampler(self, store, fold_num):
        """Each fold's oversampling draws come from a generator of their own (seeded from --seed and the fold; numpy's
        global RNG without a seed, like the reference's RandomOverSampler()): a fold then draws the same windows
        whether the folds run one after the other or side by side (--folds-in-flight)."""
        if hasattr(store, 'sampling_rng') and self.args.seed is not None:
            import numpy as np
            store.sampling_rng = np.random.RandomState(self.args.seed + 7919 * (fold_num + 1))

    # ---- epochs --------------------------------------------------------------------------------------------------
    def run_train_epoch(self, model, train_loader, optimizer, epoch_num, fold_num):
        """:139-159.  ``optimizer`` is the trainer from get_optimizer; every batch is one gather kernel + one graph
        replay; the per-batch losses stay on the device until a meter is read.  The permutation comes from the seed when
        one is given; data-parallel ranks always shard ONE permutation (rank 0's seed is broadcast per epoch)."""
        if optimizer.model is not model:
            raise ValueError('optimizer was built for another model')
        for loss in self._train_losses(optimizer, train_loader, self._epoch_generator(fold_num, epoch_num)):
            self._book_train_loss(optimizer, loss, epoch_num, fold_num)
            if _flag(self.args, 'debug'):
                break

    def _train_epoch_iterator(self):
        """What yields an epoch's per-batch losses: the one piece of the train epoch a family replaces."""
        return run_train_epoch_from_store

    def _train_losses(self, optimizer, train_loader, generator):
        store, batch_size, shuffle = train_loader
        return self._train_epoch_iterator()(optimizer, store, batch_size=batch_size, shuffle=shuffle, generator=generator)

    def _book_train_loss(self, optimizer, loss, epoch_num, fold_num):
        self.results.update_meter('loss_epoch_{}'.format(epoch_num), fold_num, loss)
        self.results.update_meter('loss', fold_num, loss)

    def _epoch_generator(self, fold_num, epoch_num, offset=0):
        """The generator of one epoch's permutation: seeded from --seed, the fold and the epoch; ``offset`` keeps a test
        epoch (500009) and ProtoPNet's last-layer passes apart from the train epoch.  None without a seed."""
        if self.args.seed is None:
            return None
        return torch.Generator().manual_seed(self.args.seed + 1000 * fold_num + epoch_num + offset)

    @contextlib.contextmanager
    def _test_trainer(self, optimizer, make):
        """The trainer of a test epoch: the one given, or a throw-away ``make()`` whose graphs are freed on the way out, not
        in a GC pass."""
        if optimizer is not None:
            yield optimizer
        else:
            trainer = make()
            yield trainer
            trainer.release_graphs()

    def handle_train_optimization(self, optimizer, outputs, target, inputs, fold_num, total_batches, batch_idx,
                                  epoch_num, model):
        """:161-173.  loss + backward + clamp + step + zero_grad are one captured step; ``outputs`` (a forward the
        caller already ran) is not needed and ignored."""
        loss = optimizer.train_step(inputs, target)
        self.results.update_meter('loss_epoch_{}'.format(epoch_num), fold_num, loss.clone())
        return loss

    def run_test_epoch(self, epoch_num, model, test_dataset, test_loader, fold_num, optimizer=None, _steps_only=False):
        """:424-465 + record_final_epoch_testing_results (:519-524): no_grad forward with train-mode modules (the
        reference never calls eval()), loss meter, window argmax, per-patient votes -- reduced on the device."""
        store, batch_size, shuffle = test_loader
        with self._test_trainer(optimizer, lambda: HotPathTrainer(model, use_graph=_flag(self.args, 'use_graph', True),
                                                                  **self._loss_kwargs())) as trainer:
            trainer.clip_odd_batches = self.clip_odd_batches
            slot = self.args.test_patient_slot
            if slot is None:
                slot = torch.zeros(store.tiles.shape[0], dtype=torch.int64)
            # the test loader shuffles too unless --unshuffled (:333-338)
            gen = self._epoch_generator(fold_num, epoch_num, 500009) if shuffle else None
            steps = test_epoch_steps(trainer, store, slot, batch_size=batch_size, shuffle=shuffle, generator=gen)
            if _steps_only:                                   # folds in flight: the caller walks the steps of ITS trainer and finishes
                return steps
            for _ in steps:
                pass
        return self._finish_test_epoch(steps, epoch_num, fold_num)

    def _finish_test_epoch(self, steps, epoch_num, fold_num):
        res = steps.result()
        self.preds, self.pred_idx = res['window_pred'].tolist(), res['window_abs_index'].tolist()   # obs_idx is absolute
        self.results.update_meter('test_loss', fold_num, res['mean_loss'])
        self.results.patient_results[(fold_num, epoch_num)] = res
        return res

    def restore_dtypes(self):
        """Put back the process-wide conv arithmetic / activation storage this run replaced (--conv-dtype)."""
        if self._prev_dtypes is not None:
            from . import functional as F_
            conv, storage = self._prev_dtypes
            F_.set_conv_dtype(conv)
            if storage != F_.storage_dtype():
                F_.set_storage_dtype(storage)
            self._prev_dtypes = None

    def train_and_test(self):
        """:340-378 without plotting: fold loop, epoch loop, per-epoch / per-fold whole-module saves under the
        reference's file names (``deepards_amd.checkpoint.model_save_path``)."""
        try:
            return self._train_and_test()
        finally:
            self.restore_dtypes()

    def _train_and_test(self):
        from .checkpoint import model_save_path
        a = self.args
        saved_models_dir = a.saved_models_dir if getattr(a, 'saved_models_dir', None) else saved_models_default_dir
        n_flight = getattr(a, 'folds_in_flight', None)
        if n_flight is None:                             # default: up to 5 folds side by side on a single GPU (same results)
            n_flight = min(5, self.n_kfolds) if self._data_parallel()[0] == 1 else 1
        n_flight = int(n_flight)
        if self.carries_lstm_state and _flag(a, 'unshuffled'):
            # the carried-state epoch is one walk over the windows in order; the side-by-side fold loop interleaves its
            # own batches and does not hand over the per-patient flags
            if getattr(a, 'folds_in_flight', None) is not None and n_flight > 1:
                raise NotImplementedError('--folds-in-flight > 1 with cnn_lstm --unshuffled (the per-patient LSTM state carry): '
                                          'run the folds one after the other')
            n_flight = 1
        if n_flight > 1 and self.n_kfolds > 1 and a.kfolds is not None:
            return self._train_and_test_folds_in_flight(n_flight, saved_models_dir)
        my_folds = None
        n_groups = int(getattr(a, 'fold_groups', None) or 1)
        if n_groups > 1:
            # config C4: fold groups x data-parallel sub-groups (deepards_amd.train.fold_group_layout)
            if self._data_parallel()[0] == 1:
                raise ValueError('--fold-groups needs torch.distributed (python -m torch.distributed.run ...)')
            from .train import make_fold_groups
            group, gworld, grank, my_folds = make_fold_groups(n_groups, self.n_kfolds)
            self._dp_override = (gworld, grank, group)
        for fold_num, (train_dataset, train_loader, test_dataset, test_loader) in enumerate(self.get_splits()):
            if (a.only_fold and fold_num != a.only_fold) or (my_folds is not None and fold_num not in my_folds):
                continue
            model = self.get_model()
            optimizer = self.get_optimizer(model, *self._data_parallel())
            for epoch_num in range(1, a.epochs + 1):
                if not _flag(a, 'no_train'):
                    self.run_train_epoch(model, train_loader, optimizer, epoch_num, fold_num)
                if _flag(a, 'reshuffle_oversample_per_epoch'):
                    train_loader[0].set_oversampling_indices()                       # :350-351
                if not _flag(a, 'no_test_after_epochs') or epoch_num == a.epochs - 1:
                    self.run_test_epoch(epoch_num, model, test_dataset, test_loader, fold_num, optimizer=optimizer)
                if _flag(a, 'save_model_per_epoch'):
                    self._save(model, model_save_path(a.save_model, saved_models_dir, self.n_kfolds, fold_num, epoch_num))
            if a.save_model:
                self._save(model, model_save_path(a.save_model, saved_models_dir, self.n_kfolds, fold_num))
            optimizer.release_graphs()                   # this fold's captured steps go NOW, not in some later gc pass (the
            self.model, self.optimizer = model, optimizer    # trainer stays usable: it re-captures on its next step)
        if my_folds is not None:                         # every rank ends with every fold's patient results
            from .train import gather_fold_results
            self.results.patient_results = gather_fold_results(self.results.patient_results, self._data_parallel()[1] == 0)
        return self.results

    def _train_and_test_folds_in_flight(self, n_flight, saved_models_dir):
        """The fold loop of ``train_and_test`` with ``n_flight`` folds side by side on this GPU: every fold has its own
        view of the tile store (fold indices, scaling factors, oversampling draws), model, trainer (captured step) and
        HIP stream; the host walks the folds' batches round-robin, so the step kernels of different folds overlap on the
        chip (independent launches fill the ramp / drain / latency gaps a B <= 64 step leaves: +12 % aggregate at B = 64
        with two folds, +17 % at B = 16 with four, scripts/two_fold_probe.py).  Within a fold nothing changes -- same
        kernels in the same order on one stream -- so its losses, predictions and weights are those of the sequential
        loop bit for bit (tests/test_model_gpu.py)."""
        import copy
        from .checkpoint import model_save_path
        from .train import concurrent_streams, epoch_shards_on_device, place_replicas_on_streams, shared_generator
        a = self.args
        if self._data_parallel()[0] > 1:
            raise NotImplementedError('--folds-in-flight with data parallelism: give every rank group its own folds instead')
        train_dataset, test_dataset = self.get_base_datasets()
        folds = [f for f in range(self.n_kfolds) if not (a.only_fold and f != a.only_fold)]
        shuffle = not _flag(a, 'unshuffled')
        for g0 in range(0, len(folds), n_flight):
            ctx = []
            streams = concurrent_streams(len(folds[g0:g0 + n_flight]))     # on different hardware queues (measured)
            for fold_num in folds[g0:g0 + n_flight]:
                tr_ds, te_ds = copy.copy(train_dataset), copy.copy(test_dataset)
                self._seed_fold_sampler(tr_ds, fold_num)
                for ds in (tr_ds, te_ds):
                    ds.set_kfold_indexes_for_fold(fold_num)
                stream = streams[len(ctx)]
                with torch.cuda.stream(stream):
                    model = self.get_model()
                    optimizer = self.get_optimizer(model, 1, 0, None)
                ctx.append((fold_num, stream, model, optimizer, tr_ds, te_ds))
            torch.cuda.synchronize()
            placed = not _flag(a, 'use_graph', True)
            for epoch_num in range(1, a.epochs + 1):
                if not _flag(a, 'no_train'):
                    plans = []
                    for fold_num, stream, model, optimizer, tr_ds, te_ds in ctx:
                        gen = self._epoch_generator(fold_num, epoch_num)
                        if shuffle:
                            gen = shared_generator(optimizer, gen)
                        with torch.cuda.stream(stream):      # the index upload is ordered before the fold's gathers
                            plans.append(epoch_shards_on_device(tr_ds, a.batch_size, shuffle, gen, 1, 0))
                    for b in range(max(len(p) for p in plans)):
                        if not placed and all(c[3].static_batch() is not None for c in ctx) and len(ctx) > 1:
                            # every fold has its captured step: measure which streams let them overlap (restores all state)
                            streams = place_replicas_on_streams([c[3] for c in ctx])
                            ctx = [(c[0], s) + c[2:] for c, s in zip(ctx, streams)]
                            placed = True
                        for (fold_num, stream, model, optimizer, tr_ds, te_ds), plan in zip(ctx, plans):
                            if b >= len(plan) or (_flag(a, 'debug') and b > 0):
                                continue
                            idx = plan[b]
                            with torch.cuda.stream(stream):
                                static = optimizer.static_batch(len(idx))
                                x, t = tr_ds.batch_from_device(idx, out=static) if static is not None else tr_ds.batch_from_device(idx)
                                loss = optimizer.train_step(x, t).clone()
                            self.results.update_meter('loss_epoch_{}'.format(epoch_num), fold_num, loss)
                            self.results.update_meter('loss', fold_num, loss)
                    torch.cuda.synchronize()                 # the meters are read from the default stream
                for fold_num, stream, model, optimizer, tr_ds, te_ds in ctx:
                    if _flag(a, 'reshuffle_oversample_per_epoch'):
                        tr_ds.set_oversampling_indices()
                if not _flag(a, 'no_test_after_epochs') or epoch_num == a.epochs - 1:
                    walks = []                           # the folds' test epochs, one step of each in turn
                    for fold_num, stream, model, optimizer, tr_ds, te_ds in ctx:
                        with torch.cuda.stream(stream):
                            walks.append(self.run_test_epoch(epoch_num, model, te_ds, (te_ds, a.batch_size, shuffle), fold_num,
                                                             optimizer=optimizer, _steps_only=True))
                    live = list(range(len(ctx)))
                    while live:
                        for i in list(live):
                            with torch.cuda.stream(ctx[i][1]):
                                if next(walks[i], None) is None:
                                    live.remove(i)
                    torch.cuda.synchronize()
                    for (fold_num, stream, model, optimizer, tr_ds, te_ds), steps in zip(ctx, walks):
                        self._finish_test_epoch(steps, epoch_num, fold_num)
                for fold_num, stream, model, optimizer, tr_ds, te_ds in ctx:
                    if _flag(a, 'save_model_per_epoch'):
                        self._save(model, model_save_path(a.save_model, saved_models_dir, self.n_kfolds, fold_num, epoch_num))
            torch.cuda.synchronize()
            for fold_num, stream, model, optimizer, tr_ds, te_ds in ctx:
                if a.save_model:
                    self._save(model, model_save_path(a.save_model, saved_models_dir, self.n_kfolds, fold_num))
                self.model, self.optimizer = model, optimizer
            self.fold_models = getattr(self, 'fold_models', {})
            self.fold_models.update({c[0]: c[2] for c in ctx})
            for c in ctx:                                # the group's captured steps are released here, explicitly, before
                c[3].release_graphs()                    # the next group captures its own (ownership rule, train._capture_graph)
        if folds:                                        # like the sequential loop, leave the caller's stores at the last fold
            self._seed_fold_sampler(train_dataset, folds[-1])
            for ds in (train_dataset, test_dataset):
                ds.set_kfold_indexes_for_fold(folds[-1])
        return self.results

    def _save(self, model, path):
        """``torch.save(model, model_path)`` (:364,374): the whole module; under data parallelism the replicas' BatchNorm
        running statistics (updated from each rank's own shard) are averaged first, then rank 0 of the group writes."""
        world, rank, group = self._data_parallel()
        if world > 1:
            from .train import average_replica_buffers
            average_replica_buffers(model, world, group)
        if rank != 0:
            return
        os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
        # a trainer hangs its gradient destinations on the Parameters (``p._da_grad``: views into its flat bucket); pickled
        # along they would double the file and, in the loaded model, point functional._tgt at a dead buffer
        stash = [(q, q.__dict__.pop('_da_grad')) for q in model.parameters() if '_da_grad' in q.__dict__]
        try:
            torch.save(model, path)
        finally:
            for q, g in stash:
                q._da_grad = g

    _dp_override = None

    def _data_parallel(self):
        """(world_size, rank, group): one process per GPU under torch.distributed (RCCL) instead of nn.DataParallel (:96);
        every rank takes its window shard of each batch, gradients meet in one all-reduce (deepards_amd.train).  With
        --fold-groups the triple describes this rank's data-parallel SUB-group."""
        import torch.distributed as dist
        if self._dp_override is not None:
            return self._dp_override
        if dist.is_available() and dist.is_initialized():
            return dist.get_world_size(), dist.get_rank(), None
        return 1, 0, None

    def clip_odd_batch_sizes(self, obs_idx, seq, metadata, target):
        from .train import clip_odd_batch_sizes
        return clip_odd_batch_sizes(obs_idx, seq, metadata, target)

    def transform_obs_idx(self, obs_idx, outputs):
        return obs_idx


class PatientClassifierMixin(object):
    def set_loss_criterion(self):
        """:526-532: BCEWithLogitsLoss (mean over B*2), VacillatingLoss(valpha) or ConfidencePenaltyLoss(conf_beta) --
        ``da_bce_logits`` / ``da_vacillating_loss`` / ``da_confidence_loss``, inside the trainer's step too.  The
        vacillating loss on a network whose output is not (B, NB, 2) is refused here (train.check_loss_choice)."""
        from . import functional as F_
        from .train import check_loss_choice
        a = self.args
        check_loss_choice(a.loss_func, self.per_breath_outputs and self._loss_calc() == 'all_breaths')
        if a.loss_func == 'vacillating':
            self.criterion = F_.VacillatingLoss(float('inf') if getattr(a, 'valpha', None) is None else a.valpha)
        elif a.loss_func == 'confidence':
            self.criterion = F_.ConfidencePenaltyLoss(1.0 if getattr(a, 'conf_beta', None) is None else a.conf_beta)
        else:
            self.criterion = F_.bce_with_logits


class CNNLinearModel(BaseTraining, PatientClassifierMixin):
    def __init__(self, args):
        super(CNNLinearModel, self).__init__(args)

    def calc_loss(self, outputs, target, inputs):
        return self.criterion(outputs, target)

    def _process_test_batch_results(self, outputs, target, inputs, fold_num):
        return outputs.argmax(dim=-1).cpu().tolist()

    def get_network(self, base_network):
        return M.CNNLinearNetwork(base_network, self.args.n_sub_batches, self.n_metadata_inputs)


class CNNDoubleLinearModel(CNNLinearModel):
    def get_network(self, base_network):
        return M.CNNDoubleLinearNetwork(base_network, self.args.n_sub_batches, self.n_metadata_inputs)


class CNNLinearToMeanModel(CNNLinearModel):
    def get_network(self, base_network):
        return M.CNNLinearToMean(base_network)


class CNNLinearComprToRFModel(CNNLinearModel):
    def get_network(self, base_network):
        return M.CNNLinearComprToRF(base_network)


class PerBreathClassifierMixin(object):
    """:539-555: the window target repeated over the breaths for the loss (the trainer's step does that for (B, NB, 2)
    outputs), one prediction and one patient vote per breath."""
    per_breath_outputs = True

    def calc_loss(self, outputs, target, inputs):
        if self.args.batch_size > 1:
            target = target.unsqueeze(1)
        return self.criterion(outputs, target.repeat((1, outputs.shape[1], 1)))

    def _process_test_batch_results(self, outputs, target, inputs, fold_num):
        return outputs.argmax(dim=-1).cpu().view(-1).tolist()

    def transform_obs_idx(self, obs_idx, outputs):
        return obs_idx.reshape((outputs.shape[0], 1)).repeat((1, outputs.shape[1])).view(-1)


class CNNSingleBreathLinearModel(PerBreathClassifierMixin, BaseTraining, PatientClassifierMixin):
    def __init__(self, args):
        super(CNNSingleBreathLinearModel, self).__init__(args)

    def get_network(self, base_network):
        return M.CNNSingleBreathLinearNetwork(base_network)


class CNNLSTMModel(PerBreathClassifierMixin, BaseTraining, PatientClassifierMixin):
    """:809-883.  ``--unshuffled`` (batch size 1): the LSTM's (hx, cx) are carried from one window to the next, detached,
    and start from zeros when the patient changes, in the train and the test epoch -- on the device, inside the trainer's
    step (``HotPathTrainer(carry_state=True)``).  The test epoch runs under ``model.eval()`` (:861): with a DenseNet
    breath block that is dropout off and nothing else (its BatchNorm keeps no running statistics); with a ResNet it would
    be inference on running statistics, which this package does not have -- refused."""
    clip_odd_batches = True
    eval_in_test_epoch = True
    carries_lstm_state = True

    def __init__(self, args):
        if getattr(M.backbone_class(args.base_network), 'running_stats', False):
            raise NotImplementedError('cnn_lstm with a ResNet / VGG base network: its test epoch runs under model.eval() '
                                      '(train_ards_detector.py:861), i.e. BatchNorm inference on running statistics, which '
                                      'is not implemented here; use a DenseNet base network')
        if _flag(args, 'bm_to_linear'):
            raise NotImplementedError('--bm-to-linear (metadata into the linear layer) is outside the accelerated path')
        super(CNNLSTMModel, self).__init__(args)

    def _loss_calc(self):
        lc = getattr(self.args, 'loss_calc', None) or 'all_breaths'
        if lc not in ('all_breaths', 'last_breath'):
            raise ValueError('loss_calc must be all_breaths or last_breath, got %r' % (lc,))
        return lc

    def calc_loss(self, outputs, target, inputs):
        if self._loss_calc() == 'last_breath':
            return self.criterion(outputs[:, -1, :], target)
        return PerBreathClassifierMixin.calc_loss(self, outputs, target, inputs)

    def get_network(self, base_network):
        return M.CNNLSTMNetwork(base_network, self.n_metadata_inputs, bool(_flag(self.args, 'bm_to_linear')),
                                self.args.time_series_hidden_units)


class CNNTransformerModel(PerBreathClassifierMixin, BaseTraining, PatientClassifierMixin):
    """:801-806.  Its test epoch is ``BaseTraining.run_test_epoch`` (no ``model.eval()``, :448): train-mode modules under
    no_grad, so both dropouts stay on and BatchNorm uses batch statistics -- ResNet and DenseNet bases alike.  NOT in
    ``network_map`` yet (README.md, "Networks"): build it directly, ``CNNTransformerModel(args).train_and_test()``."""
    eval_in_test_epoch = False

    def __init__(self, args):
        if _flag(args, 'bm_to_linear'):
            raise NotImplementedError('--bm-to-linear (metadata into the linear layer) is outside the accelerated path')
        super(CNNTransformerModel, self).__init__(args)

    def get_network(self, base_network):
        blocks = getattr(self.args, 'transformer_blocks', None)
        return M.CNNTransformerNetwork(base_network, self.n_metadata_inputs, bool(_flag(self.args, 'bm_to_linear')),
                                       self.args.time_series_hidden_units, 2 if blocks is None else blocks)


class ProtoPNetModel(object):
    """:1156-1371 for the trainer of ``deepards_amd.protopnet``: ``get_optimizer`` returns ONE ProtoPNetTrainer that holds the
    reference's three optimisers as phases (warm / joint / last layer), ``calc_loss`` is the loss kernel, ``run_train_epoch``
    carries the epoch schedule (:1255-1329) and the push.  Never clips (the reference's loops do not call the base class's
    clipping, although the experiment files set clip_grad).  One GPU, the folds one after the other."""

    def get_optimizer(self, model, world_size=1, rank=0, process_group=None):
        from .protopnet import ProtoPNetTrainer
        a = self.args
        kw = dict(self._trainer_kwargs(world_size, rank, process_group), clip_grad=False)      # never clips (the class docstring)
        return ProtoPNetTrainer(model, clust_lambda=a.clust_lambda, sep_lambda=a.sep_lambda, use_l1=bool(_flag(a, 'use_l1')), **kw)

    def calc_loss(self, model, cls_output, target, min_distances):
        """-> loss, cls_loss, cluster_cost, separation_cost, l1 (:1194-1247), one launch (+ the l1 term with --use-l1)."""
        from . import protopnet_ops as PO
        w = mask = None
        if _flag(self.args, 'use_l1'):
            w = model.last_layer.weight
            mask = (1 - torch.t(model.prototype_class_identity_linear_layer)).to(w.device)
        nb = min_distances.shape[1] // model.num_prototypes
        parts = PO.ppnet_loss(cls_output.detach().contiguous(), target.contiguous(), min_distances.detach().contiguous(), nb,
                              model.num_prototypes, self.max_dist, self.args.clust_lambda, self.args.sep_lambda,
                              want_grad=False, l1_weight=w, l1_mask=mask)[0]
        return tuple(parts[i] for i in range(5))

    def _process_test_batch_results(self, outputs, target, inputs, fold_num):
        return outputs.argmax(dim=-1).cpu().tolist()

    def run_train_epoch(self, model, train_loader, optimizer, epoch_num, fold_num):
        """:1255-1329: the warm optimiser while epoch_num <= n_warm_epochs, the joint one after; from push_start_epoch on,
        every push_every_n epochs, the push and n_push_iters last-layer passes over the training set."""
        a = self.args
        optimizer.set_phase('warm' if epoch_num <= a.n_warm_epochs else 'joint')
        BaseTraining.run_train_epoch(self, model, train_loader, optimizer, epoch_num, fold_num)
        if epoch_num >= a.push_start_epoch and (epoch_num - a.push_start_epoch) % a.push_every_n == 0:
            self.push_func(train_loader, model, epoch_num)
            optimizer.set_phase('last_layer')
            for it in range(a.n_push_iters):
                for loss in self._train_losses(optimizer, train_loader, self._epoch_generator(fold_num, epoch_num, 100003 * (it + 1))):
                    self.results.update_meter('loss', fold_num, loss)
                if _flag(a, 'debug'):
                    break

    def _book_train_loss(self, optimizer, loss, epoch_num, fold_num):
        parts = optimizer.last_parts.clone()                  # (the captured step's own buffer: the next replay refills it)
        for i, name in ((1, 'cls_loss'), (2, 'clst_loss'), (3, 'sep_loss'), (4, 'l1_loss')):
            self.results.update_meter(name, fold_num, parts[i])
        BaseTraining._book_train_loss(self, optimizer, loss, epoch_num, fold_num)

    def run_test_epoch(self, epoch_num, model, test_dataset, test_loader, fold_num, optimizer=None, _steps_only=False):
        """:1331-1349: under model.eval(), the loss kernel, softmaxed outputs; the votes as in BaseTraining.run_test_epoch."""
        with self._test_trainer(optimizer, lambda: self.get_optimizer(model)) as trainer:
            return BaseTraining.run_test_epoch(self, epoch_num, model, test_dataset, test_loader, fold_num, optimizer=trainer,
                                               _steps_only=_steps_only)


class ProtoPNet1DModel(ProtoPNetModel, BaseTraining, PatientClassifierMixin):
    """:1374-1391.  NOT in ``network_map`` (its key set is pinned, as for cnn_transformer; README.md, "Networks"): build it
    directly, ``ProtoPNet1DModel(args).train_and_test()``.  The base network must be one of this package's DenseNets."""

    def __init__(self, args):
        if M.backbone_class(args.base_network) is not M.DenseNet:
            raise NotImplementedError('protopnet needs a DenseNet base network (forward_no_pool exists only there), got %r'
                                      % (args.base_network,))
        _one_gpu_one_fold_at_a_time(
            args, 'protopnet runs on one GPU: its phases and the push are not sharded over ranks',
            '--folds-in-flight > 1 with protopnet: the phase schedule and the push walk one fold at a time; run the folds one '
            'after the other')
        super(ProtoPNet1DModel, self).__init__(args)

    def get_network(self, base_network):
        a = self.args
        model = M.construct_PPNet(base_network, sub_batch_size=a.n_sub_batches, prototype_shape=(a.n_prototypes * 2, 128, 1),
                                  batch_size=a.batch_size, incorrect_strength=a.incorrect_strength,
                                  average_linear=bool(_flag(a, 'average_linear_layer')))
        self.max_dist = model.prototype_shape[1] * model.prototype_shape[2]
        return model

    def push_func(self, train_loader, model, epoch_num):
        from .protopnet import push_prototypes
        store, batch_size, _ = train_loader
        self.last_push = push_prototypes(model, store, batch_size=batch_size)
        return self.last_push


class LSTMOnlyModel(BaseTraining, PatientClassifierMixin):
    """:1024-1040.  The network reads the raw waveform with an LSTM and has no CNN: no base network is built
    (``get_base_network`` is not called, ``--base-network`` is ignored), so ``--load-base-network`` and
    ``--freeze-base-network`` have nothing to act on and are refused.  Window-level (B, 2) outputs; the test epoch is
    ``BaseTraining.run_test_epoch`` (no ``model.eval()``).  NOT in ``network_map`` (its key set is pinned, as for
    cnn_transformer; README.md, "Networks"): build it directly, ``LSTMOnlyModel(args).train_and_test()``."""
    clip_odd_batches = True

    def __init__(self, args):
        for flag in ('load_base_network', 'freeze_base_network'):
            if _flag(args, flag, None):
                raise ValueError('--%s with %s: the network has no base network (the LSTM reads the raw waveform), so there '
                                 'is nothing to load into or freeze' % (flag.replace('_', '-'), type(self).__name__))
        super(LSTMOnlyModel, self).__init__(args)

    def calc_loss(self, outputs, target, inputs):
        return self.criterion(outputs, target)

    def _process_test_batch_results(self, outputs, target, inputs, fold_num):
        return outputs.argmax(dim=-1).cpu().tolist()

    def get_base_network(self):
        raise RuntimeError('%s has no base network' % type(self).__name__)

    def get_model(self):
        """BaseTraining.get_model without a base network: ``get_network(None)``."""
        if self.args.load_checkpoint:
            from .checkpoint import load_model_weights
            model = load_model_weights(self.args.load_checkpoint, lambda: self.get_network(None))
        else:
            if self.args.seed is not None:
                torch.manual_seed(self.args.seed)
            model = self.get_network(None)
        return self.model_cuda_wrapper(model)

    def _hidden_units(self):
        h = getattr(self.args, 'time_series_hidden_units', None)
        return 16 if h is None else h

    def get_network(self, _):
        return M.LSTMOnlyNetwork(self._hidden_units(), self.args.n_sub_batches)


class LSTMOnlyWithPackingModel(LSTMOnlyModel):
    """:1043-1059: LSTMOnlyModel on padded breath-by-breath datasets, whose padding is exactly 0.0."""

    def get_network(self, _):
        return M.LSTMOnlyWithPacking(self._hidden_units(), self.args.n_sub_batches)


class MeterSummaryMixin(object):
    """``perform_post_modeling_actions`` of the pretraining stages (SiameseMixin, RegressorMixin)."""

    def perform_post_modeling_actions(self):
        """:576-577 / :676-677 save the results object; here: the meters' means, returned and kept as ``self.summary``."""
        self.summary = {}
        for (name, fold), vals in self.results.meters.items():
            host = [float(v.detach()) if isinstance(v, torch.Tensor) else float(v) for v in vals]
            self.summary['%s/%s' % (name, fold)] = sum(host) / len(host) if host else None
        return self.summary


class SiameseMixin(MeterSummaryMixin):
    """:558-658 for the trainer of ``deepards_amd.siamese``: the datasets are ``SiameseTileStore`` s (``--train-from-pickle`` /
    ``--test-from-pickle``: a SiameseNetworkDataset pickle, read without unpickling, or any prepared ARDSRawDataset pickle /
    .npz; or stores handed in as ``args.train_store`` / ``args.test_store``), ``get_optimizer`` returns a ``SiameseTrainer``,
    the train epoch draws and gathers every triplet batch on the device, the test epoch (under ``model.eval()``, :635) fills the
    ``accuracy`` and ``test_loss`` meters per fold and per epoch (``accuracy_epoch_<n>`` / ``test_loss_epoch_<n>``).

    With a base network whose BatchNorm keeps running statistics (ResNet, SE-ResNet, VGG) ``model.eval()`` would mean
    inference on them, which this package does not have: such a run TRAINS, prints one notice and skips its test epochs.
    No k-folds (the reference's dataset is not meant for them), one GPU, no folds in flight.  ``--share-anchor`` runs the
    anchor once per triplet -- a departure, see ``deepards_amd.siamese``."""

    def __init__(self, args):
        if getattr(args, 'kfolds', None):
            raise ValueError('siamese pretraining is not meant to be run with k-folds (dataset.py:1597): triplets are drawn over '
                             'the whole training set')
        _one_gpu_one_fold_at_a_time(
            args, 'siamese pretraining runs on one GPU: the triplet draw and its batch are not sharded over ranks',
            '--folds-in-flight > 1 with siamese pretraining: its dataset has no folds')
        self._test_skipped = False
        super(SiameseMixin, self).__init__(args)

    def set_loss_criterion(self):
        from . import functional as F_
        self.criterion = F_.bce_with_logits

    def calc_loss(self, outputs_pos, outputs_neg):
        """:564-571 on logits somebody already has (the trainer's step computes the same sum inside the head kernel)."""
        t_pos = torch.tensor([[0.0, 1.0]], device=outputs_pos.device).repeat((outputs_pos.shape[0], 1))
        t_neg = torch.tensor([[1.0, 0.0]], device=outputs_neg.device).repeat((outputs_neg.shape[0], 1))
        return self.criterion(outputs_pos, t_pos) + self.criterion(outputs_neg, t_neg)

    def _process_test_batch_results(self, outputs_pos, outputs_neg):
        preds = torch.cat([outputs_pos, outputs_neg], dim=0).argmax(dim=1).cpu().numpy()
        return preds, [1] * outputs_pos.shape[0] + [0] * outputs_pos.shape[0]

    def record_testing_results(self, accuracy, epoch_num, fold_num):
        self.results.update_meter('accuracy', fold_num, accuracy)
        self.results.update_meter('accuracy_epoch_{}'.format(epoch_num), fold_num, accuracy)

    def get_base_datasets(self):
        from .siamese import SiameseTileStore
        a = self.args
        seed = 0 if a.seed is None else int(a.seed)
        if a.train_store is not None:
            train, test = a.train_store, a.test_store
        else:
            if not a.train_from_pickle:
                raise ValueError('no dataset: pass --train-from-pickle <dataset.pkl|.npz> (or args.train_store / args.test_store); '
                                 'building one from raw ventilator files (--data-path) is outside the accelerated path')
            train = SiameseTileStore.from_pickle(a.train_from_pickle, device=self.device, seed=seed)
            # test_dataset.scaling_factors = train_dataset.scaling_factors (:605)
            test = SiameseTileStore.from_pickle(a.test_from_pickle, device=self.device, scaling_from=train, seed=seed + 1) \
                if a.test_from_pickle else None
        if not isinstance(train, SiameseTileStore) or not (test is None or isinstance(test, SiameseTileStore)):
            raise TypeError('siamese pretraining takes SiameseTileStore datasets')
        if any(v is not None for v in self._filter_kwargs().values()) or a.train_store is None:
            for ds in (train, test):
                if ds is not None:
                    ds.set_filters(**self._filter_kwargs())
        self.n_sub_batches = train.n_sub_batches
        return train, test

    def get_optimizer(self, model, world_size=1, rank=0, process_group=None):
        from .siamese import SiameseTrainer
        return SiameseTrainer(model, share_anchor=bool(_flag(self.args, 'share_anchor')),
                              **self._trainer_kwargs(world_size, rank, process_group))

    def _train_epoch_iterator(self):
        from .siamese import run_siamese_train_epoch
        return run_siamese_train_epoch

    def run_test_epoch(self, epoch_num, model, test_dataset, test_loader, fold_num, optimizer=None, _steps_only=False):
        from .siamese import run_siamese_test_epoch
        why = None
        if test_dataset is None:
            why = 'no test dataset was given (--test-from-pickle)'
        elif getattr(model.breath_block, 'running_stats', False):
            why = ('the siamese test epoch runs under model.eval() (train_ards_detector.py:635); with a %s base network that is '
                   'BatchNorm inference on running statistics, which this package does not have'
                   % type(model.breath_block).__name__)
        if why is not None:
            if not self._test_skipped:
                print('siamese: the test epochs are skipped -- %s; training is not affected' % why)
                self._test_skipped = True
            return None
        store, batch_size, shuffle = test_loader
        with self._test_trainer(optimizer, lambda: self.get_optimizer(model)) as trainer:
            for loss, acc in run_siamese_test_epoch(trainer, store, batch_size=batch_size, shuffle=shuffle,
                                                    generator=self._epoch_generator(fold_num, epoch_num, 500009)):
                self.results.update_meter('test_loss', fold_num, loss)
                self.results.update_meter('test_loss_epoch_{}'.format(epoch_num), fold_num, loss)
                self.record_testing_results(acc, epoch_num, fold_num)
        return {'accuracy': self.results.get_meter('accuracy_epoch_{}'.format(epoch_num), fold_num),
                'test_loss': self.results.get_meter('test_loss_epoch_{}'.format(epoch_num), fold_num)}


class SiameseCNNLinearModel(SiameseMixin, BaseTraining):
    """:1137-1142.  NOT in ``network_map`` (its key set is pinned, as for cnn_transformer): reached through
    ``python -m deepards_amd.siamese -n siamese_cnn_linear`` (``siamese_network_map``) or built directly."""

    def get_network(self, base_network):
        return M.SiameseCNNLinearNetwork(base_network, self.n_sub_batches)


class SiameseCNNLSTMModel(SiameseMixin, BaseTraining):
    """:1119-1126.  NOT in ``network_map`` (pinned key set): ``python -m deepards_amd.siamese -n siamese_cnn_lstm``."""

    def get_network(self, base_network):
        return M.SiameseCNNLSTMNetwork(base_network, self.args.time_series_hidden_units, self.n_sub_batches)


class SiameseCNNTransformerModel(SiameseMixin, BaseTraining):
    """:1129-1134.  NOT in ``network_map`` (pinned key set): ``python -m deepards_amd.siamese -n siamese_cnn_transformer``."""

    def get_network(self, base_network):
        return M.SiameseCNNTransformerNetwork(base_network, self.args.time_series_hidden_units, self.n_sub_batches)


siamese_network_map = {
    'siamese_cnn_linear': SiameseCNNLinearModel,
    'siamese_cnn_lstm': SiameseCNNLSTMModel,
    'siamese_cnn_transformer': SiameseCNNTransformerModel,
}

def regression_scores(target, preds):
    """(mean_absolute_error, r2_score, mean_squared_error) of sklearn.metrics with ``multioutput='uniform_average'`` for
    (n_samples, n_outputs) arrays, in float64 numpy: the errors are averaged over the samples per output column, then over
    the columns; r2 per column is 1 - SS_res / SS_tot, and a constant column scores 1 when it is matched exactly, else 0
    (sklearn's ``force_finite``).  What the reference's RegressorMixin (:661-677) books as ``test_mae``, ``r2`` and ``test_mse``
    per test batch, without importing sklearn (``RegressorMixin.record_testing_results`` below)."""
    import numpy as np
    t, p = np.asarray(target, dtype=np.float64), np.asarray(preds, dtype=np.float64)
    if t.ndim == 1:
        t, p = t[:, None], p[:, None]
    if t.shape != p.shape or t.ndim != 2 or t.shape[0] < 1:
        raise ValueError('regression_scores: (n_samples, n_outputs) arrays of one shape expected, got %s and %s' % (t.shape, p.shape))
    mae = float(np.mean(np.mean(np.abs(t - p), axis=0)))
    mse = float(np.mean(np.mean((t - p) ** 2, axis=0)))
    num = np.sum((t - p) ** 2, axis=0)
    den = np.sum((t - np.mean(t, axis=0)) ** 2, axis=0)
    ok = den != 0
    r2 = np.ones(t.shape[1])
    r2[ok] = 1.0 - num[ok] / den[ok]
    r2[~ok & (num != 0)] = 0.0
    return mae, float(np.mean(r2)), mse


class RegressorMixin(MeterSummaryMixin):
    """:661-677: a test batch's (n_samples, n_outputs) targets and predictions booked as ``test_mae``, ``r2`` and ``test_mse``."""

    def record_testing_results(self, target, batch_preds, fold_num):
        mae, r2, mse = regression_scores(target, batch_preds)
        self.results.update_meter('test_mae', fold_num, mae)
        self.results.update_meter('r2', fold_num, r2)
        self.results.update_meter('test_mse', fold_num, mse)

    def record_final_epoch_testing_results(self, fold_num, epoch_num, test_dataset):
        return self.results.get_meter('test_mae', fold_num)

    def set_loss_criterion(self):
        self.criterion = torch.nn.MSELoss()        # (for calc_loss on tensors somebody already has; the step computes it in-kernel)


class AutoencoderModel(BaseTraining, RegressorMixin):
    """:1102-1116.  NOT in ``network_map`` (its key set is pinned): reached through ``python -m deepards_amd.autoencoder -n
    autoencoder`` (``autoencoder_network_map``) or built directly.  The network is ``AutoencoderNetwork(UNet(1))`` for
    ``--base-network unet`` and ``AutoencoderNetwork(AutoencoderCNN())`` for every other value (the reference's ``basic_cnn_ae``); any
    prepared dataset serves, its targets are ignored.
    ``get_optimizer`` returns an ``AutoencoderTrainer``; the test epoch runs under ``model.eval()`` and books ``test_loss``,
    ``test_mae``, ``r2`` and ``test_mse`` per batch.  One GPU, no folds in flight (BatchNorm over the whole batch is a different
    function when the batch is split); ``--load-base-network`` / ``--freeze-base-network`` are refused: they belong to the second
    stage -- a classifier on the pretrained encoder -- which is not built."""

    def __init__(self, args):
        if getattr(args, 'load_base_network', None):
            raise NotImplementedError('--load-base-network with -n autoencoder: the network is always a fresh AutoencoderCNN / UNet; a saved '
                                      'autoencoder resumes through --load-checkpoint, and a classifier\'s breath_block has no '
                                      'decoder to load')
        if _flag(args, 'freeze_base_network'):
            raise NotImplementedError('--freeze-base-network with -n autoencoder: the base network IS the model being pretrained; '
                                      'freezing it leaves nothing to train')
        unet = getattr(args, 'base_network', None) == 'unet'
        if unet:
            one_gpu = 'autoencoder pretraining with --base-network unet runs on one GPU: the sharded step is not built and was not run'
        else:
            one_gpu = ('autoencoder pretraining runs on one GPU: its BatchNorm takes its statistics over the whole batch, which a '
                       'batch sharded over ranks changes')
        _one_gpu_one_fold_at_a_time(args, one_gpu, '--folds-in-flight > 1 with -n autoencoder: %s' %
                                    ('not built and not run for the UNet' if unet else 'the folds run one after the other'))
        super(AutoencoderModel, self).__init__(args)

    def _process_test_batch_results(self, outputs, target, inputs, fold_num):
        batch_preds = outputs.detach().cpu().numpy().squeeze(1)
        target = inputs.reshape(inputs.shape[0] * inputs.shape[1], inputs.shape[2], inputs.shape[3]).squeeze(1).cpu().numpy()
        self.record_testing_results(target, batch_preds, fold_num)
        return batch_preds.tolist()

    def calc_loss(self, outputs, target, inputs):
        return self.criterion(outputs, inputs.reshape(inputs.shape[0] * inputs.shape[1], inputs.shape[2], inputs.shape[3]))

    def get_base_network(self):
        return M.UNet(1) if self.args.base_network == 'unet' else M.AutoencoderCNN()

    def get_network(self, base_network):
        return M.AutoencoderNetwork(base_network)

    def get_model(self):
        if self.args.load_checkpoint:
            from .checkpoint import load_autoencoder
            return self.model_cuda_wrapper(load_autoencoder(self.args.load_checkpoint))
        return super(AutoencoderModel, self).get_model()

    def get_optimizer(self, model, world_size=1, rank=0, process_group=None):
        from .autoencoder import AutoencoderTrainer
        return AutoencoderTrainer(model, **self._trainer_kwargs(world_size, rank, process_group))

    def _train_epoch_iterator(self):
        from .autoencoder import run_autoencoder_train_epoch
        return run_autoencoder_train_epoch

    def run_test_epoch(self, epoch_num, model, test_dataset, test_loader, fold_num, optimizer=None, _steps_only=False):
        from .autoencoder import run_autoencoder_test_epoch
        store, batch_size, shuffle = test_loader
        self.preds = []
        with self._test_trainer(optimizer, lambda: self.get_optimizer(model)) as trainer:
            for x, recon, loss in run_autoencoder_test_epoch(trainer, store, batch_size=batch_size, shuffle=shuffle,
                                                             generator=self._epoch_generator(fold_num, epoch_num, 500009)):
                self.results.update_meter('test_loss', fold_num, loss)
                self.preds += self._process_test_batch_results(recon, None, x, fold_num)
        return {k: self.results.get_meter(k, fold_num) for k in ('test_mae', 'r2', 'test_mse')}


autoencoder_network_map = {'autoencoder': AutoencoderModel}


class CNNRegressorModel(BaseTraining, RegressorMixin):
    """:1081-1099.  NOT in ``network_map`` (its key set is pinned): reached through ``python -m deepards_amd.regressor -n
    cnn_regressor`` (``regressor_network_map``) or built directly.  The datasets are ``BreathMetaStore`` s (``--train-from-pickle`` /
    ``--test-from-pickle``: a ``*_bm_target`` pickle, read without unpickling, its .npz, or a window dataset with per-breath
    metadata; or stores handed in as ``args.train_store`` / ``args.test_store``).  ``n_bm_features`` comes from the dataset type
    (3 / 7 / 9), for a window dataset from the width of its metadata.  ``get_optimizer`` returns a ``RegressorTrainer``; the test
    epoch is ``BaseTraining.run_test_epoch`` (:424-465: train-mode modules under ``no_grad``, no ``model.eval()``) and books
    ``test_loss``, ``test_mae``, ``r2`` and ``test_mse`` per batch.  One GPU, no folds in flight, no k-folds;
    ``--load-base-network`` is accepted (the generic path), ``--freeze-base-network`` is not."""

    def __init__(self, args):
        from .regressor import BM_TARGET_TYPES
        if getattr(args, 'kfolds', None):
            raise ValueError('--kfolds with -n cnn_regressor: the breath-metadata dataset has no class to stratify patients by '
                             '(its target slot holds [nan])')
        if _flag(args, 'freeze_base_network'):
            raise NotImplementedError('--freeze-base-network with -n cnn_regressor: the base network is what is being pretrained')
        if getattr(args, 'loss_func', None) not in (None, 'bce'):          # ('bce' is what defaults.yml merges in for "unset")
            raise ValueError('-loss %s with -n cnn_regressor: the regressor\'s loss is MSELoss (train_ards_detector.py:674), '
                             'there is no choice' % args.loss_func)
        if getattr(args, 'conv_dtype', None) not in (None, 'f32') or getattr(args, 'act_dtype', None) == 'bf16':
            raise NotImplementedError('--conv-dtype %s / --act-dtype %s with -n cnn_regressor: the regression head reads float '
                                      'maps only' % (getattr(args, 'conv_dtype', None), getattr(args, 'act_dtype', None)))
        _one_gpu_one_fold_at_a_time(
            args, 'breath-metadata pretraining runs on one GPU: BatchNorm takes its statistics over the whole batch, which a '
                  'batch sharded over ranks changes',
            '--folds-in-flight > 1 with -n cnn_regressor: its dataset has no folds')
        if args.dataset_type in BM_TARGET_TYPES:
            self.n_bm_features = BM_TARGET_TYPES[args.dataset_type]
        if getattr(args, 'loss_func', None) is None:
            args.loss_func = 'bce'                         # (BaseTraining checks the name; set_loss_criterion below ignores it)
        super(CNNRegressorModel, self).__init__(args)

    def calc_loss(self, outputs, target, inputs):
        return self.criterion(outputs, target)

    def _process_test_batch_results(self, outputs, target, inputs, fold_num):
        batch_preds = outputs.cpu().numpy()
        target = target.cpu()
        self.record_testing_results(target, batch_preds, fold_num)
        return batch_preds.tolist()

    def get_network(self, base_network):
        try:
            self.n_bm_features
        except AttributeError:
            raise Exception('You have specified cnn regressor without specifying which dataset you want to use. Do so with the '
                            '-dt flag')
        return M.CNNRegressor(base_network, self.n_bm_features)

    def get_base_datasets(self):
        from .regressor import BM_TARGET_TYPES, BreathMetaStore
        a = self.args
        if a.train_store is not None:
            train, test = a.train_store, a.test_store
        else:
            if not a.train_from_pickle:
                raise ValueError('no dataset: pass --train-from-pickle <dataset.pkl|.npz> (or args.train_store / args.test_store); '
                                 'building one from raw ventilator files (--data-path) is outside the accelerated path')
            train = BreathMetaStore.from_pickle(a.train_from_pickle, device=self.device)
            # test_dataset.scaling_factors = train_dataset.scaling_factors (:285)
            test = BreathMetaStore.from_pickle(a.test_from_pickle, device=self.device, scaling_from=train) \
                if a.test_from_pickle else None
        if not isinstance(train, BreathMetaStore) or not (test is None or isinstance(test, BreathMetaStore)):
            raise TypeError('breath-metadata pretraining takes BreathMetaStore datasets')
        for ds, name in ((train, 'train'), (test, 'test')):
            if ds is None:
                continue
            want = BM_TARGET_TYPES.get(a.dataset_type)
            if want is not None and ds.n_targets != want:
                raise ValueError('-dt %s means %d breath-metadata targets, the %s dataset has %d' %
                                 (a.dataset_type, want, name, ds.n_targets))
            if ds.n_targets != train.n_targets:
                raise ValueError('the test dataset has %d targets, the train dataset %d' % (ds.n_targets, train.n_targets))
        if a.dataset_type not in BM_TARGET_TYPES and train.dataset_type not in BM_TARGET_TYPES:
            self.n_bm_features = train.n_targets           # a window dataset's metadata (BreathMetaStore.from_windows)
        if any(v is not None for v in self._filter_kwargs().values()) or a.train_store is None:
            for ds in (train, test):
                if ds is not None:
                    ds.set_filters(**self._filter_kwargs())
        return train, test

    def get_optimizer(self, model, world_size=1, rank=0, process_group=None):
        from .regressor import RegressorTrainer
        return RegressorTrainer(model, **self._trainer_kwargs(world_size, rank, process_group))

    def _train_epoch_iterator(self):
        from .regressor import run_regressor_train_epoch
        return run_regressor_train_epoch

    def run_test_epoch(self, epoch_num, model, test_dataset, test_loader, fold_num, optimizer=None, _steps_only=False):
        from .regressor import run_regressor_test_epoch
        if test_dataset is None:
            return None
        store, batch_size, shuffle = test_loader
        self.preds = []
        with self._test_trainer(optimizer, lambda: self.get_optimizer(model)) as trainer:
            for target, out, loss in run_regressor_test_epoch(trainer, store, batch_size=batch_size, shuffle=shuffle,
                                                              generator=self._epoch_generator(fold_num, epoch_num, 500009)):
                self.results.update_meter('test_loss', fold_num, loss)
                self.preds += self._process_test_batch_results(out, target, None, fold_num)
        return {k: self.results.get_meter(k, fold_num) for k in ('test_mae', 'r2', 'test_mse')}


regressor_network_map = {'cnn_regressor': CNNRegressorModel}


class NestedMixin(object):
    """:680-769 for the nested networks (``deepards_amd.models.nested``): one item is a whole patient.  The datasets are
    ``nested.PatientSequenceStore`` s over any prepared window dataset (``--train-from-pickle`` / ``--test-from-pickle``, or stores
    handed in as ``args.train_store`` / ``args.test_store``); k-folds split patients as the window path does; a step is one patient
    (``args.batch_size`` is forced to 1, :774,785); ``calc_loss`` is BCE on every window or on the last (``--loss-calc``,
    :750-755); the test epoch runs train-mode modules under no_grad and every window's argmax votes for its patient
    (``_process_test_batch_results`` / ``transform_obs_idx``, :684-687,764-765) through the ``Results`` path of the other
    classifiers.  The step runs EAGERLY unless ``nested_graph`` (``--graph``) is set: W changes from patient to patient and
    a captured step is kept per W; ``use_graph`` is not read.  One GPU, the folds one after the other."""
    per_breath_outputs = True

    def _init_nested(self, args):
        args.batch_size = 1
        if args.loss_func != 'bce':
            raise ValueError('the nested networks train with BCEWithLogitsLoss only (NestedMixin.set_loss_criterion fixes it, '
                             'train_ards_detector.py:681-682): -loss %s is refused' % args.loss_func)
        legacy = getattr(args, 'oversample', None)
        if _flag(args, 'oversample_minority') or legacy:
            raise NotImplementedError('currently oversampling with whole patient super batch does not work')     # dataset.py:443
        _one_gpu_one_fold_at_a_time(
            args, 'the nested networks on more than one GPU: not built, not run (a step is one patient on one GPU)',
            '--folds-in-flight > 1 with the nested networks: not built, not run (the folds run one after the other)')

    def set_loss_criterion(self):
        from . import functional as F_
        self.criterion = F_.bce_with_logits

    def _loss_calc(self):
        lc = getattr(self.args, 'loss_calc', None) or 'all_breaths'
        if lc not in ('all_breaths', 'last_breath'):
            raise ValueError('loss_calc must be all_breaths or last_breath, got %r' % (lc,))
        return lc

    def calc_loss(self, outputs, target, inputs):
        if self._loss_calc() == 'all_breaths':
            return self.criterion(outputs, target.reshape(-1, 1, 2).repeat((1, outputs.shape[1], 1)))
        return self.criterion(outputs[:, -1], target)

    def _process_test_batch_results(self, outputs, target, inputs, fold_num):
        return outputs.argmax(dim=-1).cpu().view(-1).tolist()

    def transform_obs_idx(self, obs_idx, outputs):
        return obs_idx.reshape((outputs.shape[0], 1)).repeat((1, outputs.shape[1])).view(-1)

    def get_base_datasets(self):
        from .nested import PatientSequenceStore
        from .ingest import load_dataset
        a = self.args
        if a.train_store is not None:
            train, test = a.train_store, a.test_store
        else:
            if not a.train_from_pickle:
                raise ValueError('no dataset: pass --train-from-pickle <dataset.pkl|.npz> (or args.train_store / args.test_store); '
                                 'building whole-patient datasets from raw ventilator files is outside the accelerated path')
            ds = load_dataset(a.train_from_pickle)
            if a.kfolds is not None and ds.total_kfolds is None:
                ds.total_kfolds = a.kfolds
            ds.train = True
            train = PatientSequenceStore.from_windows(ds, device=self.device, random_kfold=bool(_flag(a, 'random_kfold')))
            train.store.set_filters(**self._filter_kwargs())
            if a.test_from_pickle:
                tds = load_dataset(a.test_from_pickle)
                tds.train, tds.total_kfolds = False, None
                test = PatientSequenceStore.from_windows(tds, device=self.device)
                test.store.mu, test.store.std = train.store.mu, train.store.std          # the TRAIN set's factors (:285)
                test.store.set_filters(**self._filter_kwargs())
            elif a.kfolds is not None:
                test = train.make_test_store_if_kfold()
            else:
                raise ValueError('a holdout run needs --test-from-pickle (or --kfolds)')
        if not isinstance(train, PatientSequenceStore) or not isinstance(test, PatientSequenceStore):
            raise TypeError('the nested networks take PatientSequenceStore datasets')
        self.n_sub_batches = int(train.store.tiles.shape[1])
        return train, test

    def get_optimizer(self, model, world_size=1, rank=0, process_group=None):
        kw = self._trainer_kwargs(world_size, rank, process_group)
        kw['use_graph'] = bool(_flag(self.args, 'nested_graph'))
        return HotPathTrainer(model, **kw, **self._loss_kwargs())

    def _train_epoch_iterator(self):
        from .nested import run_nested_train_epoch
        return run_nested_train_epoch

    def run_test_epoch(self, epoch_num, model, test_dataset, test_loader, fold_num, optimizer=None, _steps_only=False):
        from .nested import run_nested_test_epoch
        store = test_loader[0]
        with self._test_trainer(optimizer, lambda: self.get_optimizer(model)) as trainer:
            res = run_nested_test_epoch(trainer, store)
        self.preds, self.pred_idx = res['window_pred'].tolist(), res['window_abs_index'].tolist()
        self.results.update_meter('test_loss', fold_num, res['mean_loss'])
        self.results.patient_results[(fold_num, epoch_num)] = res
        return res

    def perform_post_modeling_actions(self):
        """:767-769 save the results object; here: per (fold, epoch) the patient-level accuracy over the patients served,
        returned and kept as ``self.summary``."""
        self.summary = {}
        for key, res in self.results.patient_results.items():
            self.summary[key] = dict(patients=res['patients'].tolist(), prediction=res['prediction'][res['patients']].tolist(),
                                     mean_loss=res['mean_loss'])
        return self.summary


class CNNToNestedRNNModel(NestedMixin, BaseTraining):
    """:772-778.  NOT in ``network_map`` (its key set is pinned, as for cnn_transformer): reached through
    ``python -m deepards_amd.nested -n cnn_to_nested_rnn`` (``nested_network_map``) or built directly."""

    def __init__(self, args):
        self._init_nested(args)
        super(CNNToNestedRNNModel, self).__init__(args)

    def get_network(self, base_network):
        return M.CNNToNestedRNNNetwork(base_network, self.args.n_sub_batches, True)


class CNNToNestedLSTMModel(NestedMixin, BaseTraining):
    """:781-789.  NOT in ``network_map`` (pinned key set): ``python -m deepards_amd.nested -n cnn_to_nested_lstm``."""
    clip_odd_batches = True

    def __init__(self, args):
        self._init_nested(args)
        super(CNNToNestedLSTMModel, self).__init__(args)

    def get_network(self, base_network):
        return M.CNNToNestedLSTMNetwork(base_network, self.args.n_sub_batches, True)


nested_network_map = {'cnn_to_nested_rnn': CNNToNestedRNNModel, 'cnn_to_nested_lstm': CNNToNestedLSTMModel}


network_map = {
    'cnn_lstm': CNNLSTMModel,
    'cnn_linear': CNNLinearModel,
    'cnn_single_breath_linear': CNNSingleBreathLinearModel,
    'cnn_double_linear': CNNDoubleLinearModel,
    'cnn_linear_to_mean': CNNLinearToMeanModel,
    'cnn_linear_compr_to_rf': CNNLinearComprToRFModel,
}

# flags of the reference's parser that steer code outside the hot path: recognised so that the error says why
OUT_OF_SCOPE_FLAGS = (
    '--transforms', '-tp', '--transform-probability', '--use-i', '-r2', '--drop-if-under-r2', '--drop-i-lim', '--drop-e-lim',
    '--truncate-e-lim', '--butter-low', '--post-hoc-downsampling', '--load-siamese', '--fl-gamma', '--fl-alpha',
    '--plot-untiled-disease-evol', '--plot-tiled-disease-evol', '--plot-dtw-with-disease', '--plot-pt-dtw-by-minute',
    '--perform-dtw-preprocessing', '-vse', '--viz-start-epoch', '--viz-every-n', '--prototype-results-dir',
    '--prototype-fname-prefix', '-2dt', '--two-dim-transforms', '-bks', '--block-kernel-size', '--multitask-epochs', '--row-mix', '-usf',
    '--undersample-factor', '-usdf', '--undersample-std-factor', '--train-pt-frac', '--final-validation',
    '--holdout-set-type', '--downsample-factor', '--bm-to-linear',
)


def build_parser():
    """The reference's parser (:1439-1576) for the flags the hot path reads: same names, short forms, types and
    all-None defaults (so that ``Configuration`` can tell "not given" from a value).  Flags that only steer code
    outside the hot path are refused by ``main`` with the reason (``OUT_OF_SCOPE_FLAGS``)."""
    parser = argparse.ArgumentParser(prog='deepards_amd.train_ards_detector')

    def true_false_flag(flag, help):
        return parser.add_argument(flag, action='store_true', help=help, default=None)
    parser.add_argument('-co', '--config-override', help='path to yml file that overrides elements of defaults.yml')
    parser.add_argument('-dp', '--data-path', help='kept for the configuration files; raw-file ingestion is out of scope')
    parser.add_argument('-en', '--experiment-num', type=int)
    parser.add_argument('-c', '--cohort-file')
    parser.add_argument('-n', '--network', choices=list(network_map.keys()))
    parser.add_argument('-e', '--epochs', type=int)
    parser.add_argument('-p', '--train-from-pickle', help='ARDSRawDataset pickle (read without unpickling) or its .npz export')
    parser.add_argument('--train-to-pickle', help='write the ingested train dataset as .npz')
    parser.add_argument('--test-from-pickle')
    parser.add_argument('--test-to-pickle')
    true_false_flag('--cuda', 'run on the GPU(s): one process per GPU under torch.distributed.run')
    true_false_flag('--cuda-no-dp', 'run on the single GPU --cuda-device')
    parser.add_argument('-b', '--batch-size', type=int)
    parser.add_argument('--base-network', choices=sorted(base_networks) + sorted(M.UNLISTED_BACKBONES))
    parser.add_argument('-nb', '--n-sub-batches', type=int)
    true_false_flag('--no-print-progress', '')
    parser.add_argument('--kfolds', type=int)
    parser.add_argument('-rip', '--initial-planes', type=int)
    parser.add_argument('-rfpt', '--resnet-first-pool-type', choices=['max', 'avg'])
    true_false_flag('--no-test-after-epochs', '')
    true_false_flag('--debug', 'debug code and dont train')
    parser.add_argument('--optimizer', choices=['adam', 'sgd'])
    parser.add_argument('-dt', '--dataset-type', choices=['unpadded_centered_sequences', 'padded_breath_by_breath',
                                                          'padded_breath_by_breath_with_flow_time_features',
                                                          'unpadded_centered_with_bm',
                                                          'unpadded_downsampled_autoencoder_sequences'])
    parser.add_argument('-lr', '--learning-rate', type=float)
    parser.add_argument('--loader-threads', type=int, help='accepted and ignored: batches are gathered on the device')
    parser.add_argument('--save-model', help='save the model to a specific file')
    true_false_flag('--save-model-per-epoch', 'save the model at the end of each epoch')
    parser.add_argument('--load-base-network', help='load base network only from a saved model')
    parser.add_argument('--load-checkpoint', help='load a checkpoint of the model for further training or inference')
    true_false_flag('--no-train', 'Dont train model, just evaluate for inference')
    true_false_flag('--resnet-double-conv', '')
    parser.add_argument('-exp', '--experiment-name')
    parser.add_argument('-wd', '--weight-decay', type=float)
    parser.add_argument('-loss', '--loss-func', choices=['bce', 'vacillating', 'confidence'])
    parser.add_argument('--valpha', type=float, help='alpha of the vacillating loss (defaults.yml: inf); lower values make '
                        'the vacillating term contribute less')
    parser.add_argument('--conf-beta', type=float, help='intensity of the confidence penalty (defaults.yml: 1.0)')
    parser.add_argument('-lc', '--loss-calc', choices=['all_breaths', 'last_breath'], help='cnn_lstm: loss over every '
                        'breath\'s output or over the last breath\'s only')
    parser.add_argument('--time-series-hidden-units', type=int)
    parser.add_argument('--transformer-blocks', type=int, help='cnn_transformer: number of Blocks (defaults.yml: 2)')
    true_false_flag('--unshuffled', 'dont shuffle data')
    true_false_flag('--oversample-minority', '')
    parser.add_argument('--oversample-all-factor', type=float)
    true_false_flag('--reshuffle-oversample-per-epoch', '')
    true_false_flag('--freeze-base-network', '')
    true_false_flag('--stop-on-loss', '')
    parser.add_argument('--stop-thresh', type=float)
    parser.add_argument('--stop-after-epoch', type=int)
    true_false_flag('--clip-grad', '')
    parser.add_argument('--clip-val', type=float)
    parser.add_argument('--cuda-device', type=int, help='number of cuda device you want to use')
    parser.add_argument('--only-fold', type=int, default=None, help='only run specific fold')
    parser.add_argument('--saved-models-dir', help='directory to save models')
    true_false_flag('--print-progress', '')
    true_false_flag('--with-fft', '')
    true_false_flag('--only-fft', '')
    true_false_flag('--fft-real-only', '')
    true_false_flag('--random-kfold', 'perform a random kfold splitting.')
    # (--butter-low and --post-hoc-downsampling are read from the experiment file only: butter_low, post_hoc_downsampling)
    parser.add_argument('--butter-high', type=float, help='10th-order Butterworth filter on every row; with butter_low of the '
                        'experiment file: alone a HIGHPASS at this frequency, with butter_low 0 a lowpass, else a bandpass')
    parser.add_argument('--fft-filtering-low', type=float, help='FFT band filter: keep |f| above this (Hz); needs both bounds')
    parser.add_argument('--fft-filtering-high', type=float, help='FFT band filter: keep |f| below this (Hz); needs both bounds')
    true_false_flag('--bootstrap', '')
    # protopnet (ProtoPNet1DModel; :1546-1560)
    parser.add_argument('--n-warm-epochs', type=int, help='number of warm epochs to run with protopnet')
    parser.add_argument('-pse', '--push-start-epoch', type=int, help='epoch to start the projection pushes')
    parser.add_argument('--push-every-n', type=int, help='starting at push start, push every n epochs')
    parser.add_argument('--n-push-iters', type=int, help='number of iterations to optimize last layer following push')
    parser.add_argument('--clust-lambda', type=float, help='multiplier of cluster loss for protopnet')
    parser.add_argument('--sep-lambda', type=float, help='multiplier of separation loss for protopnet')
    parser.add_argument('-np', '--n-prototypes', type=int, help='number of prototypes to use per class in our model')
    parser.add_argument('-ic', '--incorrect-strength', type=float, help='the incorrect strength value for the linear layer of protopnet')
    true_false_flag('--average-linear-layer', 'protopnet: average like features over the breaths in front of the last layer')
    true_false_flag('--use-l1', 'add an l1 regularization for ppnet')
    # this build's own switches
    parser.add_argument('--seed', type=int, help='seed of the initialisation, the shuffles and the oversampler')
    parser.add_argument('--no-graph', dest='use_graph', action='store_false', default=None, help='run the step eagerly')
    parser.add_argument('--conv-dtype', choices=['f32', 'bf16', 'f32x3p'], help='arithmetic of the residual-block convs')
    parser.add_argument('--folds-in-flight', type=int, help='k-folds trained side by side on this GPU, each on its own stream '
                        '(same per-fold results as one after the other; a B <= 64 step leaves the chip partly idle).  '
                        'Default: min(5, kfolds) on one GPU, 1 under data parallelism; 1 = the sequential loop')
    parser.add_argument('--fold-groups', type=int, help='under torch.distributed: split the ranks into this many groups; group g '
                        'trains folds g, g + G, ... data-parallel over its own ranks (BASELINE config C4: 5 folds over 4 GPUs '
                        'as e.g. 2 groups x 2 ranks).  Default 1: every fold over all ranks')
    parser.add_argument('--act-dtype', choices=['f32', 'bf16'], help='activation storage under --conv-dtype bf16 (default bf16 for ResNets)')
    return parser


def stage_main(argv, parser, networks, stage_map, defaults):
    """The command line of a pretraining stage (``deepards_amd.siamese`` / ``deepards_amd.autoencoder``): the stage's own
    ``parser``, the ``-n`` names it allows, its map of driver classes and its defaults -> (the driver class, its results).
    One GPU, so none of the distributed set-up of ``main``."""
    import sys
    argv = sys.argv[1:] if argv is None else list(argv)
    for a in argv:
        if a.split('=')[0] in OUT_OF_SCOPE_FLAGS:
            raise SystemExit('%s steers code outside the accelerated hot path and is not accepted by this build' % a.split('=')[0])
    args = Configuration(parser.parse_args(argv), defaults)
    if args.network not in networks:
        raise SystemExit('-n must be one of %s' % ', '.join(networks))
    if args.save_model_per_epoch and not args.save_model:
        raise Exception('Must specify a filename to save your model using --save-model')
    cls = stage_map[args.network](args)
    results = cls.train_and_test()
    cls.perform_post_modeling_actions()
    return cls, results


def main(argv=None):
    """:1579-1590.  Under ``python -m torch.distributed.run --nproc-per-node N`` every process takes the GPU
    LOCAL_RANK and joins the RCCL process group before the model class is built."""
    import sys
    argv = sys.argv[1:] if argv is None else list(argv)
    for a in argv:
        if a.split('=')[0] == '--butter-low':
            raise SystemExit('--butter-low is not accepted on the command line -- the flag used to steer code outside the accelerated '
                             'hot path and its refusal is pinned by a test: give butter_low in the -co experiment file')
        if a.split('=')[0] == '--post-hoc-downsampling':
            raise SystemExit('--post-hoc-downsampling is not accepted on the command line -- the flag used to steer code outside the '
                             'accelerated hot path and its refusal is pinned by a test: give post_hoc_downsampling in the -co '
                             'experiment file')
        if a.split('=')[0] in OUT_OF_SCOPE_FLAGS:
            raise SystemExit('%s steers code outside the accelerated cnn_linear hot path (SURVEY.md section 2) and is not '
                             'accepted by this build' % a.split('=')[0])
    for i, a in enumerate(argv):
        if (a in ('-n', '--network') and argv[i + 1:i + 2] == ['cnn_regressor']) or a == '--network=cnn_regressor':
            raise SystemExit('-n cnn_regressor is a pretraining stage with its own command line (the network_map of this driver '
                             'is pinned): python -m deepards_amd.regressor -n cnn_regressor ...')
    args = Configuration(build_parser().parse_args(argv), BUILD_DEFAULTS)
    if args.save_model_per_epoch and not args.save_model:
        raise Exception('Must specify a filename to save your model using --save-model')
    world = int(os.environ.get('WORLD_SIZE', '1'))
    if world > 1:
        import torch.distributed as dist
        if not dist.is_initialized():                    # (a caller may bring its own group: the one-GPU rehearsals use gloo)
            local = int(os.environ.get('LOCAL_RANK', '0'))
            torch.cuda.set_device(local)
            os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
            dist.init_process_group('nccl', device_id=torch.device('cuda', local))
    cls = network_map[args.network](args)
    results = cls.train_and_test()
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()
    return cls, results


if __name__ == "__main__":
    main()
