"""Grad-CAM explainers of a trained cnn_linear + DenseNet model (reference gradcam.py:28-205, patient_gradcam.py:84-115),
batched on the device.

The reference hooks the gradient of ``breath_block.features(x)``, runs relu -> avgpool -> view(-1) -> linear_final, and
backpropagates a one-hot class score: one forward, one backward, two device-to-host copies and Python loops over the channels
PER WINDOW.  Behind ``features`` that head is linear in relu(F), so the guided gradient is closed form,

    d out[k] / d F[n, c, l] = (F[n, c, l] > 0) * W[k, n * C + c] / Lm,

and every CAM the reference defines, for both classes, is a reduction over the map the forward already produced.
``GradCam.cams`` runs ONE forward over a whole batch of windows and the two launches of ``hip_ops.gradcam``
(csrc/gradcam.hip): no backward, no stored gradient, no host loop, no host synchronisation -- the call can be captured and
replayed as a single-stream graph.  The classes keep the reference's names and single-window methods.

BatchNorm mode.  The forward runs each window as its own BatchNorm batch (``rows_per_window = NB``), in the module's CURRENT
mode: the reference deliberately does not call ``eval()`` (gradcam.py:74-76), and neither does this module.  A DenseNet here
always normalises with batch statistics (``track_running_stats=False``), so ``model.eval()`` on it only switches dropout off;
with ``drop_rate > 0`` and ``train()`` the dropout masks are live, as in the reference, and two calls differ.  Call
``model.eval()`` for deterministic CAMs.

Degenerate rows.  ``MaxMinNormCam.normalize`` divides by ``max - min`` of the ReLU'd CAM; where they are equal (a CAM that is
nowhere positive, a constant one, Lm == 1) the reference divides 0 by 0 and casts the NaN to uint8, which is
platform-defined.  Here those bytes are 0 and a ``degenerate`` flag is set (``cam_degenerate`` / ``read_degenerate``).

Only what the reference's own ``CamExtractor`` can run is accepted: a ``CNNLinearNetwork`` whose breath block has ``features``
and hands out the 7-position map (the DenseNets).  Everything else raises ``NotImplementedError`` before any launch.

Command line (arrays, not figures; plotting, medians, DTW clustering and the 2-D analytics are not built):

    python -m deepards_amd.gradcam model.pth -pdp dataset.pkl|.npz --fold K [--only-patient P]
        [--target ground_truth|ards|other] [--kfolds N] [--batched-forward] --ops averages|read_cam -o out.npz
"""
import argparse

import numpy as np
import torch

from . import hip_ops as H
from .models.backbone import HEAD_MAP
from .models.torch_cnn_linear_network import CNNLinearNetwork, SEQ_LEN


def check_model(model):
    """-> (NB, C) of a model the explainers can run; NotImplementedError with the reason otherwise (nothing is launched)."""
    if not isinstance(model, CNNLinearNetwork):
        raise NotImplementedError('Grad-CAM is built for CNNLinearNetwork only (got %s): the closed-form gradient is that of '
                                  'relu -> avgpool -> view(-1) -> linear_final' % type(model).__name__)
    bb = model.breath_block
    feats = getattr(bb, 'features', None)
    if feats is None or not hasattr(feats, 'forward_rlc'):
        raise NotImplementedError('Grad-CAM needs a breath block with `features` (the DenseNets); %s has none -- the '
                                  "reference's CamExtractor cannot run it either" % type(bb).__name__)
    if bb.head_operand_kind(SEQ_LEN) != HEAD_MAP:
        raise NotImplementedError('Grad-CAM needs the 7-position map behind `features`; %s does not hand one out at %d '
                                  'samples' % (type(bb).__name__, SEQ_LEN))
    nb, c = int(model.n_sub_batches), int(bb.n_out_filters)
    if model.linear_final.in_features != nb * c:
        raise NotImplementedError('linear_final takes %d inputs, not NB * C = %d * %d (metadata features are not part of '
                                  'the explainers)' % (model.linear_final.in_features, nb, c))
    return nb, c


class CamExtractor(object):
    """The reference's extractor (gradcam.py:28-65), batched: ``forward_map`` is its ``forward_pass_on_convolutions`` for B
    windows at once -- no hook is registered, the gradient is closed form."""

    def __init__(self, model):
        self.nb, self.channels = check_model(model)
        self.model = model

    def forward_map(self, x):
        """x (B, NB, C_in, 224) on the device -> the norm5 map (B * NB, Lm, C), channels-last, WITHOUT the final ReLU;
        every window its own BatchNorm batch, the module's current mode."""
        if x.dim() != 4 or x.shape[1] != self.nb:
            raise ValueError('expected (B, %d, C_in, %d) windows, got %s' % (self.nb, SEQ_LEN, tuple(x.shape)))
        if x.shape[-1] != SEQ_LEN:
            raise Exception('input breaths must have sequence length of 224')
        if x.shape[0] == 0:
            raise IndexError('index 0 is out of bounds for dimension 0 with size 0')
        b, nb, c, l = x.shape
        bb = self.model.breath_block
        rows = x.reshape(b * nb, c, l)
        bb._check(rows, nb, want_map=True)
        with torch.no_grad():
            return bb.features.forward_rlc(rows, nb, False)


class GradCam(object):
    """Produces class activation maps (gradcam.py:68-107).  ``eval()`` is not called, as there."""

    def __init__(self, model):
        self.model = model
        self.extractor = CamExtractor(self.model)

    def _targets(self, targets, b, device):
        if targets is None:
            return torch.full((b,), -1, dtype=torch.int32, device=device)
        if isinstance(targets, (int, np.integer)):
            if int(targets) not in (-1, 0, 1):
                raise ValueError('a target is 0, 1 or -1 (the predicted class), got %r' % (targets,))
            return torch.full((b,), int(targets), dtype=torch.int32, device=device)
        if isinstance(targets, torch.Tensor) and targets.is_cuda:
            t = targets.to(torch.int32).contiguous()                # (values are not read on the host: no synchronisation)
        else:
            a = np.asarray(targets).astype(np.int64).reshape(-1)
            if a.size and (a.min() < -1 or a.max() > 1):
                raise ValueError('targets are 0, 1 or -1 (the predicted class)')
            t = torch.as_tensor(a, dtype=torch.int32).to(device)
        if tuple(t.shape) != (b,):
            raise ValueError('one target per window expected: (%d,), got %s' % (b, tuple(t.shape)))
        return t

    def _run(self, x, targets, per_window_forward=False):
        if per_window_forward:
            fmap = torch.cat([self.extractor.forward_map(x[i:i + 1]) for i in range(x.shape[0])])
        else:
            fmap = self.extractor.forward_map(x)
        lin = self.model.linear_final
        out = H.gradcam(fmap, lin.weight.detach(), lin.bias.detach(), self._targets(targets, x.shape[0], x.device),
                        self.extractor.nb)
        return fmap, out

    def cams(self, x, targets=None, per_window_forward=False):
        """x (B, NB, C_in, 224) on the device; targets: None (every window's predicted class), an int, or (B,) of 0 / 1 / -1
        (-1: predicted); host-side targets outside -1 .. 1 raise.  A device tensor is taken as it is, without a look at its
        values (that would synchronise): the kernel reads any negative value as "predicted" and any value above 1 as class 1
        (include/deepards_hip.h).  -> ``gradcam_ops.GradCamOutputs`` of device tensors (logits,
        target, raw A / R of both classes, and the three normalisations of the target class) from one forward and two
        launches.
        The CAM kernels give a window the same bits in any batch; the breath block's forward does not: a window's map at a
        later position of a batch differs in its last bits from its map alone (the BatchNorm statistics are merged from
        records of 64-unit tiles, whose boundaries fall differently inside a window that does not start on one; up to 1.5e-5
        measured on densenet18).  per_window_forward=True runs one forward per window (B forwards, still two CAM launches):
        every window's outputs are then bit for bit those of the single-window methods."""
        return self._run(x, targets, per_window_forward)[1]

    def _one(self, input, target):
        if input.dim() != 3:
            raise ValueError('one (NB, C_in, %d) window expected, got %s' % (SEQ_LEN, tuple(input.shape)))
        return self._run(input.unsqueeze(0), target)

    def generate_one_hot_grad_and_output(self, input, target):
        """-> (conv_output, guided_gradients, model_output): numpy (NB, C, Lm) arrays and the (1, 2) logits, as
        gradcam.py:80-99; the gradient is materialised on the host from the closed form."""
        fmap, out = self._one(input, target)
        conv = fmap.permute(0, 2, 1).cpu().numpy()                                     # (NB, C, Lm)
        t = int(out.target[0])
        nb, c, lm = conv.shape
        w = self.model.linear_final.weight.detach()[t].cpu().numpy().reshape(nb, c, 1)
        grad = np.where(conv > 0, w / np.float32(lm), np.float32(0)).astype(np.float32)
        return conv, grad, out.logits


class MaxMinNormCam(GradCam):
    """CAMs normalised by the max / min of the single class output (gradcam.py:110-162).  The reference's class-level
    ``grads`` / ``preds`` lists are NOT kept: they grow without bound over a patient sweep and nothing here reads them."""

    def generate_read_cam(self, input, target):
        """-> (cam (NB, Lm) float32 holding the 0..255 bytes, as the reference's float32 array does, model_output (1, 2))."""
        out = self._one(input, target)[1]
        return out.read_maxmin[0].cpu().numpy().astype(np.float32), out.logits

    def generate_cam(self, input, target=None):
        """-> (cam (Lm,) uint8, model_output (1, 2))."""
        out = self._one(input, target)[1]
        return out.cam_maxmin[0].cpu().numpy(), out.logits


class FracTotalNormCam(GradCam):
    """The target class's share of both classes' ReLU'd read CAMs (gradcam.py:165-192)."""

    def generate_cam(self, input, target):
        raise NotImplementedError('Havent done this yet')

    def generate_read_cam(self, input, target):
        """-> (cam (NB, Lm) float32 holding the 0..255 bytes; 0 where both classes' CAMs are 0, model_output (1, 2))."""
        out = self._one(input, target)[1]
        return out.read_frac[0].cpu().numpy().astype(np.float32), out.logits


class UnNormalizedCam(GradCam):
    def generate_cam(self, input, target=None):
        """-> (max(cam, 0) (Lm,) float32, model_output (1, 2)) (gradcam.py:195-205)."""
        out = self._one(input, target)[1]
        return out.cam[0].cpu().numpy(), out.logits


def resize_cam(cam, breath_len=SEQ_LEN):
    """A (Lm,) CAM stretched to ``breath_len`` samples -> (breath_len, 1) float64: linear interpolation with half-pixel
    centres (source coordinate (i + 0.5) Lm / breath_len - 0.5) and clamped edges, in float64 on the host.  This is the
    FLOAT rule of ``cv2.resize(cam, (1, breath_len))`` (INTER_LINEAR), which the reference applies (gradcam.py:237,
    patient_gradcam.py:78,110).  cv2 is not a dependency of this package, and on uint8 input it interpolates with fixed-point
    coefficients and rounds back to uint8: bit equality with cv2 on uint8 input is NOT claimed and has not been checked."""
    a = np.asarray(cam, dtype=np.float64)
    if a.ndim == 2 and a.shape[1] == 1:
        a = a[:, 0]
    if a.ndim != 1 or a.size < 1:
        raise ValueError('resize_cam takes one (Lm,) CAM, got %s' % (np.shape(cam),))
    n = a.size
    src = (np.arange(breath_len, dtype=np.float64) + 0.5) * (float(n) / breath_len) - 0.5
    src = np.clip(src, 0.0, float(n - 1))
    i0 = np.minimum(np.floor(src).astype(np.int64), max(n - 2, 0))
    i1 = np.minimum(i0 + 1, n - 1)
    f = src - i0
    return (a[i0] * (1.0 - f) + a[i1] * f).reshape(breath_len, 1)


_TARGETS = {'ards': 1, 'other': 0}


class PatientCams(object):
    """Per-patient CAM statistics over a ``DeviceTileStore`` (patient_gradcam.py:30-115 ``PatientGradCam``), in batches.
    target: 'ground_truth' | 'ards' | 'other' | 0 | 1; 'both' is refused, as the reference's averages refuse it.
    By default the results are those of the reference's loop over single windows, bit for bit: a batch is gathered and goes
    through the CAM kernels at once, but every window takes its own forward (``GradCam.cams(per_window_forward=True)``, which
    says why).  ``per_window_forward=False`` on ``window_cams`` / ``averages`` takes ONE forward per batch instead: about 50
    times faster at B = 64 (DESIGN_APPENDIX.md, "Grad-CAM"), equal to the forward's accuracy (logits to ~1e-7, a byte of a CAM
    may move by one)."""

    def __init__(self, model, store, target):
        if target == 'both':
            raise NotImplementedError('both mode currently doesnt support operations outside sampled_seqs')
        if not (target == 'ground_truth' or target in _TARGETS or (isinstance(target, (int, np.integer)) and int(target) in (0, 1))):
            raise ValueError("target must be 'ground_truth', 'ards', 'other', 0 or 1, got %r" % (target,))
        self.grad_cam = MaxMinNormCam(model)
        self.store, self.target = store, target
        groups = store.patient_slot if getattr(store, 'patient_slot', None) is not None else getattr(store, 'patients', None)
        if groups is None:
            raise ValueError('the store carries no patient information (patient_slot / patients)')
        self.groups = np.asarray(groups)

    def _fold(self):
        """-> (absolute window index, patient, ground truth) of the store's current fold, in fold order."""
        n = len(self.store)
        abs_idx = np.arange(n) if self.store.kfold_indexes is None else self.store.kfold_indexes.cpu().numpy()
        gt = self.store.targets.argmax(dim=1).cpu().numpy()[abs_idx]
        return abs_idx, self.groups[abs_idx], gt

    def get_target(self, ground_truth):
        if self.target == 'ground_truth':
            return int(ground_truth)
        return _TARGETS[self.target] if self.target in _TARGETS else int(self.target)

    def _window_targets(self, patients, gt):
        """The target of every window: its patient's, taken from the patient's first window (patient_gradcam.py:89-90)."""
        first = {}
        for p, y in zip(patients.tolist(), gt.tolist()):
            first.setdefault(p, y)
        return np.array([self.get_target(first[p]) for p in patients.tolist()], dtype=np.int32)

    def window_cams(self, batch_size=64, only_patient=None, fields=('cam_maxmin',), per_window_forward=True):
        """``cams`` over the fold's windows (of one patient, if given) in batches of ``batch_size`` -> (absolute indices,
        patients, targets, {field: host array}, logits (N, 2)); one device-to-host copy per field at the end."""
        abs_idx, patients, gt = self._fold()
        tgt = self._window_targets(patients, gt)
        rel = np.arange(len(abs_idx))
        if only_patient is not None:
            rel = rel[patients == only_patient]
            if rel.size == 0:
                raise ValueError('patient %r has no window in the current fold' % (only_patient,))
        parts = {f: [] for f in tuple(fields) + ('logits',)}
        for s in range(0, len(rel), batch_size):
            idx = rel[s:s + batch_size]
            x, _ = self.store.batch(idx)
            out = self.grad_cam.cams(x, tgt[idx], per_window_forward=per_window_forward)
            for f in parts:
                parts[f].append(getattr(out, f))
        host = {f: torch.cat(v).cpu().numpy() for f, v in parts.items()}
        return abs_idx[rel], patients[rel], tgt[rel], host, host.pop('logits')

    def averages(self, batch_size=64, only_patient=None, per_window_forward=True):
        """-> {patient: dict(cam (Lm,) float64, model_output (2,) float64, count, target)}: the mean over the patient's
        windows of the max-min window CAM -- the reference's np.mean of the uint8 CAMs -- and of ``model_output``
        (patient_gradcam.py:97-109), in batches through ``DeviceTileStore.batch``; a patient may span batches."""
        _, patients, tgt, host, logits = self.window_cams(batch_size, only_patient, per_window_forward=per_window_forward)
        cams = host['cam_maxmin']
        res = {}
        for p in dict.fromkeys(patients.tolist()):
            sel = np.nonzero(patients == p)[0]
            mean_out = np.zeros((2,), dtype=np.float64)
            for i in sel:
                mean_out += logits[i]
            res[p] = dict(cam=np.mean(cams[sel].astype(np.float64), axis=0), model_output=mean_out / len(sel), count=int(len(sel)),
                          target=int(tgt[sel[0]]))
        return res


# ---- command line -----------------------------------------------------------------------------------------------------------
def build_parser():
    parser = argparse.ArgumentParser(prog='python -m deepards_amd.gradcam',
                                     description='Grad-CAM arrays of a trained cnn_linear + DenseNet model')
    parser.add_argument('model_path', help='path to the saved model')
    parser.add_argument('-pdp', '--pickled-data-path', required=True,
                        help='ARDSRawDataset pickle (read without unpickling) or its .npz export')
    parser.add_argument('--only-patient')
    parser.add_argument('--fold', type=int, required=True, help='k-fold whose TEST patients are explained')
    parser.add_argument('--kfolds', type=int, default=None,
                        help='folds to split a dataset into that carries none (the driver\'s --kfolds)')
    parser.add_argument('--ops', choices=['averages', 'read_cam'], required=True,
                        help='averages: per-patient mean of the max-min window CAMs; read_cam: the max-min read CAM of every window')
    parser.add_argument('--target', choices=['ards', 'other', 'ground_truth', 'both'], default='ground_truth')
    parser.add_argument('--base-network', default=None,
                        help='architecture of a file that holds weights only (a whole-module file names its own)')
    parser.add_argument('--batch-size', type=int, default=64)
    parser.add_argument('--batched-forward', action='store_true',
                        help='one forward per batch instead of one per window: much faster, equal to the single-window '
                             'results to the accuracy of the forward instead of bit for bit')
    parser.add_argument('-o', '--output', required=True, help='the .npz to write')
    return parser


def load_model(path, base_network=None):
    """The model of a checkpoint file, through the readers the driver uses for --load-checkpoint (nothing is unpickled
    outside torch's restricted unpickler): a whole module of this package as it is; for any other file a fresh
    CNNLinearNetwork of the architecture the file (or ``base_network``) names receives the weights."""
    from . import checkpoint as ck
    from . import models as M
    if ck.checkpoint_kind(path) == 'own':
        return ck.load_own_module(path)
    name = base_network
    if name is None and ck.checkpoint_kind(path) == 'foreign':
        name = ck.read_module_checkpoint(path)['network_name']
    if name not in M.base_networks:
        raise ValueError('base network %r of %s is not built by this package (pass --base-network)' % (name, path))

    def build():
        bb = M.build_base_network(name)
        sd = ck.read_module_checkpoint(path)['state_dict'] if ck.checkpoint_kind(path) == 'foreign' else \
            torch.load(path, weights_only=True, map_location='cpu')
        width = next(v for k, v in sd.items() if k.endswith('linear_final.weight')).shape[1]
        return M.CNNLinearNetwork(bb, width // bb.n_out_filters, width % bb.n_out_filters)

    return ck.load_model_weights(path, build)


def main(argv=None):
    args = build_parser().parse_args(argv)
    from .ingest import load_dataset
    ds = load_dataset(args.pickled_data_path)
    if ds.total_kfolds is None:
        if args.kfolds is None:
            raise SystemExit('--fold needs a k-fold dataset: %s carries no folds (pass --kfolds)' % args.pickled_data_path)
        ds.total_kfolds = args.kfolds                                # an unfolded dataset split now, as the driver does
    ds.train = True
    store = ds.to_store('cuda').make_test_store_if_kfold()          # patient_gradcam.py:406-407
    store.set_kfold_indexes_for_fold(args.fold)
    model = load_model(args.model_path, args.base_network).cuda()
    pc = PatientCams(model, store, args.target)
    only = args.only_patient
    if only is not None:
        if ds.patients is not None and only in set(ds.patients.tolist()):
            only = int(ds.patient_slot[np.nonzero(ds.patients == only)[0][0]])
        else:
            only = int(only)
    names = None if ds.patients is None else {int(s): p for s, p in zip(ds.patient_slot.tolist(), ds.patients.tolist())}
    label = (lambda s: str(s)) if names is None else (lambda s: names[int(s)])
    if args.ops == 'averages':
        res = pc.averages(args.batch_size, only, per_window_forward=not args.batched_forward)
        keys = list(res)
        out = dict(patient=np.array([label(k) for k in keys]), cam=np.stack([res[k]['cam'] for k in keys]),
                   model_output=np.stack([res[k]['model_output'] for k in keys]),
                   count=np.array([res[k]['count'] for k in keys], dtype=np.int64),
                   target=np.array([res[k]['target'] for k in keys], dtype=np.int64))
    else:
        abs_idx, patients, tgt, host, logits = pc.window_cams(args.batch_size, only, fields=('read_maxmin', 'read_degenerate'),
                                                               per_window_forward=not args.batched_forward)
        out = dict(patient=np.array([label(p) for p in patients.tolist()]), window_index=abs_idx.astype(np.int64),
                   read_cam=host['read_maxmin'], read_degenerate=host['read_degenerate'], model_output=logits,
                   target=tgt.astype(np.int64))
    np.savez_compressed(args.output, **out)
    print('%s: %s of %d %s -> %s' % (args.ops, args.target, len(out['patient']),
                                     'patients' if args.ops == 'averages' else 'windows', args.output))
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
