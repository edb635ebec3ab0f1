"""Training the 1-D ProtoPNet on MI355X: the three-phase trainer and the prototype push.

Mirrors ``ProtoPNetModel`` of the reference's ``train_ards_detector.py`` (:1156-1371: ``get_optimizer`` :1158-1192,
``calc_loss`` :1194-1247, the batch loops of ``run_train_epoch`` :1255-1329, ``run_test_epoch`` :1331-1349) and
``models/protopnet1d/ppnet_push.py`` (:214-305 ``push_prototypes``, :311-427 ``update_prototypes_on_batch``, without the figures).

The reference keeps three optimisers -- warm (add-on layers + prototypes), joint (breath block + add-on layers + prototypes),
last layer -- each of which zeroes and steps only its own parameters.  Here the parameters live in ONE flat bucket ordered
``[breath_block | add_on | prototypes | last_layer]`` and a phase is a set of sub-ranges of it (``phase_ranges``): the existing
fused optimiser kernels run once per (range, weight decay) with momentum 0 and no clip.  Backward work a phase does not need
is skipped -- the parameters outside the phase do not require a gradient, so warm stops at the breath block's map and last
layer computes only ``dW`` of the last layer; equivalent to the reference, whose stale gradients are zeroed before any
optimiser reads them.

NOT clipped: ``ProtoPNetModel.run_train_epoch`` never calls the clipping its base class has, although the experiment files
set ``clip_grad``; this trainer takes ``clip_grad`` / ``clip_val`` and ignores them.
"""
import torch

from . import functional as F_
from . import hip_ops as H
from . import protopnet_ops as PO
from .models.protopnet1d import PPNet
from .train import FlatBucket, HotPathTrainer

PHASES = ('warm', 'joint', 'last_layer')
GROUPS = ('breath_block', 'add_on', 'prototypes', 'last_layer')       # the order of the flat bucket
PHASE_GROUPS = {'warm': ('add_on', 'prototypes'), 'joint': ('breath_block', 'add_on', 'prototypes'),
                'last_layer': ('last_layer',)}
DECAYED = ('breath_block', 'add_on', 'last_layer')                    # the prototypes take no weight decay (:1172-1174, :1182-1184)


def phase_ranges(phase, bounds, weight_decay):
    """[(start, end, weight decay)] of the flat bucket that ``phase``'s optimiser updates; ``bounds``: {group: (start, end)}.
    Neighbouring groups with one weight decay are one range (joint: the breath block and the add-on layers)."""
    if phase not in PHASES:
        raise ValueError('phase must be one of %s, got %r' % (', '.join(PHASES), phase))
    out = []
    for name in GROUPS:
        if name not in PHASE_GROUPS[phase]:
            continue
        s, e = bounds[name]
        if e <= s:
            continue
        wd = float(weight_decay) if name in DECAYED else 0.0
        if out and out[-1][1] == s and out[-1][2] == wd:
            out[-1] = (out[-1][0], e, wd)
        else:
            out.append((s, e, wd))
    return out


def group_parameters(model):
    """{group: [parameters]} of a PPNet in bucket order (``ones`` is no trainable parameter)."""
    return {'breath_block': list(model.breath_block.parameters()), 'add_on': list(model.add_on_layers.parameters()),
            'prototypes': [model.prototype_vectors], 'last_layer': list(model.last_layer.parameters())}


class ProtoPNetTrainer(HotPathTrainer):
    """One PPNet on one GPU.  ``set_phase('warm' | 'joint' | 'last_layer')`` selects the reference's optimiser;
    ``train_step`` is one iteration of its batch loops (eager or a captured graph per (input shape, phase)) and returns the
    total loss (1,), with ``last_parts`` = (total, cls, cluster, separation, l1); ``test_step`` runs under ``model.eval()``
    (:1335 -- on a DenseNet: dropout off) and returns (loss (1,), softmaxed outputs (B, 2), predictions (B,)) with the five
    parts in ``last_test_parts``.  ``optimizer``: 'sgd' (torch.optim.SGD without momentum) or 'adam'."""

    def __init__(self, model, optimizer='sgd', learning_rate=1e-3, weight_decay=1e-4, clust_lambda=0.8, sep_lambda=0.2,
                 use_l1=False, phase='warm', world_size=1, rank=0, process_group=None, use_graph=True, clip_grad=False,
                 clip_val=0.01):
        if not isinstance(model, PPNet):
            raise TypeError('ProtoPNetTrainer trains a PPNet, got %s' % type(model).__name__)
        if world_size != 1:
            raise NotImplementedError('the ProtoPNet trainer runs on one GPU: its phases and the push are not sharded over '
                                      '%d ranks' % world_size)
        super(ProtoPNetTrainer, self).__init__(model, optimizer=optimizer, learning_rate=learning_rate, weight_decay=weight_decay,
                                               momentum=0.0, clip_grad=False, world_size=1, rank=0, process_group=None,
                                               use_graph=use_graph, eval_test=True)
        self.clust_lambda, self.sep_lambda, self.use_l1 = float(clust_lambda), float(sep_lambda), bool(use_l1)
        self.max_dist = float(model.prototype_shape[1] * model.prototype_shape[2])        # ProtoPNet1DModel.get_network (:1387)
        self._groups = {k: [p for p in ps if p.requires_grad] for k, ps in group_parameters(model).items()}
        self._graphs_by_phase = {p: {} for p in PHASES}
        self._l1_mask = None
        self._test_parts, self._test_parts_live = {}, None
        self.last_parts = self.last_test_parts = None
        self.bounds, self._ranges = None, None
        self.phase = None
        self.set_phase(phase)

    # ---- phases ------------------------------------------------------------------------------------------------------
    def set_phase(self, phase):
        """Select the optimiser of the steps that follow: which parameters require a gradient, which ranges of the bucket
        are updated, and which captured graphs are replayed."""
        if phase not in PHASES:
            raise ValueError('phase must be one of %s, got %r' % (', '.join(PHASES), phase))
        self.phase = phase
        for name, params in self._groups.items():
            on = name in PHASE_GROUPS[phase]
            for p in params:
                p.requires_grad_(on)
        self._graphs = self._graphs_by_phase[phase]
        self._graph = self._static = None
        return self

    def _build_bucket(self):
        ordered = [p for name in GROUPS for p in self._groups[name]]
        self.bucket = FlatBucket(ordered)
        starts, i = {}, 0
        for name in GROUPS:
            starts[name] = self.bucket.offsets[i] if self._groups[name] else None
            i += len(self._groups[name])
        self.bounds, end = {}, self.bucket.numel
        for name in reversed(GROUPS):
            s = starts[name]
            self.bounds[name] = (end, end) if s is None else (s, end)
            end = end if s is None else s
        self._ranges = {ph: phase_ranges(ph, self.bounds, self.wd) for ph in PHASES}
        dev = self.bucket.p.device
        if self.optimizer == 'sgd':
            self.state['scratch'] = torch.empty_like(self.bucket.p)       # the kernel's momentum buffer: written, never read
        else:
            for ph in PHASES:                                             # every optimiser has its own moments and step count
                for i, (s, e, _) in enumerate(self._ranges[ph]):
                    self.state['%s.%d.m' % (ph, i)] = torch.zeros(e - s, device=dev, dtype=torch.float32)
                    self.state['%s.%d.v' % (ph, i)] = torch.zeros(e - s, device=dev, dtype=torch.float32)
                    self.state['%s.%d.t' % (ph, i)] = torch.zeros(1, device=dev, dtype=torch.int64)

    def named_gradients(self):
        """{parameter name: its gradient view in the flat bucket} (after a step: what that step's backward wrote)."""
        return {n: p._da_grad for n, p in self.model.named_parameters() if getattr(p, '_da_grad', None) is not None}

    # ---- one step ----------------------------------------------------------------------------------------------------
    def _l1_operands(self):
        if not self.use_l1:
            return None, None
        w = self.model.last_layer.weight
        if self._l1_mask is None or self._l1_mask.device != w.device:
            self._l1_mask = (1 - torch.t(self.model.prototype_class_identity_linear_layer)).to(w.device).contiguous()
        return w, self._l1_mask

    def _loss_parts(self, logits, target, min_d, want_grad):
        m = self.model
        w, mask = self._l1_operands()
        nb = min_d.shape[1] // m.num_prototypes
        return PO.ppnet_loss(logits, target.contiguous(), min_d, nb, m.num_prototypes, self.max_dist, self.clust_lambda,
                             self.sep_lambda, want_grad=want_grad, l1_weight=w, l1_mask=mask)

    def _forward_backward(self, inputs, target, zero_grad=False):
        if zero_grad:
            self.bucket.zero_grad()
        with F_.training_step(self.model):
            logits, min_d = self.model(inputs, None)
            F_.flush_forward(defer=True)
            parts, dlogits, dmin, dw_l1 = self._loss_parts(logits.detach(), target, min_d.detach(), True)
            if self.phase == 'last_layer':                   # only dW of the last layer: the distances' gradient has no reader
                torch.autograd.backward([logits], [dlogits])
            else:
                torch.autograd.backward([logits, min_d], [dlogits, dmin])
            F_.flush_backward()
            if dw_l1 is not None and self.phase == 'last_layer':
                self.model.last_layer.weight._da_grad.add_(dw_l1)
        return parts[:1], logits.detach()

    def compute_gradients(self, inputs, target):
        """Forward, loss and backward of the current phase WITHOUT the update -> ((5,) loss parts, {name: gradient copy} of
        the phase's parameters).  Eager; the model's dropout seed moves as in a step."""
        if self.bucket is None:
            self._build_bucket()
        if not self.model.training:
            self.model.train()
        loss, _ = self._forward_backward(inputs, target, zero_grad=True)
        live = {id(p) for name in PHASE_GROUPS[self.phase] for p in self._groups[name]}
        return loss.as_strided((5,), (1,)).clone(), {n: p._da_grad.clone() for n, p in self.model.named_parameters()
                                                      if id(p) in live}

    def _optimizer_step(self):
        b = self.bucket
        for i, (s, e, wd) in enumerate(self._ranges[self.phase]):
            p, g = b.p[s:e], b.g[s:e]
            if self.optimizer == 'sgd':                      # momentum 0, no clip, "first": the buffer is written, not read
                H.clamp_sgd_nesterov_(p, g, self.state['scratch'][s:e], self.lr, 0.0, wd, 0.0, True, 1.0)
            else:
                if wd:
                    PO.grad_add_decay_(g, p, wd)             # torch.optim.Adam(weight_decay): grad + wd * param
                key = '%s.%d.' % (self.phase, i)
                H.clamp_adam_dev_(p, g, self.state[key + 'm'], self.state[key + 'v'], self.lr, self.state[key + 't'], 0.0)

    def _first_step(self, inputs, target):
        self.model.train()
        self._build_bucket()
        return self._eager_step(inputs, target)

    def train_step(self, inputs, target, reset=None):
        loss = super(ProtoPNetTrainer, self).train_step(inputs, target, reset)
        self.last_parts = loss.as_strided((5,), (1,))         # the (1,) loss is the head of the kernel's five parts
        return loss

    def release_graphs(self):
        super(ProtoPNetTrainer, self).release_graphs()
        for graphs in self._graphs_by_phase.values():
            graphs.clear()
        self._test_parts.clear()
        self.last_parts = self.last_test_parts = self._test_parts_live = None

    # ---- test --------------------------------------------------------------------------------------------------------
    def _test_forward(self, inputs, target):
        with torch.no_grad(), F_.training_step(self.model):
            logits, min_d = self.model(inputs, None)
            F_.flush_forward()
            parts, _, _, _ = self._loss_parts(logits, target, min_d, False)
            outputs = torch.softmax(logits, dim=1)            # :1344
        self._test_parts_live = parts
        return parts[:1], outputs, outputs.argmax(dim=-1)

    def test_step(self, inputs, target, reset=None):
        out = super(ProtoPNetTrainer, self).test_step(inputs, target, reset)
        if self.use_graph:                                    # the graph's own parts buffer, refilled by every replay
            key = (tuple(inputs.shape), tuple(target.shape))
            if key not in self._test_parts:
                self._test_parts[key] = self._test_parts_live
            self.last_test_parts = self._test_parts[key].clone()
        else:
            self.last_test_parts = self._test_parts_live
        return out


def push_prototypes(trainer_or_model, store, indices=None, batch_size=16):
    """Push every prototype onto the nearest patch of the prototype layer's input over the windows ``indices`` of ``store``
    (fold-relative, in this order; None: all of them): per prototype the global minimum of the unpooled distance over the
    windows of the prototype's own class, then over breaths and positions -- the first minimum in (window order, breath,
    position) wins, a later batch replaces an earlier one only on a strict < -- and that patch is copied into
    ``prototype_vectors``.  The running minimum and its source stay in device tensors (nothing is read back per batch).  A
    prototype whose class has no window gets a zero patch, as in the reference.  Runs under ``model.eval()``.
    -> dict(global_min_proto_dist (P,), source (P, 3) int64 = (absolute window index, breath, position), -1 where none,
    proto_rf_boxes (P, 4) int64 = (absolute window index, -1, -1, class) as the reference fills them).
    No figures, no proto_bound_boxes, no prototype_viz."""
    model = trainer_or_model.model if isinstance(trainer_or_model, HotPathTrainer) else trainer_or_model
    if not isinstance(model, PPNet):
        raise TypeError('push_prototypes needs a PPNet (or its trainer), got %s' % type(model).__name__)
    rel = torch.arange(len(store)) if indices is None else torch.as_tensor(indices, dtype=torch.int64)
    dev_idx = store.device_indices(rel)
    p, d = model.num_prototypes, model.prototype_shape[1]
    dev = model.prototype_vectors.device
    gmin = torch.full((p,), float('inf'), device=dev, dtype=torch.float32)
    gpatch = torch.zeros((p, d), device=dev, dtype=torch.float32)
    gsrc = torch.full((p, 3), -1, device=dev, dtype=torch.int64)
    pclass = (torch.arange(p, device=dev) // (p // model.num_classes))             # prototype_class_identity_orig's arg-max
    model.eval()
    with torch.no_grad():
        for s in range(0, len(rel), batch_size):
            idx = dev_idx[s:s + batch_size]
            x, t = store.batch_from_device(idx)
            z, dist = model.push_forward(x)                                          # (B, NB, D, L), (B, NB, P, L)
            b, nb, _, l = dist.shape
            own = t.argmax(dim=1).view(b, 1) == pclass.view(1, p)                    # (B, P): window b is of prototype p's class
            masked = torch.where(own.view(b, 1, p, 1), dist, torch.full_like(dist, float('inf')))
            bmin, bidx = masked.permute(2, 0, 1, 3).reshape(p, b * nb * l).min(dim=1)
            better = bmin < gmin
            patches = z.permute(0, 1, 3, 2).reshape(b * nb * l, d)[bidx]
            src = torch.stack((idx[bidx // (nb * l)], (bidx // l) % nb, bidx % l), dim=1)
            gmin = torch.where(better, bmin, gmin)
            gpatch = torch.where(better.view(p, 1), patches, gpatch)
            gsrc = torch.where(better.view(p, 1), src, gsrc)
        model.prototype_vectors.data.copy_(gpatch.view(p, d, 1))
    found = gsrc[:, 0] >= 0
    boxes = torch.full((p, 4), -1, device=dev, dtype=torch.int64)
    boxes[:, 0] = gsrc[:, 0]
    boxes[:, 3] = torch.where(found, pclass, torch.full_like(pclass, -1))
    return dict(global_min_proto_dist=gmin, source=gsrc, proto_rf_boxes=boxes)
