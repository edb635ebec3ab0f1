"""The 1-D ProtoPNet on MI355X.

Operator surface of reference ``deepards/models/protopnet1d/model.py`` (the five receptive-field functions :11-110, PPNet
:113-354, construct_PPNet :359-382): same constructor arguments, attributes, methods and ``state_dict`` keys
(``breath_block.*``, ``add_on_layers.{0,2,..}.weight / .bias``, ``prototype_vectors``, ``ones``, ``last_layer.weight``).  The
children of ``add_on_layers`` and ``last_layer`` are parameter containers: the 1x1 convolutions run on the GEMM conv path, the
bias / activation, the L2 prototype layer with its min-pool and log similarity, and the bias-free last layer in the kernels of
csrc/protopnet.hip (``protopnet_ops``).  All B windows go through the network in ONE pass over B * NB rows (BatchNorm
statistics still per window) instead of the reference's Python loop (:268-281).

Two stated departures from the reference:
  * ``prototype_class_identity`` repeats ``sub_batch_size`` times where the reference hard-codes 20 (:143); identical at NB = 20.
  * ``push_forward`` computes window i from x[i]; the reference recomputes x[0] for every i (:291), so that its push searches only
    the first window of each batch.
Refused with a reason: prototype activations other than 'log', a prototype kernel size other than 1, a base network that is
not one of this package's DenseNets (``forward_no_pool`` exists only there).
"""
import math

import torch
import torch.nn as nn

from .. import functional as F_
from .. import protopnet_ops as PO
from .densenet import DenseNet


def compute_layer_rf_info(layer_filter_size, layer_stride, layer_padding, previous_layer_rf_info):
    """[n, jump, receptive-field size, centre of the first field] behind one more layer (model.py:11-46); layer_padding is
    'SAME', 'VALID' or the padding of one side."""
    n_in, j_in, r_in, start_in = previous_layer_rf_info[:4]
    if layer_padding == 'SAME':
        n_out = math.ceil(float(n_in) / float(layer_stride))
        rem = n_in % layer_stride
        pad = max(layer_filter_size - (layer_stride if rem == 0 else rem), 0)
        assert n_out == math.floor((n_in - layer_filter_size + pad) / layer_stride) + 1
        assert pad == (n_out - 1) * layer_stride - n_in + layer_filter_size
    elif layer_padding == 'VALID':
        n_out = math.ceil(float(n_in - layer_filter_size + 1) / float(layer_stride))
        pad = 0
        assert n_out == math.floor((n_in - layer_filter_size + pad) / layer_stride) + 1
        assert pad == (n_out - 1) * layer_stride - n_in + layer_filter_size
    else:
        pad = layer_padding * 2
        n_out = math.floor((n_in - layer_filter_size + pad) / layer_stride) + 1
    p_left = math.floor(pad / 2)
    j_out = j_in * layer_stride
    r_out = r_in + (layer_filter_size - 1) * j_in
    start_out = start_in + ((layer_filter_size - 1) / 2 - p_left) * j_in
    return [n_out, j_out, r_out, start_out]


def compute_rf_protoL_at_spatial_location(seq_len, width_index, protoL_rf_info):
    """[start, end) of the input samples position ``width_index`` of the prototype layer sees, clipped to the row (:49-61)."""
    n, j, r, start = protoL_rf_info[:4]
    assert width_index < n
    center_w = start + (width_index * j)
    return [max(int(center_w - (r / 2)), 0), min(int(center_w + (r / 2)), seq_len)]


def compute_rf_prototype(seq_len, prototype_patch_index, protoL_rf_info):
    """(index, ., position) -> [index, start, end] (:64-70)."""
    rf = compute_rf_protoL_at_spatial_location(seq_len, prototype_patch_index[2], protoL_rf_info)
    return [prototype_patch_index[0], rf[0], rf[1]]


def compute_rf_prototypes(seq_len, prototype_patch_indices, protoL_rf_info):
    return [compute_rf_prototype(seq_len, idx, protoL_rf_info) for idx in prototype_patch_indices]


def compute_proto_layer_rf_info_v2(seq_len, layer_filter_sizes, layer_strides, layer_paddings, prototype_kernel_size):
    """The receptive field of the prototype layer behind the base network's convs and pools (:81-110)."""
    assert len(layer_filter_sizes) == len(layer_strides)
    assert len(layer_filter_sizes) == len(layer_paddings)
    rf_info = [seq_len, 1, 1, 0.5]
    for k, s, p in zip(layer_filter_sizes, layer_strides, layer_paddings):
        rf_info = compute_layer_rf_info(k, s, p, rf_info)
    return compute_layer_rf_info(prototype_kernel_size, 1, 'VALID', rf_info)


class PPNet(nn.Module):
    def __init__(self, features, seq_len, prototype_shape, sub_batch_size, batch_size, proto_layer_rf_info, num_classes,
                 init_weights=True, prototype_activation_function='log', add_on_layers_type='bottleneck',
                 incorrect_strength=-0.5, average_linear=False):
        super(PPNet, self).__init__()
        if not isinstance(features, DenseNet):
            raise NotImplementedError('PPNet needs one of this package\'s DenseNets as its base network (the reference\'s '
                                      'forward_no_pool exists only there), got %s' % type(features).__name__)
        if prototype_activation_function != 'log':
            raise NotImplementedError("the prototype layer's kernel computes the 'log' similarity; 'linear' and callables "
                                      'are not built (got %r)' % (prototype_activation_function,))
        prototype_shape = tuple(int(v) for v in prototype_shape)
        if len(prototype_shape) != 3 or prototype_shape[2] != 1:
            raise NotImplementedError('the prototype layer is built for prototype kernel size 1 (the reference\'s '
                                      '(2 * n_prototypes, 128, 1)), got %s' % (prototype_shape,))
        if num_classes != 2:
            raise NotImplementedError('the last layer and the loss are built for 2 classes, got %d' % num_classes)
        if add_on_layers_type not in ('bottleneck', 'regular'):
            raise ValueError("add_on_layers_type must be 'bottleneck' or 'regular', got %r" % (add_on_layers_type,))
        p, d = prototype_shape[:2]
        mult = 1 if average_linear else int(sub_batch_size)
        if p % num_classes or not 2 <= p <= PO.MAX_P or (p * mult) % 4 or d % 32 or not 32 <= d <= PO.MAX_D:
            raise NotImplementedError('prototype_shape %s: the kernels take 2 ... %d prototypes split evenly over the classes, '
                                      'last-layer inputs (%d) in quads, and 32 ... %d channels, a multiple of 32'
                                      % (prototype_shape, PO.MAX_P, p * mult, PO.MAX_D))
        self.seq_len = seq_len
        self.prototype_shape = prototype_shape
        self.num_prototypes = p
        self.num_classes = num_classes
        self.epsilon = PO.EPSILON
        self.sub_batch_size = sub_batch_size
        self.incorrect_strength = incorrect_strength
        self.average_linear = average_linear
        self.prototype_activation_function = prototype_activation_function

        # one-hot class identity of every prototype: the same number of prototypes for each class (:136-141)
        self.prototype_class_identity_orig = torch.zeros(p, num_classes)
        per_class = p // num_classes
        for j in range(p):
            self.prototype_class_identity_orig[j, j // per_class] = 1
        # (the reference repeats 20 times, :143: its NB)
        self.prototype_class_identity = self.prototype_class_identity_orig.repeat((int(sub_batch_size), 1))
        self.prototype_class_identity_linear_layer = (self.prototype_class_identity_orig if average_linear
                                                      else self.prototype_class_identity)
        self.proto_layer_rf_info = proto_layer_rf_info
        self.breath_block = features
        # A window's outputs must not depend on where it sits in a batch: the push copies a patch of z into a prototype, and
        # that prototype is at distance exactly 0 from its source window only while a later forward recomputes the same
        # bits in whatever batch the window comes.  The fused dense-block kernels merge BatchNorm statistics from tile
        # records whose boundaries depend on the position; the per-layer Functions do not (set it back to True for their
        # speed, at the price of that property).
        features.features.block_kernels = False

        first_in = [m for m in features.modules() if isinstance(m, nn.BatchNorm1d)][-1].num_features
        layers = []
        if add_on_layers_type == 'bottleneck':
            cur = first_in
            while cur > d or not layers:
                out = max(d, cur // 2)
                layers += [nn.Conv1d(cur, out, kernel_size=1), nn.ReLU(), nn.Conv1d(out, out, kernel_size=1)]
                if out > d:
                    layers.append(nn.ReLU())
                else:
                    assert out == d
                    layers.append(nn.Sigmoid())
                cur = cur // 2
        else:
            layers = [nn.Conv1d(first_in, d, kernel_size=1), nn.ReLU(), nn.Conv1d(d, d, kernel_size=1), nn.Sigmoid()]
        for m in layers:
            if isinstance(m, nn.Conv1d) and (m.in_channels % 32 or m.out_channels % 32):
                raise NotImplementedError('add-on conv %d -> %d: channel counts must be multiples of 32' %
                                          (m.in_channels, m.out_channels))
        self.add_on_layers = nn.Sequential(*layers)
        self.prototype_vectors = nn.Parameter(torch.rand(self.prototype_shape), requires_grad=True)
        self.ones = nn.Parameter(torch.ones(self.prototype_shape), requires_grad=False)      # (a state_dict key of the reference)
        self.last_layer = nn.Linear(p * mult, num_classes, bias=False)
        if init_weights:
            self._initialize_weights()

    # ---- the map behind the add-on layers --------------------------------------------------------------------------------
    def _add_on(self, h):
        """(rows, L, C) channels-last -> (rows, L, D): conv1x1 (GEMM path) + bias / activation kernel per add-on layer."""
        mods = list(self.add_on_layers)
        for conv, act in zip(mods[0::2], mods[1::2]):
            h = PO.PointwiseConvFunction.apply(h, conv.weight)
            h = PO.BiasActFunction.apply(h, conv.bias, PO.SIGMOID if isinstance(act, nn.Sigmoid) else PO.RELU)
        return h

    def _features_rlc(self, x, rows_per_window):
        """x (rows, C_in, L) -> z (rows, 7, D) channels-last, BatchNorm statistics per window of ``rows_per_window`` rows."""
        PO._check_f32_path('PPNet')
        return self._add_on(self.breath_block.forward_windows(x, rows_per_window, pooled=False))

    def conv_features(self, x):
        """One window x (N, C_in, L) -> the input of the prototype layer in the reference's (N, D, L') layout (:209-215)."""
        return self._features_rlc(x, x.shape[0]).permute(0, 2, 1)

    def _l2_convolution(self, x):
        """x (N, D, L') -> the squared L2 distances (N, P, L') between every prototype and every position (:217-242), in the
        direct form sum_c (x - p)^2.  No gradient flows through this view of the layer (the push and the analyses use it)."""
        z = x.detach().permute(0, 2, 1).contiguous()
        return PO.proto_fwd(z, self.prototype_vectors.detach(), want_dist=True)[0]

    def prototype_distances(self, x):
        return self._l2_convolution(self.conv_features(x))

    def distance_2_similarity(self, distances):
        return torch.log((distances + 1) / (distances + self.epsilon))

    def seq_forward(self, x):
        """One window x (N, C_in, L) -> prototype activations (N, P), min_distances (N, P) (:260-266)."""
        return PO.PrototypeLayerFunction.apply(self._features_rlc(x, x.shape[0]), self.prototype_vectors)

    def _windows(self, x):
        if x.dim() != 4:
            raise ValueError('expected (B, NB, C, L) windows, got %s' % (tuple(x.shape),))
        if x.shape[0] == 0:           # the reference indexes x[0] first (:269)
            raise IndexError('index 0 is out of bounds for dimension 0 with size 0')
        b, nb, c, l = x.shape
        return b, nb, self._features_rlc(x.reshape(b * nb, c, l), nb)

    def forward(self, x, metadata):
        """x (B, NB, C_in, 224) -> logits (B, 2), min_distances (B, NB * P) (:268-281)."""
        b, nb, z = self._windows(x)
        if not self.average_linear and nb != self.sub_batch_size:
            raise ValueError('the last layer is sized for windows of %d breaths, got %d' % (self.sub_batch_size, nb))
        sim, min_d = PO.PrototypeLayerFunction.apply(z, self.prototype_vectors)
        flat = F_.WindowMeanFunction.apply(sim, nb) if self.average_linear else sim.view(b, nb * self.num_prototypes)
        return PO.LastLayerFunction.apply(flat, self.last_layer.weight), min_d.view(b, nb * self.num_prototypes)

    def push_forward(self, x):
        """x (B, NB, C_in, L) -> the prototype layer's input (B, NB, D, L') and the unpooled distances (B, NB, P, L'), window
        i from x[i] (the reference recomputes x[0] for every i, :291)."""
        with torch.no_grad():
            b, nb, z = self._windows(x)
            dist = PO.proto_fwd(z, self.prototype_vectors.detach(), want_dist=True)[0]
        return z.view(b, nb, z.shape[1], z.shape[2]).permute(0, 1, 3, 2), dist.view(b, nb, dist.shape[1], dist.shape[2])

    def __repr__(self):
        rep = ('PPNet(\n'
               '\tfeatures: {},\n'
               '\tseq_len: {},\n'
               '\tprototype_shape: {},\n'
               '\tproto_layer_rf_info: {},\n'
               '\tnum_classes: {},\n'
               '\tepsilon: {}\n'
               ')')
        return rep.format(self.breath_block, self.seq_len, self.prototype_shape, self.proto_layer_rf_info, self.num_classes,
                          self.epsilon)

    def set_last_layer_incorrect_connection(self):
        """1 on a prototype's own class, ``incorrect_strength`` elsewhere (:319-333)."""
        pos = torch.t(self.prototype_class_identity_linear_layer)
        weights = 1 * pos + self.incorrect_strength * (1 - pos)
        self.last_layer.weight.data.copy_(weights)

    def _initialize_weights(self):
        for m in self.add_on_layers.modules():
            if isinstance(m, nn.Conv1d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
        self.set_last_layer_incorrect_connection()

    def ensure_incorrect_protos_zeroed(self):
        weights = self.last_layer.weight.data
        self.last_layer.weight.data.copy_(weights * torch.t(self.prototype_class_identity_linear_layer.to(weights.device)))


def construct_PPNet(base_architecture, sub_batch_size, seq_len=224, prototype_shape=(20, 128, 1), num_classes=2,
                    prototype_activation_function='log', add_on_layers_type='bottleneck', batch_size=16,
                    incorrect_strength=-0.5, average_linear=False):
    if not isinstance(base_architecture, DenseNet):
        raise NotImplementedError('construct_PPNet needs one of this package\'s DenseNets (conv_info / forward_no_pool), got %s'
                                  % type(base_architecture).__name__)
    if len(tuple(prototype_shape)) != 3 or prototype_shape[2] != 1:
        raise NotImplementedError('the prototype layer is built for prototype kernel size 1, got %s' % (tuple(prototype_shape),))
    layer_filter_sizes, layer_strides, layer_paddings = base_architecture.conv_info()
    proto_layer_rf_info = compute_proto_layer_rf_info_v2(seq_len=seq_len, layer_filter_sizes=layer_filter_sizes,
                                                         layer_strides=layer_strides, layer_paddings=layer_paddings,
                                                         prototype_kernel_size=prototype_shape[2])
    return PPNet(features=base_architecture, seq_len=seq_len, prototype_shape=prototype_shape, sub_batch_size=sub_batch_size,
                 batch_size=batch_size, proto_layer_rf_info=proto_layer_rf_info, num_classes=num_classes, init_weights=True,
                 prototype_activation_function=prototype_activation_function, add_on_layers_type=add_on_layers_type,
                 incorrect_strength=incorrect_strength, average_linear=average_linear)
