"""The head of the 1-D ProtoPNet (reference models/protopnet1d/model.py:113-354 PPNet; train_ards_detector.py:1194-1247
ProtoPNetModel.calc_loss) as wrappers of the C ABI (``da_bias_act_*``, ``da_proto_*``, ``da_ppnet_loss``; kernels in
csrc/protopnet.hip) and the autograd Functions over them.  Same conventions as the other wrappers: contiguous float32 CUDA
operands, the current stream, no host synchronisation, shapes checked here so that an unsupported one raises with the shape
before anything is launched.  The map is (rows, L, C) channels-last, rows = B * NB.

Where the similarity's derivative goes: ``proto_bwd`` takes the gradient on ``sim`` and the gradient on ``min_d`` apart and
folds d sim / d min_d = -(1 - eps) / ((min_d + 1) (min_d + eps)) in the kernel; the loss's own min_d term (cluster and
separation cost) comes in as the gradient on ``min_d``."""
import torch
from torch.autograd import Function

from . import functional as F_
from . import hip_ops as _H

RELU, SIGMOID = 0, 1
EPSILON = 1e-4                       # PPNet.epsilon (model.py:124)
MAX_P, MAX_L, MAX_D, MAX_N = 64, 64, 512, 4096
L1_COEF = 1e-4                       # calc_loss: loss + 1e-4 * l1 (train_ards_detector.py:1246)


def _mn(t, n, who):
    if t.dim() < 2 or t.shape[-1] != n or t.numel() == 0:
        raise ValueError('%s: expected (..., %d), got %s' % (who, n, tuple(t.shape)))
    m = t.numel() // n
    if n % 4 or n > MAX_N or t.numel() >= 2 ** 31:
        raise _H.HipError('%s: unsupported (M, N) = (%d, %d): N %% 4 == 0 up to %d, fewer than 2^31 elements' % (who, m, n, MAX_N))
    return m


def _act(act):
    if act not in (RELU, SIGMOID):
        raise ValueError('act must be RELU (0) or SIGMOID (1), got %r' % (act,))
    return act


def bias_act_fwd(x, bias, act, out=None):
    """y = act(x + bias) over the last axis: x (..., N), bias (N,) -> y like x (``out``: the destination, x itself allowed)."""
    n = _H._f32(bias, 'bias').numel()
    m = _mn(_H._f32(x, 'x'), n, 'bias_act_fwd')
    y = _H._out(out, x.shape, torch.float32, x.device, False, 'bias_act_fwd', strict=True)
    _H._chk(_H._lib.lib().da_bias_act_fwd(_H._p(x), _H._p(bias), _H._p(y), m, n, _act(act), _H._stream()), 'da_bias_act_fwd')
    return y


def bias_act_bwd(dy, y, act, need_dx=True, dbias=None, accumulate=False, need_dbias=True):
    """-> dx = dy * act'(y) (None without need_dx), dbias (N,) = column sums of dx in a fixed order (None without need_dbias);
    ``dbias``: the destination, written or -- accumulate -- added to."""
    n = y.shape[-1]
    m = _mn(_H._f32(y, 'y'), n, 'bias_act_bwd')
    if tuple(_H._f32(dy, 'dy').shape) != tuple(y.shape):
        raise ValueError('bias_act_bwd: dy %s must be shaped like y %s' % (tuple(dy.shape), tuple(y.shape)))
    if not (need_dx or need_dbias):
        return None, None
    L = _H._lib.lib()
    dx = torch.empty_like(y) if need_dx else None
    ws = None
    if need_dbias:
        dbias = _H._out(dbias, (n,), torch.float32, y.device, accumulate, 'bias_act_bwd', strict=True)
        ws = torch.empty((max(L.da_bias_act_bwd_workspace(m, n) // 4, 1),), device=y.device, dtype=torch.float32)
    _H._chk(L.da_bias_act_bwd(_H._p(dy), _H._p(y), _H._p(dx), _H._p(dbias if need_dbias else None), 1 if accumulate else 0,
                              _H._p(ws), m, n, _act(act), _H._stream()), 'da_bias_act_bwd')
    return dx, dbias if need_dbias else None


def proto_shape_ok(rows, l, d, p):
    """da_proto_shape_ok restated: the shapes csrc/protopnet.hip takes."""
    return rows >= 1 and 1 <= l <= MAX_L and 32 <= d <= MAX_D and d % 32 == 0 and 2 <= p <= MAX_P and \
        rows * l * d < 2 ** 31 and rows * p * l < 2 ** 31


def proto_row_tile(l, p):
    """Rows of the map one block of the distance kernel takes at (L, P)."""
    return int(_H._lib.lib().da_proto_row_tile(l, p))


def _protos2d(protos, who):
    _H._f32(protos, 'protos')
    if protos.dim() == 3:
        if protos.shape[2] != 1:
            raise NotImplementedError('%s: the prototype layer is built for prototype kernel size 1, got %s' % (who, tuple(protos.shape)))
        return protos.view(protos.shape[0], protos.shape[1])
    if protos.dim() != 2:
        raise ValueError('%s: protos must be (P, D) or (P, D, 1), got %s' % (who, tuple(protos.shape)))
    return protos


def _zp(z, protos, who):
    if not (z.is_cuda and z.dtype == torch.float32 and z.dim() == 3 and z.is_contiguous() and z.data_ptr() % 16 == 0):
        raise ValueError('%s: z must be a contiguous float32 CUDA (rows, L, D) tensor, got %s %s' % (who, tuple(z.shape), z.dtype))
    p2 = _protos2d(protos, who)
    rows, l, d = z.shape
    p = p2.shape[0]
    if p2.shape[1] != d:
        raise ValueError('%s: protos %s do not have the map\'s %d channels' % (who, tuple(protos.shape), d))
    if not proto_shape_ok(rows, l, d, p):
        raise _H.HipError('%s: unsupported (rows, L, D, P) = (%d, %d, %d, %d): D %% 32 == 0 up to %d, 2 <= P <= %d, 1 <= L <= %d, '
                          'fewer than 2^31 elements' % (who, rows, l, d, p, MAX_D, MAX_P, MAX_L))
    return p2, rows, l, d, p


def proto_fwd(z, protos, want_dist=False):
    """z (rows, L, D), protos (P, D[, 1]) -> dist (rows, P, L) (None without want_dist), min_d (rows, P), arg (rows, P) int32
    (the lowest l attaining the minimum), sim (rows, P) = log((min_d + 1) / (min_d + 1e-4)).  The distance is the direct form
    sum_c (z - p)^2: exactly 0 for a prototype that is bitwise a patch."""
    p2, rows, l, d, p = _zp(z, protos, 'proto_fwd')
    dev = z.device
    dist = torch.empty((rows, p, l), device=dev, dtype=torch.float32) if want_dist else None
    min_d = torch.empty((rows, p), device=dev, dtype=torch.float32)
    arg = torch.empty((rows, p), device=dev, dtype=torch.int32)
    sim = torch.empty((rows, p), device=dev, dtype=torch.float32)
    _H._chk(_H._lib.lib().da_proto_fwd(_H._p(z), _H._p(p2), _H._p(dist), _H._p(min_d), _H._p(arg), _H._p(sim), rows, l, d, p,
                                       _H._stream()), 'da_proto_fwd')
    return dist, min_d, arg, sim


def proto_bwd(dsim, dmin, min_d, arg, z, protos, need_dz=True, dprotos=None, accumulate=False, need_dprotos=True):
    """Gradients of the prototype layer from the gradient on sim and / or on min_d (rows, P; either may be None):
    -> dz (rows, L, D), every element written (None without need_dz), dprotos shaped like protos (None without need_dprotos;
    ``dprotos``: the destination, written or -- accumulate -- added to)."""
    p2, rows, l, d, p = _zp(z, protos, 'proto_bwd')
    if dsim is None and dmin is None:
        raise ValueError('proto_bwd: needs the gradient on sim or on min_d')
    for t, name in ((dsim, 'dsim'), (dmin, 'dmin'), (min_d, 'min_d')):
        if t is not None and tuple(_H._f32(t, name).shape) != (rows, p):
            raise ValueError('proto_bwd: %s must be (rows, P) = (%d, %d), got %s' % (name, rows, p, tuple(t.shape)))
    if not (arg.is_cuda and arg.dtype == torch.int32 and arg.is_contiguous() and tuple(arg.shape) == (rows, p)):
        raise ValueError('proto_bwd: arg must be the int32 (rows, P) arg-min of proto_fwd')
    if not (need_dz or need_dprotos):
        return None, None
    L = _H._lib.lib()
    dz = torch.empty_like(z) if need_dz else None
    ws = None
    if need_dprotos:
        dprotos = _H._out(dprotos, protos.shape, torch.float32, z.device, accumulate, 'proto_bwd', strict=True)
        ws = torch.empty((max(L.da_proto_bwd_workspace(rows, d, p) // 4, 1),), device=z.device, dtype=torch.float32)
    _H._chk(L.da_proto_bwd(_H._p(dsim), _H._p(dmin), _H._p(min_d), _H._p(arg), _H._p(z), _H._p(p2), _H._p(dz),
                           _H._p(dprotos if need_dprotos else None), 1 if accumulate else 0, _H._p(ws), rows, l, d, p,
                           _H._stream()), 'da_proto_bwd')
    return dz, dprotos if need_dprotos else None


LossParts = ('loss', 'cls', 'cluster', 'separation', 'l1')


def ppnet_loss(logits, target, min_d, nb, num_prototypes, max_dist, clust_lambda, sep_lambda, want_grad=True, gscale=1.0,
               l1_weight=None, l1_mask=None):
    """ProtoPNetModel.calc_loss (train_ards_detector.py:1194-1247) and its gradients, without autograd: logits, target (B, 2),
    min_d (B, NB * P) -> parts (5,) = (total, cls, cluster, separation, l1), dlogits (B, 2), dmin_d (B, NB * P) (None without
    want_grad) and dW, the l1 term's gradient on ``l1_weight`` (None without it).  One launch; with ``l1_weight`` (use_l1: the
    last layer's weight; ``l1_mask`` = 1 - identity^T, shaped like it) 1e-4 * |W * mask|_1 is added to parts[0], stored in
    parts[4] and differentiated with stock torch ops on its 2 * K numbers.  gscale multiplies the gradients only."""
    _H._f32(logits, 'logits')
    _H._f32(target, 'target')
    _H._f32(min_d, 'min_d')
    b = logits.shape[0]
    p = int(num_prototypes)
    if logits.dim() != 2 or logits.shape[1] != 2 or tuple(target.shape) != (b, 2) or b < 1:
        raise ValueError('ppnet_loss: logits %s and target %s must be (B, 2)' % (tuple(logits.shape), tuple(target.shape)))
    if nb < 1 or p < 2 or p % 2 or p > MAX_P or tuple(min_d.shape) != (b, nb * p):
        raise ValueError('ppnet_loss: min_d %s must be (B, NB * P) = (%d, %d) with an even P in [2, %d]' %
                         (tuple(min_d.shape), b, nb * p, MAX_P))
    out = torch.empty((5,), device=logits.device, dtype=torch.float32)
    dlogits = torch.empty_like(logits) if want_grad else None
    dmin = torch.empty_like(min_d) if want_grad else None
    _H._chk(_H._lib.lib().da_ppnet_loss(_H._p(logits), _H._p(target), _H._p(min_d), b, nb, p, float(max_dist), float(clust_lambda),
                                        float(sep_lambda), float(gscale), _H._p(out), _H._p(dlogits), _H._p(dmin), _H._stream()),
            'da_ppnet_loss')
    dw = None
    if l1_weight is not None:
        wm = l1_weight.detach() * l1_mask
        l1 = wm.abs().sum()
        out[4] = l1
        out[0] += L1_COEF * l1
        if want_grad:
            dw = torch.sign(wm) * l1_mask * (L1_COEF * gscale)
    return out, dlogits, dmin, dw


def grad_add_decay_(g, p, weight_decay):
    """g += weight_decay * p in place (flat float32 CUDA ranges): Adam's L2 term, in front of clamp_adam_dev_."""
    if _H._f32(g, 'g').numel() != _H._f32(p, 'p').numel():
        raise ValueError('grad_add_decay_: g and p differ in size')
    _H._chk(_H._lib.lib().da_grad_add_decay(_H._p(g), _H._p(p), g.numel(), float(weight_decay), _H._stream()), 'da_grad_add_decay')
    return g


def _check_f32_path(who):
    if F_.conv_dtype() != 'f32' or F_.storage_dtype() != 'f32':
        raise NotImplementedError("%s runs with conv arithmetic 'f32' and float storage only (got %s / %s)"
                                  % (who, F_.conv_dtype(), F_.storage_dtype()))


class PointwiseConvFunction(Function):
    """Conv1d(kernel_size=1) WITHOUT its bias on a (rows, L, Ci) map, w (Co, Ci, 1): the existing fp32 GEMM conv path --
    forward, data gradient and weight gradient, the ``precise`` forms (an add-on layer of PPNet, model.py:164-170)."""

    @staticmethod
    def forward(ctx, x, w):
        _check_f32_path('PointwiseConvFunction')
        x = x.contiguous()
        ctx.save_for_backward(x, w)
        ctx.gt = F_._tgt(w)
        return F_._conv_fwd(x, w, 1, 0, precise=True)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        (tw,) = ctx.gt
        dy = dy.contiguous()
        dx = F_._conv_dgrad(dy, w, 1, 0, x.shape[1], precise=True) if ctx.needs_input_grad[0] else None
        dw = F_._wgrad(dy, x, 1, 1, 0, tw, precise=True) if ctx.needs_input_grad[1] else None
        return dx, dw


class BiasActFunction(Function):
    """y = act(x + bias): the bias and the ReLU / Sigmoid behind an add-on layer's 1x1 conv.  The bias gradient goes straight
    into the trainer's destination (``bias._da_grad``) where there is one."""

    @staticmethod
    def forward(ctx, x, bias, act):
        y = bias_act_fwd(x.contiguous(), bias, act)
        ctx.save_for_backward(y)
        ctx.act = act
        ctx.gt = F_._tgt(bias)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        (tb,) = ctx.gt
        need_b = ctx.needs_input_grad[1]
        direct = need_b and tb is not None
        dx, db = bias_act_bwd(dy.contiguous(), y, ctx.act, need_dx=ctx.needs_input_grad[0], dbias=tb if direct else None,
                              accumulate=direct and F_._acc(), need_dbias=need_b)
        return dx, None if direct else db, None


class PrototypeLayerFunction(Function):
    """z (rows, L, D), prototype_vectors (P, D, 1) -> sim (rows, P), min_d (rows, P): _l2_convolution in the direct form, the
    global min-pool and distance_2_similarity ('log') of PPNet.seq_forward (model.py:217-266) in one launch; the backward takes
    the gradients on both outputs (two launches and a fold)."""

    @staticmethod
    def forward(ctx, z, protos):
        z = z.contiguous()
        _, min_d, arg, sim = proto_fwd(z, protos)
        ctx.save_for_backward(z, protos, min_d, arg)
        ctx.gt = F_._tgt(protos)
        ctx.set_materialize_grads(False)
        return sim, min_d

    @staticmethod
    def backward(ctx, dsim, dmin):
        z, protos, min_d, arg = ctx.saved_tensors
        (tp,) = ctx.gt
        if dsim is None and dmin is None:
            return None, None
        need_p = ctx.needs_input_grad[1]
        direct = need_p and tp is not None
        dz, dp = proto_bwd(None if dsim is None else dsim.contiguous(), None if dmin is None else dmin.contiguous(), min_d, arg,
                           z, protos, need_dz=ctx.needs_input_grad[0], dprotos=tp if direct else None,
                           accumulate=direct and F_._acc(), need_dprotos=need_p)
        return dz, None if direct else dp


class LastLayerFunction(Function):
    """PPNet.last_layer, Linear(K, 2, bias=False): da_linear2_* with a null bias pointer."""

    @staticmethod
    def forward(ctx, flat, w):
        flat = flat.contiguous()
        if flat.shape[1] % 4:
            raise _H.HipError('last_layer: %d inputs are not a multiple of 4' % flat.shape[1])
        ctx.save_for_backward(flat, w)
        ctx.gt = F_._tgt(w)
        return _H.linear2_fwd(flat, w, None)

    @staticmethod
    def backward(ctx, dlogits):
        flat, w = ctx.saved_tensors
        (tw,) = ctx.gt
        need_w = ctx.needs_input_grad[1]
        direct = need_w and tw is not None
        dflat = torch.empty_like(flat) if ctx.needs_input_grad[0] else None
        dw = (tw if direct else torch.empty_like(w)) if need_w else None
        b, k = flat.shape
        _H._chk(_H._lib.lib().da_linear2_bwd(_H._p(dlogits.contiguous()), _H._p(flat), _H._p(w), _H._p(dflat), _H._p(dw), None, b, k,
                                             1 if direct and F_._acc() else 0, _H._stream()), 'da_linear2_bwd')
        return dflat, None if direct else dw


class PPNetLossFunction(Function):
    """calc_loss as one autograd node: (logits, min_d, target) -> parts (5,); parts[0] is the loss to call backward() on (the
    kernel computed both gradients in the forward's launch; the backward scales them by the upstream gradient on parts[0])."""

    @staticmethod
    def forward(ctx, logits, min_d, target, nb, num_prototypes, max_dist, clust_lambda, sep_lambda):
        out, dlogits, dmin, _ = ppnet_loss(logits.contiguous(), target.contiguous(), min_d.contiguous(), nb, num_prototypes,
                                           max_dist, clust_lambda, sep_lambda)
        ctx.save_for_backward(dlogits, dmin)
        return out

    @staticmethod
    def backward(ctx, dout):
        dlogits, dmin = ctx.saved_tensors
        g = dout[0]
        return dlogits * g, dmin * g, None, None, None, None, None, None
