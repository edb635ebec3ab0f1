"""The pooled stages and the feature layout of the VGG backbones (reference models/vgg.py:37-50 make_layers, :15,20-24) as
wrappers of the C ABI (``da_bn_relu_maxpool2_*``, ``da_bn_mean_bias``, ``da_adaptive_avgpool_flat_*``; kernels in csrc/vgg.hip).
Reached as ``hip_ops.bn_relu_maxpool2_fwd`` ...; same conventions as the other wrappers: contiguous float32 CUDA operands, the
current stream, no host synchronisation, shapes checked here so that an unsupported one raises with the shape before anything
is launched."""
import torch

from . import hip_ops as _H


def _vp_y(y, R, who):
    _H._float_storage_only(who, 'the VGG stages run')
    _H._rlc(y, 'y')
    rows, l, c, w, wn = _H._bn_win(y, R)
    if c % 32 or l < 2 or rows * l * c >= 1 << 32:
        raise ValueError('%s: y %s needs C %% 32 == 0, L >= 2 and fewer than 2^32 elements' % (who, tuple(y.shape)))
    return rows, l, c, w, wn


def _vp_stats(mean, invstd, w, c, who):
    for t in (mean, invstd):
        if tuple(_H._f32(t, 'statistics').shape) != (w, c):
            raise ValueError('%s: mean / invstd must be (W, C) = (%d, %d)' % (who, w, c))


def _vp_affine(gamma, beta, c, who):
    for t in (gamma, beta):
        if tuple(_H._f32(t, 'gamma / beta').shape) != (c,):
            raise ValueError('%s: gamma / beta must be (%d,)' % (who, c))


def vgg_stats(y, R, eps=1e-5):
    """Per-window statistics of a stage's conv output: one launch where the shape has the single-pass geometry
    (bn_stats_fused), else partial + merge (the first stages: windows of up to 20 x 224 positions).  -> mean, invstd (W, C)."""
    rows, l, c, w, wn = _vp_y(y, R, 'vgg_stats')
    if w and _H.bn_single_pass(w, wn, c):
        mean, invstd = _H._bn_stats_pair(w, c, y.device)
        _H.bn_stats_fused(y, R, mean, invstd, eps)
        return mean, invstd
    return _H.bn_stats(y, R, eps)


def bn_relu_maxpool2_fwd(y, R, mean, invstd, gamma, beta, out=None):
    """-> out (rows, L // 2, C) = MaxPool1d(2, 2)(relu(bn(y))); the activated full-resolution map is never stored."""
    rows, l, c, w, wn = _vp_y(y, R, 'bn_relu_maxpool2_fwd')
    _vp_stats(mean, invstd, w, c, 'bn_relu_maxpool2_fwd')
    _vp_affine(gamma, beta, c, 'bn_relu_maxpool2_fwd')
    out = _H._out(out, (rows, l // 2, c), torch.float32, y.device, False, 'bn_relu_maxpool2_fwd', strict=True)
    _H._chk(_H._lib.lib().da_bn_relu_maxpool2_fwd(_H._p(y), c, _H._p(out), rows, R, l, c, _H._p(mean), _H._p(invstd), _H._p(gamma),
                                                  _H._p(beta), _H._stream()), 'da_bn_relu_maxpool2_fwd')
    return out


def bn_relu_maxpool2_bwd(dout, y, R, mean, invstd, gamma, beta, out=None):
    """The backward of bn_relu_maxpool2_fwd through pool, ReLU and BatchNorm: dout (rows, L // 2, C) -> dy (rows, L, C),
    ds (2, W, C) (the window sums bn_param_grad_multi folds into dgamma / dbeta)."""
    rows, l, c, w, wn = _vp_y(y, R, 'bn_relu_maxpool2_bwd')
    _vp_stats(mean, invstd, w, c, 'bn_relu_maxpool2_bwd')
    _vp_affine(gamma, beta, c, 'bn_relu_maxpool2_bwd')
    _H._bn_same(_H._rlc(dout, 'dout'), (rows, l // 2, c), 'dout')
    dy = _H._out(out, y.shape, torch.float32, y.device, False, 'bn_relu_maxpool2_bwd', strict=True)
    ds = _H._bn_sums(w, c, y.device)
    L = _H._lib.lib()
    ws = torch.empty((max(L.da_bn_relu_maxpool2_bwd_workspace(rows, R, l, c) // 4, 1),), device=y.device, dtype=torch.float32)
    _H._chk(L.da_bn_relu_maxpool2_bwd(_H._p(dout), _H._p(y), c, _H._p(dy), _H._p(ds), _H._p(ws), rows, R, l, c, _H._p(mean),
                                      _H._p(invstd), _H._p(gamma), _H._p(beta), _H._stream()), 'da_bn_relu_maxpool2_bwd')
    return dy, ds


def bn_mean_bias(mean, bias, dbias=None):
    """-> mean + bias per window (W, C): the batch mean of ``conv + bias`` when ``mean`` is the one of the stored, bias-free
    conv output -- what bn_running_multi takes so that running_mean is the reference's.  dbias: a (C,) destination that
    receives exact zeros (the gradient of a conv bias in front of a train-mode BatchNorm), written by the same launch."""
    w, c = _H._f32(mean, 'mean').shape
    if tuple(_H._f32(bias, 'bias').shape) != (c,) or (dbias is not None and tuple(_H._f32(dbias, 'dbias').shape) != (c,)):
        raise ValueError('bn_mean_bias: bias / dbias must be (%d,)' % c)
    out = torch.empty_like(mean)
    _H._chk(_H._lib.lib().da_bn_mean_bias(_H._p(mean), _H._p(bias), _H._p(out), w, c, _H._p(dbias), _H._stream()), 'da_bn_mean_bias')
    return out


def adaptive_avgpool_flat_fwd(x, lout, out=None):
    """AdaptiveAvgPool1d(lout) + ``view(rows, -1)``: x (rows, L, C) -> (rows, C * lout) float, channel slowest."""
    _H._float_storage_only('adaptive_avgpool_flat_fwd')
    rows, lin, c = _H._rlc(x, 'x').shape
    if lout < 1 or lin < 1 or rows * max(lin, lout) * c >= 1 << 32:
        raise ValueError('adaptive_avgpool_flat_fwd: x %s -> %d positions is not served' % (tuple(x.shape), lout))
    feat = _H._out(out, (rows, c * lout), torch.float32, x.device, False, 'adaptive_avgpool_flat_fwd', strict=True)
    _H._chk(_H._lib.lib().da_adaptive_avgpool_flat_fwd(_H._p(x), _H._p(feat), rows, lin, lout, c, _H._stream()),
            'da_adaptive_avgpool_flat_fwd')
    return feat


def adaptive_avgpool_flat_bwd(dfeat, lin, lout, out=None):
    """dfeat (rows, C * lout) -> dx (rows, lin, C)."""
    _H._float_storage_only('adaptive_avgpool_flat_bwd')
    _H._f32(dfeat, 'dfeat')
    if dfeat.dim() != 2 or lout < 1 or lin < 1 or dfeat.shape[1] % lout:
        raise ValueError('adaptive_avgpool_flat_bwd: dfeat must be (rows, C * %d), got %s' % (lout, tuple(dfeat.shape)))
    rows, c = dfeat.shape[0], dfeat.shape[1] // lout
    if rows * max(lin, lout) * c >= 1 << 32:
        raise ValueError('adaptive_avgpool_flat_bwd: more than 2^32 elements')
    dx = _H._out(out, (rows, lin, c), torch.float32, dfeat.device, False, 'adaptive_avgpool_flat_bwd', strict=True)
    _H._chk(_H._lib.lib().da_adaptive_avgpool_flat_bwd(_H._p(dfeat), _H._p(dx), rows, lin, lout, c, _H._stream()),
            'da_adaptive_avgpool_flat_bwd')
    return dx
