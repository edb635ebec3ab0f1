"""One Block of the cnn_transformer head (reference models/transformer.py:59-88) as wrappers of the C ABI
(``da_tfm_block_fwd`` / ``_bwd`` / ``_pgrad``; kernels in csrc/transformer.hip).  Reached as ``hip_ops.tfm_block_fwd`` ...;
same conventions as the other wrappers: contiguous float32 CUDA operands, the current stream, no host synchronisation,
shapes checked here so that an unsupported one raises with the shape before anything is launched."""
import ctypes

import torch

from . import hip_ops as _H

TFM_PARAMS = 16        # q / k / v / joint_linear (weight, bias), attention_norm, ff.0, ff.2, ff_norm: named_parameters() order


def tfm_check_shape(t, d, h, who='transformer block'):
    """The shapes the block kernels take (include/deepards_hip.h); anything else raises before a launch."""
    if not (1 <= t <= 64 and 64 <= d <= 2048 and d % 64 == 0 and 8 <= h <= 64 and h % 8 == 0):
        raise ValueError('%s: unsupported shape (T, D, H) = (%d, %d, %d): T must lie in [1, 64], D be a multiple of 64 up '
                         'to 2048, H a multiple of 8 in [8, 64] (4 heads)' % (who, t, d, h))


def tfm_block_form(t, d, h):
    """-> (tokens_fwd, tokens_bwd, lds_fwd, lds_bwd): tokens a wave takes per pass and bytes of dynamic LDS of the forward
    and the data backward at (T, D, H), from the expressions the launches use (``da_tfm_block_form``); launches nothing."""
    tfm_check_shape(t, d, h)
    tf, tb, lf, lb = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t(), ctypes.c_size_t()
    _H._chk(_H._lib.lib().da_tfm_block_form(t, d, h, ctypes.byref(tf), ctypes.byref(tb), ctypes.byref(lf), ctypes.byref(lb)),
            'da_tfm_block_form')
    return tf.value, tb.value, lf.value, lb.value


def _tfm_args(x, params, drop):
    _H._f32(x, 'x')
    if x.dim() != 3 or len(params) != TFM_PARAMS:
        raise ValueError('transformer block: x must be (B, T, D) with %d parameters' % TFM_PARAMS)
    b, t, d = x.shape
    h = params[0].shape[0]
    tfm_check_shape(t, d, h)
    shapes = [(h, d), (h,)] * 3 + [(d, h), (d,), (d,), (d,), (h, d), (h,), (d, h), (d,), (d,), (d,)]
    for q, shp in zip(params, shapes):
        if tuple(q.shape) != shp or not (q.is_cuda and q.dtype == torch.float32 and q.is_contiguous()):
            raise ValueError('transformer block: parameter of shape %s where %s (contiguous float32 CUDA) belongs' %
                             (tuple(q.shape), shp))
    seed, salt1, salt2, p = drop if drop is not None else (None, 0, 0, 0.0)
    if not 0.0 <= p < 1.0 or (p > 0 and not (seed is not None and seed.is_cuda and seed.dtype == torch.int64)):
        raise ValueError('transformer block: dropout needs 0 <= p < 1 and a one-element int64 CUDA seed')
    ptrs = (ctypes.c_void_p * TFM_PARAMS)(*[q.data_ptr() for q in params])
    return b, t, d, h, ptrs, (_H._p(seed) if p > 0 else None, int(salt1), int(salt2), float(p))


def tfm_block_fwd(x, params, drop=None):
    """x (B, T, D), params: the 16 tensors of one Block, drop = (seed, salt1, salt2, p) or None ->
    y (B, T, D), saved = (q, k, v (B, T, H), weights (B, 4, T, T), hid (B, T, H), stats (B, T, 4))."""
    b, t, d, h, ptrs, dr = _tfm_args(x, params, drop)
    mk = lambda *shape: torch.empty(shape, device=x.device, dtype=torch.float32)
    y, qkv, aw, hid, stats = mk(b, t, d), mk(3, b, t, h), mk(b, 4, t, t), mk(b, t, h), mk(b, t, 4)
    _H._chk(_H._lib.lib().da_tfm_block_fwd(_H._p(x), ptrs, _H._p(y), _H._p(qkv[0]), _H._p(qkv[1]), _H._p(qkv[2]), _H._p(aw), _H._p(hid), _H._p(stats),
                                     b, t, d, h, *dr, _H._stream()), 'da_tfm_block_fwd')
    return y, (qkv[0], qkv[1], qkv[2], aw, hid, stats)


def tfm_block_bwd(dy, x, params, saved, drop=None):
    """-> dx (B, T, D), work = (dq, dk, dv, dhid, wv (B, T, H), da1, da2 (B, T, D)) for tfm_block_pgrad."""
    b, t, d, h, ptrs, dr = _tfm_args(x, params, drop)
    _H._f32(dy, 'dy')
    if dy.shape != x.shape:
        raise ValueError('transformer block: dy %s for x %s' % (tuple(dy.shape), tuple(x.shape)))
    q, k, v, aw, hid, stats = saved
    mk = lambda *shape: torch.empty(shape, device=x.device, dtype=torch.float32)
    dx, th, td = mk(b, t, d), mk(5, b, t, h), mk(2, b, t, d)
    _H._chk(_H._lib.lib().da_tfm_block_bwd(_H._p(dy), _H._p(x), ptrs, _H._p(q), _H._p(k), _H._p(v), _H._p(aw), _H._p(hid), _H._p(stats), _H._p(dx), _H._p(th[0]),
                                     _H._p(th[1]), _H._p(th[2]), _H._p(th[3]), _H._p(td[0]), _H._p(td[1]), _H._p(th[4]), b, t, d, h, *dr,
                                     _H._stream()), 'da_tfm_block_bwd')
    return dx, (th[0], th[1], th[2], th[3], th[4], td[0], td[1])


def tfm_block_pgrad(dy, x, params, saved, work, grads=None, accumulate=False, drop=None):
    """The 16 parameter gradients of the block, in the order of ``params``: into ``grads`` (16 destinations of the
    parameters' shapes; accumulate adds) or new tensors."""
    b, t, d, h, ptrs, dr = _tfm_args(x, params, drop)
    if grads is None:
        if accumulate:
            raise ValueError('tfm_block_pgrad: accumulate needs grads')
        grads = [torch.empty_like(q) for q in params]
    if len(grads) != TFM_PARAMS or any(g.shape != q.shape or not (g.is_cuda and g.dtype == torch.float32 and g.is_contiguous())
                                       for g, q in zip(grads, params)):
        raise ValueError('tfm_block_pgrad: grads must be %d contiguous float32 CUDA tensors of the parameters\' shapes' % TFM_PARAMS)
    _, _, _, _, hid, stats = saved
    dq, dk, dv, dhid, wv, da1, da2 = work
    gp = (ctypes.c_void_p * TFM_PARAMS)(*[g.data_ptr() for g in grads])
    _H._chk(_H._lib.lib().da_tfm_block_pgrad(_H._p(dy), _H._p(x), ptrs, _H._p(hid), _H._p(stats), _H._p(wv), _H._p(dq), _H._p(dk), _H._p(dv), _H._p(dhid),
                                       _H._p(da1), _H._p(da2), gp, 1 if accumulate else 0, b, t, d, h, *dr, _H._stream()),
         'da_tfm_block_pgrad')
    return list(grads)
