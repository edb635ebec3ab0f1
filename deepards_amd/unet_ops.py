"""The UNet's layers between its convs (reference models/unet.py: bias + ReLU without BatchNorm, ReLU + MaxPool1d(2) with the
full-resolution map kept as a skip, ReLU + Upsample(scale_factor=2, 'linear', align_corners=True), Conv1d(64, 1, 1) + MSELoss) as
wrappers of the C ABI (``da_unet_*``; kernels in csrc/unet.hip).  Reached as ``hip_ops.unet_bias_relu`` ...; same conventions as
the other wrappers: float32 CUDA operands, the current stream, no host synchronisation, shapes checked here so that an
unsupported one raises with the shape before anything is launched.

An operand called a *slice* may be C channels of a pitched (rows, L, ld) buffer (``hip_ops._pv``): the concat of the UNet is
never copied -- the skip conv and the upsample write the two channel ranges of one buffer.  No pool decision is stored: the
backward re-derives the winner from the stored activation (the second member only when strictly greater)."""
import collections
import ctypes

import torch

from . import hip_ops as _H

OUT_C = 64                                   # channels in front of conv_last (Conv1d(64, 1, 1))
OPS = ('bias_relu', 'bias_relu_pool2_fwd', 'relu_upsample2_fwd', 'relu_upsample2_bwd', 'pool2_skip_bwd', 'relu_bwd', 'out_fwd',
       'out_bwd')                            # da_unet_plan's op codes, in the header's order

UNetPlan = collections.namedtuple('UNetPlan', 'blocks workspace')


def unet_plan(op, rows, l, c, ld=None):
    """Launch geometry of entry point ``op`` (a name of OPS) on a (rows, l, c) map whose widest operand has pitch ld (None: c);
    launches nothing.  ``l`` as the entry point takes it: the pool's full-resolution length, the upsample's low-resolution one.
    -> UNetPlan(blocks of 256 threads, workspace bytes), or HipError for a shape that is not taken."""
    b, ws = ctypes.c_int(), ctypes.c_size_t()
    args = (OPS.index(op), int(rows), int(l), int(c), int(c if ld is None else ld))
    if any(not -2 ** 31 <= a < 2 ** 31 for a in args) or \
            _H._lib.lib().da_unet_plan(*args, ctypes.byref(b), ctypes.byref(ws)) != 0:
        raise _H.HipError('unet_plan: no launch of %s for (rows, L, C, ld) = %s' % (op, args[1:]))
    return UNetPlan(b.value, ws.value)


def _f32_only(who):
    _H._float_storage_only(who, 'the UNet layers run')


def _slice(t, who, name, even=False):
    """-> (rows, L, C, ld) of a channel slice; the shape rules of csrc/unet.hip."""
    ld = _H._pv(t, name)
    rows, l, c = t.shape
    if c % 32 or rows < 1 or (even and l % 2) or rows * l * ld >= 1 << 32:
        raise ValueError('%s: %s %s needs C %% 32 == 0%s and fewer than 2^32 elements' %
                         (who, name, tuple(t.shape), ', an even L' if even else ''))
    return rows, l, c, ld


def _bias(bias, c, who):
    if tuple(_H._f32(bias, 'bias').shape) != (c,):
        raise ValueError('%s: bias must be (%d,)' % (who, c))
    return bias


def _dense(t, shape, who, name):
    if tuple(_H._rlc(t, name).shape) != tuple(shape):
        raise ValueError('%s: %s must be %s, got %s' % (who, name, tuple(shape), tuple(t.shape)))
    return t


def unet_bias_relu(y, bias):
    """y (a slice) = relu(y + bias) in place -> y."""
    _f32_only('unet_bias_relu')
    rows, l, c, ld = _slice(y, 'unet_bias_relu', 'y')
    _H._chk(_H._lib.lib().da_unet_bias_relu(_H._p(y), ld, _H._p(_bias(bias, c, 'unet_bias_relu')), rows, l, c, _H._stream()),
            'da_unet_bias_relu')
    return y


def unet_bias_relu_pool2_fwd(y, bias, out=None):
    """y (a slice, even L) = relu(y + bias) in place -- the skip -- and -> pooled (rows, L // 2, C) = MaxPool1d(2) of it."""
    who = 'unet_bias_relu_pool2_fwd'
    _f32_only(who)
    rows, l, c, ld = _slice(y, who, 'y', even=True)
    pooled = _H._out(out, (rows, l // 2, c), torch.float32, y.device, False, who, strict=True)
    _H._chk(_H._lib.lib().da_unet_bias_relu_pool2_fwd(_H._p(y), ld, _H._p(_bias(bias, c, who)), _H._p(pooled), rows, l, c,
                                                      _H._stream()), 'da_unet_bias_relu_pool2_fwd')
    return pooled


def unet_relu_upsample2_fwd(y, bias, out):
    """out (a slice, (rows, 2 L, C)) = Upsample(x2, linear, align_corners=True)(relu(y + bias)); y (rows, L, C) contiguous; the
    activated low-resolution map is never stored."""
    who = 'unet_relu_upsample2_fwd'
    _f32_only(who)
    rows, l2, c, ld = _slice(out, who, 'out')
    _dense(y, (rows, l2 // 2, c), who, 'y')
    if l2 % 2:
        raise ValueError('%s: out %s must have twice the positions of y' % (who, tuple(out.shape)))
    _H._chk(_H._lib.lib().da_unet_relu_upsample2_fwd(_H._p(y), _H._p(_bias(bias, c, who)), _H._p(out), ld, rows, l2 // 2, c,
                                                     _H._stream()), 'da_unet_relu_upsample2_fwd')
    return out


def unet_relu_upsample2_bwd(d, y, bias, out=None):
    """d (a slice, (rows, 2 L, C)): the gradient at the upsampled map -> dy (rows, L, C), the gradient at y (masked by
    y + bias > 0)."""
    who = 'unet_relu_upsample2_bwd'
    _f32_only(who)
    rows, l2, c, ld = _slice(d, who, 'd', even=True)
    _dense(y, (rows, l2 // 2, c), who, 'y')
    dy = _H._out(out, y.shape, torch.float32, y.device, False, who, strict=True)
    _H._chk(_H._lib.lib().da_unet_relu_upsample2_bwd(_H._p(d), ld, _H._p(y), _H._p(_bias(bias, c, who)), _H._p(dy), rows, l2 // 2, c,
                                                     _H._stream()), 'da_unet_relu_upsample2_bwd')
    return dy


def unet_pool2_skip_bwd(dpooled, dskip, a, out=None):
    """The two gradients that reach a skip map a (a slice, the stored relu output): dskip (a slice of the concat's gradient) and
    dpooled (rows, L // 2, C) through the pool -> dy (rows, L, C), masked by a > 0."""
    who = 'unet_pool2_skip_bwd'
    _f32_only(who)
    rows, l, c, lda = _slice(a, who, 'a', even=True)
    if _slice(dskip, who, 'dskip', even=True)[:3] != (rows, l, c):
        raise ValueError('%s: dskip %s does not match a %s' % (who, tuple(dskip.shape), tuple(a.shape)))
    _dense(dpooled, (rows, l // 2, c), who, 'dpooled')
    dy = _H._out(out, (rows, l, c), torch.float32, a.device, False, who, strict=True)
    _H._chk(_H._lib.lib().da_unet_pool2_skip_bwd(_H._p(dpooled), _H._p(dskip), _H._pv(dskip, 'dskip'), _H._p(a), lda, _H._p(dy), rows,
                                                 l, c, _H._stream()), 'da_unet_pool2_skip_bwd')
    return dy


def unet_relu_bwd(dout, a, out=None):
    """-> dy = dout [a > 0]; a may be a slice; ``out`` may be dout itself (in place)."""
    who = 'unet_relu_bwd'
    _f32_only(who)
    rows, l, c, lda = _slice(a, who, 'a')
    _dense(dout, (rows, l, c), who, 'dout')
    dy = _H._out(out, (rows, l, c), torch.float32, a.device, False, who, strict=True)
    _H._chk(_H._lib.lib().da_unet_relu_bwd(_H._p(dout), _H._p(a), lda, _H._p(dy), rows, l, c, _H._stream()), 'da_unet_relu_bwd')
    return dy


def _out_operands(a, w, who):
    _f32_only(who)
    rows, l, c = _H._rlc(a, 'a').shape
    if c != OUT_C or rows < 1 or l < 1 or rows * l * c >= 1 << 32:
        raise ValueError('%s: a %s must be a (rows, L, %d) map of fewer than 2^32 elements' % (who, tuple(a.shape), OUT_C))
    if tuple(_H._f32(w, 'w').shape) != (1, c, 1):
        raise ValueError('%s: w must be (1, %d, 1)' % (who, c))
    return rows, l


def unet_out_fwd(a, w, bias, x):
    """recon = Conv1d(64, 1, 1)(a) and the MSE against x (rows, L).  -> recon (rows, L), dr = d loss / d recon, loss (1,)."""
    rows, l = _out_operands(a, w, 'unet_out_fwd')
    if tuple(_H._f32(x, 'x').shape) != (rows, l) or tuple(_H._f32(bias, 'bias').shape) != (1,):
        raise ValueError('unet_out_fwd: x must be (rows, L) = (%d, %d) and bias (1,)' % (rows, l))
    recon, dr = torch.empty_like(x), torch.empty_like(x)
    loss = torch.empty((1,), device=x.device, dtype=torch.float32)
    ws = torch.empty((max(unet_plan('out_fwd', rows, l, OUT_C).workspace // 4, 1),), device=x.device, dtype=torch.float32)
    _H._chk(_H._lib.lib().da_unet_out_fwd(_H._p(a), _H._p(w), _H._p(bias), _H._p(x), _H._p(recon), _H._p(dr), _H._p(ws), _H._p(loss),
                                          rows, l, _H._stream()), 'da_unet_out_fwd')
    return recon, dr, loss


def unet_out_bwd(dr, a, w, dw=None, db=None, accumulate=False):
    """-> dy (rows, L, 64) = dr w [a > 0] (the gradient at the conv output behind a), dw (1, 64, 1), db (1,); with destinations
    the two parameter gradients are written there, or -- accumulate -- added."""
    rows, l = _out_operands(a, w, 'unet_out_bwd')
    if tuple(_H._f32(dr, 'dr').shape) != (rows, l):
        raise ValueError('unet_out_bwd: dr must be (rows, L) = (%d, %d)' % (rows, l))
    dw = _H._out(dw, (1, OUT_C, 1), torch.float32, a.device, accumulate, 'unet_out_bwd', strict=True)
    db = _H._out(db, (1,), torch.float32, a.device, accumulate, 'unet_out_bwd', strict=True)
    dy = torch.empty_like(a)
    ws = torch.empty((max(unet_plan('out_bwd', rows, l, OUT_C).workspace // 4, 1),), device=a.device, dtype=torch.float32)
    _H._chk(_H._lib.lib().da_unet_out_bwd(_H._p(dr), _H._p(a), _H._p(w), _H._p(dy), _H._p(dw), _H._p(db), _H._p(ws), rows, l,
                                          1 if accumulate else 0, _H._stream()), 'da_unet_out_bwd')
    return dy, dw, db
