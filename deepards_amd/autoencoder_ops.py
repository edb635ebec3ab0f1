"""The autoencoder's own layers (reference models/autoencoder_cnn.py: BatchNorm1d + MaxPool1d(2, return_indices), MaxUnpool1d(2),
ConvTranspose1d(64, 1, 3, padding=1) + MSELoss) as wrappers of the C ABI (``da_bn_maxpool2_idx_*``, ``da_unpool2_*``,
``da_ae_out_*``; kernels in csrc/autoencoder.hip).  Reached as ``hip_ops.bn_maxpool2_idx_fwd`` ...; same conventions as the
other wrappers: contiguous float32 CUDA operands, the current stream, no host synchronisation, shapes checked here so that an
unsupported one raises with the shape before anything is launched.

A pool decision is one bit per pooled element, set where the SECOND member of the pair won; 32 channels to a word, word
((row Lo + j) C + c) / 32, bit c % 32, carried as an int32 tensor of (rows, Lo, C / 32).  ``sel_from_bool`` / ``sel_to_bool``
convert between that packing and (N, C, Lo) bool arrays (tests/tools/ae_ref.py's layout) in plain torch, on any device."""
import collections
import ctypes

import torch

from . import hip_ops as _H

OUT_C = 64                                   # channels in front of the output stage (conv_up4: ConvTranspose1d(64, 1))

PoolPlan = collections.namedtuple('PoolPlan', 'chunks chunk_pairs workspace')


# ---- the decision bits ---------------------------------------------------------------------------------------------------------
def sel_from_bool(sel):
    """(N, C, Lo) bool (True: the second member of the pair won) -> (N, Lo, C / 32) int32 words."""
    sel = torch.as_tensor(sel)
    if sel.dim() != 3 or sel.shape[1] % 32:
        raise ValueError('sel_from_bool: (N, C, Lo) decisions with C %% 32 == 0 expected, got %s' % (tuple(sel.shape),))
    n, c, lo = sel.shape
    bits = sel.to(torch.bool).permute(0, 2, 1).reshape(n, lo, c // 32, 32).to(torch.int64)
    words = (bits << torch.arange(32, device=sel.device, dtype=torch.int64)).sum(dim=-1)
    words = torch.where(words >= 1 << 31, words - (1 << 32), words)               # (the int32 with the same 32 bits)
    return words.to(torch.int32).contiguous()


def sel_to_bool(words, c=None):
    """(N, Lo, C / 32) int32 words -> (N, C, Lo) bool."""
    words = torch.as_tensor(words)
    if words.dim() != 3 or words.dtype != torch.int32 or (c is not None and words.shape[2] * 32 != c):
        raise ValueError('sel_to_bool: (N, Lo, C / 32) int32 words expected, got %s %s' % (tuple(words.shape), words.dtype))
    n, lo, wpp = words.shape
    bits = (words.to(torch.int64).unsqueeze(-1) >> torch.arange(32, device=words.device, dtype=torch.int64)) & 1
    return bits.reshape(n, lo, wpp * 32).permute(0, 2, 1).to(torch.bool).contiguous()


def _sel(sel, rows, lo, c, who, name='sel'):
    if not (sel.is_cuda and sel.dtype == torch.int32 and sel.is_contiguous() and tuple(sel.shape) == (rows, lo, c // 32)):
        raise ValueError('%s: %s must be contiguous int32 CUDA words (rows, Lo, C / 32) = (%d, %d, %d), got %s %s' %
                         (who, name, rows, lo, c // 32, tuple(sel.shape), sel.dtype))
    return sel


# ---- BatchNorm + MaxPool1d(2) with its decisions ---------------------------------------------------------------------------------
def _pool_y(y, R, who):
    _H._float_storage_only(who, 'the autoencoder stages run')
    _H._rlc(y, 'y')
    rows, l, c, w, wn = _H._bn_win(y, R)
    if c % 32 or l < 2 or l % 2 or rows < 1 or rows * l * c >= 1 << 32:
        raise ValueError('%s: y %s needs C %% 32 == 0, an even L >= 2 and fewer than 2^32 elements' % (who, tuple(y.shape)))
    return rows, l, c, w, wn


def _pool_params(mean, invstd, gamma, beta, w, c, who):
    for t in (mean, invstd):
        if tuple(_H._f32(t, 'statistics').shape) != (w, c):
            raise ValueError('%s: mean / invstd must be (W, C) = (%d, %d)' % (who, w, c))
    for t in (gamma, beta):
        if tuple(_H._f32(t, 'gamma / beta').shape) != (c,):
            raise ValueError('%s: gamma / beta must be (%d,)' % (who, c))


def bn_maxpool2_idx_plan(rows, R, l, c):
    """Chunk geometry of bn_maxpool2_idx_bwd on a (rows, l, c) map in windows of R rows; launches nothing.  Chunk p of a window
    holds its pairs [p chunk_pairs, min((p + 1) chunk_pairs, R l / 2)).  -> PoolPlan, or HipError for a shape that is not taken."""
    p, ch, ws = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
    args = (int(rows), int(R), int(l), int(c))
    if any(not -2 ** 31 <= a < 2 ** 31 for a in args) or \
            _H._lib.lib().da_bn_maxpool2_idx_plan(*args, ctypes.byref(p), ctypes.byref(ch), ctypes.byref(ws)) != 0:
        raise _H.HipError('bn_maxpool2_idx_plan: no launch for (rows, R, L, C) = (%d, %d, %d, %d)' % args)
    return PoolPlan(p.value, ch.value, ws.value)


def bn_maxpool2_idx_fwd(y, R, mean, invstd, gamma, beta, sel_in=None, out=None, sel=None):
    """-> (out (rows, L // 2, C), sel words): MaxPool1d(2, return_indices)(bn(y)); bn(y) is never stored.  sel_in: the decisions
    to take instead of deciding (teacher forcing) -- returned as they are unless a ``sel`` destination asks for a copy."""
    who = 'bn_maxpool2_idx_fwd'
    rows, l, c, w, wn = _pool_y(y, R, who)
    _pool_params(mean, invstd, gamma, beta, w, c, who)
    lo = l // 2
    if sel_in is not None:
        _sel(sel_in, rows, lo, c, who, 'sel_in')
    if sel is not None:
        _sel(sel, rows, lo, c, who)
    elif sel_in is None:
        sel = torch.empty((rows, lo, c // 32), device=y.device, dtype=torch.int32)
    out = _H._out(out, (rows, lo, c), torch.float32, y.device, False, who, strict=True)
    _H._chk(_H._lib.lib().da_bn_maxpool2_idx_fwd(_H._p(y), c, _H._p(out), _H._p(sel), _H._p(sel_in), rows, R, l, c, _H._p(mean),
                                                 _H._p(invstd), _H._p(gamma), _H._p(beta), _H._stream()), 'da_bn_maxpool2_idx_fwd')
    return out, (sel if sel is not None else sel_in)


def bn_maxpool2_idx_bwd(dout, sel, y, R, mean, invstd, gamma, beta, out=None):
    """The backward of bn_maxpool2_idx_fwd through the pool and BatchNorm: dout (rows, L // 2, C) -> dy (rows, L, C),
    ds (2, W, C) (the window sums bn_param_grad_multi folds into dgamma / dbeta)."""
    who = 'bn_maxpool2_idx_bwd'
    rows, l, c, w, wn = _pool_y(y, R, who)
    _pool_params(mean, invstd, gamma, beta, w, c, who)
    _H._bn_same(_H._rlc(dout, 'dout'), (rows, l // 2, c), 'dout')
    _sel(sel, rows, l // 2, c, who)
    plan = bn_maxpool2_idx_plan(rows, R, l, c)
    dy = _H._out(out, y.shape, torch.float32, y.device, False, who, strict=True)
    ds = _H._bn_sums(w, c, y.device)
    ws = torch.empty((max(plan.workspace // 4, 1),), device=y.device, dtype=torch.float32)
    _H._chk(_H._lib.lib().da_bn_maxpool2_idx_bwd(_H._p(dout), _H._p(sel), _H._p(y), c, _H._p(dy), _H._p(ds), _H._p(ws), rows, R, l, c,
                                                 _H._p(mean), _H._p(invstd), _H._p(gamma), _H._p(beta), _H._stream()),
            'da_bn_maxpool2_idx_bwd')
    return dy, ds


# ---- MaxUnpool1d(2) --------------------------------------------------------------------------------------------------------------
def _unpool_v(v, who, name, div=1):
    _H._float_storage_only(who, 'the autoencoder stages run')
    rows, l, c = _H._rlc(v, name).shape
    if c % 32 or l < div or l % div or rows < 1 or rows * l * c * (2 // div) >= 1 << 32:
        raise ValueError('%s: %s %s needs C %% 32 == 0 and fewer than 2^32 elements' % (who, name, tuple(v.shape)))
    return rows, l // div, c


def unpool2_fwd(v, sel, bias=None, out=None):
    """-> out (rows, 2 Lo, C): out[2j + sel] = v[j] + bias (None: no bias), the partner exactly +0.0; every element written."""
    rows, lo, c = _unpool_v(v, 'unpool2_fwd', 'v')
    _sel(sel, rows, lo, c, 'unpool2_fwd')
    if bias is not None and tuple(_H._f32(bias, 'bias').shape) != (c,):
        raise ValueError('unpool2_fwd: bias must be (%d,)' % c)
    out = _H._out(out, (rows, 2 * lo, c), torch.float32, v.device, False, 'unpool2_fwd', strict=True)
    _H._chk(_H._lib.lib().da_unpool2_fwd(_H._p(v), _H._p(bias), _H._p(sel), _H._p(out), rows, lo, c, _H._stream()), 'da_unpool2_fwd')
    return out


def unpool2_bwd(dout, sel, out=None):
    """dout (rows, 2 Lo, C) -> dv (rows, Lo, C) = dout[2j + sel]."""
    rows, lo, c = _unpool_v(dout, 'unpool2_bwd', 'dout', div=2)
    _sel(sel, rows, lo, c, 'unpool2_bwd')
    dv = _H._out(out, (rows, lo, c), torch.float32, dout.device, False, 'unpool2_bwd', strict=True)
    _H._chk(_H._lib.lib().da_unpool2_bwd(_H._p(dout), _H._p(sel), _H._p(dv), rows, lo, c, _H._stream()), 'da_unpool2_bwd')
    return dv


# ---- the output stage ------------------------------------------------------------------------------------------------------------
def _out_operands(v, bias3, sel1, w4, who):
    _H._float_storage_only(who, 'the autoencoder stages run')
    rows, lo, c = _H._rlc(v, 'v').shape
    if c != OUT_C or rows < 1 or lo < 1 or rows * lo * c >= 1 << 31:
        raise ValueError('%s: v %s must be a (rows, L / 2, %d) map of fewer than 2^31 elements' % (who, tuple(v.shape), OUT_C))
    _sel(sel1, rows, lo, c, who, 'sel1')
    if tuple(_H._f32(bias3, 'bias3').shape) != (c,) or tuple(_H._f32(w4, 'w4').shape) != (c, 1, 3):
        raise ValueError('%s: bias3 must be (%d,) and w4 (%d, 1, 3)' % (who, c, c))
    return rows, 2 * lo


def ae_out_fwd(v, bias3, sel1, w4, bias4, x):
    """recon = ConvTranspose1d(64, 1, 3, padding=1)(unpool(v + bias3, sel1)) and the MSE against x (rows, L), without storing the
    unpooled map.  -> recon (rows, L), dr = d loss / d recon (rows, L), loss (1,)."""
    rows, l = _out_operands(v, bias3, sel1, w4, 'ae_out_fwd')
    if tuple(_H._f32(x, 'x').shape) != (rows, l) or tuple(_H._f32(bias4, 'bias4').shape) != (1,):
        raise ValueError('ae_out_fwd: x must be (rows, L) = (%d, %d) and bias4 (1,)' % (rows, l))
    L = _H._lib.lib()
    recon, dr = torch.empty_like(x), torch.empty_like(x)
    loss = torch.empty((1,), device=x.device, dtype=torch.float32)
    ws = torch.empty((max(L.da_ae_out_fwd_workspace(rows, l) // 4, 1),), device=x.device, dtype=torch.float32)
    _H._chk(L.da_ae_out_fwd(_H._p(v), _H._p(bias3), _H._p(sel1), _H._p(w4), _H._p(bias4), _H._p(x), _H._p(recon), _H._p(dr),
                            _H._p(ws), _H._p(loss), rows, l, _H._stream()), 'da_ae_out_fwd')
    return recon, dr, loss


def ae_out_bwd(dr, v, bias3, sel1, w4, dw4=None, db4=None, accumulate=False):
    """-> dv (rows, L / 2, 64) (the gradient at v + bias3: its column sum is bias3's), dw4 (64, 1, 3), db4 (1,); with
    destinations the two parameter gradients are written there, or -- accumulate -- added."""
    rows, l = _out_operands(v, bias3, sel1, w4, 'ae_out_bwd')
    if tuple(_H._f32(dr, 'dr').shape) != (rows, l):
        raise ValueError('ae_out_bwd: dr must be (rows, L) = (%d, %d)' % (rows, l))
    dw4 = _H._out(dw4, (OUT_C, 1, 3), torch.float32, v.device, accumulate, 'ae_out_bwd', strict=True)
    db4 = _H._out(db4, (1,), torch.float32, v.device, accumulate, 'ae_out_bwd', strict=True)
    L = _H._lib.lib()
    dv = torch.empty_like(v)
    ws = torch.empty((max(L.da_ae_out_bwd_workspace(rows, l) // 4, 1),), device=v.device, dtype=torch.float32)
    _H._chk(L.da_ae_out_bwd(_H._p(dr), _H._p(v), _H._p(bias3), _H._p(sel1), _H._p(w4), _H._p(dv), _H._p(dw4), _H._p(db4), _H._p(ws),
                            rows, l, 1 if accumulate else 0, _H._stream()), 'da_ae_out_bwd')
    return dv, dw4, db4
