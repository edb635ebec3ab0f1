"""The grouped k3 convolution of the SE-ResNeXt 32x4d bottleneck (reference models/senet.py:147-168: conv2, Conv1d(width,
width, 3, stride, padding=1, groups=32)) as wrappers of the C ABI (``da_gconv3_*``; kernels in csrc/conv_grouped.hip).  Reached
as ``hip_ops.gconv3_fwd`` ...; same conventions as the other wrappers: contiguous float32 CUDA operands, the current stream,
no host synchronisation, shapes checked here so that an unsupported one raises with the shape before anything is launched.
The weight is torch's own (C, C / 32, 3): there is no packed form."""
import collections
import ctypes

import torch

from . import hip_ops as _H

GROUPS = 32
FWD, DGRAD, WGRAD = 0, 1, 2

GConvPlan = collections.namedtuple('GConvPlan', 'grid block lds workspace tile_positions tiles_per_block tiles')


def gconv3_ok(c, groups, stride):
    """The shapes csrc/conv_grouped.hip takes: groups == 32, C in {128, 256, 512, 1024}, stride 1 / 2.  A pure function of
    the shape (the library's da_gconv3_shape_ok answers the same; tests compare the two)."""
    return groups == GROUPS and c in (128, 256, 512, 1024) and stride in (1, 2)


def gconv3_out_len(l, stride):
    return (l - 1) // stride + 1


def gconv3_plan(which, rows, l, c, stride):
    """Launch geometry of kernel ``which`` (FWD / DGRAD / WGRAD) on a (rows, l, c) input map, from the expressions the launch
    itself uses; launches nothing.  -> GConvPlan, or raises HipError for a shape without a legal launch."""
    L = _H._lib.lib()
    grid, block = (ctypes.c_int * 3)(), (ctypes.c_int * 3)()
    lds, ws = ctypes.c_size_t(), ctypes.c_size_t()
    tp, tb, tiles = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    args = (int(which), int(rows), int(l), int(c), int(stride))
    if any(not -2 ** 31 <= a < 2 ** 31 for a in args) or \
            L.da_gconv3_plan(*args, grid, block, ctypes.byref(lds), ctypes.byref(ws)) != 0 or \
            L.da_gconv3_tiling(*args, ctypes.byref(tp), ctypes.byref(tb), ctypes.byref(tiles)) != 0:
        raise _H.HipError('gconv3_plan: no launch for which = %d, (rows, L, C) = (%d, %d, %d), stride %d' % args)
    return GConvPlan(tuple(grid), tuple(block), lds.value, ws.value, tp.value, tb.value, tiles.value)


def _check(who, t, w, stride, name):
    """-> rows, l, c of the map ``t`` beside the grouped weight ``w`` (C, C / 32, 3)."""
    _H._float_storage_only(who, 'the grouped convolution runs')
    rows, l, c = _H._rlc(t, name).shape
    if not gconv3_ok(c, GROUPS, stride):
        raise NotImplementedError('%s: no grouped k3 kernel for C = %d, stride %s (32 groups on 128 / 256 / 512 / 1024 '
                                  'channels, stride 1 / 2)' % (who, c, stride))
    if w is not None and tuple(_H._f32(w, 'weight').shape) != (c, c // GROUPS, 3):
        raise ValueError('%s: weight must be (C, C / 32, 3) = (%d, %d, 3), got %s' % (who, c, c // GROUPS, tuple(w.shape)))
    if rows < 1 or l < 1:
        raise ValueError('%s: empty map %s' % (who, tuple(t.shape)))
    return rows, l, c


def _same_device(who, *ts):
    if len({t.device for t in ts}) != 1:
        raise ValueError('%s: operands on different devices' % who)


def gconv3_fwd(x, w, stride, out=None):
    """y (rows, Lo, C) = grouped conv k3 p1 of x (rows, L, C) with w (C, C / 32, 3): one launch."""
    rows, l, c = _check('gconv3_fwd', x, w, stride, 'x')
    _same_device('gconv3_fwd', x, w)
    gconv3_plan(FWD, rows, l, c, stride)
    y = _H._out(out, (rows, gconv3_out_len(l, stride), c), torch.float32, x.device, False, 'gconv3_fwd', strict=True)
    _H._chk(_H._lib.lib().da_gconv3_fwd(_H._p(x), _H._p(w), _H._p(y), rows, l, c, stride, _H._stream()), 'da_gconv3_fwd')
    return y


def gconv3_dgrad(dy, w, stride, l_in, out=None, accumulate=False):
    """dx (rows, l_in, C) from dy (rows, Lo, C): every element written, or -- accumulate -- added to ``out``.  One launch."""
    rows, lo, c = _check('gconv3_dgrad', dy, w, stride, 'dy')
    _same_device('gconv3_dgrad', dy, w)
    if l_in < 1 or gconv3_out_len(l_in, stride) != lo:
        raise ValueError('gconv3_dgrad: dy has %d positions, an input of %d under stride %d gives %d' %
                         (lo, l_in, stride, gconv3_out_len(max(l_in, 1), stride)))
    gconv3_plan(DGRAD, rows, l_in, c, stride)
    dx = _H._out(out, (rows, l_in, c), torch.float32, dy.device, accumulate, 'gconv3_dgrad', strict=True)
    if not dx.is_cuda or dx.device != dy.device:
        raise ValueError('gconv3_dgrad: out must be on %s' % dy.device)
    _H._chk(_H._lib.lib().da_gconv3_dgrad(_H._p(dy), _H._p(w), _H._p(dx), rows, l_in, c, stride, 1 if accumulate else 0,
                                          _H._stream()), 'da_gconv3_dgrad')
    return dx


def gconv3_wgrad(dy, x, stride, out=None, accumulate=False):
    """dw (C, C / 32, 3) = sum over rows and positions of dy x: partials per chunk of tiles into a workspace, folded in chunk
    order (two launches, no atomics); written, or -- accumulate -- added to ``out``."""
    rows, l, c = _check('gconv3_wgrad', x, None, stride, 'x')
    _H._rlc(dy, 'dy')
    _same_device('gconv3_wgrad', dy, x)
    if tuple(dy.shape) != (rows, gconv3_out_len(l, stride), c):
        raise ValueError('gconv3_wgrad: dy must be %s, got %s' % ((rows, gconv3_out_len(l, stride), c), tuple(dy.shape)))
    plan = gconv3_plan(WGRAD, rows, l, c, stride)
    dw = _H._out(out, (c, c // GROUPS, 3), torch.float32, x.device, accumulate, 'gconv3_wgrad', strict=True)
    if not dw.is_cuda or dw.device != x.device:
        raise ValueError('gconv3_wgrad: out must be on %s' % x.device)
    ws = torch.empty((gconv3_workspace_floats(plan),), device=x.device, dtype=torch.float32)
    _H._chk(_H._lib.lib().da_gconv3_wgrad(_H._p(dy), _H._p(x), _H._p(dw), _H._p(ws), rows, l, c, stride, 1 if accumulate else 0,
                                          _H._stream()), 'da_gconv3_wgrad')
    return dw


def gconv3_workspace_floats(plan):
    """Floats gconv3_wgrad allocates for a WGRAD plan."""
    return plan.workspace // 4
