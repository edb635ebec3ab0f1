"""The Squeeze-and-Excitation tail of an SE-ResNet BasicBlock (reference models/senet.py:15-34 SEModule, :52-68
SEBasicBlock.forward) as wrappers of the C ABI (``da_se_*``; kernels in csrc/se.hip), the same tail at a Bottleneck's width
(:71-95, :122-144; ``da_se_wide_*``, csrc/se_wide.hip) with the rule that picks between the two (``se_gate_family``), and the
length rule of the ceil-mode stem pool that SENet.layer0 uses (csrc/stem_pool.hip, pool_mode 2).  Reached as ``hip_ops.se_gate_fwd`` ...; same conventions
as the other wrappers: contiguous float32 CUDA operands, the current stream, no host synchronisation, shapes checked here so
that an unsupported one raises with the shape before anything is launched."""
import torch

from . import hip_ops as _H


def pool_out_len(lin, pool_mode):
    """Pooled length of a ``lin``-long row.  Modes 0 / 1 (F.POOL_MAX / POOL_AVG): pool(3, 2, 1).  Mode 2 (F.POOL_MAX_CEIL):
    MaxPool1d(3, 2, ceil_mode=True) without padding -- ATen's rule: ceil((lin - 3) / 2) + 1 windows, minus one if the last
    would start at or beyond ``lin`` (112 -> 56, the last window holding two elements; a one-element row has no window)."""
    if pool_mode not in (0, 1, 2):
        raise ValueError('pool_mode must be 0 (max), 1 (avg) or 2 (max, ceil mode)')
    if pool_mode != 2:
        return (lin - 1) // 2 + 1
    lout = -((3 - lin) // 2) + 1                        # ceil((lin - 3) / 2) + 1
    return lout - 1 if (lout - 1) * 2 >= lin else lout


# ------------------------------------------------------------------------------------------------
# Squeeze-and-Excitation tail of an SE-ResNet BasicBlock (se.hip; reference models/senet.py:15-34, :52-68)
#     out = relu(z * s + res),  z = bn2(y2) (never stored),  s = sigmoid(fc2(relu(fc1(mean_L z))))
# ------------------------------------------------------------------------------------------------
def _se_y(y2, R, who):
    _H._float_storage_only(who, 'the SE tail runs')
    _H._rlc(y2, 'y2')
    return _H._bn_win(y2, R)


def _se_stats(mean, invstd, w, c, who):
    for t in (mean, invstd):
        if tuple(_H._f32(t, 'statistics').shape) != (w, c):
            raise ValueError('%s: mean / invstd must be (W, C) = (%d, %d)' % (who, w, c))


def _se_rc(t, rows, c, name):
    if tuple(_H._f32(t, name).shape) != (rows, c):
        raise ValueError('%s must be (%d, %d), got %s' % (name, rows, c, tuple(t.shape)))
    return t


def _se_fc(w1, b1, w2, b2, c, who):
    """fc1 / fc2 of an SEModule (Conv1d k1 weights (Cr, C, 1) / (C, Cr, 1), or their 2-D views) -> Cr."""
    cr = w1.shape[0]
    for t, shape, name in ((w1, (cr, c), 'fc1.weight'), (b1, (cr,), 'fc1.bias'), (w2, (c, cr), 'fc2.weight'), (b2, (c,), 'fc2.bias')):
        if t is None:
            continue
        _H._f32(t, name)
        if tuple(t.shape) != shape and (len(shape) == 1 or tuple(t.shape) != shape + (1,)):
            raise ValueError('%s: %s must be %s, got %s' % (who, name, shape, tuple(t.shape)))
    return cr


def se_stats(y2, R, eps=1e-5):
    """Per-window statistics of y2 in front of the gate: one launch where the shape has the single-pass geometry
    (bn_stats_fused), else partial + merge.  -> mean, invstd (W, C)."""
    rows, l, c, w, wn = _se_y(y2, R, 'se_stats')
    if w and _H.bn_single_pass(w, wn, c):
        mean, invstd = _H._bn_stats_pair(w, c, y2.device)
        _H.bn_stats_fused(y2, R, mean, invstd, eps)
        return mean, invstd
    return _H.bn_stats(y2, R, eps)


def _ptrs(*ts):
    return tuple(_H._p(t) for t in ts)


def se_gate_fwd(y2, R, mean, invstd, gamma, beta, w1, b1, w2, b2):
    """-> pool (rows, C) = bn2's affine of mean_L(y2), hid (rows, Cr) = relu(fc1(pool)), s (rows, C) = sigmoid(fc2(hid)):
    one launch, a tile of rows per workgroup."""
    rows, l, c, w, wn = _se_y(y2, R, 'se_gate_fwd')
    _se_stats(mean, invstd, w, c, 'se_gate_fwd')
    cr = _se_fc(w1, b1, w2, b2, c, 'se_gate_fwd')
    pool = torch.empty((rows, c), device=y2.device, dtype=torch.float32)
    hid = torch.empty((rows, cr), device=y2.device, dtype=torch.float32)
    s = torch.empty((rows, c), device=y2.device, dtype=torch.float32)
    _H._chk(_H._lib.lib().da_se_gate_fwd(_H._p(y2), rows, R, l, c, cr,
                                         *_ptrs(mean, invstd, _H._f32(gamma), _H._f32(beta), w1, b1, w2, b2, pool, hid, s),
                                         _H._stream()), 'da_se_gate_fwd')
    return pool, hid, s


def se_scale_fwd(y2, R, mean, invstd, gamma, beta, s, res, out=None):
    """-> out = max(fmaf(z, s, res), 0), mask (int64 words, one bit per element in memory order: bit (i % 8) of byte i / 8
    says out[i] > 0)."""
    rows, l, c, w, wn = _se_y(y2, R, 'se_scale_fwd')
    _se_stats(mean, invstd, w, c, 'se_scale_fwd')
    _se_rc(s, rows, c, 's')
    _H._bn_same(_H._rlc(res, 'res'), y2.shape)
    out = _H._out(out, y2.shape, torch.float32, y2.device, False, 'se_scale_fwd', strict=True)
    mask = torch.empty((rows * l * c // 64,), device=y2.device, dtype=torch.int64)          # (C % 64 == 0)
    _H._chk(_H._lib.lib().da_se_scale_fwd(*_ptrs(y2, res, out, mask), rows, R, l, c,
                                          *_ptrs(mean, invstd, _H._f32(gamma), _H._f32(beta), s), _H._stream()), 'da_se_scale_fwd')
    return out, mask


def se_bwd_reduce(dout, mask, y2, R, mean, invstd, gamma, beta):
    """-> g = dout . mask (rows, L, C), dsum (rows, C) = sum_l g z."""
    rows, l, c, w, wn = _se_y(y2, R, 'se_bwd_reduce')
    _se_stats(mean, invstd, w, c, 'se_bwd_reduce')
    _H._bn_same(_H._rlc(dout, 'dout'), y2.shape, 'dout')
    if not (mask.is_cuda and mask.dtype == torch.int64 and mask.is_contiguous() and mask.numel() == y2.numel() // 64):
        raise ValueError('mask must be the bit mask of se_scale_fwd (%d int64 words)' % (y2.numel() // 64))
    g = torch.empty_like(y2)
    dsum = torch.empty((rows, c), device=y2.device, dtype=torch.float32)
    _H._chk(_H._lib.lib().da_se_bwd_reduce(*_ptrs(dout, mask, y2, g, dsum), rows, R, l, c,
                                           *_ptrs(mean, invstd, _H._f32(gamma), _H._f32(beta)), _H._stream()), 'da_se_bwd_reduce')
    return g, dsum


def se_gate_bwd(dsum, s, hid, pool, w1, w2, grads=None, accumulate=False):
    """Backward of the gate: -> dpool (rows, C), (dw1, db1, dw2, db2).  grads: the four destinations (shaped like the
    parameters; a trainer's bucket views), written or -- accumulate -- added to; None: new tensors.  Fixed summation order."""
    rows, c = _H._f32(dsum, 'dsum').shape
    cr = _se_fc(w1, None, w2, None, c, 'se_gate_bwd')
    _se_rc(s, rows, c, 's')
    _se_rc(pool, rows, c, 'pool')
    _se_rc(hid, rows, cr, 'hid')
    shapes = (tuple(w1.shape), (cr,), tuple(w2.shape), (c,))
    if grads is None:
        if accumulate:
            raise ValueError('se_gate_bwd: accumulate needs grads')
        grads = tuple(torch.empty(sh, device=dsum.device, dtype=torch.float32) for sh in shapes)
    for t, sh in zip(grads, shapes):
        if tuple(_H._f32(t, 'gradient destination').shape) != sh:
            raise ValueError('se_gate_bwd: bad gradient destination %s, expected %s' % (tuple(t.shape), sh))
    dpool = torch.empty((rows, c), device=dsum.device, dtype=torch.float32)
    L = _H._lib.lib()
    ws = torch.empty((max(L.da_se_gate_bwd_workspace(rows, c, cr) // 4, 1),), device=dsum.device, dtype=torch.float32)
    _H._chk(L.da_se_gate_bwd(*_ptrs(dsum, s, hid, pool, w1, w2, dpool, *grads), 1 if accumulate else 0, _H._p(ws), rows, c, cr,
                             _H._stream()), 'da_se_gate_bwd')
    return dpool, tuple(grads)


def se_bwd_scale(g, s, dpool, out=None):
    """-> dz = fmaf(g, s, dpool / L): the gradient of z, which bn_bwd(mask_mode=0) of bn2 takes."""
    _H._float_storage_only('se_bwd_scale', 'the SE tail runs')
    rows, l, c = _H._rlc(g, 'g').shape
    _se_rc(s, rows, c, 's')
    _se_rc(dpool, rows, c, 'dpool')
    dz = _H._out(out, g.shape, torch.float32, g.device, False, 'se_bwd_scale', strict=True)
    _H._chk(_H._lib.lib().da_se_bwd_scale(*_ptrs(g, s, dpool, dz), rows, l, c, _H._stream()), 'da_se_bwd_scale')
    return dz


# ------------------------------------------------------------------------------------------------
# The same tail at an SE-ResNet Bottleneck's width (se_wide.hip; reference models/senet.py:71-95, :122-144): the gate acts on
# 4 planes channels with reduction 16, (C, Cr) = (256, 16) ... (2048, 128)
# ------------------------------------------------------------------------------------------------
NARROW, WIDE = 'narrow', 'wide'
# The shapes BOTH families take at which the wide one runs: decided by timing both (scripts/bench_se_bottleneck.py; figures
# in DESIGN_APPENDIX.md, "se_resnet50").  Every other shared shape -- se_resnet18's (reduction 4) among them -- stays narrow.
WIDE_SHARED = frozenset({(512, 32)})


def se_narrow_ok(c, cr):
    """se.hip's shapes (se_shape_ok): C = 64 ... 512 whose quads divide a block, Cr a multiple of 16 that divides 256."""
    return c in (64, 128, 256, 512) and cr >= 16 and cr % 16 == 0 and cr <= 256 and 256 % cr == 0 and (c // 4) % (256 // cr) == 0


def se_wide_ok(c, cr):
    """se_wide.hip's shapes (sew_shape_ok)."""
    return 64 <= c <= 2048 and c % 64 == 0 and 16 <= cr <= 128 and cr % 16 == 0


def se_gate_family(c, cr):
    """Which kernel family the SE tail of C channels with a hidden width of Cr runs on: a pure function of the shape.
    Above 512 channels only the wide family exists; a shape both take runs narrow unless it is listed in WIDE_SHARED."""
    narrow, wide = se_narrow_ok(c, cr), se_wide_ok(c, cr)
    if not (narrow or wide):
        raise NotImplementedError('no SE gate kernels for (C, Cr) = (%d, %d): C %% 64 == 0 up to 2048 with Cr %% 16 == 0 up to 128, '
                                  'or 64 / 128 / 256 / 512 channels with a Cr that divides 256' % (c, cr))
    if narrow and wide:
        return WIDE if (c, cr) in WIDE_SHARED else NARROW
    return WIDE if wide else NARROW


def se_wide_stats(y3, R, eps=1e-5):
    """One pass over y3 (rows, L, C) from memory (each block reads its row slice twice, the second time from the cache) -> mean, invstd (W, C) of its windows of R rows and rowsum (rows, C) = sum_l y3: the
    gate (se_wide_gate_fwd) takes the row sums and never reads the map."""
    rows, l, c, w, wn = _se_y(y3, R, 'se_wide_stats')
    mean, invstd = _H._bn_stats_pair(w, c, y3.device)
    rowsum = torch.empty((rows, c), device=y3.device, dtype=torch.float32)
    ws = torch.empty((max(rows * c, 1),), device=y3.device, dtype=torch.float32)
    _H._chk(_H._lib.lib().da_se_wide_stats(_H._p(y3), rows, R, l, c, eps, *_ptrs(mean, invstd, rowsum, ws), _H._stream()),
            'da_se_wide_stats')
    return mean, invstd, rowsum


def se_wide_gate_fwd(rowsum, R, L, mean, invstd, gamma, beta, w1, b1, w2, b2):
    """rowsum (rows, C) of a (rows, L, C) map -> pool = fmaf(rowsum / L, sc, sh), hid = relu(fc1(pool)), s = sigmoid(fc2(hid)):
    three launches (the elementwise pool, then hid and s as GEMMs on the fp32 matrix cores over tiles of 32 rows)."""
    _H._float_storage_only('se_wide_gate_fwd', 'the SE tail runs')
    rows, c = _H._f32(rowsum, 'rowsum').shape
    if R < 1 or rows % R or L < 1:
        raise ValueError('se_wide_gate_fwd: rows must be a multiple of R, L >= 1')
    _se_stats(mean, invstd, rows // R, c, 'se_wide_gate_fwd')
    cr = _se_fc(w1, b1, w2, b2, c, 'se_wide_gate_fwd')
    pool = torch.empty((rows, c), device=rowsum.device, dtype=torch.float32)
    hid = torch.empty((rows, cr), device=rowsum.device, dtype=torch.float32)
    s = torch.empty((rows, c), device=rowsum.device, dtype=torch.float32)
    _H._chk(_H._lib.lib().da_se_wide_gate_fwd(_H._p(rowsum), rows, R, L, c, cr,
                                              *_ptrs(mean, invstd, _H._f32(gamma), _H._f32(beta), w1, b1, w2, b2, pool, hid, s),
                                              _H._stream()), 'da_se_wide_gate_fwd')
    return pool, hid, s


def se_wide_scale_fwd(y3, R, mean, invstd, gamma, beta, s, res, out=None):
    """se_scale_fwd at the wide family's widths: -> out = max(fmaf(z, s, res), 0), mask (int64 words, one bit per element)."""
    rows, l, c, w, wn = _se_y(y3, R, 'se_wide_scale_fwd')
    _se_stats(mean, invstd, w, c, 'se_wide_scale_fwd')
    _se_rc(s, rows, c, 's')
    _H._bn_same(_H._rlc(res, 'res'), y3.shape)
    if c % 64:
        raise _H.HipError('se_wide_scale_fwd: C = %d is not a multiple of 64' % c)
    out = _H._out(out, y3.shape, torch.float32, y3.device, False, 'se_wide_scale_fwd', strict=True)
    mask = torch.empty((rows * l * c // 64,), device=y3.device, dtype=torch.int64)
    _H._chk(_H._lib.lib().da_se_wide_scale_fwd(*_ptrs(y3, res, out, mask), rows, R, l, c,
                                               *_ptrs(mean, invstd, _H._f32(gamma), _H._f32(beta), s), _H._stream()),
            'da_se_wide_scale_fwd')
    return out, mask


def se_wide_bwd_reduce(dout, mask, y3, R, mean, invstd, gamma, beta):
    """-> g = dout . mask (rows, L, C), dsum (rows, C) = sum_l g z, a block per (row, 64 channels)."""
    rows, l, c, w, wn = _se_y(y3, R, 'se_wide_bwd_reduce')
    _se_stats(mean, invstd, w, c, 'se_wide_bwd_reduce')
    _H._bn_same(_H._rlc(dout, 'dout'), y3.shape, 'dout')
    if not (mask.is_cuda and mask.dtype == torch.int64 and mask.is_contiguous() and mask.numel() * 64 == y3.numel()):
        raise ValueError('mask must be the bit mask of se_wide_scale_fwd (%d int64 words)' % (y3.numel() // 64))
    g = torch.empty_like(y3)
    dsum = torch.empty((rows, c), device=y3.device, dtype=torch.float32)
    _H._chk(_H._lib.lib().da_se_wide_bwd_reduce(*_ptrs(dout, mask, y3, g, dsum), rows, R, l, c,
                                                *_ptrs(mean, invstd, _H._f32(gamma), _H._f32(beta)), _H._stream()),
            'da_se_wide_bwd_reduce')
    return g, dsum


def se_wide_chunk_rows():
    """Rows per chunk of se_wide_gate_bwd's parameter-gradient partials."""
    return int(_H._lib.lib().da_se_wide_chunk_rows())


def se_wide_gate_bwd(dsum, s, hid, pool, w1, w2, grads=None, accumulate=False):
    """se_gate_bwd on the wide family: -> dpool (rows, C), (dw1, db1, dw2, db2); the parameter gradients are GEMMs with K =
    rows, split over chunks of rows and folded in chunk order into ``grads`` (written, or -- accumulate -- added to)."""
    rows, c = _H._f32(dsum, 'dsum').shape
    cr = _se_fc(w1, None, w2, None, c, 'se_wide_gate_bwd')
    _se_rc(s, rows, c, 's')
    _se_rc(pool, rows, c, 'pool')
    _se_rc(hid, rows, cr, 'hid')
    shapes = (tuple(w1.shape), (cr,), tuple(w2.shape), (c,))
    if grads is None:
        if accumulate:
            raise ValueError('se_wide_gate_bwd: accumulate needs grads')
        grads = tuple(torch.empty(sh, device=dsum.device, dtype=torch.float32) for sh in shapes)
    for t, sh in zip(grads, shapes):
        if tuple(_H._f32(t, 'gradient destination').shape) != sh:
            raise ValueError('se_wide_gate_bwd: bad gradient destination %s, expected %s' % (tuple(t.shape), sh))
    L = _H._lib.lib()
    if not L.da_se_wide_shape_ok(c, cr):
        raise _H.HipError('se_wide_gate_bwd: unsupported (C, Cr) = (%d, %d)' % (c, cr))
    dpool = torch.empty((rows, c), device=dsum.device, dtype=torch.float32)
    ws = torch.empty((max(L.da_se_wide_gate_bwd_workspace(rows, c, cr) // 4, 1),), device=dsum.device, dtype=torch.float32)
    _H._chk(L.da_se_wide_gate_bwd(*_ptrs(dsum, s, hid, pool, w1, w2, dpool, *grads), 1 if accumulate else 0, _H._p(ws), rows, c, cr,
                                  _H._stream()), 'da_se_wide_gate_bwd')
    return dpool, tuple(grads)


def se_wide_bwd_scale(g, s, dpool, out=None):
    """se_bwd_scale at the wide family's widths: -> dz = fmaf(g, s, dpool / L)."""
    _H._float_storage_only('se_wide_bwd_scale', 'the SE tail runs')
    rows, l, c = _H._rlc(g, 'g').shape
    _se_rc(s, rows, c, 's')
    _se_rc(dpool, rows, c, 'dpool')
    dz = _H._out(out, g.shape, torch.float32, g.device, False, 'se_wide_bwd_scale', strict=True)
    _H._chk(_H._lib.lib().da_se_wide_bwd_scale(*_ptrs(g, s, dpool, dz), rows, l, c, _H._stream()), 'da_se_wide_bwd_scale')
    return dz
