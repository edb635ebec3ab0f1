"""Host side of csrc/dtw.hip: checked wrappers around ``da_dtw_pairs`` / ``da_dtw_segment_mean`` and the Python twins of
``da_dtw_shape_ok`` / ``da_dtw_plan`` (no library needed).  PyTorch allocates and orders streams; all arithmetic is in the
kernels.  The definition of the distance is in include/deepards_hip.h; ``deepards_amd.dtw`` is the surface built on this."""
import ctypes

import numpy as np
import torch

from . import _lib
from . import hip_ops as H

MAX_LEN = 4608                                  # csrc/dtw.hip DTW_MAXLEN: 64 lanes x the widest strip
CLASSES = (1, 2, 4, 8, 16, 32, 48, 72)          # DTW_CLASSES: columns per lane
WAVES_PER_BLOCK = 4                             # DTW_WAVES: pairs of one block
ACC = {'f32': 0, 'f64': 1}
METRICS = {'euclidean': 0, 'sqeuclidean': 1}
_ACC_DTYPE = {'f32': torch.float32, 'f64': torch.float64}
PLAN_FIELDS = ('lanes', 'cols_per_lane', 'steps', 'waves_per_block', 'grid', 'block', 'lds')


def _acc(acc):
    if acc not in ACC:
        raise ValueError("dtw: acc must be 'f32' or 'f64', got %r" % (acc,))
    return ACC[acc]


def dtw_refusal(n, m, acc='f64', a64=False, b64=False):
    """Why the kernels do not take this shape, or None."""
    if acc not in ACC:
        return "acc must be 'f32' or 'f64', got %r" % (acc,)
    if n < 1 or m < 1:
        return 'sequences must hold at least one sample, got lengths %d and %d' % (n, m)
    if n > MAX_LEN or m > MAX_LEN:
        return 'sequences of up to %d samples are supported (64 lanes x %d columns), got lengths %d and %d; nothing is ' \
               'truncated' % (MAX_LEN, CLASSES[-1], n, m)
    if acc == 'f32' and (a64 or b64):
        return "acc='f32' takes float32 tables only: a float64 table would be rounded on the way in; use acc='f64'"
    return None


def dtw_shape_ok(n, m, acc='f64', a64=False, b64=False):
    """Python twin of ``da_dtw_shape_ok``."""
    return dtw_refusal(n, m, acc, a64, b64) is None


def dtw_class(m):
    """Columns per lane for rows of m samples: the smallest class that covers ceil(m / 64)."""
    need = (m + 63) // 64
    for w in CLASSES:
        if w >= need:
            return w
    raise ValueError(dtw_refusal(1, m))


def dtw_plan(n, m, p, acc='f64'):
    """Python twin of ``da_dtw_plan``: lanes that hold columns, columns per lane, steps, pairs per block, grid, threads per
    block and LDS bytes of the launch for P pairs of an (n, m) problem.  A refused shape (or P < 1) raises ValueError."""
    why = dtw_refusal(n, m, acc) or (None if p >= 1 else 'P must be at least 1, got %d' % p)
    if why:
        raise ValueError('dtw: ' + why)
    w = dtw_class(m)
    lanes = -(-m // w)
    return dict(lanes=lanes, cols_per_lane=w, steps=n + lanes - 1, waves_per_block=WAVES_PER_BLOCK,
                grid=-(-p // WAVES_PER_BLOCK), block=64 * WAVES_PER_BLOCK, lds=0)


def dtw_plan_lib(n, m, p, acc='f64'):
    """``da_dtw_plan`` itself -> the same dict, or None where the library refuses."""
    out = (ctypes.c_int * len(PLAN_FIELDS))()
    if _lib.lib().da_dtw_plan(n, m, p, ACC.get(acc, -1), out) != 0:
        return None
    return dict(zip(PLAN_FIELDS, [int(v) for v in out]))


def class_edges():
    """The lengths m at which the columns per lane change: (last m of a class, first m of the next), up to MAX_LEN."""
    return [(64 * w, 64 * w + 1) for w in CLASSES[:-1]] + [(MAX_LEN, MAX_LEN + 1)]


def _table(t, name):
    """t: (S, L) float32 / float64 CUDA with unit column stride and a row pitch >= L (a column slice of a wider buffer is fine)
    -> (S, L, pitch, is64)."""
    if not isinstance(t, torch.Tensor):
        raise ValueError('dtw: %s must be a torch tensor on the device, got %s' % (name, type(t).__name__))
    if not t.is_cuda:
        raise ValueError('dtw: %s is a CPU tensor; the kernels read device memory only (move it with .cuda())' % name)
    if t.dtype not in (torch.float32, torch.float64):
        raise ValueError('dtw: %s must be float32 or float64, got %s' % (name, t.dtype))
    if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError('dtw: %s must be a table (S, L) of S >= 1 rows of L >= 1 samples, got %s' % (name, tuple(t.shape)))
    s, l = t.shape
    if t.stride(1) != 1 or (s > 1 and t.stride(0) < l):
        raise ValueError('dtw: %s must have contiguous samples and a row pitch >= %d, got strides %s' % (name, l, t.stride()))
    if s > 0x7fffffff or (s > 1 and t.stride(0) > 0x7fffffff):
        raise ValueError('dtw: %s is too large for int32 row indices' % name)
    return s, l, (t.stride(0) if s > 1 else max(l, t.stride(0))), t.dtype == torch.float64


def _indices(v, rows, name, device):
    """Pair indices -> contiguous int32 device tensor.  A host list / array is range-checked here; a device tensor is not read
    back (no synchronisation): the kernel answers NaN for an index outside its table and reads nothing."""
    if isinstance(v, torch.Tensor) and v.is_cuda:
        if v.dtype not in (torch.int32, torch.int64) or v.dim() != 1:
            raise ValueError('dtw: %s must be a 1-D int32 / int64 tensor, got %s %s' % (name, v.dtype, tuple(v.shape)))
        return v.to(torch.int32).contiguous()
    a = np.asarray(v.numpy() if isinstance(v, torch.Tensor) else v)
    if a.ndim != 1 or a.dtype.kind not in 'iu':
        raise ValueError('dtw: %s must be a 1-D list of integers' % name)
    if a.size and (int(a.min()) < 0 or int(a.max()) >= rows):
        raise IndexError('dtw: %s holds a row outside [0, %d)' % (name, rows))
    return torch.as_tensor(a.astype(np.int32)).to(device)


def dtw_pairs(table_a, ia, ib, table_b=None, metric='euclidean', band=None, acc='f64', out=None):
    """P distances in one launch: out[p] = dtw(table_a[ia[p]], table_b[ib[p]]) (table_b None: table_a).  Tables (S, L)
    float32 / float64 on the device; ia, ib host lists (range-checked) or device tensors; band None or a Sakoe-Chiba radius
    >= 0; acc the accumulation type, which is the type of the result.  ``out``: a (P,) device destination of that type with
    unit stride."""
    if metric not in METRICS:
        raise ValueError("dtw: metric must be 'euclidean' or 'sqeuclidean', got %r" % (metric,))
    code = _acc(acc)
    table_b = table_a if table_b is None else table_b
    sa, n, lda, a64 = _table(table_a, 'table_a')
    sb, m, ldb, b64 = _table(table_b, 'table_b')
    if table_b.device != table_a.device:
        raise ValueError('dtw: the two tables are on different devices')
    why = dtw_refusal(n, m, acc, a64, b64)
    if why:
        raise ValueError('dtw: ' + why)
    if band is None:
        k = -1
    else:
        k = int(band)
        if k < 0 or k != band:
            raise ValueError('dtw: band must be None or an integer >= 0, got %r' % (band,))
        k = min(k, MAX_LEN)
    dev = table_a.device
    ia, ib = _indices(ia, sa, 'ia', dev), _indices(ib, sb, 'ib', dev)
    p = ia.numel()
    if p < 1 or ib.numel() != p:
        raise ValueError('dtw: ia and ib must hold the same number of pairs, at least one; got %d and %d' % (p, ib.numel()))
    dtype = _ACC_DTYPE[acc]
    if out is None:
        out = torch.empty((p,), device=dev, dtype=dtype)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.device == dev and out.dtype == dtype and
              tuple(out.shape) == (p,) and (p == 1 or out.stride(0) == 1)):
        raise ValueError('dtw: out must be a (%d,) %s device tensor with unit stride' % (p, dtype))
    with torch.cuda.device(dev):
        H._chk(_lib.lib().da_dtw_pairs(H._p(table_a), int(a64), lda, sa, n, H._p(table_b), int(b64), ldb, sb, m, H._p(ia), H._p(ib),
                                       p, code, METRICS[metric], k, H._p(out), H._stream()), 'da_dtw_pairs')
    return out


def segment_mean(dist, offsets, out=None):
    """out[g] = the float64 sum of dist[offsets[g]:offsets[g + 1]] in index order, divided by the segment's length; NaN for an
    empty segment.  dist (P,) float32 / float64, offsets (G + 1,) int32 (a host list is checked and uploaded), both on the
    device.  ``out``: a (G,) float64 device destination with unit stride."""
    if not (isinstance(dist, torch.Tensor) and dist.is_cuda and dist.dtype in (torch.float32, torch.float64) and dist.dim() == 1
            and (dist.numel() <= 1 or dist.stride(0) == 1)):
        raise ValueError('segment_mean: dist must be a 1-D float32 / float64 device tensor with unit stride')
    p = dist.numel()
    if isinstance(offsets, torch.Tensor) and offsets.is_cuda:
        if offsets.dtype != torch.int32 or offsets.dim() != 1 or not offsets.is_contiguous():
            raise ValueError('segment_mean: device offsets must be a contiguous 1-D int32 tensor')
    else:
        a = np.asarray(offsets.numpy() if isinstance(offsets, torch.Tensor) else offsets)
        if a.ndim != 1 or a.dtype.kind not in 'iu' or a.size < 2:
            raise ValueError('segment_mean: offsets must be a 1-D list of G + 1 >= 2 integers')
        if int(a[0]) < 0 or int(a[-1]) > p or (np.diff(a) < 0).any():
            raise IndexError('segment_mean: offsets must rise from >= 0 to <= %d' % p)
        offsets = torch.as_tensor(a.astype(np.int32)).to(dist.device)
    g = offsets.numel() - 1
    if g < 1:
        raise ValueError('segment_mean: offsets must hold G + 1 >= 2 entries')
    if out is None:
        out = torch.empty((g,), device=dist.device, dtype=torch.float64)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.device == dist.device and out.dtype == torch.float64 and
              tuple(out.shape) == (g,) and (g == 1 or out.stride(0) == 1)):
        raise ValueError('segment_mean: out must be a (%d,) float64 device tensor with unit stride' % g)
    with torch.cuda.device(dist.device):
        H._chk(_lib.lib().da_dtw_segment_mean(H._p(dist) if p else None, int(dist.dtype == torch.float64), p, H._p(offsets), g,
                                              H._p(out), H._stream()), 'da_dtw_segment_mean')
    return out
