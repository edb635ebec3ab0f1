"""The batch gather with the reference's frequency filters behind the normalisation, as wrappers of the C ABI
(``da_gather_normalize_filter`` and, for padded datasets and post-hoc downsampling, ``da_gather_normalize_chain``; kernels in
csrc/filters.hip).  Reached as ``hip_ops.gather_normalize_filter`` / ``hip_ops.gather_normalize_chain``; same conventions as
``hip_ops.gather_normalize``: contiguous CUDA operands, the current stream, no host synchronisation."""
import ctypes

import torch

from . import hip_ops as _H
from .filters import FFT_FILTER_LEN, MAX_BUTTER_LEN


def _kernel(t, name, l, like, caller='gather_normalize_filter'):
    if t is None:
        return
    if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and tuple(t.shape) == (l,) and t.device == like.device):
        raise ValueError('%s: %s must be a contiguous float64 CUDA tensor of %d samples' % (caller, name, l))


def gather_normalize_filter(tiles, idx, mu, std, h=None, g=None, out=None):
    """tiles (N, NB, C <= 4, L) float64 CUDA raw windows, idx (B,) int64 CUDA -> (B, NB, C, L) float32: every row
    normalised ((x - mu) / std, scalars for C = 1 or one per channel), convolved causally with h (L <= 512 float64 CUDA
    samples: a Butterworth cascade's impulse response, dataset.py:546-557,1381-1382), then circularly with g (L == 224:
    real(ifft(band mask)), dataset.py:1393-1400), in float64, then cast.  h or g may be None, not both.  Like
    ``gather_normalize`` the kernel reads tiles[idx[b]] unchecked: idx must already be known to lie in [0, N)."""
    if not (tiles.is_cuda and tiles.dtype == torch.float64 and tiles.is_contiguous() and tiles.dim() == 4):
        raise ValueError('gather_normalize_filter: tiles must be a contiguous float64 CUDA tensor (N, NB, C, L)')
    if not (idx.is_cuda and idx.dtype == torch.int64 and idx.is_contiguous() and idx.dim() == 1):
        raise ValueError('gather_normalize_filter: idx must be a contiguous 1-D int64 CUDA tensor')
    _, nb, c, l = tiles.shape
    if h is None and g is None:
        raise ValueError('gather_normalize_filter: no filter given (gather_normalize is the unfiltered gather)')
    if c > 4 or l > MAX_BUTTER_LEN or (g is not None and l != FFT_FILTER_LEN):
        raise ValueError('gather_normalize_filter: C <= 4, rows of up to %d samples for h and of exactly %d for g expected, '
                         'got C %d, L %d' % (MAX_BUTTER_LEN, FFT_FILTER_LEN, c, l))
    _kernel(h, 'h', l, tiles)
    _kernel(g, 'g', l, tiles)
    mu, std = (list(mu), list(std)) if isinstance(mu, (tuple, list)) else ([mu], [std])
    if len(mu) != c or len(std) != c:
        raise ValueError('gather_normalize_filter: one (mu, std) per channel expected')
    b = idx.numel()
    shape = (b, nb, c, l)
    if out is None:
        out = torch.empty(shape, device=tiles.device, dtype=torch.float32)
    elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == shape):
        raise ValueError('gather_normalize_filter: out must be a contiguous float32 CUDA tensor of shape %s, got %s %s' %
                         (shape, tuple(out.shape), out.dtype))
    if b == 0:
        return out
    dbl = ctypes.c_double * c
    _H._chk(_H._lib.lib().da_gather_normalize_filter(_H._p(tiles), _H._p(idx), dbl(*[float(v) for v in mu]),
                                                     dbl(*[float(v) for v in std]), _H._p(h), _H._p(g), _H._p(out), b, nb, c, l,
                                                     _H._stream()), 'da_gather_normalize_filter')
    return out


def resample_operand(r, device='cuda'):
    """The (new_len, L) matrix of ``filters.resample_matrix`` as ``gather_normalize_chain`` takes it: a float64 tensor of that
    shape on ``device`` whose MEMORY is the transpose (strides (1, new_len)), so that the threads of a wave, one per output
    sample, read consecutive doubles."""
    r = torch.as_tensor(r, dtype=torch.float64)
    if r.dim() != 2:
        raise ValueError('resample_operand: a (new_len, L) matrix expected')
    return r.t().contiguous().to(device).t()


def gather_normalize_chain(tiles, idx, mu, std, padded=False, h=None, r=None, g=None, out=None):
    """tiles (N, NB, C <= 4, L <= 512) float64 CUDA raw windows, idx (B,) int64 CUDA -> (B, NB, C, L) float32: the whole item
    chain of ``ARDSRawDataset.__getitem__`` (dataset.py:1375-1400) per row, in float64, then the cast.  padded: mu is
    subtracted only from non-zero samples (``padded_breath_by_breath`` datasets; zeros stay exactly 0), otherwise
    ``(x - mu) / std`` with the bits of ``gather_normalize``.  Then, each optional: the causal sum with h (L float64 CUDA
    samples), post-hoc downsampling r (the (new_len, L) resampling matrix as ``resample_operand`` lays it out; samples
    new_len .. L - 1 of every row become 0), the circular sum with g (L == 224).  Like ``gather_normalize`` the kernel reads
    tiles[idx[b]] unchecked: idx must already be known to lie in [0, N)."""
    name = 'gather_normalize_chain'
    if not (tiles.is_cuda and tiles.dtype == torch.float64 and tiles.is_contiguous() and tiles.dim() == 4):
        raise ValueError('%s: tiles must be a contiguous float64 CUDA tensor (N, NB, C, L)' % name)
    if not (idx.is_cuda and idx.dtype == torch.int64 and idx.is_contiguous() and idx.dim() == 1):
        raise ValueError('%s: idx must be a contiguous 1-D int64 CUDA tensor' % name)
    _, nb, c, l = tiles.shape
    if c > 4 or l > MAX_BUTTER_LEN or (g is not None and l != FFT_FILTER_LEN):
        raise ValueError('%s: C <= 4, rows of up to %d samples and of exactly %d for g expected, got C %d, L %d' %
                         (name, MAX_BUTTER_LEN, FFT_FILTER_LEN, c, l))
    _kernel(h, 'h', l, tiles, name)
    _kernel(g, 'g', l, tiles, name)
    new_len = 0
    if r is not None:
        if not (r.is_cuda and r.dtype == torch.float64 and r.device == tiles.device and r.dim() == 2 and r.shape[1] == l
                and 1 <= r.shape[0] <= l and r.t().is_contiguous()):
            raise ValueError('%s: r must be a float64 CUDA matrix (1 <= new_len <= %d, %d) laid out by resample_operand()' % (name, l, l))
        new_len = r.shape[0]
    mu, std = (list(mu), list(std)) if isinstance(mu, (tuple, list)) else ([mu], [std])
    if len(mu) != c or len(std) != c:
        raise ValueError('%s: one (mu, std) per channel expected' % name)
    b = idx.numel()
    shape = (b, nb, c, l)
    if out is None:
        out = torch.empty(shape, device=tiles.device, dtype=torch.float32)
    elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == shape):
        raise ValueError('%s: out must be a contiguous float32 CUDA tensor of shape %s, got %s %s' %
                         (name, shape, tuple(out.shape), out.dtype))
    if b == 0:
        return out
    dbl = ctypes.c_double * c
    _H._chk(_H._lib.lib().da_gather_normalize_chain(_H._p(tiles), _H._p(idx), dbl(*[float(v) for v in mu]),
                                                    dbl(*[float(v) for v in std]), int(bool(padded)), _H._p(h), _H._p(r), new_len,
                                                    _H._p(g), _H._p(out), b, nb, c, l, _H._stream()), 'da_gather_normalize_chain')
    return out
