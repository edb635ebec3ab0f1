"""Batched Grad-CAM from the norm5 map (reference gradcam.py:28-205) as a wrapper of the C ABI (``da_gradcam``; kernels in
csrc/gradcam.hip).  Reached as ``hip_ops.gradcam``; same conventions as the other wrappers: contiguous CUDA operands, the
current stream, no host synchronisation, shapes checked here so that an unsupported one raises with the shape before anything
is launched."""
import collections

import torch

from . import hip_ops as _H

MAX_LM, MAX_NB, MAX_C = 8, 1024, 1920

# every output of one call, all on the device; t = target[b]
GradCamOutputs = collections.namedtuple('GradCamOutputs', (
    'logits',            # (B, 2) float32
    'target',            # (B,) int32: target_in where it is >= 0, else the arg-max of logits (a tie gives 0)
    'A',                 # (B, 2, Lm) float32: the window CAM of both classes, raw
    'R',                 # (B, 2, NB, Lm) float32: the read CAM of both classes, raw
    'cam',               # (B, Lm) float32: max(A_t, 0) (UnNormalizedCam)
    'cam_maxmin',        # (B, Lm) uint8 (MaxMinNormCam.generate_cam)
    'cam_degenerate',    # (B,) uint8: 1 where max r == min r over the window CAM: its bytes are 0
    'read_maxmin',       # (B, NB, Lm) uint8 (MaxMinNormCam.generate_read_cam)
    'read_degenerate',   # (B, NB) uint8: 1 where max r == min r over that row: its bytes are 0
    'read_frac'))        # (B, NB, Lm) uint8 (FracTotalNormCam.generate_read_cam)


def gradcam_shape_ok(nb, lm, c):
    """da_gradcam_shape_ok restated: the shapes csrc/gradcam.hip takes."""
    return 1 <= nb <= MAX_NB and 1 <= lm <= MAX_LM and 32 <= c <= MAX_C and c % 32 == 0


def gradcam_workspace(b, nb, c):
    """Bytes of da_gradcam's workspace."""
    return int(_H._lib.lib().da_gradcam_workspace(b, nb, c))


def gradcam(fmap, weight, bias, target_in, nb, workspace=None):
    """fmap (B * nb, Lm, C) float32 channels-last -- the norm5 map WITHOUT its ReLU, ``features.forward_rlc(x, nb, False)`` --
    with ``linear_final``'s weight (2, nb * C) and bias (2,) and target_in (B,) int32 (0 / 1: that class, -1: the predicted
    one) -> GradCamOutputs: two launches, no backward.  workspace: None (allocated here) or a float32 tensor of at least
    gradcam_workspace() bytes; it is written before it is read."""
    if not (fmap.is_cuda and fmap.dtype == torch.float32 and fmap.dim() == 3 and fmap.is_contiguous() and fmap.data_ptr() % 16 == 0):
        raise ValueError('gradcam: the map must be a contiguous float32 CUDA (rows, Lm, C) tensor, got %s %s %s' %
                         (tuple(fmap.shape), fmap.dtype, fmap.device))
    rows, lm, c = fmap.shape
    if nb < 1 or rows < nb or rows % nb:
        raise ValueError('gradcam: %d rows are not windows of %d' % (rows, nb))
    b = rows // nb
    if not gradcam_shape_ok(nb, lm, c) or rows * lm * c >= 2 ** 31:
        raise _H.HipError('gradcam: unsupported (B, NB, Lm, C) = (%d, %d, %d, %d): C %% 32 == 0 up to %d, NB <= %d, Lm <= %d, '
                          'fewer than 2^31 elements' % (b, nb, lm, c, MAX_C, MAX_NB, MAX_LM))
    if tuple(_H._f32(weight, 'weight').shape) != (2, nb * c) or weight.data_ptr() % 16:
        raise ValueError('gradcam: weight must be (2, NB * C) = (2, %d), got %s' % (nb * c, tuple(weight.shape)))
    if tuple(_H._f32(bias, 'bias').shape) != (2,):
        raise ValueError('gradcam: bias must be (2,), got %s' % (tuple(bias.shape),))
    if not (target_in.is_cuda and target_in.dtype == torch.int32 and target_in.is_contiguous() and tuple(target_in.shape) == (b,)):
        raise ValueError('gradcam: target_in must be a contiguous int32 CUDA (B,) = (%d,) tensor, got %s %s' %
                         (b, tuple(target_in.shape), target_in.dtype))
    L = _H._lib.lib()
    need = L.da_gradcam_workspace(b, nb, c) // 4
    if workspace is None:
        workspace = torch.empty((need,), device=fmap.device, dtype=torch.float32)
    elif _H._f32(workspace, 'workspace').numel() < need or workspace.data_ptr() % 16:
        raise ValueError('gradcam: the workspace needs %d floats' % need)
    dev, f32, u8 = fmap.device, torch.float32, torch.uint8
    out = GradCamOutputs(
        logits=torch.empty((b, 2), device=dev, dtype=f32), target=torch.empty((b,), device=dev, dtype=torch.int32),
        A=torch.empty((b, 2, lm), device=dev, dtype=f32), R=torch.empty((b, 2, nb, lm), device=dev, dtype=f32),
        cam=torch.empty((b, lm), device=dev, dtype=f32), cam_maxmin=torch.empty((b, lm), device=dev, dtype=u8),
        cam_degenerate=torch.empty((b,), device=dev, dtype=u8), read_maxmin=torch.empty((b, nb, lm), device=dev, dtype=u8),
        read_degenerate=torch.empty((b, nb), device=dev, dtype=u8), read_frac=torch.empty((b, nb, lm), device=dev, dtype=u8))
    _H._chk(L.da_gradcam(_H._p(fmap), _H._p(weight), _H._p(bias), _H._p(target_in), b, nb, lm, c, _H._p(workspace),
                         *(_H._p(t) for t in out), _H._stream()), 'da_gradcam')
    return out
