"""Drives a chain of real models.resnet.BasicBlock modules (real nn.BatchNorm1d buffers) over an (rows, L, C) input with the
loop body of ResNet._map -- ``takes_x3``, then ``forward_rlc(h, R, h3, takes3[i + 1], pool_out, split_dx)`` under the same
flag expressions (``flags``; the ``lens[i] == 7`` clause of pool_out is the case's ``pool_len``) -- in three modes:

  eager            no training_step; gradients arrive in ``.grad``
  step             ``with F_.training_step(stage)``: forward, flush_forward(defer=True), backward, flush_backward(); every
                   parameter has ``p._da_grad`` set to a destination tensor, the way the trainer's bucket attaches it
  step-overwrite   the same under F_.grad_overwrite(True), destinations pre-filled with NaN

Two instruments: functional.DECISION_TAP (the device's post-ReLU activations -> the decisions the reference runs under) and
counting wrappers on the hip_ops entry points that tell the paths apart (``counted``, as tests/test_dense_edges_gpu.py has
them), plus a recording dict in functional._STEP['dout2'] (who left a second gradient term, who picked it up).
"""
import collections

import torch
import torch.nn as nn

from . import resblock_ref as RR

MODES = ('eager', 'step', 'step-overwrite')
DEST_FILL = 0.375                 # what a step's gradient destinations hold before it (exact in every format)


def build_modules(case, data):
    """(nn.Sequential of BasicBlocks, linear_final | None) on the CPU with the case's parameters loaded; every key of
    ``data`` that is a parameter must land, and nothing but BatchNorm buffers may be missing."""
    from deepards_amd.models.resnet import BasicBlock, conv1d
    blocks = []
    for blk in case.blocks:
        cin, planes, s = blk
        ds = nn.Sequential(conv1d(cin, planes, 1, s), nn.BatchNorm1d(planes)) if RR.has_ds(blk) else None
        blocks.append(BasicBlock(cin, planes, s, ds))
    stage = nn.Sequential(*blocks)
    sd = {n: data[n].float() for n in RR.param_names(data) if not n.startswith('linear_final')}
    r = stage.load_state_dict(sd, strict=False)
    assert not r.unexpected_keys, r.unexpected_keys
    assert all(k.rsplit('.', 1)[1] in ('running_mean', 'running_var', 'num_batches_tracked') for k in r.missing_keys), r.missing_keys
    head = None
    if case.head:
        head = nn.Linear(case.R * case.blocks[-1][1], 2)
        head.load_state_dict({'weight': data['linear_final.weight'].float(), 'bias': data['linear_final.bias'].float()})
    return stage, head


def flags(blocks, takes3, i, fused, pool_len, h, R):
    """(pool_out, split_dx) of block i: ResNet._map's expressions, with ``pool_len`` for its ``lens[i] == 7``."""
    from deepards_amd import functional as F_
    from deepards_amd.models import resnet as R_
    blk = blocks[i]
    pool_out = fused and R_._FUSED_TAIL and i == len(blocks) - 1 and not takes3[i] and \
        blk.downsample is None and blk.stride == 1 and pool_len and F_.H.bn_pool_ok(h, R)
    split_dx = R_._SPLIT_DX and i > 0 and blk.downsample is None and not takes3[i] and not takes3[i - 1]
    return bool(pool_out), bool(split_dx)


class counted(object):
    """Wraps hip_ops entry points for the duration of a run: calls[name] = one small record per call."""
    NAMES = ('bn_fwd', 'bn_fwd_pair', 'bn_fwd_pool', 'bn_fwd_x', 'bn_bwd', 'bn_bwd_two', 'bn_bwd_pair', 'bn_bwd_pool', 'bn_bwd_x',
             'bn_bwd_ss', 'conv_fwd', 'conv_dgrad', 'conv_fwd_multi', 'conv_dgrad_s2_pair', 'conv3_winograd', 'conv3_x3p',
             'conv3_bf16', 'conv3_bf16_bn', 'conv_x3p_s2_fwd', 'conv_x3p_s2_dgrad', 'conv_fwd_bf16_s2', 'conv_dgrad_bf16_s2',
             'conv_dgrad_bf16_s2_pair', 'head_fwd', 'head_flat_fwd', 'bn_running_multi', 'step_tail_multi', 'conv_kernel',
             's2_entry_kernel')

    def __enter__(self):
        from deepards_amd import hip_ops
        self.H, self.old, self.calls = hip_ops, {}, {n: [] for n in self.NAMES}
        for n in self.NAMES:
            self.old[n] = getattr(hip_ops, n)
            setattr(hip_ops, n, self._wrap(n, self.old[n]))
        return self.calls

    def _wrap(self, name, fn):
        def wrapped(*a, **kw):
            rec = None
            if name == 'bn_bwd':                        # (mask_mode, took the ReLU bit mask)
                rec = (a[7], kw.get('mask') is not None)
            elif name == 'bn_bwd_pair':                 # with the second term of the upstream gradient
                rec = kw.get('dout2') is not None
            r = fn(*a, **kw)
            if name in ('conv_kernel', 's2_entry_kernel'):
                rec = r
            elif name in ('bn_running_multi', 'step_tail_multi'):
                rec = len(a[0]) if name == 'bn_running_multi' else len(a[2])      # running-statistics items of the launch
            self.calls[name].append(rec)
            return r
        return wrapped

    def __exit__(self, *exc):
        for n, fn in self.old.items():
            setattr(self.H, n, fn)


class _Dout2(dict):
    """functional._STEP['dout2'] that remembers: ``left`` second terms stored, ``taken`` picked up."""

    def __init__(self):
        dict.__init__(self)
        self.left, self.taken = 0, 0

    def __setitem__(self, k, v):
        self.left += 1
        dict.__setitem__(self, k, v)

    def pop(self, k, *default):
        had = k in self
        v = dict.pop(self, k, *default)
        self.taken += int(had)
        return v


def _to_rlc(t, dtype):
    return t.permute(0, 2, 1).contiguous().float().cuda().to(dtype)


def _from_rlc(t):
    return t.detach().float().cpu().permute(0, 2, 1).contiguous()


def tap_masks(taps):
    """The decisions of the recorded post-ReLU activations (float / bf16 (rows, L, C) or x3) as bool (rows, C, L) arrays."""
    out = []
    for t in taps:
        if t.dim() == 5:                                # x3: the sign of the leading term is the sign of the value
            t = t[:, :, :, 0, :].reshape(t.shape[0], t.shape[1], -1)
        out.append((t.detach().float() > 0).permute(0, 2, 1).cpu().numpy())
    return out


def run_chain(case, data, mode='eager', tap=False, dest_fill=DEST_FILL):
    """One forward / backward of the case's chain on the device under the conv / storage types and switches that are set.
    -> dict: 'raw' name -> CPU float tensor with the device's bits ('out' | 'logits', 'loss'; 'dx'; 'grad <param>' what
    autograd returned or 'dest <param>' a step's destination; '<bn>.running_mean' / '.running_var' / '.num_batches_tracked'),
    'masks' (tap), 'calls' (counted), 'left' / 'taken' (second gradient terms), 'flags' [(takes3, pool_out, split_dx)],
    'ov_ok' functional._OV['ok'] after the run."""
    from deepards_amd import functional as F_
    H = F_.H
    assert mode in MODES
    stage, head = build_modules(case, data)
    stage, head = stage.cuda().train(), (head.cuda() if head is not None else None)
    blocks, R, rows = list(stage), case.R, case.R * case.W
    named = [(n, p) for n, p in stage.named_parameters()] + \
        ([('linear_final.' + n, p) for n, p in head.named_parameters()] if head is not None else [])
    dests = collections.OrderedDict()
    if mode != 'eager':
        fill = float('nan') if mode == 'step-overwrite' else dest_fill
        for n, p in named:
            dests[n] = p._da_grad = torch.full_like(p, fill)
    x = _to_rlc(data['x'], H.ACT).requires_grad_(True)
    lens = RR.lengths(case)
    res = {'flags': []}
    ov_old = dict(F_._OV)
    F_._OV['ok'] = True
    dout2 = _Dout2()
    taps = []
    try:
        with counted() as calls:
            if tap:
                F_.DECISION_TAP = taps

            def forward():
                takes3 = [blk.takes_x3(rows, li, R) for blk, li in zip(blocks, lens)] + [False]
                h, leaf = x, x
                if takes3[0]:                           # the x3 input of a first block that takes one
                    h3 = H.x3_split(x.detach())
                    leaf = F_.x3_handle(h3).detach().requires_grad_(True)
                    h = (leaf, h3)
                for i, blk in enumerate(blocks):
                    hin = h[0] if takes3[i] else h
                    pool_out, split_dx = flags(blocks, takes3, i, case.head, case.pool_len, hin, R)
                    pool_out, split_dx = pool_out or case.force_pool, split_dx or (case.lone_split and i == 0)
                    res['flags'].append((takes3[i], pool_out, split_dx))
                    if takes3[i]:
                        h, h3 = h
                        h = blk.forward_rlc(h, R, h3, takes3[i + 1])
                    else:
                        h = blk.forward_rlc(h, R, None, takes3[i + 1], pool_out, split_dx)
                if head is not None:
                    return leaf, F_.head_loss(h, head.weight, head.bias, data['target'].float().cuda(), R)
                return leaf, h

            def backward(out):
                if head is not None:
                    out[0].backward(torch.ones_like(out[0]))
                else:
                    out.backward(_to_rlc(data['dout'], H.ACT))

            if mode == 'eager':
                leaf, out = forward()
                backward(out)
            else:
                F_.grad_overwrite(mode == 'step-overwrite')
                with F_.training_step(stage):
                    F_._STEP['dout2'] = dout2
                    leaf, out = forward()
                    F_.flush_forward(defer=True)
                    backward(out)
                    F_.flush_backward()
            torch.cuda.synchronize()
    finally:
        F_.DECISION_TAP = None
        F_.grad_overwrite(ov_old['on'])
        res['ov_ok'] = F_._OV['ok']
        F_._OV['ok'] = ov_old['ok']
    raw = collections.OrderedDict()
    if head is not None:                # (inside a step the backward fills them)
        raw['loss'], raw['logits'] = out[0].detach().float().cpu(), out[1].detach().float().cpu()
    else:
        raw['out'] = _from_rlc(out)
    raw['dx'] = _from_rlc(leaf.grad)
    for n, p in named:
        if mode == 'eager':
            raw['grad ' + n] = p.grad.detach().float().cpu()
        else:
            assert p.grad is None, '%s: a parameter with a destination got a .grad too' % n
            raw['dest ' + n] = dests[n].detach().float().cpu()
    for n in RR.bn_names(case):
        bn = stage.get_submodule(n)
        raw[n + '.running_mean'], raw[n + '.running_var'] = bn.running_mean.detach().cpu(), bn.running_var.detach().cpu()
        raw[n + '.num_batches_tracked'] = bn.num_batches_tracked.detach().cpu()
    res.update(raw=raw, masks=tap_masks(taps) if tap else None, calls=calls, left=dout2.left, taken=dout2.taken)
    return res


def as_compared(raw, mode, dest_fill=DEST_FILL):
    """The device's results under the names of resblock_ref.compared (float64 arrays): a step's destinations minus what they
    held before it."""
    out = {}
    for n, t in raw.items():
        a = t.double().numpy()
        if n.startswith('grad '):
            out['d ' + n[5:]] = a
        elif n.startswith('dest '):
            out['d ' + n[5:]] = a - (0.0 if mode == 'step-overwrite' else dest_fill)
        elif not n.endswith('num_batches_tracked'):
            out[n] = a.reshape(()) if n == 'loss' else a
    return out
