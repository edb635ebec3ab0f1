"""Reference of a chain of residual BasicBlocks (reference models/resnet.py:24-40) for the path tests of
functional.BasicBlockFunction: stock torch on the CPU in float64, per-window train-mode BatchNorm (the vocabulary of
tests/test_functions_gpu.py: ``bnw``), an optional tail [global average pool -> linear_final on view(-1) of every window's
(R, C) block -> BCEWithLogits mean] -- the chain functional.HeadLossFunction replaces.

The ReLU takes an optional MASK: with one it is ``z * mask`` in the forward too, so forward and backward are one function and
the reference can run under the decisions the device took; without, it uses its own sign.  Running statistics: W sequential
momentum updates per BatchNorm with the unbiased variance, and num_batches_tracked.  The same chain in float32 (``dtype``)
gives the reference's own fp32 error per tensor, which is what the device is held to (``bound``).

CASES is the table of chains the GPU tests run, with the path each must take as LITERALS (tests/test_resblock_ref_cpu.py
holds them against the library's host-only predicates, tests/test_resblock_paths_gpu.py against counted launches).
"""
import collections

import numpy as np
import torch
import torch.nn.functional as F

FLOOR, CEIL = 16 * 2.0 ** -23, 1e-4          # the clamp of tests/test_vgg_gpu.py
NEAR = 1e-5                                   # a decision is undecidable where |z| <= NEAR * (1 + max|z|)
NEAR_SHARE = 1e-4                             # ... and at most this share of an activation may be


def bound(err32):
    """What a compared tensor may be off by, relative to 1 + max|ref|: 8 x the reference chain's own float32-vs-float64 error
    on the same inputs (the factor: summation orders a stock fp32 run does not have -- Winograd transforms, split-K slabs),
    clamped to [FLOOR, CEIL]."""
    return min(max(8 * err32, FLOOR), CEIL)


def rel_err(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(got - ref).max() / (1.0 + np.abs(ref).max())) if ref.size else 0.0


def bnw(x, g, b, R, eps=1e-5):
    """per-window train-mode BN on (rows, C, L) CPU tensors"""
    return torch.cat([F.batch_norm(x[i:i + R], None, None, g, b, True, 0.1, eps) for i in range(0, x.shape[0], R)])


def running_stats(y, R, momentum=0.1):
    """(running_mean, running_var, num_batches_tracked) of a fresh BatchNorm1d after one train-mode forward per window of R
    rows of y (rows, C, L), in window order: mean and UNBIASED variance, momentum updates from (0, 1)."""
    y = y.detach().double()
    rm, rv = torch.zeros(y.shape[1], dtype=torch.float64), torch.ones(y.shape[1], dtype=torch.float64)
    w = 0
    for i in range(0, y.shape[0], R):
        win = y[i:i + R]
        rm = (1 - momentum) * rm + momentum * win.mean(dim=(0, 2))
        rv = (1 - momentum) * rv + momentum * win.var(dim=(0, 2), unbiased=True)
        w += 1
    return rm.numpy(), rv.numpy(), w


# ---- the cases ---------------------------------------------------------------------------------------------------------------
# blocks: (cin, planes, stride) each; a block has a downsample iff stride != 1 or cin != planes.  pool_len: what stands in for
# ResNet._map's ``lens[i] == 7`` clause of pool_out.  The expectation, as literals (f32 arithmetic, inside a training step):
#   single   the BatchNorms of the LAST map run single-pass (ReLU bit mask); False: two-stage, `out` saved, mask_mode 2
#   two      the block in front takes the two-term upstream gradient in its bn2 backward (bn_bwd_two / bn_bwd_pair(dout2=));
#            False with a split block behind: it sums dout + d2 on the host
#   pair     a stride-2 entry's BatchNorms run as bn_fwd_pair / bn_bwd_pair
#   pool     the last block pools for the head (bn_fwd_pool / bn_bwd_pool, head on pooled features)
#   raises   the error the case ends in
Case = collections.namedtuple('Case', 'name blocks R W L head pool_len single two pair pool raises wino lone_split force_pool')


def _case(name, blocks, R, W, L, head=False, pool_len=False, single=True, two=False, pair=False, pool=False, raises=None,
          wino=4, lone_split=False, force_pool=False):
    return Case(name, tuple(blocks), R, W, L, head, pool_len, single, two, pair, pool, raises, wino, lone_split, force_pool)


ID2, ENTRY = [(64, 64, 1), (64, 64, 1)], [(64, 128, 2), (128, 128, 1)]
CASES = collections.OrderedDict((c.name, c) for c in [
    _case('id2_L64', ID2, 20, 2, 64, two=True),                       # Wn 1280: the last two-term length
    _case('id2_L65', ID2, 20, 2, 65),                                 # Wn 1300, odd: single-pass mask form, host sum
    _case('id2_L128', ID2, 20, 2, 128),                               # Wn 2560: the last single-pass length
    _case('id2_L129', ID2, 20, 2, 129, single=False),                 # Wn 2580: two-stage
    _case('id2_W128_L160', ID2, 4, 128, 160, two=True),               # 32-channel blocks: two-term up to Wn 640
    _case('id2_W128_L165', ID2, 4, 128, 165),                         # Wn 660
    _case('entry_L128', ENTRY, 20, 2, 128, two=True, pair=True),      # out Wn 1280
    _case('entry_L130', ENTRY, 20, 2, 130, pair=True),                # out Wn 1300
    _case('entry_L258', ENTRY, 20, 2, 258, single=False),             # out Wn 2580: no pair forms
    _case('entry_L57', ENTRY, 20, 2, 57, two=True, pair=True),        # odd length, out L 29
    _case('tail_L7', ID2, 20, 2, 7, head=True, pool_len=True, two=True, pool=True),
    _case('tail_L8', ID2, 20, 2, 8, head=True, pool_len=True, two=True, pool=True),          # Wn 160: the last pooled one
    _case('tail_R8_L7', ID2, 8, 2, 7, head=True, pool_len=True, two=True, pool=True),
    _case('tail_R40_L7', ID2, 40, 2, 7, head=True, pool_len=True, two=True),                 # Wn 280: map stored
    _case('pool_L9', [(64, 64, 1)], 20, 2, 9, pool_len=True, two=True, force_pool=True, raises=ValueError),        # Wn 180
    _case('tail_C512_L7', [(512, 512, 1), (512, 512, 1)], 20, 2, 7, head=True, pool_len=True, two=True, pool=True, wino=6),
    _case('lone_split_L14', [(64, 64, 1)], 20, 2, 14, two=True, lone_split=True, raises=RuntimeError),
])

# seeds: one per case, picked so that the reference's own pre-activations keep off zero (near_zero_share < NEAR_SHARE per
# activation; tests/test_resblock_ref_cpu.py holds every one of them to it)
SEEDS = dict({name: 1 for name in CASES}, tail_L7=3, tail_R8_L7=3, tail_R40_L7=2, tail_C512_L7=2)


def out_len(l, stride):
    return (l - 1) // stride + 1 if stride > 1 else l


def lengths(case):
    lens = [case.L]
    for _, _, s in case.blocks:
        lens.append(out_len(lens[-1], s))
    return lens


def has_ds(blk):
    return blk[2] != 1 or blk[0] != blk[1]


def make_data(case, seed=None):
    """name -> float64 CPU tensor, every value exactly representable in float32: the input x (rows, C, L) (post-ReLU: >= 0),
    the cotangent ``dout`` of the chain output (or ``target`` (W, 2) with a head) and the parameters under the names of a
    list of models.resnet.BasicBlock modules ('<i>.conv1.weight', ...) and 'linear_final.weight' / '.bias'."""
    rng = np.random.default_rng(1000 + (SEEDS[case.name] if seed is None else seed))
    f32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32).astype(np.float64))
    norm = lambda *shape, scale=1.0, shift=0.0: f32(rng.standard_normal(shape) * scale + shift)
    rows, lens = case.R * case.W, lengths(case)
    d = collections.OrderedDict()
    d['x'] = norm(rows, case.blocks[0][0], case.L).clamp_(min=0)
    for i, blk in enumerate(case.blocks):
        cin, planes, _ = blk
        d['%d.conv1.weight' % i] = norm(planes, cin, 3, scale=np.sqrt(2.0 / (3 * planes)))
        d['%d.bn1.weight' % i], d['%d.bn1.bias' % i] = norm(planes, scale=0.2, shift=1.0), norm(planes, scale=0.2)
        d['%d.conv2.weight' % i] = norm(planes, planes, 3, scale=np.sqrt(2.0 / (3 * planes)))
        d['%d.bn2.weight' % i], d['%d.bn2.bias' % i] = norm(planes, scale=0.2, shift=1.0), norm(planes, scale=0.2)
        if has_ds(blk):
            d['%d.downsample.0.weight' % i] = norm(planes, cin, 1, scale=np.sqrt(2.0 / planes))
            d['%d.downsample.1.weight' % i], d['%d.downsample.1.bias' % i] = norm(planes, scale=0.2, shift=1.0), norm(planes, scale=0.2)
    c_out = case.blocks[-1][1]
    if case.head:
        d['linear_final.weight'], d['linear_final.bias'] = norm(2, case.R * c_out, scale=0.05), norm(2, scale=0.05)
        t = np.zeros((case.W, 2))
        t[np.arange(case.W), np.arange(case.W) % 2] = 1
        d['target'] = f32(t)
    else:
        d['dout'] = norm(rows, c_out, lens[-1])
    return d


NOT_PARAMS = ('x', 'dout', 'target')


def param_names(data):
    return [n for n in data if n not in NOT_PARAMS]


def bn_names(case):
    return [n for i, blk in enumerate(case.blocks) for n in ['%d.bn1' % i, '%d.bn2' % i] + (['%d.downsample.1' % i] if has_ds(blk) else [])]


def _relu(z, mask, plain):
    if plain:
        return F.relu(z)
    m = (z.detach() > 0) if mask is None else torch.as_tensor(mask)
    return z * m.to(z.dtype)


def run_ref(case, data, dtype=torch.float64, masks=None, plain=False):
    """The chain forward and backward.  masks: one bool (rows, C, L) array per ReLU in forward order (h1, out of every block),
    or None: the chain's own signs; plain: F.relu and stock autograd throughout.
    -> dict: 'out' (or 'logits', 'loss' with a head), 'dx', 'grads' {parameter name: array}, 'running' {bn name: (mean, var,
    num_batches_tracked)}, 'z' the pre-activations and 'masks' the decisions taken, in forward order."""
    R = case.R
    p = {n: (data[n].to(dtype).clone().requires_grad_(True) if n not in ('dout', 'target') else data[n].to(dtype)) for n in data}
    h, zs, used, running = p['x'], [], [], {}
    masks = list(masks) if masks is not None else None

    def act(z):
        zs.append(z.detach().double().numpy())
        m = masks[len(zs) - 1] if masks is not None else None
        used.append(np.asarray(m, dtype=bool) if m is not None else zs[-1] > 0)
        return _relu(z, m, plain)

    def bn(y, name):
        running[name] = running_stats(y, R)
        return bnw(y, p[name + '.weight'], p[name + '.bias'], R)

    for i, blk in enumerate(case.blocks):
        s = blk[2]
        h1 = act(bn(F.conv1d(h, p['%d.conv1.weight' % i], None, s, 1), '%d.bn1' % i))
        o = bn(F.conv1d(h1, p['%d.conv2.weight' % i], None, 1, 1), '%d.bn2' % i)
        r = bn(F.conv1d(h, p['%d.downsample.0.weight' % i], None, s, 0), '%d.downsample.1' % i) if has_ds(blk) else h
        h = act(o + r)
    res = {}
    if case.head:
        feat = h.mean(dim=2)                                                  # global average pool: (rows, C)
        logits = F.linear(feat.reshape(case.W, -1), p['linear_final.weight'], p['linear_final.bias'])
        loss = F.binary_cross_entropy_with_logits(logits, p['target'])
        loss.backward()
        res['logits'], res['loss'] = logits.detach().double().numpy(), float(loss.detach())
    else:
        h.backward(p['dout'])
        res['out'] = h.detach().double().numpy()
    res['dx'] = p['x'].grad.double().numpy()
    res['grads'] = {n: p[n].grad.double().numpy() for n in param_names(data)}
    res['running'], res['z'], res['masks'] = running, zs, used
    return res


def near_zero_share(z):
    """The share of a pre-activation's elements whose ReLU decision is within rounding of zero."""
    return float((np.abs(z) <= NEAR * (1 + np.abs(z).max())).mean())


def compared(res):
    """name -> array of everything assertion (a) compares."""
    out = {'dx': res['dx']}
    for k in ('out', 'logits', 'loss'):
        if k in res:
            out[k] = np.asarray(res[k], dtype=np.float64)
    out.update({'d ' + n: g for n, g in res['grads'].items()})
    for n, (rm, rv, _) in res['running'].items():
        out[n + '.running_mean'], out[n + '.running_var'] = rm, rv
    return out


# ---- the arithmetic and storage matrix ----------------------------------------------------------------------------------------
# The conv kernels by their da_repack_desc.points names (tests/test_host_cpu.py pins the numbers).
DIRECT, WINO2, WINO4, BF16, X3 = 0, 4, 6, 16, 49
ID_ENTRY = [(64, 64, 1), (64, 128, 2)]
EXTRA = collections.OrderedDict((c.name, c) for c in [
    _case('idE_L57', ID_ENTRY, 20, 2, 57, two=True, pair=True),       # f32x3p: the front block takes x3, the odd entry does not
    _case('idE_L128', ID_ENTRY, 20, 2, 128, two=True, pair=True),     # f32x3p: an X3 entry
    _case('id2_L6', ID2, 20, 2, 6, two=True),                         # bf16, _BN1_FUSED: R L = 120, not fused
    _case('id2_L7', ID2, 20, 2, 7, two=True),                         # ... R L = 140, fused
])
SEEDS.update(idE_L57=2, idE_L128=1, id2_L6=4, id2_L7=3)
ALL_CASES = collections.OrderedDict(list(CASES.items()) + list(EXTRA.items()))

# (conv dtype, storage) -> case -> what runs, as literals: takes3 per block, the entry form of the stride-2 block (None: no
# entry, or its two convs apart), the kernels H.conv_kernel names for the convs outside an entry launch; fused: blocks
# whose bn1 rides on the convs (_BN1_FUSED on); raises: what the Function answers
Arith = collections.namedtuple('Arith', 'takes3 entry kernels fused raises')


def _ar(takes3=(False, False), entry=None, kernels=(), fused=0, raises=None):
    return Arith(tuple(takes3), entry, frozenset(kernels), fused, raises)


ARITH = {
    ('f32x3p', 'f32'): collections.OrderedDict([
        ('id2_L128', _ar((True, True), None, [X3])),                  # the x3 flow: in3, mid3, want_out3
        ('id2_L129', _ar((False, False), None, [WINO2])),             # no store forms: the fp32 kernels
        ('idE_L57', _ar((True, False), DIRECT, [X3])),                # float between the blocks, DIRECT entry
        ('idE_L128', _ar((True, True), X3, [X3])),
    ]),
    ('bf16', 'f32'): collections.OrderedDict([
        ('id2_L64', _ar(kernels=[BF16])), ('id2_L65', _ar(kernels=[BF16])), ('id2_L128', _ar(kernels=[BF16])),
        ('entry_L128', _ar(entry=BF16, kernels=[BF16])), ('entry_L130', _ar(entry=BF16, kernels=[BF16])),
        ('entry_L57', _ar(entry=None, kernels=[DIRECT, BF16])),       # odd: conv1 and the downsample conv apart, fp32 DIRECT
        ('tail_L7', _ar(kernels=[BF16])),
        ('id2_L6', _ar(kernels=[BF16], fused=0)), ('id2_L7', _ar(kernels=[BF16], fused=2)),
    ]),
    ('bf16', 'bf16'): collections.OrderedDict([
        ('id2_L64', _ar(kernels=[BF16])), ('id2_L65', _ar(kernels=[BF16])), ('id2_L128', _ar(kernels=[BF16])),
        ('entry_L128', _ar(entry=BF16, kernels=[BF16])), ('entry_L130', _ar(entry=BF16, kernels=[BF16])),
        ('entry_L57', _ar(entry=None, raises=NotImplementedError)),   # no bf16 kernel at odd length
        ('tail_L7', _ar(kernels=[BF16])),
        ('id2_L6', _ar(kernels=[BF16], fused=0)), ('id2_L7', _ar(kernels=[BF16], fused=2)),
    ]),
}


def arith_f32(case):
    """The same record for fp32 arithmetic, from the case's own literals."""
    entry = DIRECT if any(has_ds(b) for b in case.blocks) else None
    return _ar((False,) * len(case.blocks), entry, [case.wino])
