"""The reference of the BasicBlock path tests (tests/tools/resblock_ref.py) held to itself, and its table of expected paths
held to the library's host-only predicates -- no GPU."""
import numpy as np
import pytest
import torch

from tools import resblock_chain as RC
from tools import resblock_ref as RR

_RUNS = {}


def ref_run(name):
    """The float64 chain of a case under its own decisions, once per module."""
    if name not in _RUNS:
        case = RR.ALL_CASES[name]
        _RUNS[name] = RR.run_ref(case, RR.make_data(case))
    return _RUNS[name]


@pytest.fixture(scope='module')
def lib():
    from deepards_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize('name', ['id2_L65', 'entry_L57', 'tail_R8_L7', 'tail_L8', 'lone_split_L14'])
def test_masked_relu_equals_plain_autograd(name):
    """z * mask with the chain's own signs is F.relu under stock autograd: every compared quantity to 1e-12."""
    case = RR.ALL_CASES[name]
    data = RR.make_data(case)
    plain, masked = RR.run_ref(case, data, plain=True), ref_run(name)
    again = RR.run_ref(case, data, masks=masked['masks'])           # ... and handing those signs back changes nothing
    a, b, c = RR.compared(plain), RR.compared(masked), RR.compared(again)
    assert sorted(a) == sorted(b) == sorted(c)
    for n in a:
        assert RR.rel_err(b[n], a[n]) <= 1e-12, n
        assert np.array_equal(b[n], c[n]), n


def test_running_statistics_are_those_of_batchnorm1d():
    """running_stats against a real nn.BatchNorm1d fed one window after the other."""
    rng = np.random.default_rng(3)
    y = torch.from_numpy(rng.standard_normal((12, 8, 5)) * 2 + 1)
    bn = torch.nn.BatchNorm1d(8).double().train()
    for i in range(0, 12, 4):
        bn(y[i:i + 4])
    rm, rv, n = RR.running_stats(y, 4)
    assert np.abs(rm - bn.running_mean.numpy()).max() < 1e-14 and np.abs(rv - bn.running_var.numpy()).max() < 1e-14
    assert n == int(bn.num_batches_tracked) == 3


@pytest.mark.parametrize('name', list(RR.ALL_CASES))
def test_case_loads_and_runs_in_float64(name):
    """Every case of the table loads its parameters into real BasicBlock modules and runs in float64; its seed keeps the
    pre-activations off zero: below NEAR_SHARE of every activation within NEAR * (1 + max|z|) -- a property of the reference
    alone, which the GPU tests rely on."""
    case = RR.ALL_CASES[name]
    data = RR.make_data(case)
    assert all(t.dtype == torch.float64 and torch.equal(t.float().double(), t) for t in data.values())
    stage, head = RC.build_modules(case, data)
    assert len(stage) == len(case.blocks) and (head is not None) == case.head
    for n, p in stage.named_parameters():
        assert torch.equal(p.detach().double(), data[n]), n
    r = ref_run(name)
    cmp = RR.compared(r)
    assert all(np.isfinite(v).all() for v in cmp.values())
    assert sorted(r['grads']) == sorted(RR.param_names(data)) and tuple(r['dx'].shape) == tuple(data['x'].shape)
    assert sorted(r['running']) == sorted(RR.bn_names(case)) and all(v[2] == case.W for v in r['running'].values())
    assert len(r['z']) == 2 * len(case.blocks)
    for i, z in enumerate(r['z']):
        share = RR.near_zero_share(z)
        assert share < RR.NEAR_SHARE, 'activation %d: %.2e of the pre-activations within rounding of zero' % (i, share)


def test_float32_twin_gives_a_bound_inside_the_clamp():
    case = RR.ALL_CASES['id2_L65']
    data = RR.make_data(case)
    r64 = ref_run('id2_L65')
    r32 = RR.run_ref(case, data, dtype=torch.float32, masks=r64['masks'])
    a, b = RR.compared(r64), RR.compared(r32)
    errs = {n: RR.rel_err(b[n], a[n]) for n in a}
    assert 0 < max(errs.values()) < 1e-5, errs                       # fp32 arithmetic, not fp64 and not broken
    assert all(RR.FLOOR <= RR.bound(e) <= RR.CEIL for e in errs.values())
    assert RR.bound(0.0) == RR.FLOOR and RR.bound(1.0) == RR.CEIL and RR.bound(1e-6) == 8e-6


def test_path_table_agrees_with_the_bn_predicates(lib):
    """single / two / pool of every case are what da_bn_mask_words, da_bn_two_ok and da_bn_pool_ok answer for the case's last
    map at the default target of 256 blocks; the lengths named 'last' are last: one position more answers the other way."""
    for case in RR.ALL_CASES.values():
        lo, co = RR.lengths(case)[-1], case.blocks[-1][1]
        wn = case.R * lo
        got = (lib.da_bn_mask_words(case.W, wn, co) > 0, bool(lib.da_bn_two_ok(case.W, wn, co)), bool(lib.da_bn_pool_ok(case.W, wn, co, lo)))
        assert got[0] == case.single and got[1] == case.two, (case.name, got)
        assert got[2] == (case.pool or (case.name in ('id2_L6', 'id2_L7'))), (case.name, got)       # (those two run without a head)
    # the thresholds the table sits on, W C / 32 < 256: single-pass iff Wn <= 2560, two-term iff Wn <= 1280, pooled iff
    # Wn <= 160 and L | Wn; W C / 32 >= 256 (32-channel blocks): two-term up to Wn 640
    assert lib.da_bn_mask_words(2, 2560, 64) > 0 and lib.da_bn_mask_words(2, 2561, 64) == 0
    assert lib.da_bn_two_ok(2, 1280, 64) and not lib.da_bn_two_ok(2, 1281, 64)
    assert lib.da_bn_pool_ok(2, 160, 64, 8) and not lib.da_bn_pool_ok(2, 168, 64, 8) and not lib.da_bn_pool_ok(2, 160, 64, 7)
    assert lib.da_bn_two_ok(128, 640, 64) and not lib.da_bn_two_ok(128, 641, 64) and lib.da_bn_mask_words(128, 660, 64) > 0
    # a stride-2 entry's pair forms ask for single-pass geometry of its OUTPUT map
    for name in ('entry_L128', 'entry_L130', 'entry_L258', 'entry_L57'):
        case = RR.CASES[name]
        lo = RR.lengths(case)[1]
        assert (lib.da_bn_mask_words(case.W, case.R * lo, 128) > 0) == case.pair, name


def _what_runs(case, H):
    """(takes3, entry form, conv kernels) from the predicates BasicBlockFunction asks, block by block; raises what they raise."""
    stage, _ = RC.build_modules(case, RR.make_data(case))
    rows, lens = case.R * case.W, RR.lengths(case)
    takes3 = tuple(blk.takes_x3(rows, li, case.R) for blk, li in zip(stage, lens))
    entry, kernels = None, set()
    for i, blk in enumerate(stage):
        w1, w2, li, lo = blk.conv1.weight.shape, blk.conv2.weight.shape, lens[i], lens[i + 1]
        wd = None if blk.downsample is None else blk.downsample[0].weight.shape
        e = H.s2_entry_kernel(w1, wd, blk.stride, li, takes3[i])
        if wd is not None:
            entry = e
        if e is None:
            kernels.add(H.conv_kernel(*w1, blk.stride, 1, takes3[i], li))
            if wd is not None:
                kernels.add(H.conv_kernel(*wd, blk.stride, 0, False, li))
        mid3 = H.x3_block_ok(rows, lo, w2[0], case.R) and H.conv_kernel_wanted(*w2, 1, 1) == H.X3
        kernels.add(H.conv_kernel(*w2, 1, 1, mid3, lo))
    return takes3, entry, frozenset(kernels)


def test_path_table_agrees_with_the_conv_predicates(lib):
    """takes3, the entry form and the conv kernels of every case under every arithmetic are what takes_x3 (H.x3_block_ok),
    H.s2_entry_kernel and H.conv_kernel answer."""
    from deepards_amd import functional as F_, hip_ops as H
    assert (H.DIRECT, H.WINO2, H.WINO4, H.BF16, H.X3) == (RR.DIRECT, RR.WINO2, RR.WINO4, RR.BF16, RR.X3)
    old = (F_.conv_dtype(), H.ACT, H.WGRAD_BF16)
    try:
        for case in RR.CASES.values():
            exp = RR.arith_f32(case)
            assert _what_runs(case, H) == (exp.takes3, exp.entry, exp.kernels), case.name
        for (dtype, storage), table in RR.ARITH.items():
            H.ACT = torch.float32
            F_.set_conv_dtype(dtype)
            H.ACT = torch.bfloat16 if storage == 'bf16' else torch.float32      # (set_storage_dtype would call the library)
            for name, exp in table.items():
                case = RR.ALL_CASES[name]
                if exp.raises is not None:
                    with pytest.raises(exp.raises):
                        _what_runs(case, H)
                    continue
                assert _what_runs(case, H) == (exp.takes3, exp.entry, exp.kernels), (dtype, storage, name)
                # _BN1_FUSED's shape clause: a window covers a 128-position tile and its halo
                if name in ('id2_L6', 'id2_L7'):
                    assert (case.R * case.L >= 130) == (exp.fused > 0)
    finally:
        H.ACT = torch.float32
        F_.set_conv_dtype(old[0])
        H.ACT, H.WGRAD_BF16 = old[1:]
