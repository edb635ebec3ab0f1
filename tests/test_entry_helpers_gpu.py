"""functional._entry_fwd / _entry_dgrad: the one place a stride-2 block entry (k3 s2 p1 conv + 1x1 s2 downsample reading the
same input) goes from its kernel name (hip_ops.s2_entry_kernel: X3 / BF16 / DIRECT / None) to its launches, against the
numpy oracle (oracle/np_ref.py conv1d_fwd / conv1d_bwd in float64, the data gradient summed over the two convs).

Shapes: the smallest that reach each form -- 4 rows, 64 -> 128 channels, length 8 for the three shared launches; length 7
(odd: the fallback forms -- the direct pair as conv_dgrad twice, conv dtype bf16 apart on the fp32 kernels); 32 -> 64
channels (the direct forms without the 64-channel tail tiles and pair kernels).  Bounds: those tests/test_hip_ops_gpu.py
(direct: 2e-6, bf16 on the bf16-rounded operands: 3e-6, of 1 + max|ref|) and tests/test_x3p_gpu.py (x3: 3e-6 of max|ref|)
hold the same kernels to at these forms."""
import functools

import numpy as np
import pytest
import torch

from oracle import np_ref

pytestmark = pytest.mark.gpu

# conv dtype, Ci, Co, L, x3 input, the entry kernel's name ('none': the convs run apart)
CASES = [('f32', 64, 128, 8, False, 'DIRECT'), ('bf16', 64, 128, 8, False, 'BF16'), ('f32x3p', 64, 128, 8, True, 'X3'),
         ('f32', 64, 128, 7, False, 'DIRECT'), ('bf16', 64, 128, 7, False, 'none'), ('f32x3p', 64, 128, 7, False, 'DIRECT'),
         ('f32', 32, 64, 8, False, 'DIRECT')]
ROWS = 4


@functools.lru_cache(maxsize=None)
def _reference(ci, co, L, rounded):
    """(x, w1, wd, dy1, dyd) float64 NCL and the oracle's (y1, yd, dx) -- on the bf16-rounded operands if ``rounded``."""
    rng = np.random.default_rng(1000 * ci + 10 * co + L)
    r = np_ref.round_bf16 if rounded else (lambda a: a)
    x = rng.standard_normal((ROWS, ci, L))
    w1 = rng.standard_normal((co, ci, 3)) * np.sqrt(2.0 / (3 * co))
    wd = rng.standard_normal((co, ci, 1)) * np.sqrt(2.0 / co)
    y1, yd = np_ref.conv1d_fwd(r(x), r(w1), 2, 1), np_ref.conv1d_fwd(r(x), r(wd), 2, 0)
    dy1, dyd = rng.standard_normal(y1.shape), rng.standard_normal(yd.shape)
    dx = np_ref.conv1d_bwd(r(x), r(w1), r(dy1), 2, 1)[0] + np_ref.conv1d_bwd(r(x), r(wd), r(dyd), 2, 0)[0]
    for a in (x, w1, wd, dy1, dyd, y1, yd, dx):
        a.setflags(write=False)
    return x, w1, wd, dy1, dyd, y1, yd, dx


def _rlc(a):
    return torch.from_numpy(np.ascontiguousarray(a.transpose(0, 2, 1)).astype(np.float32)).cuda()


def _ncl(t):
    return t.detach().cpu().numpy().astype(np.float64).transpose(0, 2, 1)


def _check(got, ref, tol, relative, name):
    err = np.abs(_ncl(got) - ref).max()
    bound = tol * (np.abs(ref).max() if relative else 1.0 + np.abs(ref).max())
    print('%s: max err %.3e, bound %.3e' % (name, err, bound))
    assert err <= bound, '%s: max err %.3e > %.3e' % (name, err, bound)


@pytest.mark.parametrize('dtype,ci,co,L,in3,kernel', CASES)
def test_entry_helpers_against_the_oracle(dtype, ci, co, L, in3, kernel):
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from deepards_amd import functional as F, hip_ops as H
    prev = F.conv_dtype()
    F.set_conv_dtype(dtype)
    try:
        w1s, wds = (co, ci, 3), (co, ci, 1)
        entry = H.s2_entry_kernel(w1s, wds, 2, L, in3)
        assert entry == {'DIRECT': H.DIRECT, 'BF16': H.BF16, 'X3': H.X3, 'none': None}[kernel]
        x, w1, wd, dy1, dyd, y1_ref, yd_ref, dx_ref = _reference(ci, co, L, entry == H.BF16)
        tol, rel = {H.DIRECT: (2e-6, False), H.BF16: (3e-6, False), H.X3: (3e-6, True), None: (2e-6, False)}[entry]
        xt, w1t, wdt = _rlc(x), torch.from_numpy(w1.astype(np.float32)).cuda(), torch.from_numpy(wd.astype(np.float32)).cuda()
        d1t, ddt = _rlc(dy1), _rlc(dyd)
        if entry is not None:
            y1, yd = F._entry_fwd(entry, xt, H.x3_split(xt) if in3 else None, w1t, wdt, 2)
            _check(y1, y1_ref, tol, rel, '%s fwd conv1' % kernel)
            _check(yd, yd_ref, tol, rel, '%s fwd downsample' % kernel)
        if entry == H.BF16:            # the shared launch == the two single launches, bit for bit
            assert torch.equal(y1, H.conv_fwd_bf16_s2(xt, F._pack(w1t, H.BF16)[2]))
            assert torch.equal(yd, H.conv_fwd_bf16_s2(xt, F._pack(wdt, H.BF16)[2]))
        g1, gd = (H.x3_split(d1t), H.x3_split(ddt)) if entry == H.X3 else (d1t, ddt)
        dx = F._entry_dgrad(entry, g1, w1t, gd, wdt, 2, L)
        assert tuple(dx.shape) == (ROWS, L, ci)
        _check(dx, dx_ref, tol, rel, '%s dgrad' % kernel)
        if entry == H.BF16:            # ... and its two-launch form, bit for bit (float storage)
            try:
                F._BF16_DGRAD_PAIR = False
                two = F._entry_dgrad(entry, d1t, w1t, ddt, wdt, 2, L)
            finally:
                F._BF16_DGRAD_PAIR = True
            _check(two, dx_ref, tol, rel, 'BF16 dgrad in two launches')
            assert torch.equal(dx, two)
            assert torch.equal(two, F._entry_dgrad(None, d1t, w1t, ddt, wdt, 2, L))       # (entry None: the same two launches)
    finally:
        F.set_conv_dtype(prev)
