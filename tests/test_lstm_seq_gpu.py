"""GPU tests of the waveform-LSTM kernels (csrc/lstm_seq.hip, deepards_amd/lstm_seq_ops.py), the lstm_only networks, the
trainer and the two driver classes.

Yardstick of every comparison: the case in float64 stock torch on the CPU is the reference; the SAME case in float32 stock
torch (nn.LSTM / nn.Linear) gives the error a float32 implementation makes; the kernels' max error may be at most 8 times
that (both relative to the output's max magnitude: the factor cancels).  The margin covers another summation order and the
device expf / tanhf over 224 dependent steps.  Every figure is printed before it is asserted."""
import ctypes
import os
import sys
import zlib

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, 'tests', 'golden')
MARGIN = 8.0

from tools import poison as P                                                       # noqa: E402
from test_lstm_only_cpu import CASES, load_golden, golden_params, restated          # noqa: E402

if torch.cuda.is_available():
    from deepards_amd import _lib, hip_ops as H, lstm_seq_ops as S
else:                                   # collected without a GPU (-m "not gpu" deselects every test of this file)
    _lib = H = S = None


# ---- inputs and references ----------------------------------------------------------------------------------------------
def rng_of(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def weights(h, g):
    """nn.LSTM(1, h)'s four parameters under torch's default initialisation, as float32 CPU tensors."""
    k = 1.0 / np.sqrt(h)
    u = lambda *s: (torch.rand(*s, generator=g) * 2 - 1) * k
    return u(4 * h, 1), u(4 * h, h), u(4 * h), u(4 * h)


def rows_of(n, t, scale, g, packed):
    """n rows at data scale (unit normal) times ``scale``; with ``packed`` they cycle through the row kinds of the length rule:
    zeros from 100 on, a zero at 0, zeros from 1 on, a zero only at the last sample, no zero, all zeros, a -0.0 in the middle."""
    x = torch.randn(n, t, generator=g) * scale
    x[x == 0] = 1.0
    if packed:
        for r in range(n):
            kind = r % 7
            if kind == 0:
                x[r, min(100, t - 1):] = 0.0
            elif kind == 1:
                x[r, 0] = 0.0
            elif kind == 2:
                x[r, 1:] = 0.0
            elif kind == 3:
                x[r, t - 1] = 0.0
            elif kind == 5:
                x[r, :] = 0.0
            elif kind == 6:
                x[r, t // 2] = -0.0
    return x


def lengths(x):
    t = x.shape[1]
    out = []
    for r in x:
        z = (r == 0).nonzero()
        out.append(int(z[0]) + 1 if z.numel() and int(z[0]) > 0 else t)
    return out


def torch_lstm(x, ws, dhs, lens, dtype):
    """Stock nn.LSTM on the CPU in ``dtype`` -> hs (masked behind the lengths), gradients of sum(hs * dhs) on the four
    parameters (float64 numpy)."""
    h = ws[1].shape[1]
    m = torch.nn.LSTM(1, h, batch_first=True).to(dtype)
    with torch.no_grad():
        for p, w in zip((m.weight_ih_l0, m.weight_hh_l0, m.bias_ih_l0, m.bias_hh_l0), ws):
            p.copy_(w.to(dtype))
    out = m(x.to(dtype).unsqueeze(-1))[0]
    mask = (torch.arange(x.shape[1]).unsqueeze(0) < torch.tensor(lens).unsqueeze(1)).to(dtype).unsqueeze(-1)
    out = out * mask
    (out * dhs.to(dtype)).sum().backward()
    grads = [p.grad.double().numpy() for p in (m.weight_ih_l0, m.weight_hh_l0, m.bias_ih_l0, m.bias_hh_l0)]
    return out.detach().double().numpy(), grads


def judge(what, got, ref64, ref32, ratios=None):
    """max |got - ref64| <= MARGIN * max |ref32 - ref64|, printed first."""
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), what
    e, e32, mag = np.abs(got - ref64).max(), np.abs(ref32 - ref64).max(), np.abs(ref64).max()
    ratio = e / e32 if e32 > 0 else (0.0 if e == 0 else float('inf'))
    print('%-58s err %.3e  fp32 torch %.3e  ratio %6.2f  (max |ref| %.3e)' % (what, e, e32, ratio, mag))
    if ratios is not None:
        ratios.append(ratio)
    assert e <= MARGIN * e32, '%s: error %.3e is %.2f x the float32 torch error %.3e (allowed %g x)' % (what, e, ratio, e32, MARGIN)


def cu(*ts):
    return [t.cuda().contiguous() for t in ts]


def n_values(h):
    spb = S.block_seqs(h)
    return sorted({1, max(1, spb - 1), spb + 1, 2 * spb + 3})


# ---- the recurrence kernels against float64 torch ------------------------------------------------------------------------
@pytest.mark.parametrize('scale', [1.0, 50.0])
@pytest.mark.parametrize('packed', [False, True])
@pytest.mark.parametrize('t', [1, 2, 224])
@pytest.mark.parametrize('h', [8, 16, 24, 64])
def test_recurrence_against_float64(h, t, packed, scale):
    """hs and the three parameter gradients at N = 1, one fewer and one more than a block's sequences, and a non-multiple;
    with ``packed`` the rows take every kind of zero pattern, hs behind a length is +0.0 bit for bit and the lengths are the
    rule's.  scale 50: saturated gates, finite results."""
    for n in n_values(h):
        g = rng_of('rec', h, t, int(packed), int(scale), n)
        ws = weights(h, g)
        x = rows_of(n, t, scale, g, packed)
        dhs = torch.randn(n, t, h, generator=g)
        lens = lengths(x) if packed else [t] * n
        hs64, g64 = torch_lstm(x, ws, dhs, lens, torch.float64)
        hs32, g32 = torch_lstm(x, ws, dhs, lens, torch.float32)
        xd, dd = cu(x, dhs)
        wd = cu(*ws)
        hs, cs, ln = S.lstm_seq_fwd(xd, *wd, packed=packed)
        assert ln.tolist() == lens
        tag = 'H %d T %d N %d packed %d x%g' % (h, t, n, packed, scale)
        judge(tag + ' hs', hs.cpu().numpy(), hs64, hs32)
        if packed:
            behind = torch.arange(t).unsqueeze(0) >= torch.tensor(lens).unsqueeze(1)
            assert not hs.cpu().view(torch.int32)[behind].any(), 'hs behind a length must be +0.0 bit for bit'
        dw_ih, dw_hh, db = S.lstm_seq_bwd(dd, xd, *wd, hs, cs, ln)
        for name, got, r64, r32 in (('dw_ih', dw_ih, g64[0], g32[0]), ('dw_hh', dw_hh, g64[1], g32[1]), ('db', db, g64[2], g32[2])):   # (the one db serves both biases)
            judge(tag + ' ' + name, got.cpu().numpy(), r64, r32)


def test_packed_gradients_ignore_dhs_behind_the_lengths():
    g = rng_of('ignore')
    ws, x, dhs = weights(16, g), rows_of(9, 224, 1.0, g, True), torch.randn(9, 224, 16, generator=g)
    lens = torch.tensor(lengths(x))
    xd, dd = cu(x, dhs)
    wd = cu(*ws)
    hs, cs, ln = S.lstm_seq_fwd(xd, *wd, packed=True)
    first = S.lstm_seq_bwd(dd, xd, *wd, hs, cs, ln)
    behind = (torch.arange(224).unsqueeze(0) >= lens.unsqueeze(1)).cuda()
    assert behind.any()
    dd2 = dd.clone()
    dd2[behind] = float('nan')
    second = S.lstm_seq_bwd(dd2, xd, *wd, hs, cs, ln)
    for a, b in zip(first, second):
        assert P.same_bits(a, b) and torch.isfinite(b).all()


def test_a_sequence_does_not_depend_on_its_neighbours_or_position():
    """One row alone (N = 1) and at the first, a middle and the last position of N = 7: the same hs and cs bits."""
    for h in (8, 16, 24):
        for packed in (False, True):
            g = rng_of('alone', h, int(packed))
            ws, x = weights(h, g), rows_of(7, 224, 1.0, g, packed)
            wd = cu(*ws)
            row = x[2:3]
            alone = S.lstm_seq_fwd(row.cuda().contiguous(), *wd, packed=packed)
            for pos in (0, 3, 6):
                y = x.clone()
                y[pos] = row[0]
                many = S.lstm_seq_fwd(y.cuda().contiguous(), *wd, packed=packed)
                assert P.same_bits(alone[0][0], many[0][pos]) and P.same_bits(alone[1][0], many[1][pos])
                assert int(alone[2][0]) == int(many[2][pos])


def test_two_identical_calls_are_bit_equal():
    for h, n in ((8, 5), (16, 37), (64, 3)):
        g = rng_of('twice', h)
        ws, x, dhs = weights(h, g), rows_of(n, 224, 1.0, g, True), torch.randn(n, 224, h, generator=g)
        xd, dd = cu(x, dhs)
        wd = cu(*ws)
        a = S.lstm_seq_fwd(xd, *wd, packed=True)
        b = S.lstm_seq_fwd(xd, *wd, packed=True)
        assert all(P.same_bits(u, v) for u, v in zip(a, b))
        ga = S.lstm_seq_bwd(dd, xd, *wd, *a)
        gb = S.lstm_seq_bwd(dd, xd, *wd, *b)
        assert all(P.same_bits(u, v) for u, v in zip(ga, gb))
        w, bias = torch.randn(16, 224 * h, generator=g).cuda() * 0.02, torch.randn(16, generator=g).cuda()
        rows, dy = a[0].view(n, -1), torch.randn(n, 16, generator=g).cuda()
        assert P.same_bits(S.proj_fwd(rows, w, bias), S.proj_fwd(rows, w, bias))
        assert all(P.same_bits(u, v) for u, v in zip(S.proj_bwd(dy, rows, w, bias), S.proj_bwd(dy, rows, w, bias)))


def test_accumulate_adds_to_the_destinations():
    g = rng_of('acc')
    ws, x, dhs = weights(16, g), rows_of(5, 224, 1.0, g, False), torch.randn(5, 224, 16, generator=g)
    xd, dd = cu(x, dhs)
    wd = cu(*ws)
    hs, cs, ln = S.lstm_seq_fwd(xd, *wd)
    dw_ih, dw_hh, db = S.lstm_seq_bwd(dd, xd, *wd, hs, cs, ln)
    base = [torch.randn_like(t) for t in (dw_ih, dw_hh, db, db)]
    dst = [t.clone() for t in base]
    S.lstm_seq_bwd(dd, xd, *wd, hs, cs, ln, dw_ih=dst[0], dw_hh=dst[1], db=dst[2], db2=dst[3], accumulate=True)
    for d, b0, gr in zip(dst, base, (dw_ih, dw_hh, db, db)):
        assert P.same_bits(d, b0 + gr)
    S.lstm_seq_bwd(dd, xd, *wd, hs, cs, ln, dw_ih=dst[0], dw_hh=dst[1], db=dst[2], db2=dst[3], accumulate=False)
    for d, gr in zip(dst, (dw_ih, dw_hh, db, db)):
        assert P.same_bits(d, gr)


# ---- refusals and memory discipline ---------------------------------------------------------------------------------------
def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def test_refused_shapes_return_minus_one_and_touch_nothing():
    lib = _lib.lib()
    st = H._stream()
    for h, t in ((4, 224), (12, 224), (72, 224), (16, 0)):
        n, tt = 3, max(t, 1)
        x = torch.randn(n, tt).cuda()
        w_ih, w_hh, b = torch.randn(4 * h).cuda(), torch.randn(4 * h, h).cuda(), torch.randn(4 * h).cuda()
        hs, cs = torch.empty(n, tt, h).cuda(), torch.empty(n, tt, h).cuda()
        lens = torch.empty(n, dtype=torch.int32).cuda()
        dws = [torch.empty(4 * h).cuda(), torch.empty(4 * h, h).cuda(), torch.empty(4 * h).cuda()]
        work = torch.empty(1 << 16).cuda()
        for o in [hs, cs, lens, work] + dws:
            P.fill_poison(o)
        assert lib.da_lstm_seq_fwd(_ptr(x), _ptr(w_ih), _ptr(w_hh), _ptr(b), _ptr(b), 0, _ptr(hs), _ptr(cs), _ptr(lens), n, t, h,
                                   st) == -1
        assert lib.da_lstm_seq_bwd(_ptr(hs), _ptr(x), _ptr(w_ih), _ptr(w_hh), _ptr(b), _ptr(b), _ptr(hs), _ptr(cs), _ptr(lens),
                                   _ptr(dws[0]), _ptr(dws[1]), _ptr(dws[2]), None, _ptr(work), 0, n, t, h, st) == -1
        assert h == 16 or lib.da_lstm_seq_bwd_workspace(n, h) == 0
        torch.cuda.synchronize()
        for o in [hs, cs, lens, work] + dws:
            assert P.count_poison(o) == o.numel()
    assert lib.da_lstm_seq_block_seqs(12) == -1 and lib.da_lstm_seq_bwd_workspace(3, 12) == 0
    rows, w, bias = torch.randn(3, 32).cuda(), torch.randn(24, 32).cuda(), torch.randn(24).cuda()
    for f, k in ((8, 32), (24, 32), (80, 32), (16, 30), (16, 0)):
        y, drows, dw, dbias = torch.empty(3, 80).cuda(), torch.empty(3, 32).cuda(), torch.empty(80, 32).cuda(), torch.empty(80).cuda()
        for o in (y, drows, dw, dbias):
            P.fill_poison(o)
        assert lib.da_lstm_seq_proj_fwd(_ptr(rows), _ptr(w), _ptr(bias), _ptr(y), 3, k, f, st) == -1
        assert lib.da_lstm_seq_proj_bwd(_ptr(y), _ptr(rows), _ptr(w), _ptr(drows), _ptr(dw), _ptr(dbias), _ptr(y), 0, 3, k, f,
                                        st) == -1
        assert lib.da_lstm_seq_proj_bwd_workspace(3, k, f) == 0
        torch.cuda.synchronize()
        for o in (y, drows, dw, dbias):
            assert P.count_poison(o) == o.numel()
    with pytest.raises(ValueError):
        S.lstm_seq_fwd(torch.randn(3, 224).cuda(), *cu(*weights(12, rng_of('r'))))


@pytest.mark.parametrize('h,n,t', [(8, 3, 224), (16, 5, 224), (24, 2, 7), (64, 2, 224)])
def test_guard_bands_stay_intact(h, n, t):
    """Every operand, output and workspace of the four entry points inside pattern-filled guard bands: the results keep the
    bits of the plain call and no guard word changes."""
    lib, st = _lib.lib(), H._stream()
    g = rng_of('guard', h, n, t)
    ws, x, dhs = weights(h, g), rows_of(n, t, 1.0, g, True), torch.randn(n, t, h, generator=g)
    f, k = 16, t * h
    w, bias, dy = torch.randn(f, k, generator=g) * 0.05, torch.randn(f, generator=g), torch.randn(n, f, generator=g)
    xd, dd, wp, bp, dyd = cu(x, dhs, w, bias, dy)
    wd = cu(*ws)
    hs, cs, ln = S.lstm_seq_fwd(xd, *wd, packed=True)
    grads = S.lstm_seq_bwd(dd, xd, *wd, hs, cs, ln)
    y = S.proj_fwd(hs.view(n, k), wp, bp)
    pg = S.proj_bwd(dyd, hs.view(n, k), wp, bp)
    handles = []

    def gd(tensor):
        v, hd = P.guarded(tensor)
        handles.append(hd)
        return v
    gx, gdd, gwp, gbp, gdy = [gd(v) for v in (xd, dd, wp, bp, dyd)]
    gw = [gd(v) for v in wd]
    ghs, gcs, gln = gd(torch.zeros_like(hs)), gd(torch.zeros_like(cs)), gd(torch.zeros_like(ln))
    gg = [gd(torch.zeros_like(v)) for v in grads]
    work = gd(torch.zeros(lib.da_lstm_seq_bwd_workspace(n, h) // 4, device='cuda'))
    assert lib.da_lstm_seq_fwd(_ptr(gx), *[_ptr(v) for v in gw], 1, _ptr(ghs), _ptr(gcs), _ptr(gln), n, t, h, st) == 0
    assert lib.da_lstm_seq_bwd(_ptr(gdd), _ptr(gx), *[_ptr(v) for v in gw], _ptr(ghs), _ptr(gcs), _ptr(gln), _ptr(gg[0]),
                               _ptr(gg[1]), _ptr(gg[2]), None, _ptr(work), 0, n, t, h, st) == 0
    gy, gdr, gdw, gdb = gd(torch.zeros_like(y)), gd(torch.zeros_like(pg[0])), gd(torch.zeros_like(pg[1])), gd(torch.zeros_like(pg[2]))
    pwork = gd(torch.zeros(lib.da_lstm_seq_proj_bwd_workspace(n, k, f) // 4, device='cuda'))
    assert lib.da_lstm_seq_proj_fwd(_ptr(ghs), _ptr(gwp), _ptr(gbp), _ptr(gy), n, k, f, st) == 0
    assert lib.da_lstm_seq_proj_bwd(_ptr(gdy), _ptr(ghs), _ptr(gwp), _ptr(gdr), _ptr(gdw), _ptr(gdb), _ptr(pwork), 0, n, k, f,
                                    st) == 0
    torch.cuda.synchronize()
    P.assert_guards_intact(handles)
    for a, b in zip((ghs, gcs, gln) + tuple(gg) + (gy, gdr, gdw, gdb), (hs, cs, ln) + tuple(grads) + (y,) + tuple(pg)):
        assert P.same_bits(a, b)


def test_poisoned_allocations_do_not_reach_the_results():
    g = rng_of('poison')
    ws, x, dhs = weights(16, g), rows_of(5, 224, 1.0, g, True), torch.randn(5, 224, 16, generator=g)
    xd, dd = cu(x, dhs)
    wd = cu(*ws)
    clean_f = S.lstm_seq_fwd(xd, *wd, packed=True)
    clean_b = S.lstm_seq_bwd(dd, xd, *wd, *clean_f)
    with P.poisoned_allocations() as stats:
        f = S.lstm_seq_fwd(xd, *wd, packed=True)
        b = S.lstm_seq_bwd(dd, xd, *wd, *f)
    assert stats.filled > 0
    assert P.same_bits(f[0], clean_f[0]) and P.same_bits(f[2], clean_f[2]) and all(P.same_bits(u, v) for u, v in zip(b, clean_b))
    assert not P.has_poison(f[0]) and not any(P.has_poison(u) for u in b)


# ---- the projection ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('f', [16, 64])
@pytest.mark.parametrize('n,k', [(1, 8), (3, 1792), (5, 48), (33, 1792), (70, 3584)])
def test_projection_against_float64(n, k, f):
    """Linear(K -> F) forward and backward: N below, at a non-multiple of and across the 4-row tiles and the 32-row chunks."""
    g = rng_of('proj', n, k, f)
    rows, w, bias, dy = torch.randn(n, k, generator=g) * 0.3, (torch.rand(f, k, generator=g) * 2 - 1) / np.sqrt(k), \
        torch.randn(f, generator=g) * 0.1, torch.randn(n, f, generator=g)

    def ref(dtype):
        r, ww, bb = rows.to(dtype).requires_grad_(True), w.to(dtype).requires_grad_(True), bias.to(dtype).requires_grad_(True)
        y = torch.nn.functional.linear(r, ww, bb)
        (y * dy.to(dtype)).sum().backward()
        return [v.detach().double().numpy() for v in (y, r.grad, ww.grad, bb.grad)]
    r64, r32 = ref(torch.float64), ref(torch.float32)
    rd, wd, bd, dd = cu(rows, w, bias, dy)
    got = (S.proj_fwd(rd, wd, bd),) + S.proj_bwd(dd, rd, wd, bd)
    for name, a, b64, b32 in zip(('y', 'drows', 'dw', 'dbias'), got, r64, r32):
        judge('proj N %d K %d F %d %s' % (n, k, f, name), a.cpu().numpy(), b64, b32)


# ---- the models against the goldens -----------------------------------------------------------------------------------------
def build(name):
    import deepards_amd.models as M
    z = load_golden(name)
    b, nb, h = [int(v) for v in z['shape']]
    cls = M.LSTMOnlyWithPacking if CASES[name] else M.LSTMOnlyNetwork
    m = cls(h, nb)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in golden_params(z).items()}, strict=True)
    return z, m.cuda()


@pytest.mark.parametrize('name', sorted(CASES))
def test_model_against_the_goldens(name):
    """Logits and every parameter gradient of sum(logits * r) against the reference's float64 record; the yardstick is the
    float32 run of the stock-torch restatement of tests/test_lstm_only_cpu.py."""
    z, m = build(name)
    l32, g32, _ = restated(golden_params(z), z['x'], z['r'], CASES[name], dtype=torch.float32)
    logits = m(torch.from_numpy(z['x']).cuda(), None)
    assert tuple(logits.shape) == z['logits'].shape
    (logits * torch.from_numpy(z['r']).cuda()).sum().backward()
    judge(name + ' logits', logits.detach().cpu().numpy(), z['logits'], l32.astype(np.float64))
    for k, p in m.named_parameters():
        judge('%s grad %s' % (name, k), p.grad.cpu().numpy(), z['grad/' + k], g32[k].astype(np.float64))


# ---- trainer and drivers --------------------------------------------------------------------------------------------------------
def _target(b):
    t = torch.zeros(b, 2)
    t[torch.arange(b), torch.arange(b) % 2] = 1.0
    return t.cuda()


@pytest.mark.parametrize('optimizer', ['sgd', 'adam'])
@pytest.mark.parametrize('name', ['2x3x8', 'packing_2x4x8'])
def test_eager_and_captured_steps_agree_bit_for_bit(name, optimizer):
    from deepards_amd.train import HotPathTrainer
    z, _ = build(name)
    x, t = torch.from_numpy(z['x']).cuda(), _target(z['x'].shape[0])
    out = []
    for use_graph in (False, True):
        m = build(name)[1]
        tr = HotPathTrainer(m, optimizer=optimizer, learning_rate=1e-2, use_graph=use_graph)
        losses = [tr.train_step(x, t).clone() for _ in range(3)]
        test = tr.test_step(x, t)
        assert tuple(test[1].shape) == (x.shape[0], 2) and torch.isfinite(test[0]).all()
        out.append((losses, [p.detach().clone() for p in m.parameters()], test))
        tr.release_graphs()
    (l0, p0, t0), (l1, p1, t1) = out
    assert all(torch.isfinite(v).all() for v in l0)
    assert all(P.same_bits(a, b) for a, b in zip(l0, l1)) and all(P.same_bits(a, b) for a, b in zip(p0, p1))
    assert all(P.same_bits(a, b) for a, b in zip(t0, t1))
    assert not P.same_bits(p0[1], build(name)[1].lstm_breath_block.weight_hh_l0)         # the steps did move the weights


@pytest.mark.parametrize('cls_name,data', [('LSTMOnlyModel', 'test_dataset.npz'), ('LSTMOnlyWithPackingModel', 'test_dataset_masked.pkl')])
def test_driver_classes_train_and_test(cls_name, data):
    """2 folds, 1 epoch on the ingested fixture: finite losses, a vote for every test window, no base network built."""
    from deepards_amd import train_ards_detector as T
    import deepards_amd.models as M
    cls = getattr(T, cls_name)(T.make_args(train_from_pickle=os.path.join(GOLD, data), kfolds=2, epochs=1, batch_size=4, seed=3,
                                           base_network='no_such_network', cuda=False, cuda_no_dp=True))
    res = cls.train_and_test()
    assert type(cls.model) is (M.LSTMOnlyNetwork if cls_name == 'LSTMOnlyModel' else M.LSTMOnlyWithPacking)
    assert not hasattr(cls.model, 'breath_block')
    for fold in (0, 1):
        assert len(res.get_meter('loss', fold)) > 0
        assert np.isfinite(res.get_meter('loss', fold)).all() and np.isfinite(res.get_meter('test_loss', fold)).all()
        assert np.isfinite(res.patient_results[(fold, 1)]['mean_loss']) and res.patient_results[(fold, 1)]['votes'].sum() > 0
