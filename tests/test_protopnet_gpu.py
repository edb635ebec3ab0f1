"""GPU tests of the 1-D ProtoPNet: the kernels of csrc/protopnet.hip, the autograd Functions, the model, the three-phase
trainer and the push against the float64 restatement of tests/tools/ppnet_ref.py.

Bounds.  The prototype layer's forward is held COMPONENTWISE to the summation bound of D squared differences of exactly
representable inputs: |d - d64| <= (D + 2) 2^-23 d64, and |sim - sim64| <= that bound * (1 - eps) / ((d64 + 1)(d64 + eps))
+ 4 * 2^-23 |sim64|; the arg-min is compared exactly on inputs whose two smallest distances per (row, prototype) differ by more
than twice the bound (asserted where the inputs are made).  Everything with a backward is held to the project's yardstick
(tests/test_vgg_gpu.py): rel-l2 <= min(max(4 err32, 16 2^-23), 1e-4), err32 the golden's (the reference's own float32 run
against its float64 run) where there is one, else the float32 run of ppnet_ref.  Bit-for-bit where the issue says bits."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'tools'))
import ppnet_ref as R                                        # noqa: E402
import poison as P                                           # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), 'golden')
U = 2.0 ** -23
EPS = 1e-4


@pytest.fixture(scope='module')
def PO():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from deepards_amd import protopnet_ops
    return protopnet_ops


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def check(got, ref, err32, tag):
    e, b = R.rel_l2(host(got) if torch.is_tensor(got) else got, ref), R.bound(err32)
    print('%-44s rel-l2 %.3e  bound %.3e' % (tag, e, b))
    assert e <= b, '%s: rel-l2 %.3e over %.3e' % (tag, e, b)


# ---- 1. the prototype layer against float64 ----------------------------------------------------------------------------------
_CASES = {}


def safe_case(rows, l, d, p, seed=0):
    """z (rows, l, d), protos (p, d) float32 (every float32 is exactly representable) whose two smallest distances of every
    (row, prototype) differ by more than twice the summation bound: rows are redrawn until they do.  -> z, protos, d64."""
    key = (rows, l, d, p, seed)
    if key not in _CASES:
        rng = np.random.default_rng([seed, rows, l, d, p])
        protos = rng.random((p, d)).astype(np.float32)
        p64 = protos.astype(np.float64)
        z = np.empty((rows, l, d), np.float32)
        d64 = np.empty((rows, p, l))
        for r in range(rows):
            for _ in range(2000):
                zr = rng.random((l, d)).astype(np.float32)
                dd = ((zr.astype(np.float64)[None] - p64[:, None]) ** 2).sum(2)
                srt = np.sort(dd, axis=1)
                if l == 1 or bool((srt[:, 1] - srt[:, 0] > 2 * (d + 2) * U * srt[:, 1]).all()):
                    break
            else:
                raise AssertionError('no row with the margin in 2000 draws')
            z[r], d64[r] = zr, dd
        _CASES[key] = (z, protos, d64)
    return _CASES[key]


def check_proto_fwd(PO, z, protos, d64, tag):
    d = z.shape[2]
    dist, min_d, arg, sim = PO.proto_fwd(dev(z), dev(protos), want_dist=True)
    dist, min_d, arg, sim = host(dist), host(min_d), host(arg), host(sim)
    bd = (d + 2) * U * d64
    assert (np.abs(dist - d64) <= bd).all(), '%s: dist off by %.3e of the bound' % (tag, (np.abs(dist - d64) / np.maximum(bd, 1e-300)).max())
    m64, a64 = d64.min(axis=2), d64.argmin(axis=2)
    assert np.array_equal(arg, a64), '%s: arg-min differs in %d places' % (tag, int((arg != a64).sum()))
    assert np.array_equal(min_d, np.take_along_axis(dist, arg[..., None].astype(np.int64), 2)[..., 0]), tag
    s64 = np.log((m64 + 1) / (m64 + EPS))
    bs = (d + 2) * U * m64 * (1 - EPS) / ((m64 + 1) * (m64 + EPS)) + 4 * U * np.abs(s64)
    assert (np.abs(sim - s64) <= bs).all(), '%s: sim off by %.3e of the bound' % (tag, (np.abs(sim - s64) / bs).max())
    _, m2, a2, s2 = PO.proto_fwd(dev(z), dev(protos))                 # without the distances: the same bits
    assert np.array_equal(host(m2), min_d) and np.array_equal(host(a2), arg) and np.array_equal(host(s2), sim), tag


@pytest.mark.parametrize('p', [2, 20, 64])
@pytest.mark.parametrize('d', [32, 128, 512])
@pytest.mark.parametrize('l', [1, 7, 16])
def test_prototype_layer_forward_componentwise(PO, l, d, p):
    tile = PO.proto_row_tile(l, p)
    assert 1 <= tile <= 4
    for rows in sorted({1, 3, tile + 1, 41}):
        z, protos, d64 = safe_case(rows, l, d, p)
        check_proto_fwd(PO, z, protos, d64, 'rows %d L %d D %d P %d' % (rows, l, d, p))


def test_prototype_layer_at_the_largest_map_length(PO):
    z, protos, d64 = safe_case(3, 64, 64, 64)                         # L P = 4096: one row a block, 16 distances a thread
    assert PO.proto_row_tile(64, 64) == 1
    check_proto_fwd(PO, z, protos, d64, 'L 64 P 64')


def test_prototype_layer_tie_takes_the_lowest_position(PO):
    rng = np.random.default_rng(5)
    one = rng.random((5, 1, 128)).astype(np.float32)
    z = np.repeat(one, 7, axis=1)                                     # identical z at every l
    protos = rng.random((20, 128)).astype(np.float32)
    dist, min_d, arg, _ = PO.proto_fwd(dev(z), dev(protos), want_dist=True)
    assert int(arg.abs().max()) == 0
    assert bool((dist == dist[:, :, :1]).all()) and bool((min_d == dist[:, :, 0]).all())


def test_pushed_prototype_is_at_distance_zero_exactly(PO):
    z, protos, _ = safe_case(6, 7, 128, 20)
    protos = protos.copy()
    src = [(0, 0), (5, 6), (3, 2)]
    for j, (r, l) in zip((0, 7, 19), src):
        protos[j] = z[r, l]                                           # bitwise a patch
    dist, min_d, arg, sim = (host(t) for t in PO.proto_fwd(dev(z), dev(protos), want_dist=True))
    want = np.float32(np.log(1.0 / EPS))
    for j, (r, l) in zip((0, 7, 19), src):
        assert dist[r, j, l] == 0.0 and min_d[r, j] == 0.0 and arg[r, j] == l
        assert abs(np.float32(sim[r, j]) - want) <= np.spacing(want), (sim[r, j], want)


# ---- 2. prototype backward, bias / activation, the loss ------------------------------------------------------------------------
def proto_bwd_ref(z, protos, g_sim, g_min, dtype):
    zt = torch.from_numpy(z).to(dtype).permute(0, 2, 1).contiguous().requires_grad_(True)          # (rows, D, L)
    pt = torch.from_numpy(protos).to(dtype).unsqueeze(2).requires_grad_(True)
    _, min_d, _, sim = R.prototype_layer(zt, pt)
    s = 0
    if g_sim is not None:
        s = s + (sim * torch.from_numpy(g_sim).to(dtype)).sum()
    if g_min is not None:
        s = s + (min_d * torch.from_numpy(g_min).to(dtype)).sum()
    s.backward()
    return dict(dz=zt.grad.permute(0, 2, 1).numpy().astype(np.float64), dprotos=pt.grad[:, :, 0].numpy().astype(np.float64))


@pytest.mark.parametrize('rows, l, d, p', [(1, 1, 32, 2), (5, 7, 128, 20), (65, 7, 128, 20), (3, 16, 512, 64), (41, 7, 64, 4)])
def test_prototype_layer_backward(PO, rows, l, d, p):
    z, protos, _ = safe_case(rows, l, d, p)
    rng = np.random.default_rng([7, rows, l, d, p])
    g_sim = rng.standard_normal((rows, p)).astype(np.float32)
    g_min = (rng.standard_normal((rows, p)) * 0.1).astype(np.float32)
    zt, pt = dev(z), dev(protos)
    _, min_d, arg, _ = PO.proto_fwd(zt, pt)
    for tag, gs, gm in (('both', g_sim, g_min), ('sim', g_sim, None), ('min', None, g_min)):
        r64, r32 = proto_bwd_ref(z, protos, gs, gm, torch.float64), proto_bwd_ref(z, protos, gs, gm, torch.float32)
        dz, dp = PO.proto_bwd(None if gs is None else dev(gs), None if gm is None else dev(gm), min_d, arg, zt, pt)
        for k, got in (('dz', dz), ('dprotos', dp)):
            check(got, r64[k], R.rel_l2(r32[k], r64[k]), 'proto_bwd %s %s %s' % ((rows, l, d, p), tag, k))
    # accumulate adds to the destination; each half alone gives the same bits as the call for both
    r64, r32 = proto_bwd_ref(z, protos, g_sim, g_min, torch.float64), proto_bwd_ref(z, protos, g_sim, g_min, torch.float32)
    dz, dp = PO.proto_bwd(dev(g_sim), dev(g_min), min_d, arg, zt, pt)
    base = torch.full((p, d), 0.5, device='cuda')
    acc = base.clone()
    PO.proto_bwd(dev(g_sim), dev(g_min), min_d, arg, zt, pt, need_dz=False, dprotos=acc, accumulate=True)
    dz_only, none = PO.proto_bwd(dev(g_sim), dev(g_min), min_d, arg, zt, pt, need_dprotos=False)
    assert none is None and not P.diff_report(dz_only, dz)
    check(acc - base, r64['dprotos'], R.rel_l2(r32['dprotos'], r64['dprotos']) + 4 * U, 'proto_bwd accumulate')


def bias_act_ref(x, b, dy, act, dtype):
    xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
    bt = torch.from_numpy(b).to(dtype).requires_grad_(True)
    y = torch.relu(xt + bt) if act == 0 else torch.sigmoid(xt + bt)
    y.backward(torch.from_numpy(dy).to(dtype))
    return dict(y=y.detach().numpy().astype(np.float64), dx=xt.grad.numpy().astype(np.float64),
                db=bt.grad.numpy().astype(np.float64))


@pytest.mark.parametrize('act', [0, 1])
@pytest.mark.parametrize('m, n', [(1, 4), (7, 32), (130, 128), (287, 512), (65, 160), (3, 1024)])
def test_bias_activation_forward_and_backward(PO, m, n, act):
    rng = np.random.default_rng([m, n, act])
    x = rng.standard_normal((m, n)).astype(np.float32)
    b = (rng.standard_normal((n,)) * 0.5).astype(np.float32)
    dy = rng.standard_normal((m, n)).astype(np.float32)
    r64, r32 = bias_act_ref(x, b, dy, act, torch.float64), bias_act_ref(x, b, dy, act, torch.float32)
    y = PO.bias_act_fwd(dev(x), dev(b), act)
    dx, db = PO.bias_act_bwd(dev(dy), y, act)
    for k, got in (('y', y), ('dx', dx), ('db', db)):
        check(got, r64[k], R.rel_l2(r32[k], r64[k]), 'bias_act %s act %d %s' % ((m, n), act, k))
    if act == 0:
        assert np.array_equal(host(y) > 0, r64['y'] > 0)
    # in place, halves alone, accumulate
    x2 = dev(x)
    assert PO.bias_act_fwd(x2, dev(b), act, out=x2) is x2 and not P.diff_report(x2, y)
    dx2, none = PO.bias_act_bwd(dev(dy), y, act, need_dbias=False)
    none2, db2 = PO.bias_act_bwd(dev(dy), y, act, need_dx=False)
    assert none is None and none2 is None and not P.diff_report(dx2, dx) and not P.diff_report(db2, db)
    acc = torch.full((n,), 2.0, device='cuda')
    PO.bias_act_bwd(dev(dy), y, act, need_dx=False, dbias=acc, accumulate=True)
    assert not P.diff_report(acc, db + 2.0)


def loss_ref(logits, target, min_d, p, nb, cl, sl, dtype, w=None):
    lt = torch.from_numpy(logits).to(dtype).requires_grad_(True)
    mt = torch.from_numpy(min_d).to(dtype).requires_grad_(True)
    wt = None if w is None else torch.from_numpy(w).to(dtype).requires_grad_(True)
    parts = R.calc_loss(lt, torch.from_numpy(target).to(dtype), mt, p, nb, 128.0, cl, sl, l1_weight=wt,
                        l1_identity=None if w is None else R.class_identity(p, nb))
    parts[0].backward()
    out = dict(parts=np.array([float(v.detach()) for v in parts]), dlogits=lt.grad.numpy().astype(np.float64),
               dmin=mt.grad.numpy().astype(np.float64))
    if w is not None:
        out['dw'] = wt.grad.numpy().astype(np.float64)
    return out


LOSS_CASES = {                       # B, NB, P, classes of the windows, a far row, (clust, sep), use_l1
    'b1': (1, 20, 20, None, False, (0.8, 0.2), False), 'b2': (2, 20, 20, None, False, (0.8, 0.2), False),
    'b5_nb3_p4': (5, 3, 4, None, False, (0.8, 0.2), False), 'b17': (17, 20, 20, None, False, (0.8, 0.2), False),
    'one_class': (4, 20, 20, 1, False, (0.8, 0.2), False), 'far_row': (3, 20, 20, None, True, (0.8, 0.2), False),
    'lambda0': (2, 20, 20, None, False, (0.0, 0.0), False), 'use_l1': (2, 20, 20, None, False, (0.8, 0.2), True),
    'p64_nb2': (2, 2, 64, None, False, (0.5, 1.5), False)}


@pytest.mark.parametrize('name', sorted(LOSS_CASES))
def test_ppnet_loss_and_its_gradients(PO, name):
    b, nb, p, cls, far, (cl, sl), l1 = LOSS_CASES[name]
    rng = np.random.default_rng([len(name), b, nb, p])
    logits = (rng.standard_normal((b, 2)) * 2).astype(np.float32)
    labels = rng.integers(0, 2, b) if cls is None else np.full(b, cls)
    if cls is None and b > 1:
        labels[:2] = (0, 1)
    target = np.eye(2, dtype=np.float32)[labels]
    min_d = (rng.random((b, nb * p)) * 40).astype(np.float32)
    if far:
        min_d[1] += 200.0
    w = (rng.standard_normal((2, nb * p))).astype(np.float32) if l1 else None
    r64, r32 = (loss_ref(logits, target, min_d, p, nb, cl, sl, dt, w) for dt in (torch.float64, torch.float32))
    mask = None if w is None else dev((1 - R.class_identity(p, nb).numpy().T).astype(np.float32))
    parts, dlogits, dmin, dw = PO.ppnet_loss(dev(logits), dev(target), dev(min_d), nb, p, 128.0, cl, sl,
                                             l1_weight=None if w is None else dev(w), l1_mask=mask)
    got = host(parts).astype(np.float64)
    for i, part in enumerate(('total', 'cls', 'cluster', 'separation', 'l1')):
        e32 = abs(r32['parts'][i] - r64['parts'][i]) / max(abs(r64['parts'][i]), 1e-300)
        tol = R.bound(e32) * abs(r64['parts'][i])
        print('%-10s %-10s got %.9g ref %.9g tol %.3e' % (name, part, got[i], r64['parts'][i], tol))
        assert abs(got[i] - r64['parts'][i]) <= tol, (name, part, got[i], r64['parts'][i])
    check(dlogits, r64['dlogits'], R.rel_l2(r32['dlogits'], r64['dlogits']), name + ' dlogits')
    if cl or sl:
        check(dmin, r64['dmin'], R.rel_l2(r32['dmin'], r64['dmin']), name + ' dmin_d')
        assert np.array_equal(host(dmin) != 0, r64['dmin'] != 0), 'the maxima\'s gradients sit elsewhere'
    else:
        assert float(dmin.abs().max()) == 0.0
    if far:
        assert float(dmin[1].abs().max()) == 0.0 and float(dmin[0].abs().max()) > 0      # the zero maximum: no gradient
    if l1:
        check(dw, r64['dw'], R.rel_l2(r32['dw'], r64['dw']), name + ' dW of the l1 term')
        assert got[4] > 0
    # without gradients: the same parts; gscale scales the gradients only
    p2, n1, n2, _ = PO.ppnet_loss(dev(logits), dev(target), dev(min_d), nb, p, 128.0, cl, sl, want_grad=False)
    assert n1 is None and n2 is None and (l1 or not P.diff_report(p2, parts))
    p3, dl3, dm3, _ = PO.ppnet_loss(dev(logits), dev(target), dev(min_d), nb, p, 128.0, cl, sl, gscale=0.5)
    assert not P.diff_report(p3, p2) and not P.diff_report(dl3, dlogits * 0.5) and not P.diff_report(dm3, dmin * 0.5)


def test_loss_function_routes_gradients_through_autograd(PO):
    rng = np.random.default_rng(2)
    logits = dev((rng.standard_normal((3, 2))).astype(np.float32)).requires_grad_(True)
    min_d = dev((rng.random((3, 80)) * 30).astype(np.float32)).requires_grad_(True)
    target = dev(np.eye(2, dtype=np.float32)[[0, 1, 1]])
    parts = PO.PPNetLossFunction.apply(logits, min_d, target, 4, 20, 128.0, 0.8, 0.2)
    parts[0].backward()
    _, dl, dm, _ = PO.ppnet_loss(logits.detach(), target, min_d.detach(), 4, 20, 128.0, 0.8, 0.2)
    assert not P.diff_report(logits.grad, dl) and not P.diff_report(min_d.grad, dm)


# ---- 3. the head on the golden ---------------------------------------------------------------------------------------------------
def head_model(hp, nb, backbone='densenet18', average_linear=False, **kw):
    import deepards_amd.models as M
    model = M.construct_PPNet(getattr(M, backbone)(**kw), nb, prototype_shape=tuple(hp['prototype_vectors'].shape),
                              average_linear=average_linear)
    missing = model.load_state_dict({k: torch.from_numpy(v) for k, v in hp.items()}, strict=False)
    assert not missing.unexpected_keys
    return model.cuda()


def run_head(PO, model, hmap, nb, g_logits, g_min):
    """The head Functions on a map (rows, C, L) -> logits, min_distances, the gradients on the map and the head parameters."""
    from deepards_amd import functional as F_
    for q in model.parameters():
        q.grad = None
    h = dev(hmap).permute(0, 2, 1).contiguous().requires_grad_(True)
    z = model._add_on(h)
    sim, min_d = PO.PrototypeLayerFunction.apply(z, model.prototype_vectors)
    b, p = h.shape[0] // nb, model.num_prototypes
    flat = F_.WindowMeanFunction.apply(sim, nb) if model.average_linear else sim.view(b, nb * p)
    logits = PO.LastLayerFunction.apply(flat, model.last_layer.weight)
    min_distances = min_d.view(b, nb * p)
    torch.autograd.backward([logits, min_distances], [dev(g_logits), dev(g_min)])
    out = dict(logits=logits, min_distances=min_distances, dmap=h.grad.permute(0, 2, 1))
    out.update({'grad/' + n: q.grad for n, q in model.named_parameters() if not n.startswith('breath_block.') and q.grad is not None})
    return out


def test_head_on_the_golden(PO):
    z = np.load(os.path.join(GOLD, 'ppnet_head.npz'))
    g = {k: z[k] for k in z.files}
    hp = {k[3:]: v for k, v in g.items() if k.startswith('hp/')}
    model = head_model(hp, int(g['nb']))
    out = run_head(PO, model, g['map'], int(g['nb']), g['g_logits'], g['g_min'])
    names = ['logits', 'min_distances', 'dmap'] + ['grad/' + k for k in hp]
    assert sorted(out) == sorted(names)
    for k in names:
        check(out[k], g[k], float(g['err32/' + k]), 'golden head ' + k)


# ---- 4. the whole model ------------------------------------------------------------------------------------------------------------
def window_batch(b, nb, seed):
    rng = np.random.default_rng([seed, b, nb])
    x = rng.standard_normal((b, nb, 1, 224)).astype(np.float32)
    t = np.eye(2, dtype=np.float32)[np.arange(b) % 2]
    return x, t


def head_params(model):
    return {n: host(q) for n, q in model.state_dict().items() if not n.startswith('breath_block.') and n != 'ones'}


@pytest.mark.parametrize('backbone, nb, average_linear', [('densenet18', 20, False), ('densenet18', 3, False),
                                                          ('densenet18', 20, True), ('densenet121', 2, False)])
def test_whole_model_equals_the_reference_head_on_our_own_map(PO, backbone, nb, average_linear):
    import deepards_amd.models as M
    torch.manual_seed(3)
    model = M.construct_PPNet(getattr(M, backbone)(drop_rate=0.0), nb, average_linear=average_linear).cuda()
    with torch.no_grad():                                                 # biases and a last layer that are not the initial constants
        for q in model.add_on_layers.parameters():
            if q.dim() == 1:
                q.normal_(0, 0.1)
        model.last_layer.weight.add_(torch.randn_like(model.last_layer.weight) * 0.05)
    assert len([m for m in model.add_on_layers if isinstance(m, torch.nn.Conv1d)]) == (6 if backbone == 'densenet121' else 2)
    x, _ = window_batch(2, nb, 1)
    xt = dev(x)
    logits, min_d = model(xt, None)
    assert tuple(logits.shape) == (2, 2) and tuple(min_d.shape) == (2, nb * 20)
    with torch.no_grad():
        hmap = model.breath_block.forward_windows(xt.reshape(2 * nb, 1, 224), nb, pooled=False)      # (rows, 7, C)
    assert hmap.shape[1] == 7
    hm = host(hmap.permute(0, 2, 1))
    hp = head_params(model)
    rng = np.random.default_rng([9, nb])
    g_logits = rng.standard_normal((2, 2)).astype(np.float32)
    g_min = (rng.standard_normal((2, nb * 20)) * 0.1).astype(np.float32)
    r64 = R.head_case(hm, hp, nb, g_logits, g_min, torch.float64, average_linear)
    r32 = R.head_case(hm, hp, nb, g_logits, g_min, torch.float32, average_linear)
    tag = '%s nb %d%s ' % (backbone, nb, ' mean' if average_linear else '')
    for k, got in (('logits', logits), ('min_distances', min_d)):
        check(got, r64[k], R.rel_l2(r32[k], r64[k]), tag + k)
    out = run_head(PO, model, hm, nb, g_logits, g_min)                    # the head's gradients on that map
    for k in ('logits', 'min_distances', 'dmap', 'grad/prototype_vectors', 'grad/last_layer.weight'):
        check(out[k], r64[k], R.rel_l2(r32[k], r64[k]), tag + 'head ' + k)
    assert not P.diff_report(out['logits'], logits) and not P.diff_report(out['min_distances'], min_d)
    # the single-window methods of the reference's surface
    sim0, md0 = model.seq_forward(xt[0])
    assert not P.diff_report(md0.reshape(-1), min_d[0]) and tuple(sim0.shape) == (nb, 20)
    zf = model.conv_features(xt[0])
    dist = model.prototype_distances(xt[0])
    assert tuple(zf.shape) == (nb, 128, 7) and tuple(dist.shape) == (nb, 20, 7)
    assert not P.diff_report(dist.min(dim=2)[0].reshape(-1), min_d[0])
    zs, ds = model.push_forward(xt)
    assert tuple(zs.shape) == (2, nb, 128, 7) and not P.diff_report(ds[0], dist) and not P.diff_report(zs[0], zf)
    assert bool((ds[1] != ds[0]).any())                                   # window 1 from x[1], not x[0] again


def head_only(PO, model, hmap, nb):
    """logits, min_distances of the head on a channels-last map (rows, L, C), no gradients."""
    with torch.no_grad():
        sim, min_d = PO.PrototypeLayerFunction.apply(model._add_on(hmap), model.prototype_vectors)
        b = hmap.shape[0] // nb
        return PO.LastLayerFunction.apply(sim.view(b, -1), model.last_layer.weight), min_d.view(b, -1)


def test_the_head_gives_a_window_the_same_bits_at_any_position(PO):
    """Everything behind the breath block's map -- add-on layers, prototype layer, last layer -- on a FIXED map of 5 windows:
    every window's logits and distances have the bits of that window alone and of the batch in reverse order."""
    import deepards_amd.models as M
    torch.manual_seed(5)
    model = M.construct_PPNet(M.densenet18(), 20).cuda().eval()
    hmap = dev(np.maximum(np.random.default_rng(4).standard_normal((5 * 20, 7, 128)), 0).astype(np.float32))
    logits, min_d = head_only(PO, model, hmap, 20)
    for pos in range(5):
        l1, m1 = head_only(PO, model, hmap[pos * 20:(pos + 1) * 20].contiguous(), 20)
        assert not P.diff_report(l1, logits[pos:pos + 1]) and not P.diff_report(m1, min_d[pos:pos + 1]), pos
    rev = torch.flip(hmap.view(5, 20, 7, 128), dims=(0,)).reshape(100, 7, 128).contiguous()
    l2, m2 = head_only(PO, model, rev, 20)
    assert not P.diff_report(torch.flip(l2, dims=(0,)), logits) and not P.diff_report(torch.flip(m2, dims=(0,)), min_d)


def test_a_window_has_the_same_bits_at_any_position(PO):
    """The issue's statement on the WHOLE model: a window's logits and min_distances have the same bits alone and at any
    position of a batch.  The figures are printed before the assertion.

    PPNet runs its breath block on the per-layer DenseNet Functions (``features.block_kernels = False``) for this: on the
    fused dense-block kernels, whose BatchNorm statistics are merged from records of 64-unit tiles, the distances at the
    positions 1 ... 4 differed from the window alone by 4.3e-7 ... 1.0e-6 relative (measured)."""
    import deepards_amd.models as M
    torch.manual_seed(5)
    model = M.construct_PPNet(M.densenet18(), 20).cuda().eval()
    x, _ = window_batch(5, 20, 2)
    xt = dev(x)
    problems = []
    with torch.no_grad():
        logits, min_d = model(xt, None)
        for pos in range(5):
            l1, m1 = model(xt[pos:pos + 1], None)
            dl = float((l1 - logits[pos:pos + 1]).abs().max())
            dm = float(((m1 - min_d[pos:pos + 1]).abs() / m1.abs()).max())
            print('position %d: logits differ by %.3e absolute, min_distances by %.3e relative' % (pos, dl, dm))
            if P.diff_report(l1, logits[pos:pos + 1]) or P.diff_report(m1, min_d[pos:pos + 1]):
                problems.append(pos)
    assert not problems, 'windows at the positions %s do not have the bits they have alone' % problems


# ---- 5. the trainer --------------------------------------------------------------------------------------------------------------------
def small_trainer(optimizer, phase, use_graph=False, seed=11, nb=3, drop_rate=0.0, **kw):
    import deepards_amd.models as M
    from deepards_amd.protopnet import ProtoPNetTrainer
    torch.manual_seed(seed)
    model = M.construct_PPNet(M.densenet18(drop_rate=drop_rate), nb).cuda()
    return ProtoPNetTrainer(model, optimizer=optimizer, learning_rate=0.05, weight_decay=0.1, phase=phase, use_graph=use_graph, **kw)


def torch_step(p0, grads, groups_wd, optimizer, lr):
    """One step of torch.optim.SGD (no momentum) / Adam in float64 on the exported gradients -> {name: new value}."""
    params = {n: torch.from_numpy(p0[n].astype(np.float64)).requires_grad_(True) for n in grads}
    specs = []
    for names, wd in groups_wd:
        names = [n for n in names if n in params]
        if names:
            specs.append({'params': [params[n] for n in names], 'lr': lr, 'weight_decay': wd})
    opt = torch.optim.SGD(specs, lr=lr) if optimizer == 'sgd' else torch.optim.Adam(specs, lr=lr)
    for n, q in params.items():
        q.grad = torch.from_numpy(grads[n].astype(np.float64))
    opt.step()
    return {n: q.detach().numpy() for n, q in params.items()}


PHASE_PREFIXES = {'warm': ('add_on_layers', 'prototype_vectors'), 'joint': ('breath_block', 'add_on_layers', 'prototype_vectors'),
                  'last_layer': ('last_layer',)}


@pytest.mark.parametrize('optimizer', ['sgd', 'adam'])
@pytest.mark.parametrize('phase', ['warm', 'joint', 'last_layer'])
def test_one_step_of_each_phase_against_torch_optim(PO, phase, optimizer):
    tr = small_trainer(optimizer, phase, use_l1=(phase == 'last_layer'))
    model = tr.model
    x, t = window_batch(2, 3, 4)
    xt, tt = dev(x), dev(t)
    parts, grads = tr.compute_gradients(xt, tt)
    p0 = {n: host(q).copy() for n, q in model.named_parameters()}
    grads = {n: host(g) for n, g in grads.items()}
    assert {n.split('.')[0] for n in grads} == set(PHASE_PREFIXES[phase])
    assert max(float(np.abs(g).max()) for g in grads.values()) > 0.01 * (0 if phase == 'last_layer' else 1), 'nothing a clip at 0.01 would touch'
    loss = tr.train_step(xt, tt)                                          # the same gradients: no dropout, the parameters unchanged
    assert not P.diff_report(tr.last_parts, parts) and not P.diff_report(loss, parts[:1])
    p1 = {n: host(q) for n, q in model.named_parameters()}
    decayed = [n for n in grads if not n.startswith('prototype_vectors')]
    ref = torch_step(p0, grads, ((decayed, 0.1), (['prototype_vectors'], 0.0)), optimizer, 0.05)
    for n in grads:
        upd = np.abs(ref[n] - p0[n])
        # float32 rounding of the update's own arithmetic: a few ulps of the parameter and of the update ...
        tol = 16 * 2.0 ** -24 * (np.abs(p0[n]) + upd) + 1e-30
        if optimizer == 'adam':
            # ... and, for Adam's first step u = lr g' / (|g'| + eps) with g' = g + wd p formed in float32 (error at most
            # 2^-23 (|g| + wd |p|)): du / dg' = lr eps / (|g'| + eps)^2, which only counts where g and wd p cancel to ~eps
            wd = 0.0 if n.startswith('prototype_vectors') else 0.1
            g64, p64 = grads[n].astype(np.float64), p0[n].astype(np.float64)
            tol = tol + 0.05 * 1e-8 / (np.abs(g64 + wd * p64) + 1e-8) ** 2 * 2.0 ** -23 * (np.abs(g64) + wd * np.abs(p64))
        bad = np.abs(p1[n] - ref[n]) > tol
        assert not bad.any(), '%s: %d elements off, worst %.3e of its tolerance' % (n, int(bad.sum()), (np.abs(p1[n] - ref[n]) / tol).max())
        assert float(upd.max()) > 0, n
    if optimizer == 'sgd' and phase != 'last_layer':                      # no decay on the prototypes, nothing clipped: p - lr g
        n = 'prototype_vectors'
        assert float(np.abs(grads[n]).max()) > 0.01
        assert np.abs(p1[n] - (p0[n].astype(np.float64) - 0.05 * grads[n].astype(np.float64))).max() <= 2.0 ** -23 * 2
    for n in p0:                                                          # every other parameter: bitwise unchanged
        if n not in grads:
            assert np.array_equal(p0[n].view(np.int32), p1[n].view(np.int32)), n
    if phase == 'last_layer':
        assert [n for n in grads] == ['last_layer.weight'] and float(parts[4]) > 0
    if phase == 'warm':
        assert not any(n.startswith(('breath_block', 'last_layer')) for n in grads)


def test_captured_steps_replay_the_eager_bits_across_phase_switches(PO):
    a = small_trainer('sgd', 'warm', use_graph=False, drop_rate=0.2)
    b = small_trainer('sgd', 'warm', use_graph=True, drop_rate=0.2)
    b.model.load_state_dict(copy.deepcopy(a.model.state_dict()))
    x, t = window_batch(2, 3, 6)
    xt, tt = dev(x), dev(t)
    for i, phase in enumerate(('warm', 'joint', 'last_layer', 'warm', 'joint')):
        a.set_phase(phase)
        b.set_phase(phase)
        for step in range(3):
            la, lb = a.train_step(xt, tt).clone(), b.train_step(xt, tt).clone()
            assert not P.diff_report(la, lb), (phase, step)
            assert not P.diff_report(a.last_parts, b.last_parts), (phase, step)
            assert not P.diff_report(a.bucket.p, b.bucket.p), (phase, i, step)
    assert sorted(k for k, v in b._graphs_by_phase.items() if v) == ['joint', 'last_layer', 'warm']
    assert len(b._graphs_by_phase['warm']) == 1                           # the switch back replays the graph it captured first
    ta, tb = a.test_step(xt, tt), b.test_step(xt, tt)
    tb2 = b.test_step(xt, tt)                                             # a replay
    for u, v, w in zip(ta, tb, tb2):
        assert not P.diff_report(u, v) and not P.diff_report(v, w)
    assert not P.diff_report(a.last_test_parts, b.last_test_parts) and not a.model.training
    loss, outputs, pred = ta
    assert tuple(loss.shape) == (1,) and tuple(a.last_test_parts.shape) == (5,) and not P.diff_report(loss, a.last_test_parts[:1])
    assert torch.allclose(outputs.sum(dim=1), torch.ones(2, device='cuda'), atol=1e-6) and tuple(pred.shape) == (2,)
    b.release_graphs()


# ---- 6. the push -----------------------------------------------------------------------------------------------------------------------
def push_store(labels, nb, seed):
    from deepards_amd.data import DeviceTileStore
    rng = np.random.default_rng([seed, len(labels), nb])
    windows = rng.standard_normal((len(labels), nb, 1, 224))
    targets = np.eye(2, dtype=np.float32)[np.asarray(labels)]
    return DeviceTileStore.with_derived_scaling(windows, targets)


def test_push_equals_the_numpy_push(PO):
    import deepards_amd.models as M
    from deepards_amd.protopnet import push_prototypes
    torch.manual_seed(21)
    nb, bs = 3, 4
    model = M.construct_PPNet(M.densenet18(), nb).cuda()
    labels = [0, 1, 1, 0, 1, 0]
    store = push_store(labels, nb, 1)
    order = list(range(6))
    # the reference push, batch by batch, with absolute window indices
    st = R.push_state(20, 128)
    idx = store.device_indices(torch.as_tensor(order))
    model.eval()
    batches = []
    for s in range(0, 6, bs):
        x, t = store.batch_from_device(idx[s:s + bs])
        z, dist = model.push_forward(x)
        batches.append((s, x))
        st = R.push_batch(st, host(z), host(dist), host(t).argmax(1), start=s)
    before = model.prototype_vectors.detach().clone()
    out = push_prototypes(model, store, batch_size=bs)
    assert np.array_equal(host(out['source']), st['source'])
    assert np.array_equal(host(out['global_min_proto_dist']), st['min_dist'].astype(np.float32))
    assert np.array_equal(host(out['proto_rf_boxes']), st['rf_boxes'])
    assert not P.diff_report(model.prototype_vectors.detach().cpu()[:, :, 0], torch.from_numpy(st['patches']))
    assert bool((model.prototype_vectors != before).any())
    # afterwards the source window's min_d for that prototype is exactly 0
    src = host(out['source'])
    with torch.no_grad():
        for s, x in batches:
            _, min_d = model(x, None)
            md = host(min_d).reshape(x.shape[0], nb, 20)
            for j in range(20):
                w, n, _ = src[j]
                if s <= w < s + x.shape[0]:
                    assert md[w - s, n, j] == 0.0, (j, src[j], md[w - s, n, j])
    # the same windows again as later batches: equal distances are not strictly smaller, nothing moves
    model.prototype_vectors.data.copy_(before)
    again = push_prototypes(model, store, indices=order + order, batch_size=bs)
    assert np.array_equal(host(again['source']), st['source'])
    assert not P.diff_report(model.prototype_vectors.detach().cpu()[:, :, 0], torch.from_numpy(st['patches']))


def test_push_with_a_class_that_has_no_window(PO):
    import deepards_amd.models as M
    from deepards_amd.protopnet import push_prototypes
    torch.manual_seed(22)
    model = M.construct_PPNet(M.densenet18(), 3).cuda()
    out = push_prototypes(model, push_store([0, 0, 0], 3, 2), batch_size=2)
    src, gmin = host(out['source']), host(out['global_min_proto_dist'])
    assert (src[:10, 0] >= 0).all() and (src[10:] == -1).all() and np.isinf(gmin[10:]).all() and np.isfinite(gmin[:10]).all()
    pv = host(model.prototype_vectors)[:, :, 0]
    assert not pv[10:].any() and pv[:10].any(axis=1).all()                # the reference's zero patch
    assert host(out['proto_rf_boxes'])[10:].tolist() == [[-1, -1, -1, -1]] * 10


def test_driver_runs_the_schedule_on_the_fixture(PO):
    """ProtoPNet1DModel(args).train_and_test() on the fixture dataset, one fold: epoch 1 warm, epoch 2 joint, then the push
    and one last-layer pass; the test epochs under model.eval()."""
    from deepards_amd import train_ards_detector as T
    cls = T.ProtoPNet1DModel(T.make_args(train_from_pickle=os.path.join(GOLD, 'test_dataset.npz'), kfolds=2, only_fold=1, epochs=2,
                                         batch_size=4, seed=3, n_warm_epochs=1, push_start_epoch=2, push_every_n=1, n_push_iters=1,
                                         cuda=False, cuda_no_dp=True))
    res = cls.train_and_test()
    model, tr = cls.model, cls.optimizer
    assert type(model).__name__ == 'PPNet' and model.prototype_shape == (20, 128, 1) and cls.max_dist == 128
    assert tr.phase == 'last_layer' and sorted(k for k, v in tr._graphs_by_phase.items()) == ['joint', 'last_layer', 'warm']
    for name in ('loss', 'cls_loss', 'clst_loss', 'sep_loss', 'l1_loss', 'test_loss'):
        vals = res.get_meter(name, 1)
        assert len(vals) > 0 and np.isfinite(vals).all(), name
    assert np.isfinite(res.patient_results[(1, 2)]['mean_loss']) and not res.get_meter('loss', 0)
    push = cls.last_push
    src, gmin = host(push['source']), host(push['global_min_proto_dist'])
    assert (src[:, 0] >= 0).any() and np.isfinite(gmin[src[:, 0] >= 0]).all()
    # the last-layer pass behind the push moved the last layer only: the prototypes are still the pushed patches
    pv = host(model.prototype_vectors)[:, :, 0]
    assert (pv[src[:, 0] < 0] == 0).all() and pv[src[:, 0] >= 0].any(axis=1).all()


# ---- 7. memory discipline ----------------------------------------------------------------------------------------------------------------
def op_cases(PO):
    def rnd(name, *shape):
        g = torch.Generator().manual_seed(sum(map(ord, name)) + len(shape))
        return torch.rand(*shape, generator=g).cuda()

    def fwd_state(z, protos):
        return PO.proto_fwd(z, protos)

    def build_proto(name, rows, l, d, p):
        def build():
            z, protos = rnd(name + 'z', rows, l, d), rnd(name + 'p', p, d)
            return dict(z=z, protos=protos)
        return build

    def build_proto_bwd(name, rows, l, d, p):
        def build():
            z, protos = rnd(name + 'z', rows, l, d), rnd(name + 'p', p, d)
            _, min_d, arg, _ = PO.proto_fwd(z, protos)
            return dict(z=z, protos=protos, min_d=min_d, arg=arg, dsim=rnd(name + 's', rows, p) - 0.5,
                        dmin=rnd(name + 'm', rows, p) - 0.5, dprotos=torch.zeros(p, d, device='cuda'))
        return build

    def build_ba(name, m, n):
        return lambda: dict(x=rnd(name + 'x', m, n) - 0.5, bias=rnd(name + 'b', n) - 0.5)

    def build_ba_bwd(name, m, n, act):
        def build():
            y = PO.bias_act_fwd(rnd(name + 'x', m, n) - 0.5, rnd(name + 'b', n) - 0.5, act)
            return dict(dy=rnd(name + 'd', m, n) - 0.5, y=y, dbias=torch.zeros(n, device='cuda'))
        return build

    def build_loss(name, b, nb, p):
        def build():
            t = torch.eye(2, device='cuda')[torch.arange(b, device='cuda') % 2].contiguous()
            return dict(logits=rnd(name + 'l', b, 2) - 0.5, target=t, min_d=rnd(name + 'm', b, nb * p) * 40)
        return build

    rows_iso = lambda names, paths: dict(inputs=tuple(names.split()), R=1, axis=paths)
    cases = []
    for name, (rows, l, d, p) in (('proto_fwd_5x7x128x20', (5, 7, 128, 20)), ('proto_fwd_3x16x64x4', (3, 16, 64, 4))):
        cases.append(P.OpCase(name, 'proto_fwd', build_proto(name, rows, l, d, p),
                              lambda z, protos: PO.proto_fwd(z, protos, want_dist=True), rows=rows_iso('z', {})))
    for name, (rows, l, d, p) in (('proto_bwd_5x7x128x20', (5, 7, 128, 20)), ('proto_bwd_66x3x32x6', (66, 3, 32, 6))):
        cases.append(P.OpCase(name, 'proto_bwd', build_proto_bwd(name, rows, l, d, p),
                              lambda z, protos, min_d, arg, dsim, dmin, dprotos: PO.proto_bwd(dsim, dmin, min_d, arg, z, protos, dprotos=dprotos),
                              dests=('dprotos',), rows=rows_iso('z dsim dmin min_d', {'[1]': None})))
    for name, (m, n) in (('bias_act_fwd_70x160', (70, 160)), ('bias_act_fwd_3x32', (3, 32))):
        cases.append(P.OpCase(name, 'bias_act_fwd', build_ba(name, m, n), lambda x, bias: PO.bias_act_fwd(x, bias, PO.SIGMOID),
                              rows=rows_iso('x', {})))
    for name, (m, n, act) in (('bias_act_bwd_70x160', (70, 160, 1)), ('bias_act_bwd_3x32', (3, 32, 0))):
        cases.append(P.OpCase(name, 'bias_act_bwd', build_ba_bwd(name, m, n, act),
                              lambda dy, y, dbias, act=act: PO.bias_act_bwd(dy, y, act, dbias=dbias), dests=('dbias',),
                              rows=rows_iso('dy y', {'[1]': None})))
    for name, (b, nb, p) in (('ppnet_loss_3x20x20', (3, 20, 20)), ('ppnet_loss_18x2x6', (18, 2, 6))):
        cases.append(P.OpCase(name, 'ppnet_loss', build_loss(name, b, nb, p),
                              lambda logits, target, min_d, nb=nb, p=p: PO.ppnet_loss(logits, target, min_d, nb, p, 128.0, 0.8, 0.2)[:3]))
    return cases


def test_memory_discipline_of_every_new_entry(PO):
    """Poisoned allocations, operands inside guard bands, pattern-filled destinations, NaN rows and a repeat behind another
    shape: the same bits as a clean run, no output element left unwritten, every guard intact."""
    cases = op_cases(PO)
    problems = []
    for i, c in enumerate(cases):
        other = cases[i + 1] if i % 2 == 0 else cases[i - 1]             # the other shape of the same family
        assert other.family == c.family
        for check_name in P.CHECKS:
            problems += P.run_check(check_name, c, other)
    assert not problems, '\n'.join(problems)


def test_unsupported_shapes_return_minus_one_and_touch_nothing(PO):
    from deepards_amd import _lib, hip_ops as H
    L = _lib.lib()
    f = lambda *s: P.fill_poison(torch.empty(s, device='cuda'))
    z, protos = torch.rand(4, 7, 128, device='cuda'), torch.rand(20, 128, device='cuda')
    outs = [f(4, 20, 7), f(4, 20), P.fill_poison(torch.empty((4, 20), device='cuda', dtype=torch.int32)), f(4, 20)]
    ptr = lambda ts: [H._p(t) for t in ts]
    for rows, l, d, p in ((0, 7, 128, 20), (4, 0, 128, 20), (4, 65, 128, 20), (4, 7, 48, 20), (4, 7, 544, 20), (4, 7, 16, 20),
                          (4, 7, 128, 1), (4, 7, 128, 65)):
        assert L.da_proto_fwd(H._p(z), H._p(protos), *ptr(outs), rows, l, d, p, H._stream()) == -1, (rows, l, d, p)
        assert L.da_proto_shape_ok(rows, l, d, p) == 0 and not PO.proto_shape_ok(rows, l, d, p)
        dz, dp, ws = f(4, 7, 128), f(20, 128), f(64)
        assert L.da_proto_bwd(H._p(outs[1]), None, H._p(outs[1]), H._p(outs[2]), H._p(z), H._p(protos), H._p(dz), H._p(dp), 0,
                              H._p(ws), rows, l, d, p, H._stream()) == -1
        torch.cuda.synchronize()
        assert all(P.count_poison(t) == t.numel() for t in outs + [dz, dp, ws])
    assert L.da_proto_shape_ok(4, 7, 128, 20) == 1 and L.da_proto_row_tile(7, 20) == 4 and L.da_proto_row_tile(65, 20) == 0
    x, b, y, db, ws = torch.rand(8, 32, device='cuda'), torch.rand(32, device='cuda'), f(8, 32), f(32), f(64)
    for m, n, act in ((0, 32, 0), (8, 6, 0), (8, 0, 0), (8, 32, 2), (8, 4100, 0)):
        assert L.da_bias_act_fwd(H._p(x), H._p(b), H._p(y), m, n, act, H._stream()) == -1, (m, n, act)
        assert L.da_bias_act_bwd(H._p(x), H._p(x), H._p(y), H._p(db), 0, H._p(ws), m, n, act, H._stream()) == -1
    assert L.da_bias_act_bwd(H._p(x), H._p(x), None, None, 0, None, 8, 32, 0, H._stream()) == -1          # nothing asked for
    lg, tg, md = torch.rand(2, 2, device='cuda'), torch.eye(2, device='cuda'), torch.rand(2, 40, device='cuda')
    out, dl, dm = f(5), f(2, 2), f(2, 40)
    for bb, nb, p in ((0, 2, 20), (2, 0, 20), (2, 2, 3), (2, 2, 0), (2, 2, 66)):
        assert L.da_ppnet_loss(H._p(lg), H._p(tg), H._p(md), bb, nb, p, 128.0, 0.8, 0.2, 1.0, H._p(out), H._p(dl), H._p(dm),
                               H._stream()) == -1, (bb, nb, p)
    torch.cuda.synchronize()
    assert all(P.count_poison(t) == t.numel() for t in (y, db, ws, out, dl, dm))
    with pytest.raises(H.HipError, match='unsupported'):
        PO.proto_fwd(torch.rand(2, 7, 48, device='cuda'), torch.rand(4, 48, device='cuda'))
    with pytest.raises(NotImplementedError, match='kernel size 1'):
        PO.proto_fwd(z, torch.rand(20, 128, 3, device='cuda'))
    with pytest.raises(H.HipError, match='unsupported'):
        PO.bias_act_fwd(torch.rand(2, 6, device='cuda'), torch.rand(6, device='cuda'), 0)
    with pytest.raises(ValueError):
        PO.ppnet_loss(lg, tg, md, 2, 21, 128.0, 0.8, 0.2)


def test_last_layer_without_a_bias_and_the_linear_with_one(PO):
    """da_linear2_* with a null bias pointer: x W^T and its gradients; with a bias the entry does what it did."""
    from deepards_amd import hip_ops as H
    rng = np.random.default_rng(8)
    x = rng.standard_normal((5, 60)).astype(np.float32)
    w = rng.standard_normal((2, 60)).astype(np.float32)
    g = rng.standard_normal((5, 2)).astype(np.float32)
    xt, wt = dev(x).requires_grad_(True), dev(w).requires_grad_(True)
    out = PO.LastLayerFunction.apply(xt, wt)
    out.backward(dev(g))
    x64, w64, g64 = (a.astype(np.float64) for a in (x, w, g))
    for got, ref in ((out, x64 @ w64.T), (xt.grad, g64 @ w64), (wt.grad, g64.T @ x64)):
        assert R.rel_l2(host(got), ref) <= 16 * U
    bias = dev(np.array([0.25, -1.5], np.float32))
    with_bias = H.linear2_fwd(dev(x), dev(w), bias)
    assert R.rel_l2(host(with_bias), x64 @ w64.T + np.array([0.25, -1.5])) <= 16 * U
