"""The oracle's small-op helpers (oracle/np_ref.py: sliding pool in ``view`` order, head chain, vote table, float64
gather-normalise) pinned against CPU torch in double.  tests/test_head_data_ops_gpu.py judges the HIP kernels by these
helpers, so they must themselves agree with the torch ops the reference runs.  Bound: 1e-12 (both sides are float64)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import np_ref

TOL = 1e-12


def _err(got, ref):
    return float(np.abs(np.asarray(got, dtype=np.float64) - np.asarray(ref, dtype=np.float64)).max())


@pytest.mark.parametrize('rows,lin,k,c', [(5, 7, 7, 8), (3, 8, 7, 4), (2, 16, 7, 12), (1, 14, 7, 16), (2, 9, 2, 4)])
def test_sliding_pool_in_view_order_and_its_backward(rows, lin, k, c):
    rng = np.random.default_rng(11)
    x = rng.standard_normal((rows, c, lin))
    xt = torch.from_numpy(x).requires_grad_(True)
    ft = F.avg_pool1d(xt, k, 1).flatten(1)
    feat = np_ref.avgpool_slide_fwd(x, k)
    assert feat.shape == tuple(ft.shape)
    assert _err(feat, ft.detach().numpy()) <= TOL
    # the helper the GPU test names as the forward reference gives the same features
    assert _err(np_ref.avgpool_fwd(x, k, 1).reshape(rows, -1), feat) <= TOL
    d = rng.standard_normal(feat.shape)
    ft.backward(torch.from_numpy(d))
    assert _err(np_ref.avgpool_slide_bwd(d, k, lin, c), xt.grad.numpy()) <= TOL


@pytest.mark.parametrize('b,r,l,f,bias_mag', [(3, 7, 5, 36, 0.1), (2, 3, 16, 32, 0.1), (5, 2, 3, 8, 30.0), (1, 20, 7, 64, 0.1)])
def test_head_chain_and_its_backward(b, r, l, f, bias_mag):
    rng = np.random.default_rng(12)
    x = rng.standard_normal((b * r, f, l))
    w = rng.standard_normal((2, r * f)) / np.sqrt(r * f)
    bias = np.array([bias_mag, -bias_mag])
    target = np.eye(2)[rng.integers(0, 2, b)]
    for gscale in (1.0, 0.5):
        ref = np_ref.head_chain(x, w, bias, target, r, gscale=gscale)
        xt, wt, bt = (torch.from_numpy(a).requires_grad_(True) for a in (x, w, bias))
        flat = xt.mean(dim=2).reshape(b, r * f)
        logits = F.linear(flat, wt, bt)
        loss = torch.nn.BCEWithLogitsLoss()(logits, torch.from_numpy(target))
        (loss * gscale).backward()
        assert _err(ref['flat'], flat.detach().numpy()) <= TOL
        assert _err(ref['logits'], logits.detach().numpy()) <= TOL
        assert abs(ref['loss'] - loss.item()) <= TOL                       # gscale never touches the loss
        assert _err(ref['dx'], xt.grad.numpy()) <= TOL
        assert _err(ref['dw'], wt.grad.numpy()) <= TOL
        assert _err(ref['dbias'], bt.grad.numpy()) <= TOL


def test_vote_table():
    rng = np.random.default_rng(13)
    n_groups = 3
    logits = rng.standard_normal((500, 2))
    logits[::7, 1] = logits[::7, 0]                                          # exact ties -> class 0
    logits[0], logits[1], logits[2] = (0.0, -0.0), (-0.0, 0.0), (0.0, 0.0)
    group = rng.integers(0, n_groups, 500)
    pred, votes = np_ref.vote_table(logits, group, n_groups)
    tp = torch.argmax(torch.from_numpy(logits), dim=1)
    assert np.array_equal(pred, tp.numpy())
    assert pred[::7].sum() == 0 and pred[:3].sum() == 0
    tv = torch.bincount(torch.from_numpy(group) * 2 + tp, minlength=2 * n_groups).reshape(n_groups, 2)
    assert np.array_equal(votes, tv.numpy())
    # a second batch adds onto the table; group ids outside [0, n_groups) add nothing
    g2 = group.copy()
    g2[:50] = -1
    g2[50:100] = n_groups
    _, votes2 = np_ref.vote_table(logits, g2, n_groups, votes=votes)
    keep = torch.from_numpy(g2[100:]) * 2 + tp[100:]
    assert np.array_equal(votes2, (tv + torch.bincount(keep, minlength=2 * n_groups).reshape(n_groups, 2)).numpy())
    assert votes.sum() == 500                                                # the table handed in is not modified


def test_gather_normalize_in_float64():
    rng = np.random.default_rng(14)
    tiles = rng.standard_normal((6, 3, 37)) * 40.0
    idx = np.array([5, 0, 0, 3, 5, 1, 2, 4])
    out = np_ref.gather_normalize(tiles, idx, -3.7, 23.4)
    ref = ((torch.from_numpy(tiles)[torch.from_numpy(idx)] - (-3.7)) / 23.4).float()
    assert out.dtype == np.float32 and np.array_equal(out, ref.numpy())
    t4 = rng.standard_normal((6, 3, 4, 37)) * 40.0
    mu, std = [-3.7, 0.5, 12.0, -0.25], [23.4, 7.0, 0.3, 110.0]
    out4 = np_ref.gather_normalize(t4, idx, mu, std)
    m = torch.tensor(mu, dtype=torch.float64).reshape(1, 1, 4, 1)
    s = torch.tensor(std, dtype=torch.float64).reshape(1, 1, 4, 1)
    assert np.array_equal(out4, ((torch.from_numpy(t4)[torch.from_numpy(idx)] - m) / s).float().numpy())
