"""CPU tests of the autoencoder's reference side: tests/tools/ae_ref.py against the goldens of the real reference classes, the
decision condition on the golden inputs, teacher forcing, the regression scores, the refusal of an autoencoder checkpoint as a
base network, and the driver maps that must stay as they are."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle.weights import digest                                                   # noqa: E402
from tools import ae_ref as R                                                       # noqa: E402

_MODELS = {}


def _runs(n, l):
    """(golden, its sel bits, ae_ref in float64, ae_ref in float32), computed once per shape."""
    if (n, l) not in _MODELS:
        g, sels = R.load_golden(n, l)
        seed = int(g['seed'][0])
        x, p = R.seeded_rows(n, l, seed), R.seeded_params(seed)
        _MODELS[(n, l)] = (g, sels, R.model(x, p), R.model(x, p, dtype=torch.float32))
    return _MODELS[(n, l)]


@pytest.mark.parametrize('n,l', R.MODEL_SHAPES)
def test_ae_ref_reproduces_the_goldens(n, l):
    g, sels, m64, _ = _runs(n, l)
    assert tuple(g['shape']) == (n, l)
    names = [k[len('err32/'):] for k in g.files if k.startswith('err32/') and k != 'err32/encoded']
    assert len(names) == 2 + 20 + 8                             # output, loss; 20 of 24 parameters; 8 running statistics
    for name in names:
        big = 'dig/' + name in g.files
        ref = g['dig/' + name] if big else g[name]
        mine = digest(m64[name]) if big else m64[name]
        assert R.rel_l2(np.ravel(mine), np.ravel(ref)) < 1e-12, name
    # the four conv biases in front of a BatchNorm: gradient exactly 0, rounding noise in both runs -- a marker, no err32
    zeros = sorted(k[len('exact_zero/'):] for k in g.files if k.startswith('exact_zero/'))
    assert zeros == ['grad/conv_down%d.bias' % k for k in range(1, 5)]
    for name in zeros:
        assert 'err32/' + name not in g.files and name not in g.files and 'dig/' + name not in g.files
        assert float(g['exact_zero/' + name][0]) < 1e-10 and np.abs(m64[name]).max() < 1e-10
    assert R.rel_l2(m64['recon'], g['full/recon']) < 1e-13
    for a, b in zip(sels, m64['sel']):
        assert np.array_equal(a, b)                                         # the reference's indices % 2
    for k, want in ((1, 64), (2, 128), (3, 256), (4, 512)):
        assert tuple(g['selshape/%d' % k]) == (n, want, l >> k)


def test_ae_ref_encoder_reproduces_the_golden():
    g, _, _, _ = _runs(3, 224)
    seed = int(g['seed'][0])
    enc = R.model(R.seeded_rows(3, 224, seed), R.seeded_params(seed), encoder_only=True)['encoded']
    assert enc.shape == (3, 512, 1)
    ref = g['dig/encoded'] if 'dig/encoded' in g.files else g['encoded']
    assert R.rel_l2(np.ravel(digest(enc)), np.ravel(ref)) < 1e-12


@pytest.mark.parametrize('n,l', R.MODEL_SHAPES)
def test_golden_inputs_satisfy_the_decision_condition_in_fp32(n, l):
    """The condition the GPU tests hold the kernels to, on the reference's own fp32 arithmetic: no pool decision differs from
    the float64 run (the golden seeds were picked for that), so a fortiori none differs at a gap of 1e-4 or more."""
    g, _, m64, m32 = _runs(n, l)
    for pairs, differ, gap, near in R.decision_report(m64['sel'], m32['sel'], m64['gap']):
        assert differ == 0 and near <= 0.0005 * pairs
    for k in range(1, 5):
        assert int(g['near/%d' % k][0]) == int((m64['gap'][k - 1] < 1e-4).sum())


def test_teacher_forcing_takes_the_bits_as_given():
    g, sels, m64, _ = _runs(4, 16)
    seed = int(g['seed'][0])
    x, p = R.seeded_rows(4, 16, seed), R.seeded_params(seed)
    same = R.model(x, p, sels=sels)
    assert np.array_equal(same['recon'], m64['recon'])
    flipped = [s.copy() for s in sels]
    flipped[0][0, 0, 0] ^= True
    other = R.model(x, p, sels=flipped)
    assert other['sel'][0][0, 0, 0] == flipped[0][0, 0, 0] and not np.array_equal(other['recon'], m64['recon'])


# ---- the meters ---------------------------------------------------------------------------------------------------------------
def test_regression_scores_match_the_written_out_formulas():
    import deepards_amd.train_ards_detector as T
    r = np.random.RandomState(0)
    t, p = r.standard_normal((7, 5)), r.standard_normal((7, 5))
    t[:, 2] = 1.5                                                           # a constant column that is missed: r2 = 0
    t[:, 3] = -2.0
    p[:, 3] = -2.0                                                          # a constant column that is matched: r2 = 1
    mae, r2, mse = T.regression_scores(t, p)
    want_mae = np.mean([np.mean(np.abs(t[:, j] - p[:, j])) for j in range(5)])
    want_mse = np.mean([np.mean((t[:, j] - p[:, j]) ** 2) for j in range(5)])
    cols = []
    for j in range(5):
        num, den = np.sum((t[:, j] - p[:, j]) ** 2), np.sum((t[:, j] - t[:, j].mean()) ** 2)
        cols.append(1.0 - num / den if den != 0 else (1.0 if num == 0 else 0.0))
    assert abs(mae - want_mae) < 1e-15 and abs(mse - want_mse) < 1e-15 and abs(r2 - np.mean(cols)) < 1e-15
    assert cols[2] == 0.0 and cols[3] == 1.0
    assert T.regression_scores(t[:, 0], t[:, 0]) == (0.0, 1.0, 0.0)
    with pytest.raises(ValueError, match='one shape'):
        T.regression_scores(t, p[:, :4])


# ---- the checkpoint refusal and the driver maps ----------------------------------------------------------------------------
def test_autoencoder_checkpoint_is_refused_as_a_base_network(tmp_path):
    from deepards_amd import checkpoint
    import deepards_amd.train_ards_detector as T
    g, _ = R.load_golden(4, 16)
    keys = [str(k) for k in g['keys']]
    assert len(keys) == 92 and keys[0] == 'base_network.conv_down1.weight' and 'breath_block.0.weight' in keys
    reason = 'not built in this package.*second stage.*the reference cannot run either'
    with pytest.raises(ValueError, match=reason):
        checkpoint._refuse_autoencoder('f.pth', keys=keys)
    with pytest.raises(ValueError, match=reason):
        checkpoint._refuse_autoencoder('f.pth', 'deepards.models.autoencoder_network.AutoencoderNetwork')
    # no other file is taken for one: another class, a classifier's keys, a name that merely contains it, half the key set
    checkpoint._refuse_autoencoder('f.pth', 'CNNLinearNetwork', ['breath_block.conv1.weight'])
    checkpoint._refuse_autoencoder('f.pth', 'mine.DenoisingAutoencoderNetworkV2', ['base_network.conv_down1.weight'])
    checkpoint._refuse_autoencoder('f.pth', 'mine.MyAutoencoderNetwork')
    # a state_dict file with the reference's keys, through the public entry point
    params = R.seeded_params(0)
    sd = {k: torch.tensor(v, dtype=torch.float32) for k, v in R.full_state_dict(params, 'base_network.').items()}
    sd.update({'breath_block.' + k[len('encoder.'):]: torch.tensor(v, dtype=torch.float32)
               for k, v in R.full_state_dict(params).items() if k.startswith('encoder.')})
    path = str(tmp_path / 'ae_state.pth')
    torch.save(sd, path)
    with pytest.raises(ValueError, match=reason):
        checkpoint.load_base_network(path, T.base_networks, {})


def test_driver_maps_are_unchanged():
    import deepards_amd.models as M
    import deepards_amd.train_ards_detector as T
    assert set(T.network_map) == {'cnn_lstm', 'cnn_linear', 'cnn_single_breath_linear', 'cnn_double_linear', 'cnn_linear_to_mean',
                                  'cnn_linear_compr_to_rf'}
    assert T.base_networks is M.base_networks and set(M.base_networks) == set(M.BACKBONES) and len(M.BACKBONES) == 12
    with pytest.raises(SystemExit):
        T.build_parser().parse_args(['-n', 'autoencoder'])
