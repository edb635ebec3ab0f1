"""CPU tests of the per-breath losses' oracle (tests/tools/loss_ref.py against the goldens captured from the reference's
deepards/loss.py, tests/tools/make_golden_losses.py) and of the driver plumbing that selects them: the -loss / --valpha /
--conf-beta / -lc flags, ``network_map['cnn_lstm']`` and the refusals that must come before any launch."""
import glob
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'tools'))
import loss_ref  # noqa: E402

LOSS_GOLD = sorted(glob.glob(os.path.join(ROOT, 'tests', 'golden', 'loss_*.npz')))


def _gold(path):
    z = np.load(path, allow_pickle=False)
    return {k: z[k] for k in z.files}


def _oracle(g):
    if str(g['kind']) == 'vacillating':
        return loss_ref.vacillating(g['logits'], g['target'], float(g['alpha']))
    return loss_ref.confidence(g['logits'], g['target'], float(g['beta']))


def test_the_issue_s_golden_cases_are_all_there():
    names = {os.path.basename(p)[5:-4] for p in LOSS_GOLD}
    want = {'vac_a%s_%s' % (a, s) for a in ('inf', '2', '0p5') for s in ('4x20', '1x20')} | \
           {'conf_b%s_%s' % (b, s) for b in ('1', '0p25') for s in ('4x20', '8')} | \
           {'vac_ainf_4x20_decided', 'conf_b1_4x20_decided'}
    assert names == want
    for p in LOSS_GOLD:
        g = _gold(p)
        assert os.path.getsize(p) < 16384 and all(v.dtype.kind in 'fU' for v in g.values()), p
        assert g['logits'].dtype == np.float32 and g['grad64'].dtype == np.float64 and g['grad32'].dtype == np.float32
        if str(g['kind']) == 'vacillating':                      # the condition on the vacillating inputs
            xm = loss_ref.class_means(g['logits'])
            assert np.abs(xm - 0.5).min() >= 1e-3
            assert g['logits'].ndim == 3
        if p.endswith('_decided.npz'):
            assert loss_ref.class_means(g['logits']).max() > 0.99


@pytest.mark.parametrize('path', LOSS_GOLD, ids=[os.path.basename(p)[:-4] for p in LOSS_GOLD])
def test_oracle_matches_the_reference_capture(path):
    """1e-10 on the loss and on every gradient element: the bound tests/test_oracle_golden.py holds np_ref to."""
    g = _gold(path)
    loss, grad = _oracle(g)
    assert grad.shape == g['grad64'].shape
    assert abs(loss - float(g['loss64'])) <= 1e-10
    assert np.abs(grad - g['grad64']).max() <= 1e-10


@pytest.mark.parametrize('path', LOSS_GOLD, ids=[os.path.basename(p)[:-4] for p in LOSS_GOLD])
def test_oracle_gradient_matches_central_differences(path):
    """Central differences with step 1e-6 in float64: truncation ~1e-12 |f'''|, rounding ~1e-16 / 1e-6 = 1e-10 of the loss;
    1e-7 relative to the largest gradient element (plus 1e-9 absolute) leaves two orders of room over both."""
    g = _gold(path)
    if str(g['kind']) == 'vacillating':
        fn = lambda x: loss_ref.vacillating(x, g['target'], float(g['alpha']))[0]
    else:
        fn = lambda x: loss_ref.confidence(x, g['target'], float(g['beta']))[0]
    _, grad = _oracle(g)
    fd = loss_ref.finite_difference(fn, g['logits'])
    assert np.abs(fd - grad).max() <= 1e-7 * np.abs(grad).max() + 1e-9


def test_oracle_alpha_inf_and_the_left_branch_at_one_half():
    x = np.zeros((1, 4, 2))
    x[0, :, 1] = [1.0, -1.0, 2.0, -2.0]                           # class means exactly 0.5 / 0.5
    loss, grad = loss_ref.vacillating(x, np.array([[0.0, 1.0]]), 2.0)
    bce, _ = loss_ref.bce_mean(x, np.array([[0.0, 1.0]]))
    assert abs(loss - bce - 2.0) < 1e-12                          # both classes on the left branch: -log(e^-alpha) = alpha
    g = _gold(os.path.join(ROOT, 'tests', 'golden', 'loss_vac_ainf_4x20.npz'))
    loss, grad = loss_ref.vacillating(g['logits'], g['target'], np.inf)
    assert np.isfinite(loss) and np.isfinite(grad).all()


# ---- parser / configuration / refusals ----------------------------------------------------------------------------------
def _parse(argv):
    from deepards_amd import train_ards_detector as T
    from deepards_amd.config import Configuration
    return Configuration(T.build_parser().parse_args(argv), T.BUILD_DEFAULTS)


def test_loss_flags_parse_with_the_reference_defaults():
    from deepards_amd import train_ards_detector as T
    a = _parse([])
    assert (a.loss_func, a.valpha, a.conf_beta, a.loss_calc) == ('bce', float('inf'), 1.0, 'all_breaths')
    b = _parse(['-loss', 'vacillating', '--valpha', '2.0', '-lc', 'last_breath', '-n', 'cnn_lstm',
                '--time-series-hidden-units', '32'])
    assert (b.loss_func, b.valpha, b.loss_calc, b.network, b.time_series_hidden_units) == \
        ('vacillating', 2.0, 'last_breath', 'cnn_lstm', 32)
    c = _parse(['-loss', 'confidence', '--conf-beta', '0.25', '--loss-calc', 'all_breaths'])
    assert (c.loss_func, c.conf_beta, c.loss_calc) == ('confidence', 0.25, 'all_breaths')
    with pytest.raises(SystemExit):
        T.build_parser().parse_args(['-loss', 'focal'])
    with pytest.raises(SystemExit):
        T.build_parser().parse_args(['-lc', 'first_breath'])
    for flag in ('--valpha', '--conf-beta', '-lc', '--loss-calc'):
        assert flag not in T.OUT_OF_SCOPE_FLAGS
    m = T.make_args()
    assert (m.loss_func, m.valpha, m.conf_beta, m.loss_calc) == ('bce', float('inf'), 1.0, 'all_breaths')


def test_network_map_has_cnn_lstm_first_like_the_reference():
    from deepards_amd import train_ards_detector as T
    assert T.network_map['cnn_lstm'] is T.CNNLSTMModel and next(iter(T.network_map)) == 'cnn_lstm'
    assert T.CNNLSTMModel.clip_odd_batches is True
    assert T.CNNLSTMModel.__mro__[1:4] == (T.PerBreathClassifierMixin, T.BaseTraining, T.PatientClassifierMixin)


def test_vacillating_on_window_level_outputs_is_refused_before_any_launch():
    """-loss vacillating -n cnn_linear: a ValueError that names the reason, at construction (no device is touched: this
    runs without a GPU)."""
    from deepards_amd import train_ards_detector as T
    for net in ('cnn_linear', 'cnn_linear_to_mean', 'cnn_double_linear'):
        with pytest.raises(ValueError, match=r'per-breath outputs \(B, NB, 2\).*class axis'):
            T.main(['-loss', 'vacillating', '-n', net, '--cuda-no-dp'])
    with pytest.raises(ValueError, match='per-breath outputs'):   # the last breath alone is a window-level output
        T.main(['-loss', 'vacillating', '-n', 'cnn_lstm', '-lc', 'last_breath', '--cuda-no-dp'])
    from deepards_amd.train import check_loss_choice
    check_loss_choice('vacillating', True)
    check_loss_choice('confidence', False)
    with pytest.raises(ValueError, match='loss must be one of'):
        check_loss_choice('focal', True)


def test_cnn_lstm_on_a_resnet_base_is_refused():
    from deepards_amd import train_ards_detector as T
    with pytest.raises(NotImplementedError, match=r'model\.eval\(\).*running statistics'):
        T.main(['-n', 'cnn_lstm', '--base-network', 'resnet18', '--cuda-no-dp'])


def test_bm_to_linear_is_still_refused():
    from deepards_amd import train_ards_detector as T
    assert '--bm-to-linear' in T.OUT_OF_SCOPE_FLAGS
    with pytest.raises(SystemExit, match='outside the accelerated'):
        T.main(['-n', 'cnn_lstm', '--bm-to-linear'])
    with pytest.raises(SystemExit, match='outside the accelerated'):
        T.main(['--fl-gamma', '2'])                                # focal loss stays out of scope


def test_carry_flags_follow_the_patient():
    """0 at the epoch's first window and wherever the patient changes, 1 where the state is carried on."""
    import torch
    from deepards_amd.train import carry_flags
    slots = np.array([0, 1, 2, 2, 3, 3, 4, 5, 5, 6])
    f = carry_flags(slots, np.arange(10), torch.device('cpu'))
    assert f.dtype == torch.int64 and f.tolist() == [0, 0, 0, 1, 0, 1, 0, 0, 1, 0]
    f = carry_flags(slots, np.array([3, 2, 5, 4, 9]), torch.device('cpu'))
    assert f.tolist() == [0, 1, 0, 1, 0]
