"""CPU tests of the Grad-CAM explainers (deepards_amd/gradcam.py, csrc/gradcam.hip): the numpy oracle the GPU tests compare
against (tests/tools/gradcam_ref.py) is itself pinned -- to the committed golden of the reference's hook-and-backward run and
to a real register_hook + backward in stock torch --, then the host helpers, the refusals, the bindings and the command line."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'tools'))
import gradcam_ref as G                                      # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), 'golden', 'gradcam_densenet18.npz')


def test_closed_form_gradient_is_the_goldens_hooked_gradient():
    """The guided gradient the reference modules delivered through register_hook + backward (oracle/make_golden_gradcam.py,
    float64) is the closed form, exactly; the head's logits agree to 1e-12."""
    from oracle.weights import seeded_params
    g = np.load(GOLD, allow_pickle=False)
    sd = seeded_params('densenet18', int(g['seed']))
    W, b = sd['linear_final.weight'].astype(np.float64), sd['linear_final.bias'].astype(np.float64)
    out, _ = G.head_forward(g['conv64'], W, b)
    assert np.abs(out - g['out64']).max() < 1e-12
    t = int(np.argmax(out))
    assert t == int(g['target64'])
    assert np.array_equal(G.closed_form_gradient(g['conv64'], W, t), g['grad64'])


@pytest.mark.parametrize('target', [None, 0, 1])
def test_oracle_equals_a_hooked_backward_on_a_small_net(target):
    """A small random net from stock CPU torch ops, float64: features -> hook -> relu -> AvgPool1d -> view(-1) -> Linear, the
    one-hot score backpropagated as gradcam.py:80-107 does; the reference's numpy loops on those arrays == the oracle."""
    torch.manual_seed(3)
    nb, c, lm = 4, 6, 7
    feats = torch.nn.Sequential(torch.nn.Conv1d(1, c, 5, stride=4, padding=2), torch.nn.BatchNorm1d(c)).double()
    lin = torch.nn.Linear(nb * c, 2).double()
    x = torch.randn(nb, 1, 4 * lm, dtype=torch.float64)
    grads = {}
    conv = feats(x)
    conv.register_hook(lambda gr: grads.__setitem__('g', gr))
    out = lin(torch.nn.AvgPool1d(lm, stride=1)(torch.relu(conv)).view(-1)).unsqueeze(0)
    t = int(np.argmax(out.detach().numpy())) if target is None else target
    one_hot = torch.zeros((1, 2), dtype=torch.float64)
    one_hot[0, t] = 1
    torch.sum(one_hot * out).backward()
    conv_np, grad = conv.detach().numpy(), grads['g'].numpy()
    assert conv_np.shape == (nb, c, lm)
    W, b = lin.weight.detach().numpy(), lin.bias.detach().numpy()
    ref = G.window(conv_np, W, b, -1 if target is None else target)
    assert ref['target'] == t
    assert np.abs(ref['logits'] - out.detach().numpy()[0]).max() < 1e-13
    assert np.abs(G.closed_form_gradient(conv_np, W, t) - grad).max() < 1e-15
    # the reference's loops on the hooked gradient
    weights = np.mean(grad, axis=(0, 2))
    cm = np.mean(conv_np, axis=0)
    cam = np.zeros(lm)
    for i, w in enumerate(weights):
        cam += w * cm[i, :]
    assert np.abs(cam - ref['A'][t]).max() < 1e-14
    assert np.array_equal(np.maximum(0, ref['A'][t]), ref['cam'])
    wr = np.mean(grad, axis=2)
    for i in range(nb):
        row = np.zeros(lm)
        for j in range(c):
            row += wr[i, j] * conv_np[i, j, :]
        assert np.abs(row - ref['R'][t][i]).max() < 1e-14
    assert (ref['S_A'] >= np.abs(ref['A']) - 1e-15).all() and (ref['S_R'] >= np.abs(ref['R']) - 1e-15).all()


def test_normalisations_of_the_oracle():
    by, y, deg = G.maxmin_normalize(np.array([-1.0, 0.5, 2.0, 1.0]))
    assert by.tolist() == [0, 63, 255, 127] and not deg and by.dtype == np.uint8
    by, y, deg = G.maxmin_normalize(np.array([-1.0, -0.5]))
    assert by.tolist() == [0, 0] and deg
    by, y = G.frac_normalize(np.array([1.0, -1.0, 3.0, 0.0]), np.array([1.0, 2.0, -1.0, -2.0]))
    assert by.tolist() == [127, 0, 255, 0]
    assert G.window(np.zeros((2, 3, 7)), np.zeros((2, 6)), np.array([0.3, 0.3]))['target'] == 0        # a tie gives 0


@pytest.mark.parametrize('name', sorted(G.CASES))
def test_excused_share_of_the_kernel_cases(name):
    """The share of uint8 entries of a kernel-level case that the rule excuses from equality (the oracle's pre-truncation value
    within d of an integer) is at most 5 %: the oracle alone shows it, no GPU needed.  Every planted hard input is there."""
    case = G.make_case(name)
    refs = G.batch(case['fmap'], case['W'], case['bias'], case['targets'], case['nb'])
    n, m = G.excused_share(refs)
    print('%s: %d of %d uint8 entries excused from equality = %.2f %%' % (name, n, m, 100.0 * n / m))
    assert n <= 0.05 * m
    for ref in refs:                                         # no row is too flat for the rule to say anything about it
        assert all(np.isfinite(d).all() for y, d in G.byte_slacks(ref).values())
    plant = G.CASES[name]['plant']
    if 'negative_row' in plant:
        row = case['nb'] // 2
        assert refs[-1]['read_degenerate'][row] and not refs[-1]['read_maxmin'][row].any()
        assert (refs[-1]['R'][:, row] == 0).all()
    if 'negative_class' in plant:
        assert refs[0]['target'] == 1 and (refs[0]['A'][1] < 0).all() and refs[0]['cam_degenerate']
        assert not refs[0]['cam'].any() and not refs[0]['cam_maxmin'].any()
    if 'zeros' in plant:
        assert (case['fmap'] == 0).sum() > 30 and np.signbit(case['fmap'][case['fmap'] == 0]).any()
    for ref in refs:                                         # the arg-max / arg-min rule holds in the oracle itself
        for by, y, deg in [(ref['cam_maxmin'], ref['cam_y'], ref['cam_degenerate'])] + \
                [(ref['read_maxmin'][i], ref['read_y'][i], ref['read_degenerate'][i]) for i in range(case['nb'])]:
            if not deg:
                assert ((by == 255) == (y == y.max())).all() and ((by == 0) >= (y == y.min())).all()


def test_resize_cam_is_half_pixel_linear_interpolation():
    from deepards_amd.gradcam import resize_cam
    cam = np.array([0, 255, 48, 157, 0, 3, 91], dtype=np.uint8)
    got = resize_cam(cam)
    assert got.shape == (224, 1) and got.dtype == np.float64
    # the rule restated per output sample with scalars
    want = np.zeros(224)
    for i in range(224):
        s = min(max((i + 0.5) * 7.0 / 224.0 - 0.5, 0.0), 6.0)
        j = min(int(np.floor(s)), 5)
        want[i] = float(cam[j]) + (s - j) * (float(cam[j + 1]) - float(cam[j]))
    assert np.abs(got[:, 0] - want).max() < 1e-11
    assert (got[:16] == 0).all() and (got[-16:] == 91).all()                        # clamped edges: half a source pixel
    assert got[16 + 32 - 1, 0] > 247 and got[:, 0].max() <= 255
    assert np.array_equal(resize_cam(np.full(7, 3.5)), np.full((224, 1), 3.5))      # a constant stays one
    ramp = resize_cam(np.arange(7.0))                                               # a ramp stays a ramp between the centres
    inner = np.arange(16, 208)
    assert np.abs(ramp[inner, 0] - ((inner + 0.5) / 32.0 - 0.5)).max() < 1e-12
    assert np.array_equal(resize_cam(np.arange(7.0), 7)[:, 0], np.arange(7.0))
    assert resize_cam(np.array([2.0]), 5).tolist() == [[2.0]] * 5
    with pytest.raises(ValueError):
        resize_cam(np.zeros((20, 7)))


def test_refusals_before_any_launch():
    import deepards_amd.models as M
    from deepards_amd import gradcam as GC
    for bb in (M.resnet18(), M.vgg11_bn(), M.se_resnet18()):
        with pytest.raises(NotImplementedError, match='features|7-position'):
            GC.GradCam(M.CNNLinearNetwork(bb, 20, 0))
    with pytest.raises(NotImplementedError, match='CNNLinearNetwork'):
        GC.MaxMinNormCam(M.CNNSingleBreathLinearNetwork(M.densenet18()))
    with pytest.raises(NotImplementedError, match='NB \\* C'):
        GC.GradCam(M.CNNLinearNetwork(M.densenet18(), 20, 9))
    model = M.CNNLinearNetwork(M.densenet18(), 20, 0)
    assert GC.check_model(model) == (20, 128)
    with pytest.raises(NotImplementedError, match='both'):
        GC.PatientCams(model, None, 'both')
    with pytest.raises(ValueError):
        GC.PatientCams(model, None, 'neither')
    with pytest.raises(NotImplementedError, match='Havent done this yet'):
        GC.FracTotalNormCam(model).generate_cam(torch.zeros(20, 1, 224), 1)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        GC.UnNormalizedCam(model).generate_cam(torch.zeros(20, 1, 224))
    assert not hasattr(GC.MaxMinNormCam, 'grads') and not hasattr(GC.MaxMinNormCam, 'preds')


def test_bindings_header_and_wrapper_shape_rule():
    from deepards_amd import _lib, gradcam_ops
    names = [n for n in _lib.SIGNATURES if n.startswith('da_gradcam')]
    assert sorted(names) == ['da_gradcam', 'da_gradcam_shape_ok', 'da_gradcam_workspace']
    assert set(names) <= set(_lib.header_symbols()) and 'gradcam.hip' in _lib.SOURCES
    L = _lib.lib()
    for nb, lm, c in ((20, 7, 128), (1, 1, 32), (1024, 8, 1920), (20, 7, 1664), (20, 7, 96), (0, 7, 128), (1025, 7, 128),
                      (20, 9, 128), (20, 0, 128), (20, 7, 1952), (20, 7, 0), (20, 7, 100), (20, 7, 16)):
        assert bool(L.da_gradcam_shape_ok(nb, lm, c)) == gradcam_ops.gradcam_shape_ok(nb, lm, c), (nb, lm, c)
    assert L.da_gradcam_shape_ok(20, 7, 1664) and not L.da_gradcam_shape_ok(20, 9, 128)
    # one record per (window, 64-channel slice): (NB + 1) * 16 + 4 floats
    assert L.da_gradcam_workspace(64, 20, 1920) == 64 * 30 * (21 * 16 + 4) * 4
    assert L.da_gradcam_workspace(1, 1, 96) == 2 * (2 * 16 + 4) * 4
    # refused with the library's error code before any launch (no device is touched)
    assert L.da_gradcam(*([None] * 4), 1, 20, 9, 128, *([None] * 12)) == -1
    assert L.da_gradcam(*([None] * 4), 0, 20, 7, 128, *([None] * 12)) == -1
    assert L.da_gradcam(*([None] * 4), 2 ** 20, 1024, 8, 1920, *([None] * 12)) == -1


def test_command_line_parses():
    from deepards_amd import gradcam as GC
    p = GC.build_parser()
    a = p.parse_args(['model.pth', '-pdp', 'data.npz', '--fold', '2', '--ops', 'averages', '-o', 'out.npz'])
    assert (a.model_path, a.pickled_data_path, a.fold, a.ops, a.target, a.output, a.only_patient, a.batch_size) == \
        ('model.pth', 'data.npz', 2, 'averages', 'ground_truth', 'out.npz', None, 64)
    a = p.parse_args(['m.pth', '--pickled-data-path', 'd.pkl', '--fold', '0', '--ops', 'read_cam', '--target', 'ards',
                      '--only-patient', '0015RPI0320150401', '--output', 'o.npz', '--base-network', 'densenet121'])
    assert (a.ops, a.target, a.only_patient, a.base_network) == ('read_cam', 'ards', '0015RPI0320150401', 'densenet121')
    assert not a.batched_forward and p.parse_args(['m', '-pdp', 'd', '--fold', '0', '--ops', 'averages', '-o', 'o', '--batched-forward']).batched_forward
    for bad in (['m.pth', '--fold', '0', '--ops', 'averages', '-o', 'o.npz'],                       # no dataset
                ['m.pth', '-pdp', 'd.pkl', '--fold', '0', '--ops', 'medians', '-o', 'o.npz'],      # an op that is not built
                ['m.pth', '-pdp', 'd.pkl', '--ops', 'averages', '-o', 'o.npz']):                   # no fold
        with pytest.raises(SystemExit):
            p.parse_args(bad)
