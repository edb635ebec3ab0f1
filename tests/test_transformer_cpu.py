"""CPU tests of the cnn_transformer head: the numpy oracle against the reference's goldens, state_dict keys, the parser,
refusals before any launch, and the untouched network_map."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'tools'))

from oracle.weights import digest  # noqa: E402
import transformer_ref as R  # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
BLOCK_GOLDENS = ['tfm_block_2x20x128x16.npz', 'tfm_block_2x20x512x16.npz', 'tfm_block_2x5x128x8.npz', 'tfm_masked_2x20x128x16.npz']


def _gold(name):
    z = np.load(os.path.join(GOLD, name), allow_pickle=False)
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize('name', BLOCK_GOLDENS)
def test_oracle_equals_the_reference_classes(name):
    """transformer_ref in float64 against the reference's own fp64 run (Transformer of 2 blocks + Linear + BCE; one case
    with fixed dropout masks, p = 0.2, stored bit-packed): every tensor at 1e-10 (digests where the golden stores those)."""
    g = _gold(name)
    b, t, d, h = [int(v) for v in g['shape']]
    blocks = [[g['param/blocks.%d.%s' % (i, n)].astype(np.float64) for n in R.PARAM_NAMES] for i in range(2)]
    masks = None
    if 'masks_packed' in g:
        m = np.unpackbits(g['masks_packed'])[:4 * b * t * d].reshape(2, 2, b, t, d).astype(bool)
        masks = [[m[i, 0], m[i, 1]] for i in range(2)]
        assert 0.75 < m.mean() < 0.85
    o = R.transformer_loss(g['x'].astype(np.float64), blocks, g['param/linear_final.weight'], g['param/linear_final.bias'],
                           g['target'], masks, float(g['p']))
    ours = {'y': o['y'], 'logits': o['logits'], 'loss': np.asarray(o['loss']), 'dx': o['dx'], 'grad/linear_final.weight': o['dwf'],
            'grad/linear_final.bias': o['dbf']}
    for i in range(2):
        ours['weights%d' % i] = o['weights'][i]
        for n, a in zip(R.PARAM_NAMES, o['grads'][i]):
            ours['grad/blocks.%d.%s' % (i, n)] = a
    for k, a in ours.items():
        if k in g:
            np.testing.assert_allclose(a, g[k], rtol=0, atol=1e-10, err_msg=k)
        else:
            np.testing.assert_allclose(digest(a), g['dig/' + k], rtol=1e-10, atol=1e-10, err_msg=k)
    assert [str(n) for n in g['names'][:16]] == ['blocks.0.' + n for n in R.PARAM_NAMES]


@pytest.mark.parametrize('backbone', ['resnet18', 'densenet18'])
def test_whole_model_oracle_equals_the_reference(backbone):
    """np_ref's breath block with transformer_ref as its head against the reference's fp64 CNNTransformerNetwork run: logits
    and loss at 1e-10, every gradient's digest at the bound test_oracle_golden.py uses for digests."""
    g = _gold('tfm_model_b2_%s.npz' % backbone)
    ref = R.model_reference(g, backbone)
    np.testing.assert_allclose(ref['logits'], g['logits'], rtol=0, atol=1e-10)
    assert abs(float(ref['loss']) - float(g['loss'])) < 1e-10
    keys = [k for k in g if k.startswith('dig/grad/')]
    assert sorted(k[len('dig/grad/'):] for k in keys) == sorted(ref['grads'])
    for k in keys:
        np.testing.assert_allclose(digest(ref['grads'][k[len('dig/grad/'):]]), g[k], rtol=1e-7, atol=1e-10, err_msg=k)


@pytest.mark.parametrize('backbone', ['resnet18', 'densenet18'])
def test_state_dict_keys_and_order_are_the_references(backbone):
    import deepards_amd.models as M
    g = _gold('tfm_model_b2_%s.npz' % backbone)
    bb = M.resnet18() if backbone == 'resnet18' else M.densenet18()
    model = M.CNNTransformerNetwork(bb, 0, False, 16, 2)
    assert list(model.state_dict().keys()) == [str(n) for n in g['names']]
    head = [n for n, _ in model.named_parameters() if not n.startswith('breath_block.')]
    assert head == ['transformer.blocks.%d.%s' % (i, n) for i in range(2) for n in R.PARAM_NAMES] + \
        ['linear_final.weight', 'linear_final.bias']
    blk = model.transformer.blocks[0]
    assert blk.dropout == 0.2 and isinstance(blk.attention_dropout, torch.nn.Dropout) and isinstance(blk.ff[3], torch.nn.Dropout)
    assert isinstance(blk.ff[1], torch.nn.ReLU) and model.seq_size == 224


def test_parser_takes_transformer_blocks():
    from deepards_amd import train_ards_detector as T
    from deepards_amd.config import Configuration
    p = T.build_parser()
    assert p.parse_args(['--transformer-blocks', '3']).transformer_blocks == 3
    assert '--transformer-blocks' not in T.OUT_OF_SCOPE_FLAGS
    assert all(v is None for v in vars(p.parse_args([])).values())
    assert Configuration(p.parse_args([]), T.BUILD_DEFAULTS).transformer_blocks == 2
    assert Configuration(p.parse_args(['--transformer-blocks', '1']), T.BUILD_DEFAULTS).transformer_blocks == 1
    assert T.make_args().transformer_blocks == 2


def test_refusals_come_before_any_launch():
    import deepards_amd.models as M
    from deepards_amd import train_ards_detector as T
    with pytest.raises(NotImplementedError, match='metadata features are outside the accelerated path'):
        M.CNNTransformerNetwork(M.densenet18(), 9, False, 16, 2)
    with pytest.raises(NotImplementedError, match='outside the accelerated path'):
        M.CNNTransformerNetwork(M.densenet18(), 0, True, 16, 2)
    for h in (12, 4, 72):
        with pytest.raises(NotImplementedError, match=r'\(T, D, H\) = \(1, 128, %d\)' % h):
            M.CNNTransformerNetwork(M.densenet18(), 0, False, h, 2)
    with pytest.raises(NotImplementedError, match='--bm-to-linear'):
        T.CNNTransformerModel(T.make_args(bm_to_linear=True))
    with pytest.raises(ValueError, match='vacillating|loss'):
        T.CNNTransformerModel(T.make_args(loss_func='nope'))
    assert T.CNNTransformerModel.per_breath_outputs and not T.CNNTransformerModel.eval_in_test_epoch


def test_network_map_is_untouched():
    from deepards_amd import train_ards_detector as T
    assert sorted(T.network_map) == ['cnn_double_linear', 'cnn_linear', 'cnn_linear_compr_to_rf', 'cnn_linear_to_mean',
                                     'cnn_lstm', 'cnn_single_breath_linear']
    assert T.CNNTransformerModel not in T.network_map.values()


def test_block_form_of_every_accepted_shape_fits_the_lds():
    """da_tfm_block_form (host only: the expressions the launches use) over every accepted (T, D, H): both kernels' dynamic
    LDS stays within the 160 KB a workgroup has, so no accepted shape is refused at launch; the largest need is the
    backward's at (64, 2048, 64); the multi-token form is taken where D <= 512 and T H <= 1024, the one-token form elsewhere;
    and the sizes are the layouts' (csrc/transformer.hip, above each kernel)."""
    from deepards_amd import hip_ops as H
    worst_f, worst_b, multi = (0, None), (0, None), 0
    for t in range(1, 65):
        for d in range(64, 2049, 64):
            for h in range(8, 65, 8):
                tf, tb, lf, lb = H.tfm_block_form(t, d, h)
                assert (tf, tb) == ((5, 3) if d <= 512 and t * h <= 1024 else (1, 1)), (t, d, h)
                assert lf == 4 * (3 * t * h + 4 * tf * d) and lb == 4 * (5 * t * h + 4 * t + 4 * tb * 2 * d), (t, d, h)
                assert lf <= 160 * 1024 and lb <= 160 * 1024, (t, d, h, lf, lb)
                multi += tf > 1
                worst_f, worst_b = max(worst_f, (lf, (t, d, h))), max(worst_b, (lb, (t, d, h)))
    assert worst_b == (148480, (64, 2048, 64)) and worst_f[1] == (64, 2048, 64) and worst_b[0] >= worst_f[0]
    assert 0 < multi < 64 * 32 * 8
    assert H.tfm_block_form(64, 512, 16)[3] == 70656                      # above the 64 KB a kernel gets without the attribute
    for bad in ((0, 128, 16), (65, 128, 16), (20, 96, 16), (20, 2112, 16), (20, 128, 12), (20, 128, 72)):
        with pytest.raises(ValueError):
            H.tfm_block_form(*bad)
