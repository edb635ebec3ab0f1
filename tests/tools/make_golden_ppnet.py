"""Goldens of the 1-D ProtoPNet from the REAL reference classes (models/protopnet1d/model.py), run where the reference is
checked out ($DEEPARDS_REFERENCE, default: a `reference` directory beside this repository); never imported by a test:

    python tests/tools/make_golden_ppnet.py

Writes tests/golden/ppnet_keys.npz   per base network (densenet18, densenet121): the state_dict keys of construct_PPNet outside
                                     ``breath_block.`` in order, their shapes, ``proto_layer_rf_info``, the repr's tail
       tests/golden/ppnet_head.npz   the head alone at densenet18's shapes: a seeded (2 * 20, 128, 7) map and seeded head
                                     parameters (ppnet_ref.seeded_map / seeded_head) through the reference's own add_on_layers,
                                     _l2_convolution, min-pool, distance_2_similarity and last_layer: logits, min_distances and,
                                     under seeded upstream gradients on both, the gradients on the map and on every head
                                     parameter in float64; ``err32/<name>``: the rel-l2 of the reference's float32 run against
                                     its float64 run -- the yardstick of the GPU tests.
The reference's calc_loss cannot be imported (its module imports packages that are not installed here): the loss is pinned by
ppnet_ref.calc_loss, which tests/test_protopnet_cpu.py holds against a second composition."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.environ.get('DEEPARDS_REFERENCE', os.path.join(os.path.dirname(ROOT), 'reference')))

import ppnet_ref as R                                                                       # noqa: E402
from deepards.models.protopnet1d.model import construct_PPNet                               # noqa: E402
from deepards.models.densenet import densenet18, densenet121                                # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden')
SEED, B, NB = 31, 2, 20


def save(name, rec):
    path = os.path.join(OUT, name)
    np.savez_compressed(path, **rec)
    size = os.path.getsize(path)
    assert size < (1 << 20), (name, size)
    print(name, size)


def keys():
    rec = {}
    for name, fn in (('densenet18', densenet18), ('densenet121', densenet121)):
        m = construct_PPNet(fn(), NB)
        sd = [(k, v) for k, v in m.state_dict().items() if not k.startswith('breath_block.')]
        rec[name + '/names'] = np.array([k for k, _ in sd])
        rec[name + '/shapes'] = np.array(['x'.join(map(str, v.shape)) for _, v in sd])
        rec[name + '/rf_info'] = np.array(m.proto_layer_rf_info, np.float64)
        rec[name + '/last_layer'] = m.last_layer.weight.detach().numpy()
        rec[name + '/identity'] = m.prototype_class_identity.numpy()
        print(name, m.proto_layer_rf_info, len(sd))
    save('ppnet_keys.npz', rec)


def reference_head(h, hp, g_logits, g_min, dtype):
    """The head through the reference's own modules and methods -> {name: float64 array}."""
    m = construct_PPNet(densenet18(), NB)
    missing = m.load_state_dict({k: torch.from_numpy(v) for k, v in hp.items()}, strict=False)
    assert not missing.unexpected_keys and all(k.startswith('breath_block.') or k == 'ones' for k in missing.missing_keys)
    m = m.to(dtype)
    ht = torch.from_numpy(h).to(dtype).requires_grad_(True)
    z = m.add_on_layers(ht)
    dist = m._l2_convolution(z)
    min_d = (-F.max_pool1d(-dist, kernel_size=dist.size()[2])).view(-1, m.num_prototypes)
    sim = m.distance_2_similarity(min_d)
    logits = m.last_layer(sim.view(B, -1))
    min_distances = min_d.view(B, -1)
    s = (logits * torch.from_numpy(g_logits).to(dtype)).sum() + (min_distances * torch.from_numpy(g_min).to(dtype)).sum()
    s.backward()
    vals = dict(logits=logits, min_distances=min_distances, dmap=ht.grad)
    vals.update({'grad/' + k: dict(m.named_parameters())[k].grad for k in hp})
    return {k: v.detach().numpy().astype(np.float64) for k, v in vals.items()}


def head():
    hp = R.seeded_head(SEED, 128, 128, 20, NB)
    h = R.seeded_map(SEED, B * NB, 128, 7)
    rng = np.random.default_rng([SEED, 99])
    g_logits = rng.standard_normal((B, 2)).astype(np.float32)
    g_min = (rng.standard_normal((B, NB * 20)) * 0.1).astype(np.float32)
    v64 = reference_head(h, hp, g_logits, g_min, torch.float64)
    v32 = reference_head(h, hp, g_logits, g_min, torch.float32)
    mine = R.head_case(h, hp, NB, g_logits, g_min)
    rec = dict(map=h, g_logits=g_logits, g_min=g_min, seed=SEED, nb=NB)
    rec.update({'hp/' + k: v for k, v in hp.items()})
    for k, a in v64.items():
        e = R.rel_l2(mine[k], a)
        assert e < 1e-12, (k, e)                        # ppnet_ref against the reference's modules
        rec[k] = a
        rec['err32/' + k] = R.rel_l2(v32[k], a)
        print('%-32s err32 %.3e  ppnet_ref %.1e' % (k, rec['err32/' + k], e))
    save('ppnet_head.npz', rec)


if __name__ == '__main__':
    keys()
    head()
