"""The head of the 1-D ProtoPNet restated with stock torch ops on the CPU, float64 by default: the add-on layers, the L2
prototype layer in the reference's EXPANDED form relu(sum z^2 - 2 sum z p + sum p^2), the global min-pool, the log
similarity, the bias-free last layer, calc_loss, and the prototype push in numpy (reference models/protopnet1d/model.py
:209-281, train_ards_detector.py:1194-1247, models/protopnet1d/ppnet_push.py:311-427).  The reference of the ProtoPNet tests;
tests/tools/make_golden_ppnet.py holds it against the reference's own classes.

Layouts are the reference's: maps (N, C, L), head parameters under their state_dict names."""
import numpy as np
import torch
import torch.nn.functional as F

EPSILON = 1e-4
L1_COEF = 1e-4


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    den = float(np.sqrt((b * b).sum()))
    return float(np.sqrt(((a - b) ** 2).sum())) / (den if den > 0 else 1.0)


def bound(err32):
    """The project's yardstick (tests/test_vgg_gpu.py): rel-l2 <= min(max(4 err32, 16 2^-23), 1e-4)."""
    return min(max(4.0 * float(err32), 16.0 * 2.0 ** -23), 1e-4)


def conv_indices(hp):
    """Indices of the add-on convs in ``add_on_layers`` (0, 2, 4, ...), from the parameter names."""
    return sorted(int(k.split('.')[1]) for k in hp if k.startswith('add_on_layers.') and k.endswith('.weight'))


def add_on(h, hp):
    """h (N, C, L) through the add-on layers: every conv is followed by a ReLU, the last one by the Sigmoid (both add-on
    shapes of model.py:159-185)."""
    idx = conv_indices(hp)
    for i in idx:
        h = F.conv1d(h, hp['add_on_layers.%d.weight' % i], hp['add_on_layers.%d.bias' % i])
        h = torch.sigmoid(h) if i == idx[-1] else torch.relu(h)
    return h


def l2_convolution(z, protos):
    """(N, D, L), (P, D, 1) -> (N, P, L): the expanded form of model.py:217-242."""
    x2 = F.conv1d(z ** 2, torch.ones_like(protos))
    p2 = (protos ** 2).sum(dim=(1, 2)).view(-1, 1)
    xp = F.conv1d(z, protos)
    return torch.relu(x2 + (-2 * xp + p2))


def l2_direct(z, protos):
    """(N, D, L), (P, D, 1) -> (N, P, L): sum_c (z - p)^2."""
    return ((z.unsqueeze(1) - protos.view(1, protos.shape[0], protos.shape[1], 1)) ** 2).sum(2)


def similarity(d):
    return torch.log((d + 1) / (d + EPSILON))


def prototype_layer(z, protos, direct=False):
    """-> dist (N, P, L), min_d (N, P), arg (N, P), sim (N, P)."""
    dist = l2_direct(z, protos) if direct else l2_convolution(z, protos)
    min_d = -F.max_pool1d(-dist, kernel_size=dist.shape[2])
    min_d = min_d.view(-1, protos.shape[0])
    return dist, min_d, dist.argmin(dim=2), similarity(min_d)


def head_forward(h, hp, nb, average_linear=False):
    """h (B * nb, C, L) the breath block's map, hp the head parameters -> logits (B, 2), min_distances (B, nb * P) and the
    intermediate z, dist, sim."""
    z = add_on(h, hp)
    protos = hp['prototype_vectors']
    dist, min_d, _, sim = prototype_layer(z, protos)
    b, p = h.shape[0] // nb, protos.shape[0]
    flat = sim.view(b, nb, p).mean(dim=1) if average_linear else sim.view(b, nb * p)
    logits = F.linear(flat, hp['last_layer.weight'])
    return dict(logits=logits, min_distances=min_d.view(b, nb * p), z=z, dist=dist, sim=sim)


def class_identity(num_prototypes, nb):
    """prototype_class_identity (nb * P, 2): prototype p belongs to class p // (P / 2), repeated over the breaths."""
    ident = torch.zeros(num_prototypes, 2, dtype=torch.float64)
    for j in range(num_prototypes):
        ident[j, j // (num_prototypes // 2)] = 1
    return ident.repeat((nb, 1))


def calc_loss(logits, target, min_distances, num_prototypes, nb, max_dist, clust_lambda, sep_lambda, l1_weight=None,
              l1_identity=None):
    """calc_loss, literally (train_ards_detector.py:1197-1246) -> total, cls, cluster, separation, l1."""
    ident = class_identity(num_prototypes, nb).to(logits.dtype)
    cls_loss = F.binary_cross_entropy(F.softmax(logits, dim=1), target)
    label = target.argmax(dim=1)
    correct = torch.t(ident[:, label])
    inverted, _ = torch.max((max_dist - min_distances) * correct, dim=1)
    cluster = torch.mean(max_dist - inverted)
    wrong = 1 - correct
    inverted_wrong, _ = torch.max((max_dist - min_distances) * wrong, dim=1)
    separation = torch.mean(max_dist - inverted_wrong)
    if l1_weight is not None:
        l1 = (l1_weight * (1 - torch.t(l1_identity.to(logits.dtype)))).norm(p=1)
    else:
        l1 = torch.zeros(1, dtype=logits.dtype).norm(p=1)
    loss = cls_loss + clust_lambda * cluster + sep_lambda * separation + L1_COEF * l1
    return loss, cls_loss, cluster, separation, l1


# ---- seeded head inputs (exactly representable float32 values) ----------------------------------------------------------
def head_shapes(c_in, d):
    """[(in, out)] of the bottleneck add-on convs behind a map of c_in channels (model.py:159-177)."""
    shapes, cur = [], c_in
    while cur > d or not shapes:
        out = max(d, cur // 2)
        shapes += [(cur, out), (out, out)]
        cur //= 2
    return shapes


def seeded_head(seed, c_in=128, d=128, p=20, nb=20, average_linear=False):
    """Head parameters under their state_dict names, float32: kaiming-like conv weights, small biases, uniform prototypes,
    a last layer of 1 / -0.5 plus noise."""
    rng = np.random.default_rng([seed, c_in, d, p, nb])
    hp = {}
    for i, (ci, co) in enumerate(head_shapes(c_in, d)):
        hp['add_on_layers.%d.weight' % (2 * i)] = (rng.standard_normal((co, ci, 1)) * np.sqrt(2.0 / co)).astype(np.float32)
        hp['add_on_layers.%d.bias' % (2 * i)] = (rng.standard_normal((co,)) * 0.1).astype(np.float32)
    hp['prototype_vectors'] = rng.random((p, d, 1)).astype(np.float32)
    k = p if average_linear else nb * p
    ident = class_identity(p, 1 if average_linear else nb).numpy()
    hp['last_layer.weight'] = (ident.T * 1.5 - 0.5 + rng.standard_normal((2, k)) * 0.05).astype(np.float32)
    return hp


def seeded_map(seed, rows, c, l):
    """A ReLU'd map (rows, c, l), float32."""
    rng = np.random.default_rng([seed, rows, c, l])
    return np.maximum(rng.standard_normal((rows, c, l)), 0).astype(np.float32)


def head_case(h, hp, nb, g_logits, g_min, dtype=torch.float64, average_linear=False):
    """logits, min_distances and, under the upstream gradients (g_logits (B, 2), g_min (B, nb * P)), the gradients on the map
    and on every head parameter -> {name: float64 array}."""
    ht = torch.from_numpy(np.asarray(h)).to(dtype).requires_grad_(True)
    pt = {k: torch.from_numpy(np.asarray(v)).to(dtype).requires_grad_(True) for k, v in hp.items()}
    out = head_forward(ht, pt, nb, average_linear)
    s = (out['logits'] * torch.from_numpy(np.asarray(g_logits)).to(dtype)).sum() + \
        (out['min_distances'] * torch.from_numpy(np.asarray(g_min)).to(dtype)).sum()
    s.backward()
    vals = dict(logits=out['logits'], min_distances=out['min_distances'], dmap=ht.grad)
    vals.update({'grad/' + k: v.grad for k, v in pt.items()})
    return {k: v.detach().numpy().astype(np.float64) for k, v in vals.items()}


# ---- the push, in numpy (ppnet_push.py:214-305, 311-427, without the figures) -------------------------------------------
def push_state(num_prototypes, d):
    return dict(min_dist=np.full(num_prototypes, np.inf), patches=np.zeros((num_prototypes, d), np.float32),
                source=np.full((num_prototypes, 3), -1, np.int64), rf_boxes=np.full((num_prototypes, 4), -1, np.int64))


def push_batch(state, z, dist, labels, start):
    """One search batch: z (B, NB, D, L) the prototype layer's input, dist (B, NB, P, L), labels (B,), ``start`` the absolute
    index of its first window.  Per prototype the first minimum in (window, breath, position) order over the windows of its
    own class; a later batch replaces an earlier one on a strict < only."""
    p = dist.shape[2]
    for j in range(p):
        cls = j // (p // 2)
        idx = [i for i, y in enumerate(labels) if int(y) == cls]
        if not idx:
            continue
        dj = dist[idx, :, j, :]
        m = np.amin(dj)
        if m < state['min_dist'][j]:
            w, n, l = np.unravel_index(np.argmin(dj, axis=None), dj.shape)
            w = idx[w]
            state['min_dist'][j] = m
            state['patches'][j] = z[w, n, :, l]
            state['source'][j] = (start + w, n, l)
            state['rf_boxes'][j, 0] = start + w
            state['rf_boxes'][j, 3] = cls
    return state
