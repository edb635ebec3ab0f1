"""Goldens of the lstm_only networks from the REAL reference classes (models/lstm_only.py), run where the reference is
checked out ($DEEPARDS_REFERENCE, default: a `reference` directory beside this repository); never imported by a test:

    python tests/tools/make_golden_lstm_only.py

Writes tests/golden/lstm_only_<name>.npz per case: the module's seeded parameters (torch's default initialisation under
torch.manual_seed, float32), the input windows (float32: rows of test_dataset_windows.npz scaled as the store scales them,
(x - mu) / std), a fixed random r (B, 2), and -- from the module converted with .double() -- the logits and the gradient of
sum(logits * r) on every parameter, float64.  A case whose file would pass the size limit keeps the gradient of
linear_breath_inst.weight in a second file, lstm_only_<name>_gradw.npz.

Cases: LSTMOnlyNetwork at (B, NB, H) = (2, 3, 8) and (2, 20, 16); LSTMOnlyWithPacking at (2, 4, 8), whose eight rows are
    0  zeros from 100 on            (length 101)      4  no zero                       (224)
    1  a zero at 0 only             (224)             5  all zeros                     (224)
    2  zeros from 1 on              (2)               6  a -0.0 at 150, nothing before (151)
    3  a zero only at 223           (224)             7  zeros from 57 on              (58)
``lens`` records the lengths the reference's pack_sequence took."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.environ.get('DEEPARDS_REFERENCE', os.path.join(os.path.dirname(ROOT), 'reference')))

from deepards.models.lstm_only import LSTMOnlyNetwork, LSTMOnlyWithPacking                   # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden')
LIMIT = 1 << 20


def windows(b, nb):
    z = np.load(os.path.join(OUT, 'test_dataset_windows.npz'))
    x = ((z['x'] - float(z['mu'])) / float(z['std'])).astype(np.float32)                    # (20, 20, 1, 224)
    x = np.ascontiguousarray(x[:b, :nb])
    assert not (x == 0).any()                           # real samples: no exact zero after scaling
    return x


def packing_rows(x):
    rows = x.reshape(-1, 224)
    assert rows.shape[0] == 8
    rows[0, 100:] = 0.0
    rows[1, 0] = 0.0
    rows[2, 1:] = 0.0
    rows[3, 223] = 0.0
    rows[5, :] = 0.0
    rows[6, 150] = -0.0
    rows[7, 57:] = 0.0
    return rows.reshape(x.shape), np.array([101, 224, 2, 224, 224, 224, 151, 58])


def run(cls, h, x, r, seed):
    torch.manual_seed(seed)
    m = cls(h, x.shape[1])
    params = {k: v.detach().numpy().copy() for k, v in m.state_dict().items()}
    m = m.double()
    logits = m(torch.from_numpy(x).double(), None)
    (logits * torch.from_numpy(r).double()).sum().backward()
    grads = {k: p.grad.numpy().astype(np.float64) for k, p in m.named_parameters()}
    return params, logits.detach().numpy().astype(np.float64), grads


def save(name, rec):
    path = os.path.join(OUT, name)
    np.savez_compressed(path, **rec)
    size = os.path.getsize(path)
    print(name, size)
    return size


def case(name, cls, b, nb, h, seed, packing=False):
    x = windows(b, nb)
    lens = None
    if packing:
        x, lens = packing_rows(x)
        got = np.argmax(x.reshape(-1, 224) == 0, axis=1)
        got[got == 0] = 223
        assert (got + 1 == lens).all(), (got + 1, lens)
    r = np.random.default_rng([seed, 7]).standard_normal((b, 2)).astype(np.float32)
    params, logits, grads = run(cls, h, x, r, seed)
    assert np.isfinite(logits).all() and tuple(logits.shape) == (b, 2)
    rec = dict(x=x, r=r, logits=logits, seed=seed, shape=np.array([b, nb, h]))
    if lens is not None:
        rec['lens'] = lens
    rec.update({'param/' + k: v for k, v in params.items()})
    rec.update({'grad/' + k: v for k, v in grads.items()})
    big = 'grad/linear_breath_inst.weight'
    if sum(v.nbytes for v in rec.values() if isinstance(v, np.ndarray)) > LIMIT - (64 << 10):
        assert save('lstm_only_%s_gradw.npz' % name, {big: rec.pop(big)}) < LIMIT
    assert save('lstm_only_%s.npz' % name, rec) < LIMIT


if __name__ == '__main__':
    case('2x3x8', LSTMOnlyNetwork, 2, 3, 8, 41)
    case('2x20x16', LSTMOnlyNetwork, 2, 20, 16, 42)
    case('packing_2x4x8', LSTMOnlyWithPacking, 2, 4, 8, 43, packing=True)
