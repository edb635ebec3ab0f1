"""The operands of the whole-model regressor goldens, shared by tests/tools/make_golden_regressor.py (which runs the reference on
them) and tests/test_regressor_gpu.py (which runs this package and the numpy oracle on them): seeded backbone weights
(``oracle.weights.seeded_params``), a (9, F) ``linear_final``, R breath-like rows and raw-metadata-like targets."""
import zlib

import numpy as np

from oracle.weights import seeded_batch, seeded_params

M_OUT = 9
WIDTH = {'resnet18': 512, 'densenet18': 128}


def regressor_case(net, r):
    """-> dict(params {state_dict key: float32 array}, x (R, 1, 224) float32, target (R, 9) float32)."""
    seed = 40 + r
    params = {k: v for k, v in seeded_params(net, seed).items() if not k.startswith('linear_final.')}
    rng = np.random.default_rng([seed, zlib.crc32(net.encode()), 9])
    f = WIDTH[net]
    bound = 1.0 / np.sqrt(f)
    params['linear_final.weight'] = rng.uniform(-bound, bound, (M_OUT, f)).astype(np.float32)
    params['linear_final.bias'] = rng.uniform(-bound, bound, (M_OUT,)).astype(np.float32)
    x = np.ascontiguousarray(seeded_batch(1, r, seed, 'flow')[0][0])                    # (R, 1, 224)
    # targets of the scales the head's outputs have at these weights (|out| ~ 1): the loss and its gradients then weigh the
    # network's outputs and the targets alike; the raw-metadata scales, 1e-2 ... 1e3, are the head tests' own cases
    target = (rng.standard_normal((r, M_OUT)) * np.linspace(0.25, 4.0, M_OUT)).astype(np.float32)
    return dict(params=params, x=x.astype(np.float32), target=target)


def regressor_oracle(net, r, dtype=np.float64):
    """The numpy oracle (oracle/np_ref through decision_match.feature_reference) of CNNRegressor on ``regressor_case(net, r)`` in
    ``dtype``: ALL R rows one BatchNorm window, the head stated by regress_ref -> dict(feat, out, loss, grads, tape, rebackward)."""
    import regress_ref as RR
    from decision_match import feature_reference
    c = regressor_case(net, r)
    cast = lambda a: np.asarray(a, dtype=dtype)
    w, b, target = cast(c['params']['linear_final.weight']), cast(c['params']['linear_final.bias']), cast(c['target'])

    def head(feat):
        fwd = RR.forward(feat, w, b, target)
        bwd = RR.backward(feat, w, fwd['out'], target)
        return bwd['dx'], dict(grads={'linear_final.weight': bwd['dW'], 'linear_final.bias': bwd['db']}, out=fwd['out'],
                               loss=fwd['loss'])
    params = {k: cast(v) for k, v in c['params'].items() if not k.startswith('linear_final.')}
    return feature_reference(params, r, cast(c['x']), head, net)
