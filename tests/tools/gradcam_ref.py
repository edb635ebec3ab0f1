"""Float64 numpy restatement of the reference's CAM arithmetic (gradcam.py:125-205: MaxMinNormCam.generate_read_cam /
generate_cam / normalize, FracTotalNormCam.generate_read_cam / normalize, UnNormalizedCam.generate_cam), with the np.mean
weights and the channel loops kept as they stand there.  The guided gradients come from the closed form

    d out[k] / d conv[n, c, l] = (conv[n, c, l] > 0) * W[k, n * C + c] / Lm

of the head relu -> AvgPool1d(Lm) -> view(-1) -> linear_final (CamExtractor.forward_pass, :51-65).  Beside every float output
the functions return S, the sum of the absolute values of the terms that make it up: a summation whose longest serial chain
has k additions is within k * 2^-24 * S of the exact value in float32, which is what the GPU tests assert with k = 160.

Also here, because the CPU and the GPU tests share them: the synthetic cases of the kernel-level tests (``CASES`` /
``make_case``) and the rule for the uint8 outputs (``maxmin_slack`` / ``frac_slack`` / ``excused``).
"""
import numpy as np

U32 = 2.0 ** -24            # unit round-off of float32
CHAIN = 160                 # the serial-chain limit the kernels keep: the bound is CHAIN * U32 * S


def head_forward(conv, W, bias):
    """conv (NB, C, Lm) float64 -> (out (2,), S (2,)): relu -> avgpool -> view(-1) -> linear_final."""
    h = np.maximum(conv, 0.0)
    flat = np.mean(h, axis=2).reshape(-1)
    out = W @ flat + bias
    return out, np.abs(W) @ flat + np.abs(bias)


def closed_form_gradient(conv, W, k):
    """The guided gradient of out[k] at conv (NB, C, Lm): what register_hook + backward deliver in the reference."""
    nb, c, lm = conv.shape
    return (conv > 0).astype(np.float64) * W[k].reshape(nb, c, 1) / lm


def read_cam(conv, grad):
    """generate_read_cam's loop (:130-134) without the normalisation -> (cam (NB, Lm), S (NB, Lm))."""
    weights = np.mean(grad, axis=(2,))
    cam = np.zeros((conv.shape[0], conv.shape[2]), dtype=np.float64)
    s = np.zeros_like(cam)
    for i, b in enumerate(conv):
        for j, w in enumerate(weights[i, :]):
            cam[i] += w * conv[i, j, :]
            s[i] += np.abs(w * conv[i, j, :])
    return cam, s


def window_cam(conv, grad):
    """generate_cam's loop (:143-153) without the normalisation -> (cam (Lm,), S (Lm,)).  S: every weight is a mean of
    gradients and every map value a mean over the breaths, so the terms are the products of the absolute values' means."""
    weights = np.mean(grad, axis=(0, 2))
    aweights = np.mean(np.abs(grad), axis=(0, 2))
    conv_output = np.mean(conv, axis=0)
    aconv = np.mean(np.abs(conv), axis=0)
    cam = np.zeros(conv_output.shape[1:], dtype=np.float64)
    s = np.zeros_like(cam)
    for i, w in enumerate(weights):
        cam += w * conv_output[i, :]
        s += aweights[i] * aconv[i, :]
    return cam, s


def maxmin_normalize(cam):
    """MaxMinNormCam.normalize (:157-162) over the last axis of a (Lm,) CAM -> (bytes, y, degenerate): y = 255 (r - min) /
    (max - min) before the truncation.  max == min: the reference casts 0 / 0 to uint8 (platform-defined); here 0, flagged."""
    r = np.maximum(cam, 0)
    lo, hi = np.min(r), np.max(r)
    if hi == lo:
        return np.zeros(r.shape, dtype=np.uint8), np.zeros(r.shape), True
    y = (r - lo) / (hi - lo) * 255
    return np.uint8(y), y, False


def frac_normalize(cam_target, cam_other):
    """FracTotalNormCam.normalize (:187-192) -> (bytes, y); 0 where both ReLU'd CAMs are 0."""
    t, o = np.maximum(cam_target, 0), np.maximum(cam_other, 0)
    den = o + t
    y = np.where(den > 0, t / np.where(den > 0, den, 1.0) * 255, 0.0)
    return np.uint8(y), y


def window(conv, W, bias, target_in=-1):
    """Everything the device computes for one window.  conv (NB, C, Lm) (any float type; taken to float64), W (2, NB C),
    bias (2,), target_in 0 / 1 / -1 (the predicted class: np.argmax, a tie gives 0)."""
    conv, W, bias = np.asarray(conv, np.float64), np.asarray(W, np.float64), np.asarray(bias, np.float64)
    nb, c, lm = conv.shape
    out, s_out = head_forward(conv, W, bias)
    t = int(target_in) if target_in >= 0 else int(np.argmax(out))
    res = dict(logits=out, S_logits=s_out, target=t, A=np.zeros((2, lm)), S_A=np.zeros((2, lm)), R=np.zeros((2, nb, lm)),
               S_R=np.zeros((2, nb, lm)))
    for k in (0, 1):
        grad = closed_form_gradient(conv, W, k)
        res['A'][k], res['S_A'][k] = window_cam(conv, grad)
        res['R'][k], res['S_R'][k] = read_cam(conv, grad)
    res['cam'] = np.maximum(0, res['A'][t])                                    # UnNormalizedCam
    res['cam_maxmin'], res['cam_y'], res['cam_degenerate'] = maxmin_normalize(res['A'][t])
    rows = [maxmin_normalize(res['R'][t][i]) for i in range(nb)]
    res['read_maxmin'] = np.stack([r[0] for r in rows])
    res['read_y'] = np.stack([r[1] for r in rows])
    res['read_degenerate'] = np.array([r[2] for r in rows])
    res['read_frac'], res['frac_y'] = frac_normalize(res['R'][t], res['R'][1 - t])
    return res


def batch(fmap, W, bias, targets, nb):
    """``window`` for every window of a channels-last map (B * nb, Lm, C) -> list of B results."""
    fmap = np.asarray(fmap)
    b = fmap.shape[0] // nb
    return [window(np.transpose(fmap[i * nb:(i + 1) * nb], (0, 2, 1)), W, bias, int(targets[i])) for i in range(b)]


# ---- the rule for the uint8 outputs -------------------------------------------------------------------------------------------
def maxmin_slack(v, e):
    """d: the largest error the pre-truncation value y_i = 255 (r_i - mn) / D, D = mx - mn, of a row can carry when every
    CAM value v_i (last axis) is known to e_i (same shape; the float bound CHAIN * U32 * S).
    ReLU, min and max do not amplify: |r'_i - r_i| <= e_i, |mn' - mn| and |mx' - mx| <= E = max e.  With N_i = r_i - mn,
        |N'_i - N_i| <= e_i + E,  |D' - D| <= 2 E,   y'_i - y_i = 255 (dN D - N_i dD) / (D D')
        => |y'_i - y_i| <= 255 (e_i + E + (N_i / D) 2 E) / (D - 2 E)          (D > 2 E; else nothing can be said: inf)
    plus the float32 evaluation of the expression itself: two subtractions, a division and a product, each within 2^-24
    relative, on a value of at most 255: 255 * 4.1 * 2^-24."""
    v, e = np.asarray(v, np.float64), np.asarray(e, np.float64)
    r = np.maximum(v, 0)
    mn, mx = r.min(axis=-1, keepdims=True), r.max(axis=-1, keepdims=True)
    big = e.max(axis=-1, keepdims=True)
    d = mx - mn
    ok = d > 2 * big
    safe = np.where(ok, d - 2 * big, 1.0)
    slack = 255 * (e + big + (r - mn) / np.where(d > 0, d, 1.0) * 2 * big) / safe + 255 * 4.1 * U32
    # entries whose byte is exact whatever the errors (D' > 0 given): a value at or below -e is 0 on the device too, and with
    # one such value in the row the minimum is 0 on both sides: y' = 0; a maximum (minimum) that stays the only one under the
    # errors of every value is the device's too: y' = 255 (0) from x / x = 1 (0 / D' = 0).  A row whose every value is at or
    # below -e is degenerate on both sides: all bytes 0.
    off = v <= -e
    exact = off & off.any(axis=-1, keepdims=True)
    lo, hi = r - e, r + e
    n = r.shape[-1]
    if n > 1:
        top, bot = np.argmax(r, axis=-1)[..., None], np.argmin(r, axis=-1)[..., None]
        idx = np.arange(n)
        others_hi = np.where(idx == top, -np.inf, hi).max(axis=-1, keepdims=True)
        others_lo = np.where(idx == bot, np.inf, lo).min(axis=-1, keepdims=True)
        exact = exact | ((idx == top) & (np.take_along_axis(lo, top, -1) > others_hi))
        exact = exact | ((idx == bot) & (np.take_along_axis(hi, bot, -1) < others_lo))
    return np.where(off.all(axis=-1, keepdims=True), 0.0, np.where(ok, np.where(exact, 0.0, slack), np.inf))


def frac_slack(vt, et, vo, eo):
    """d for y = 255 rt / (rt + ro): with den = rt + ro and the errors et, eo of the two CAM values,
        y' - y = 255 (ro dt - rt do) / (den den')  =>  |y' - y| <= 255 (ro et + rt eo) / (den (den - et - eo))
    (den > et + eo; else inf), plus one addition, a division and a product in float32: 255 * 3.1 * 2^-24."""
    vt, vo = np.asarray(vt, np.float64), np.asarray(vo, np.float64)
    et, eo = np.asarray(et, np.float64), np.asarray(eo, np.float64)
    rt, ro = np.maximum(vt, 0), np.maximum(vo, 0)
    den = rt + ro
    ok = den > et + eo
    slack = 255 * (ro * et + rt * eo) / np.where(ok, den * (den - et - eo), 1.0) + 255 * 3.1 * U32
    # exact whatever the errors: a target value at or below -et is 0 on the device too (y' = 0 with any denominator); the
    # other class's at or below -eo with a target value above et gives x / x = 1: y' = 255
    exact = (vt <= -et) | ((vo <= -eo) & (vt > et))
    return np.where(exact, 0.0, np.where(ok, slack, np.inf))


def excused(y, d):
    """Where the byte trunc(y) may differ by one: y lies within d of an integer (d = 0: the byte is exact, never excused)."""
    y, d = np.asarray(y, np.float64), np.asarray(d, np.float64)
    return (np.abs(y - np.rint(y)) <= d) & (d > 0)


# ---- the synthetic cases of the kernel-level tests ------------------------------------------------------------------------------
# (B, NB, C) at Lm = 7 with the targets of the windows; `plant` names the hard inputs of the case (make_case)
CASES = {
    'b1_nb1_c128': dict(shape=(1, 1, 128), targets=(-1,), plant=('zeros',), seed=11),
    'b2_nb20_c128': dict(shape=(2, 20, 128), targets=(1, -1), plant=('negative_class', 'negative_row'), seed=12),
    'b3_nb3_c1664': dict(shape=(3, 3, 1664), targets=(0, -1, 1), plant=('zeros', 'negative_row'), seed=13),
    'b2_nb2_c1920': dict(shape=(2, 2, 1920), targets=(-1, 1), plant=(), seed=14),
    'b1_nb20_c1024': dict(shape=(1, 20, 1024), targets=(0,), plant=('zeros',), seed=15),
}
LM = 7


def make_case(name):
    """-> dict(fmap (B NB, Lm, C) float32 channels-last, W (2, NB C) float32, bias (2,) float32, targets (B,) int32, nb).
    The map is a position profile per row times a positive channel amplitude, plus noise, so that a CAM has the contrast
    over l that a trained network's has (a map of independent noise gives CAMs whose max - min is a rounding-error-sized
    share of their terms, and bytes that say nothing); both classes' weights have a positive mean, class 1's smaller.
    Planted: 'zeros' -- exact +0.0 and -0.0 in whole (row, position, channel) blocks, which must not count in m;
    'negative_row' -- the last window's row NB // 2 all negative: P = 0 there and its read CAM is degenerate;
    'negative_class' -- W[1] = -|W[1]| and window 0 all positive with target 1: its window CAM and every read CAM are
    nowhere positive."""
    spec = CASES[name]
    b, nb, c = spec['shape']
    rng = np.random.RandomState(spec['seed'])
    prof = 0.15 + 1.6 * rng.rand(b * nb, LM, 1)
    amp = 0.2 + np.abs(rng.randn(b * nb, 1, c))
    fmap = (prof * amp + 0.35 * rng.randn(b * nb, LM, c) - 0.25).astype(np.float32)
    W = ((rng.randn(2, nb * c) + np.array([[1.0], [0.6]])) / np.sqrt(nb * c)).astype(np.float32)
    bias = np.array([0.05, -0.02], dtype=np.float32)
    if 'zeros' in spec['plant']:
        fmap[0, 2, ::3] = 0.0
        fmap[-1, 5, 1::4] = -0.0
        fmap[0, :, 8:16] = 0.0                    # channels that are zero at every position: m = 0
    if 'negative_row' in spec['plant']:
        n = (b - 1) * nb + nb // 2
        fmap[n] = -np.abs(fmap[n]) - 1e-3
    if 'negative_class' in spec['plant']:
        W[1] = -np.abs(W[1])
        fmap[:nb] = np.abs(fmap[:nb]) + 1e-3
    return dict(fmap=np.ascontiguousarray(fmap), W=np.ascontiguousarray(W), bias=bias,
                targets=np.array(spec['targets'], dtype=np.int32), nb=nb)


def byte_slacks(ref):
    """The three uint8 outputs of one window's result -> {name: (y, d)}; the CAM values are known to CHAIN * U32 * S.  d = 0:
    the byte is exact; inf (a row too flat for its errors): nothing can be said of that row, its degenerate flag included."""
    t = ref['target']
    ea, er = CHAIN * U32 * ref['S_A'], CHAIN * U32 * ref['S_R']
    return {'cam_maxmin': (ref['cam_y'], maxmin_slack(ref['A'][t], ea[t])),
            'read_maxmin': (ref['read_y'], maxmin_slack(ref['R'][t], er[t])),
            'read_frac': (ref['frac_y'], frac_slack(ref['R'][t], er[t], ref['R'][1 - t], er[1 - t]))}


def excused_share(refs):
    """(excused entries, entries) over the uint8 outputs of a case's windows."""
    n = m = 0
    for ref in refs:
        for y, d in byte_slacks(ref).values():
            n += int(excused(y, d).sum())
            m += d.size
    return n, m
