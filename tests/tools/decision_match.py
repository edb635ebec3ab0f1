"""Test helper: gradient parity under matched activation decisions (see the docstring)."""
import os

import numpy as np

from oracle import np_ref


def _stem_effects(ref, known, base, cands):
    """``ref['rebackward'](known + [c])`` for every stem decision c, at the price of the stem's backward alone: the gradient
    that reaches the stem does not depend on the stem's own decisions, so it is taken once from a run under ``known`` and
    only the stem's parameters are recomputed (tests/test_gradient_yardstick_cpu.py holds this to the full re-run)."""
    t = ref['tape']
    ref['rebackward'](known)                                   # leaves the cotangent of THESE known flips on the tape
    stem_in, kept = t.stem_in, t.g
    for name, i, _ in cands:
        d = t.decisions[name]
        key = 'mask' if d['kind'] == 'relu' else 'idx'
        saved = d[key]
        np_ref._apply_flip(t, name, i)
        t.g = {}
        try:
            t.stem_bwd(stem_in)
            g = dict(base)
            g.update(t.g)
        finally:
            d[key], t.g = saved, kept
        yield g


def decision_matched_gradients(ref, ours, log_tag='', tols=(1e-5, 3e-5), log=print, max_eval=128, known=(), only=None,
                               accept=None):
    """The exact (fp64 oracle) gradients under the activation decisions THIS run took.

    An fp32 forward differs from the fp64 one by ~1e-6 relative, enough to take a ReLU / max-pool decision the other way
    on the few elements whose pre-activation is that close to zero; ONE such element changes every upstream gradient by
    up to ~3e-2 relative (it is one of ~10^4 elements of a late feature map).  The reference does it to itself: its own
    fp32 vs fp64 gradients differ by 3.1e-2 rel-l2 on densenet18_b4_flow.  So gradients are compared with the oracle's
    gradients under the SAME decisions.  The oracle lists its ambiguous decisions (|pre-activation| or max-pool gap
    < tol); for each the backward is re-run with that one decision flipped (forward untouched) -> its effect D_e.
    Matching pursuit over the candidates in order of decreasing effect: a flip is adopted when the current residual
    (ours - exact - adopted effects) projects onto D_e with coefficient > 1/2.  The adopted set is then applied at once
    in an exact re-run.  Effects are matched on a fixed coordinate subsample (<= 2048 per parameter), the verdict is
    taken by the caller on the full tensors.  At most ``max_eval`` candidates are evaluated per tolerance, those closest
    to their decision boundary first (every evaluation is one oracle backward: seconds for the deeper backbones).
    ``known``: flips [(name, index)] that are not searched for but KNOWN -- the decisions the run under test exported
    (``hip_relu_flips``) -- they are part of every backward here; ``only(name)``: restrict the search to those decisions
    (the ones the run cannot export: the stem's fused ReLU / max-pool).
    ``accept(gradients) -> bool``: the caller's verdict on ``ours`` against these gradients; the search stops as soon as it
    holds and is not begun where it holds already.  Without one: not begun below 2e-5, stopped below 1e-4 (rel-l2, worst
    parameter) -- shortcuts as loose as the 1e-4 criterion they were written for, so a caller with a tighter bound per
    tensor must hand it in, or a stem decision worth 1e-5 of conv0.weight is never looked for.
    Returns (gradients, flips adopted (known ones first), number of candidates)."""
    known = list(known)
    base = ref['rebackward'](known) if known else ref['grads']
    names = [n for n in base if n in ours]
    # gradients that are analytically zero (a conv in front of a BatchNorm when every ReLU is active) get a unit
    # scale: their error is judged absolutely, not relative to a norm of ~1e-17
    # ... and one whose norm is small but not zero is weighted by the size of error the verdict tolerates on it (1e-4 per
    # element), or fp32 noise on ~1e-9 gradients would steer the matching
    scale = {n: max(float(np.linalg.norm(base[n])), 1e-4 * np.sqrt(base[n].size)) for n in names}
    known3 = [(n, i, 0.0) for n, i in known]
    if accept(base) if accept is not None else max(np.linalg.norm(ours[n] - base[n]) / scale[n] for n in names) < 2e-5:
        return base, known3, 0
    stem_only = only is is_stem_decision and hasattr(ref['tape'], 'stem_bwd')
    rng = np.random.RandomState(0)
    sub = {n: (np.arange(base[n].size) if base[n].size <= 2048 else np.sort(rng.choice(base[n].size, 2048, replace=False)))
           for n in names}
    pack = lambda g: np.concatenate([(g[n].ravel()[sub[n]] - base[n].ravel()[sub[n]]) *
                                     (np.sqrt(base[n].size / len(sub[n])) / scale[n]) for n in names])
    got, chosen, cands = base, [], []
    for tol in tols:
        cands = [c for c in np_ref.ambiguous_decisions(ref['tape'], tol) if (only is None or only(c[0])) and (c[0], c[1]) not in set(known)]
        cands = sorted(cands, key=lambda c: c[2])[:max_eval]
        if stem_only:
            effects = [pack(g) for g in _stem_effects(ref, known, base, cands)]
        else:
            effects = [pack(ref['rebackward'](known + [(name, i)])) for name, i, _ in cands]
        resid = pack(ours)
        chosen = []
        for k in np.argsort([-float(e @ e) for e in effects]):
            e = effects[k]
            if float(e @ e) < 1e-12:                          # cannot move any parameter by 1e-6 relative
                break
            if float(resid @ e) / float(e @ e) > 0.5:
                chosen.append(cands[k])
                resid = resid - e
        got = ref['rebackward'](known + [(n, i) for n, i, _ in chosen]) if chosen else base
        worst = max(np.linalg.norm(ours[n] - got[n]) / scale[n] for n in names)
        log('   %s decision matching: tol %.0e, %d candidates, %d flips adopted %s, worst rel-l2 after %.2e' %
            (log_tag, tol, len(cands), len(chosen), [(n.split('.', 1)[1], i, '%.1e' % m) for n, i, m in chosen], worst))
        if accept(got) if accept is not None else worst < 1e-4:
            break
    return got, known3 + chosen, len(cands)


STEM_DECISIONS = ('bn1.relu', 'bn1.maxpool', 'bn2.relu', 'bn2.maxpool', 'norm0.relu', 'norm0.maxpool')


def is_stem_decision(name):
    return name.endswith(STEM_DECISIONS)


def hip_relu_flips(tape, taps, log=print, tag='', near=3e-5):
    """The ReLU decisions the run under test TOOK, as flips of the oracle's: ``taps`` are the post-ReLU activations the
    block Functions recorded (deepards_amd.functional.DECISION_TAP: float (rows, L, C) or x3 tensors, in forward order),
    one per ReLU of the oracle's tape behind the stem (the stem's ReLU and max-pool are fused into one kernel and export
    nothing: ``decision_matched_gradients(only=is_stem_decision)`` searches those).  Every differing element must be one
    whose fp64 pre-activation is within ``near`` of zero -- anything else is a wrong value, not a decision.  ``near`` is
    the oracle's own ambiguity tolerance (``decision_matched_gradients(tols=...)``: 3e-5; the largest exported
    pre-activation ever measured is 7.5e-6): a looser bound would let a 1e-4-sized VALUE error pass as
    "a decision"."""
    names = [n for n in tape.order if tape.decisions[n]['kind'] == 'relu' and not is_stem_decision(n)]
    assert len(names) == len(taps), 'decision tap: %d activations for %d ReLUs' % (len(taps), len(names))
    flips = []
    for name, t in zip(names, taps):
        d = tape.decisions[name]
        if t.dim() == 5:                                    # x3 format: the sign of the leading term is the sign of the value
            t = t[:, :, :, 0, :].reshape(t.shape[0], t.shape[1], -1)
        mask = (t.detach().float() > 0).permute(0, 2, 1).cpu().numpy()
        assert mask.shape == d['mask'].shape, (name, mask.shape, d['mask'].shape)
        idx = np.flatnonzero(mask != d['mask'])
        if len(idx):
            far = np.abs(d['pre'].flat[idx]).max()
            assert far < near, '%s: a ReLU decision differs where the fp64 pre-activation is %.2e from zero' % (name, far)
            flips += [(name, int(i)) for i in idx]
    if flips:
        log('   %s exported decisions: %d ReLU elements on the other side of zero than the fp64 oracle (|pre| <= %.1e)' %
            (tag, len(flips), max(abs(tape.decisions[n]['pre'].flat[i]) for n, i in flips)))
    return flips


def rel_l2(a, b):
    """||a - b|| / ||b||; a reference of norm zero has no relative scale: 0 where a == b, inf otherwise."""
    err, nb = float(np.linalg.norm(a - b)), float(np.linalg.norm(b))
    return err / nb if nb > 0 else (0.0 if err == 0 else float('inf'))


NORTH_STAR = 1e-4                 # BASELINE north_star: the ceiling of every bound here
MARGIN = 8                        # x the oracle's own fp32 error: the BasicBlock chain's convention
FLOOR = 16 * 2.0 ** -23           # as tests/test_se_gpu.py: no bound below a few fp32 roundings
MAX_UNPINNED = 2                  # per case that is not '_active' (the oracle alone gives at most 1 on every golden)


def bound(err32):
    return min(max(MARGIN * err32, FLOOR), NORTH_STAR)


def fp32_noise(ref64, ref32):
    """What float32 arithmetic alone does to every parameter gradient of one case: ``ref32`` is the oracle call that made
    ``ref64`` on float32 operands.  Its gradients are compared with the float64 gradients under the decisions the float32
    run itself took: its ReLU masks and max-pool indices are read off its tape and put on the float64 tape for one
    ``rebackward`` (no matching pursuit: the oracle exports every decision, the stem's included).
    -> {name: dict(err32=rel-l2, abs=||g32 - g64||, norm=||g64||)}, plus under the key None the number of decision
    elements the two runs took differently."""
    t64, t32 = ref64['tape'], ref32['tape']
    assert t64.order == t32.order
    saved, differ = {}, 0
    for name in t64.order:
        d64, d32 = t64.decisions[name], t32.decisions[name]
        key = 'mask' if d64['kind'] == 'relu' else 'idx'
        n = int(np.count_nonzero(d64[key] != d32[key]))
        if n:
            differ += n
            saved[name] = (key, d64[key])
            d64[key] = d32[key]
    try:
        exact = ref64['rebackward']([]) if saved else ref64['grads']
    finally:
        for name, (key, val) in saved.items():
            t64.decisions[name][key] = val
    out = {None: differ}
    for n, g in ref32['grads'].items():
        assert g.dtype == np.float32, (n, g.dtype)               # a float64 constant in the oracle would flatter err32
        e = exact[n]
        assert e.dtype == np.float64, (n, e.dtype)
        out[n] = dict(err32=rel_l2(g.astype(np.float64), e), abs=float(np.linalg.norm(g.astype(np.float64) - e)),
                      norm=float(np.linalg.norm(e)))
    return out


_NOISE = {}


def cached_noise(key, ref64, make_ref32):
    """``fp32_noise`` once per process and ``key`` (a golden's name + whatever else selects the oracle call): several tests
    share one golden, and the float32 oracle run costs as much as the float64 one."""
    if key not in _NOISE:
        _NOISE[key] = fp32_noise(ref64, make_ref32())
    return _NOISE[key]


def oracle_pair(params, x, target, key=None, **kw):
    """``np_ref.cnn_linear_forward_backward`` on float64 copies of the operands and, for the noise figure, on float32
    copies -> (ref64, fp32_noise); ``key``: cache the figure under that name."""
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    ref = np_ref.cnn_linear_forward_backward({k: f64(v) for k, v in params.items()}, f64(x), f64(target), **kw)
    make32 = lambda: np_ref.cnn_linear_forward_backward(as_f32(params), as_f32(x), as_f32(target), **kw)
    return ref, (cached_noise(key, ref, make32) if key is not None else fp32_noise(ref, make32()))


def plain_twin(path):
    """The golden of the same case without the BatchNorm shift that makes every ReLU active."""
    return path.replace('_active', '')


def as_f32(tree):
    """float32 copies of a dict of arrays / an array (the operands of the float32 oracle run)."""
    return {k: as_f32(v) for k, v in tree.items()} if isinstance(tree, dict) else np.asarray(tree, dtype=np.float32)


def assert_gradients_match(ref, ours, ref32, tag='', strict=False, max_flips=12, log=print, allow=None, taps=None,
                           active=None, twin=None, zero=()):
    """THE gradient yardstick of this suite.  Every parameter of ``ours`` (name -> float64 array) against the oracle's exact
    gradients under the activation decisions this run took (``decision_matched_gradients``), each tensor held to a
    RELATIVE bound taken from what float32 does to that very tensor in the oracle itself.

    ``ref32``: the oracle call of ``ref`` on float32 operands, or the ``fp32_noise(ref, ...)`` dict made from it.  Per tensor
    with err32 = rel-l2 of the float32 oracle against the float64 one under its own decisions:
      pinned   (8 * err32 <= 1e-4):  rel-l2(ours, matched) <= min(max(8 * err32, 16 * 2^-23), 1e-4), no absolute escape;
      unpinned (8 * err32 >  1e-4):  the exact gradient is ~0 or ill-conditioned in float32 itself, there is no relative
               scale: max|err| <= 1e-4 * max(1, max|ref|), and ||ours - matched|| / ||g32 - g64|| is logged (each side
               against the exact gradient under its OWN decisions).
    A case that is not ``active`` (default: no '_active' in ``tag``) may have at most 2 unpinned tensors, not counting the
    parameters named in ``zero``: gradients that are zero in exact arithmetic for a reason the caller documents, which must
    then be ~zero in the oracle (norm <= 1e-12) and stay under the absolute rule.  An '_active' case
    (every ReLU active: the net in front of a BatchNorm is affine and many gradients are analytically zero) has no cap; it
    logs ``pinned k of n``, and where k < n / 2 it is no gradient evidence: ``twin`` (the path of its plain twin golden)
    must then exist.
    At most ``max_flips`` adopted flips, no ReLU flip when ``strict`` (goldens whose every ReLU is active; a DenseNet
    stem's max-pool keeps its near-ties even there: two neighbouring conv outputs 1e-5 apart are not moved by a BatchNorm
    shift).  ``allow(name) -> bool`` exempts named parameters (callers document why).  ``taps``: the post-ReLU activations
    the run recorded (functional.DECISION_TAP) -- its decisions are then TAKEN from the run (``hip_relu_flips``) and only
    the stem's fused ReLU / max-pool decisions are searched.
    Returns (worst rel-l2, flips)."""
    noise = ref32 if 'grads' not in ref32 else fp32_noise(ref, ref32)

    def verdict(n, exact):
        """(within its bound, pinned, figure judged, bound) of one tensor against ``exact``."""
        if MARGIN * noise[n]['err32'] <= NORTH_STAR:
            rl2, lim = rel_l2(ours[n], exact[n]), bound(noise[n]['err32'])
            return rl2 <= lim, True, rl2, lim
        abs_err, peak = float(np.abs(ours[n] - exact[n]).max()), float(np.abs(exact[n]).max())
        return abs_err <= NORTH_STAR * max(1.0, peak), False, abs_err, NORTH_STAR * max(1.0, peak)
    accept = lambda exact: all(verdict(n, exact)[0] or (allow is not None and allow(n)) for n in ours if n in exact)
    if taps is not None:       # the run exported its ReLU decisions: nothing to search for behind the stem
        known = hip_relu_flips(ref['tape'], taps, log=log, tag=tag)
        matched, flips, ncand = decision_matched_gradients(ref, ours, tag, log=log, known=known, only=is_stem_decision,
                                                           accept=accept)
    else:
        matched, flips, ncand = decision_matched_gradients(ref, ours, tag, log=log, accept=accept)
    if strict:
        assert not [f for f in flips if not f[0].endswith('.maxpool')], flips
    assert len(flips) <= max_flips, flips
    active = ('_active' in tag) if active is None else active
    worst, worst_ratio, bad, unpinned, total = 0.0, 0.0, [], [], 0
    for n in ours:
        if n not in matched:
            continue
        total += 1
        e32 = noise[n]
        rl2 = rel_l2(ours[n], matched[n])
        ok, is_pinned, figure, lim = verdict(n, matched)
        if is_pinned:
            ratio = rl2 / max(e32['err32'], FLOOR / MARGIN)
            worst, worst_ratio = max(worst, rl2), max(worst_ratio, ratio)
            log('   %s grad %-60s pinned   rel-l2 %.3e err32 %.3e bound %.3e (%.2f x err32)' % (tag, n, rl2, e32['err32'], lim, ratio))
        else:
            if n in zero:
                assert e32['norm'] <= 1e-12, (n, e32['norm'])
            unpinned.append(n)
            ratio = float(np.linalg.norm(ours[n] - matched[n])) / e32['abs'] if e32['abs'] > 0 else float('inf')
            log('   %s grad %-60s unpinned rel-l2 %.3e err32 %.3e max|err| %.3e bound %.3e (abs); ||ours - exact|| = %.2f x the '
                'float32 oracle\'s' % (tag, n, rl2, e32['err32'], figure, lim, ratio))
        entry = (n, 'pinned' if is_pinned else 'unpinned', figure, e32['err32'], lim)
        if not ok and not (allow is not None and allow(n)):
            bad.append(entry)
    pinned = total - len(unpinned)
    log('   %s pinned %d of %d; worst pinned rel-l2 %.3e = %.2f x err32; %d flips of %d candidates; the float32 oracle took %d '
        'decisions the other way' % (tag, pinned, total, worst, worst_ratio, len(flips), ncand, noise[None]))
    assert not bad, bad
    if not active:
        assert len([n for n in unpinned if n not in zero]) <= MAX_UNPINNED, unpinned
    elif pinned < total / 2.0:
        log('   %s is NOT gradient evidence (fewer than half of its gradients have a relative scale); its plain twin is: %s' %
            (tag, twin))
        assert twin is not None and os.path.exists(twin), twin
    return worst, flips


def feature_reference(params, rows_per_window, x, cotangent, backbone='resnet18', **tape_flags):
    """The oracle at breath-block level, in the dtype of its operands (float64: the reference; float32: the noise figure of
    ``fp32_noise``) -- features of ``x`` (rows, 1, L) and the parameter gradients of
    sum(features * cotangent) -- in the form ``decision_matched_gradients`` wants (grads, tape, rebackward).  Used where
    CNNLinearNetwork itself refuses the shape (seq_len != 224, torch_cnn_linear_network.py:106-107)."""
    t = np_ref._Tape(params, rows_per_window)
    for k, v in tape_flags.items():
        setattr(t, k, v)
    fn = np_ref.resnet18_features if backbone.startswith('resnet') else np_ref.densenet18_features
    feat, bwd = fn(t, x)
    extra = {}
    if callable(cotangent):                 # a head stated by the caller: feat -> (d loss / d feat, its own gradients, ...)
        cotangent, extra = cotangent(feat)

    def run():
        t.g = {}
        bwd(cotangent)
        g = dict(t.g)
        g.update(extra.get('grads', {}))
        return g

    def rebackward(flips):
        saved = {}
        for name, i in flips:
            d = t.decisions[name]
            key = 'mask' if d['kind'] == 'relu' else 'idx'
            saved.setdefault(name, (key, d[key]))
            np_ref._apply_flip(t, name, i)
        try:
            return run()
        finally:
            for name, (key, val) in saved.items():
                t.decisions[name][key] = val
    out = dict(feat=feat, grads=run(), tape=t, rebackward=rebackward)
    out.update({k: v for k, v in extra.items() if k != 'grads'})
    return out
