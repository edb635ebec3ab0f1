"""Float64 numpy restatement of the siamese head, its loss, their gradients and the triplet draw -- the oracle of
tests/test_siamese_gpu.py, itself checked against stock torch autograd in tests/test_siamese_cpu.py.  Written from the formulas:

    u[p][r][c] = b1[c] + sum_d W1[c][d] |fc_p[r][d] - fa_p[r][d]|          p = 0: (anchor, positive), 1: (anchor, negative)
    z[p][b][o] = b2[o] + sum_j W2[o][j] vec(u[p][b NB : (b + 1) NB])[j]
    loss       = mean_{b,o} bce(z[0], [0, 1]) + mean_{b,o} bce(z[1], [1, 0]),   bce(z, t) = max(z, 0) - z t + log1p(exp(-|z|))

Every function also returns ``S``: the same expression evaluated on absolute values (the scale a float32 rounding error is
relative to), and ``bound(n, S) = 4 (n + 2) 2^-24 S`` is the componentwise tolerance of an n-term float32 sum in any order, the
factor 4 covering the transcendental and the two-stage folds."""
import numpy as np

U = 2.0 ** -24
TARGET = np.array([[0.0, 1.0], [1.0, 0.0]])             # [pair][logit]


def bound(n, S):
    return 4.0 * (n + 2) * U * np.asarray(S, dtype=np.float64)


# ---- the draw -------------------------------------------------------------------------------------------------------------
def mix32(a, b):
    """common.h's mix32 on uint32 values (numpy arrays or ints), computed in uint64 and masked."""
    m = np.uint64(0xffffffff)
    a = np.asarray(a, dtype=np.uint64) & m
    b = np.asarray(b, dtype=np.uint64) & m
    h = ((a * np.uint64(0x9E3779B1)) & m) ^ ((b + np.uint64(0x7F4A7C15)) & m)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & m
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & m
    h ^= h >> np.uint64(16)
    return h


def patient_tables(counts):
    """(pat_start, pat_count) int32 per window, (patient per window) for patients with ``counts`` contiguous windows each."""
    counts = np.asarray(counts, dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    return (np.repeat(starts, counts).astype(np.int32), np.repeat(counts, counts).astype(np.int32),
            np.repeat(np.arange(len(counts)), counts))


def draw(anchor, pat_start, pat_count, seed, step, literal):
    """-> int64 [anchor | pos | anchor | neg] (literal) or [anchor | pos | neg]."""
    anchor = np.asarray(anchor, dtype=np.int64)
    n = len(pat_start)
    ps, pc = pat_start[anchor].astype(np.int64), pat_count[anchor].astype(np.int64)
    pos = np.where(anchor + 1 < ps + pc, anchor + 1, anchor - 1)
    r = mix32(mix32(seed, step), np.arange(len(anchor)))
    off = ((r * (n - pc).astype(np.uint64)) >> np.uint64(32)).astype(np.int64)
    neg = np.where(off < ps, off, off + pc)
    return np.concatenate([anchor, pos, anchor, neg] if literal else [anchor, pos, neg]).astype(np.int64)


# ---- the head -------------------------------------------------------------------------------------------------------------
def _f64(*arrays):
    return [np.asarray(a, dtype=np.float64) for a in arrays]


def sigmoid(z):
    return np.where(z >= 0, 1.0 / (1.0 + np.exp(-np.abs(z))), np.exp(-np.abs(z)) / (1.0 + np.exp(-np.abs(z))))


def head_forward(fa_pos, fc_pos, fa_neg, fc_neg, W1, b1, W2, b2, B, NB):
    """-> dict(u (2, B NB, 2), z (2, B, 2), loss, S_u, S_z, S_loss)."""
    fa_pos, fc_pos, fa_neg, fc_neg, W1, b1, W2, b2 = _f64(fa_pos, fc_pos, fa_neg, fc_neg, W1, b1, W2, b2)
    x = np.stack([np.abs(fc_pos - fa_pos), np.abs(fc_neg - fa_neg)])                   # (2, R, D)
    u = x @ W1.T + b1
    S_u = x @ np.abs(W1).T + np.abs(b1)
    z = u.reshape(2, B, 2 * NB) @ W2.T + b2
    S_z = S_u.reshape(2, B, 2 * NB) @ np.abs(W2).T + np.abs(b2)
    t = TARGET[:, None, :]
    terms = np.maximum(z, 0) - z * t + np.log1p(np.exp(-np.abs(z)))
    S_terms = S_z + S_z * t + np.log1p(np.exp(-np.abs(z)))
    return dict(u=u, z=z, loss=terms.sum() / (2 * B), S_u=S_u, S_z=S_z, S_loss=S_terms.sum() / (2 * B))


def head_backward(fa_pos, fc_pos, fa_neg, fc_neg, W1, W2, u, z, B, NB, shared, gscale=1.0):
    """Gradients of ``gscale * loss`` from the forward's u and z (as the backward kernel takes them) -> dict of dfa_pos,
    dfc_pos, dfa_neg (None when shared: dfa_pos is then the sum over both pairs), dfc_neg, dW1, db1, dW2, db2 and S_<name>."""
    fa_pos, fc_pos, fa_neg, fc_neg, W1, W2, u, z = _f64(fa_pos, fc_pos, fa_neg, fc_neg, W1, W2, u, z)
    R = B * NB
    gs = gscale / (2.0 * B)
    t = TARGET[:, None, :]
    dz = (sigmoid(z) - t) * gs                                                          # (2, B, 2)
    S_dz = (sigmoid(z) + t) * abs(gs)
    du = (dz @ W2).reshape(2, R, 2)                                                     # (2, B, 2 NB) -> per row
    S_du = (S_dz @ np.abs(W2)).reshape(2, R, 2)
    diff = np.stack([fc_pos - fa_pos, fc_neg - fa_neg])
    sgn = np.sign(diff)
    dfc = sgn * (du @ W1)                                                               # (2, R, D)
    S_dfc = np.abs(sgn) * (S_du @ np.abs(W1))
    out = dict(dfc_pos=dfc[0], dfc_neg=dfc[1], S_dfc_pos=S_dfc[0], S_dfc_neg=S_dfc[1])
    if shared:
        out.update(dfa_pos=-dfc[0] - dfc[1], S_dfa_pos=S_dfc[0] + S_dfc[1], dfa_neg=None, S_dfa_neg=None)
    else:
        out.update(dfa_pos=-dfc[0], S_dfa_pos=S_dfc[0], dfa_neg=-dfc[1], S_dfa_neg=S_dfc[1])
    ad = np.abs(diff)
    out.update(dW1=np.einsum('prc,prd->cd', du, ad), S_dW1=np.einsum('prc,prd->cd', S_du, ad),
               db1=du.sum(axis=(0, 1)), S_db1=S_du.sum(axis=(0, 1)),
               dW2=np.einsum('pbo,pbj->oj', dz, u.reshape(2, B, 2 * NB)),
               S_dW2=np.einsum('pbo,pbj->oj', S_dz, np.abs(u).reshape(2, B, 2 * NB)),
               db2=dz.sum(axis=(0, 1)), S_db2=S_dz.sum(axis=(0, 1)))
    return out


def sum_lengths(B, NB, D, shared):
    """n of ``bound`` per output: the length of the longest sum behind an element."""
    return dict(u=D, z=2 * NB, loss=4 * B, dfc_pos=2, dfc_neg=2, dfa_pos=4 if shared else 2, dfa_neg=2, dW1=2 * B * NB,
                db1=2 * B * NB, dW2=2 * B, db2=2 * B)


# ---- inputs of the head tests ---------------------------------------------------------------------------------------------
def make_case(B, NB, D, shared, seed=0):
    """float32 operands and parameters of one head case with the hard spots the tests name:
      * equal: pair 0, every third column of every row and (R > 1) the whole of row 0 have fc == fa exactly;
      * denormal: pair 0, last row, columns d % 3 == 1: fa = 1.5e-38 (normal), fc = fa +- m 2^-149, so fc - fa is denormal;
      * big: pair 1, window B - 1: fc scaled until both |z| of that window exceed 45.
    -> dict of numpy float32 arrays (fa_neg IS fa_pos when shared) and ``big`` = (pair, window)."""
    rng = np.random.RandomState(1000 * seed + 97 * B + 13 * NB + D + (7 if shared else 0))
    R = B * NB
    f = lambda *s: rng.randn(*s).astype(np.float32)
    fa_pos, fc_pos, fc_neg = f(R, D), f(R, D), f(R, D)
    fa_neg = fa_pos if shared else f(R, D)
    W1, b1 = (f(2, D) / np.float32(np.sqrt(D))), f(2) * np.float32(0.1)
    W2, b2 = (f(2, 2 * NB) / np.float32(np.sqrt(2 * NB))), f(2) * np.float32(0.1)
    fc_pos[:, 0::3] = fa_pos[:, 0::3]
    if R > 1:
        fc_pos[0] = fa_pos[0]
    cols = np.arange(1, D, 3)
    if len(cols):
        m = (rng.randint(1, 1000, size=len(cols)) * np.where(np.arange(len(cols)) % 2, -1, 1)).astype(np.float64)
        base = np.float32(1.5e-38)
        fa_pos[R - 1, cols] = base
        fc_pos[R - 1, cols] = (np.float64(base) + m * 2.0 ** -149).astype(np.float32)
    win = slice((B - 1) * NB, B * NB)
    k = 1.0
    for _ in range(60):
        trial = fc_neg.copy()
        trial[win] *= np.float32(k)
        z = head_forward(fa_pos, fc_pos, fa_neg, trial, W1, b1, W2, b2, B, NB)['z'][1, B - 1]
        if np.abs(z).min() > 45:
            break
        k *= 2.0
    fc_neg = trial
    return dict(fa_pos=fa_pos, fc_pos=fc_pos, fa_neg=fa_neg, fc_neg=fc_neg, W1=W1, b1=b1, W2=W2, b2=b2, big=(1, B - 1))
