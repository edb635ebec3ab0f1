"""A float64 numpy model of the statistics records (include/deepards_hip.h "Statistics records") and of the shapes at which
tests/test_dense_edges_gpu.py runs their producers.

Layout of a record buffer for ``units`` units of N channels, tiles = ceil(units / 64):

    floats [tiles][2 window slots][{mean, M2}][N]  |  counts [tiles][2]

A tile of 64 units touches at most two windows of Wu >= 64 units.  Slot 0 of tile t belongs to the window that holds the
tile's first unit, slot 1 to the window that STARTS inside the tile (common.h merge_stat_records: "a tile whose first unit
lies in front of the window: the window is its second slot").  count is the number of stored POSITIONS, not units: a
Winograd unit is an output pair, 2 positions, or 1 where an odd row ends (conv_wino.hip ``scnt[sl] += has1 ? 2.f : 1.f``)."""
import numpy as np


def tiles_of(units):
    return (units + 63) // 64


class positions(object):
    """per_unit of the producers whose units are output positions (conv1x1_bn, conv3_bf16_bn)."""

    def __init__(self, n):
        self.units = n

    def __call__(self, u):
        return (u,)


class pairs(object):
    """per_unit of the Winograd producer: unit u = row * ceil(L / 2) + p holds positions 2p and 2p + 1 of its row of L, the
    second one absent where an odd row ends."""

    def __init__(self, rows, L):
        self.L, self.pl = L, (L + 1) // 2
        self.units = rows * self.pl

    def __call__(self, u):
        row, p = divmod(u, self.pl)
        base = row * self.L + 2 * p
        return (base, base + 1) if 2 * p + 1 < self.L else (base,)


def unpack(buf, units, N):
    """flat record buffer -> (mean[tiles, 2, N], M2[tiles, 2, N], count[tiles, 2])"""
    buf = np.asarray(buf).reshape(-1)
    t = tiles_of(units)
    assert buf.size == t * 4 * N + t * 2, (buf.size, units, N)
    body = buf[:t * 4 * N].reshape(t, 2, 2, N)
    return body[:, :, 0, :], body[:, :, 1, :], buf[t * 4 * N:].reshape(t, 2)


def records(values, Wu, per_unit, units=None, dtype=np.float64):
    """The records a producer owes for its stored output ``values`` (positions, N), windows of Wu units.  Two-pass mean and
    centred M2 per (tile, slot) in ``dtype``; empty slots hold count 0 (and zeros, which nobody may read)."""
    values = np.asarray(values, dtype=dtype)
    units = per_unit.units if units is None else units
    assert Wu >= 64 and units % Wu == 0
    t, N = tiles_of(units), values.shape[1]
    mean, M2, count = np.zeros((t, 2, N), dtype), np.zeros((t, 2, N), dtype), np.zeros((t, 2))
    for tile in range(t):
        first = (tile * 64) // Wu                                    # the window of the tile's first unit: slot 0
        pos = ([], [])
        for u in range(tile * 64, min(tile * 64 + 64, units)):
            sl = u // Wu - first
            assert sl in (0, 1)
            pos[sl].extend(per_unit(u))
        for sl in (0, 1):
            if pos[sl]:
                v = values[pos[sl]]
                count[tile, sl] = len(pos[sl])
                mean[tile, sl] = v.sum(axis=0, dtype=dtype) / dtype(len(pos[sl]))
                M2[tile, sl] = ((v - mean[tile, sl]) ** 2).sum(axis=0, dtype=dtype)
    return mean, M2, count


def spreads(values, Wu, per_unit):
    """For allowances derived from a single-pass kernel's summation (sums about a pivot, which is one of the tile's stored
    values): per (tile, slot, channel) the mean absolute deviation of the slot's values from their mean, and the largest
    distance of ANY value of the tile -- either slot -- from that mean.  Float64, from the stored values alone."""
    values = np.asarray(values, np.float64)
    units = per_unit.units
    t, N = tiles_of(units), values.shape[1]
    mad, far = np.zeros((t, 2, N)), np.zeros((t, 2, N))
    for tile in range(t):
        first = (tile * 64) // Wu
        pos = ([], [])
        for u in range(tile * 64, min(tile * 64 + 64, units)):
            pos[u // Wu - first].extend(per_unit(u))
        everything = values[pos[0] + pos[1]]
        for sl in (0, 1):
            if pos[sl]:
                m = values[pos[sl]].mean(axis=0)
                mad[tile, sl] = np.abs(values[pos[sl]] - m).mean(axis=0)
                far[tile, sl] = np.abs(everything - m).max(axis=0)
    return mad, far


def merge(mean, M2, count, Wu, W, eps, dtype=np.float64):
    """Chan's update over a window's records in tile order, as merge_stat_records does -> (mean[W, N], invstd[W, N])."""
    t, _, N = mean.shape
    out_m, out_i = np.zeros((W, N), dtype), np.zeros((W, N), dtype)
    for w in range(W):
        u0 = w * Wu
        n, mu, m2 = dtype(0), np.zeros(N, dtype), np.zeros(N, dtype)
        for r in range(u0 >> 6, min((u0 + Wu - 1) >> 6, t - 1) + 1):
            sl = 0 if (r << 6) >= u0 else 1
            nb = dtype(count[r, sl])
            if nb > 0:
                d = mean[r, sl].astype(dtype) - mu
                nt = n + nb
                mu = mu + d * (nb / nt)
                m2 = m2 + M2[r, sl].astype(dtype) + d * d * (n * nb / nt)
                n = nt
        out_m[w] = mu
        out_i[w] = dtype(1) / np.sqrt(m2 / max(n, dtype(1)) + dtype(eps))
    return out_m, out_i


def window_stats(values, positions_per_window, W, eps):
    """The direct float64 statistics of the stored output (positions, N) -> (mean[W, N], invstd[W, N]), biased variance."""
    v = np.asarray(values, np.float64).reshape(W, positions_per_window, -1)
    return v.mean(axis=1), 1.0 / np.sqrt(v.var(axis=1) + eps)


# ---- the shapes of tests/test_dense_edges_gpu.py, as (R, L, W): rows = R W -------------------------------------------------
WINO_SHAPES = [(16, 8, 3),            # Wu = 64: whole tiles, every second slot empty
               (16, 7, 3),            # the same with a half-filled last pair per row
               (13, 9, 3),            # Wu = 65: every window but the first starts inside a tile, last tile of 3 pairs
               (129, 4, 2),           # Wu = 258: a window over 5-6 records -- the merge loop's second pass and clamped tail
               (64, 1, 2), (64, 2, 2),  # L = 1, 2: one pair per row ((32, 2, 2) has 32 pairs a window: refused, asserted there)
               (32, 4, 1),            # one window, one tile, a launch of one block
               (1, 128, 2)]           # R = 1
C1_SHAPES = [(16, 4, 3), (13, 5, 3), (43, 6, 2), (16, 4, 1), (64, 1, 2), (1, 64, 2)]       # (R, Lout, W); pool: L = 2 Lout
C1_WINO_BN_SHAPES = [(32, 4, 2), (33, 3, 3), (13, 10, 3)]       # the 1x1 conv in front of conv3_winograd_bn
BF16_SHAPES = [(65, 2, 3), (10, 13, 3),   # Wn = 130, the minimum: 128-position tiles of two records, last tile of 6 positions
               (131, 1, 2),               # L = 1
               (193, 3, 2),               # Wn = 579: ten records per window, the 8-record loop's second pass
               (130, 1, 1)]               # one window


def record_geometries():
    """Every (name, units, Wu, per_unit, positions per window, W) of the tables above."""
    out = []
    for R, L, W in WINO_SHAPES:
        pu = pairs(R * W, L)
        out.append(('wino %s' % ((R, L, W),), pu.units, R * pu.pl, pu, R * L, W))
    for R, L, W in C1_SHAPES + C1_WINO_BN_SHAPES:
        out.append(('conv1x1 %s' % ((R, L, W),), R * L * W, R * L, positions(R * L * W), R * L, W))
    for R, L, W in BF16_SHAPES:
        out.append(('bf16 %s' % ((R, L, W),), R * L * W, R * L, positions(R * L * W), R * L, W))
    return out


def windowed(rng, W, R, C, L):
    """(rows, C, L) float32-valued inputs whose windows do NOT look alike: every (window, channel) has its own offset
    (within +-3) and scale (0.5 .. 2), and every row a small ramp.  -> x, offsets (W, C), scales (W, C)"""
    off = rng.uniform(-3, 3, (W, 1, C, 1))
    sc = rng.uniform(0.5, 2, (W, 1, C, 1))
    ramp = 0.05 * np.arange(R)[None, :, None, None] / max(R - 1, 1)
    x = rng.standard_normal((W, R, C, L)) * sc + off + ramp
    x = x.reshape(W * R, C, L).astype(np.float32).astype(np.float64)
    return x, off.reshape(W, C), sc.reshape(W, C)


def neighbours_differ(y, R):
    """The share of channels, worst over the pairs of neighbouring windows, in which the per-channel means of y (rows, N, L)
    differ by more than half a standard deviation (the larger of the two windows')."""
    rows, N, L = y.shape
    v = y.reshape(rows // R, R, N, L)
    m, s = v.mean(axis=(1, 3)), v.std(axis=(1, 3))
    share = 1.0
    for w in range(rows // R - 1):
        share = min(share, float((np.abs(m[w + 1] - m[w]) > 0.5 * np.maximum(s[w], s[w + 1])).mean()))
    return share
