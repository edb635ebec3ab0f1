"""The float64 model of the statistics records (tests/tools/stat_records_ref.py) pinned by itself, before
tests/test_dense_edges_gpu.py lets it judge a kernel: its slot and layout rule must merge to the direct per-window statistics
at every geometry of that file's tables, and its counts must be the hand-written ones below."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'tools'))

import stat_records_ref as SR  # noqa: E402

GEOMETRIES = SR.record_geometries()


@pytest.mark.parametrize('geo', GEOMETRIES, ids=[g[0] for g in GEOMETRIES])
def test_merged_records_are_the_window_statistics(geo):
    name, units, Wu, per_unit, wn, W = geo
    N, eps = 5, 1e-5
    rng = np.random.default_rng(units + Wu)
    v = rng.standard_normal((W, wn, N)) * rng.uniform(0.5, 2, (W, 1, N)) + rng.uniform(-3, 3, (W, 1, N))
    v = v.reshape(W * wn, N)
    assert per_unit.units == units and units == W * Wu
    seen = sorted(p for u in range(units) for p in per_unit(u))
    assert seen == list(range(W * wn)), 'the units cover every stored position exactly once'
    mean, M2, count = SR.records(v, Wu, per_unit)
    assert mean.shape == (SR.tiles_of(units), 2, N) and count.shape == (SR.tiles_of(units), 2)
    assert count.sum() == W * wn
    got_m, got_i = SR.merge(mean, M2, count, Wu, W, eps)
    ref_m, ref_i = SR.window_stats(v, wn, W, eps)
    assert np.abs(got_m - ref_m).max() <= 1e-12 * (1 + np.abs(ref_m).max())
    assert np.abs(got_i / ref_i - 1).max() <= 1e-12
    # the flat layout round-trips, counts behind the bodies
    flat = np.concatenate([np.stack([mean, M2], axis=2).reshape(-1), count.reshape(-1)])
    m2, q2, c2 = SR.unpack(flat, units, N)
    assert np.array_equal(m2, mean) and np.array_equal(q2, M2) and np.array_equal(c2, count)


def test_a_record_in_the_wrong_slot_is_noticed():
    """The 1e-12 above means something: move one window-start record to the other slot and the merge is off by O(1)."""
    R, L, W = 13, 9, 3
    pu = SR.pairs(R * W, L)
    rng = np.random.default_rng(1)
    v = (rng.standard_normal((W, R * L, 4)) + 4 * np.arange(W)[:, None, None]).reshape(-1, 4)
    mean, M2, count = SR.records(v, R * pu.pl, pu)
    for a in (mean, M2, count):
        a[1] = a[1, ::-1].copy()
    got_m, _ = SR.merge(mean, M2, count, R * pu.pl, W, 1e-5)
    assert np.abs(got_m - SR.window_stats(v, R * L, W, 1e-5)[0]).max() > 0.01


def test_counts_by_hand():
    """Wu = 64: every second slot is empty.  Wu = 65 (13 rows of 9 = 5 pairs, the last one half-filled): worked out by hand.
    Wu = 64 with L = 7: 16 rows of 7 positions in every tile."""
    _, _, count = SR.records(np.zeros((16 * 3 * 8, 1)), 64, SR.pairs(48, 8))
    assert count.tolist() == [[128, 0], [128, 0], [128, 0]]
    # pairs 0..63: rows 0..11 (108 positions) and 4 pairs of row 12 (8) | pair 64: the single last position of row 12 closes
    # window 0, pairs 65..127 = rows 13..24 (108) + 3 pairs of row 25 (6) | pairs 128, 129 close window 1 (2 + 1), pairs
    # 130..191 = rows 26..37 (108) + 2 pairs of row 38 (4) | pairs 192..194: the rest of row 38 (2 + 2 + 1)
    _, _, count = SR.records(np.zeros((13 * 3 * 9, 1)), 65, SR.pairs(39, 9))
    assert count.tolist() == [[116, 0], [1, 114], [3, 112], [5, 0]]
    _, _, count = SR.records(np.zeros((16 * 3 * 7, 1)), 64, SR.pairs(48, 7))
    assert count.tolist() == [[112, 0], [112, 0], [112, 0]]


def test_float32_evaluation_is_a_float32_evaluation():
    """records(dtype=float32) / merge(dtype=float32) -- the e32 figures of the GPU tests -- stay in float32."""
    v = np.random.default_rng(0).standard_normal((130, 3))
    mean, M2, count = SR.records(v, 130, SR.positions(130), dtype=np.float32)
    assert mean.dtype == np.float32 and M2.dtype == np.float32
    m, i = SR.merge(mean, M2, count, 130, 1, 1e-5, dtype=np.float32)
    assert m.dtype == np.float32 and i.dtype == np.float32
    assert np.abs(m - v.mean(axis=0)).max() < 1e-6
