"""NumPy restatement of the sharded stats rows' exchange, shared by
tests/test_stats_sharded_cpu.py and tests/test_stats_sharded_gpu.py: "zero-padded sum, then rank-order
combine".

Rank r holds partial rows P_r[m][16] and contributes the slab X_r[world][m][16] that is zero except
X_r[r] = P_r.  A sum-allreduce adds the world slabs in SOME order or tree; every element has exactly one
non-zero addend, so the result is that addend (a -0.0 arrives as +0.0) whatever the order.  The combine
then adds the ranks' rows in rank order (slot 2: max) — one fixed order on every rank.
"""
import numpy as np

ROW = 16
N_STATS = 12
S_MAX = 2
S_POWER = 12


def padded(parts, r):
    """Rank r's contribution: [world][m][16], zero except its own rows."""
    x = np.zeros((len(parts),) + parts[r].shape, np.float64)
    x[r] = parts[r]
    return x


def allreduce_chain(parts, order):
    """The slabs added one by one in ``order`` (a permutation of the ranks)."""
    acc = padded(parts, order[0]).copy()
    for r in order[1:]:
        acc = acc + padded(parts, r)
    return acc


def allreduce_tree(parts, order):
    """The slabs added pairwise, level by level, in ``order``."""
    level = [padded(parts, r) for r in order]
    while len(level) > 1:
        nxt = [level[i] + level[i + 1] for i in range(0, len(level) - 1, 2)]
        if len(level) % 2:
            nxt.append(level[-1])
        level = nxt
    return level[0]


def combine(x, rank):
    """Rows [m][16] from the allreduced slab x[world][m][16], as k_stats_rows_combine<false> forms
    them on ``rank``: slots 0..11 over the ranks in rank order (slot 2 by max), slot 12 from the
    rank's own rows, 13..15 zero."""
    world, m, _ = x.shape
    rows = np.zeros((m, ROW), np.float64)
    for k in range(N_STATS):
        v = x[0, :, k].copy()
        for r in range(1, world):
            v = np.maximum(v, x[r, :, k]) if k == S_MAX else v + x[r, :, k]
        rows[:, k] = v
    rows[:, S_POWER] = x[rank, :, S_POWER]
    return rows


def sum_slot_bound(single_rows, n):
    """|sharded - single| allowed per sum slot of the rows [m][16] of a cluster of n houses: two
    groupings of the same n terms differ by at most 2 (n - 1) 2^-53 sum|t_i| <= n 2^-52 A_k, with
    A_k = sum|t_i| taken from the single-process row itself: slot 0 (signed) from slot 1 (its absolute
    values), slot 6 from slot 7, slot 4 from |slot 4| (1 + 8 * 2^-53) (every reward <= 0: |sum| = sum of
    the absolute values, up to the row's own rounding), the others from themselves (non-negative terms)."""
    a = np.abs(single_rows[:, :N_STATS]).copy()
    a[:, 0] = single_rows[:, 1]
    a[:, 6] = single_rows[:, 7]
    a[:, 4] = np.abs(single_rows[:, 4]) + 8 * 2.0 ** -53 * np.abs(single_rows[:, 4])
    return n * 2.0 ** -52 * a
