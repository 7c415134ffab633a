"""CPU side of the stats rows of closed-loop bang-bang rollouts (tests/test_bangbang_stats_gpu.py).

1. The size guard of the block partials a STATS window launch writes: ``mdr_window_stats_check`` passes
   with ``mdr_window_stats_bytes(n)`` and fails with MDR_EARG one byte short (host-only functions).

2. The GPU test's inputs do not degenerate under the oracle, for both controllers and per shape: the
   ON count and the lockout count each take at least 3 distinct values over the ticks (so slots 10 and
   11 are not a constant), and a signed temperature sum has terms of both signs at some tick (so a
   signed slot is not its absolute twin).

   Two of the shapes cannot meet this as stated and the test says so instead of hiding it.
   * n = 1 has counts in {0, 1} and one term per sum: the shape is there for the one-lane path, and is
     left out here, as tests/test_bangbang_rollout_cpu.py leaves it out.
   * ``e = T - target / N`` (slots 0-3: Metrics' operator precedence, kept from the reference) is
     positive for every house at every tick of every shape with N >= 2: T is about 20 degC and
     target / N at most 10.  No input of this kind gives it both signs, so the two-sign property is
     asserted on ``d = T - target`` (slots 6 and 7), the difference the controllers regulate; the
     smallest e is printed.
"""
import random

import numpy as np
import pytest

import golden_util as gu
from bangbang_inputs import CTRLS, SEED, SHAPES, overrides
from oracle import env_np as O

STATS_SHAPES = SHAPES + [(300, 37, 32)]  # + a ragged last block


def test_window_stats_size_guard():
    from mdr_amd import _lib

    lib = _lib.load()
    hpt, kmax, kstats = 2, 32, 12  # kWinHpt, kWindowMax, kStats (mdr_kernels.h)
    for n in (1, 128, 129, 513, 4099):
        need = lib.mdr_window_stats_bytes(n)
        tiles = (n + 64 * hpt - 1) // (64 * hpt)
        assert need == (tiles + 3) // 4 * kmax * kstats * 8, n  # a partial per tick and 4-wave block
        assert lib.mdr_window_stats_check(n, need) == 0, lib.mdr_last_error()
        assert lib.mdr_window_stats_check(n, need + 1) == 0
        assert lib.mdr_window_stats_check(n, need - 1) == -1  # MDR_EARG
        assert b"stats partial" in lib.mdr_last_error()
    assert lib.mdr_window_stats_bytes(-1) == 0
    assert lib.mdr_window_stats_check(0, 1 << 20) == -1


def oracle_variety(n, ticks, ctrl):
    props = gu.props_from_overrides(overrides(n))
    ora = O.OracleEnv(props, random.Random(SEED))
    db = props.cluster_prop.house_prop.deadband
    tg = ora.pop["target"]
    on, lock, d_both, e_min = set(), set(), 0, np.inf
    for _ in range(ticks):
        a = O.bangbang(ora.T, tg) if ctrl == "bangbang" else O.deadband_bangbang(ora.T, tg, db, ora.on)
        ora.step(a)
        on.add(int(ora.on.sum()))
        lock.add(int(ora.lock.sum()))
        d = ora.T - tg
        d_both += int((d > 0).any() and (d < 0).any())
        e_min = min(e_min, float((ora.T - tg / n).min()))
    return on, lock, d_both, e_min


@pytest.mark.parametrize("ctrl", CTRLS)
@pytest.mark.parametrize("n,ticks,win", [s for s in STATS_SHAPES if s[0] >= 2])
def test_inputs_do_not_degenerate(n, ticks, win, ctrl):
    on, lock, d_both, e_min = oracle_variety(n, ticks, ctrl)
    print(f"n={n} ticks={ticks} {ctrl}: {len(on)} ON counts, {len(lock)} lockout counts, "
          f"{d_both} ticks with T - target of both signs, min (T - target / N) = {e_min:.3f}")
    assert len(on) >= 3 and len(lock) >= 3
    assert d_both > 0
