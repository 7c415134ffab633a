"""The inputs of tests/test_bangbang_sharded_gpu.py cannot hide a missing or misplaced allreduce:
under the oracle, with the product's split of the houses over the ranks ([r n // w, (r + 1) n // w)),
over the first 70 ticks of the GPU script (its three-window rollout) and for both controllers,

* at every tick at least two ranks have houses ON, so a rank-local cluster power differs from the
  cluster's at every tick (a finish that skipped the allreduce would miss every reward row), and
* the per-rank ON counts take at least 50 distinct values over the ticks, so totals of the wrong
  tick or window (a slot reused too early, an allreduce one window off) do not go unnoticed.
"""
import random

import numpy as np
import pytest

import golden_util as gu
from bangbang_inputs import CTRLS, SEED, overrides
from oracle import env_np as O

TICKS = 70


def rank_counts(n, world, ctrl, ticks=TICKS):
    """[ticks][world] ON houses per rank after each tick of the controller under the oracle."""
    props = gu.props_from_overrides(overrides(n))
    ora = O.OracleEnv(props, random.Random(SEED))
    db = props.cluster_prop.house_prop.deadband
    tg = ora.pop["target"]
    edges = [r * n // world for r in range(world + 1)]
    rows = []
    for _ in range(ticks):
        a = O.bangbang(ora.T, tg) if ctrl == "bangbang" else O.deadband_bangbang(ora.T, tg, db, ora.on)
        o, _ = ora.step(a)
        on = np.asarray(o["on"], bool)
        rows.append(tuple(int(on[edges[r]:edges[r + 1]].sum()) for r in range(world)))
    return rows


@pytest.mark.parametrize("ctrl", CTRLS)
@pytest.mark.parametrize("n,world", [(130, 2), (3001, 3)])
def test_every_tick_needs_the_allreduce(n, world, ctrl):
    from mdr_amd.environment import shard_range

    for r in range(world):  # (the product's split is the one counted here)
        lo, cnt = shard_range(n, r, world)
        assert (lo, lo + cnt) == (r * n // world, (r + 1) * n // world)
    rows = rank_counts(n, world, ctrl)
    print(f"n={n} world={world} {ctrl}: min rank count {min(min(r) for r in rows)}, "
          f"max {max(max(r) for r in rows)}, distinct tuples {len(set(rows))}")
    assert all(sum(1 for v in r if v > 0) >= 2 for r in rows)
    assert len(set(rows)) >= 50
