"""Stats rows of a house-sharded cluster, without a GPU: the new C entry points are
declared, bound and exported and refuse bad arguments before any HIP call; the exchange's arithmetic
("zero-padded sum, then rank-order combine", tests/stats_sharded_np.py) gives the same bits for every
order of the collective; and the inputs of tests/test_stats_sharded_gpu.py cannot hide a wrong combine.
"""
import ctypes as C
import itertools
import os
import random
import re

import numpy as np
import pytest

import golden_util as gu
import stats_sharded_np as X
from bangbang_inputs import CTRLS, SEED, overrides
from oracle import env_np as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mdr_stats_exchange_bytes", "mdr_stats_exchange_ranks", "mdr_stats_exchange_buffer", "mdr_tick_stats_sharded",
       "mdr_stats_rows_combine", "mdr_stats_rows_exchange", "mdr_rollout_sharded_stats",
       "mdr_rollout_sharded_stats_path", "mdr_actor_rollout_sharded_stats")
TICKS = 70


def _prototypes():
    with open(os.path.join(ROOT, "include", "mdr.h")) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"^(?:int|size_t)\s+(mdr_\w+)\s*\(([^;]*)\)\s*;", src, re.M)}


def test_new_symbols_declared_bound_exported():
    from mdr_amd import _lib

    lib = _lib.load()
    protos = _prototypes()
    for name in NEW:
        assert name in protos, f"{name} not declared in include/mdr.h"
        assert name in _lib.SIGNATURES, f"{name} not in _lib.SIGNATURES"
        assert hasattr(lib, name), f"{name} not exported"
        assert len(protos[name].split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert _lib.ABI_VERSION == 5 and lib.mdr_abi_version() == 5  # (no struct changed)


def test_exchange_bytes():
    from mdr_amd import _lib

    f = _lib.load().mdr_stats_exchange_bytes
    assert f(1, 1) == 128
    assert f(2, 70) == 2 * 70 * 16 * 8
    assert f(3, 37) == 3 * 37 * 16 * 8
    assert f(8, 2000) == 8 * 2000 * 128
    for world, m in ((0, 4), (4, 0), (-1, 4), (4, -1), (2 ** 31 - 1, 2 ** 31 - 1)):
        assert f(world, m) == 0, (world, m)


def _refused(rc, word):
    from mdr_amd import _lib

    with pytest.raises(_lib.MdrError, match=f"MDR_EARG.*{word}"):
        _lib.check(rc, "call")


def test_bad_arguments_refused_before_any_hip_call():
    """Every call here has a NULL context or an argument that is refused before the context is looked
    at, on a machine without a GPU: nothing can have reached HIP.  (`buf` is host memory that is never
    dereferenced.)"""
    from mdr_amd import _lib

    lib = _lib.load()
    buf = (C.c_double * 16)()
    p = C.addressof(buf)
    vp, n64 = C.c_void_p(), C.c_int64()
    _refused(lib.mdr_stats_exchange_ranks(None, 2, 0), "null ctx")
    _refused(lib.mdr_stats_exchange_buffer(None, 4, None, C.byref(n64)), "dev_ptr")
    _refused(lib.mdr_stats_exchange_buffer(None, 4, C.byref(vp), None), "count")
    _refused(lib.mdr_stats_exchange_buffer(None, 4, C.byref(vp), C.byref(n64)), "null ctx")
    _refused(lib.mdr_tick_stats_sharded(None, None, None, 0.0, 4, 4, None), "row outside")
    _refused(lib.mdr_tick_stats_sharded(None, None, None, 0.0, 4, -1, None), "row outside")
    _refused(lib.mdr_tick_stats_sharded(None, None, None, 0.0, 4, 3, None), "null ctx")
    _refused(lib.mdr_tick_stats_sharded(None, None, None, 0.0, 0, 0, None), "null ctx")
    for fn in (lib.mdr_stats_rows_combine, lib.mdr_stats_rows_exchange):
        # the row range answers first, whatever else is wrong with the call
        _refused(fn(None, 4, None, 3, 0, None), "stats_row0")
        _refused(fn(None, 4, p, 8, 5, None), "stats_row0")
        _refused(fn(None, 4, p, 8, -1, None), "stats_row0")
        _refused(fn(None, 4, None, 8, 4, None), "null stats")
        _refused(fn(None, 4, p, 8, 4, None), "null ctx")
    _refused(lib.mdr_rollout_sharded_stats_path(None, _lib.ACT_BANGBANG), "null ctx")
    # mdr_rollout_sharded_stats / mdr_actor_rollout_sharded_stats: the row range first, then the pointers
    _refused(lib.mdr_rollout_sharded_stats(None, 5, None, None, 0, _lib.ACT_BANGBANG, None, 0, None, p, 4, 0, None),
             "stats_row0")
    _refused(lib.mdr_rollout_sharded_stats(None, 5, None, None, 0, _lib.ACT_BANGBANG, None, 0, None, p, 8, 4, None),
             "stats_row0")
    _refused(lib.mdr_rollout_sharded_stats(None, 5, None, None, 0, _lib.ACT_BANGBANG, None, 0, None, p, 8, 3, None),
             "bad argument")
    _refused(lib.mdr_actor_rollout_sharded_stats(None, 5, None, None, None, None, 0, None, 0, None, 0, None, None, None,
                                                 0, p, 4, 0, None), "stats_row0")
    _refused(lib.mdr_actor_rollout_sharded_stats(None, 5, None, None, None, None, 0, None, 0, None, 0, None, None, None,
                                                 0, p, 8, 3, None), "bad argument")


@pytest.mark.parametrize("world", [1, 2, 3, 4])
def test_every_order_of_the_sum_gives_the_same_rows(world):
    """The zero-padded sum is exact: every permutation of the ranks' addends, chained or as a tree,
    leaves the same bits in the slab, so the rank-order combine behind it sees the same operands on
    every rank and under every collective.  A -0.0 partial arrives as +0.0 (== all the same)."""
    rs = np.random.RandomState(20 + world)
    m = 5
    parts = [rs.standard_normal((m, X.ROW)) * 10.0 ** rs.randint(-8, 9, (m, X.ROW)) for _ in range(world)]
    parts[0][0, 3] = -0.0
    parts[-1][1, 7] = 0.0
    first = None
    for order in itertools.permutations(range(world)):
        for slab in (X.allreduce_chain(parts, order), X.allreduce_tree(parts, order)):
            if first is None:
                first = slab
            assert slab.tobytes() == first.tobytes(), order
    for r in range(world):
        assert np.array_equal(first[r], parts[r])  # (==: -0.0 == +0.0)
    assert np.signbit(first[0][0, 3]) == (world == 1)  # (one rank: nothing is added to it)
    rows = [X.combine(first, r) for r in range(world)]
    for r in range(world):
        assert np.array_equal(rows[r][:, :X.N_STATS], rows[0][:, :X.N_STATS])
        assert np.array_equal(rows[r][:, X.S_POWER], parts[r][:, X.S_POWER])
        assert not rows[r][:, 13:].any()
    want = parts[0][:, :X.N_STATS].copy()
    for r in range(1, world):  # rank order, slot 2 by max
        nxt = want + parts[r][:, :X.N_STATS]
        nxt[:, X.S_MAX] = np.maximum(want[:, X.S_MAX], parts[r][:, X.S_MAX])
        want = nxt
    assert np.array_equal(rows[0][:, :X.N_STATS], want)


def _rank_terms(n, world, ctrl, ticks=TICKS):
    """Per tick under the oracle: each rank's max of T - target / N, whether it has a locked house,
    and the cluster's lowest temperature."""
    from mdr_amd.environment import shard_range

    props = gu.props_from_overrides(overrides(n))
    ora = O.OracleEnv(props, random.Random(SEED))
    db = props.cluster_prop.house_prop.deadband
    tg = ora.pop["target"]
    cuts = [shard_range(n, r, world) for r in range(world)]
    assert [lo for lo, _ in cuts] == [r * n // world for r in range(world)]
    mx, locked, tmin = [], [], []
    for _ in range(ticks):
        a = O.bangbang(ora.T, tg) if ctrl == "bangbang" else O.deadband_bangbang(ora.T, tg, db, ora.on)
        o, _ = ora.step(a)
        e = np.asarray(o["T"]) - tg / n
        lock = np.asarray(o["lock"], bool)
        mx.append([float(e[lo:lo + c].max()) for lo, c in cuts])
        locked.append([bool(lock[lo:lo + c].any()) for lo, c in cuts])
        tmin.append(min(float(np.min(o["T"])), float(np.min(o["Tm"])), float(np.min(tg))))
    return np.array(mx), np.array(locked), np.array(tmin)


OWNERS = {  # ticks (of the first 70) at which each rank owns the cluster's maximum of T - target / N
    (130, 2, "bangbang"): {1: 70},
    (130, 2, "deadband_bangbang"): {0: 70},
    (3001, 3, "bangbang"): {0: 15, 2: 55},
    (3001, 3, "deadband_bangbang"): {2: 70},
}


@pytest.mark.parametrize("ctrl", CTRLS)
@pytest.mark.parametrize("n,world", [(130, 2), (3001, 3)])
def test_inputs_show_a_wrong_combine(n, world, ctrl):
    mx, locked, tmin = _rank_terms(n, world, ctrl)
    owner = mx.argmax(axis=1)
    counts = {int(r): int((owner == r).sum()) for r in np.unique(owner)}
    print(f"n={n} world={world} {ctrl}: owners {counts}, min rank max {mx.min():.6f}, min T {tmin.min():.3f}")
    # the ranks' maxima are pairwise distinct and positive at every tick: a combine that SUMMED slot 2
    # gives more than the maximum, and one that took the wrong rank's gives another value
    assert (mx > 0).all()
    for t in range(TICKS):
        assert len(set(mx[t])) == world, t
    assert (mx.sum(axis=1) > mx.max(axis=1)).all()
    # every rank has a locked house at every tick: a combine that dropped a rank misses slot 10 (and,
    # all temperatures being positive, slots 5, 8 and 9) at every tick
    assert locked.all()
    assert (tmin > 0).all()  # (the sum slots' tolerance also uses it: sum |T| = sum T)
    assert counts == OWNERS[n, world, ctrl]


def test_max_owner_is_rank_0_in_one_case_and_another_rank_elsewhere():
    """A combine that took rank 0's maximum is seen where another rank owns it at every tick, and one
    that took the last rank's where rank 0 does."""
    assert any(set(v) == {0} for v in OWNERS.values())
    assert any(0 not in v for v in OWNERS.values())
    owners_not0 = [k for k, v in OWNERS.items() if any(r != 0 for r in v)]
    assert {k[:2] for k in owners_not0} == {(130, 2), (3001, 3)}  # (both shapes of the GPU test)
