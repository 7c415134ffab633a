"""CPU-side checks of the per-tick stats entry points (mdr_tick_stats, mdr_actor_rollout_stats):
they are declared, bound and exported, and refuse null and short arguments before any HIP call,
naming the argument in mdr_last_error (no GPU calls here)."""
import ctypes as C
import os
import re

import golden_util as gu  # noqa: F401  (sys.path set by conftest)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mdr_tick_stats", "mdr_actor_rollout_stats")


def test_symbols_declared_bound_and_exported():
    from mdr_amd import _lib

    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "mdr.h")) as f:
        src = f.read()
    declared = set(re.findall(r"^int\s+(mdr_\w+)\s*\(", src, re.M))
    for s in NEW:
        assert s in declared and s in _lib.SIGNATURES and hasattr(lib, s), s
        proto = re.search(r"^int\s+" + s + r"\s*\(([^;]*)\)\s*;", src, re.M | re.S).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[s][1]), s
    # the rollout with stats rows is mdr_actor_rollout_snap's arguments plus the rows before the stream
    snap_args = _lib.SIGNATURES["mdr_actor_rollout_snap"][1]
    assert _lib.SIGNATURES["mdr_actor_rollout_stats"][1] == snap_args[:-1] + [C.c_void_p, C.c_int64, C.c_int64,
                                                                              C.c_void_p]


def test_python_layer_exports():
    import inspect

    from mdr_amd import services
    from mdr_amd.actor import DeviceActor
    from mdr_amd.mappo import DeviceMAPPO
    from mdr_amd.shard import HipShard

    assert services.TICK_ROW == 16 and services.S_POWER == 12
    for name in ("rows", "clear", "begin_rows", "commit_rows", "host"):
        assert name == "rows" or callable(getattr(services.RolloutStats, name)), name
    assert callable(services.DeviceMetrics.update_rollout)
    assert "stats" in inspect.signature(DeviceActor.rollout).parameters
    assert "metrics" in inspect.signature(DeviceMAPPO.collect).parameters
    assert list(inspect.signature(DeviceMAPPO.evaluate).parameters)[1:] == ["n_ticks", "env", "return_actions"]
    assert callable(HipShard.tick_stats) and callable(HipShard.actor_rollout_stats)


def _rollout_stats(lib, ctx, n, spec, snap, stats, rows, row0):
    return lib.mdr_actor_rollout_stats(ctx, n, None, None, spec, None, 0, None, 0, None, 0, None, 1, snap, 0,
                                       stats, rows, row0, None)


def test_null_arguments_name_the_argument():
    from mdr_amd import _lib

    lib = _lib.load()
    out = (C.c_double * 16)()
    lib.mdr_create(None, None)  # (another message in mdr_last_error first)
    assert lib.mdr_tick_stats(None, None, None, 0.0, None, None) == -1
    assert b"mdr_tick_stats" in lib.mdr_last_error() and b"out16" in lib.mdr_last_error()
    assert lib.mdr_tick_stats(None, None, None, 0.0, out, None) == -1
    assert b"mdr_tick_stats" in lib.mdr_last_error() and b"ctx" in lib.mdr_last_error()
    assert list(out) == [0.0] * 16
    # the rollout: without stats rows it reports as the snapshot rollout does, with them under its own name
    spec = _lib.mdr_obs_spec()
    assert _rollout_stats(lib, None, 1, None, None, None, 0, 0) == -1
    assert b"mdr_actor_rollout: bad argument" in lib.mdr_last_error()
    assert _rollout_stats(lib, None, 1, C.byref(spec), None, out, 1, 0) == -1
    assert b"mdr_actor_rollout_stats: bad argument" in lib.mdr_last_error()
    snap = _lib.mdr_snap(0, 4, 8, 0, 0, 0, 0)
    assert _rollout_stats(lib, None, 1, C.byref(spec), C.byref(snap), out, 1, 0) == -1
    assert b"mdr_snap.struct_bytes" in lib.mdr_last_error()


def test_short_stats_rows_are_refused_first():
    """stats_row0 + n_ticks past stats_rows (or a negative row) is MDR_EARG whatever else is passed."""
    from mdr_amd import _lib

    lib = _lib.load()
    out = (C.c_double * 64)()  # 4 rows
    spec = _lib.mdr_obs_spec()
    for n, rows, row0 in ((2, 4, 3), (5, 4, 0), (1, 4, 4), (1, 4, -1), (1, -1, 0), (1, 0, 0),
                          (2, 2 ** 62, 2 ** 63 - 1)):
        lib.mdr_create(None, None)
        assert _rollout_stats(lib, None, n, C.byref(spec), None, out, rows, row0) == -1, (n, rows, row0)
        assert b"stats_row0" in lib.mdr_last_error(), (n, rows, row0)
    assert list(out) == [0.0] * 64
    # rows that fit leave the next check to answer
    assert _rollout_stats(lib, None, 2, C.byref(spec), None, out, 4, 2) == -1
    assert b"bad argument" in lib.mdr_last_error()
