"""CPU-side checks of the replay-snapshot entry points (mdr_snapshot, mdr_actor_rollout_snap,
mdr_obs_gather): they are declared, bound and exported, and refuse bad arguments before any HIP
call (no GPU calls here)."""
import ctypes as C
import os
import re

import golden_util as gu  # noqa: F401  (sys.path set by conftest)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mdr_snapshot", "mdr_actor_rollout_snap", "mdr_obs_gather")


def test_symbols_declared_bound_and_exported():
    from mdr_amd import _lib

    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "mdr.h")) as f:
        src = f.read()
    declared = set(re.findall(r"^int\s+(mdr_\w+)\s*\(", src, re.M))
    for s in NEW:
        assert s in declared and s in _lib.SIGNATURES and hasattr(lib, s), s
    # the C prototype and the ctypes signature take the same number of arguments
    for s in NEW:
        proto = re.search(r"^int\s+" + s + r"\s*\(([^;]*)\)\s*;", src, re.M | re.S).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[s][1]), s


def test_mdr_snap_layout():
    """mdr.h's mdr_snap: int32 struct_bytes, int32 cap_rows, int64 row_stride, four pointers."""
    from mdr_amd import _lib

    assert C.sizeof(_lib.mdr_snap) == 48
    assert [f[0] for f in _lib.mdr_snap._fields_] == ["struct_bytes", "cap_rows", "row_stride", "t_air", "t_mass",
                                                       "hvac", "scalars"]
    assert _lib.mdr_snap.row_stride.offset == 8 and _lib.mdr_snap.scalars.offset == 40
    assert _lib.mdr_snap not in _lib.ABI_STRUCTS  # (struct_bytes is this struct's own check)


def test_null_arguments():
    from mdr_amd import _lib

    lib = _lib.load()
    assert lib.mdr_snapshot(None, None, 0, None, None, None) == -1
    assert lib.mdr_actor_rollout_snap(None, 1, None, None, None, None, 0, None, 0, None, 0, None, 1, None, 0,
                                      None) == -1
    assert lib.mdr_obs_gather(None, None, None, 0, None, 0, None, None) == -1
    # a well-formed snap does not make a NULL context acceptable
    snap = _lib.mdr_snap(C.sizeof(_lib.mdr_snap), 4, 8, 0, 0, 0, 0)
    sc = _lib.mdr_obs_scalars()
    spec = _lib.mdr_obs_spec()
    assert lib.mdr_snapshot(None, C.byref(snap), 0, C.byref(sc), None, None) == -1
    assert lib.mdr_obs_gather(None, C.byref(spec), C.byref(snap), 0, None, 0, None, None) == -1
    assert lib.mdr_actor_rollout_snap(None, 1, None, None, C.byref(spec), None, 0, None, 0, None, 0, None, 1,
                                      C.byref(snap), 0, None) == -1


def test_wrong_struct_bytes_names_the_struct():
    from mdr_amd import _lib

    lib = _lib.load()
    sc = _lib.mdr_obs_scalars()
    spec = _lib.mdr_obs_spec()
    for bad in (0, C.sizeof(_lib.mdr_snap) - 8, C.sizeof(_lib.mdr_snap) + 8):
        snap = _lib.mdr_snap(bad, 4, 8, 0, 0, 0, 0)
        lib.mdr_create(None, None)  # (another message in mdr_last_error first)
        assert b"mdr_snap" not in lib.mdr_last_error()
        assert lib.mdr_snapshot(None, C.byref(snap), 0, C.byref(sc), None, None) == -1
        assert b"mdr_snap.struct_bytes" in lib.mdr_last_error()
        lib.mdr_create(None, None)
        assert lib.mdr_obs_gather(None, C.byref(spec), C.byref(snap), 0, None, 0, None, None) == -1
        assert b"mdr_snap.struct_bytes" in lib.mdr_last_error()
        lib.mdr_create(None, None)
        assert lib.mdr_actor_rollout_snap(None, 1, None, None, C.byref(spec), None, 0, None, 0, None, 0, None, 1,
                                          C.byref(snap), 0, None) == -1
        assert b"mdr_snap.struct_bytes" in lib.mdr_last_error()


def test_store_bytes_per_house_tick():
    from mdr_amd.replay import RolloutStore

    assert RolloutStore.nbytes_per_house_tick == 33
