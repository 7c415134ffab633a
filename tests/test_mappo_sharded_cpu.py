"""CPU-side checks of sharded MA-PPO training: the cross-shard discounted returns, the minibatch
ownership arithmetic and the bindings of the sharded snapshot entry points (no GPU calls here)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import golden_util as gu  # noqa: F401  (sys.path set by conftest)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mdr_snapshot_sharded", "mdr_actor_rollout_sharded_snap", "mdr_obs_gather_sharded")
SHAPES = [(7, 1), (7, 2), (7, 3), (101, 1), (101, 2), (101, 3), (3001, 1), (3001, 2), (3001, 3)]


def _oracle_returns(reward, done, gamma):
    """The reference's reversed loop (mappo.py:135-140) over the concatenated buffer, float64."""
    T, N = reward.shape
    r = reward.reshape(-1)
    d = np.repeat(done, N)
    g = np.empty_like(r)
    nxt = 0.0
    for i in range(r.size - 1, -1, -1):
        nxt = r[i] + gamma * (0.0 if d[i] else nxt)
        g[i] = nxt
    return g.reshape(T, N)


def _done_flags(T, which):
    d = np.zeros(T, bool)
    if which == "last":
        d[-1] = True
    elif which == "middle":
        d[T // 2] = True
    return d


@pytest.mark.parametrize("gamma", [0.99, 0.5])
@pytest.mark.parametrize("which", ["none", "last", "middle"])
@pytest.mark.parametrize("T", [1, 6, 40])
@pytest.mark.parametrize("n,world", SHAPES)
def test_cross_shard_returns(n, world, T, which, gamma):
    """Every rank's rows of sharded_reference_returns, concatenated along the house axis, are the
    float64 reversed loop over the whole buffer to relative 1e-12 (rewards <= 0, so no cancellation;
    gamma = 0.99 leaves a window of a few thousand terms at 2^-53 each, about 4e-13)."""
    import torch

    from mdr_amd.environment import shard_range
    from mdr_amd.mappo import discounted_returns, sharded_reference_returns

    rng = np.random.RandomState(1000 * T + n + world)
    reward = -rng.uniform(0.0, 3.0, (T, n))  # r = -(...) <= 0 by construction
    assert (reward <= 0).all()
    done = _done_flags(T, which)
    want = _oracle_returns(reward, done, gamma)
    ranges = [shard_range(n, r, world) for r in range(world)]
    assert sum(nl for _, nl in ranges) == n and (world == 1 or n % world == 0 or len({nl for _, nl in ranges}) > 1)
    d_t = torch.from_numpy(done.astype(np.float64))
    local = [torch.from_numpy(np.ascontiguousarray(reward[:, lo:lo + nl])) for lo, nl in ranges]

    # the fake all-gather: every rank's (A, C) rows, formed by running the ranks one after another —
    # a first pass records what each rank contributes, the second pass hands all of them to each
    contributed = [None] * world

    def recorder(r):
        def ag(mine):
            contributed[r] = mine.clone()
            return torch.stack([mine] * world)  # (placeholder: this pass's result is discarded)
        return ag

    for r in range(world):
        sharded_reference_returns(local[r], d_t, gamma, r, world, recorder(r))
    everyone = torch.stack(contributed)
    assert everyone.shape == (world, T, 2) and everyone.dtype == torch.float64
    got = [sharded_reference_returns(local[r], d_t, gamma, r, world, lambda mine: everyone).numpy()
           for r in range(world)]
    got = np.concatenate(got, axis=1)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    if world == 1:
        flat = discounted_returns(torch.from_numpy(reward.reshape(-1)),
                                  torch.from_numpy(np.repeat(done, n).astype(np.float64)), gamma).numpy()
        np.testing.assert_allclose(got.reshape(-1), flat, rtol=1e-12, atol=0)


@pytest.mark.parametrize("n,world", SHAPES)
def test_minibatch_ownership(n, world):
    """shard_owner maps a global transition index to the rank whose shard_range holds its house and
    to tick * n_local + local house there; in every chunk of a permutation every position is owned
    by exactly one rank."""
    import torch

    from mdr_amd.environment import shard_range
    from mdr_amd.mappo import shard_owner

    T, batch = 6, 64
    L = T * n
    ranges = [shard_range(n, r, world) for r in range(world)]
    perm = torch.from_numpy(np.random.RandomState(n + world).permutation(L))
    covered = np.zeros(L, np.int64)
    for k in range(0, L, batch):
        idx = perm[k:k + batch]
        rank, loc = shard_owner(idx, n, world)
        owners = np.zeros(idx.numel(), np.int64)
        for r, (lo, nl) in enumerate(ranges):
            own = (rank == r).numpy()
            owners += own
            tick, house = idx.numpy()[own] // n, idx.numpy()[own] % n
            assert ((house >= lo) & (house < lo + nl)).all()
            np.testing.assert_array_equal(loc.numpy()[own], tick * nl + (house - lo))
            assert ((loc.numpy()[own] >= 0) & (loc.numpy()[own] < T * nl)).all()
        assert (owners == 1).all()
        covered[idx.numpy()] += 1
    assert (covered == 1).all()
    # numpy indices give the same answer
    rank_np, loc_np = shard_owner(perm.numpy(), n, world)
    rank_t, loc_t = shard_owner(perm, n, world)
    np.testing.assert_array_equal(rank_np, rank_t.numpy())
    np.testing.assert_array_equal(loc_np, loc_t.numpy())


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
    # the new rollout takes mdr_actor_rollout_sharded's arguments, then snap, halo and row0 before the stream
    base = _lib.SIGNATURES["mdr_actor_rollout_sharded"][1]
    assert _lib.SIGNATURES["mdr_actor_rollout_sharded_snap"][1] == base[:-1] + [
        C.POINTER(_lib.mdr_snap), C.POINTER(_lib.mdr_snap_halo), C.c_int, C.c_void_p]
    # the existing entry points keep their signatures and mdr_snap its size
    assert len(_lib.SIGNATURES["mdr_snapshot"][1]) == 6 and len(_lib.SIGNATURES["mdr_obs_gather"][1]) == 8
    assert C.sizeof(_lib.mdr_snap) == 48


def test_mdr_snap_halo_size_is_the_headers():
    """mdr.h's mdr_snap_halo: int32 struct_bytes, int32 cap_rows, int64 row_stride, one pointer; the
    library accepts exactly the binding's sizeof as struct_bytes (its own size check)."""
    from mdr_amd import _lib

    lib = _lib.load()
    assert C.sizeof(_lib.mdr_snap_halo) == 24
    assert [f[0] for f in _lib.mdr_snap_halo._fields_] == ["struct_bytes", "cap_rows", "row_stride", "rows"]
    assert _lib.mdr_snap_halo not in _lib.ABI_STRUCTS
    snap = _lib.mdr_snap(C.sizeof(_lib.mdr_snap), 4, 8, 0, 0, 0, 0)
    sc, spec = _lib.mdr_obs_scalars(), _lib.mdr_obs_spec()

    def calls(halo):
        yield lib.mdr_snapshot_sharded(None, C.byref(spec), C.byref(snap), C.byref(halo), 0, C.byref(sc), None, None,
                                       None)
        yield lib.mdr_obs_gather_sharded(None, C.byref(spec), C.byref(snap), C.byref(halo), 0, None, 0, None, None)
        yield lib.mdr_actor_rollout_sharded_snap(None, 1, None, None, C.byref(spec), None, 0, None, 0, None, 0, None,
                                                 C.byref(snap), C.byref(halo), 0, None)

    good = _lib.mdr_snap_halo(C.sizeof(_lib.mdr_snap_halo), 4, 110, 0)
    it = calls(good)
    for _ in range(3):
        lib.mdr_create(None, None)  # (another message in mdr_last_error first)
        assert next(it) == -1  # (the NULL context) ...
        assert b"struct_bytes" not in lib.mdr_last_error()  # ... not the struct's size
    for bad in (0, C.sizeof(_lib.mdr_snap_halo) - 8, C.sizeof(_lib.mdr_snap_halo) + 8):
        it = calls(_lib.mdr_snap_halo(bad, 4, 110, 0))
        for _ in range(3):
            lib.mdr_create(None, None)
            assert next(it) == -1
            assert b"mdr_snap_halo.struct_bytes" in lib.mdr_last_error()
    # and mdr_snap's check still comes first
    it = calls(good)
    snap.struct_bytes = 40
    for _ in range(3):
        assert next(it) == -1
        assert b"mdr_snap.struct_bytes" in lib.mdr_last_error()


def test_null_arguments():
    from mdr_amd import _lib

    lib = _lib.load()
    assert lib.mdr_snapshot_sharded(None, None, None, None, 0, None, None, None, None) == -1
    assert lib.mdr_obs_gather_sharded(None, None, None, None, 0, None, 0, None, None) == -1
    assert lib.mdr_actor_rollout_sharded_snap(None, 1, None, None, None, None, 0, None, 0, None, 0, None, None, None, 0,
                                              None) == -1
