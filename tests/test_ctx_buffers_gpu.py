"""The context's device buffers on their success path: every regrow a caller can drive is driven
once, and what the context computes afterwards is compared bit for bit with a context that never
regrew.  (What happens when an allocation FAILS cannot be shown on a GPU and is not tried here: that
is tests/devbuf_check.cpp, a counting allocator under the same owner type.)

257 houses (two window tiles, the second ragged, as tests/test_rollout_sequence_gpu.py), window 7.

Regrows other tests already drive and this one does not repeat: the sharded actor rollout's d_halo
and d_c5 (tests/test_distributed_gpu.py, first use), the second ON-mask set of the count-ahead
pipeline (d_onb2 / d_wah2, same file), the stats partials (tests/test_bangbang_stats_gpu.py,
tests/test_tick_stats_gpu.py, tests/test_greedy_stats_gpu.py)."""
import json
import random

import numpy as np
import pytest

import golden_util as gu
from bangbang_inputs import SEED, overrides

pytestmark = pytest.mark.gpu

N, WIN = 257, 7


@pytest.fixture(scope="module")
def torch_gpu():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _env(population="reference"):
    from mdr_amd.environment import Environment

    kw = {} if population == "reference" else {"population": population, "seed": SEED}
    env = Environment(gu.props_from_overrides(overrides(N, "individual_L2")), rng=random.Random(SEED), **kw)
    env.shard.set_rollout_window(WIN)
    return env


def _same_state(torch, a, b):
    for k in ("t_air", "t_mass", "hvac"):
        assert torch.equal(getattr(a.shard, k), getattr(b.shard, k)), k


def test_tick_buffers_regrow(torch_gpu):
    """40, 200, 40 ticks with cached graphs: the 200-tick call is past the 128 tick records the first
    call allocated, so the records and the obs scalars regrow and the first call's graph is dropped
    (it held the old addresses).  Rewards and state == the same calls launched directly on a twin."""
    torch = torch_gpu
    a, b = _env(), _env()
    rew40 = torch.empty((40, N), dtype=torch.float64, device="cuda")  # (the graph key: calls 1 and 3 share it)
    g = [a.shard.graph_info()]
    for k, n in enumerate((40, 200, 40)):
        ra = a.rollout(n, rewards=rew40 if n == 40 else None, use_graph=True)
        rb = b.rollout(n, use_graph=False)
        assert torch.equal(ra, rb), (k, n)
        g.append(a.shard.graph_info())
        assert g[-1]["guarded"] == g[-2]["guarded"] + 1, (k, g)  # (a capture each: the third one again)
    assert g[1]["rollout_graphs"] == 1 and g[2]["rollout_graphs"] == 1 and g[3]["rollout_graphs"] == 2, g
    _same_state(torch, a, b)


# (case id, MDR_OPT_ACTOR_GENERIC, hidden layers of the narrow and of the wide net)
ACTOR_CASES = [("fused", 0, (16, 16), (100, 100)),
               # the option selects k_actor's generic-layout form, still the fused kernel ...
               ("generic", 1, (16, 16), (100, 100)),
               # ... so the layer chain, whose row buffer d_chain grows with the widest layer, gets a
               # three-layer net, which the fused kernel does not take
               ("chain", 1, (16, 16, 16), (100, 100, 100))]


@pytest.mark.parametrize("case,generic,narrow_l,wide_l", ACTOR_CASES, ids=[c[0] for c in ACTOR_CASES])
def test_actor_buffers_regrow(torch_gpu, case, generic, narrow_l, wide_l):
    """A narrow net, an actor rollout with a graph, then a wider net in the same context: the raw
    weights and the packed image (fused) or the layer chain's rows (chain) regrow and the actor
    graphs are dropped.  The wide net's rollout == a twin's that only ever loaded it."""
    torch = torch_gpu
    from mdr_amd.actor import DeviceActor

    T = 5
    a, b = _env(), _env()
    for e in (a, b):
        e.shard.set_option("actor_generic", generic)
    F = a.obs_spec().n_feat
    m = a.obs_tensor().abs().amax(0).double().cpu().numpy()
    narrow = gu.calibrated_actor(F, m, seed=2, layers=narrow_l).to("cuda")
    wide = gu.calibrated_actor(F, m, seed=3, layers=wide_l).to("cuda")
    da = DeviceActor(a, narrow)
    assert da.fused() == (case != "chain")
    acts0 = torch.empty((T, N), dtype=torch.uint8, device="cuda")
    da.rollout(T, actions=acts0)
    assert a.shard.graph_info()["actor_graphs"] == 1
    da.actor = wide  # (the same DeviceActor: a new one's set_option would drop the graphs by itself)
    da.load_weights()
    assert a.shard.graph_info()["actor_graphs"] == 0
    for t in range(T):  # the twin reaches the same state without ever loading the narrow net
        b.step_tensor(acts0[t])
    _same_state(torch, a, b)
    db = DeviceActor(b, wide)
    out = []
    for d in (da, db):
        rew = torch.empty((T, N), dtype=torch.float64, device="cuda")
        acts = torch.empty((T, N), dtype=torch.uint8, device="cuda")
        probs = torch.empty((T, N), dtype=torch.float32, device="cuda")
        d.rollout(T, rewards=rew, actions=acts, probs=probs)
        out.append((acts, probs, rew))
    for x, y, name in zip(out[0], out[1], ("actions", "probs", "rewards")):
        assert torch.equal(x, y), name
    assert a.shard.graph_info()["actor_graphs"] == 1
    _same_state(torch, a, b)


def test_interp_table_regrow(torch_gpu):
    """mdr_interp_load with a small table (the last axis cut to two points), then the whole one:
    mdr_interp_values == a fresh context's that loaded only the whole table."""
    torch = torch_gpu
    d = gu.load("interp.npz")
    with open(gu.path("interp_parameters_dict.json")) as f:
        params = json.load(f)
    grids = [np.asarray(params[str(k)], np.float64) for k in d["keys"]]
    table = np.load(gu.interp_table_path()).reshape([len(g) for g in grids])
    cfg = (1.0, 1.0, 1.0, 1.0)
    a, b = _env("synthetic"), _env("synthetic")
    a.shard.interp_load(grids[:-1] + [grids[-1][:2]], np.ascontiguousarray(table[..., :2]), cfg)
    ids = torch.arange(N, dtype=torch.int64, device="cuda")
    small = torch.empty(N, dtype=torch.float64, device="cuda")
    a.shard.interp_values(ids, 31.3, 51234.0, 200.0, small)
    vals = []
    for e in (a, b):
        e.shard.interp_load(grids, table, cfg)
        v = torch.empty(N, dtype=torch.float64, device="cuda")
        e.shard.interp_values(ids, 31.3, 51234.0, 200.0, v)
        vals.append(v)
    assert torch.equal(vals[0], vals[1])
    assert bool(torch.isfinite(vals[0]).all()) and bool(torch.isfinite(small).all())


def test_greedy_scratch_lifetimes(torch_gpu):
    """The greedy scratch and the fused tick's: a default-form greedy_rollout, then three contexts in
    turn that run the fused form (MDR_OPT_GQ_FUSED) with the phase stamps on, then off, and are
    destroyed.  Every call returns MDR_OK (the wrappers raise otherwise) and the fused actions == the
    default form's."""
    torch = torch_gpu
    from mdr_amd import _lib as L

    T = 8
    ref = _env("synthetic")
    want = torch.empty((T, N), dtype=torch.uint8, device="cuda")
    for h in (0, T // 2):
        ref.greedy_rollout(T // 2, actions=want[h:h + T // 2])
    for _ in range(3):
        e = _env("synthetic")
        sh = e.shard
        sh.set_option("gq_fused", 1)
        got = torch.empty((T, N), dtype=torch.uint8, device="cuda")
        for h, on in ((0, 1), (T // 2, 0)):
            L.check(sh.lib.mdr_greedy_fused_stamps(sh.ctx, on, None), "mdr_greedy_fused_stamps")
            e.greedy_rollout(T // 2, actions=got[h:h + T // 2])
        assert torch.equal(got, want)
        assert sh.greedy_fused_diag()["calls"] == T
        torch.cuda.synchronize()
        sh.close()
