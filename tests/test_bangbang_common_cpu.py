"""The == comparisons of tests/test_bangbang_common_gpu.py discriminate the summation order of the
cluster's mean penalty: under the oracle, at every shape of its window-against-loop test with
n >= 129 and both controllers,

  * houses with pen_i > 0 are never fewer than a quarter of n on any tick (a sum of few non-zero
    terms has the same bits in most orders), and
  * the order of the one-tick path (k_step_t's block partial + k_pen_reduce) and the order of the
    open-loop window (k_step_window<..., COMMON> + k_win_pen_reduce over per-wave partials) give
    different bits on at least one tick.

So a closed-loop window that added the terms in k_step_window's order would fail the GPU test.  Also:
the closed-loop window's procedure (k_step_closed<..., COMMON>) equals the one-tick order bit for
bit on random ragged tiles.

The three orders are restated here in numpy from csrc/mdr_kernels.hip; every addition is one IEEE
double addition, as on the device (no fused or reassociated arithmetic: -ffp-contract=off).
"""
import random

import numpy as np
import pytest

import golden_util as gu
from bangbang_inputs import CTRLS, SEED, SHAPES, overrides
from oracle import env_np as O

LANES = np.arange(64)


def _butterfly(v, offsets):
    """v [..., 64] += __shfl_xor(v, off) for off in offsets."""
    for off in offsets:
        v = v + v[..., LANES ^ off]
    return v


def _tiles(terms):
    """terms [n] -> ([blocks, 4, 128] padded with 0.0, valid mask): a block holds 4 wave tiles of
    128 consecutive houses (k_step_t's grid and k_step_window's / k_step_closed's alike)."""
    n = terms.shape[0]
    nb = -(-n // 512)
    x = np.zeros(nb * 512)
    x[:n] = terms
    v = np.zeros(nb * 512, bool)
    v[:n] = True
    return x.reshape(nb, 4, 128), v.reshape(nb, 4, 128)


def wave_sum_per_tick(x, v):
    """k_step_t: lane L holds houses 2L, 2L + 1; sacc = 0.0, += each valid term; xor 32 .. 1; lane 0."""
    s = np.zeros(x.shape[:-1] + (64,))
    for h in range(2):
        s = np.where(v[..., h::2], s + x[..., h::2], s)
    return _butterfly(s, (32, 16, 8, 4, 2, 1))[..., 0]


def wave_sum_open_window(x, v):
    """k_step_window<..., COMMON>: lane l holds houses l, 64 + l; the same accumulate and butterfly."""
    s = np.zeros(x.shape[:-1] + (64,))
    for h in range(2):
        s = np.where(v[..., 64 * h:64 * h + 64], s + x[..., 64 * h:64 * h + 64], s)
    return _butterfly(s, (32, 16, 8, 4, 2, 1))[..., 0]


def wave_sum_closed_window(x, v):
    """k_step_closed<..., COMMON>: per slot h, u_h = a_h + (a_h of lane l ^ 1), a house the tile does
    not hold being 0.0; v = u_0 + u_1; xor 32 .. 2; lane 0."""
    u = []
    for h in range(2):
        a = np.where(v[..., 64 * h:64 * h + 64], x[..., 64 * h:64 * h + 64], 0.0)
        u.append(a + a[..., LANES ^ 1])
    return _butterfly(u[0] + u[1], (32, 16, 8, 4, 2))[..., 0]


def _strided_then_tree(part):
    """k_pen_reduce / k_win_pen_reduce: thread t adds entries t, t + 256, ... from 0.0, then the
    256-wide LDS tree."""
    m = part.shape[0]
    pad = np.zeros(-(-m // 256) * 256)
    pad[:m] = part  # (a thread's missing entry: no addition; + 0.0 to a sum >= +0 is the same bits)
    ss = np.zeros(256)
    for row in pad.reshape(-1, 256):
        ss = ss + row
    w = 128
    while w > 0:
        ss[:w] = ss[:w] + ss[w:2 * w]
        w //= 2
    return ss[0]


def block_serial(ws):
    """thread 0 of a block: its 4 waves added in index order from 0.0."""
    bs = np.zeros(ws.shape[0])
    for r in range(4):
        bs = bs + ws[:, r]
    return bs


def mean_per_tick(pen, N):
    x, v = _tiles(pen / N)
    return _strided_then_tree(block_serial(wave_sum_per_tick(x, v)))


def mean_open_window(pen, N):
    x, v = _tiles(pen / N)
    return _strided_then_tree(wave_sum_open_window(x, v).reshape(-1))  # (per-wave partials, tiles padded to blocks)


def mean_closed_window(pen, N):
    x, v = _tiles(pen / N)
    return _strided_then_tree(block_serial(wave_sum_closed_window(x, v)))


def oracle_penalties(n, ticks, ctrl):
    """[ticks, n] per-house temperature penalties of the GPU test's first rollout under the oracle."""
    props = gu.props_from_overrides(overrides(n))
    ora = O.OracleEnv(props, random.Random(SEED))
    db = props.cluster_prop.house_prop.deadband
    tg = ora.pop["target"]
    rows = []
    for _ in range(ticks):
        a = O.bangbang(ora.T, tg) if ctrl == "bangbang" else O.deadband_bangbang(ora.T, tg, db, ora.on)
        ora.step(a)
        rows.append(np.asarray(O.deadband_l2(tg, db, ora.T), np.float64).copy())
    return np.stack(rows)


@pytest.mark.parametrize("ctrl", CTRLS)
@pytest.mark.parametrize("n,ticks,win", [s for s in SHAPES if s[0] >= 129])
def test_inputs_discriminate_the_order(n, ticks, win, ctrl):
    pen = oracle_penalties(n, ticks, ctrl)
    assert np.all(pen >= 0.0) and np.all(np.isfinite(pen))
    positive = (pen > 0.0).sum(axis=1)
    differ = 0
    for row in pen:
        a, b, c = mean_per_tick(row, float(n)), mean_open_window(row, float(n)), mean_closed_window(row, float(n))
        assert a.tobytes() == c.tobytes()  # the closed-loop window's order is the one-tick order
        differ += a.tobytes() != b.tobytes()
    print(f"n={n} ticks={ticks} {ctrl}: pen > 0 on {positive.min()}..{positive.max()} houses, "
          f"{differ} ticks where the two orders differ in bits")
    assert positive.min() * 4 >= n
    assert differ >= 1


def test_closed_window_order_is_the_per_tick_order_on_ragged_tiles():
    """20,000 random ragged tiles (1 .. 128 houses, a third of the penalties zero, random N): the
    closed-loop window's wave sum has the one-tick wave sum's bits."""
    rs = np.random.RandomState(13)
    m = 20000
    pen = rs.uniform(0.0, 9.0, (m, 128)) ** 2 * (rs.uniform(size=(m, 128)) > 1.0 / 3.0)
    N = rs.randint(1, 1 << 20, (m, 1)).astype(np.float64)
    held = rs.randint(1, 129, (m, 1))
    v = np.arange(128)[None, :] < held
    x = np.where(v, pen / N, 7.0)  # (a term the tile does not hold is never read)
    a, c = wave_sum_per_tick(x, v), wave_sum_closed_window(x, v)
    assert a.tobytes() == c.tobytes()
    b = wave_sum_open_window(x, v)
    assert (a != b).any()  # (and the open-loop window's order is a different one)
