"""The NumPy restatement of the device random controller (tests/philox_np.py) reproduces the
published Philox4x32-10 known-answer vectors (Random123 kat_vectors), and its bit layout matches
mdr_device.h (one 64-bit word per 64-house group and tick)."""
import numpy as np

import philox_np as P

KAT = [  # (counter x4, key x2) -> output x4
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def test_philox_known_answers():
    for ctr, key, want in KAT:
        got = P.philox4x32_10(*ctr, *key)
        assert [int(x) for x in got] == list(want)


def test_random_action_bit_layout():
    seed, tick = 1234, 7
    gids = np.arange(0, 256, dtype=np.uint64)
    a = P.random_actions(seed, gids, tick)
    for g in range(4):
        lo, hi = P.philox_words(seed, np.uint64(g), np.uint64(tick))
        word = int(lo) | (int(hi) << 32)
        bits = np.array([(word >> b) & 1 for b in range(64)], bool)
        np.testing.assert_array_equal(a[64 * g:64 * (g + 1)], bits)
    # a shard offset does not change a house's action (keyed by global id)
    np.testing.assert_array_equal(P.random_actions(seed, gids[100:], tick), a[100:])


def test_u01f_range_grid_and_vectorisation():
    """u01f (the actor's sampling uniform, mdr_actor.hip philox_u01f): float32 values in [0, 1) that
    are exact multiples of 2^-24, from word 0 of the documented counter / key; the array form equals
    the scalar form house by house."""
    seed, tick = 0x1234_5678_9ABC_DEF0, (5 << 32) | 77
    gids = np.concatenate([np.arange(0, 4099, dtype=np.uint64),
                           np.array([2**32 - 1, 2**32, 2**40 + 3], np.uint64)])  # (the gid's high word too)
    u = P.u01f(seed, gids, tick)
    assert u.dtype == np.float32 and u.shape == gids.shape
    assert u.min() >= 0.0 and u.max() < 1.0
    k = u.astype(np.float64) * 2.0 ** 24
    np.testing.assert_array_equal(k, np.floor(k))  # exact multiples of 2^-24
    assert 0.45 < u.mean() < 0.55
    # the counter and key as documented, through the known-answer-checked block function
    for i in (0, 1, 63, 64, 4098, 4099, 4100, 4101):
        g = int(gids[i])
        c0 = int(P.philox4x32_10(g & 0xFFFFFFFF, g >> 32, tick & 0xFFFFFFFF, (tick >> 32) ^ 0xAC7,
                                 (seed & 0xFFFFFFFF) ^ 0x3C6EF372, seed >> 32)[0])
        assert float(u[i]) == (c0 >> 8) / 2.0 ** 24
        assert P.u01f(seed, np.uint64(g), tick) == u[i]  # scalar == vector element
    # a shard offset does not change a house's uniform (keyed by global id); the tick does
    np.testing.assert_array_equal(P.u01f(seed, gids[100:], tick), u[100:])
    assert np.mean(P.u01f(seed, gids, tick + 1) == u) < 0.01


def test_random_actions_are_fair():
    a = P.random_actions(99, np.arange(1 << 18, dtype=np.uint64), 3)
    assert abs(a.mean() - 0.5) < 4 * 0.5 / np.sqrt(a.size)
