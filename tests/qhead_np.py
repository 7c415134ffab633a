"""NumPy restatement of the actor's Q head (csrc/mdr_actor.hip actor_head / philox_word) — test
infrastructure for tests/test_dqn_cpu.py and tests/test_qhead_gpu.py.

The house's Philox block is the one ``philox_np.u01f`` restates (the softmax head's sampling
uniform); the Q head reads word x of it twice: explore iff float32(x >> 8) * 2^-24 < epsilon, random
action = bit 0 of x (below the 24 bits of the uniform, so the two are independent).  Otherwise the
action is torch.argmax over (q0, q1): 1 iff q1 > q0 or (q1 is NaN and q0 is not) — a tie gives 0, a
NaN counts as the maximum and the first one wins.
"""
from __future__ import annotations

import numpy as np

import philox_np as PH

_MASK = np.uint64(0xFFFFFFFF)

# The Q rows' tolerance where the project has no number for logits (tests/test_qhead_gpu.py):
# max |q - q_torch| / max(1, max |q|) against torch fp32, 4 x the largest value measured over that
# file's cases on an MI355X (bf16x3 9.8e-5, bf16 2.67e-2)
Q_RTOL = {"bf16x3": 4 * 9.8e-5, "bf16": 4 * 2.67e-2}
# The x3-scaled Q-net of the torch-argmax check: the smallest torch seed for which torch alone, on the
# oracle's obs rows, has no house with |q1 - q0| inside twice the widest (bf16) tolerance at 1, 37, 300
# and 4,099 houses (tests/test_dqn_cpu.py test_argmax_net_keeps_torch_outside_the_band asserts it;
# seed 3, the other tests' net, has 24 % and 58 % of the houses inside it at 37 and 300)
ARGMAX_SEED = 2
ARGMAX_SIZES = (1, 37, 300, 4099)


def actor_word(seed: int, gid, tick) -> np.ndarray:
    """Word x (uint32) of the actor's Philox block of global house ``gid`` at tick ``tick``: counter
    (gid lo, gid hi, tick lo, tick hi ^ 0xAC7), key (seed lo ^ 0x3C6EF372, seed hi)."""
    gid = np.asarray(gid, np.uint64)
    tick = np.broadcast_to(np.asarray(tick, np.uint64), gid.shape)
    s = np.uint64(seed & 0xFFFFFFFFFFFFFFFF)
    c0 = PH.philox4x32_10(gid & _MASK, gid >> np.uint64(32), tick & _MASK,
                          (tick >> np.uint64(32)) ^ np.uint64(0xAC7),
                          (s & _MASK) ^ np.uint64(0x3C6EF372), s >> np.uint64(32))[0]
    return c0.astype(np.uint32)


def word_u01f(word) -> np.ndarray:
    return (np.asarray(word, np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def greedy(q) -> np.ndarray:
    """torch.argmax over the two columns of ``q`` [n, 2] (uint8)."""
    q = np.asarray(q, np.float32)
    q0, q1 = q[:, 0], q[:, 1]
    with np.errstate(invalid="ignore"):
        return ((q1 > q0) | (np.isnan(q1) & ~np.isnan(q0))).astype(np.uint8)


def explore(word, eps: float) -> np.ndarray:
    return word_u01f(word) < np.float32(eps)


def decide(q, word, eps: float) -> np.ndarray:
    """The Q head's action (uint8) from its Q rows, the houses' Philox words and epsilon."""
    word = np.asarray(word, np.uint32)
    return np.where(explore(word, eps), (word & np.uint32(1)).astype(np.uint8), greedy(q)).astype(np.uint8)
