"""The stats row of one cluster and tick in k_batch_eval's documented summation order, in NumPy; shared by
tests/test_env_batch_eval_gpu.py (the batch's rows are == to it) and tests/test_env_batch_eval_cpu.py
(the order is deterministic and is not np.sum's).

Order (include/mdr.h, mdr_batch_rollout_eval): wave w, lane l owns houses 128 w + 2 l and 128 w + 2 l + 1;
a lane starts every slot at 0.0 and adds its first house, then its second (houses past the cluster add
nothing); the 64 lanes of a wave combine by the xor butterfly 32, 16, ..., 1 as v = v + v[l ^ off] (slot 2:
the maximum, from 0.0); the waves are added in ascending index, from wave 0's value."""
import numpy as np

ROW = 16
SUM_ONE_SIGNED = (1, 3, 4, 5, 7, 8, 9)  # sums of one sign on these inputs (slot 4: the rewards are <= 0)
SIGNED = {0: 1, 6: 7}                   # signed sum -> its magnitude slot
EXACT = (2, 10, 11, 12)                 # the maximum, two counts, the cluster power
_IDX = np.arange(64)


def house_terms(T, Tm, tg, lock, on, r):
    """tick_acc's twelve per-house values, [12, n] (slot 2: the value the maximum runs over)."""
    T, Tm, tg, r = (np.asarray(x, np.float64) for x in (T, Tm, tg, r))
    N = np.float64(len(T))
    e = T - tg / N
    d = T - tg
    return np.stack([e, np.abs(e), e, e * e, r / N, T, d, np.abs(d), Tm, tg,
                     np.asarray(lock, bool).astype(np.float64), np.asarray(on, bool).astype(np.float64)])


def ordered_reduce(terms):
    """[12, n] per-house values -> the 12 slots in the kernel's order."""
    n = terms.shape[1]
    nw = (n + 127) // 128
    house = (np.arange(nw)[:, None] * 128 + _IDX[None, :] * 2)  # [nw, 64]: a lane's first house
    out = np.empty(12, np.float64)
    for k in range(12):
        v = np.zeros((nw, 64), np.float64)
        for h in range(2):
            i = house + h
            ok = i < n
            x = terms[k][np.where(ok, i, 0)]
            v = np.where(ok, np.maximum(v, x) if k == 2 else v + x, v)
        for off in (32, 16, 8, 4, 2, 1):
            o = v[:, _IDX ^ off]
            v = np.maximum(v, o) if k == 2 else v + o
        res = v[0, 0]
        for w in range(1, nw):
            res = max(res, v[w, 0]) if k == 2 else res + v[w, 0]
        out[k] = res
    return out


def stats_row(T, Tm, tg, lock, on, r, P):
    """The 16 doubles of a cluster after a tick: post-step air / mass temperatures, targets, the lock and on
    bits of the post-step FSM words (shard.decode_hvac), the tick's rewards and cluster power."""
    row = np.zeros(ROW, np.float64)
    row[:12] = ordered_reduce(house_terms(T, Tm, tg, lock, on, r))
    row[12] = P
    return row
