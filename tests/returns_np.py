"""NumPy restatements of what ``rollout_returns`` accumulates, shared by
tests/test_returns_cpu.py and tests/test_returns_gpu.py.

* ``weights``: w[0] = weight0, w[t + 1] = w[t] * gamma, fp64 products in that order.
* ``row_form``: ret = ret + w[t] * rows[t], left to right, a multiply then an add per tick (NumPy
  never fuses them) — the contract of the open-loop sources and of the one-launch-per-tick sequence,
  bit for bit.
* ``window_form``: the closed-loop windows' regrouping.  Per window of K ticks
  a_i = sum_j w_j pen_i(j) and S = sum_j w_j sig(j), each from 0.0 in tick order, then
  ret_i = ret_i + -(alpha_temp a_i / norm_temp + S).
* ``bound``: both forms add terms of one sign (alpha_temp, alpha_sig >= 0, norm_* > 0, 0 < gamma <= 1),
  so each is within (T + 8) 2^-53 relative of the exact sum of the T ticks accumulated so far — the
  longest rounding chain is T + 4 roundings for the row form (per tick: the reward's own 3 or 4
  roundings happen once, then one product and one add per tick) and K + T / K + 5 for the window
  form — and they differ by at most twice that.
"""
import numpy as np

EPS = 2.0 ** -53


def weights(weight0, gamma, n):
    w = np.empty(n + 1, np.float64)
    w[0] = weight0
    for t in range(n):
        w[t + 1] = w[t] * np.float64(gamma)
    return w


def row_form(ret, w, rows):
    ret = np.array(ret, np.float64)
    for t in range(rows.shape[0]):
        ret = ret + w[t] * rows[t]
    return ret


def window_plan(n, win):
    """The library's WinPlan: ceil(n / win) windows of near-equal size, the larger ones first."""
    nw = (n + win - 1) // win
    base, rem = divmod(n, nw)
    return [base + (1 if w < rem else 0) for w in range(nw)]


def window_form(ret, w, pen, sig, win, alpha_temp, norm_temp):
    """pen: [T, N] raw temperature penalties; sig: [T] signal terms (alpha_sig x^2 / norm_sig)."""
    ret = np.array(ret, np.float64)
    t0 = 0
    for K in window_plan(pen.shape[0], win):
        a = np.zeros(pen.shape[1], np.float64)
        S = np.float64(0.0)
        for j in range(t0, t0 + K):
            a = a + w[j] * pen[j]
            S = S + w[j] * sig[j]
        tpen = alpha_temp * a
        ret = ret + -((tpen if norm_temp == 1.0 else tpen / norm_temp) + S)
        t0 += K
    return ret


def bound(T, ref):
    """|ret - ref| allowed after T accumulated ticks, per house."""
    return 2.0 * (T + 8) * EPS * np.abs(ref)
