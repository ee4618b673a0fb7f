"""The exact two-sided p-value of the two-sample Kolmogorov-Smirnov statistic (include/m6a.h: m6a_ks_exact), stated in NumPy float64.

Take n >= 1, m >= 1 and an integer h, the statistic in units of 1 / (n m): h = max(d_pos, d_neg) of tests/ks_statement.py.  A cell (i, j),
0 <= i <= n, 0 <= j <= m, is OUTSIDE when |m i - n j| >= h (Python integers).  v[i][j] is the probability that a uniformly drawn monotone
path from (i, j) to (n, m) meets an outside cell, (i, j) included:
    v[i][j] = 1.0 when (i, j) is outside,    v[n][m] = 0.0 when it is inside,    otherwise
    v[i][j] = ((n - i) * v[i+1][j] + (m - j) * v[i][j+1]) / (n + m - i - j),    a neighbour beyond the grid being 0.0,
two products, one sum and one division of IEEE doubles, each rounded on its own.  p = v[0][0] = P(D >= h / (n m)), what
scipy.stats.ks_2samp(method="exact") computes.  The grid is walked one anti-diagonal i + j = s at a time, from s = n + m down to 0, with
elementwise operations only; a diagonal's inside cells are a run of consecutive i (|(n + m) i - n s| < h), so only that run is held and
every other cell of the grid is 1.0.  h <= 0 gives 1.0 ((0, 0) is outside); h > n m gives 0.0 by the recurrence.

Undefined, p = NaN: n < 1, m < 1, h < 0 (the undefined pair of the KS kernels has d_pos = d_neg = -1), min(n, m) > SHORT or n m > CELLS."""
import numpy as np

SHORT = 2047                    # M6A_KS_EXACT_SHORT
CELLS = 100_000_000             # M6A_KS_EXACT_CELLS


def undefined(n, m, h):
    return n < 1 or m < 1 or h < 0 or min(n, m) > SHORT or n * m > CELLS


def inside_run(n, m, h, s):
    """the inside cells of the diagonal i + j = s are i_lo <= i <= i_hi (empty: i_lo > i_hi), inside the grid"""
    N = n + m
    i_lo = (n * s - h) // N + 1                                  # (n + m) i > n s - h
    i_hi = -((-(n * s + h)) // N) - 1                            # (n + m) i < n s + h
    return max(i_lo, 0, s - m), min(i_hi, n, s)


def p_exact(n, m, h):
    n, m, h = int(n), int(m), int(h)
    if undefined(n, m, h):
        return float("nan")
    if h <= 0:
        return 1.0
    lo1, run1 = 0, np.zeros(0)                                   # the inside run of the diagonal s + 1: its first i and its values

    def neighbour(i, j):
        """v at the cells (i[k], j[k]) of the diagonal s + 1: 0.0 beyond the grid, the held value inside the band, 1.0 outside it"""
        held = (i >= lo1) & (i < lo1 + run1.size)
        out = np.where((i > n) | (j > m), 0.0, 1.0)
        out[held] = run1[i[held] - lo1]
        return out

    for s in range(n + m, -1, -1):
        i_lo, i_hi = inside_run(n, m, h, s)
        i = np.arange(i_lo, i_hi + 1, dtype=np.int64)
        j = s - i
        if s == n + m:
            run = np.zeros(i.size)                               # (n, m), inside
        else:
            a = (n - i).astype(np.float64) * neighbour(i + 1, j)
            b = (m - j).astype(np.float64) * neighbour(i, j + 1)
            run = (a + b) / np.float64(n + m - s)
        lo1, run1 = i_lo, run
    return float(run1[0])                                        # s = 0: the cell (0, 0), inside since h >= 1


def ks_h(d_pos, d_neg):
    """h of an item from the two integers of m6a_site_ks: -1 for an undefined pair"""
    return np.maximum(np.asarray(d_pos, np.int64), np.asarray(d_neg, np.int64))


def p_exact_many(n, m, h):
    n, m, h = (np.asarray(x, np.int64).ravel() for x in (n, m, h))
    return np.array([p_exact(a, b, c) for a, b, c in zip(n.tolist(), m.tolist(), h.tolist())], np.float64)
