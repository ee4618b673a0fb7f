"""The rank-sum test on the nine signal features (include/m6a.h: m6a_site_signal_ranksum), stated in plain NumPy: for every pair and
every column c of X, tests/ranksum_statement.py's `pair` on column c of the rows of the two sites.  Nothing of the test itself is
written here again -- the integers, the lines of z and what is undefined are ranksum_statement's.  A NaN is in one column, so it leaves
that column of the pair undefined and no other; an empty bag or more than 2^20 pooled rows leave all nine undefined, since every
column has the bag's size.
"""
import numpy as np

import ranksum_statement as RS

N_COLUMNS = 9


def pair(Xa, Xb):
    """Xa [n, 9], Xb [m, 9] float32 -> nine (gt, eq, tie, z), one per column"""
    Xa, Xb = np.asarray(Xa, np.float32).reshape(-1, N_COLUMNS), np.asarray(Xb, np.float32).reshape(-1, N_COLUMNS)
    return [RS.pair(Xa[:, c], Xb[:, c]) for c in range(N_COLUMNS)]


def site_signal_ranksum(X_a, off_a, X_b, off_b, pair_a=None, pair_b=None):
    """(gt, eq, tie int64 [P, 9], z float64 [P, 9]) as m6a_site_signal_ranksum delivers them"""
    X_a, X_b = np.asarray(X_a, np.float32).reshape(-1, N_COLUMNS), np.asarray(X_b, np.float32).reshape(-1, N_COLUMNS)
    off_a, off_b = np.asarray(off_a, np.int64), np.asarray(off_b, np.int64)
    if pair_a is None or pair_b is None:
        assert off_a.size == off_b.size
    pa = np.arange(off_a.size - 1) if pair_a is None else np.asarray(pair_a, np.int64)
    pb = np.arange(off_b.size - 1) if pair_b is None else np.asarray(pair_b, np.int64)
    assert pa.size == pb.size
    P = pa.size
    gt, eq, tie = (np.empty((P, N_COLUMNS), np.int64) for _ in range(3))
    z = np.empty((P, N_COLUMNS), np.float64)
    for k in range(P):
        a0, a1, b0, b1 = off_a[pa[k]], off_a[pa[k] + 1], off_b[pb[k]], off_b[pb[k] + 1]
        for c in range(N_COLUMNS):
            gt[k, c], eq[k, c], tie[k, c], z[k, c] = RS.pair(X_a[a0:a1, c], X_b[b0:b1, c])
    return gt, eq, tie, z
