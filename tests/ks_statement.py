"""The per-site Kolmogorov-Smirnov integers and medians (include/m6a.h: m6a_site_ks, m6a_site_signal_ks), stated in plain NumPy.

A pair has bag a (n reads, float32) and bag b (m reads, float32).  With A(v) = #{a_i <= v} and B(v) = #{b_j <= v}, counted here from the
full comparison tables of the pooled sample against either bag -- the definition itself --
    d_pos = max over the pooled v of (m A(v) - n B(v)),    d_neg = max over the pooled v of (n B(v) - m A(v)),
two exact integers, both >= 0.  A median is the mean of the two middle order statistics lo = x_((s-1)/2) and hi = x_(s/2) of the sorted
bag, one line of IEEE double operations (Python floats are IEEE doubles); a result that compares equal to zero is +0.0, and +inf and -inf
as the two middles give NaN.  An undefined pair (tests/ranksum_statement.py's rule: an empty bag, a NaN, more than 2^20 pooled reads)
is (-1, -1, NaN, NaN).  The signal form is this statement on each of the nine columns of X."""
import numpy as np

import ranksum_statement as RS

UNDEFINED = (-1, -1, float("nan"), float("nan"))
N_COLUMNS = 9


def median(x):
    s = np.sort(np.asarray(x, np.float32))
    lo, hi = float(s[(s.size - 1) // 2]), float(s[s.size // 2])
    with np.errstate(invalid="ignore"):
        med = float(np.float64(lo) * 0.5 + np.float64(hi) * 0.5)
    return 0.0 if med == 0.0 else med


def d_by_table(a, b):
    """d_pos, d_neg from the comparison tables: the definition, O((n + m) max(n, m)) memory"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    pooled = np.concatenate([a, b])
    A = (a[None, :] <= pooled[:, None]).sum(axis=1, dtype=np.int64)
    B = (b[None, :] <= pooled[:, None]).sum(axis=1, dtype=np.int64)
    t = b.size * A - a.size * B
    return int(t.max()), int((-t).max())


def d_by_sort(a, b):
    """the same two integers from sorted copies, for bags whose tables would not fit"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    pooled = np.concatenate([a, b])
    A = np.searchsorted(np.sort(a), pooled, side="right").astype(np.int64)
    B = np.searchsorted(np.sort(b), pooled, side="right").astype(np.int64)
    t = b.size * A - a.size * B
    return int(t.max()), int((-t).max())


def pair(a, b, table_limit=6000):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    n, m = a.size, b.size
    if n == 0 or m == 0 or n + m > RS.MAX_POOLED or np.isnan(a).any() or np.isnan(b).any():
        return UNDEFINED
    d_pos, d_neg = d_by_table(a, b) if n + m <= table_limit else d_by_sort(a, b)
    return d_pos, d_neg, median(a), median(b)


def site_ks(prob_a, off_a, prob_b, off_b, pair_a=None, pair_b=None):
    """(d_pos int64 [P], d_neg int64 [P], med_a float64 [P], med_b float64 [P]) as m6a_site_ks delivers them"""
    prob_a, prob_b = np.asarray(prob_a, np.float32), np.asarray(prob_b, np.float32)
    off_a, off_b = np.asarray(off_a, np.int64), np.asarray(off_b, np.int64)
    if pair_a is None or pair_b is None:
        assert off_a.size == off_b.size
    pa = np.arange(off_a.size - 1) if pair_a is None else np.asarray(pair_a, np.int64)
    pb = np.arange(off_b.size - 1) if pair_b is None else np.asarray(pair_b, np.int64)
    assert pa.size == pb.size
    P = pa.size
    d_pos, d_neg, med_a, med_b = np.empty(P, np.int64), np.empty(P, np.int64), np.empty(P, np.float64), np.empty(P, np.float64)
    for k in range(P):
        i, j = int(pa[k]), int(pb[k])
        d_pos[k], d_neg[k], med_a[k], med_b[k] = pair(prob_a[off_a[i]:off_a[i + 1]], prob_b[off_b[j]:off_b[j + 1]])
    return d_pos, d_neg, med_a, med_b


def signal_pair(Xa, Xb):
    """Xa [n, 9], Xb [m, 9] float32 -> nine (d_pos, d_neg, med_a, med_b), one per column"""
    Xa, Xb = np.asarray(Xa, np.float32).reshape(-1, N_COLUMNS), np.asarray(Xb, np.float32).reshape(-1, N_COLUMNS)
    return [pair(Xa[:, c], Xb[:, c]) for c in range(N_COLUMNS)]


def site_signal_ks(X_a, off_a, X_b, off_b, pair_a=None, pair_b=None):
    """(d_pos, d_neg int64 [P, 9], med_a, med_b float64 [P, 9]) as m6a_site_signal_ks delivers them"""
    X_a, X_b = np.asarray(X_a, np.float32).reshape(-1, N_COLUMNS), np.asarray(X_b, np.float32).reshape(-1, N_COLUMNS)
    off_a, off_b = np.asarray(off_a, np.int64), np.asarray(off_b, np.int64)
    if pair_a is None or pair_b is None:
        assert off_a.size == off_b.size
    pa = np.arange(off_a.size - 1) if pair_a is None else np.asarray(pair_a, np.int64)
    pb = np.arange(off_b.size - 1) if pair_b is None else np.asarray(pair_b, np.int64)
    assert pa.size == pb.size
    P = pa.size
    d_pos, d_neg = np.empty((P, N_COLUMNS), np.int64), np.empty((P, N_COLUMNS), np.int64)
    med_a, med_b = np.empty((P, N_COLUMNS), np.float64), np.empty((P, N_COLUMNS), np.float64)
    for k in range(P):
        a0, a1, b0, b1 = off_a[pa[k]], off_a[pa[k] + 1], off_b[pb[k]], off_b[pb[k] + 1]
        for c in range(N_COLUMNS):
            d_pos[k, c], d_neg[k, c], med_a[k, c], med_b[k, c] = pair(X_a[a0:a1, c], X_b[b0:b1, c])
    return d_pos, d_neg, med_a, med_b
