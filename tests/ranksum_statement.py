"""The per-site rank-sum test (include/m6a.h: m6a_site_ranksum), stated in plain NumPy.

A pair has bag a (n reads, float32) and bag b (m reads, float32).  Three exact integers come first -- gt, eq and tie, counted here
from the full n x m and N x N comparison tables, the definition itself -- then one double z, every operation of which is a single
IEEE double operation in the order the header writes them.  Python floats are IEEE doubles and math.sqrt rounds correctly, so the
lines of `z_of` are the header's lines.  An undefined pair (an empty bag, a NaN, more than 2^20 pooled reads) is (-1, -1, -1, NaN).
"""
import math

import numpy as np

MAX_POOLED = 1 << 20
UNDEFINED = (-1, -1, -1, float("nan"))


def z_of(n, m, gt, eq, tie):
    nm = float(n) * float(m)
    N = float(n + m)
    U = float(2 * gt + eq) * 0.5
    d = U - nm * 0.5
    tc = float(tie) / (N * (N - 1.0))
    var = nm / 12.0 * ((N + 1.0) - tc)
    s = math.sqrt(var)
    num = max(abs(d) - 0.5, 0.0)
    return math.copysign(num, d) / s if num > 0 else math.copysign(0.0, d)


def counts_by_table(a, b):
    """gt, eq, tie from the comparison tables: the definition, O((n + m)^2) memory"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    pooled = np.concatenate([a, b])
    c = (pooled[:, None] == pooled[None, :]).sum(axis=1, dtype=np.int64)
    return int((a[:, None] > b[None, :]).sum(dtype=np.int64)), int((a[:, None] == b[None, :]).sum(dtype=np.int64)), int((c * c - 1).sum())


def counts_by_sort(a, b):
    """the same three integers from sorted copies, for bags whose tables would not fit"""
    a, b = np.asarray(a, np.float32) + np.float32(0), np.asarray(b, np.float32) + np.float32(0)     # -0.0 + 0.0 = 0.0: one value
    sb = np.sort(b)
    below = np.searchsorted(sb, a, side="left").astype(np.int64)
    upto = np.searchsorted(sb, a, side="right").astype(np.int64)
    _, t = np.unique(np.concatenate([a, b]), return_counts=True)
    t = t.astype(object)                                        # Python integers: t^3 of 2^20 reads needs 60 bits
    return int(below.sum()), int((upto - below).sum()), int((t * t * t - t).sum())


def pair(a, b, table_limit=6000):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    n, m = a.size, b.size
    if n == 0 or m == 0 or n + m > MAX_POOLED or np.isnan(a).any() or np.isnan(b).any():
        return UNDEFINED
    gt, eq, tie = counts_by_table(a, b) if n + m <= table_limit else counts_by_sort(a, b)
    return gt, eq, tie, z_of(n, m, gt, eq, tie)


def site_ranksum(prob_a, off_a, prob_b, off_b, pair_a=None, pair_b=None):
    """(gt int64 [P], eq int64 [P], tie int64 [P], z float64 [P]) as m6a_site_ranksum delivers them"""
    prob_a, prob_b = np.asarray(prob_a, np.float32), np.asarray(prob_b, np.float32)
    off_a, off_b = np.asarray(off_a, np.int64), np.asarray(off_b, np.int64)
    if pair_a is None or pair_b is None:
        assert off_a.size == off_b.size
    pa = np.arange(off_a.size - 1) if pair_a is None else np.asarray(pair_a, np.int64)
    pb = np.arange(off_b.size - 1) if pair_b is None else np.asarray(pair_b, np.int64)
    assert pa.size == pb.size
    P = pa.size
    gt, eq, tie, z = np.empty(P, np.int64), np.empty(P, np.int64), np.empty(P, np.int64), np.empty(P, np.float64)
    for k in range(P):
        i, j = int(pa[k]), int(pb[k])
        gt[k], eq[k], tie[k], z[k] = pair(prob_a[off_a[i]:off_a[i + 1]], prob_b[off_b[j]:off_b[j + 1]])
    return gt, eq, tie, z
