"""The shapes tests/test_deep_sites.py (the references and the host cores) and tests/test_gpu_deep_sites.py (the kernels) run the
per-bag code on past the places where a narrow integer would wrap: bags of more than 2^16 reads and pairs whose counts pass 2^32.

BIG        bag sizes around 2^12 + 2, 2^13, 2^14 + 1, 2^15, 2^16, 2^16 +- 1 and 2^17 (+ 1), with two small bags between the first large
           ones: a rejection mask of up to 18 bits, a bag index past 2^16, bags 128 times the 1024-read LDS bag.
scalar     three pairs of bags with n = N_A = 70000 and m = N_B = 62000 reads (n m = 4 340 000 000 > 2^32, n + m = 132 000 < 2^20),
           each also swapped: sites 0..5 of set A against sites 0..5 of set B (NAMES).
             separated    a uniform in (0.6, 0.9), b uniform in (0.1, 0.4): gt = n m, d_neg = n m; swapped: gt = 0, d_pos = n m
             all equal    both bags 0.5: eq = n m, one tie group of n + m > 2^16 reads, tie = N^3 - N
             four values  both bags drawn from {0, 0.25, 0.5, 1}: four tie groups of about 33 000 reads, gt and eq about n m / 4
limit      a pair of 2^19 + 1 and 2^19 reads (2^20 + 1 pooled: undefined) before a pair of 30 and 25 reads (defined).
signal     one pair of SIGNAL_ROWS = 36000 and 30000 rows of nine: tests/signal_ranksum_cases.py's value families, with the three
           constructions above in columns 0, 4 and 8 and one NaN in column 2 of one row of a.  n m > 2^30, a tie group of 66 000 > 2^16
           and tie > 2^32; the crossings of 2^32 by gt, eq, d_pos and d_neg are the scalar pairs'.  (At 70000 x 62000 rows the pair
           took its one wavefront 27 s on an MI355X, at this size it takes a quarter of that.)
What the statements (tests/ranksum_statement.py, tests/ks_statement.py, through their sorted-copy routes) say of them is computed once
and shared."""
import functools

import numpy as np

import ks_statement as KS
import ranksum_cases as RC
import ranksum_statement as RS
import signal_ranksum_cases as SC
import signal_ranksum_statement as SS
from ranksum_cases import same_bits  # noqa: F401  (the comparison the tests use)

BIG = [70000, 20, 65536, 21, 65537, 65535, 4098, 8191, 8192, 8193, 16385, 32768, 131072, 131073]
ENCODER_BAGS = [70000, 20, 65536, 21, 65537, 65535]
EXPECTATION_BAGS = [70000, 65536, 65537, 1, 131073, 20]
CHOICE_N = [65535, 65536, 65537, 70000, 131073]
SEED = 11
N_A, N_B = 70000, 62000
SIGNAL_ROWS = (36000, 30000)
NAN_ROW = 12345                                               # the row of a whose column 2 is NaN
NAMES = ("separated", "all equal", "four values", "separated, swapped", "all equal, swapped", "four values, swapped")
f32 = np.float32


def csr(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, np.int64))]).astype(np.int64)


def constructions(rng, n, m):
    """the three pairs (a [n], b [m]), in the order of NAMES"""
    sep = ((0.6 + 0.3 * rng.random(n)).astype(f32), (0.1 + 0.3 * rng.random(m)).astype(f32))
    equal = (np.full(n, 0.5, f32), np.full(m, 0.5, f32))
    four = (RC.four(rng, n), RC.four(rng, m))
    return sep, equal, four


@functools.lru_cache(maxsize=None)
def scalar_pairs():
    return constructions(np.random.default_rng(SEED), N_A, N_B)


@functools.lru_cache(maxsize=None)
def scalar_sets():
    """(prob_a, off_a, prob_b, off_b): site k of A against site k of B is pair NAMES[k]"""
    p = scalar_pairs()
    a = [x[0] for x in p] + [x[1] for x in p]
    b = [x[1] for x in p] + [x[0] for x in p]
    return np.concatenate(a), csr([x.size for x in a]), np.concatenate(b), csr([x.size for x in b])


def _columns(rows, n_int):
    """rows of four values -> four arrays, the first n_int of them int64 and the others float64"""
    return tuple(np.array([r[f] for r in rows], np.int64 if f < n_int else np.float64) for f in range(4))


def _want(statement, n_int, sets):
    va, oa, vb, ob = sets
    return _columns([statement(va[oa[k]:oa[k + 1]], vb[ob[k]:ob[k + 1]]) for k in range(oa.size - 1)], n_int)


@functools.lru_cache(maxsize=None)
def scalar_ranksum_want():
    """(gt, eq, tie int64 [6], z float64 [6])"""
    return _want(RS.pair, 3, scalar_sets())


@functools.lru_cache(maxsize=None)
def scalar_ks_want():
    """(d_pos, d_neg int64 [6], med_a, med_b float64 [6])"""
    return _want(KS.pair, 2, scalar_sets())


@functools.lru_cache(maxsize=None)
def limit_sets(pooled=RS.MAX_POOLED + 1):
    """(prob_a, off_a, prob_b, off_b): pair 0 has `pooled` reads in its two bags together, pair 1 has 30 + 25"""
    rng = np.random.default_rng(SEED + 1)
    n = pooled - pooled // 2
    a = [RC.probs(rng, n), RC.probs(rng, 30)]
    b = [RC.probs(rng, pooled - n), RC.four(rng, 25)]
    return np.concatenate(a), csr([x.size for x in a]), np.concatenate(b), csr([x.size for x in b])


@functools.lru_cache(maxsize=None)
def limit_want(pooled=RS.MAX_POOLED + 1):
    """((gt, eq, tie, z), (d_pos, d_neg, med_a, med_b)) of the two pairs of limit_sets(pooled)"""
    return _want(RS.pair, 3, limit_sets(pooled)), _want(KS.pair, 2, limit_sets(pooled))


@functools.lru_cache(maxsize=None)
def signal_sets():
    """(X_a [n, 9], off_a, X_b [m, 9], off_b): one site on either side"""
    n, m = SIGNAL_ROWS
    rng = np.random.default_rng(SEED + 2)
    Xa, Xb = SC.rows(rng, n, 0), SC.rows(rng, m, 1)
    for column, (a, b) in zip((0, 4, 8), constructions(rng, n, m)):
        Xa, Xb = SC.put(Xa, column, a), SC.put(Xb, column, b)
    Xa = SC.put(Xa, 2, np.nan, row=NAN_ROW)
    return np.ascontiguousarray(Xa, f32), csr([n]), np.ascontiguousarray(Xb, f32), csr([m])


@functools.lru_cache(maxsize=None)
def signal_ranksum_want():
    """(gt, eq, tie int64 [1, 9], z float64 [1, 9])"""
    Xa, _, Xb, _ = signal_sets()
    return tuple(x.reshape(1, 9) for x in _columns(SS.pair(Xa, Xb), 3))


@functools.lru_cache(maxsize=None)
def signal_ks_want():
    """(d_pos, d_neg int64 [1, 9], med_a, med_b float64 [1, 9])"""
    Xa, _, Xb, _ = signal_sets()
    return tuple(x.reshape(1, 9) for x in _columns(KS.signal_pair(Xa, Xb), 2))


def largest_tie_group(a, b):
    return int(np.unique(np.concatenate([a, b]) + f32(0), return_counts=True)[1].max())
