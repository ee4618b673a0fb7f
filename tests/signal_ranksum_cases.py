"""The shapes tests/test_signal_ranksum_core.py (the host core) and tests/test_gpu_signal_ranksum.py (the kernel) run
m6a_site_signal_ranksum on, and what tests/signal_ranksum_statement.py says of them, computed once per (site of A, site of B) and shared.

Two sets of sites with the same number of sites, so that the identity pairing is a legal call.  Sites 0..15 of either set are bags of
SIZES rows: the sizes around the wavefront's chunk of 64 and around TILE, the kernel's LDS tile in rows (M6A_PAIR_TILE in
m6anet_amd/csrc/m6a_pairs.h).  The sites behind them are the two sides of the special pairs, in order.  Every column of X has a
value family of its own (COLUMNS), so a result that took another column's values, or its neighbour's, is another number."""
import functools

import numpy as np

import signal_ranksum_statement as SS
from ranksum_cases import same_bits  # noqa: F401  (the comparison the tests use)

TILE = 256
SIZES = (1, 2, 19, 20, 21, 63, 64, 65, 127, 128, 129, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE + 1)
C = 9
GRID_PAIRS = 4 * 64 * 256          # four pairs per block times the largest grid of the launch (64 blocks per CU, 256 CUs)
f32 = np.float32
COLUMNS = ("continuous", "four values", "quantised to 0.1", "all equal", "continuous, skewed", "the negation of column 4",
           "quantised to 0.1, wider", "four other values", "continuous, b shifted")


def rows(rng, n, side):
    """n rows [n, 9], one value family per column; `side` (0: a, 1: b) moves some columns so that z is not near 0 everywhere"""
    X = np.empty((n, C), f32)
    X[:, 0] = rng.random(n, f32)
    X[:, 1] = rng.choice(np.array([0, 0.25, 0.5, 1], f32), n)
    X[:, 2] = np.round(rng.normal(0.1 * side, 0.6, n), 1)
    X[:, 3] = 0.5
    X[:, 4] = rng.random(n, f32) ** 4
    X[:, 5] = -X[:, 4]
    X[:, 6] = np.round(rng.normal(0, 2.0, n), 1)
    X[:, 7] = rng.choice(np.array([-3, -1, 2, 7], f32), n, p=(0.4, 0.3, 0.2, 0.1) if side else (0.1, 0.2, 0.3, 0.4))
    X[:, 8] = rng.normal(0.5 * side, 1.0, n)
    return X


def put(X, column, values, row=None):
    X = X.copy()
    if row is None:
        X[:, column] = np.asarray(values, f32)
    else:
        X[row, column] = values
    return X


@functools.lru_cache(maxsize=None)
def sets():
    """(X_a [Ra, 9], off_a, X_b [Rb, 9], off_b, names): names[k] is what special pair k -- sites len(SIZES) + k of both sets -- is there for"""
    rng = np.random.default_rng(3201)
    a = [rows(rng, n, 0) for n in SIZES]
    b = [rows(rng, n, 1) for n in SIZES]
    every = rows(rng, 40, 0)
    for c in range(C):
        every[(7 * c) % 40, c] = np.nan                       # another row for every column
    none = np.zeros((0, C), f32)
    special = [
        ("3000 x 2500", rows(rng, 3000, 0), rows(rng, 2500, 1)),
        ("three rows", rows(rng, 3, 0), rows(rng, 3, 1)),
        ("nan in column 4 of a", put(rows(rng, 25, 0), 4, np.nan, row=11), rows(rng, 30, 1)),
        ("nan in column 8 of b", rows(rng, 70, 0), put(rows(rng, 70, 1), 8, np.nan, row=69)),
        ("nan in every column", every, rows(rng, 33, 1)),
        ("signed zeros in column 2", put(rows(rng, 4, 0), 2, [-0.0, 0.0, -0.0, 0.25]), put(rows(rng, 3, 1), 2, [0.0, -0.0, 0.5])),
        ("infinities in column 6", put(rows(rng, 4, 0), 6, [np.inf, 0.5, -np.inf, np.inf]), put(rows(rng, 3, 1), 6, [np.inf, 0.25, 0.5])),
        ("empty a", none, rows(rng, 20, 1)),
        ("empty b", rows(rng, 20, 0), none),
        ("both empty", none, none),
        ("complete separation in column 1", put(rows(rng, 30, 0), 1, np.linspace(0.6, 0.9, 30)), put(rows(rng, 25, 1), 1, np.linspace(0.1, 0.4, 25))),
    ]
    a += [s[1] for s in special]
    b += [s[2] for s in special]
    off = lambda bags: np.concatenate([[0], np.cumsum([x.shape[0] for x in bags])]).astype(np.int64)    # noqa: E731
    return (np.ascontiguousarray(np.concatenate(a), f32), off(a), np.ascontiguousarray(np.concatenate(b), f32), off(b),
            tuple(s[0] for s in special))


def n_sites():
    return sets()[1].size - 1


@functools.lru_cache(maxsize=None)
def one(i, j):
    """the statement for site i of A against site j of B: (gt [9], eq [9], tie [9], z [9])"""
    Xa, oa, Xb, ob, _ = sets()
    r = SS.pair(Xa[oa[i]:oa[i + 1]], Xb[ob[j]:ob[j + 1]])
    return tuple(np.array([x[f] for x in r], np.float64 if f == 3 else np.int64) for f in range(4))


def want(pair_a=None, pair_b=None):
    """the statement's (gt, eq, tie, z), each [P, 9], for a pair list over sets(); None: the identity"""
    S = n_sites()
    ia = np.arange(S) if pair_a is None else np.asarray(pair_a)
    ib = np.arange(S) if pair_b is None else np.asarray(pair_b)
    keys, inverse = np.unique(ia * S + ib, return_inverse=True)
    each = [one(int(k) // S, int(k) % S) for k in keys]
    return tuple(np.array([e[f] for e in each], np.float64 if f == 3 else np.int64).reshape(-1, C)[inverse.ravel()] for f in range(4))


@functools.lru_cache(maxsize=None)
def pair_lists():
    """name -> (pair_a, pair_b): the bag sizes crossed and every special pair; that list backwards; lists of 0, 1, 65 and 4097 pairs drawn
    with repetition from the sites of at most TILE + 1 rows; and one list of more than GRID_PAIRS pairs, drawn from the sites of at
    most 3 rows, which no grid of the launch covers in one pass"""
    S, K = n_sites(), len(SIZES)
    ca, cb = np.repeat(np.arange(K), K), np.tile(np.arange(K), K)
    full = (np.concatenate([ca, np.arange(K, S)]).astype(np.int64), np.concatenate([cb, np.arange(K, S)]).astype(np.int64))
    out = {"crossed and special": full, "backwards": (full[0][::-1].copy(), full[1][::-1].copy())}
    _, oa, _, ob, _ = sets()
    small_a, small_b = np.flatnonzero(np.diff(oa) <= TILE + 1), np.flatnonzero(np.diff(ob) <= TILE + 1)
    rng = np.random.default_rng(3202)
    for P in (0, 1, 65, 4097):
        out["%d drawn" % P] = (rng.choice(small_a, P).astype(np.int64), rng.choice(small_b, P).astype(np.int64))
    tiny_a, tiny_b = np.flatnonzero(np.diff(oa) <= 3), np.flatnonzero(np.diff(ob) <= 3)
    out["past the grid"] = (rng.choice(tiny_a, GRID_PAIRS + 7).astype(np.int64), rng.choice(tiny_b, GRID_PAIRS + 7).astype(np.int64))
    return out


LISTS = ("crossed and special", "backwards", "0 drawn", "1 drawn", "65 drawn", "4097 drawn", "past the grid", "identity")
