"""The shapes tests/test_ranksum_core.py (the host core) and tests/test_gpu_ranksum.py (the kernel) run m6a_site_ranksum on, and
what tests/ranksum_statement.py says of them, computed once per (site of A, site of B) and shared.

Two sets of sites with the same number of sites, so that the identity pairing is a legal call.  Sites 0..10 of either set are bags
of SIZES reads; the sites behind them are the two sides of the special pairs below, in order.  TILE is the kernel's LDS tile
(M6A_PAIR_TILE in m6anet_amd/csrc/m6a_pairs.h); its wavefront owns the pooled sample in chunks of 64."""
import functools

import numpy as np

import ranksum_statement as RS

TILE = 256
SIZES = (1, 2, 19, 20, 21, 63, 64, 65, 127, 128, 129)
f32 = np.float32


def probs(rng, n):
    """read probabilities as the encoder gives them: most near 0, some anywhere; ties are rare"""
    p = rng.random(n, f32) ** 4
    return np.where(rng.random(n) < 0.1, rng.random(n, f32), p).astype(f32)


def four(rng, n):
    return rng.choice(np.array([0, 0.25, 0.5, 1], f32), n)


@functools.lru_cache(maxsize=None)
def sets():
    """(prob_a, off_a, prob_b, off_b, names): names[k] is what special pair k -- sites len(SIZES) + k of both sets -- is there for"""
    rng = np.random.default_rng(31)
    a = [four(rng, n) if k % 3 == 0 else probs(rng, n) for k, n in enumerate(SIZES)]
    b = [four(rng, n) if k % 2 == 0 else probs(rng, n) for k, n in enumerate(SIZES)]
    special = [
        ("1 x 1000", probs(rng, 1), probs(rng, 1000)),
        ("1000 x 1", probs(rng, 1000), probs(rng, 1)),
        ("3000 x 2500", probs(rng, 3000), np.concatenate([probs(rng, 1500), four(rng, 1000)])),
        ("a tile less", probs(rng, TILE - 1), four(rng, TILE - 1)),
        ("a tile", four(rng, TILE), probs(rng, TILE)),
        ("a tile more", probs(rng, TILE + 1), probs(rng, TILE + 1)),
        ("two tiles and one", four(rng, 2 * TILE + 1), four(rng, 2 * TILE - 1)),
        ("empty a", np.zeros(0, f32), probs(rng, 20)),
        ("empty b", probs(rng, 20), np.zeros(0, f32)),
        ("both empty", np.zeros(0, f32), np.zeros(0, f32)),
        ("all equal", np.full(70, 0.5, f32), np.full(33, 0.5, f32)),
        ("four values", four(rng, 50), four(rng, 41)),
        ("signed zeros", np.array([-0.0, 0.0, -0.0, 0.25], f32), np.array([0.0, -0.0, 0.5], f32)),
        ("inf", np.array([np.inf, 0.5, -np.inf, np.inf], f32), np.array([np.inf, 0.25, 0.5], f32)),
        ("nan in a", np.array([0.25, np.nan, 0.5], f32), probs(rng, 20)),
        ("nan in b", probs(rng, 70), np.concatenate([probs(rng, 69), [f32(np.nan)]]).astype(f32)),
        ("complete separation", np.linspace(0.6, 0.9, 30).astype(f32), np.linspace(0.1, 0.4, 25).astype(f32)),
    ]
    a += [s[1] for s in special]
    b += [s[2] for s in special]
    off = lambda bags: np.concatenate([[0], np.cumsum([x.size for x in bags])]).astype(np.int64)    # noqa: E731
    return np.concatenate(a).astype(f32), off(a), np.concatenate(b).astype(f32), off(b), tuple(s[0] for s in special)


def n_sites():
    return sets()[1].size - 1


@functools.lru_cache(maxsize=None)
def one(i, j):
    pa, oa, pb, ob, _ = sets()
    return RS.pair(pa[oa[i]:oa[i + 1]], pb[ob[j]:ob[j + 1]])


def want(pair_a=None, pair_b=None):
    """the statement's (gt, eq, tie, z) for a pair list over sets(); None: the identity"""
    ia = np.arange(n_sites()) if pair_a is None else np.asarray(pair_a)
    ib = np.arange(n_sites()) if pair_b is None else np.asarray(pair_b)
    rows = [one(int(i), int(j)) for i, j in zip(ia, ib)]
    return (np.array([r[0] for r in rows], np.int64), np.array([r[1] for r in rows], np.int64), np.array([r[2] for r in rows], np.int64),
            np.array([r[3] for r in rows], np.float64))


@functools.lru_cache(maxsize=None)
def pair_lists():
    """name -> (pair_a, pair_b): the bag sizes crossed and every special pair; that list backwards; and lists of 0, 1, 65 and 4097
    pairs drawn with repetition from the sites of at most TILE + 1 reads (a site in many pairs, in no order)"""
    S, K = n_sites(), len(SIZES)
    ca, cb = np.repeat(np.arange(K), K), np.tile(np.arange(K), K)
    full = (np.concatenate([ca, np.arange(K, S)]).astype(np.int64), np.concatenate([cb, np.arange(K, S)]).astype(np.int64))
    out = {"crossed and special": full, "backwards": (full[0][::-1].copy(), full[1][::-1].copy())}
    _, oa, _, ob, _ = sets()
    small_a, small_b = np.flatnonzero(np.diff(oa) <= TILE + 1), np.flatnonzero(np.diff(ob) <= TILE + 1)
    rng = np.random.default_rng(32)
    for P in (0, 1, 65, 4097):
        out["%d drawn" % P] = (rng.choice(small_a, P).astype(np.int64), rng.choice(small_b, P).astype(np.int64))
    return out


def same_bits(a, b):
    """equal bit for bit; NaN (whatever its payload) only where the other is NaN"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind != "f":
        return np.array_equal(a, b)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))
