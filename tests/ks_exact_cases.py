"""The items (n, m, h) tests/test_gpu_ks_exact.py holds ks_exact_kernel to the host core on, and tests/test_ks_exact_core.py the host core to
tests/ks_exact_statement.py on.  The kernel takes rows in stripes of 64 with the shorter bag on j, so the sizes stand around 64, 128 and
192 on either axis; h runs from the undefined -1 over 0, the narrowest band and the middle to the band that covers the grid.
  cross()    SIZES x SIZES, each with the seven h of hs()
  SPECIAL    named items: the two bands at their extremes, both caps from both sides and on either axis, a subnormal and a zero result
  mixed()    one launch of more items than four per block of the largest grid covers: 288 distinct items, tiny ones and a few of some
             10^5 cells, ordered so that the four wavefronts of a block get very different amounts of work
A statement value is computed once per distinct item and process (statement())."""
import functools
import math

import numpy as np

import ks_exact_statement as ST

SIZES = (1, 2, 20, 63, 64, 65, 127, 128, 129, 192, 193)


def hs(n, m):
    """0, the narrowest band, about a quarter and a half of n m, n m, one beyond every attainable value, and the undefined pair's -1"""
    return (0, math.gcd(n, m), n * m // 4, n * m // 2, n * m, n * m + 1, -1)


def cross():
    return [(n, m, h) for n in SIZES for m in SIZES for h in hs(n, m)]


SPECIAL = {
    "a band narrower than one cell": (64, 63, 1),                # coprime sizes: (0, 0) and (n, m) alone are inside
    "a band narrower than one cell, three stripes": (193, 128, 1),
    "a band that covers the grid": (129, 65, 129 * 65 + 1),
    "an h far beyond the grid": (20, 20, 1 << 62),
    "the short cap": (2047, 2047, 2047 * 40),
    "the short cap, longer bag": (2047, 3000, 150000),
    "one past the short cap": (2048, 2048, 2048 * 40),
    "one past the short cap, longer bag": (2048, 3000, 150000),
    "the cell cap": (50000, 2000, 2000000),                     # 10^8 cells, some 4 10^6 of them inside the band
    "the cell cap, swapped": (2000, 50000, 2000000),
    "one past the cell cap": (50001, 2000, 2000000),
    "one past the cell cap, swapped": (2000, 50001, 2000000),
    "past the cell cap by far": (1 << 40, 1 << 40, 5),
    "a product past int64": (1 << 62, 2047, 5),
    "a subnormal result": (520, 520, 520 * 520),                # 2 / C(2 n, n)
    "a zero result": (600, 600, 600 * 600),
    "an empty first bag": (0, 20, 1),
    "an empty second bag": (20, 0, 1),
    "a negative size": (-3, 20, 1),
}
NAN = ("one past the short cap", "one past the short cap, longer bag", "one past the cell cap", "one past the cell cap, swapped",
       "past the cell cap by far", "a product past int64", "an empty first bag", "an empty second bag", "a negative size")


@functools.lru_cache(maxsize=None)
def mixed_pool():
    """(tiny, large): 256 items of 1..30 reads a side with any h, 32 of 193..600 reads a side with h around the middle of the distribution"""
    rng = np.random.default_rng(20250)
    tiny, large = [], []
    for _ in range(256):
        n, m = (int(x) for x in rng.integers(1, 31, 2))
        tiny.append((n, m, int(rng.integers(-1, n * m + 2))))
    for _ in range(32):
        n, m = (int(x) for x in rng.integers(193, 601, 2))
        lam = float(rng.uniform(0.4, 2.5))                      # h = lambda n m / sqrt(n m / (n + m)), so p runs from near 1 to 1e-5
        large.append((n, m, int(lam * n * m / math.sqrt(n * m / (n + m)))))
    return tuple(tiny), tuple(large)


def mixed(count):
    """`count` items: wavefront 1 of every eighth block gets a large item, everything else a tiny one"""
    tiny, large = mixed_pool()
    return [large[(k // 32) % len(large)] if k % 32 == 1 else tiny[(k * 7 + k // 256) % len(tiny)] for k in range(count)]


def arrays(items):
    a = np.array(items, np.int64).reshape(-1, 3)
    return tuple(np.ascontiguousarray(a[:, c]) for c in range(3))


def distinct(items):
    return sorted(set(items))


@functools.lru_cache(maxsize=None)
def statement(item):
    return ST.p_exact(*item)


def from_distinct(items, value_of):
    """value_of(distinct items) -> float64, spread back over `items`"""
    d = distinct(items)
    where = {it: k for k, it in enumerate(d)}
    v = np.asarray(value_of(d), np.float64)
    return v[[where[it] for it in items]]


def host(items):
    """the host core's p of every item, each distinct one computed once"""
    from m6anet_amd import _io
    return from_distinct(items, lambda d: _io.ks_exact(*arrays(d)))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())
