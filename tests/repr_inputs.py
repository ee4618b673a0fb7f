"""The doubles the number core of the data.json writer (m6anet_amd/csrc/m6a_repr.h) is held to, from one seeded generator that the
CPU tests (test_repr_core.py) and the GPU tests (test_gpu_dataprep_writer.py) share.  The core TAKES exactly the finite v with
1e-4 <= v < 1e16 and DECLINES everything else."""
import gzip
import json
import os
import struct

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LO, HI = 1e-4, 1e16


def from_bits(e, mantissa):
    """The double 2^e * (1 + mantissa / 2^52)."""
    return struct.unpack("<d", struct.pack("<Q", ((e + 1023) << 52) | mantissa))[0]


def golden_features():
    """All nine feature columns of ref_tests_data/data.json, flattened."""
    out = []
    for line in open(os.path.join(GOLD, "ref_tests_data", "data.json")):
        (tx, by_pos), = json.loads(line).items()
        (pos, by_kmer), = by_pos.items()
        (kmer, reads), = by_kmer.items()
        for r in reads:
            out.extend(r[:9])
    return out


def declined():
    return [0.0, -0.0, -1.0, -0.25, -1e-4, -123456.789, 5e-324, 9.9e-5, 1e16, 1e300, float("nan"), float("inf"), float("-inf")]


_cache = {}


def taken():
    """float64 array: every value here lies in [1e-4, 1e16)."""
    if "taken" in _cache:
        return _cache["taken"]
    v = []
    for e in range(-14, 54):                                         # every binade, at its edges and its middle
        for m in (0, 1, 2, 2 ** 51 - 1, 2 ** 51, 2 ** 51 + 1, 2 ** 52 - 2, 2 ** 52 - 1):
            v.append(from_bits(e, m))
    for k in range(1, 20001):                                        # what np.round(x, 1) and np.round(x, 3) produce, and their neighbours
        for x in (k / 10, k / 1000):
            v += [float(np.nextafter(x, 0.0)), x, float(np.nextafter(x, np.inf))]
    for k in range(-4, 17):                                          # powers of ten and three ulps either side
        x = float("1e%d" % k)
        lo = hi = x
        v.append(x)
        for _ in range(3):
            lo, hi = float(np.nextafter(lo, 0.0)), float(np.nextafter(hi, np.inf))
            v += [lo, hi]
    v += [LO, float(np.nextafter(LO, 1.0)), float(np.nextafter(HI, 0.0))]   # the doubles around 1e-4 and 1e16 that are inside
    rng = np.random.RandomState(20240517)
    es = rng.randint(-14, 54, size=100000)
    ms = rng.randint(0, 2 ** 31, size=100000).astype(np.uint64) << np.uint64(21) | rng.randint(0, 2 ** 21, size=100000).astype(np.uint64)
    bits = (es + 1023).astype(np.uint64) << np.uint64(52) | ms
    v += bits.view(np.float64).tolist()
    v += golden_features()
    a = np.array(v, np.float64)
    a = a[(a >= LO) & (a < HI)]                                      # (2^-14 < 1e-4 and 2^53 (1 + m) may pass 1e16: those are declined ones)
    _cache["taken"] = a
    return a


def all_values():
    """taken() with the declined set and the out-of-range ends of the binade sweep spliced in: (values, is_taken)."""
    if "all" in _cache:
        return _cache["all"]
    extra = declined() + [from_bits(-14, 0), from_bits(-14, 2 ** 51), float(np.nextafter(LO, 0.0)), from_bits(53, 2 ** 51), from_bits(53, 2 ** 52 - 1)]
    t = taken()
    rng = np.random.RandomState(7)
    at = np.sort(rng.randint(0, t.size + 1, size=len(extra)))
    v = np.insert(t, at, np.array(extra, np.float64))
    ok = (v >= LO) & (v < HI)
    assert ok.sum() == t.size and (~ok).sum() == len(extra)
    _cache["all"] = (v, ok)
    return v, ok


def expected(v, round3=False):
    """Python's repr of every value (of np.round(v, 3) with round3), or None where the core declines."""
    r = np.round(v, 3) if round3 else np.asarray(v, np.float64)
    return [repr(float(x)) if LO <= x < HI else None for x in r]
