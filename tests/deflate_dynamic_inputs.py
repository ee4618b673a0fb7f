"""The texts level 2 of the BGZF writer (dynamic Huffman codes: m6anet_amd/csrc/m6a_deflate.h; include/m6a.h states it) is held to, on
the host in tests/test_deflate_dynamic_core.py and on the device in tests/test_gpu_deflate_dynamic.py: about 2.5 MB in all."""
import functools
import os

import numpy as np

import deflate_inputs as DI

BLOCK, PART, GOLD = DI.BLOCK, DI.PART, DI.GOLD
SIZES = (1, 2, 3, 64, 65, 258, 259, PART - 1, PART, PART + 1, BLOCK - 1, BLOCK, BLOCK + 1)
FAMILIES = ("same", "period2", "text", "sparse", "high", "random")
# one match length for each of the length symbols 257..285
LENGTHS = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
FIB_SYMBOLS = 22


def every_symbol(rng):
    """a block in which all 256 byte values and every length symbol occur: part k + 1 begins with a run of LENGTHS[k] + 1 equal
    bytes -- one literal and one match of exactly that length at distance 1 -- and part 40 with the 256 values"""
    t = bytearray(rng.integers(0, 256, BLOCK, dtype=np.uint8))
    for k, n in enumerate(LENGTHS):
        at = (k + 1) * PART
        t[at - 1:at + n + 2] = bytes([k + 2]) + bytes([k]) * (n + 1) + bytes([k + 1])
    t[40 * PART:40 * PART + 256] = bytes(range(256))
    assert len(t) == BLOCK
    return bytes(t)


def fibonacci(rng):
    """a block whose literals 0..21 occur 1, 1, 2, 3, ... 17 711 times -- an unlimited Huffman code of them alone is 21 bits deep --
    laid out so that no three bytes repeat within the 1 020 + 256 bytes behind them, which is as far as the finder can see: the symbols
    come in shuffled order, the next one that gives a new triple is taken, and where none does the lowest byte of 22..255 that gives
    one is put in between.  Those bytes flatten the tree; with them and the end-of-block code it is still 16 deep, which
    tests/deflate_dynamic_main.cpp confirms on the counts the core takes."""
    f = [1, 1]
    while len(f) < FIB_SYMBOLS:
        f.append(f[-1] + f[-2])
    pool = np.repeat(np.arange(FIB_SYMBOLS, dtype=np.uint8), f)
    rng.shuffle(pool)
    pool = [int(v) for v in pool]
    out, last = bytearray(), {}

    def fresh(c):
        p = last.get((out[-2], out[-1], c))
        return p is None or p < len(out) - 2 - (PART + 256)

    def put(v):
        out.append(v)
        if len(out) >= 3:
            last[tuple(out[-3:])] = len(out) - 3

    while pool:
        if len(out) < 2:
            put(pool.pop())
            continue
        seen = set()
        for k in range(1, min(len(pool), 200) + 1):
            s = pool[-k]
            if s not in seen and fresh(s):
                pool[-k], pool[-1] = pool[-1], pool[-k]
                put(pool.pop())
                break
            seen.add(s)
        else:
            put(next(v for v in range(FIB_SYMBOLS, 256) if fresh(v)))
    assert len(out) <= BLOCK, len(out)
    return bytes(out)


@functools.lru_cache(maxsize=None)
def texts():
    """name -> bytes"""
    rng = np.random.default_rng(12)
    old = DI.texts()
    gold = DI.golden_text(DI.GOLDEN[0])
    out = {}
    for n in SIZES:
        out["same_%d" % n] = b"a" * n                       # one literal, length symbol 285, one distance code: the 1-bit code, HLIT 29
        out["period2_%d" % n] = DI.cycle(b"xy", n)
        out["text_%d" % n] = DI.cycle(gold, n)
        out["sparse_%d" % n] = DI.sparse(rng, n)            # no match, so no distance code at all
        out["high_%d" % n] = bytes(rng.choice(np.array([144, 145, 200, 254, 255], np.uint8), n))
        out["random_%d" % n] = bytes(rng.integers(0, 256, n, dtype=np.uint8))
    for name in ("straddles_a_part_edge", "ends_at_the_block_end"):
        out[name] = old[name]
    out["every_symbol"] = every_symbol(rng)
    out["fibonacci"] = fibonacci(np.random.default_rng(12))     # a generator of its own: the layout is held to a depth
    for name in DI.GOLDEN:
        out["golden_" + name.split("_")[0]] = DI.golden_text(name)
    out["golden_site"] = open(os.path.join(GOLD, "config1_site_proba.csv"), "rb").read()
    return out
