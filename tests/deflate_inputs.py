"""The texts the BGZF writer (m6anet_amd/csrc/m6a_deflate.h; include/m6a.h states it) is held to, on the host in
tests/test_deflate_core.py and on the device in tests/test_gpu_deflate.py, and the checks every output must pass."""
import functools
import gzip
import os
import struct
import tempfile

import numpy as np

import bgzf_statement as B
import csv_edges as E
from m6anet_amd import _io, bgzf

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BLOCK = 0xff00                                  # text bytes per BGZF block
PART = BLOCK // 64                              # bytes per part of a full block: 1020
SIZES = (0, 1, 2, 3, 63, 64, 65, 257, 258, 259, 260, PART - 1, PART, PART + 1, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1)
GOLDEN = ("config1_indiv_proba.csv.gz", "replicate_indiv_proba.csv.gz")


def golden_text(name):
    return gzip.open(os.path.join(GOLD, name)).read()


def cycle(base, n):
    return (base * (n // len(base) + 1))[:n]


def sparse(rng, n):
    """letters that hardly ever repeat for three bytes in a row: what stands between two placed repeats"""
    return bytes(rng.integers(32, 127, n, dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def texts():
    """name -> bytes.  Every size with every kind of content, then the placed repeats, the golden files and the CSV edge cases."""
    rng = np.random.default_rng(11)
    gold = golden_text(GOLDEN[0])
    out = {}
    for n in SIZES:
        out["same_%d" % n] = b"a" * n                       # matches of 258 bytes at distance 1
        out["period2_%d" % n] = cycle(b"xy", n)
        out["period3_%d" % n] = cycle(b"xyz", n)
        out["text_%d" % n] = cycle(gold, n)
        out["high_%d" % n] = bytes(rng.choice(np.array([144, 145, 200, 254, 255], np.uint8), n))     # the 9-bit literals, with matches
        out["random_%d" % n] = bytes(rng.integers(0, 256, n, dtype=np.uint8))
    out["period32769"] = cycle(gold[:32769], 4 * 32769)     # one byte farther than a distance can reach
    x = bytes(rng.integers(0, 256, 200, dtype=np.uint8))
    t = bytearray(sparse(rng, BLOCK))
    t[700:900] = x
    t[950:1150] = x                                         # the repeat lies across the edge between parts 0 and 1 (byte 1020)
    out["straddles_a_part_edge"] = bytes(t)
    t = bytearray(sparse(rng, BLOCK + 500))
    t[BLOCK - 500:BLOCK - 300] = x
    t[BLOCK - 200:BLOCK] = x                                # the repeat's last byte is the block's last byte
    out["ends_at_the_block_end"] = bytes(t)
    for name in GOLDEN:
        out["golden_" + name.split("_")[0]] = golden_text(name)
    from test_csv_statement import host_texts
    import pathlib
    for name, a in sorted(E.cases().items()):
        with tempfile.TemporaryDirectory() as d:
            out["edges_%s_site" % name], out["edges_%s_indiv" % name] = host_texts(pathlib.Path(d), a)
    return out


def blocks_of(data):
    """[(offset, total, isize)] by BSIZE alone"""
    out, at = [], 0
    while at < len(data):
        assert data[at:at + 4] == b"\x1f\x8b\x08\x04" and data[at + 10:at + 18] == b"\x06\x00BC\x02\x00" + data[at + 16:at + 18], at
        total = struct.unpack("<H", data[at + 16:at + 18])[0] + 1
        out.append((at, total, struct.unpack("<I", data[at + total - 4:at + total])[0]))
        at += total
    assert at == len(data)
    return out


def _statement_piece(piece):
    text, blocks = B.inflate_file(piece)
    return text, [b["types"] for b in blocks]


def statement(data):
    """tests/bgzf_statement.py's inflate_file on the file: (text, the deflate block types of every BGZF block).  The statement
    inflates about a third of a megabyte a second and BGZF blocks are independent, so a long file is cut at block boundaries and its
    pieces -- each a BGZF file -- go through the statement in several processes."""
    if len(data) < 1 << 20:
        return _statement_piece(data)
    blocks = blocks_of(data)
    pieces = [data[blocks[k][0]:blocks[min(k + 8, len(blocks)) - 1][0] + blocks[min(k + 8, len(blocks)) - 1][1]] for k in range(0, len(blocks), 8)]
    import multiprocessing as mp
    with mp.get_context("fork").Pool(min(16, _io.usable_cpus())) as pool:
        res = pool.map(_statement_piece, pieces, chunksize=4)
    return b"".join(r[0] for r in res), [t for r in res for t in r[1]]


def check(name, text, out):
    """what the issue asks of every output; returns the deflate block types of its blocks"""
    assert out[-28:] == bgzf.EOF_MARKER, name
    blocks = blocks_of(out)
    assert len(blocks) == (len(text) + BLOCK - 1) // BLOCK + 1, name
    assert all(total <= 65536 and isize <= BLOCK for _, total, isize in blocks), name
    assert [isize for _, _, isize in blocks[:-1]] == [min(BLOCK, len(text) - at) for at in range(0, len(text), BLOCK)], name
    assert gzip.decompress(out) == text, name
    got, types = statement(out)
    assert got == text, name
    assert all(t in ([0], [1]) for t in types[:-1]), (name, types[:4])          # one deflate block each: stored, or fixed codes
    return types[:-1]
