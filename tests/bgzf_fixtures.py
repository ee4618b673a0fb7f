"""Seeded BGZF files for tests/test_bgzf_statement.py and tests/test_gpu_bgzf.py: good ones named for the edge they reach (the
statement's report proves it), and the malformed set, one file per reason of tests/bgzf_statement.py with a good block before and
after the bad one.  zlib.compressobj(level, DEFLATED, -15, 9, strategy) makes the ordinary streams; a small bit-writer makes the ones
zlib never writes (a match at distance 32768 -- zlib stops at 32506 --, the malformed streams)."""
import functools
import struct
import zlib

import numpy as np

import bgzf_statement as B
import eventalign_gen as G
from m6anet_amd import bgzf


class BitWriter:
    def __init__(self):
        self.out, self.buf, self.cnt = bytearray(), 0, 0

    def bits(self, value, n):                    # n bits, least significant first (header fields, extra bits)
        self.buf |= value << self.cnt
        self.cnt += n
        while self.cnt >= 8:
            self.out.append(self.buf & 0xff)
            self.buf >>= 8
            self.cnt -= 8
        return self

    def code(self, code, n):                     # a Huffman code of n bits, most significant first
        for k in range(n - 1, -1, -1):
            self.bits(code >> k & 1, 1)
        return self

    def done(self):
        if self.cnt:
            self.out.append(self.buf & 0xff)
            self.buf = self.cnt = 0
        return bytes(self.out)


def flat_lengths(n):
    """a complete set of n code lengths: 2^L - n symbols of L - 1 bits, the rest of L bits"""
    L = max(1, (n - 1).bit_length())
    k = (1 << L) - n
    return [L - 1] * k + [L] * (n - k)


def codes_of(lengths):
    """{symbol: (code, bits)}, canonical (RFC 1951 3.2.2)"""
    out, code = {}, 0
    for n in range(1, 16):
        for s, m in enumerate(lengths):
            if m == n:
                out[s] = (code, n)
                code += 1
        code <<= 1
    return out


def put_lengths(w, litlen, dist, cl_lengths=None):
    """the header of a dynamic block: every length sent as itself through a code-length code of sixteen 4-bit codes (or cl_lengths)"""
    cl = cl_lengths or [4] * 16 + [0] * 3
    w.bits(len(litlen) - 257, 5).bits(len(dist) - 1, 5).bits(15, 4)
    for s in B.ORDER:
        w.bits(cl[s], 3)
    cc = codes_of(cl)
    for n in list(litlen) + list(dist):
        w.code(*cc[n])


def dynamic_block(tokens, last=1, litlen=None, dist=None):
    """tokens: ints (literals) and (length, distance) pairs, as one dynamic deflate block with flat code lengths"""
    litlen, dist = litlen or flat_lengths(286), dist or flat_lengths(30)
    w = BitWriter().bits(last, 1).bits(2, 2)
    put_lengths(w, litlen, dist)
    lc, dc = codes_of(litlen), codes_of(dist)
    for t in tokens:
        if isinstance(t, int):
            w.code(*lc[t])
            continue
        n, d = t
        s = max(i for i in range(29) if B.LBASE[i] <= n and (i < 28 or n == 258))
        w.code(*lc[257 + s]).bits(n - B.LBASE[s], B.LEXT[s])
        s = max(i for i in range(30) if B.DBASE[i] <= d)
        w.code(*dc[s]).bits(d - B.DBASE[s], B.DEXT[s])
    w.code(*lc[256])
    return w.done()


def expand(tokens):
    out = bytearray()
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            for _ in range(t[0]):
                out.append(out[-t[1]])
    return bytes(out)


def raw(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return c.compress(data) + c.flush()


def text(rng, n):
    """compressible filler: eventalign-like lines"""
    rows = []
    while sum(map(len, rows)) < n:
        rows.append(b"ENST%05d\t%d\tGGACT\t%d\tt\t%d\t%.2f\t%.3f\t%.5f\n" % (rng.integers(0, 40), rng.integers(0, 3000), rng.integers(0, 500),
                                                                         rng.integers(0, 10 ** 6), rng.uniform(60, 130), rng.uniform(0.5, 9),
                                                                         rng.uniform(0.001, 0.05)))
    return b"".join(rows)[:n]


def far_match():
    """258 bytes, filler that repeats them, and a match of 258 at distance 32768 -- in a dynamic block"""
    tokens = list(range(256)) + [7, 9] + [(258, 258)] * 126 + [1, 2] + [(258, 32768)]
    data = expand(tokens)
    return bgzf.wrap(dynamic_block(tokens), zlib.crc32(data), len(data))


def two_deflate_blocks(rng):
    a, b = text(rng, 9000), text(rng, 7000)
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 9)
    body = c.compress(a) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(b) + c.flush()
    return bgzf.wrap(body, zlib.crc32(a + b), len(a + b))


@functools.lru_cache(maxsize=None)
def good():
    """{name: file bytes}"""
    rng = np.random.default_rng(20240611)
    t = text(rng, 40000)
    sub = b"XY" + struct.pack("<H", 5) + b"hello"
    out = {
        "eof_only": bgzf.block(b""),
        "stored": bgzf.block(rng.integers(0, 256, 65280, dtype=np.uint8).tobytes(), level=0) + bgzf.EOF_MARKER,
        "fixed": bgzf.block(t[:20000], strategy=zlib.Z_FIXED) + bgzf.EOF_MARKER,
        "dynamic": bgzf.block(t) + bgzf.EOF_MARKER,
        "all_A": bgzf.block(b"A" * 65536) + bgzf.EOF_MARKER,
        "far_match": far_match() + bgzf.EOF_MARKER,
        "two_deflate_blocks": two_deflate_blocks(rng) + bgzf.EOF_MARKER,
        "extra_subfields": bgzf.block(t[:5000], extra_before=sub) + bgzf.block(t[5000:9000], extra_after=sub) + bgzf.EOF_MARKER,
        "empty_in_the_middle": bgzf.block(t[:3000]) + bgzf.EOF_MARKER + bgzf.block(t[3000:6000]) + bgzf.EOF_MARKER,
        "no_eof_marker": bgzf.block(t[:3000]) + bgzf.block(t[3000:4000]),
        "small_300": b"".join(bgzf.block(t[97 * i:97 * i + 97]) for i in range(300)) + bgzf.EOF_MARKER,
    }
    for family in sorted(G.FAMILIES):
        out["family_" + family] = bgzf.compress(G.case(family, 1).data)
    return out


@functools.lru_cache(maxsize=None)
def inflated(name):
    """the statement's (text, blocks) of a good fixture, computed once"""
    return B.inflate_file(good()[name])


def fixed_stream(*parts):
    """a final fixed-Huffman block of (code, bits) / ("x", value, bits) parts"""
    w = BitWriter().bits(1, 1).bits(1, 2)
    for p in parts:
        if p[0] == "x":
            w.bits(p[1], p[2])
        else:
            w.code(*p)
    return w.done()


def patched(block, isize=None, crc_flip=False, cut=0, pad=b"", bsize=None, magic=False):
    """a good block with its ISIZE replaced, its CRC flipped, `cut` bytes off its stream's end or `pad` behind it, its BSIZE replaced"""
    hdr = 12 + struct.unpack("<H", block[10:12])[0]
    body, crc, n = block[hdr:-8], struct.unpack("<I", block[-8:-4])[0], struct.unpack("<I", block[-4:])[0]
    body = (body[:len(body) - cut] if cut else body) + pad
    out = bytearray(bgzf.wrap(body, crc ^ (1 if crc_flip else 0), n if isize is None else isize))
    if bsize is not None:
        out[16:18] = struct.pack("<H", bsize)
    if magic:
        out[1] = 0x8c
    return bytes(out)


@functools.lru_cache(maxsize=None)
def malformed():
    """{name: (file bytes, reason, index of the bad block)}: good, bad, good (+ the marker) -- or as the name says"""
    rng = np.random.default_rng(20240612)
    t = text(rng, 9000)
    g0, g1, g2 = bgzf.block(t[:3000]), bgzf.block(t[3000:6000]), bgzf.block(t[6000:])

    def mid(bad):
        return g0 + bad + g2 + bgzf.EOF_MARKER
    body = lambda stream, n=0: bgzf.wrap(stream, 0, n)      # noqa: E731
    lit_A, len3 = (0x30 + 65, 8), (1, 7)
    over = BitWriter().bits(1, 1).bits(2, 2)
    put_lengths(over, flat_lengths(286), flat_lengths(30), cl_lengths=[1] * 19)
    incomplete = flat_lengths(286)
    incomplete[0] += 1
    no_eob = [0] * 286
    no_eob[0] = no_eob[1] = 1
    sets = {}
    for name, ll in (("incomplete_set", incomplete), ("no_end_of_block", no_eob)):
        w = BitWriter().bits(1, 1).bits(2, 2)
        put_lengths(w, ll, flat_lengths(30))
        sets[name] = w.bits(0, 16).done()
    bad = {
        "bad_header": (patched(g1, magic=True), B.HEADER),
        "bsize_past_the_end": (patched(g1, bsize=65535), B.BSIZE),
        "isize_over": (patched(g1, isize=70000), B.ISIZE),
        "block_type_3": (body(BitWriter().bits(1, 1).bits(3, 2).done()), B.BTYPE),
        "stored_nlen": (body(b"\x01" + struct.pack("<HH", 4, 4) + b"abcd", 4), B.STORED),
        "oversubscribed_set": (body(over.bits(0, 16).done()), B.CODELEN),
        "incomplete_set": (body(sets["incomplete_set"]), B.CODELEN),
        "no_end_of_block": (body(sets["no_end_of_block"]), B.CODELEN),
        "symbol_286": (body(fixed_stream((0b11000110, 8), ("x", 0, 16))), B.SYMBOL),
        "distance_symbol_30": (body(fixed_stream(lit_A, len3, (30, 5), ("x", 0, 16)), 4), B.SYMBOL),
        "distance_too_far": (body(fixed_stream(lit_A, len3, (1, 5), (0, 7)), 4), B.DISTANCE),
        "output_beyond_isize": (patched(g1, isize=2999), B.OVERFLOW),
        "input_exhausted": (patched(g1, cut=1), B.INPUT),
        "trailing_byte": (patched(g1, pad=b"\0"), B.TRAILING),
        "length_not_isize": (patched(g1, isize=3001), B.LENGTH),
        "crc": (patched(g1, crc_flip=True), B.CRC),
    }
    out = {name: (mid(b), reason, 1) for name, (b, reason) in bad.items()}
    out["two_bad_blocks"] = (g0 + bad["crc"][0] + g1 + bad["block_type_3"][0] + g2 + bgzf.EOF_MARKER, B.CRC, 1)
    return out


def offset_of(data, index):
    """file offset of block `index`, by BSIZE alone"""
    at = 0
    for _ in range(index):
        hdr = 12 + struct.unpack("<H", data[at + 10:at + 12])[0]
        q = at + 12
        while data[q:q + 2] != b"BC":
            q += 4 + struct.unpack("<H", data[q + 2:q + 4])[0]
        assert q < at + hdr
        at += struct.unpack("<H", data[q + 4:q + 6])[0] + 1
    return at
