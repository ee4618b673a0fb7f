"""A deflate writer that covers RFC 1951, for tests/test_bgzf_generated.py and tests/test_gpu_bgzf_generated.py: token lists (literals
and (length, distance) pairs) become raw deflate -- stored, fixed and dynamic blocks joined at any bit offset by one BitWriter --, every
stream carries a `features` record of what it really emitted, and corpus() holds every item of FEATURES (the coverage test asserts it).
mutants() damages a stream (seeded bit flip, cut, appended byte), directed() builds the errors random damage does not reach, and the
files for the CRC kernel's coverage and the upload's chunk edges are built here too.  Everything is seeded and made at test time.

One item of the format cannot occur in a good stream: HCLEN 4 sends lengths for the code-length symbols 16, 17, 18 and 0 only, so
every literal/length length is 0, the end-of-block code is missing and zlib refuses the block.  It is in directed(); the smallest HCLEN
of a good stream is 5 (every code of 8 bits: 255 literals and the end-of-block code, no distance code), which corpus() holds."""
import collections
import functools
import struct
import zlib

import numpy as np

import bgzf_statement as B
from bgzf_fixtures import BitWriter, codes_of, patched, text
from bgzf_fixtures import raw as F_raw
from m6anet_amd import bgzf

GRID_D = (1, 2, 3, 4, 5, 7, 63, 64, 65, 127, 129)
GRID_L = (3, 4, 63, 64, 65, 127, 128, 129, 257, 258)
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
CHUNK = 4096

FEATURES = (["ll_bits_15", "dist_bits_15", "cl_bits_7", "unused_literal_length_code", "unused_distance_code", "hlit_257", "hlit_286", "hdist_1",
             "hdist_30", "hclen_5", "hclen_19", "single_distance_code", "single_distance_code_used", "no_distance_code", "lengths_plain",
             "lengths_rle", "rep16_3", "rep16_6", "rep17_3", "rep17_10", "rep18_11", "rep18_138", "rep16_crosses_into_distance_lengths",
             "len_258_as_284", "dist_eq_pos", "types_mixed", "match_into_stored", "empty_fixed_block", "empty_final_block", "isize_0",
             "isize_1", "isize_65535", "isize_65536"]
            + ["len_sym_%d_%s" % (s, e) for s in range(257, 286) for e in ("lo", "hi")]
            + ["dist_sym_%d_%s" % (s, e) for s in range(30) for e in ("lo", "hi")]
            + ["grid_%d_%d" % (d, n) for d in GRID_D for n in GRID_L]
            + ["sync_flush_at_bit_%d" % k for k in range(8)])

Stream = collections.namedtuple("Stream", "name body data features")


def member(s, crc=None, isize=None):
    """the stream as one BGZF block"""
    return bgzf.wrap(s.body, zlib.crc32(s.data) if crc is None else crc, len(s.data) if isize is None else isize)


def draw_lengths(rng, n, cap=15, deep=False):
    """the lengths of a complete code of n >= 2 symbols, drawn by splitting leaves; deep: from the chain 1, 2, .., cap - 1, cap, cap"""
    leaves = list(range(1, cap)) + [cap, cap] if deep else [1, 1]
    assert len(leaves) <= n <= 1 << cap
    while len(leaves) < n:
        can = [i for i, d in enumerate(leaves) if d < cap]
        i = can[int(rng.integers(len(can)))]
        leaves[i] += 1
        leaves.append(leaves[i])
    return leaves


def spread(rng, size, symbols, lengths):
    out = [0] * size
    for s, n in zip(symbols, rng.permutation(lengths)):
        out[s] = int(n)
    return out


def rle_ops(seq, mode, rng):
    """the code-length symbols that send seq: [(symbol, extra value, extra bits, index in seq, lengths sent)]; mode plain (each length
    as itself), max (the longest repeats) or random"""
    ops, i = [], 0
    while i < len(seq):
        v, j = seq[i], i
        while j < len(seq) and seq[j] == v:
            j += 1
        if mode == "plain":
            ops += [(v, 0, 0, k, 1) for k in range(i, j)]
            i = j
            continue
        if v:
            ops.append((v, 0, 0, i, 1))
            i += 1
        while i < j:
            left = j - i
            lo, hi, sym = (11, 138, 18) if v == 0 and left >= 11 else (3, 10, 17) if v == 0 and left >= 3 else (3, 6, 16) if v and left >= 3 else (1, 1, v)
            if mode == "random" and sym == 18 and rng.integers(4) == 0:
                lo, hi, sym = 3, 10, 17
            rep = min(left, hi) if mode == "max" else int(rng.integers(lo, min(left, hi) + 1))
            if sym < 16 or (mode == "random" and rng.integers(8) == 0):
                ops.append((v, 0, 0, i, 1))
                i += 1
                continue
            ops.append((sym, rep - lo, {16: 2, 17: 3, 18: 7}[sym], i, rep))
            i += rep
    return ops


class Deflate:
    """one member: deflate blocks appended through one bit-writer, the output they expand to, and what was emitted.  Tokens: a literal
    byte, (length, distance), (258, distance, 284) for the length spelled as symbol 284 + 31, and for damaged streams ("L", symbol) /
    ("D", symbol) -- that symbol's code alone -- and ("bits", value, n)."""

    def __init__(self, rng):
        self.rng, self.w, self.data, self.features, self.kinds, self.stored_at = rng, BitWriter(), bytearray(), set(), [], []
        self.valid = True

    def header(self, last, kind):
        self.w.bits(last, 1).bits(kind, 2)
        self.kinds.append(kind)

    def stored(self, data, last=0, nlen_xor=0xffff):
        if not data and self.kinds and self.kinds[-1] in (1, 2):
            self.features.add("sync_flush_at_bit_%d" % self.w.cnt)
        self.header(last, 0)
        if self.w.cnt:
            self.w.bits(0, 8 - self.w.cnt)
        for v in struct.pack("<HH", len(data), len(data) ^ nlen_xor) + bytes(data):
            self.w.bits(v, 8)
        if last and not data:
            self.features.add("empty_final_block")
        self.stored_at.append((len(self.data), len(self.data) + len(data)))
        self.data += data
        return self

    def tokens(self, tokens, lc, dc, eob=True):
        w, f, used_l, used_d = self.w, self.features, {256}, set()
        for t in tokens:
            if isinstance(t, int):
                w.code(*lc[t])
                self.data.append(t)
                used_l.add(t)
                continue
            if t[0] in ("L", "D"):
                w.code(*(lc if t[0] == "L" else dc)[t[1]])
                self.valid = False
                continue
            if t[0] == "bits":
                w.bits(t[1], t[2])
                self.valid = False
                continue
            n, d, pos = t[0], t[1], len(self.data)
            s = t[2] - 257 if len(t) > 2 else max(i for i in range(29) if B.LBASE[i] <= n and (i < 28 or n == 258))
            x = n - B.LBASE[s]
            assert 0 <= x < 1 << B.LEXT[s] and 3 <= n <= 258
            w.code(*lc[257 + s]).bits(x, B.LEXT[s])
            used_l.add(257 + s)
            if s == 27 and n == 258:
                f.add("len_258_as_284")
            f.update("len_sym_%d_%s" % (257 + s, e) for e, edge in (("lo", 0), ("hi", (1 << B.LEXT[s]) - 1)) if x == edge)
            s = max(i for i in range(30) if B.DBASE[i] <= d)
            x = d - B.DBASE[s]
            assert 0 <= x < 1 << B.DEXT[s]
            w.code(*dc[s]).bits(x, B.DEXT[s])
            used_d.add(s)
            f.update("dist_sym_%d_%s" % (s, e) for e, edge in (("lo", 0), ("hi", (1 << B.DEXT[s]) - 1)) if x == edge)
            if d > pos:                                   # a damaged stream: what follows is never produced
                self.valid = False
                continue
            if d == pos:
                f.add("dist_eq_pos")
            if d in GRID_D and n in GRID_L:
                f.add("grid_%d_%d" % (d, n))
            if any(lo < pos - d + min(n, d) and pos - d < hi for lo, hi in self.stored_at):
                f.add("match_into_stored")
            for _ in range(n):
                self.data.append(self.data[-d])
        if eob:
            w.code(*lc[256])
        return used_l, used_d

    def fixed(self, tokens, last=0):
        self.header(last, 1)
        before = len(self.data)
        self.tokens(tokens, codes_of(FIXED_LL), codes_of([5] * 32))
        if len(self.data) == before:
            self.features.add("empty_final_block" if last else "empty_fixed_block")
        return self

    def dynamic(self, tokens, ll, dd, last=0, rle="max", cl_deep=False, hclen=None, edit=None, eob=True):
        """ll, dd: the code lengths as sent (257..286 and 1..30 of them); edit(ops) -> ops damages how they are sent"""
        f, rng = self.features, self.rng
        self.header(last, 2)
        before = len(self.data)
        ops = rle_ops(list(ll) + list(dd), rle, rng)
        if edit:
            ops = edit(ops)
            self.valid = False
        need = sorted({o[0] for o in ops})
        while len(need) < (8 if cl_deep else 2):          # a code-length code is complete: two symbols at least, eight for 7 bits
            need.append(next(s for s in (0, 8, 7, 9, 6, 10, 5, 11, 4) if s not in need))
        cl = spread(rng, 19, need, draw_lengths(rng, len(need), 7, cl_deep))
        ncode = max(4, max(i + 1 for i, s in enumerate(B.ORDER) if cl[s]))
        ncode = max(ncode, hclen or 0)
        self.w.bits(len(ll) - 257, 5).bits(len(dd) - 1, 5).bits(ncode - 4, 4)
        for s in B.ORDER[:ncode]:
            self.w.bits(cl[s], 3)
        cc = codes_of(cl)
        for sym, x, nx, at, rep in ops:
            self.w.code(*cc[sym]).bits(x, nx)
            if sym >= 16:
                f.add("rep%d_%d" % (sym, rep))
            if sym == 16 and at < len(ll) < at + rep:
                f.add("rep16_crosses_into_distance_lengths")
        f.add("lengths_rle" if any(o[0] >= 16 for o in ops) else "lengths_plain")
        f.update(name for name, hit in (("hlit_%d" % len(ll), len(ll) in (257, 286)), ("hdist_%d" % len(dd), len(dd) in (1, 30)),
                                        ("hclen_%d" % ncode, ncode in (5, 19)), ("cl_bits_7", max(cl) == 7), ("ll_bits_15", max(ll) == 15),
                                        ("dist_bits_15", max(dd) == 15), ("no_distance_code", not any(dd)),
                                        ("single_distance_code", sorted(dd)[-2:] in ([1], [0, 1]))) if hit)
        used_l, used_d = self.tokens(tokens, codes_of(ll), codes_of(dd), eob)
        if {s for s, n in enumerate(ll) if n} - used_l:
            f.add("unused_literal_length_code")
        if {s for s, n in enumerate(dd) if n} - used_d:
            f.add("unused_distance_code")
        if used_d and "single_distance_code" in f and sum(dd) == 1:
            f.add("single_distance_code_used")
        if last and len(self.data) == before:
            f.add("empty_final_block")
        return self

    def done(self, name):
        f = self.features
        if len(self.data) in (0, 1, 65535, 65536):
            f.add("isize_%d" % len(self.data))
        if set(self.kinds) == {0, 1, 2}:
            f.add("types_mixed")
        return Stream(name, self.w.done(), bytes(self.data), frozenset(f) if self.valid else frozenset())


def sets_for(rng, tokens, deep=False, hlit=None, hdist=None, unused=0, single=True):
    """drawn code lengths (ll, dd) that hold every symbol the tokens use, and `unused` symbols more"""
    used_l, used_d = {256}, set()
    for t in tokens:
        if isinstance(t, int):
            used_l.add(t)
        elif isinstance(t[0], int):
            used_l.add(t[2] if len(t) > 2 else 257 + max(i for i in range(29) if B.LBASE[i] <= t[0] and (i < 28 or t[0] == 258)))
            used_d.add(max(i for i in range(30) if B.DBASE[i] <= t[1]))
    nlen = hlit or int(rng.integers(max(used_l | {256}) + 1, 287))
    ndist = hdist or int(rng.integers(max(used_d | {0}) + 1, 31))
    out = []
    for used, size, least in ((used_l, nlen, 16 if deep else 1), (used_d, ndist, 16 if deep else 0)):
        syms = sorted(used)
        spare = [int(s) for s in rng.permutation(size) if s not in used]
        want = max(least, len(syms) + unused) if syms else 0
        syms += spare[:max(0, min(want, size) - len(syms))]
        if len(syms) == 1 and (spare and not single):
            syms.append(spare[0])
        if len(syms) <= 1:                                # no code at all, or the single code of one bit
            out.append([1 if s in syms else 0 for s in range(size)])
        else:
            out.append(spread(rng, size, syms, draw_lengths(rng, len(syms), 15, deep and len(syms) >= 16)))
    return out


def random_tokens(rng, pos, n_out):
    some = rng.permutation(256)[:int(rng.choice([1, 2, 5, 20, 90, 256]))]
    tokens, end = [], pos + n_out
    while pos < end:
        if pos and end - pos >= 3 and rng.integers(5) < 2:
            d = int(rng.choice([1, 2, 3, int(rng.integers(1, 66)), pos, int(rng.integers(1, pos + 1))]))
            n = int(rng.choice([3, 4, 63, 64, 65, 127, 128, 129, 257, 258, int(rng.integers(3, 259))]))
            tokens.append((min(n, end - pos), min(d, pos, 32768)))
            pos += tokens[-1][0]
        else:
            tokens.append(int(some[rng.integers(len(some))]))
            pos += 1
    return tokens


def random_stream(rng, name):
    z = Deflate(rng)
    n = int(rng.integers(1, 4))
    for b in range(n):
        last, kind = int(b == n - 1), int(rng.choice([0, 1, 2, 2, 2]))
        if kind == 0:
            z.stored(rng.integers(0, 256, int(rng.integers(0, 300)), dtype=np.uint8).tobytes(), last)
            continue
        tokens = random_tokens(rng, len(z.data), int(rng.choice([0, 1, 40, 300, 1500])))
        if kind == 1:
            z.fixed(tokens, last)
        else:
            ll, dd = sets_for(rng, tokens, deep=rng.integers(4) == 0, unused=int(rng.integers(0, 12)), single=rng.integers(2) == 0)
            z.dynamic(tokens, ll, dd, last, rle=str(rng.choice(["plain", "max", "random", "random"])), cl_deep=rng.integers(4) == 0,
                      hclen=19 if rng.integers(6) == 0 else None)
    return z.done(name)


def filler(rng, pos, upto):
    """tokens that bring an output of `pos` bytes to `upto`: literals up to 300 bytes, then matches of every length at any distance"""
    tokens = []
    while pos < upto:
        if pos < 300 or upto - pos < 3:
            tokens.append(int(rng.integers(0, 256)))
            pos += 1
        else:
            n = min(upto - pos, int(rng.choice([258, 258, 258, int(rng.integers(3, 259))])))
            tokens.append((n, int(rng.integers(1, min(pos, 32768) + 1))))
            pos += n
    return tokens


def directed_good(rng):
    """the streams that reach the listed edges on purpose"""
    out = []
    lits = lambda n: [int(v) for v in rng.integers(0, 256, n)]        # noqa: E731

    # every length symbol at both ends of its extra bits, 258 as 284 + 31 too; in a fixed and in a deep dynamic block
    t = lits(2)
    for s in range(29):
        for x in sorted({0, (1 << B.LEXT[s]) - 1}):
            n = B.LBASE[s] + x
            t += [(n, 1 + (s + x) % 2, 284) if (s, n) == (27, 258) else (n, 1 + (s + x) % 2)] + lits(1)
    out.append(Deflate(rng).fixed(t, 1).done("length_symbols_fixed"))
    ll, dd = sets_for(rng, t, deep=True, hlit=286, hdist=30)
    out.append(Deflate(rng).dynamic(t, ll, dd, 1).done("length_symbols_deep"))
    # 7 bits in the code-length code, 15 in neither alphabet (a code of 7 bits sends eight different lengths at most)
    ll, dd = [0] * 257, [2, 2, 2, 2]
    for s, n in zip([65, 66, 67, 68, 69, 70, 256], [1, 2, 3, 4, 5, 6, 6]):
        ll[s] = n
    out.append(Deflate(rng).dynamic([65, 66, 67, 68, 69, 70, 65], ll, dd, 1, rle="plain", cl_deep=True).done("code_length_code_7_bits"))

    # every distance symbol at both ends, in the member of 65536 bytes; 15 bits in both alphabets, HLIT 286, HDIST 30
    t, pos = filler(rng, 0, 300), 300
    for s in range(30):
        for x in sorted({0, (1 << B.DEXT[s]) - 1}):
            d = B.DBASE[s] + x
            if d > pos:
                more = [(258, int(rng.integers(1, pos + 1)))] * ((d - pos + 257) // 258)
                t += more
                pos += 258 * len(more)
            t.append((3 + (s + x) % 5, d))
            pos += t[-1][0]
    t += filler(rng, pos, 65536)
    ll, dd = sets_for(rng, t, deep=True, hlit=286, hdist=30)
    out.append(Deflate(rng).dynamic(t, ll, dd, 1, rle="random").done("distance_symbols_65536"))
    # 65535 bytes: a stored block, then a fixed block whose matches reach back into it
    z = Deflate(rng).stored(rng.integers(0, 256, 30000, dtype=np.uint8).tobytes())
    out.append(z.fixed(filler(rng, 30000, 65535), 1).done("stored_then_fixed_65535"))

    # how the lengths are sent: each repeat code at its smallest and largest count (see the runs in ll)
    ll = [0] * 138 + [5] * 7 + [0] * 11 + [5] * 4 + [0] * 10 + [5] + [0] * 3 + [5] + [0] * 81 + [1, 5, 4]
    assert len(ll) == 259 and B.code_of(ll)[1] == 0
    out.append(Deflate(rng).dynamic([138, 144, 156, 170, 174, (3, 1), 138], ll, [1, 1], 1).done("repeat_codes_at_their_ends"))
    # a 16 whose run starts in the literal/length lengths and ends in the distance lengths
    ll = [0] * 286
    for sym, n in ((65, 2), (66, 2), (67, 3), (68, 3), (69, 4), (70, 4), (256, 4), (284, 5), (285, 5)):
        ll[sym] = n
    dd = [5, 5, 5, 5, 1, 2, 3]
    assert B.code_of(ll)[1] == 0 and B.code_of(dd)[1] == 0
    some = [65, 66, 67, 68, 69, 70]
    out.append(Deflate(rng).dynamic(some + [(258, 2)] + some, ll, dd, 1).done("repeat_runs_into_the_distance_lengths"))

    # the ends of HLIT, HDIST and HCLEN; the single distance code; no distance code
    t = lits(40)
    ll, dd = sets_for(rng, t, hlit=257, hdist=1)
    out.append(Deflate(rng).dynamic(t, ll, dd, 1, hclen=19).done("hlit_257_hdist_1_hclen_19_no_distance_code"))
    ll = [8] * 255 + [0, 8]
    out.append(Deflate(rng).dynamic([v % 255 for v in lits(30)], ll, [0], 1).done("hclen_5"))
    t = [7, (258, 1), (3, 1), 9]
    ll, dd = sets_for(rng, t, hlit=286, hdist=1)
    out.append(Deflate(rng).dynamic(t, ll, dd, 1).done("single_distance_code_hdist_1"))
    t = [7, 8, 9, (64, 3), (129, 3)]
    ll, dd = sets_for(rng, t, hdist=30, unused=5)
    out.append(Deflate(rng).dynamic(t, ll, dd, 1).done("few_distance_codes_hdist_30"))
    out.append(Deflate(rng).dynamic([], [0] * 256 + [1], [0], 1).done("single_end_of_block_code"))

    # a distance equal to the bytes produced so far, at every small count
    for k in (1, 2, 3, 63, 64, 65, 300):
        t = lits(k) + [(258, k)] + lits(1) + [(3, k + 259)]
        ll, dd = sets_for(rng, t)
        out.append(Deflate(rng).dynamic(t, ll, dd, 1, rle="random").done("distance_is_position_%d" % k))

    # members of several deflate blocks
    z = Deflate(rng).stored(bytes(lits(150)))
    z.fixed([(130, 150), 1, 2, (64, 3), (5, 200)])
    t = [(258, 281), 5, (100, 1), (65, 400)]
    ll, dd = sets_for(rng, t, unused=4)
    z.dynamic(t, ll, dd).stored(bytes(lits(7))).fixed([(7, 7), (258, 8)])
    out.append(z.stored(b"", 1).done("stored_fixed_dynamic_mixed"))
    for k in range(8):                                    # zlib's sync flush behind a Huffman block that ends at every bit offset
        for trial in range(256):
            z = Deflate(rng).fixed([65 + (trial >> b & 1) * 100 for b in range(8)] + [(4, 2)])
            if z.w.cnt == k:
                break
        assert z.w.cnt == k
        t = [(6, 3), 200, (3, 1)]
        ll, dd = sets_for(rng, t)
        out.append(z.stored(b"").dynamic(t, ll, dd, 1).done("sync_flush_at_bit_%d" % k))
    out.append(Deflate(rng).fixed([]).fixed([]).fixed(lits(3)).fixed([], 1).done("empty_fixed_blocks"))
    out.append(Deflate(rng).fixed([], 1).done("isize_0_fixed"))
    out.append(Deflate(rng).stored(b"", 1).done("isize_0_stored"))
    out.append(Deflate(rng).fixed([]).stored(b"").dynamic([], [0] * 256 + [1], [0], 1).done("isize_0_three_blocks"))
    out.append(Deflate(rng).fixed([0x41], 1).done("isize_1_fixed"))
    out.append(Deflate(rng).stored(b"\xff", 1).done("isize_1_stored"))
    return out


def grid_stream(rng, d, n):
    """`d` literals, the match at a distance equal to the bytes so far, a few literals, the same match again; dynamic or fixed by turns"""
    t = [int(v) for v in rng.integers(0, 256, d)] + [(n, d)] + [int(v) for v in rng.integers(0, 256, 3)] + [(n, d), 0x0a]
    z = Deflate(rng)
    if (GRID_D.index(d) + GRID_L.index(n)) % 2:
        return z.fixed(t, 1).done("grid_%d_%d" % (d, n))
    ll, dd = sets_for(rng, t, unused=3)
    return z.dynamic(t, ll, dd, 1, rle="random").done("grid_%d_%d" % (d, n))


@functools.lru_cache(maxsize=None)
def grid():
    rng = np.random.default_rng(20240702)
    return {(d, n): grid_stream(rng, d, n) for d in GRID_D for n in GRID_L}


N_RANDOM = 850


@functools.lru_cache(maxsize=None)
def corpus():
    """every good stream, in a fixed order"""
    rng = np.random.default_rng(20240701)
    out = directed_good(rng) + list(grid().values())
    return out + [random_stream(rng, "random_%d" % i) for i in range(N_RANDOM)]


def packed(streams, per=256):
    """[(file bytes, its text, its blocks)]: `per` members to a file, then the marker"""
    out = []
    for i in range(0, len(streams), per):
        part = streams[i:i + per]
        out.append((b"".join(member(s) for s in part) + bgzf.EOF_MARKER, b"".join(s.data for s in part), len(part) + 1))
    return out


# ---- damaged streams
Mutant = collections.namedtuple("Mutant", "name block")   # block: one BGZF block


def mutants(s, rng, n=6):
    """n seeded mutants of a stream: one bit of the stream or the footer flipped, the stream cut at a byte, or one byte appended"""
    out, crc, isize = [], zlib.crc32(s.data), len(s.data)
    for k in range(n):
        kind = int(rng.integers(0, 6))
        if kind < 4 or not s.body:
            whole = bytearray(s.body + struct.pack("<II", crc, isize))
            bit = int(rng.integers(0, 8 * len(whole)))
            whole[bit >> 3] ^= 1 << (bit & 7)
            body, (c, n_out) = bytes(whole[:-8]), struct.unpack("<II", whole[-8:])
            out.append(Mutant("%s/flip_%d" % (s.name, bit), bgzf.wrap(body, c, n_out)))
        elif kind == 4:
            cut = int(rng.integers(0, len(s.body)))
            out.append(Mutant("%s/cut_%d" % (s.name, cut), bgzf.wrap(s.body[:cut], crc, isize)))
        else:
            out.append(Mutant("%s/pad" % s.name, bgzf.wrap(s.body + bytes([int(rng.integers(0, 256))]), crc, isize)))
    return out


def directed():
    """the errors that random damage does not reach, each alone in its member and behind a fixed block that shifts it by some bits"""
    rng = np.random.default_rng(20240703)
    out = []

    def both(name, build, isize=0):
        for shifted in (0, 1, 2):
            z = Deflate(rng)
            if shifted:
                z.fixed([66, 200][:shifted] + [67])
            build(z)
            s = z.done(name)
            out.append(Mutant("directed/%s_%d" % (name, shifted), bgzf.wrap(s.body + b"\0\0", 0, isize + len(s.data))))

    for sym in (286, 287):
        both("literal_length_code_%d" % sym, lambda z: z.fixed([65, ("L", sym)], 1))
    for sym in (30, 31):
        both("distance_code_%d" % sym, lambda z: z.fixed([65, ("L", 257), ("D", sym)], 1), 3)
    ll = [0] * 258
    ll[65], ll[256], ll[257] = 1, 2, 2
    both("unused_code_of_a_single_distance_code", lambda z: z.dynamic([65, ("L", 257), ("bits", 1, 1)], ll, [1], 1), 3)
    both("first_code_length_symbol_16", lambda z: z.dynamic([65], ll, [1], 1, edit=lambda ops: [(16, 0, 2, 0, 3)] + ops[1:]))
    both("repeat_past_hlit_and_hdist", lambda z: z.dynamic([65], ll, [1], 1, edit=lambda ops: ops[:-1] + [(16, 3, 2, 0, 6)]))
    both("zero_repeat_past_hlit_and_hdist", lambda z: z.dynamic([65], ll, [0], 1, edit=lambda ops: ops[:-1] + [(18, 127, 7, 0, 138)]))
    no_eob = list(ll)
    no_eob[256], no_eob[66] = 0, 2
    both("zeroed_end_of_block_length", lambda z: z.dynamic([65, 66], no_eob, [1], 1, eob=False))
    both("hclen_4", lambda z: z.dynamic([], [0] * 257, [0], 1, eob=False, edit=lambda ops: ops))
    both("distance_one_byte_too_far", lambda z: z.fixed([65, 66, 67, (3, len(z.data) + 4)], 1))

    def too_far(z):
        d = len(z.data) + 2
        z.dynamic([65, (3, d)], ll, [0] * max(i for i in range(30) if B.DBASE[i] <= d) + [1], 1)
    both("distance_one_byte_too_far_dynamic", too_far)
    both("block_type_3", lambda z: z.header(1, 3))
    both("block_type_3_not_last", lambda z: z.header(0, 3))
    both("wrong_nlen", lambda z: z.stored(b"abcd", 1, nlen_xor=0xfffe))
    both("nlen_is_len", lambda z: z.stored(b"abcd", 1, nlen_xor=0))
    for s in corpus()[:40:4]:                             # ISIZE one off, the stream and the CRC as they were
        for delta in (-1, 1):
            if 0 <= len(s.data) + delta <= 65536:
                out.append(Mutant("directed/%s/isize_%+d" % (s.name, delta), member(s, isize=len(s.data) + delta)))
    return out


def header_level():
    """the reasons of the block chain, from the fixtures' patched()"""
    rng = np.random.default_rng(20240704)
    t = text(rng, 6000)
    out = []
    for i in range(3):
        g = bgzf.block(t[2000 * i:2000 * i + 2000])
        out += [Mutant("header/magic_%d" % i, patched(g, magic=True)), Mutant("header/bsize_small_%d" % i, patched(g, bsize=10 + i)),
                Mutant("header/bsize_%d" % i, patched(g, bsize=(65535, 30000, 40000)[i])),
                Mutant("header/isize_%d" % i, patched(g, isize=(65537, 70000, 0xffffffff)[i]))]
    return out


N_MUTANTS = 6


@functools.lru_cache(maxsize=None)
def all_mutants():
    rng = np.random.default_rng(20240705)
    out = []
    for s in corpus():
        out += mutants(s, rng, N_MUTANTS)
    return out + directed() + header_level()


@functools.lru_cache(maxsize=None)
def around():
    """(good block before a mutant, good block and the marker behind it, their text): small, so that a file costs what its mutant costs"""
    rng = np.random.default_rng(20240706)
    t = text(rng, 150)
    return bgzf.block(t[:80]), bgzf.block(t[80:]) + bgzf.EOF_MARKER, t


def in_file(m):
    g0, tail, _ = around()
    return g0 + m.block + tail


@functools.lru_cache(maxsize=None)
def verdicts():
    """the statement on every mutant in its file: [(offset, reason)], or None where the damage changed nothing the format reads"""
    out = []
    for m in all_mutants():
        try:
            B.inflate_file(in_file(m))
            out.append(None)
        except B.Bad as e:
            out.append((e.offset, e.reason))
    return out


def zlib_accepts(block):
    """zlib on one block: the stream ends where the footer starts, gives ISIZE bytes, and the CRC is the footer's"""
    hdr = 12 + struct.unpack("<H", block[10:12])[0]
    crc, isize = struct.unpack("<II", block[-8:])
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(block[hdr:-8])
    except zlib.error:
        return False
    return d.eof and not d.unused_data and len(out) == isize and zlib.crc32(out) == crc


def sample_by_reason(per_reason=21):
    """{reason or "accepted": indices into all_mutants()}: at most per_reason of each, by a fixed stride -- never fewer than 3"""
    by = collections.defaultdict(list)
    for i, v in enumerate(verdicts()):
        by[v[1] if v else "accepted"].append(i)
    out = {}
    for reason, idx in by.items():
        k = max(3, per_reason)
        out[reason] = idx if len(idx) <= k else [idx[j * len(idx) // k] for j in range(k)]
    return out


# ---- every output byte is under the CRC
CRC_SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 65505)


def stored_stream(data):
    """one final stored block"""
    return b"\x01" + struct.pack("<HH", len(data), len(data) ^ 0xffff) + data


def crc_positions(n):
    per = -(-n // 64)
    last = (n - 1) // per
    want = [0, n - 1, per - 1, per, per + 1, 31 * per, 63 * per - 1, 63 * per, last * per, n - 1]
    return sorted({p for p in want if 0 <= p < n})


@functools.lru_cache(maxsize=None)
def crc_cases():
    """{name: (data, [(position, file bytes)])}: one output byte flipped, the footer keeps the CRC of the data"""
    rng = np.random.default_rng(20240707)
    g0, tail, _ = around()
    out = {}
    for n in CRC_SIZES + ("compressible",):
        if n == "compressible":
            data, level = text(rng, 65536), 6
        else:
            data, level = rng.integers(0, 256, n, dtype=np.uint8).tobytes(), 0
        files = []
        for p in crc_positions(len(data)):
            flipped = bytearray(data)
            flipped[p] ^= 1 << int(rng.integers(0, 8))
            stream = F_raw(bytes(flipped)) if level else stored_stream(bytes(flipped))
            files.append((p, g0 + bgzf.wrap(stream, zlib.crc32(data), len(data)) + tail))
        out[str(n)] = (data, files)
    return out


# ---- the upload's chunk edges (M6A_PREP_CHUNK_KB=4)
SUB = b"XY" + struct.pack("<H", 5) + b"hello"


def stored_block(rng, total):
    """a BGZF block of `total` bytes in all, holding random stored bytes"""
    data = rng.integers(0, 256, total - 31, dtype=np.uint8).tobytes()
    b = bgzf.wrap(stored_stream(data), zlib.crc32(data), len(data))
    assert len(b) == total
    return b


@functools.lru_cache(maxsize=None)
def chunk_cases():
    """{name: file bytes}: good files whose second block's header, or footer, lies across the first chunk's end at each of its
    bytes; files that end on a chunk's last byte; and files cut inside a header or a body (the statement says which error)"""
    rng = np.random.default_rng(20240708)
    t = text(rng, 3000)
    second = bgzf.block(t[:700], extra_before=SUB, extra_after=SUB)
    assert 12 + struct.unpack("<H", second[10:12])[0] >= 30
    out = {}
    for k in range(41):
        out["header_at_%d" % k] = stored_block(rng, CHUNK - k) + second + bgzf.EOF_MARKER
    for k in range(9):
        out["footer_at_%d" % k] = stored_block(rng, CHUNK - (len(second) - 8 + k)) + second + bgzf.EOF_MARKER
    out["ends_on_a_chunk"] = stored_block(rng, CHUNK - 100) + stored_block(rng, CHUNK + 100)
    out["one_block_is_one_chunk"] = stored_block(rng, CHUNK)
    out["marker_ends_on_a_chunk"] = stored_block(rng, 2 * CHUNK - 28) + bgzf.EOF_MARKER
    hdr = 12 + struct.unpack("<H", second[10:12])[0]
    for first in (CHUNK - 5, CHUNK, 1000):
        a = stored_block(rng, first)
        for cut in (1, 4, 11, 12, 13, 20, hdr - 1):
            out["cut_in_header_%d_%d" % (first, cut)] = a + second[:cut]
        for cut in (hdr, hdr + 1, len(second) - 9, len(second) - 1):
            out["cut_in_body_%d_%d" % (first, cut)] = a + second[:cut]
    return out


@functools.lru_cache(maxsize=None)
def truncation_cases():
    """{name: file bytes}: a small file with subfields before and after BC, cut at every byte of its first header and at every byte
    from its last data block's footer to its end"""
    t = text(np.random.default_rng(20240709), 200)
    data = bgzf.block(t[:120], extra_before=SUB) + bgzf.block(t[120:], extra_before=SUB, extra_after=SUB) + bgzf.EOF_MARKER
    hdr = 12 + struct.unpack("<H", data[10:12])[0]
    return {"truncated_%d" % c: data[:c] for c in list(range(0, hdr + 2)) + list(range(len(data) - 38, len(data)))}


def statement_on(data):
    """the statement's text, or (offset, reason)"""
    try:
        return B.inflate_file(data)[0]
    except B.Bad as e:
        return e.offset, e.reason
