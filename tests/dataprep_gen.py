"""Seeded eventalign.txt files for the edges of dataprep's writers -- the host's (m6a_io.cpp) and the device's (m6a_dataprep.h, m6a_repr.h,
csv_emit in m6a_csv.h) -- built from tests/eventalign_gen.py's File and Tx: generate(family, seed) -> bytes, nothing stored, every
file under 1 MB.  The families live here and not in eventalign_gen.FAMILIES because a family's seed there is its place in the
sorted list of names: a new name would regenerate every other family.

FAMILIES[name] is eventalign_gen's shape: kw are the site filters.  case(family, seed) is the file with the statement's answers
(eventalign_gen.Case), for a family of either module; expected(family, seed, compress) is what every writer must write: the four
files as bytes and the count of values the device printer declines, from the two statements alone.

How the device cuts its text into rows, restated here from the header of m6a_csv.h and from the write kernels of m6a_dataprep.h so
that `long_names` can say what it holds:
    json_rows    a record is its reads; read 0 carries the head up to `":[`, every later read a leading comma, the last the tail
    index_rows   one per run
    offsets      a row's offset is its place in the round's buffer, which starts at byte 0 and which the default round size makes the
                 whole text.  For data.json that is the offset in the file.  For eventalign.index it is the offset in the text BEHIND
                 the header: the header is written by the host, and the buffer lands in the file after its 43 bytes, so there a row's
                 pad is not its file offset modulo 4.  (Under a small M6A_JSON_ROUND_KB offsets count from each round's first row, and
                 the tiles differ from those that TILE_EDGES speaks of.)
    batches      a wave takes up to 64 consecutive rows at a time, as many as fit TILE bytes behind a pad of (offset of the first) % 4;
                 a first row that does not fit goes out alone
"""
import functools

import numpy as np

import dataprep_json_statement as D
import eventalign_gen as G
import eventalign_statement as S
from eventalign_gen import File, Tx, site_reads, wide_reads

TILE, WAVE = 8192, 64
FILES = ("eventalign.index", "data.json", "data.info", "data.log")


# ---- the device's rows, from the statement's text ------------------------------------------------------------------------------
def json_rows(sites, round3=False):
    """[(offset in data.json, length)] per site: the rows of its reads"""
    out, at = [], 0
    for tx, pos, kmer7, features, reads in sites:
        rec = D.record(tx, pos, kmer7, features, reads, round3)
        one = [D.record(tx, pos, kmer7, [f], [r], round3) for f, r in zip(features, reads)]
        head = one[0].index("[[") + 1
        lens = [len(o) - head - 5 + (head if j == 0 else 1) + (5 if j == len(one) - 1 else 0) for j, o in enumerate(one)]
        assert sum(lens) == len(rec)
        out.append([(at + sum(lens[:j]), n) for j, n in enumerate(lens)])
        at += len(rec)
    return out


def index_rows(runs):
    """[(offset in the text of eventalign.index behind its header -- what index_write_kernel hands csv_emit --, length)] per run"""
    out, at = [], 0
    for r in runs:
        out.append((at, len(D.index_row(*r))))
        at += out[-1][1]
    return out


def batches(rows):
    """one wave's rows [(offset, length)] -> [(pad, [lengths])]: the tiles it stages, a row of its own where it exceeds one"""
    out, a = [], 0
    while a < len(rows):
        pad, b = rows[a][0] % 4, a
        while b < min(len(rows), a + WAVE) and pad + sum(n for _, n in rows[a:b + 1]) <= TILE:
            b += 1
        b = max(b, a + 1)
        out.append((pad, [n for _, n in rows[a:b]]))
        a = b
    return out


def index_waves(rows):
    return [rows[a:a + WAVE] for a in range(0, len(rows), WAVE)]


def tile_edges(waves):
    """what the waves' batches hold, as a set of words:
        fits_8192         a batch whose first row has pad + length = TILE: the last that fits
        pad_8193          a first row with pad + length = TILE + 1 at a pad that is not 0: it fails only by the pad
        over_<pad>        a first row of more than TILE bytes at that pad
        long_after_short  such a row behind shorter rows of the same wave
        pair              two long rows share a tile and three do not.  Either the batch holds exactly two rows of over 4 000 bytes
                          (a third such row can never fit), whatever short rows surround them; or it holds exactly two rows, the
                          first of over 7 000 bytes, and is not its wave's last batch, so the row behind them was there and did not fit"""
    seen = set()
    for rows in waves:
        bs = batches(rows)
        for k, (pad, lens) in enumerate(bs):
            if pad + lens[0] == TILE:
                seen.add("fits_8192")
            if pad and pad + lens[0] == TILE + 1:
                seen.add("pad_8193")
            if lens[0] > TILE:
                seen.add("over_%d" % pad)
                if k > 0:
                    seen.add("long_after_short")
            if sum(n > 4000 for n in lens) == 2 or (len(lens) == 2 and lens[0] > 7000 and k + 1 < len(bs)):
                seen.add("pair")
    return seen


TILE_EDGES = {"fits_8192", "pad_8193", "over_0", "over_1", "over_2", "over_3", "pair", "long_after_short"}


# ---- long_names ----------------------------------------------------------------------------------------------------------------------
def name_of(t, n):
    """a name of n bytes (of at least 3) that no other transcript has and that repeats nowhere: a copy that slips by a byte shows"""
    head = "L%02dx" % t
    if n < len(head):
        return ("L%02d" % t)[:max(n, 3)]
    letters = "".join(chr(97 + (i * 7 + i // 26 + t) % 26) for i in range(n - len(head)))
    return head + letters


class Growing:
    """A File that grows by one transcript at a time, with the device offsets at which the next transcript's text will land: json_at
    in data.json, index_at in the index's text behind its header.  emit() appends a transcript, rows() says how the device will cut
    it, commit() moves the offsets past it; mark() and rewind() take an uncommitted transcript back (File has no undo: its state is
    the five fields below, and writing a line draws nothing from its generator)."""

    def __init__(self, rng):
        self.f, self.t, self.json_at, self.index_at = File(rng), 0, 0, 0
        self.bases = [int(10 ** int(rng.integers(0, 17))) + int(rng.integers(0, 9)) for _ in range(40)]

    def mark(self):
        f = self.f
        return (len(f.parts), f.size, f.clock, f.at, f.npad), (self.t, self.json_at, self.index_at)

    def rewind(self, mark):
        f = self.f
        (n, f.size, f.clock, f.at, f.npad), (self.t, self.json_at, self.index_at) = mark
        del f.parts[n:]

    def emit(self, n, reads, positions=3):
        """transcript number t under a name of n bytes, `reads` over `positions` positions around its one site; returns where it starts"""
        start = self.f.size
        tx = Tx(np.random.default_rng([self.t, 77]), name_of(self.t, n), 12, (3,), base=self.bases[self.t % len(self.bases)])
        for rd in reads:
            self.f.stretch(tx, tx.base + 2, positions, rd, events=(1, 2), mismatch=0)
        return start

    def rows(self, start):
        """of the transcript that starts at byte `start`: (json rows per site, index rows), at the offsets the device will give them"""
        names, runs = S.table(G.HEADER + b"".join(self.f.parts)[start:], 1)
        for r in runs:
            r["start"] += start - len(G.HEADER)
            r["end"] += start - len(G.HEADER)
        sites, rr, _ = D.from_eventalign(names, runs, min_segment_count=1)
        js = [[(a + self.json_at, n) for a, n in rows] for rows in json_rows(sites)]
        return js, [(a + self.index_at, n) for a, n in index_rows(rr)]

    def commit(self, start):
        js, xs = self.rows(start)
        self.json_at += sum(n for rows in js for _, n in rows)
        self.index_at += sum(n for _, n in xs)
        self.t += 1

    def plain(self, n, reads, positions=3):
        self.commit(self.emit(n, reads, positions))

    def search(self, lengths, reads, positions, first):
        """A short transcript, then one of `reads` whose name length moves, from `first` bytes on, until lengths(its json rows per
        site, its index rows) -> (a row's length now, the length wanted) agree; a changed name can change the digits of the byte
        offsets the index prints, hence more than one step.  The short one's name length moves every later offset modulo 4: where
        lengths() gives None the pad does not serve, and the short name grows by a byte."""
        before = self.mark()
        for spacer in range(3, 40):
            self.rewind(before)
            self.plain(spacer, [5 + spacer, 60 + spacer, 600 + spacer])
            here, n = self.mark(), first
            for _ in range(6):
                self.rewind(here)
                start = self.emit(n, reads, positions)
                js, xs = self.rows(start)
                got = lengths(js, xs)
                if got is None:
                    break
                if got[0] == got[1]:
                    self.commit(start)
                    return
                n += got[1] - got[0]
        raise AssertionError("no name length found")

    def first_row(self, which, want, reads, positions, first):
        """a transcript whose first json row (`which` = 0) or first index row (1) has pad + length = want(pad); None: not at this pad"""
        def lengths(js, xs):
            at, n = js[0][0] if which == 0 else xs[0]
            return None if want(at % 4) is None else (n, want(at % 4) - at % 4)
        self.search(lengths, reads, positions, first)

    def two_of_three(self, reads, positions, first):
        """a site of three reads whose first tile holds its first two rows with 7 bytes to spare: the third does not fit"""
        def lengths(js, xs):
            (at, n), (_, second) = js[0][:2]
            return n, TILE - at % 4 - second - 7
        self.search(lengths, reads, positions, first)


def long_names(rng):
    """Transcripts of one to three reads whose name lengths are searched, one transcript after the other, until the statement's text
    holds every word of TILE_EDGES in data.json and again in eventalign.index (test_dataprep_files_statement.py asserts it from the
    whole file).  Every transcript with a target follows a short one whose name length moves the offsets modulo 4."""
    g = Growing(rng)
    g.plain(3, [1, 2])
    g.plain(4070, [11, 12, 13], 1)                                         # eventalign.index: two rows of 4 090 bytes share a tile, three do not
    for which in (0, 1):
        reads, positions = ([7], 3) if which == 0 else ([7, 8], 1)
        g.first_row(which, lambda pad: TILE, reads, positions, 8000)
        g.first_row(which, lambda pad: TILE + 1 if pad else None, reads, positions, 8000)
        for p in range(4):
            g.first_row(which, lambda pad, p=p: p + TILE + 9 + 50 * p if pad == p else None, reads, positions, 8100)
    g.two_of_three([3, 4, 5], 3, 7900)                                     # data.json: two rows share a tile and three do not
    g.plain(5, [1, 2, 3])
    g.plain(12000 + int(rng.integers(0, 50)), [9])                         # a line longer than two blocks of the scan
    g.plain(7, [4, 5])
    return g.f.bytes()


# ---- wide values -----------------------------------------------------------------------------------------------------------------------
def spread_reads(rng, n, must=()):
    """n distinct read indices in [0, 2^53), of every digit count from 1 to 16"""
    out = list(must)
    seen = set(out)
    while len(out) < n:
        d = int(rng.integers(1, 17))
        v = int(rng.integers(10 ** (d - 1) if d > 1 else 0, min(10 ** d, 2 ** 53)))
        if v not in seen:
            seen.add(v)
            out.append(v)
    return [out[i] for i in rng.permutation(n)]


def big_site(rng):
    """one site of 3 000 reads whose indices the device prints: 47 passes of a wave over the tile, a record far larger than a small round"""
    f = File(rng)
    tx = Tx(rng, "BIG", 8, (2,))
    for rd in spread_reads(rng, 3000, (0, 2 ** 53 - 1)):
        f.stretch(tx, 1, 3, rd, events=(1, 2), mismatch=0)
    return f.bytes()


WIDE_16 = [-1, 2 ** 53, -2 ** 63, 2 ** 63 - 1]


def index_wide(rng):
    """a kept site in two segments; between them a transcript of 16 reads at one site -- fewer than min_segment_count, so no value of
    data.json is declined -- whose read indices fill 64 bits: eventalign.index prints them"""
    f = File(rng)
    tx = Tx(rng, "IWA", 12, (3,), base=int(rng.integers(0, 5000)))
    wide = Tx(rng, "IWB", 12, (3,))
    site_reads(f, tx, tx.base + 3, range(12), mismatch=0)
    reads = wide_reads(rng, 12) + WIDE_16
    site_reads(f, wide, 3, [reads[i] for i in rng.permutation(16)], mismatch=0)
    site_reads(f, tx, tx.base + 3, range(12, 24), mismatch=0)
    return f.bytes()


def big_positions(rng):
    """eventalign_gen.split_rows with read indices the device prints: 18-digit and single-digit positions in "<pos>" and data.info"""
    f = File(rng)
    bases = [3, 10 ** 17 + int(rng.integers(0, 10 ** 9)), int(rng.integers(10 ** 8, 10 ** 9)), 9 * 10 ** 17]
    txs = [Tx(rng, "BP%d" % t, 16, (2, 9), base=bases[t]) for t in range(4)]
    reads = [spread_reads(rng, 22) for _ in txs]
    for k in range(22):
        for t in rng.permutation(4):
            f.stretch(txs[t], txs[t].base + 1, 10, reads[t][k], mismatch=0)
    return f.bytes()


# ---- the printer's value edges, from text ------------------------------------------------------------------------------------------------
# spellings inside the front half's fast path (digits [. digits], at most 15 digit characters)
TAKEN = ["0.0015", "0.0025", "2.675", "1.0005", "999999999999999", "9999999999999.99", "123456789.012345", ".5", "5."]
ROUNDED_AWAY = ["0.0001", "0.00010000000001", "0.0005", "0.00025", "0.0004", "0.00049999"]      # taken plain, 0.0 after np.round(v, 3)
HOST_HALF = [("95.31000000000001", "0.30000000000000004", "0.012345678901234568"), ("95.3", "1.2345678901234567", ".5")]   # 17 digits


def values(spellings):
    def make(rng):
        """one event per position with end_idx = start_idx + 1: a feature is the value of its text.  event_stdv and event_length take
        every spelling in turn; reads 100 and 101 spell 17 significant digits, so the front half hands their runs to the host half"""
        f = File(rng)
        tx = Tx(rng, "VAL", 12, (3,))
        assert len(spellings) % 2 == 1                  # 2 k + 1 goes through every spelling
        k = int(rng.integers(0, len(spellings)))
        for rd in range(max(24, len(spellings))):
            for pos in (2, 3, 4):
                f.line(tx.name, pos, tx.kmer(pos), rd, sd=spellings[k % len(spellings)], dwell=spellings[(k * 2 + 1) % len(spellings)],
                       start=7 * k, end=7 * k + 1)
                k += 1
        for rd, (mean, sd, dwell) in zip((100, 101), HOST_HALF):
            for pos in (2, 3, 4):
                f.line(tx.name, pos, tx.kmer(pos), rd, mean=mean, sd=sd, dwell=dwell, start=7 * k, end=7 * k + 1)
                k += 1
        return f.bytes()
    return make


FAMILIES = {
    "long_names": dict(make=long_names, kw=dict(min_segment_count=1)),
    "big_site": dict(make=big_site, kw=dict(readcount_max=5000)),
    "index_wide": dict(make=index_wide),
    "big_positions": dict(make=big_positions),
    "values_taken": dict(make=values(TAKEN)),
    "values_rounding": dict(make=values(TAKEN + ROUNDED_AWAY)),
}
SEEDS = G.SEEDS
ALL = dict(G.FAMILIES, **FAMILIES)


def generate(family, seed):
    return FAMILIES[family]["make"](np.random.default_rng([seed, 1000 + sorted(FAMILIES).index(family)]))


class Case(G.Case):
    """eventalign_gen.Case of a family of this module"""

    def __init__(self, family, seed):
        self.family, self.seed, self.nn, self.kw = family, seed, 1, FAMILIES[family].get("kw", {})
        self.data = generate(family, seed)
        self.index = self.error = None
        self.names, self.runs = S.table(self.data, 1)
        self.sites = S.sites(self.names, self.runs, **self.kw)


@functools.lru_cache(maxsize=None)
def case(family, seed):
    return Case(family, seed) if family in FAMILIES else G.case(family, seed)


@functools.lru_cache(maxsize=None)
def parts(family, seed, min_segment_count=None):
    """(sites, runs, logged) of a case that has no error, under its own filters (min_segment_count replaced where given)"""
    c = case(family, seed)
    kw = dict(c.kw) if min_segment_count is None else dict(c.kw, min_segment_count=min_segment_count)
    return D.from_eventalign(c.names, c.runs, **kw)


@functools.lru_cache(maxsize=None)
def expected(family, seed, compress, min_segment_count=None):
    """({file name: bytes}, n_declined) from the statements alone"""
    sites, runs, logged = parts(family, seed, min_segment_count)
    return {k: v.encode() for k, v in D.files(sites, runs, logged, compress).items()}, D.n_declined(sites, compress)
