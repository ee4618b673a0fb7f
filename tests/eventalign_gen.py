"""Seeded, small eventalign.txt files for the edges of the prep kernels: generate(family, seed) -> bytes, nothing stored.

FAMILIES[name] says how a family is run: nn (n_neighbors), kw (the site filters), declined = True where some runs are of the
kind the device hands to the host, and where both implementations must refuse the file the (code, leading words) of the error:
`error` from the index, `rows_error` from a run's lines, `site_error` from the sites.  case(family, seed) is the file with the
statement's answers, computed once per process.
"""
import functools

import numpy as np

import eventalign_statement as S

HEADER = b"contig\tposition\treference_kmer\tread_index\tstrand\tevent_index\tevent_level_mean\tevent_stdv\tevent_length\t" \
         b"model_kmer\tmodel_mean\tmodel_stdv\tstandardized_level\tstart_idx\tend_idx\n"
BLOCK = 4096                                  # bytes per block of the newline scan, and the unit of the upload chunk
DRACH = [d + r + "AC" + h for d in "AGT" for r in "GA" for h in "ACT"]


def b(x):
    return x if isinstance(x, bytes) else str(x).encode()


class Tx:
    """A transcript: a name, a sequence, and the position of the sequence's first base (positions can be huge, the text is not)."""

    def __init__(self, rng, name, length, drach_at=(), base=0):
        self.name, self.base = name, base
        while True:
            seq = list("ACGT"[i] for i in rng.integers(0, 4, length + 4))
            for p in drach_at:
                seq[p:p + 5] = DRACH[rng.integers(0, len(DRACH))]
            self.seq = "".join(seq)
            planted = set(drach_at)
            # no accidental DRACH: the sites are exactly the planted ones
            if all((i in planted) == S.is_drach(self.seq[i:i + 5].encode()) for i in range(length)):
                break

    def kmer(self, pos):
        return self.seq[pos - self.base:pos - self.base + 5]


class File:
    def __init__(self, rng):
        self.rng, self.parts, self.size, self.clock, self.npad = rng, [HEADER], len(HEADER), 100, 0
        self.pool, self.at = rng.random((4096, 9)).tolist(), 0       # nine numbers per line, drawn once (a line costs no generator call)

    def raw(self, text):
        self.parts.append(text)
        self.size += len(text)

    def text(self, contig, pos, kmer, read, mean=None, sd=None, dwell=None, start=None, end=None, model=None, eol=b"\n"):
        u = self.pool[self.at]
        self.at = (self.at + 1) % len(self.pool)
        if start is None:
            start = self.clock
        if end is None:
            end = int(start) + 3 + int(u[0] * 37)
            self.clock = end
        f = (contig, pos, kmer, read, "t", int(u[1] * 999),
             "%.2f" % (60 + 70 * u[2]) if mean is None else mean, "%.3f" % (0.5 + 8.5 * u[3]) if sd is None else sd,
             "%.5f" % (0.001 + 0.049 * u[4]) if dwell is None else dwell, kmer if model is None else model,
             "%.2f" % (60 + 70 * u[5]), "%.2f" % (1 + 3 * u[6]), "%.2f" % (6 * u[7] - 3), start, end)
        return "\t".join([x.decode("latin-1") if isinstance(x, bytes) else str(x) for x in f]).encode("latin-1") + eol

    def line(self, *a, **kw):
        self.raw(self.text(*a, **kw))

    def place(self, text, newline_at):
        """`text` (one line) behind a padding line, so that its last byte lies at `newline_at` modulo the block size"""
        self.pad_to((newline_at - (len(text) - 1)) % BLOCK)
        self.raw(text)
        assert (self.size - 1) % BLOCK == newline_at

    def stretch(self, tx, first, count, read, events=(1, 3), mismatch=0.1, **kw):
        """read `read` over positions first .. first + count - 1 of tx: one to two events each, some with another model k-mer"""
        for pos in range(first, first + count):
            u = self.pool[self.at][8]
            for k in range(events[0] + int(u * (events[1] - events[0]))):
                self.line(tx.name, pos, tx.kmer(pos), read, model="NNNNN" if (u * 7919 + k * 0.37) % 1 < mismatch else None, **kw)

    def pad_to(self, residue):
        """A line of a transcript of its own whose contig name is as long as it takes for the NEXT line to start at a byte
        offset that is `residue` modulo the block size: placement is exact, not left to chance."""
        self.npad += 1
        name = "PAD%d" % self.npad
        tail = b"\t".join(b(x) for x in ("", 7, "CCCCC", 1, "t", 1, "80.00", "1.000", "0.00100", "NNNNN", "80.00", "1.00", "0.00", 1, 2)) + b"\n"
        short = self.size + len(name) + len(tail)
        self.raw(name.encode() + b"x" * ((residue - short) % BLOCK) + tail)

    def bytes(self):
        return b"".join(self.parts)


def site_reads(f, tx, centre, reads, flank=1, **kw):
    """each of `reads` over the 2 flank + 1 positions around `centre`: one candidate row per read"""
    for rd in reads:
        f.stretch(tx, centre - flank, 2 * flank + 1, rd, **kw)


# ---- the families -----------------------------------------------------------------------------------------------------------
def plain(rng):
    f = File(rng)
    for t in range(3):
        tx = Tx(rng, "ENST%05d.%d" % (rng.integers(1, 99999), t + 1), 40, (4, 11, 19, 30), base=int(rng.integers(0, 5000)))
        for rd in rng.permutation(26 + 3 * t):
            a = int(rng.integers(0, 8))
            z = int(rng.integers(25, 41))
            gap = int(rng.integers(a + 1, z)) if rng.random() < 0.4 else None        # one missing position breaks the stretch
            for lo, hi in ((a, z),) if gap is None else ((a, gap), (gap + 1, z)):
                f.stretch(tx, tx.base + lo, hi - lo, int(rd) + 100 * t)
    return f.bytes()


def wide_reads(rng, n):
    """n read indices from -2^62 to 2^62, both ends included: a range of 2^63, which takes all 64 bits of a sort key"""
    mid = [int(x) for x in rng.integers(-2 ** 62, 2 ** 62, n - 2)]
    out = [-2 ** 62, 2 ** 62] + mid
    return [out[i] for i in rng.permutation(n)]


def split_runs(rng):
    """two transcripts and read indices that fill 64 bits: the run key (transcript, read) needs 65, so the sort takes two passes;
    every read comes twice in its transcript (the second run supplies the rows) so that the order matters"""
    f = File(rng)
    txs = [Tx(rng, "SR%d" % t, 12, (3,), base=50 * t) for t in range(2)]
    reads = [wide_reads(rng, 24), wide_reads(rng, 24)]
    for rnd in range(2):
        for k in range(24):
            for t in (0, 1):
                f.stretch(txs[t], txs[t].base + 2, 3, reads[t][k] if rnd == 0 else reads[t][23 - k], mismatch=0)
    return f.bytes()


def split_rows(rng):
    """positions from single digits to 18 digits in one file: the position field of the row key alone takes about 60 bits, the
    place takes 10 (readcount_max 1000) and the transcript 2, so the row sort flushes and repacks"""
    f = File(rng)
    bases = [3, 10 ** 17 + int(rng.integers(0, 10 ** 9)), int(rng.integers(10 ** 8, 10 ** 9)), 9 * 10 ** 17]
    txs = [Tx(rng, "SW%d" % t, 16, (2, 9), base=bases[t]) for t in range(4)]
    reads = [wide_reads(rng, 22) for _ in txs]
    for k in range(22):
        for t in rng.permutation(4):                                  # transcripts interleaved: segments are not adjacent
            f.stretch(txs[t], txs[t].base + 1, 10, reads[t][k], mismatch=0)
    return f.bytes()


def radix(n):
    def make(rng):
        """exactly n candidate rows, one per read, all runs used: the row sort's tiles of 4 096 keys at n"""
        f = File(rng)
        left, t = n, 0
        while left:
            here = min(left, 900)
            tx = Tx(rng, "RX%d" % t, 30, (2, 8, 14, 20, 26), base=int(rng.integers(0, 10 ** 6)))
            for rd in rng.permutation(here):
                f.stretch(tx, tx.base + 1 + 6 * int(rng.integers(0, 5)), 3, int(rd), events=(1, 2), mismatch=0)
            left, t = left - here, t + 1
        return f.bytes()
    return make


def radix_ties(rng):
    """3 000 rows that share one (transcript, position): only the place tells them apart, through every digit of the sort"""
    f = File(rng)
    tx = Tx(rng, "TIES", 8, (2,))
    for rd in rng.permutation(3000):
        f.stretch(tx, 1, 3, int(rd) * 7 - 9000, events=(1, 2), mismatch=0)
    return f.bytes()


def newlines(variant):
    def make(rng):
        f = File(rng)
        tx = Tx(rng, "NL1", 20, (3, 12))

        def some(first_read, count=3):
            for rd in range(first_read, first_read + count):
                f.stretch(tx, 2, 14, rd)
        some(0)
        f.place(f.text(tx.name, 5, tx.kmer(5), 50), BLOCK - 1)            # '\n' is the last byte of a block
        some(3)
        f.place(f.text(tx.name, 5, tx.kmer(5), 51), 0)                    # '\n' is the first byte of a block
        some(6)
        f.pad_to(16)
        f.raw(b"\n" * 16)                                                  # a lane of nothing but newlines
        some(9)
        f.pad_to(0)
        f.raw(b"\n" * BLOCK)                                               # a block of nothing but newlines
        some(12)
        f.pad_to(100)                                                      # a line longer than a block follows
        f.line("LONG" + "y" * 5000, 5, "CCCCC", 1, model="NNNNN")
        some(15, 12)
        if variant in (0, 2):                                              # the file is a whole number of blocks
            f.place(f.text(tx.name, 5, tx.kmer(5), 52, eol=b"" if variant else b"\n"), BLOCK - 1)
            assert f.size % BLOCK == 0
        else:                                                              # no final newline
            f.line(tx.name, 5, tx.kmer(5), 52, eol=b"")
        return f.bytes()
    return make


def numbers_ok(rng):
    """spellings at the edge of the fast paths, all inside them; and spellings outside them on lines whose k-mers differ"""
    f = File(rng)
    tx = Tx(rng, "NUM", 12, (3,), base=10 ** 17 + 12345)                       # 18-digit positions
    floats = ["123456789.012345", ".000000000000123", "5.", ".5", "000000095.310000", "0.00000000000001", "999999999999999", "0", "00.0"]
    for rd in range(24):
        for pos in range(tx.base + 2, tx.base + 5):
            a = int(rng.integers(10 ** 17, 8 * 10 ** 17))                      # 18-digit start_idx / end_idx
            f.line(tx.name, pos, tx.kmer(pos), rd, mean=floats[int(rng.integers(0, len(floats)))], sd=floats[int(rng.integers(0, len(floats)))],
                   dwell=floats[int(rng.integers(0, len(floats)))], start=a, end=a + int(rng.integers(1, 50)))
            f.line(tx.name, pos, tx.kmer(pos), rd, mean="-1.5", sd="1e5", dwell="+0.1234567890123456", start="12.0", end="-3", model="NNNNN")
    return f.bytes()


READ_SPELLINGS = [b" 7", b"+8", b"-3", b"12abc", b"99999999999999999999", b"-99999999999999999999", b"", b"  \v42", b"0x1F", b"007"]


def atoll(rng):
    """the read index as C atoll reads it: blanks, signs, trailing letters, saturation, an empty field"""
    f = File(rng)
    tx = Tx(rng, "ATOLL", 12, (3,))
    site_reads(f, tx, 3, range(100, 120), mismatch=0)
    for sp in READ_SPELLINGS:
        site_reads(f, tx, 3, [sp], mismatch=0)
    return f.bytes()


def combine(rng):
    f = File(rng)
    tx = Tx(rng, "CMB", 14, (3, 9))
    for rd in range(30):
        if rd == 4:                                      # hundreds of events in one group: the compensation matters
            f.stretch(tx, 2, 1, rd)
            f.stretch(tx, 3, 1, rd, events=(400, 401), mismatch=0.05)
            f.stretch(tx, 4, 1, rd)
        elif rd == 7:                                    # every event of the centre has end_idx == start_idx: 0 / 0
            f.stretch(tx, 2, 1, rd)
            for _ in range(3):
                f.line(tx.name, 3, tx.kmer(3), rd, start=500, end=500)
            f.stretch(tx, 4, 1, rd)
        elif rd == 9:                                    # one event of length 0 among others
            f.stretch(tx, 2, 1, rd)
            f.line(tx.name, 3, tx.kmer(3), rd, start=500, end=500)
            f.line(tx.name, 3, tx.kmer(3), rd)
            f.stretch(tx, 4, 1, rd)
        elif rd == 11:                                   # position 9 under two k-mers, in key order: it ends the stretch twice
            f.stretch(tx, 7, 2, rd, mismatch=0)
            f.line(tx.name, 9, "AAAAA", rd)
            f.line(tx.name, 9, tx.kmer(9), rd)                   # a DRACH 5-mer: "..AC." sorts after "AAAAA"
            f.stretch(tx, 10, 3, rd, mismatch=0)
        elif rd == 13:                                   # no line matches
            f.stretch(tx, 2, 9, rd, mismatch=1.0)
        else:
            f.stretch(tx, 2, 9, rd)
    return f.bytes()


def windows(w):
    def make(rng):
        f = File(rng)
        n = 2 * w + 1
        # stretches (first, count); DRACH planted at 10, 30 and 34 (their windows overlap), 60, 80
        tx = Tx(rng, "WIN", 100, (10, 30, 34, 60, 80))
        plan = [(10 - w, n), (10 - w, n - 1), (10 - w + 1, n - 1),           # exact; one short on the right; one short on the left
                (30 - w, n + 4), (30 - w - 3, n + 8 + w),                       # both centres; with room either side
                (60 - w, n + 6), (60 - w - 6, n + 6), (60 - w + 1, n + 6),     # centre at the first place; the last; one before the first
                (80 - w - 4, 4 + w), (80 - w - 4, 4 + n + 4)]                  # the stretch ends at the centre; covers it
        for rd, (first, count) in enumerate(plan * 2):
            f.stretch(tx, first, count, rd, mismatch=0)
            if rd % 3 == 0:                                                    # a gap, then a second stretch of the same read
                f.stretch(tx, first + count + 1, n, rd, mismatch=0)
        return f.bytes()
    return make


def filters(n):
    def make(rng):
        """sites of n - 1, n and n + 1 reads in FA; FB has exactly readcount_min = n + 2 runs, FC one fewer; FD's runs come in two
        segments with FC's between them and readcount_max = n + 4 cuts inside the second; read 3 of FA comes again with other
        values (its rows change, its place stays) and read 5 again with a single position (nothing changes)"""
        f = File(rng)
        fa, fb, fc, fd = (Tx(rng, "F" + c, 30, (3, 12, 21)) for c in "ABCD")
        for rd in range(n + 1):
            f.stretch(fa, 2, 3, rd, mismatch=0)
            if rd < n:
                f.stretch(fa, 11, 3, rd, mismatch=0)
            if rd < n - 1:
                f.stretch(fa, 20, 3, rd, mismatch=0)
            if rd == 8:
                for first in (2, 11, 20):
                    f.stretch(fa, first, 3, 3, mismatch=0)
                f.stretch(fa, 11, 1, 5, mismatch=0)
        site_reads(f, fb, 3, range(n + 2), mismatch=0)
        site_reads(f, fd, 12, range(n), mismatch=0)
        site_reads(f, fc, 3, range(n + 1), mismatch=0)
        site_reads(f, fd, 12, range(n, 2 * n), mismatch=0)
        return f.bytes()
    return make


def disagree(rng):
    f = File(rng)
    ok = Tx(rng, "DOK", 12, (3,))
    site_reads(f, ok, 3, range(21), mismatch=0)
    tx = Tx(rng, "DBAD", 30, (3, 12, 21))
    for k, c in enumerate((21, 12, 3)):
        site_reads(f, tx, c, range(10 * k, 10 * k + 5), mismatch=0)
    other = Tx(rng, "DBAD", 30, (3, 12, 21))
    swap = {"A": "C", "C": "G", "G": "T", "T": "A"}
    other.seq = "".join(swap[c] if i in (17, 26) else c for i, c in enumerate(tx.seq))     # the last base of the 7-mers at 14 and 23
    site_reads(f, other, 21, [30], mismatch=0)         # sites 14 and 23 disagree; 14 is the first, and comes later in the file
    site_reads(f, other, 12, [31, 32], mismatch=0)
    return f.bytes()


def short_line(rng):
    f = File(rng)
    tx = Tx(rng, "SHORT", 12, (3,))
    site_reads(f, tx, 3, range(4))
    f.raw(b"ctg\t1\n")
    site_reads(f, tx, 3, range(4, 6))
    f.raw(b"ctg\t1\tAAAAA\n")
    return f.bytes()


def short_in_run(rng):
    f = File(rng)
    tx = Tx(rng, "SHRUN", 12, (3,))
    site_reads(f, tx, 3, range(4))
    f.line(tx.name, 2, tx.kmer(2), 4)
    f.raw(b"\t".join([tx.name.encode(), b"3", tx.kmer(3).encode(), b"4", b"t", b"9"]) + b"\n")       # six fields, same run
    f.line(tx.name, 4, tx.kmer(4), 4)
    return f.bytes()


DECLINED_KINDS = ["plus", "minus", "exponent", "digits16", "int19", "int_as_float", "order", "kmer4", "empty_line", "crlf_ok"]


def declined(rng):
    """one run of each kind the device hands to the host, among 22 plain reads of the same site; read 200 + k is of kind k"""
    f = File(rng)
    tx = Tx(rng, "DECL", 12, (3,))
    site_reads(f, tx, 3, range(22), mismatch=0)
    for k, kind in enumerate(DECLINED_KINDS):
        rd = 200 + k
        f.stretch(tx, 2, 1, rd, mismatch=0)
        kw = dict(plus=dict(mean="+95.31"), minus=dict(sd="-1.25"), exponent=dict(dwell="2.5e-3"), digits16=dict(mean="95.31000000000001"),
                  int19=dict(start="1000000000000000001", end="1000000000000000019"), int_as_float=dict(start="12.0", end="19.0"),
                   crlf_ok=dict(eol=b"\r\n")).get(kind, {})
        if kind == "order":
            f.stretch(tx, 4, 1, rd, mismatch=0)
            f.stretch(tx, 3, 1, rd, mismatch=0)
            continue
        if kind == "kmer4":
            f.line(tx.name, 9, "GGAC", rd)
            continue
        if kind == "empty_line":
            f.raw(b"\n")
        f.line(tx.name, 3, tx.kmer(3), rd, **kw)
        f.stretch(tx, 4, 1, rd, mismatch=0)
    return f.bytes()


def midline(rng):
    """a plain file for --skip_index; midline_index() cuts one of its index rows inside the last field of a line"""
    f = File(rng)
    tx = Tx(rng, "MID", 12, (3,))
    site_reads(f, tx, 3, range(24), mismatch=0, events=(2, 3))
    return f.bytes()


def midline_index(data):
    """(index text, runs): the file's own index with the byte ranges of runs 5 and 11 ending 2 bytes and 1 byte before their last
    newline: the last line of each loses the end of its end_idx, and the lines stay whole in every other field"""
    names, runs = S.index(data)
    runs[5]["end"] -= 3
    runs[11]["end"] -= 2
    return S.index_text(names, runs), names, runs


FAMILIES = {
    "plain": dict(make=plain),
    "split_runs": dict(make=split_runs),
    "split_rows": dict(make=split_rows),
    "radix_4095": dict(make=radix(4095)), "radix_4096": dict(make=radix(4096)), "radix_4097": dict(make=radix(4097)),
    "radix_8192": dict(make=radix(8192)),
    "radix_ties": dict(make=radix_ties, kw=dict(readcount_max=5000)),
    "newlines_0": dict(make=newlines(0)), "newlines_1": dict(make=newlines(1)), "newlines_2": dict(make=newlines(2)),
    "numbers_ok": dict(make=numbers_ok),
    "atoll": dict(make=atoll),
    "combine": dict(make=combine),
    "windows_2": dict(make=windows(2), nn=2), "windows_3": dict(make=windows(3), nn=3),
    "filters_20": dict(make=filters(20), kw=dict(readcount_min=22, readcount_max=24)),
    "filters_25": dict(make=filters(25), kw=dict(readcount_min=27, readcount_max=29, min_segment_count=25)),
    "midline": dict(make=midline),
    "declined": dict(make=declined, declined=True),
    "disagree": dict(make=disagree, site_error=(S.EFORMAT, "reads disagree on the sequence at DBAD:14")),
    "short_line": dict(make=short_line, error=(S.EFORMAT, "short line at byte ")),
    "short_in_run": dict(make=short_in_run, declined=True, rows_error=(S.EFORMAT, "malformed eventalign line")),
}
SEEDS = (1, 2, 3)


def generate(family, seed):
    return FAMILIES[family]["make"](np.random.default_rng([seed, sorted(FAMILIES).index(family)]))


class Case:
    """A generated file and what the statement makes of it: names, runs (with npos and rows), sites -- or the error it raises."""

    def __init__(self, family, seed):
        spec = FAMILIES[family]
        self.family, self.seed, self.nn, self.kw = family, seed, spec.get("nn", 1), spec.get("kw", {})
        self.data = generate(family, seed)
        self.names = self.runs = self.sites = self.error = self.index = None
        try:
            if family == "midline":
                self.index, self.names, self.runs = midline_index(self.data)
            else:
                self.names, self.runs = S.index(self.data)
            for r in self.runs:                       # S.table, but a run whose lines are refused stays without npos and rows
                try:
                    positions = S.combine(self.data[r["start"]:r["end"]])
                    r["npos"], r["rows"] = len(positions), S.windows(positions, self.nn)
                except S.StatementError as e:
                    self.error = (e.code, e.text)
            if self.nn == 1 and self.error is None:
                self.sites = S.sites(self.names, self.runs, **self.kw)
        except S.StatementError as e:
            self.error = (e.code, e.text)

    def write(self, tmp_path):
        """(eventalign.txt, eventalign.index or None) under tmp_path"""
        ev = tmp_path / ("%s_%d.txt" % (self.family, self.seed))
        ev.write_bytes(self.data)
        idx = None
        if self.index is not None:
            idx = tmp_path / ("%s_%d.index" % (self.family, self.seed))
            idx.write_text(self.index)
        return str(ev), None if idx is None else str(idx)


@functools.lru_cache(maxsize=None)
def case(family, seed):
    return Case(family, seed)
