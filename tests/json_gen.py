"""Seeded inputs for the data.json decode core and its kernels (tests/json_statement.py is what they are held to): number tokens at
the edges of the conversion, records in every whitespace dress, one record per reason a site is declined for, and whole
directories (data.json + data.info) for the loaders."""
import os
import random

KMER = "AAGACTT"                 # N-DRACH-N
OTHER_KMERS = ("GGAACAT", "TTGACCA", "CAAACTG", "ATAACAC")


def _place(digits, frac):
    """the digit string with `frac` digits behind the point"""
    if frac == 0:
        return digits
    if frac >= len(digits):
        return "0." + "0" * (frac - len(digits)) + digits
    return digits[:-frac] + "." + digits[-frac:]


def ties():
    """decimal strings of exact midpoints between two doubles, m * 2^e + 2^(e - 1) with at most 19 digits, and their neighbours one
    unit in the last digit away"""
    out = []
    rng = random.Random(11)
    for e in range(1, 11):                                   # integers above 2^53: odd multiples of 2^(e - 1)
        for _ in range(6):
            m = rng.randrange(1 << 52, 1 << 53)
            mid = m * (1 << e) + (1 << (e - 1))
            if len(str(mid)) <= 19:
                out += [str(mid - 1), str(mid), str(mid + 1)]
    for e in range(-1, -20, -1):                             # fractions: (2 m + 1) / 2^(1 - e) is a decimal of 1 - e fractional digits
        for bits in (3, 10, 20, 30, 40):
            m = rng.randrange(1 << (bits - 1), 1 << bits)
            num = (2 * m + 1) * 5 ** (1 - e)                 # / 10^(1 - e)
            if len(str(num)) <= 19:
                out += [_place(str(num + d), 1 - e) for d in (-1, 0, 1)]
    # true ties need a 53-bit m: the few that fit 19 digits
    for k in range(1, 4):
        for _ in range(8):
            m = rng.randrange(1 << 52, 1 << 53)
            num = (2 * m + 1) * 5 ** k                       # (m + 1/2) * 2^(1 - k) ... as an integer over 10^k
            if len(str(num)) <= 19:
                out += [_place(str(num + d), k) for d in (-1, 0, 1)]
    return out


def numbers(seed=7):
    """accepted tokens (str): every count of significant digits 1..19 with 0..27 fractional digits, zeros, integers above 2^53,
    ties and their neighbours, the largest mantissa"""
    rng = random.Random(seed)
    out = []
    for nd in range(1, 20):
        for frac in range(0, 28):
            for _ in range(3):
                digits = str(rng.randint(1, 9)) + "".join(str(rng.randint(0, 9)) for _ in range(nd - 1))
                tok = _place(digits, frac)
                out.append("-" + tok if rng.random() < 0.25 else tok)
    out += ["0", "0.0", "-0.0", "-0", "00012.5000", "0.000", "100", "1000000.0", "7.", ".5", "-.25", "0.1", "0.3", "123456789012345.6789"]
    out += ["9007199254740992", "9007199254740993", "9007199254740994", "9007199254740995", "18014398509481985", "18014398509481987",
            "9223372036854775807", "9223372036854775808", "9999999999999999999", "999999999999999.9999", "0.9999999999999999999",
            _place("9999999999999999999", 27), _place("1", 27), _place("5", 24),
            "4503599627370496.5", "4503599627370497.5", "2251799813685248.25", "2251799813685248.75", "1.000000000000000222",
            "1.000000000000000111", "1.000000000000000112", "1.000000000000000110", "0.30000000000000004"]
    out += ties()
    return out


DECLINED_TOKENS = ("1e-05", "1E5", "+1", "12345678901234567890", "0.12345678901234567890", "NaN", "Infinity", "-Infinity", "1.2.3", "-", ".",
                   "1.-2", "0x10", _place("1", 28), "--1", "1e", "inf", "nan")


def plain_rows(rng, n, first_id=0):
    """n rows as dataprep writes them: nine features (repr of a float, or a short decimal) and the read index"""
    rows = []
    for r in range(n):
        row = []
        for j in range(9):
            v = rng.choice((rng.uniform(0.001, 0.02), rng.uniform(1.0, 12.0), rng.uniform(60.0, 130.0)))
            row.append(repr(v) if rng.random() < 0.5 else "%.*f" % (rng.randint(1, 6), v))
        row.append(str(first_id + r))
        rows.append(row)
    return rows


def record(tx, pos, kmer, rows, dress=0, tail=""):
    """the record text; dress 0: as json.dumps writes it, 1: no spaces, 2: whitespace of all four kinds between all tokens"""
    if dress == 2:
        w = " \t\r\n "
        body = ("," + w).join("[" + w + (w + "," + w).join(r) + w + "]" for r in rows)
        return ("%s{%s\"%s\"%s:%s{%s\"%s\"%s:%s{%s\"%s\"%s:%s[%s%s%s]%s}%s}%s}" % (w, w, tx, w, w, w, pos, w, w, w, kmer, w, w, w, body, w, w, w, w)) + tail
    sep, colon = (", ", ": ") if dress == 0 else (",", ":")
    body = sep.join("[" + sep.join(r) + "]" for r in rows)
    return '{"%s"%s{"%s"%s{"%s"%s[%s]}}}' % (tx, colon, pos, colon, kmer, colon, body) + tail


class Site:
    """one data.info row and its record.  reason: json_statement's verdict without a norm table; valid: the host loader parses it"""

    def __init__(self, tx, pos, n_reads, text, reason="ok", valid=True, name=""):
        self.tx, self.pos, self.n_reads, self.text, self.reason, self.valid, self.name = tx, pos, n_reads, text.encode("latin-1"), reason, valid, name


def good_site(rng, tx, pos, n, kmer=KMER, dress=0, first_id=0):
    return Site(tx, pos, n, record(tx, pos, kmer, plain_rows(rng, n, first_id), dress) + "\n")


def with_token(rng, tx, pos, tok, n=3, col=4):
    """a site whose row 1 holds `tok` in column `col`"""
    rows = plain_rows(rng, n)
    rows[1][col] = tok
    return record(tx, pos, KMER, rows) + "\n"


def declined_valid(rng, tx="ENST_DV", pos0=100):
    """declined sites the host loader parses: their rows must come out the host's"""
    out = []
    for k, tok in enumerate(("1e-05", "1.5E+1", "+1", "12345678901234567890", "NaN", "Infinity", "-Infinity", _place("1", 28))):
        out.append(Site(tx, pos0 + k, 3, with_token(rng, tx, pos0 + k, tok), "number", True, "token " + tok))
    out.append(Site(tx, pos0 + 20, 2, record(tx, pos0 + 20, KMER, plain_rows(rng, 2), tail=" junk\n"), "tail", True, "bytes behind the record"))
    return out


def malformed(rng, tx="ENST_BAD", pos=500):
    """one site per kind the host loader reports as an error: name -> Site"""
    rows = plain_rows(rng, 3)
    cut = lambda rr, k: [r[:k] for r in rr]
    out = {
        "9 columns": Site(tx, pos, 3, record(tx, pos, KMER, cut(rows, 9)), "columns", False),
        "11 columns": Site(tx, pos, 3, record(tx, pos, KMER, [r + ["1"] for r in rows]), "columns", False),
        "ragged rows": Site(tx, pos, 3, record(tx, pos, KMER, [rows[0], rows[1][:9], rows[2]]), "columns", False),
        "empty row list": Site(tx, pos, 3, record(tx, pos, KMER, []), "empty", False),
        "5-mer key": Site(tx, pos, 3, record(tx, pos, "GACTT", rows), "key", False),
        "backslash in key": Site(tx, pos, 3, record(tx, pos, "AAGA\\CT", rows), "key", False),
        "two sequence keys": Site(tx, pos, 3, record(tx, pos, KMER, rows)[:-3] + ', "%s": []}}}' % OTHER_KMERS[0], "keys", False),
        "wrong transcript": Site(tx, pos, 3, record(tx + "x", pos, KMER, rows), "transcript", False),
        "wrong position": Site(tx, pos, 3, record(tx, pos + 1, KMER, rows), "position", False),
        "fewer reads": Site(tx, pos, 4, record(tx, pos, KMER, rows), "count", False),
        "more reads": Site(tx, pos, 2, record(tx, pos, KMER, rows), "count", False),
        "not DRACH": Site(tx, pos, 3, record(tx, pos, "AACCCTT", rows), "vocabulary", False),
        "bad number": Site(tx, pos, 3, with_token(rng, tx, pos, "abc"), "number", False),
        "truncated": Site(tx, pos, 3, record(tx, pos, KMER, rows)[:-40], None, False),
        "not JSON": Site(tx, pos, 3, "x" * 50, "json", False),
    }
    for name, s in out.items():
        s.name = name
    return out


def write_dir(path, sites, info_order=None, junk=b"", lead=b"", trail=b""):
    """data.json = lead + the records in list order with `junk` between them + trail; data.info in info_order (indices; default: list
    order).  Returns the byte ranges."""
    os.makedirs(path, exist_ok=True)
    blob, ranges = bytearray(lead), []
    for k, s in enumerate(sites):
        if k:
            blob += junk
        ranges.append((len(blob), len(blob) + len(s.text)))
        blob += s.text
    blob += trail
    with open(os.path.join(path, "data.json"), "wb") as f:
        f.write(blob)
    with open(os.path.join(path, "data.info"), "w") as f:
        f.write("transcript_id,transcript_position,start,end,n_reads\n")
        for k in (info_order if info_order is not None else range(len(sites))):
            f.write("%s,%d,%d,%d,%d\n" % (sites[k].tx, sites[k].pos, ranges[k][0], ranges[k][1], sites[k].n_reads))
    return ranges
