"""eventalign.txt -> runs, candidate rows and the loader's arrays, stated in plain Python and NumPy.

This is the definition the native dataprep (m6a_io.cpp) and the device's prep kernels (m6a_prep.hip) are held to.  It is written
from what the project documents (include/m6a_io.h) and from what the reference's dataprep does with pandas; it shares
no code with either implementation, imports nothing from them, and is meant to be read top to bottom:

    index      the (contig, read index) runs of the file and their byte ranges       -> eventalign.index
    combine    one run's events -> per (position, k-mer) the length-weighted means
    windows    2w + 1 consecutive positions around a DRACH centre -> candidate rows
    sites      the readcount cut, one run per read, the sort, the filters, X         -> what the loader makes of data.json
    declines   which runs the device may hand to the host (it computes nothing)

Numbers are Python's: int() for integer fields, float() (correctly rounded for every spelling) for float fields, float64
arithmetic in the order written.  Nothing here is fast; the files it is run on hold a few thousand lines.
"""
import numpy as np

EFORMAT = -4                                  # M6A_IO_EFORMAT (include/m6a_io.h)
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1
C_BLANKS = b" \t\n\v\f\r"                     # isspace() in the C locale


class StatementError(Exception):
    """What both implementations must refuse: `code` as include/m6a_io.h numbers it, `text` = the leading words of the message."""

    def __init__(self, code, text):
        super().__init__(text)
        self.code, self.text = code, text


# ---- index -----------------------------------------------------------------------------------------------------------------
def c_atoll(data, at):
    """C atoll() of the text that starts at data[at]: blanks, one sign, digits; stops at the first other byte; saturates as
    strtoll does.  (The reference reads the column with pandas, which refuses '12abc' or an empty field outright; for such files
    include/m6a_io.h's rule -- atoll of the text after the third tab -- is the definition.  Note that the text does not end with
    the field: blanks include the tab and the newline, so an empty field reads on into whatever follows.)"""
    n = len(data)
    while at < n and data[at] in C_BLANKS:
        at += 1
    negative = False
    if at < n and data[at] in b"+-":
        negative = data[at] == ord("-")
        at += 1
    end = at
    while end < n and 48 <= data[end] <= 57:
        end += 1
    value = int(data[at:end]) if end > at else 0
    return max(I64_MIN, min(I64_MAX, -value if negative else value))


def index(data):
    """(names, runs): transcript names in order of first appearance; runs as dicts tx, read, start, end in file order.
    The first line is the header.  A body line without a tab is skipped; one with fewer than three tabs is an error at its
    offset; a run is a maximal stretch of (not skipped) lines with equal contig bytes and equal read index, and its byte range
    goes from its first line's first byte to the byte after its last line's newline (or the file's end)."""
    first = data.find(b"\n")
    if first < 0:
        raise StatementError(EFORMAT, "no header line")
    names, ids, runs = [], {}, []
    p, n = first + 1, len(data)
    while p < n:
        nl = data.find(b"\n", p)
        nxt = n if nl < 0 else nl + 1
        line = data[p:nxt]
        tab1 = line.find(b"\t")
        if tab1 >= 0:
            tab3 = line.find(b"\t", line.find(b"\t", tab1 + 1) + 1) if line.count(b"\t") >= 3 else -1
            if tab3 < 0:
                raise StatementError(EFORMAT, "short line at byte %d" % p)
            contig, read = line[:tab1], c_atoll(data, p + tab3 + 1)
            if not runs or names[runs[-1]["tx"]] != contig or runs[-1]["read"] != read:
                if contig not in ids:
                    ids[contig] = len(names)
                    names.append(contig)
                runs.append(dict(tx=ids[contig], read=read, start=p, end=p))
            runs[-1]["end"] = nxt
        p = nxt
    return names, runs


def index_text(names, runs):
    """eventalign.index as the reference writes it."""
    return "transcript_id,read_index,pos_start,pos_end\n" + "".join(
        "%s,%d,%d,%d\n" % (names[r["tx"]].decode(), r["read"], r["start"], r["end"]) for r in runs)


# ---- combine ---------------------------------------------------------------------------------------------------------------
def integer(text):
    """position, start_idx, end_idx.  pandas reads a column spelled '12.0' as float64; the documented rule is the value truncated."""
    try:
        return int(text)
    except ValueError:
        return int(float(text))


def kahan_sum(values):
    """pandas' grouped sum (group_sum): Kahan's compensated sum, the compensation reset to 0 when it is NaN."""
    total, comp = 0.0, 0.0
    for v in values:
        y = v - comp
        t = total + y
        comp = t - total - y
        if comp != comp:
            comp = 0.0
        total = t
    return total


def combine(chunk):
    """One run's bytes -> [(position, k-mer, dwell, sd, mean)] sorted by (position, k-mer).
    Lines end at '\\n' (a '\\r' before it is dropped); an empty line is skipped; a line of fewer than 15 fields is malformed.
    Only lines whose reference_kmer (field 2) equals model_kmer (field 9) count.  Per (position, k-mer), events in file order:
    length = end_idx - start_idx; the three sums of value * length; each divided by the total length; the mean rounded to one
    decimal as np.round does (times ten, to nearest even, divided by ten).  A total length of 0 gives 0 / 0 = NaN."""
    groups = {}
    for line in chunk.split(b"\n"):
        if line.endswith(b"\r"):
            line = line[:-1]
        if not line:
            continue
        f = line.split(b"\t")
        if len(f) < 15:
            raise StatementError(EFORMAT, "malformed eventalign line")
        if f[2] != f[9]:
            continue
        try:
            position, length = integer(f[1]), integer(f[14]) - integer(f[13])
            mean, sd, dwell = float(f[6]), float(f[7]), float(f[8])
        except ValueError:
            raise StatementError(EFORMAT, "malformed eventalign line")
        groups.setdefault((position, f[2]), []).append((mean, sd, dwell, length))
    out = []
    for (position, kmer) in sorted(groups):
        events = groups[(position, kmer)]
        total = float(sum(e[3] for e in events))
        s_mean = kahan_sum(e[0] * float(e[3]) for e in events)
        s_sd = kahan_sum(e[1] * float(e[3]) for e in events)
        s_dwell = kahan_sum(e[2] * float(e[3]) for e in events)
        out.append((position, kmer, divide(s_dwell, total), divide(s_sd, total), float(np.rint(divide(s_mean, total) * 10.0)) / 10.0))
    return out


def divide(a, b):
    """IEEE a / b: Python's own division, and NumPy's where Python would raise (x / 0 is an infinity, 0 / 0 a NaN)"""
    try:
        return a / b
    except ZeroDivisionError:
        with np.errstate(invalid="ignore", divide="ignore"):
            return float(np.float64(a) / np.float64(b))


# ---- windows ---------------------------------------------------------------------------------------------------------------
def is_drach(kmer):
    return len(kmer) == 5 and kmer[0] in b"AGT" and kmer[1] in b"GA" and kmer[2:4] == b"AC" and kmer[4] in b"ACT"


def windows(positions, w):
    """Candidate rows of one run: [(position + 2, (5 + 2w)-mer, [dwell, sd, mean] of the 2w + 1 positions)].
    The combined positions are cut into maximal stretches in which each position is the one before plus one (a position that
    comes twice, under two k-mers, therefore ends a stretch); inside a stretch of at least 2w + 1, every entry with w entries
    either side and a DRACH 5-mer is a row; its sequence is the first 5-mer followed by the last base of each later one."""
    rows, a = [], 0
    while a < len(positions):
        b = a + 1
        while b < len(positions) and positions[b][0] == positions[b - 1][0] + 1:
            b += 1
        for c in range(a + w, b - w):
            if is_drach(positions[c][1]):
                win = positions[c - w:c + w + 1]
                seq = win[0][1] + b"".join(p[1][-1:] for p in win[1:])
                rows.append((positions[c][0] + 2, seq, [v for p in win for v in p[2:5]]))
        a = b
    return rows


def table(data, w, runs=None):
    """What m6a_io_dataprep_rows returns: (names, runs) with npos and rows added to every run."""
    names, found = index(data)
    runs = found if runs is None else runs
    for r in runs:
        ps = combine(data[r["start"]:r["end"]])
        r["npos"], r["rows"] = len(ps), windows(ps, w)
    return names, runs


# ---- sites -----------------------------------------------------------------------------------------------------------------
def vocabulary():
    """The 66 5-mers of all N-DRACH-N 7-mers, sorted: a site's three k-mer ids index this list."""
    sevens = [a + d + r + "AC" + h + b for a in "ACGT" for d in "AGT" for r in "GA" for h in "ACT" for b in "ACGT"]
    return sorted({s[i:i + 5] for s in sevens for i in range(3)})


CANONICAL_NAN = np.array([0x7ff8000000000000], np.uint64).view(np.float64)[0]


def records(names, runs, readcount_min=1, readcount_max=1000, min_segment_count=20):
    """data.json's records in order: [(transcript, position, sequence, [(features, read index)])].
    Per transcript, in order of first appearance, its runs in index order: a run with more than one combined position enters a
    dict under its read index (a read that comes again overwrites its rows and keeps its place); after every run the count goes
    up, and the loop stops once it exceeds readcount_max (so readcount_max + 1 runs are seen); the transcript is used when the
    count reached readcount_min.  Rows are ordered by (position, the read's place in the dict) -- the project's rule; the
    reference's order inside a position comes from an unstable argsort.  The rows of one position are a site and must agree on
    the sequence; a site is written with at least min_segment_count rows."""
    out = []
    for t in range(len(names)):
        by_read, count = {}, 0
        for r in (r for r in runs if r["tx"] == t):
            if r["npos"] > 1:
                by_read[r["read"]] = r
            count += 1
            if count > readcount_max:
                break
        if count < readcount_min:
            continue
        rows = [(row[0], place, row[1], row[2], read) for place, (read, r) in enumerate(by_read.items()) for row in r["rows"]]
        rows.sort(key=lambda x: (x[0], x[1]))
        a = 0
        while a < len(rows):
            b = a
            while b < len(rows) and rows[b][0] == rows[a][0]:
                if rows[b][2] != rows[a][2]:
                    raise StatementError(EFORMAT, "reads disagree on the sequence at %s:%d" % (names[t].decode(), rows[a][0]))
                b += 1
            if b - a >= min_segment_count:
                out.append((names[t].decode(), rows[a][0], rows[a][2].decode(), [(row[3], row[4]) for row in rows[a:b]]))
            a = b
    return out


def sites(names, runs, readcount_min=1, readcount_max=1000, min_segment_count=20, norm=None, min_reads=20):
    """The loader's arrays from a table with n_neighbors = 1, as a dict: X float32 [R, 9], km uint8 [S, 3], off int64 [S + 1],
    tx_pos int64 [S], read_ids float64 [R], tx [S] (names), kmer7 [S].
    The records with at least min_reads rows.  X = float32((v - mean) / std) computed in float64 with the table row of each of
    the 7-mer's three 5-mers (norm: 5-mer -> (mean[3], std[3])); a NaN feature is the NaN that the text 'NaN' reads back as
    (data.json holds no sign or payload); the read id is float(read index), as data.json holds it."""
    voc = vocabulary()
    X, km, off, tx_pos, read_ids, tx, kmer7 = [], [], [0], [], [], [], []
    for name, position, seq, rows in records(names, runs, readcount_min, readcount_max, min_segment_count):
        if len(rows) < min_reads:
            continue
        fives = [seq[c:c + 5] for c in range(3)]
        for k in fives:
            if norm is not None and k not in norm:
                raise StatementError(EFORMAT, "no normalisation factors for %s" % k)
        for k in fives:
            if k not in voc:
                raise StatementError(EFORMAT, "site %s:%d: %s is not a DRACH context" % (name, position, seq))
        if norm is not None:
            mean = np.concatenate([np.asarray(norm[k][0], np.float64) for k in fives])
            std = np.concatenate([np.asarray(norm[k][1], np.float64) for k in fives])
        for features, read in rows:
            v = np.array(features, np.float64)
            v[np.isnan(v)] = CANONICAL_NAN
            with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                X.append((v if norm is None else (v - mean) / std).astype(np.float32))
            read_ids.append(float(read))
        km.append([voc.index(k) for k in fives])
        off.append(off[-1] + len(rows))
        tx_pos.append(position)
        tx.append(name)
        kmer7.append(seq)
    return dict(X=np.array(X, np.float32).reshape(-1, 9), km=np.array(km, np.uint8).reshape(-1, 3), off=np.array(off, np.int64),
                tx_pos=np.array(tx_pos, np.int64), read_ids=np.array(read_ids, np.float64), tx=tx, kmer7=kmer7)


# ---- what the device may decline --------------------------------------------------------------------------------------------
def plain_digits(text, most):
    return 0 < len(text) <= most and text.isdigit()


def fast_float(text):
    """digits [. digits] with 1 to 15 digit characters in all"""
    whole, dot, frac = text.partition(b".")
    return (whole + frac).isdigit() and len(whole + frac) <= 15


def declines(data, run):
    """True where the device may mark the run M6A_PREP_RUN_HOST -- the list in the header of m6a_prep.hip, restated; nothing is
    computed.  A run is declined when
      - its byte range is not whole body lines (an eventalign.index from elsewhere: --skip_index);
      - one of its lines has no tab (an empty line, too) or fewer than 15 fields;
      - on a line whose reference_kmer equals model_kmer: a float field that is not digits [. digits] of at most 15 digit
        characters (a sign, an exponent, a name, nothing), an integer field that is not 1 to 18 plain digits, or a k-mer that
        is not 5 characters;
      - two such lines follow each other out of (position, k-mer) order;
      - its contig name is longer than an int32 holds.
    Fields of lines whose k-mers differ are never read, so nothing in them declines a run."""
    start, end = run["start"], run["end"]
    if start <= 0 or data[start - 1:start] != b"\n" or not (end == len(data) or data[end - 1:end] == b"\n") or start >= end:
        return True
    chunk = data[start:end]
    lines = chunk[:-1].split(b"\n") if chunk.endswith(b"\n") else chunk.split(b"\n")
    before = None
    for line in lines:
        if b"\t" not in line:
            return True
        if line.index(b"\t") > 0x7fffffff:
            return True
        if line.endswith(b"\r"):
            line = line[:-1]
        f = line.split(b"\t")
        if len(f) < 15:
            return True
        if f[2] != f[9]:
            continue
        if not (plain_digits(f[1], 18) and plain_digits(f[13], 18) and plain_digits(f[14], 18)):
            return True
        if not (fast_float(f[6]) and fast_float(f[7]) and fast_float(f[8])) or len(f[2]) != 5:
            return True
        key = (int(f[1]), f[2])
        if before is not None and key < before:
            return True
        before = key
    return False


def bits_for(v):
    """the width of a sort-key field that holds 0 .. v (m6a_prep.hip sizes its fields by the range of the values)"""
    return int(v).bit_length()
