"""What `inference --loader device` takes of a data.json record, in plain Python: the statement the decode core
(m6anet_amd/csrc/m6a_json.h) and its kernels are held to.

A number token is ACCEPTED when it is an optional '-', digits with at most one '.', at least one digit, no exponent, at most 19
significant digits (from the first non-zero digit on) and at most 27 digits behind the point; its value is float(token).  A site is
REGULAR when walk() returns "ok"; for anything else it returns the reason the site is declined for, the first one met walking the
record from its first byte.  A declined site is not an error: the host loader parses it again and has the last word."""
import re

REASONS = ("ok", "range", "json", "transcript", "position", "key", "empty", "row", "number", "columns", "tail", "keys", "count", "norm",
           "vocabulary")
WS = b" \n\r\t"
TOKEN_BYTES = frozenset(b"0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ+-.")
NUMBER = re.compile(rb"-?(?:[0-9]+\.?[0-9]*|\.[0-9]+)\Z")
MAX_DIGITS, MAX_FRAC = 19, 27


def vocabulary():
    """the 66 5-mers of all N-DRACH-N 7-mers, sorted (m6anet/utils/constants.py)"""
    words = set()
    for a in "ACGT":
        for d in "AGT":
            for r in "GA":
                for h in "ACT":
                    for b in "ACGT":
                        k7 = a + d + r + "AC" + h + b
                        words.update(k7[i:i + 5] for i in range(3))
    return sorted(words)


def accepted(token):
    """whether the kernels convert this token (bytes)"""
    if not NUMBER.match(token):
        return False
    whole, _, frac = token.lstrip(b"-").partition(b".")
    return len((whole + frac).lstrip(b"0")) <= MAX_DIGITS and len(frac) <= MAX_FRAC


def value(token):
    return float(token)


def walk(rec, tx, pos, n_reads, norm_kmers=None):
    """(reason, rows, kmer) for the record `rec` (bytes) of data.info row (tx, pos, n_reads): rows are lists of ten floats, as far as
    the walk got; kmer is the sequence key (bytes) once the header is through.  norm_kmers: the 5-mers of the norm table, or None."""
    e = len(rec)

    def ws(i):
        while i < e and rec[i] in WS:
            i += 1
        return i

    def eat(i, c):
        i = ws(i)
        return i + 1 if i < e and rec[i] == c else None

    def string(i):
        i = ws(i)
        if i >= e or rec[i] != 0x22:
            return None
        i += 1
        q, bs = i, False
        while i < e and rec[i] != 0x22:
            if rec[i] == 0x5c:
                bs = True
                i += 1
            i += 1
        if i >= e:
            return None
        return i + 1, rec[q:i], bs

    def key(i):                                    # '{' "key" ':'
        i = eat(i, 0x7b)
        s = string(i) if i is not None else None
        if s is None:
            return None
        i = eat(s[0], 0x3a)
        return None if i is None else (i, s[1], s[2])

    rows = []
    k = key(0)
    if k is None:
        return "json", rows, None
    if k[1] != tx.encode():
        return "transcript", rows, None
    k = key(k[0])
    if k is None:
        return "json", rows, None
    if k[1] != str(pos).encode() or len(k[1].lstrip(b"-")) > 18:
        return "position", rows, None
    k = key(k[0])
    i = eat(k[0], 0x5b) if k is not None else None
    if i is None:
        return "json", rows, None
    kmer = k[1]
    if len(kmer) != 7 or k[2]:
        return "key", rows, None
    i = ws(i)
    if i < e and rec[i] == 0x5d:
        return "empty", rows, kmer
    while True:
        if i < e and rec[i] == 0x5b and len(rows) >= n_reads:
            return "count", rows, kmer
        if i >= e or rec[i] != 0x5b:
            return "row", rows, kmer
        i += 1
        row = []
        for j in range(10):
            i = ws(i)
            q = i
            while q < e and rec[q] in TOKEN_BYTES:
                q += 1
            if not accepted(rec[i:q]):
                return "number", rows, kmer
            row.append(value(rec[i:q]))
            i = ws(q)
            if i >= e or rec[i] != (0x2c if j < 9 else 0x5d):
                return "columns", rows, kmer
            i += 1
        rows.append(row)
        i = ws(i)
        if i < e and rec[i] == 0x2c:
            i = ws(i + 1)
            continue
        if i >= e or rec[i] != 0x5d:
            return "tail", rows, kmer
        i = ws(i + 1)
        if i < e and rec[i] == 0x2c:
            return "keys", rows, kmer
        for _ in range(3):
            i = eat(i, 0x7d)
            if i is None:
                return "tail", rows, kmer
        if ws(i) != e:
            return "tail", rows, kmer
        break
    if len(rows) != n_reads:
        return "count", rows, kmer
    fives = [kmer[c:c + 5].decode("latin-1") for c in range(3)]
    if norm_kmers is not None and any(f not in norm_kmers for f in fives):
        return "norm", rows, kmer
    if any(f not in VOCAB for f in fives):
        return "vocabulary", rows, kmer
    return "ok", rows, kmer


VOCAB = frozenset(vocabulary())
