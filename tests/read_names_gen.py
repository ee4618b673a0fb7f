"""Seeded eventalign files with read names in field 4 (`eventalign_inference --read_names`), each with its twin known by construction.

A family is an indexed file from tests/eventalign_gen.py's builders plus the names of its reads: case(family, seed) relabels the
read indices 0, 1, ... in order of first appearance (the twin) and writes names[index] in their place (the named file).
tests/read_names_statement.py's twin() must give the twin and the names back: test_read_names_core.py checks that, and that every
family gives at least one site, on the CPU.

    last_digit    (a) adjacent runs on one contig whose names differ only in the last hex digit
    first_digit   (b) ... only in the first digit
    same_hi       (c) equal high 64 bits, different low 64 bits
    same_lo       (d) equal low 64 bits, different high 64 bits
    decimal       (e) adjacent names with the same leading decimal digits (12ab..., 12cd...) and names that start with a letter:
                      a front half that still reads the field with atoll merges these runs
    descending    (f) names in descending order: sorted order is the reverse of first appearance
    again         (g) one name in two non-adjacent runs of one transcript (the duplicate rule), once with rows that change
    two_tx        (h) every name on two transcripts
    radix         (i) one more distinct name than one block of the radix sort holds (the number is read from m6a_prep.hip)
    windows       (j) for windows of 4 and 8 KB: every read runs on two transcripts one after the other, so that cuts fall between
                      two runs of one name, and runs are long enough for the window's end to fall inside one (cuts() says where)
    MALFORMED     (k) spellings that are no name, each on the first, a middle and the last body line of a small file; and one file
                      with a short line and a bad name, in both orders
"""
import functools
import os
import re

import numpy as np

import eventalign_gen as G
import eventalign_statement as S
import read_names_statement as RS

PREP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "m6anet_amd", "csrc", "m6a_prep_kit.h")


def radix_tile():
    """keys per block of radix_sort, from the code"""
    src = open(PREP).read()
    blk = int(re.search(r"constexpr int kBlk = (\d+);", src).group(1))
    items = int(re.search(r"constexpr int kRadixItems = (\d+),", src).group(1))
    return blk * items


def rand128(rng):
    return int.from_bytes(rng.bytes(16), "big")


def distinct(rng, n, make):
    out, seen = [], set()
    while len(out) < n:
        v = make()
        if v not in seen:
            seen.add(v)
            out.append(v)
    return out


# ---- the indexed files: read labels are arbitrary, relabel() makes them dense ----------------------------------------------------
def one_site(rng, n_reads=24, name="RN"):
    f = G.File(rng)
    tx = G.Tx(rng, name, 12, (3,))
    G.site_reads(f, tx, 3, range(n_reads), mismatch=0)
    return f.bytes()


def again(rng):
    f = G.File(rng)
    tx = G.Tx(rng, "AGAIN", 30, (3, 12))
    for rd in range(24):
        f.stretch(tx, 2, 3, rd, mismatch=0)
        f.stretch(tx, 11, 3, rd, mismatch=0)
        if rd == 8:                                        # read 3 again with other values: its rows change, its place stays
            f.stretch(tx, 2, 3, 3, mismatch=0)
            f.stretch(tx, 11, 3, 3, mismatch=0)
        if rd == 15:                                       # read 5 again with a single position: nothing changes
            f.stretch(tx, 11, 1, 5, mismatch=0)
    return f.bytes()


def two_tx(rng):
    f = G.File(rng)
    a, b = G.Tx(rng, "TWOA", 12, (3,)), G.Tx(rng, "TWOB", 12, (3,), base=700)
    G.site_reads(f, a, 3, range(24), mismatch=0)
    G.site_reads(f, b, b.base + 3, reversed(range(22)), mismatch=0)
    return f.bytes()


def radix(rng):
    n = radix_tile() + 1
    f = G.File(rng)
    tx = G.Tx(rng, "RADIX", 12, (3,))
    G.site_reads(f, tx, 3, range(12), mismatch=0, events=(1, 2))
    for rd in range(24, n):                                # a line each on other transcripts: a run, a name, no row
        f.line("RADIX%d" % (rd % 5), 9, "CCCCC", rd)
    G.site_reads(f, tx, 3, range(12, 24), mismatch=0, events=(1, 2))    # RADIX has 24 runs: all are counted
    return f.bytes()


def windows(rng):
    f = G.File(rng)
    a, b = G.Tx(rng, "WINA", 14, (3,)), G.Tx(rng, "WINB", 14, (4,), base=90)
    for rd in range(26):
        f.stretch(a, 2, 3 + rd % 4, rd, mismatch=0, events=(1, 4))
        f.stretch(b, b.base + 3, 3 + (rd + 2) % 4, rd, mismatch=0, events=(1, 4))
    return f.bytes()


# ---- the names, in index order ---------------------------------------------------------------------------------------------------
def names_last_digit(rng, n):
    bases = distinct(rng, (n + 15) // 16, lambda: rand128(rng) & ~15)
    return [bases[k // 16] | (k % 16) for k in range(n)]


def names_first_digit(rng, n):
    bases = distinct(rng, (n + 15) // 16, lambda: rand128(rng) & ((1 << 124) - 1))
    return [bases[k // 16] | (k % 16) << 124 for k in range(n)]


def names_same_hi(rng, n):
    hi = rand128(rng) >> 64 << 64
    return [hi | lo for lo in distinct(rng, n, lambda: rand128(rng) >> 64)]


def names_same_lo(rng, n):
    lo = rand128(rng) >> 64
    return [hi << 64 | lo for hi in distinct(rng, n, lambda: rand128(rng) >> 64)]


def names_decimal(rng, n):
    out = []
    for k in range(n):
        tail = rand128(rng) & ((1 << 112) - 1)
        if k < n // 2:                                     # 12ab..., 12ac..., ...: atoll reads 12 from every one
            out.append(0x12 << 120 | (10 + k % 6) << 116 | (10 + k // 6 % 6) << 112 | tail)
        else:                                              # a letter first: atoll reads 0
            out.append((10 + k % 6) << 124 | (k // 6 % 16) << 120 | (k % 16) << 116 | tail & ((1 << 116) - 1))
    assert len(set(out)) == n
    return out


def names_descending(rng, n):
    return sorted(distinct(rng, n, lambda: rand128(rng)), reverse=True)


def names_random(rng, n):
    return distinct(rng, n, lambda: rand128(rng))


FAMILIES = {
    "last_digit": (one_site, names_last_digit), "first_digit": (one_site, names_first_digit), "same_hi": (one_site, names_same_hi),
    "same_lo": (one_site, names_same_lo), "decimal": (one_site, names_decimal), "descending": (one_site, names_descending),
    "again": (again, names_random), "two_tx": (two_tx, names_random), "radix": (radix, names_random), "windows": (windows, names_random),
}
ARRAY_FAMILIES = [f for f in FAMILIES if f != "windows"]                 # (a) .. (i)
WINDOWS_KB = (4, 8)


def fields(line):
    """(start, end) of field 4 of a body line with at least three tabs"""
    t1 = line.index(b"\t")
    t3 = line.index(b"\t", line.index(b"\t", t1 + 1) + 1)
    t4 = line.find(b"\t", t3 + 1)
    return t3 + 1, len(line) if t4 < 0 else t4


def relabel(data, names_of, by_label=None):
    """(twin, named, names): the read labels of an indexed file made dense in order of first appearance, and names_of(n) -> the n
    names in index order written in their place (or by_label(label) -> the name of the read with that label).  Every body line of
    these files has its 15 fields."""
    lines = data.split(b"\n")
    assert lines[-1] == b""
    ids = {}
    for line in lines[1:-1]:
        a, b = fields(line)
        ids.setdefault(line[a:b], len(ids))
    names = names_of(len(ids)) if by_label is None else [by_label(label) for label in ids]
    assert len(set(names)) == len(names)
    twin, named = [lines[0]], [lines[0]]
    for line in lines[1:-1]:
        a, b = fields(line)
        k = ids[line[a:b]]
        twin.append(line[:a] + b"%d" % k + line[b:])
        named.append(line[:a] + RS.show(names[k]) + line[b:])
    return b"\n".join(twin) + b"\n", b"\n".join(named) + b"\n", names


class Named:
    def __init__(self, family, seed):
        make, names_of = FAMILIES[family]
        rng = np.random.default_rng([seed, sorted(FAMILIES).index(family), 128])
        self.family, self.seed = family, seed
        self.twin, self.named, self.names = relabel(make(rng), lambda n: names_of(rng, n))

    def write(self, tmp_path):
        """(named path, twin path)"""
        out = []
        for tag, data in (("named", self.named), ("twin", self.twin)):
            p = tmp_path / ("%s_%d_%s.txt" % (self.family, self.seed, tag))
            p.write_bytes(data)
            out.append(str(p))
        return out


@functools.lru_cache(maxsize=None)
def case(family, seed=1):
    return Named(family, seed)


@functools.lru_cache(maxsize=None)
def replicates(fixture="split"):
    """[(named, twin, names)] of the files of a replicate fixture (tests/replicate_fixtures.py): a read index of the bundled file has
    one name wherever it occurs, every 50th read of a later file carries the name of a read of the first file, and each file's twin numbers its own
    reads from 0"""
    import replicate_fixtures as F
    rng, book = np.random.default_rng(77), {}

    def by_label(label):
        if label not in book:
            book[label] = rand128(rng)
        return book[label]
    out = []
    for letter in F.FIXTURES[fixture]:
        data = F.parts()[letter]
        if out:                                            # every 50th read of this file carries the name of a read of the first
            mine = list(dict.fromkeys(line[slice(*fields(line))] for line in data.split(b"\n")[1:-1]))
            for here in range(0, min(len(mine), len(out[0][2]) - 3), 50):
                book.setdefault(mine[here], out[0][2][here + 3])
        twin, named, names = relabel(data, None, by_label)
        out.append((named, twin, names))
    return out


def shared_in_pooled_sites(reps, min_reads=20):
    """the names that two files of replicates() both give to a read of one pooled site (min_segment_count 1, >= min_reads reads summed)"""
    per_site = {}
    for k, (_, twin, names) in enumerate(reps):
        tx, runs = S.table(twin, 1)
        for name, position, _, rows in S.records(tx, runs, min_segment_count=1):
            per_site.setdefault((name, position), []).append((k, {names[read] for _, read in rows}))
    out = set()
    for parts in per_site.values():
        if sum(len(r) for _, r in parts) >= min_reads:
            for i, (_, a) in enumerate(parts):
                for _, b in parts[i + 1:]:
                    out |= a & b
    return out


def n_sites(twin):
    """sites the statement finds in a twin file with the default flags"""
    names, runs = S.table(twin, 1)
    return len(S.sites(names, runs)["tx_pos"])


# ---- where the windows of a named file are cut (include/m6a.h: m6a_prep_sites_build_windows, runs keyed by the name) ------------------
def cuts(data, W):
    """[(b, e, next b, kinds)] per window: kinds holds 'same_name' when the run in front of the next window's first run carries its
    name (on another contig), and 'inside' when the window's end e lies inside the run that moves to the next window."""
    n, b, out = len(data), 0, []
    while True:
        size = W
        while True:
            last = b + size >= n
            e = n if last else data.rfind(b"\n", b, b + size) + 1
            lines, p = [], b
            while p < e:
                q = data.find(b"\n", p, e)
                q = e if q < 0 else q + 1
                lines.append((p, data[p:q]))
                p = q
            body = [(p, l) for p, l in lines[(1 if b == 0 else 0):] if b"\t" in l]
            runs = []
            for p, l in body:
                a, z = fields(l.rstrip(b"\n"))
                key = (l[:l.index(b"\t")], l[a:z])
                if not runs or runs[-1][1] != key:
                    runs.append((p, key))
            if last or (len(runs) > 1):
                break
            size *= 2
        if last:
            out.append((b, e, n, set()))
            return out
        kinds = set()
        if runs[-2][1][1] == runs[-1][1][1]:
            kinds.add("same_name")
        q = data.find(b"\n", e)
        nxt = data[e:n if q < 0 else q]                    # the first line behind the window: of the run that moves?
        if b"\t" in nxt and (nxt[:nxt.index(b"\t")], nxt[slice(*fields(nxt))]) == runs[-1][1]:
            kinds.add("inside")
        out.append((b, e, runs[-1][0], kinds))
        b = runs[-1][0]


# ---- (k) what is no name ------------------------------------------------------------------------------------------------------------
GOOD = b"3f2a9c1e-7b4d-4e8a-9f10-5c6d7e8f9a0b"
SPELLINGS = {
    "upper": GOOD.upper(), "one_upper": GOOD[:30] + b"F" + GOOD[31:], "short35": GOOD[:-1], "long37": GOOD + b"0",
    "dash_moved": GOOD[:8] + GOOD[9:10] + b"-" + GOOD[10:], "no_dash": GOOD.replace(b"-", b"0"), "integer": b"1234", "empty": b"",
    "non_hex": GOOD[:5] + b"g" + GOOD[6:], "blank_first": b" " + GOOD[1:],
}
PLACES = ("first", "middle", "last")


def small(rng):
    """(lines, names): 24 reads of one site, every line named"""
    _, named, names = relabel(one_site(rng, 24, "BAD"), lambda n: names_random(rng, n))
    return named.split(b"\n")[:-1], names


def with_field(line, text):
    a, b = fields(line)
    return line[:a] + text + line[b:]


@functools.lru_cache(maxsize=None)
def malformed(spelling, place):
    """(file bytes, the file offset of the bad field)"""
    lines, _ = small(np.random.default_rng([5, sorted(SPELLINGS).index(spelling)]))
    k = {"first": 1, "middle": len(lines) // 2, "last": len(lines) - 1}[place]
    at = sum(len(l) + 1 for l in lines[:k]) + fields(lines[k])[0]
    lines = lines[:k] + [with_field(lines[k], SPELLINGS[spelling])] + lines[k + 1:]
    return b"\n".join(lines) + b"\n", at


@functools.lru_cache(maxsize=None)
def short_and_bad(short_first):
    """(file bytes, the expected text): a line of two tabs and a line with a bad name; the lower offset is reported"""
    lines, _ = small(np.random.default_rng([6, int(short_first)]))
    i, j = len(lines) // 3, 2 * len(lines) // 3
    ks, kb = (i, j) if short_first else (j, i)
    lines[ks] = b"ctg\t1\tAAAAA"
    lines[kb] = with_field(lines[kb], SPELLINGS["upper"])
    off = lambda k: sum(len(l) + 1 for l in lines[:k])
    text = "short line at byte %d" % off(ks) if short_first else "read name at byte %d: not a lowercase UUID" % (off(kb) + fields(lines[kb])[0])
    return b"\n".join(lines) + b"\n", text
