"""Seeded directories (data.json + data.info.labelled) for compute_norm_factors, built on tests/json_gen.py as it is; what the routes
make of them is held to tests/norm_statement.py.  A family is a Dir: the path, the labelled rows as written, and which Train rows
the device must take (tests/json_statement.py's verdict less its two table checks)."""
import os
import random

import json_gen as JG
import json_statement as JS

READS = (1, 7, 8, 9, 15, 16, 63, 64, 65, 127, 128, 129, 135, 136, 137, 255, 256, 257, 264, 1000, 8191, 8192, 8193, 12000, 16385)
KMERS = (JG.KMER,) + JG.OTHER_KMERS          # in the 66-word vocabulary
OUTSIDE = "CCTGCAG"                          # no DRACH: three 5-mers the vocabulary does not hold
SINGLE = "CCCCGGG"                           # seen in one site of one read
SETS = ("Train", "Val", "Test")
HEADER = "transcript_id,transcript_position,start,end,n_reads,modification_status,set_type\n"

# what the loader says of json_gen.malformed()'s kinds here (no vocabulary check: "not DRACH" is a good site; a backslash in the key
# is left out -- the loader reads the key's raw bytes where json.loads refuses the escape, so the statement has no word on it)
MALFORMED_TEXT = {
    "9 columns": "7-mer with 9 columns", "11 columns": "7-mer with 11 columns", "ragged rows": "ragged rows",
    "empty row list": "7-mer with -1 columns", "5-mer key": "5-mer with 10 columns", "two sequence keys": "more than one sequence key",
    "wrong transcript": "is for transcript", "wrong position": "holds position", "bad number": "bad number", "truncated": "ENST_BAD:500",
    "not JSON": "bad JSON",
    "fewer reads": "site ENST_BAD:500: data.info.labelled says 4 reads, data.json has 3",
    "more reads": "site ENST_BAD:500: data.info.labelled says 2 reads, data.json has 3",
}


class Dir:
    def __init__(self, path, sites, rows):
        self.path, self.sites, self.rows = path, sites, rows       # rows: (site index, set_type) in the labelled file's order

    @property
    def train(self):
        return [self.sites[i] for i, st in self.rows if st == "Train"]

    def n_declined(self):
        """Train rows the kernels may decline: every other one they must take"""
        return sum(JS.walk(s.text, s.tx, s.pos, s.n_reads)[0] not in ("ok", "vocabulary") for s in self.train)


def write(path, sites, rows, position_as_float=False, junk=b"\n", lead=b"", ranges=None):
    """data.json = lead + the records in list order with junk between them; the labelled rows in the order given"""
    got = JG.write_dir(path, sites, junk=junk, lead=lead)
    os.remove(os.path.join(path, "data.info"))
    ranges = ranges or got
    with open(os.path.join(path, "data.info.labelled"), "w") as f:
        f.write(HEADER)
        for k, (i, st) in enumerate(rows):
            s = sites[i]
            pos = "%d.0" % s.pos if position_as_float and k % 2 else "%d" % s.pos
            f.write("%s,%s,%d,%d,%d,%d,%s\n" % (s.tx, pos, ranges[i][0], ranges[i][1], s.n_reads, k % 2, st))
    return Dir(path, sites, rows)


def edge_site(tx, pos, kmer):
    """every token of json_gen.numbers() in rows of ten (the tenth column is the read id, which no sum sees)"""
    toks = JG.numbers()
    rows = [toks[k:k + 10] for k in range(0, len(toks) - 9, 10)]
    return JG.Site(tx, pos, len(rows), JG.record(tx, pos, kmer, rows, dress=1) + "\n")


def sizes(path, seed=5):
    """every read count at which colsum takes another path, in the three dresses; 5-mers in and outside the vocabulary, AAAAAAA, one
    5-mer shared by several hundred sites, one seen in a single read; Train, Val and Test rows interleaved, a Train row twice, and
    the labelled rows in an order of their own"""
    rng = random.Random(seed)
    sites = []
    for k, n in enumerate(READS):
        kmer = (KMERS + (OUTSIDE, "AAAAAAA"))[k % 7]
        sites.append(JG.good_site(rng, "ENST_%d" % (k % 4), 100 + k, n, kmer, dress=k % 3))
    for k in range(300):                                            # the long chain: KMER's three 5-mers
        sites.append(JG.good_site(rng, "ENST_C", 1000 + k, 1 + k % 5, JG.KMER, dress=k % 3))
    sites.append(JG.good_site(rng, "ENST_S", 7, 1, SINGLE))
    sites.append(edge_site("ENST_E", 9, JG.OTHER_KMERS[0]))
    rows = [(i, "Train" if i < len(READS) or i % 3 else SETS[1 + i % 2]) for i in range(len(sites))]
    rows.append((3, "Train"))                                       # a row twice: counted twice
    rng.shuffle(rows)
    return write(path, sites, rows, position_as_float=True, lead=b"\n\n")


DECLINED_TWINS = (("1e-05", "0.00001"), ("1.5E+1", "15.0"), ("+1", "1"), ("0.12345678901234567890", "0.1234567890123456789"))


def declined(path, twin=False, seed=9):
    """declined-but-valid sites between regular ones that share their 5-mers; twin: the same values spelled as the kernels take them"""
    rng = random.Random(seed)
    sites = []
    for k, (tok, plain) in enumerate(DECLINED_TWINS):
        sites.append(JG.good_site(rng, "ENST_D", 10 * k, 9 + k, JG.KMER, dress=k % 3))
        rows = JG.plain_rows(rng, 130 + k)
        for r in (0, 64, 129):
            rows[r][(3 * k + r) % 9] = plain if twin else tok
        sites.append(JG.Site("ENST_D", 10 * k + 1, len(rows), JG.record("ENST_D", 10 * k + 1, JG.KMER, rows) + "\n"))
    rows = JG.plain_rows(rng, 5)
    sites.append(JG.Site("ENST_D", 90, 5, JG.record("ENST_D", 90, JG.KMER, rows, tail="\n" if twin else " junk\n")))
    sites.append(JG.good_site(rng, "ENST_D", 91, 20, JG.KMER))
    return write(path, sites, [(i, "Train") for i in range(len(sites))])


def nonfinite(path, seed=13):
    """NaN and the infinities, which only the host half reads: their 5-mers' factors are NaN, the others' untouched"""
    rng = random.Random(seed)
    sites = [JG.good_site(rng, "ENST_N", 1, 12, JG.KMER)]
    for k, tok in enumerate(("NaN", "Infinity", "-Infinity")):
        sites.append(JG.Site("ENST_N", 10 + k, 3, JG.with_token(rng, "ENST_N", 10 + k, tok).replace(JG.KMER, JG.OTHER_KMERS[k])))
        sites.append(JG.good_site(rng, "ENST_N", 20 + k, 4, JG.OTHER_KMERS[k]))
    return write(path, sites, [(i, "Train") for i in range(len(sites))])


def scaled(path, times, seed=17):
    """forty sites over five 7-mers; `times` x the reads per site"""
    rng = random.Random(seed)
    sites = [JG.good_site(rng, "ENST_X", k, times * (2 + k % 7), KMERS[k % 5], dress=k % 3) for k in range(40)]
    return write(path, sites, [(i, "Train") for i in range(len(sites))])


FAMILIES = {"sizes": sizes, "declined": declined, "declined twin": lambda p: declined(p, twin=True), "nonfinite": nonfinite,
            "scaled x1": lambda p: scaled(p, 1), "scaled x10": lambda p: scaled(p, 10)}


def malformed(path, name, seed=21):
    """the malformed site `name` of json_gen.malformed() between good ones; a second bad site behind it, which no route may report"""
    rng = random.Random(seed)
    bad = JG.malformed(rng)
    sites = [JG.good_site(rng, "ENST_G", 1, 70, JG.KMER), bad[name], JG.good_site(rng, "ENST_G", 2, 3, JG.OTHER_KMERS[1]),
             JG.Site("ENST_LATER", 1, 3, "x" * 30)]
    return write(path, sites, [(i, "Train") for i in range(len(sites))])


def out_of_range(path, seed=23):
    """a Train row whose byte range ends behind the file"""
    rng = random.Random(seed)
    sites = [JG.good_site(rng, "ENST_G", 1, 5, JG.KMER), JG.good_site(rng, "ENST_R", 2, 3, JG.KMER)]
    d = write(path, sites, [(0, "Train"), (1, "Train")])
    size = os.path.getsize(os.path.join(path, "data.json"))
    return write(path, sites, d.rows, ranges=[(0, len(sites[0].text)), (size - 10, size + 10)])
