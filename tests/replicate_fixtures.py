"""Replicate fixtures: files cut from tests/golden/ref_tests_data/eventalign.txt.gz by whole runs (5 107 runs in 82 transcripts).

    split     a = the even runs, b = the odd runs: the pooled sites are the unsplit file's, and most of them have every part < 20
    three     a, b, c -- c = every third run, its transcripts in REVERSE order of first appearance (global ids unsorted in a file)
    c_first   c, a: the union's order is led by the reordered file
    overlap   e = all runs of transcripts 0..54, d = all runs of transcripts 30..81: sites that only the later file has
    gap       d, h (header only), e: an empty replicate keeps its number
    twice     the bundled file twice: the reference's own replicate run (tests/golden/replicate_*.csv)
"""
import gzip
import os

import eventalign_statement as S

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = {"split": "ab", "three": "abc", "c_first": "ca", "overlap": "ed", "gap": "dhe", "twice": "ww"}
_parts = {}


def parts():
    """{letter: bytes} of the files above"""
    if _parts:
        return _parts
    data = gzip.open(os.path.join(GOLD, "ref_tests_data", "eventalign.txt.gz"), "rb").read()
    header = data[:data.find(b"\n") + 1]
    names, runs = S.index(data)
    assert len(runs) == 5107 and len(names) == 82

    def cut(picked):
        return header + b"".join(data[r["start"]:r["end"]] for r in picked)
    third = runs[0::3]
    _parts.update(w=data, h=header, a=cut(runs[0::2]), b=cut(runs[1::2]),
                  c=cut([r for t in reversed(range(len(names))) for r in third if r["tx"] == t]),
                  e=cut([r for r in runs if r["tx"] <= 54]), d=cut([r for r in runs if r["tx"] >= 30]))
    return _parts


def write(tmp_path, fixture):
    """the fixture's files in tmp_path, in command-line order (the same letter twice is the same path twice)"""
    out = []
    for letter in FIXTURES[fixture]:
        p = tmp_path / ("rep_%s.txt" % letter)
        if not p.exists():
            p.write_bytes(parts()[letter])
        out.append(str(p))
    return out
