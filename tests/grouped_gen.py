"""Eventalign files for `eventalign_inference --grouped`, built on eventalign_gen's File / Tx / site_reads; seeded, nothing stored.

    many    32 transcripts, one stretch each, about 100 KB of text each; three sites of 20 to 30 reads per transcript
    moved   `many` with the second half of transcript 11 moved behind transcript 12: not grouped, and MOVED says where
    one     a single transcript
    tail    four transcripts of three sites and a last one of one site: 13 sites, so the last flush group is a short one

file(name) -> bytes; moved_offender() -> (name, start) of the run the statement must name.
"""
import functools

import numpy as np

import eventalign_gen as G

SITES = (4, 14, 24)


def transcript(f, rng, t, sites=SITES, reads=None):
    """transcript t behind what f holds: every read covers all the sites in one stretch; returns the byte span of each read"""
    tx = G.Tx(rng, "GRP%03d.%d" % (t, 1 + t % 3), 10 + max(sites), sites, base=int(rng.integers(0, 5000)))
    spans = []
    for rd in rng.permutation(reads if reads is not None else int(rng.integers(20, 31))):
        at = f.size
        f.stretch(tx, tx.base + 2, max(sites) + 5, int(rd) + 1000 * t, mismatch=0)           # every event counts: a site has the transcript's reads
        spans.append((at, f.size))
    return tx, spans


def build(n_tx, seed, last_sites=None):
    rng = np.random.default_rng([seed, n_tx])
    f = G.File(rng)
    spans = []
    for t in range(n_tx):
        _, s = transcript(f, rng, t, last_sites if last_sites is not None and t == n_tx - 1 else SITES)
        spans.append(s)
    return f.bytes(), spans


MOVED_TX = 11


@functools.lru_cache(maxsize=None)
def _many():
    return build(32, 7)


@functools.lru_cache(maxsize=None)
def _moved():
    data, spans = _many()
    mine, nxt = spans[MOVED_TX], spans[MOVED_TX + 1]
    half = mine[len(mine) // 2][0]                          # the second half begins with a read of its own: a run starts there
    a, b, c = half, mine[-1][1], nxt[-1][1]
    assert b == nxt[0][0]
    out = data[:a] + data[b:c] + data[a:b] + data[c:]
    return out, a + (c - b)


@functools.lru_cache(maxsize=None)
def file(name):
    if name == "many":
        return _many()[0]
    if name == "moved":
        return _moved()[0]
    if name == "one":
        return build(1, 8)[0]
    if name == "tail":
        return build(5, 9, last_sites=(4,))[0]
    raise KeyError(name)


def moved_offender():
    """(transcript name, file offset) of the first run of the moved half"""
    data, at = _moved()
    return data[at:data.index(b"\t", at)], at


GROUPED_FILES = ("many", "one", "tail")
