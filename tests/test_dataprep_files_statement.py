"""The four files of `dataprep --device cpu` (m6a_io.cpp) are the bytes the two plain statements give from eventalign.txt alone
(tests/eventalign_statement.py joined to tests/dataprep_json_statement.py by from_eventalign): every family of tests/eventalign_gen.py
and tests/dataprep_gen.py, every seed, --compress off and on -- the spelling of NaN, of -0.0 and of repr's scientific form, the offsets
of data.info and the lines of data.log included.  And every family of dataprep_gen holds what it claims, from the statement alone.
tests/test_gpu_dataprep_families.py holds both device routes to the same bytes."""
import os

import numpy as np
import pytest

import dataprep_gen as DG
import dataprep_json_statement as D
import eventalign_statement as S
from m6anet_amd import _io

NEW_CASES = [(f, s) for f in DG.FAMILIES for s in DG.SEEDS]
# (family, seed, min_segment_count or None for the family's own): windows_2 and windows_3 have 20 runs, so their own filters keep no site
CASES = [(f, s, None) for f in DG.ALL for s in DG.SEEDS] + [(f, s, 1) for f in ("windows_2", "windows_3") for s in DG.SEEDS]


def message(e):
    return str(e.value).split(": ")[-1]


def no_files(d):
    return not any(os.path.exists(os.path.join(d, f)) for f in DG.FILES)


def assert_files(d, want, tag):
    for name in DG.FILES:
        got = open(os.path.join(d, name), "rb").read()
        if got != want[name]:
            at = next((i for i, (a, b) in enumerate(zip(got, want[name])) if a != b), min(len(got), len(want[name])))
            raise AssertionError("%s %s: %d bytes for %d, first difference at byte %d: %r for %r"
                                 % (tag, name, len(got), len(want[name]), at, got[max(0, at - 30):at + 30], want[name][max(0, at - 30):at + 30]))


# ---- every new family holds what it claims (from the statement alone) -----------------------------------------------------------------
def all_features(sites):
    return np.array([f for s in sites for f in s[3]], np.float64).reshape(-1, 9)


@pytest.mark.parametrize("family, seed", NEW_CASES)
def test_family_holds_what_it_claims(family, seed):
    c = DG.case(family, seed)
    assert len(c.data) < 1 << 20 and DG.generate(family, seed) == c.data
    sites, runs, logged = DG.parts(family, seed)
    nd = {compress: D.n_declined(sites, compress) for compress in (False, True)}
    assert nd[False] == 0 and (nd[True] > 0) == (family == "values_rounding")
    reads = [r for s in sites for r in s[4]]
    if family == "long_names":
        assert c.kw == dict(min_segment_count=1) and not any(S.declines(c.data, r) for r in c.runs)
        # the tiles are those of the plain text (--compress makes every number of data.json shorter) and of the index under either
        # (in data.json only a record's first row carries the name, so there a row over a tile never follows a shorter one)
        # a json row's offset is its place in data.json; an index row's is its place behind the header, as the device counts it
        text = D.files(sites, runs, logged)
        jrows, xrows = DG.json_rows(sites), DG.index_rows(runs)
        assert jrows[0][0][0] == 0 and all(text["data.json"][rows[0][0]:rows[-1][0] + rows[-1][1]] == D.record(*s) for rows, s in zip(jrows, sites))
        body = text["eventalign.index"][len(D.INDEX_HEADER):]
        assert xrows[0][0] == 0 and [body[a:a + n] for a, n in xrows] == [D.index_row(*r) for r in runs]
        assert DG.tile_edges(jrows) >= DG.TILE_EDGES - {"long_after_short"}
        assert DG.tile_edges(DG.index_waves(xrows)) >= DG.TILE_EDGES
        # the pads are the device's: counted from the start of the file, 43 bytes further, the index would hold other edges
        assert len(D.INDEX_HEADER) % 4 != 0
        sizes = sorted(len(n) for n in c.names)
        assert sizes[0] == 3 and sizes[-1] >= 12000 and any(4060 <= n <= 4096 for n in sizes)
        assert max(len(l) for l in c.data.split(b"\n")) > 2 * 4096 + 12000 - 8192
        assert len({len(str(s[1])) for s in sites}) >= 4                                # positions of several digit counts
        assert max(len(s[4]) for s in sites) == 3 and len(sites) >= 20
    if family == "big_site":
        assert [len(s[4]) for s in sites] == [3000] and c.kw["readcount_max"] >= 3000
        assert min(reads) == 0 and max(reads) == 2 ** 53 - 1 and {len(str(r)) for r in reads} == set(range(1, 17))
        assert len(D.record(*sites[0])) > 200000
    if family == "index_wide":
        wide = [r[1] for r in runs if r[0] == "IWB"]
        assert len(wide) == 16 and set(DG.WIDE_16) <= set(wide) and max(wide) - min(wide) == 2 ** 64 - 1
        assert [(s[0], len(s[4])) for s in sites] == [("IWA", 24)] and logged == ["IWA", "IWB"]
        assert [r[0] for r in runs] == ["IWA"] * 12 + ["IWB"] * 16 + ["IWA"] * 12
        assert max(len(D.index_row(*r)) for r in runs if r[0] == "IWB") >= 4 + 20 + 4 + 4
    if family == "big_positions":
        pos = [s[1] for s in sites]
        assert len(sites) == 8 and all(len(s[4]) == 22 for s in sites) and min(pos) < 10 and max(pos) >= 9 * 10 ** 17
        assert all(0 <= r < 2 ** 53 for r in reads) and len({len(str(r)) for r in reads}) >= 10
        assert len({r[0] for r in runs[:4]}) == 4                                       # interleaved: a transcript's runs are not adjacent
    if family.startswith("values_"):
        spelled = DG.TAKEN + (DG.ROUNDED_AWAY if family == "values_rounding" else [])
        fields = [l.split(b"\t") for l in c.data.split(b"\n")[1:] if l]
        assert all(int(f[14]) - int(f[13]) == 1 and f[2] == f[9] for f in fields)
        feats = all_features(sites)
        assert len(sites) == 1 and len(feats) == max(24, len(spelled)) + 2
        for k, column in ((7, feats[:, 1::3]), (8, feats[:, 0::3])):                    # event_stdv -> sd, event_length -> dwell
            assert {f[k].decode() for f in fields} >= set(spelled)
            assert {float(x) for x in spelled} <= set(column.ravel().tolist())
        handed = [r["read"] for r in c.runs if S.declines(c.data, r)]
        assert handed == [100, 101] and 0.30000000000000004 in feats and 1.2345678901234567 in feats
        texts = D.record(*sites[0])
        assert "0.30000000000000004" in texts and "999999999999999.0" in texts and "0.0015" in texts
        if family == "values_rounding":
            rounded = np.round(np.array([float(x) for x in DG.ROUNDED_AWAY]), 3)
            assert (rounded == 0).all() and "0.0001," in texts and nd[True] == int((np.round(feats, 3) == 0).sum())
    # every candidate spelling the issue names is in one list or the other
    assert set(DG.TAKEN + DG.ROUNDED_AWAY) >= {"0.0001", "0.00010000000001", "0.0005", "0.0015", "0.0025", "2.675", "1.0005", "999999999999999",
                                               "9999999999999.99", "123456789.012345", ".5", "5.", "0.00025", "0.0004", "0.00049999"}


def test_statement_spells_what_is_not_finite_and_takes_wider_rows():
    assert [D.number(v) for v in (float("nan"), float("inf"), -float("inf"), -0.0, 1e-5, 1e16)] == ["NaN", "Infinity", "-Infinity", "-0.0", "1e-05", "1e+16"]
    assert D.number(float("nan"), True) == "NaN" and D.number(0.0004, True) == "0.0" and D.number(-0.0004, True) == "-0.0"
    assert D.record("t", 7, "AAGACTTCC", [[1.0] * 15], [3]) == '{"t":{"7":{"AAGACTTCC":[[' + "1.0," * 15 + '3.0]]}}}\n'
    with pytest.raises(AssertionError):
        D.record("t", 7, "AAGACTT", [[1.0] * 15], [3])


# ---- the host writer is the statement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compress", [False, True])
@pytest.mark.parametrize("family, seed, msc", CASES)
def test_host_files_are_the_statement(tmp_path, family, seed, msc, compress):
    c = DG.case(family, seed)
    ev, idx = c.write(tmp_path)
    out = str(tmp_path / "out")
    kw = dict(c.kw) if msc is None else dict(c.kw, min_segment_count=msc)
    if idx is not None:                                           # midline: its own index, cut inside two lines
        os.makedirs(out)
        open(os.path.join(out, "eventalign.index"), "w").write(c.index)
    if c.error is not None:
        with pytest.raises(_io.M6AIOError) as e:
            _io.dataprep(ev, out, n_threads=2, n_neighbors=c.nn, compress=compress, device="cpu", **kw)
        assert e.value.code == c.error[0] and message(e).startswith(c.error[1])
        assert no_files(out)
        return
    _io.dataprep(ev, out, n_threads=2, n_neighbors=c.nn, compress=compress, skip_index=idx is not None, device="cpu", **kw)
    want, _ = DG.expected(family, seed, compress, msc)
    assert_files(out, want, (family, seed, msc, compress))
    if family == "midline":
        assert want["eventalign.index"] == c.index.encode()
    if msc == 1:
        assert want["data.json"].count(b"\n") >= 5
