"""The plain statement of dataprep (tests/eventalign_statement.py) against the reference's captured output, and the host's
m6a_io_dataprep_rows / m6a_io_dataprep + m6a_io_load_sites against the statement, bit for bit and in order, on every generated
family (tests/eventalign_gen.py) and three seeds.  tests/test_gpu_prep_edges.py holds the device to the same statement."""
import gzip
import json
import os

import numpy as np
import pytest

import eventalign_gen as G
import eventalign_statement as S
from m6anet_amd import _io
from m6anet_amd.constants import PRETRAINED_CONFIGS
from m6anet_amd.data_utils import load_norm_factors

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = [(f, s) for f in G.FAMILIES for s in G.SEEDS]


def hct116():
    return load_norm_factors(PRETRAINED_CONFIGS["HCT116_RNA002"][2])


def feature_bits(a):
    """float64 -> uint64, every NaN as the one NaN: 0 / 0 has no defined sign or payload, and data.json's text 'NaN' holds none"""
    a = np.array(a, np.float64)
    a[np.isnan(a)] = S.CANONICAL_NAN
    return a.view(np.uint64)


def statement_arrays(c):
    """the statement's table in the layout of _io.table_arrays"""
    K, NF = 5 + 2 * c.nn, 3 * (2 * c.nn + 1)
    rows = [row for r in c.runs for row in r.get("rows", [])]
    return dict(names=[n.decode() for n in c.names],
                run_tx=np.array([r["tx"] for r in c.runs], np.uint32), run_read=np.array([r["read"] for r in c.runs], np.int64),
                run_start=np.array([r["start"] for r in c.runs], np.int64), run_end=np.array([r["end"] for r in c.runs], np.int64),
                run_npos=np.array([r.get("npos", -1) for r in c.runs], np.int64),
                row_off=np.cumsum([0] + [len(r.get("rows", [])) for r in c.runs]).astype(np.int64),
                row_pos=np.array([row[0] for row in rows], np.int64),
                row_kmer=np.frombuffer(b"".join(row[1] for row in rows), np.uint8).reshape(len(rows), K),
                row_feat=np.array([row[2] for row in rows], np.float64).reshape(len(rows), NF))


def assert_table_is_the_statement(a, c, tag=""):
    """names and run columns; for every run whose status is 0, npos and the rows: positions, sequences, features bit for bit.
    Returns the status column."""
    st = statement_arrays(c)
    assert a["names"] == st["names"], tag
    for k in ("run_tx", "run_read", "run_start", "run_end"):
        assert np.array_equal(a[k], st[k]), (tag, k)
    ok = a["run_status"] == 0
    assert np.array_equal(a["run_npos"][ok], st["run_npos"][ok]), tag
    n_a, n_s = np.diff(a["row_off"]), np.diff(st["row_off"])
    assert np.array_equal(n_a[ok], n_s[ok]), tag
    pick_a = np.repeat(ok, n_a)                      # the rows of the runs that were not handed on, on either side
    pick_s = np.repeat(ok, n_s)
    assert np.array_equal(a["row_pos"][pick_a], st["row_pos"][pick_s]), tag
    assert np.array_equal(a["row_kmer"][pick_a], st["row_kmer"][pick_s]), tag
    assert np.array_equal(feature_bits(a["row_feat"][pick_a]), feature_bits(st["row_feat"][pick_s])), tag
    return a["run_status"]


def assert_sites_are_the_statement(X, km, off, tx_pos, read_ids, tx, kmer5, want, tag=""):
    assert len(tx_pos) == len(want["tx_pos"]) and len(read_ids) == len(want["read_ids"]), tag
    assert np.array_equal(np.ascontiguousarray(X).view(np.uint32), want["X"].view(np.uint32)), tag
    assert np.array_equal(km, want["km"]) and np.array_equal(off, want["off"]) and np.array_equal(tx_pos, want["tx_pos"]), tag
    assert np.array_equal(np.ascontiguousarray(read_ids).view(np.uint64), want["read_ids"].view(np.uint64)), tag
    assert list(tx) == want["tx"] and list(kmer5) == [k[1:6] for k in want["kmer7"]], tag


def message(e):
    return str(e.value).split(": ")[-1]


# ---- the statement is the reference's operation ----------------------------------------------------------------------------
def reference_records(text):
    out = []
    for line in text.splitlines():
        (tx, pp), = json.loads(line).items()
        (pos, k), = pp.items()
        (kmer, rows), = k.items()
        out.append((tx, int(pos), kmer, np.array(rows, np.float64)))
    return out


def multiset(a):
    a = feature_bits(a)
    return a[np.lexsort(a.T[::-1])]


@pytest.mark.parametrize("sub, capture, nn, kw, decimals", [
    ("ref_tests_data", "dataprep_ref_run/msc1", 1, dict(min_segment_count=1), None),
    ("ref_tests_data", "dataprep_ref_run/msc20_compress", 1, dict(min_segment_count=20), 3),
    ("dataprep_synthetic", "dataprep_synthetic/nn1", 1, dict(min_segment_count=5), None),
    ("dataprep_synthetic", "dataprep_synthetic/nn2", 2, dict(min_segment_count=5), None),
    ("dataprep_synthetic", "dataprep_synthetic/nn3", 3, dict(min_segment_count=5), None)])
def test_statement_reproduces_the_reference_capture(sub, capture, nn, kw, decimals):
    """Same index, same records in the same order, same sequences, and per site the same rows bit for bit as a multiset (the
    reference's order inside a site comes from an unstable argsort: tests/test_dataprep.py)."""
    data = gzip.open(os.path.join(GOLD, sub, "eventalign.txt.gz"), "rb").read()
    names, runs = S.table(data, nn)
    assert S.index_text(names, runs) == open(os.path.join(GOLD, sub, "eventalign.index")).read()
    got = S.records(names, runs, 1, 1000, **kw)
    want = reference_records(gzip.open(os.path.join(GOLD, capture + ".data.json.gz"), "rt").read())
    assert [r[:3] for r in got] == [r[:3] for r in want] and len(want) > 3
    for g, w in zip(got, want):
        feats = np.array([f for f, _ in g[3]], np.float64)
        rows = np.column_stack([feats if decimals is None else np.round(feats, decimals), [float(rd) for _, rd in g[3]]])
        assert np.array_equal(multiset(rows), multiset(w[3])), g[:2]


# ---- every family holds what it claims (from the statement alone) ------------------------------------------------------------
def matching_fields(data):
    for line in data.split(b"\n")[1:]:
        f = line.rstrip(b"\r").split(b"\t")
        if len(f) >= 15 and f[2] == f[9]:
            yield f


@pytest.mark.parametrize("family, seed", CASES)
def test_family_holds_what_it_claims(family, seed):
    c, spec = G.case(family, seed), G.FAMILIES[family]
    data = c.data
    assert len(data) < 4 << 20
    want_error = spec.get("error") or spec.get("rows_error") or spec.get("site_error")
    assert (c.error is None) == (want_error is None) and (c.error is None or (c.error[0] == want_error[0] and c.error[1].startswith(want_error[1])))
    if c.runs is not None and "rows_error" not in spec:
        declined = [S.declines(data, r) for r in c.runs]
        assert any(declined) == (bool(spec.get("declined")) or family == "midline")
    sizes = np.diff(c.sites["off"]) if c.sites is not None else None
    if family == "plain":
        every = [len(r[3]) for r in S.records(c.names, c.runs, min_segment_count=1)]
        assert (sizes >= 20).sum() >= 3 and min(every) < 20 and len({r["tx"] for r in c.runs}) == 3
    if family == "split_runs":
        reads = [r["read"] for r in c.runs if r["npos"] > 1]
        assert S.bits_for(max(reads) - min(reads)) + S.bits_for(len(c.names) - 1) > 64
        assert len(set((r["tx"], r["read"]) for r in c.runs)) * 2 == len(c.runs) and len(sizes) == 2
    if family == "split_rows":
        pos = [row[0] for r in c.runs for row in r["rows"]]
        widths = S.bits_for(1000), S.bits_for(max(pos) - min(pos)), S.bits_for(len(c.names) - 1)
        assert widths[0] + widths[1] > 64 and widths[1] + widths[2] <= 64 and min(pos) < 10 and max(pos) >= 10 ** 17
        assert len(sizes) == 8 and (sizes >= 20).all()
    if family.startswith("radix_") and family != "radix_ties":
        n = int(family.split("_")[1])
        assert sum(len(r["rows"]) for r in c.runs) == n == len(c.runs) and all(r["npos"] == 3 for r in c.runs)
        assert len(set((r["tx"], r["read"]) for r in c.runs)) == n and np.bincount([r["tx"] for r in c.runs]).max() <= 1001
        assert S.bits_for(len(c.names) - 1) % 4 != 0 or S.bits_for(1000) % 4 != 0           # widths that are not whole digits
    if family == "radix_ties":
        assert list(sizes) == [3000] and c.kw["readcount_max"] >= 3000
    if family.startswith("newlines_"):
        at = np.flatnonzero(np.frombuffer(data, np.uint8) == 10)
        assert (at % G.BLOCK == G.BLOCK - 1).any() and (at % G.BLOCK == 0).any() and (at % 16 == 15).any() and (at % 16 == 0).any()
        arr = np.frombuffer(data, np.uint8)
        lanes = arr[:len(arr) // 16 * 16].reshape(-1, 16)
        blocks = arr[:len(arr) // G.BLOCK * G.BLOCK].reshape(-1, G.BLOCK)
        assert (lanes == 10).all(axis=1).any() and (blocks == 10).all(axis=1).any() and np.diff(at).max() > G.BLOCK
        variant = int(family[-1])
        assert (len(data) % G.BLOCK == 0) == (variant != 1) and data.endswith(b"\n") == (variant == 0)
        assert (sizes >= 20).any()
    if family == "numbers_ok":
        fields = list(matching_fields(data))
        floats = {x for f in fields for x in f[6:9]}
        assert {b"123456789.012345", b".000000000000123", b"5.", b".5", b"000000095.310000"} <= floats
        assert all(len(f[1]) == 18 and len(f[13]) == 18 for f in fields) and b"\t1e5\t" in data and list(sizes) == [24]
    if family == "atoll":
        reads = {r["read"] for r in c.runs}
        assert {7, 8, -3, 12, S.I64_MAX, S.I64_MIN, 0, 42} <= reads and list(sizes) == [28]
    if family == "combine":
        feats = np.array([row[2] for r in c.runs for row in r["rows"]])
        assert np.isnan(feats).any() and np.isnan(c.sites["X"]).any() and any(r["npos"] == 0 for r in c.runs)
        per_group = {}
        for f in matching_fields(data):
            per_group[(f[3], f[1], f[2])] = per_group.get((f[3], f[1], f[2]), 0) + 1
        assert max(per_group.values()) > 300
        assert len({(k[0], k[1]) for k in per_group}) < len(per_group)                    # one position under two k-mers
    if family.startswith("windows_"):
        n_rows = [len(r["rows"]) for r in c.runs]
        # the plan of eventalign_gen.windows, twice: exact, one short either side, two overlapping windows (twice), a centre at
        # the first place, at the last, one before the first, at the stretch's end, inside it
        assert n_rows == [1, 0, 0, 2, 2, 1, 1, 0, 0, 1] * 2
        assert all(len(row[1]) == 5 + 2 * c.nn for r in c.runs for row in r["rows"])
    if family.startswith("filters_"):
        n = int(family.split("_")[1])
        loose = {(r[0], r[1]): len(r[3]) for r in S.records(c.names, c.runs, 1, 10 ** 6, 1)}
        assert loose[("FA", 5)] == n + 1 and loose[("FA", 14)] == n and loose[("FA", 23)] == n - 1
        assert loose[("FC", 5)] == n + 1 and loose[("FD", 14)] == 2 * n
        assert list(zip(c.sites["tx"], c.sites["tx_pos"], sizes)) == [("FA", 5, n + 1), ("FA", 14, n), ("FB", 5, n + 2), ("FD", 14, n + 5)]
        assert sum(r["tx"] == c.names.index(b"FB") for r in c.runs) == c.kw["readcount_min"]
        assert any(r["npos"] == 1 for r in c.runs)
    if family == "midline":
        cut = [r for r in c.runs if data[r["end"] - 1:r["end"]] != b"\n"]
        assert len(cut) == 2 and [S.declines(data, r) for r in c.runs].count(True) == 2 and list(sizes) == [24]
    if family == "declined":
        want = {200 + k for k, kind in enumerate(G.DECLINED_KINDS) if kind != "crlf_ok"}
        assert {r["read"] for r in c.runs if S.declines(data, r)} == want and b"\r\n" in data
        assert list(sizes) == [22 + len(G.DECLINED_KINDS) - 1]                               # all but `kmer4` have the row


# ---- the host equals the statement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family, seed", CASES)
def test_host_table_is_the_statement(tmp_path, family, seed):
    c, spec = G.case(family, seed), G.FAMILIES[family]
    ev, idx = c.write(tmp_path)
    if "error" in spec:
        with pytest.raises(_io.M6AIOError) as e:
            _io.host_rows(ev, c.nn, idx, n_threads=2)
        assert e.value.code == spec["error"][0] and message(e).startswith(spec["error"][1])
        return
    with _io.host_rows(ev, c.nn, idx, n_threads=2) as t:
        a = _io.table_arrays(t.contents)
    status = assert_table_is_the_statement(a, c)
    # a malformed line inside a run: the table marks that run alone (include/m6a_io.h), and writing the files is the error
    assert [i for i in np.flatnonzero(status)] == [i for i, r in enumerate(c.runs) if "npos" not in r][:1]


@pytest.mark.parametrize("family, seed", [(f, s) for f, s in CASES if G.FAMILIES[f].get("nn", 1) == 1])
def test_host_sites_are_the_statement(tmp_path, family, seed):
    c, spec = G.case(family, seed), G.FAMILIES[family]
    ev, idx = c.write(tmp_path)
    out = str(tmp_path / "out")
    if idx is not None:
        os.makedirs(out)
        open(os.path.join(out, "eventalign.index"), "w").write(c.index)
    if c.error is not None:
        with pytest.raises(_io.M6AIOError) as e:
            _io.dataprep(ev, out, n_threads=2, **c.kw)
        assert e.value.code == c.error[0] and message(e).startswith(c.error[1])
        return
    _io.dataprep(ev, out, n_threads=2, skip_index=idx is not None, **c.kw)
    if idx is None:
        assert open(os.path.join(out, "eventalign.index")).read() == S.index_text(c.names, c.runs)
    for norm in (None, hct116()):
        want = c.sites if norm is None else S.sites(c.names, c.runs, norm=norm, **c.kw)
        nat = _io.NativeSites([out], 20, norm, 2)
        S_ = len(nat.tx_pos)
        assert_sites_are_the_statement(nat.X, nat.site_kmers, nat.off, nat.tx_pos, nat.read_id_values, [nat.tx_id(i) for i in range(S_)],
                                       [nat.kmer5(i) for i in range(S_)], want, (family, seed, norm is not None))
        nat.close()
