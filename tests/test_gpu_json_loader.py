"""`inference --loader device` (m6a_json_sites_build, include/m6a.h): data.json parsed by HIP kernels.  The handle's arrays equal
m6a_io_load_sites' on the same directory -- X bit for bit, k-mer ids, offsets, positions, read ids, transcripts and 5-mers -- on the
golden directories and on generated ones (tests/json_gen.py) whose sites sit at the edges of the kernels: 1, 63, 64, 65 and
12 000 reads, records at byte 0 and at the file's end, data.info out of order, junk between records, the edge numbers of the
conversion, declined sites among regular ones.  Errors are the loader's own code and text; only read ids and a status byte per site
come back; the command writes the bytes `--loader host` writes."""
import gzip
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import json_gen as JG
import json_statement as JS
from m6anet_amd import _io
from m6anet_amd.constants import PRETRAINED_CONFIGS
from m6anet_amd.data_utils import load_norm_factors

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")
CSVS = ("data.site_proba.csv", "data.indiv_proba.csv")


def hct116():
    return load_norm_factors(PRETRAINED_CONFIGS["HCT116_RNA002"][2])


def equal_the_loader(d, min_reads, norm, name=""):
    """json_sites(d) against NativeSites([d]); returns (n_sites, n_reads, n_declined, d2h bytes)"""
    nat = _io.NativeSites([d], min_reads, norm, 4)
    try:
        with _io.json_sites(d, min_reads, norm, 4) as p:
            X, km, off = p.inputs()
            S = len(nat.tx_pos)
            assert p.n_sites == S and p.n_reads == nat.X.shape[0], name
            assert np.array_equal(off, nat.off) and np.array_equal(p.off, nat.off), name
            bad = np.flatnonzero((X.view(np.uint32) != nat.X.view(np.uint32)).any(axis=1))
            assert bad.size == 0, (name, bad[:5], X[bad[:2]], nat.X[bad[:2]])
            assert np.array_equal(km, nat.site_kmers), name
            assert np.array_equal(p.tx_pos, nat.tx_pos), name
            assert np.array_equal(p.read_ids.view(np.uint64), nat.read_id_values.view(np.uint64)), name
            assert [p.names[t] for t in p.site_tx] == [nat.tx_id(i) for i in range(S)], name
            assert [bytes(k[1:6]).decode() for k in p.kmer7] == [nat.kmer5(i) for i in range(S)], name
            assert p.n_replicates == 1 and p.n_windows == 1 and p.n_bgzf_blocks == 0 and not p.read_rep.any(), name
            ms, d2h = p.times()
            assert ms["newlines"] == 0 and ms["parse_combine_windows"] == 0 and ms["total"] > 0, ms
            return S, p.n_reads, p.n_declined_sites, d2h - 8 * p.n_reads - 36 * p.n_reads - 3 * S - 8 * (S + 1)     # less inputs()' copies
    finally:
        nat.close()


def golden_dir(tmp_path, name):
    if name == "ref_tests_data":
        return os.path.join(GOLD, name)
    d = tmp_path / name.replace("/", "_")
    d.mkdir()
    (d / "data.json").write_bytes(gzip.open(os.path.join(GOLD, name + ".data.json.gz")).read())
    (d / "data.info").write_bytes(open(os.path.join(GOLD, name + ".data.info"), "rb").read())
    return str(d)


@pytest.mark.parametrize("name", ["ref_tests_data", "dataprep_ref_run/msc1", "dataprep_synthetic/nn1"])
def test_golden_arrays_equal_the_loader(tmp_path, name):
    d = golden_dir(tmp_path, name)
    for norm in (None, hct116()):
        for min_reads in (20, 1):
            try:
                _io.NativeSites([d], min_reads, norm, 4).close()
            except _io.M6AIOError as want:                       # a directory without a site of 20 reads: the loader's own words
                with pytest.raises(_io.M6AIOError) as got:
                    _io.json_sites(d, min_reads, norm, 4)
                assert (got.value.code, str(got.value)) == (want.code, str(want)) and "no site with at least" in str(want)
                continue
            S, R, declined, extra = equal_the_loader(d, min_reads, norm, name)
            assert declined == 0 and extra == S, (name, declined, extra)     # ids + a status byte per site + nothing


def edge_sites(rng, declined=False):
    """sites of 1, 63, 64, 65 and 12 000 reads, one made of the edge numbers, in three dresses; with declined-but-valid ones between"""
    sizes = (1, 63, 64, 65, 12000, 2, 130)
    sites = [JG.good_site(rng, "ENST%d" % (k % 3), 100 + k, n, ((JG.KMER,) + JG.OTHER_KMERS)[k % 5], dress=k % 3,
                          first_id=k * 7) for k, n in enumerate(sizes)]
    toks = JG.numbers()
    rows = [toks[k:k + 10] for k in range(0, len(toks) - 9, 10)]
    sites.append(JG.Site("ENST_EDGE", 5, len(rows), JG.record("ENST_EDGE", 5, JG.KMER, rows, dress=1) + "\n"))
    if declined:
        for k, s in enumerate(JG.declined_valid(rng)):
            sites.insert(1 + 2 * k if 1 + 2 * k < len(sites) else len(sites), s)
    sites[-1].text = sites[-1].text.rstrip(b"\n")                    # the last record ends at the file's end
    return sites


@pytest.fixture(scope="module")
def edge_dirs(tmp_path_factory):
    base = tmp_path_factory.mktemp("json_edges")
    rng = random.Random(21)
    plain, mixed = edge_sites(rng), edge_sites(rng, declined=True)
    order = list(range(len(plain)))
    random.Random(2).shuffle(order)
    JG.write_dir(str(base / "plain"), plain)                                            # first record at byte 0, last at the end
    JG.write_dir(str(base / "shuffled"), plain, info_order=order, junk=b"\n[[junk]] {\"x\": [1e5\n", lead=b"# not a record\n", trail=b"\n]]")
    JG.write_dir(str(base / "mixed"), mixed, junk=b"\n")
    return {"plain": (str(base / "plain"), plain), "shuffled": (str(base / "shuffled"), plain), "mixed": (str(base / "mixed"), mixed)}


def test_generated_edges_equal_the_loader(edge_dirs):
    extras = []
    for tag in ("plain", "shuffled"):
        d, sites = edge_dirs[tag]
        for norm in (None, hct116()):
            S, R, declined, extra = equal_the_loader(d, 1, norm, tag)
            assert S == len(sites) and R == sum(s.n_reads for s in sites) and declined == 0
            extras.append(extra - S)
    assert extras == [0] * len(extras)             # device -> host: the read ids, one status byte per site, and a constant (0)
    S20 = equal_the_loader(edge_dirs["plain"][0], 20, None, "min_reads 20")[0]
    assert S20 == sum(1 for s in edge_dirs["plain"][1] if s.n_reads >= 20)


def test_declined_sites_come_out_the_hosts(edge_dirs):
    d, sites = edge_dirs["mixed"]
    for norm in (None, hct116()):
        want = sum(1 for s in sites if JS.walk(s.text, s.tx, s.pos, s.n_reads, None if norm is None else set(norm))[0] != "ok")
        assert want == len(JG.declined_valid(random.Random(0)))
        S, R, declined, _ = equal_the_loader(d, 1, norm, "mixed")
        assert declined == want and S == len(sites)
    # a norm table that lacks a 5-mer of one kind of site: those sites are declined, and the loader's error is the answer
    norm = {k: v for k, v in hct116().items() if k != JG.OTHER_KMERS[0][:5]}
    with pytest.raises(_io.M6AIOError) as want:
        _io.NativeSites([d], 1, norm, 4)
    with pytest.raises(_io.M6AIOError) as got:
        _io.json_sites(d, 1, norm, 4)
    assert (got.value.code, str(got.value)) == (want.value.code, str(want.value)) and "no normalisation factors for" in str(got.value)


def test_small_chunks_give_the_same_arrays(edge_dirs, monkeypatch):
    monkeypatch.setenv("M6A_PREP_CHUNK_KB", "4")             # every header that straddles a 4 KB edge is read from the file
    for tag in ("shuffled", "mixed"):
        equal_the_loader(edge_dirs[tag][0], 1, hct116(), tag + " in 4 KB chunks")
    equal_the_loader(os.path.join(GOLD, "ref_tests_data"), 20, hct116(), "ref_tests_data in 4 KB chunks")


def test_over_budget_names_the_host_loader(edge_dirs, monkeypatch):
    d = edge_dirs["plain"][0]
    assert os.path.getsize(os.path.join(d, "data.json")) > 1 << 20
    monkeypatch.setenv("M6A_PREP_BUDGET_MB", "1")
    with pytest.raises(_io.M6AIOError) as e:
        _io.json_sites(d, 1, None, 4)
    assert e.value.code == -2 and "--loader host" in str(e.value)
    monkeypatch.delenv("M6A_PREP_BUDGET_MB")
    equal_the_loader(d, 1, None, "after the budget error")


def test_errors_are_the_loaders(tmp_path):
    rng = random.Random(9)
    valid = JG.declined_valid(rng)[0]
    later = JG.malformed(rng, "ENST_LATER", 9)["not DRACH"]
    good = JG.good_site(rng, "ENST_OK", 1, 70)
    cases = dict(JG.malformed(rng))
    for name, s in cases.items():
        d = str(tmp_path / name.replace(" ", "_"))
        JG.write_dir(d, [good, valid, s, good2(rng), later], junk=b"\n")
        check_error(d, name)
    # ranges outside the file: behind its end, before its start, empty
    for k, (a, b) in enumerate(((10, 10 ** 9), (-5, 40), (30, 30))):
        d = str(tmp_path / ("range%d" % k))
        JG.write_dir(d, [good, valid, good2(rng), later], junk=b"\n")
        lines = open(os.path.join(d, "data.info")).read().splitlines()
        f = lines[3].split(",")
        lines[3] = ",".join(f[:2] + [str(a), str(b), f[4]])
        open(os.path.join(d, "data.info"), "w").write("\n".join(lines) + "\n")
        assert "byte range outside data.json" in check_error(d, "range %d" % k)
    d = str(tmp_path / "fine")
    JG.write_dir(d, [good, valid, good2(rng)], junk=b"\n")
    assert equal_the_loader(d, 1, hct116(), "after the errors")[2] == 1


def good2(rng):
    return JG.good_site(rng, "ENST_OK", 2, 5, JG.OTHER_KMERS[1], dress=1)


def check_error(d, name):
    with pytest.raises(_io.M6AIOError) as want:
        _io.NativeSites([d], 1, None, 4)
    with pytest.raises(_io.M6AIOError) as got:
        _io.json_sites(d, 1, None, 4)
    assert (got.value.code, str(got.value)) == (want.value.code, str(want.value)), name
    return str(got.value)


def run(args, check=True):
    return subprocess.run([sys.executable, "-m", "m6anet_amd"] + args, cwd=REPO, timeout=600, check=check, stdout=subprocess.PIPE, stderr=subprocess.PIPE)


@pytest.mark.parametrize("flags", [[], ["--drop_unflushed_tail"]])
def test_command_writes_the_host_loaders_bytes(tmp_path, flags):
    d = os.path.join(GOLD, "ref_tests_data")
    outs = {}
    for loader in ("host", "device"):
        out = str(tmp_path / loader)
        run(["inference", "--input_dir", d, "--out_dir", out, "--num_iterations", "100", "--loader", loader] + flags)
        outs[loader] = [open(os.path.join(out, f), "rb").read() for f in CSVS]
    assert outs["host"] == outs["device"] and all(len(b) > 200 for b in outs["device"])
