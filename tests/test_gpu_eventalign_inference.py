"""`eventalign_inference` (m6a_prep_sites_build, include/m6a.h): the device's arrays equal m6a_io_load_sites' on the two-step output
(`dataprep --device cpu`, then the loader) -- X bit for bit, k-mer ids, offsets, positions, read ids, transcripts and 7-mers -- on
every n_neighbors = 1 fixture of tests/test_dataprep_rows.py with two norm tables; the command's two CSVs are byte-identical to
`dataprep` + `inference`; only ids and probabilities cross to the host; errors leave no CSV behind."""
import gzip
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from m6anet_amd import _io
from m6anet_amd.constants import PRETRAINED_CONFIGS
from m6anet_amd.data_utils import load_norm_factors
from test_dataprep_rows import cases, edge_files, ref_lines, unpack

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden", "ref_tests_data")
CSVS = ("data.site_proba.csv", "data.indiv_proba.csv")


def site_args(kw):
    return kw.get("readcount_min", 1), kw.get("readcount_max", 1000), kw.get("min_segment_count", 20)


def loader_or_error(d, norm):
    try:
        return _io.NativeSites([d], 20, norm, 4), None
    except _io.M6AIOError as e:
        return None, str(e).split(": ", 1)[1]


def arrays_equal_the_loader(ev, d, kw, norm, name):
    """The two-step path into `d`, then the device's arrays against the loader's; returns the loader's read ids per transcript
    (None where the loader finds no site), or raises if the two disagree."""
    _io.dataprep(ev, d, n_threads=4, device="cpu", **kw)
    nat, err = loader_or_error(d, norm)
    if err is not None and not err.startswith("no site with at least"):
        with pytest.raises(_io.M6AIOError) as e:
            _io.prep_sites(ev, *site_args(kw), norm=norm, n_threads=4)
        assert str(e.value).split(": ", 1)[1] == err, name
        return None
    with _io.prep_sites(ev, *site_args(kw), norm=norm, n_threads=4) as p:
        if nat is None:
            assert p.n_sites == 0, name
            return None
        X, km, off = p.inputs()
        S = len(nat.tx_pos)
        assert p.n_sites == S and p.n_reads == nat.X.shape[0], name
        assert np.array_equal(X.view(np.uint32), nat.X.view(np.uint32)), name
        assert np.array_equal(km, nat.site_kmers) and np.array_equal(off, nat.off) and np.array_equal(p.off, nat.off), name
        assert np.array_equal(p.tx_pos, nat.tx_pos), name
        assert np.array_equal(p.read_ids.view(np.uint64), nat.read_id_values.view(np.uint64)), name
        assert [p.names[t] for t in p.site_tx] == [nat.tx_id(i) for i in range(S)], name
        assert [bytes(k[1:6]).decode() for k in p.kmer7] == [nat.kmer5(i) for i in range(S)], name
    reads = {}
    for i in range(S):
        reads.setdefault(nat.tx_id(i), set()).update(int(r) for r in nat.read_id_values[nat.off[i]:nat.off[i + 1]])
    nat.close()
    return reads


@pytest.mark.parametrize("model", ["HCT116_RNA002", "arabidopsis_RNA002"])
def test_device_arrays_equal_the_loader(tmp_path, model):
    norm = load_norm_factors(PRETRAINED_CONFIGS[model][2])
    seen = 0
    for name, ev, kw in cases(tmp_path):
        if kw.get("n_neighbors", 1) != 1 or kw.get("compress"):
            continue
        if arrays_equal_the_loader(ev, str(tmp_path / (name + "_" + model)), kw, norm, name) is not None:
            seen += 1
    assert seen >= 3


def runs_of(rows):
    """[transcript, read, first line, end line] of every run (contiguous lines of one (contig, read index))"""
    runs = []
    for i, r in enumerate(rows):
        if not runs or (runs[-1][0], runs[-1][1]) != (r[0], r[3]):
            runs.append([r[0], r[3], i, i + 1])
        else:
            runs[-1][3] = i + 1
    return runs


def write_rows(path, header, rows):
    with open(path, "w") as f:
        f.write(header + "\n" + "\n".join("\t".join(r) for r in rows) + "\n")
    return str(path)


def dense(tmp_path):
    """crafted()'s cases on reads that reach kept sites (>= 20 reads): in the transcript of ref_tests_data with the most such reads,
    one read each with a float in exponent form, a signed float, a 16-digit float, an integer field written as 12.0 and two events
    out of key order (the device declines all five); read A again after the read that follows it, with other means (a repeated read
    index whose later run supplies the rows); read C three times, its third run with other means AND in exponent form (declined).
    Returns (path, transcript, {name: read index}, {name: rank of that run in its transcript})."""
    header, lines = ref_lines()
    rows = [l.split("\t") for l in lines]
    ev0 = write_rows(tmp_path / "dense_orig.txt", header, rows)
    kept = arrays_equal_the_loader(ev0, str(tmp_path / "dense_orig"), {}, None, "dense_orig")
    tx = max(kept, key=lambda t: len(kept[t]))
    runs = runs_of(rows)
    cand = [k for k, r in enumerate(runs) if r[0] == tx and int(r[1]) in kept[tx] and r[3] - r[2] >= 3]
    edits = {"exponent": cand[100], "signed": cand[110], "digits16": cand[120], "int_as_float": cand[130], "key_order": cand[140]}
    for what, k in edits.items():
        a = runs[k][2]
        if what == "exponent":
            rows[a][6] = "%.4e" % float(rows[a][6])
        elif what == "signed":
            rows[a][6] = "+" + rows[a][6]
        elif what == "digits16":
            rows[a][7] = rows[a][7] + "0" * (16 - len(rows[a][7].replace(".", "")))
        elif what == "int_as_float":
            rows[a][13] = rows[a][13] + ".0"
        else:
            rows[a], rows[a + 1] = rows[a + 1], rows[a]

    def other_means(k, fmt="%.2f"):
        out = [list(r) for r in rows[runs[k][2]:runs[k][3]]]
        for r in out:
            r[6] = fmt % (float(r[6]) + 1.0)
        return out
    A, C = cand[300], cand[400]
    after = {cand[301]: [other_means(A)], cand[401]: [other_means(C)], cand[402]: [other_means(C, "%.4e")]}
    out, ranks, reads = [], {}, {n: runs[k][1] for n, k in edits.items()}
    reads.update(A=runs[A][1], C=runs[C][1])
    rank = 0
    for k, r in enumerate(runs):
        out += rows[r[2]:r[3]]
        rank += r[0] == tx
        for j, extra in enumerate(after.get(k, [])):
            ranks["A_again" if k == cand[301] else "C_again" if k == cand[401] else "C_third"] = rank
            out += extra
            rank += 1
    return write_rows(tmp_path / "dense.txt", header, out), tx, reads, ranks


def test_declined_and_repeated_reads_in_kept_sites(tmp_path):
    """The host half's rows and the overwrite of a repeated read index, where they reach X: every edited read lies in a kept site,
    the device declines what it should, and the arrays equal the loader's -- also with readcount_max cutting between the runs of a
    repeated read."""
    ev, tx, reads, ranks = dense(tmp_path)
    with _io.prep_on_device(ev, 1) as t:
        d = _io.table_arrays(t.contents)
    declined = {str(r) for r, st, x in zip(d["run_read"], d["run_status"], d["run_tx"]) if st != 0 and d["names"][x] == tx}
    assert {reads[k] for k in ("exponent", "signed", "digits16", "int_as_float", "key_order", "C")} <= declined
    norm = load_norm_factors(PRETRAINED_CONFIGS["HCT116_RNA002"][2])
    for rmax in (1000, ranks["A_again"] - 1, ranks["C_third"] - 1):
        kw = dict(readcount_max=rmax)
        got = arrays_equal_the_loader(ev, str(tmp_path / ("dense_%d" % rmax)), kw, norm, "dense_%d" % rmax)
        want = {int(v) for k, v in reads.items() if k != "C" or rmax >= ranks["C_again"]}      # C's first run is at rank ~400
        assert got is not None and want <= got[tx], rmax
    two_step_and_fused(tmp_path, ev, "dense", [])
    two_step_and_fused(tmp_path, ev, "dense_cut", ["--readcount_max=%d" % (ranks["C_third"] - 1), "--num_iterations", "100"])


def test_host_error_texts(tmp_path):
    """The two errors the back half words itself say what the host path says: 7-mers that disagree inside a site, a malformed line
    in a run the host half combines."""
    header, lines = ref_lines()
    rows = [l.split("\t") for l in lines]
    ev0 = write_rows(tmp_path / "orig.txt", header, rows)
    kept = arrays_equal_the_loader(ev0, str(tmp_path / "orig"), {}, None, "orig")
    tx = max(kept, key=lambda t: len(kept[t]))
    runs = [r for r in runs_of(rows) if r[0] == tx and int(r[1]) in kept[tx] and r[3] - r[2] >= 3]
    bad_kmer, malformed = [list(r) for r in rows], [list(r) for r in rows]
    drach = re.compile("[AGT][GA]AC[ACT]")
    for r in runs[200:203]:                               # the first 5-mer of a window these reads share with others
        pos = [int(rows[i][1]) for i in range(r[2], r[3])]
        for i in range(r[2], r[3]):
            p = int(rows[i][1])
            if p + 1 in pos and p + 2 in pos and drach.fullmatch(rows[pos.index(p + 1) + r[2]][2]):
                for j in range(r[2], r[3]):
                    if int(rows[j][1]) == p:
                        bad_kmer[j][2] = bad_kmer[j][9] = "TTTTT"
                break
    a = runs[250][2]
    malformed[a + 1] = malformed[a + 1][:5]
    for tag, rs, want in (("kmer", bad_kmer, "reads disagree on the sequence at %s:" % tx), ("malformed", malformed,
                                                                                                "malformed eventalign line for %s" % tx)):
        ev = write_rows(tmp_path / (tag + ".txt"), header, rs)
        with pytest.raises(_io.M6AIOError) as host:
            _io.dataprep(ev, str(tmp_path / tag), n_threads=4, device="cpu")
        with pytest.raises(_io.M6AIOError) as dev:
            _io.prep_sites(ev, n_threads=4)
        h, g = str(host.value).split(": ", 1)[1], str(dev.value).split(": ", 1)[1]
        assert h.startswith(want) and g == h and dev.value.code == host.value.code == -4, (tag, h, g)


def run(args, timeout=600, env=None, check=True):
    return subprocess.run([sys.executable, "-m", "m6anet_amd"] + args, cwd=REPO, timeout=timeout, env=env, check=check,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def two_step_and_fused(tmp_path, ev, tag, flags=(), env=None, expect_fail=False):
    prep, two, fused = (str(tmp_path / (tag + s)) for s in ("_prep", "_two", "_fused"))
    site = [f for f in flags if f.split("=")[0] in ("--readcount_min", "--readcount_max", "--min_segment_count")]   # "--flag=value" form
    run(["dataprep", "--eventalign", ev, "--out_dir", prep] + site, env=env)
    infer = [f for f in flags if f not in site]
    a = run(["inference", "--input_dir", prep, "--out_dir", two] + infer, env=env, check=not expect_fail)
    b = run(["eventalign_inference", "--eventalign", ev, "--out_dir", fused] + list(flags), env=env, check=not expect_fail)
    assert (a.returncode != 0) == (b.returncode != 0) == expect_fail, b.stderr.decode()[-2000:]
    for fn in CSVS:
        assert open(os.path.join(two, fn), "rb").read() == open(os.path.join(fused, fn), "rb").read(), (tag, fn)
    return two, fused


@pytest.mark.parametrize("tag, flags", [
    ("default", []),
    ("fast", ["--encoder", "fast"]),
    ("tail", ["--drop_unflushed_tail", "--batch_size", "8", "--save_per_batch", "3", "--seed", "5"]),
    ("arabidopsis", ["--pretrained_model", "arabidopsis_RNA002"]),
    ("msc1_rc40", ["--min_segment_count=1", "--readcount_max=40", "--readcount_min=2", "--num_iterations", "100"]),
])
def test_cli_bytes_equal_the_two_step_path(tmp_path, tag, flags):
    two_step_and_fused(tmp_path, unpack(tmp_path, "ref_tests_data"), tag, flags)


def test_cli_small_upload_chunks_and_header_only(tmp_path):
    env = dict(os.environ, M6A_PREP_CHUNK_KB="4")
    two_step_and_fused(tmp_path, unpack(tmp_path, "ref_tests_data"), "chunk4", [], env=env)
    empty = edge_files(tmp_path)["header_only"]             # no site reaches 20 reads: both leave the two header lines and fail
    two, fused = two_step_and_fused(tmp_path, empty, "few", ["--min_segment_count=1"], expect_fail=True)
    assert len(open(os.path.join(fused, CSVS[0])).read().splitlines()) == 1


def test_pipeline_against_the_reference_goldens(tmp_path):
    """test_full_pipeline_from_eventalign's comparison, on the fused command's output."""
    import pandas as pd
    ev = unpack(tmp_path, "ref_tests_data")
    out = str(tmp_path / "out")
    run(["eventalign_inference", "--eventalign", ev, "--out_dir", out, "--n_processes", "0", "--min_segment_count", "1",
         "--num_iterations", "10000"])
    key_s = ["transcript_id", "transcript_position"]
    ts = pd.read_csv(os.path.join(out, "data.site_proba.csv")).sort_values(key_s).reset_index(drop=True)
    gs = pd.read_csv(os.path.join(GOLD, "data.site_proba.csv.gz")).sort_values(key_s).reset_index(drop=True)
    for k in key_s + ["n_reads", "kmer"]:
        assert (ts[k] == gs[k]).all(), k
    assert np.allclose(ts["mod_ratio"], gs["mod_ratio"])
    assert np.allclose(ts["probability_modified"], gs["probability_modified"], atol=1e-2)
    key_i = key_s + ["read_index"]
    ti = pd.read_csv(os.path.join(out, "data.indiv_proba.csv")).sort_values(key_i).reset_index(drop=True)
    gi = pd.read_csv(os.path.join(GOLD, "data.indiv_proba.csv.gz")).sort_values(key_i).reset_index(drop=True)
    assert (ti[key_i].values == gi[key_i].values).all()
    assert np.allclose(ti["probability_modified"], gi["probability_modified"], rtol=2e-5, atol=1e-7)


def test_x_stays_on_the_device(tmp_path):
    norm = load_norm_factors(PRETRAINED_CONFIGS["HCT116_RNA002"][2])
    with _io.prep_sites(unpack(tmp_path, "ref_tests_data"), 1, 1000, 1, norm=norm) as p:
        _, d2h = p.times()
        R, S = p.n_reads, p.n_sites
        assert R > 1000 and S > 10
        assert d2h < 36 * R, (d2h, R)
        assert d2h < 16 * R + 64 * S + len(p.tx_blob) + 24 * len(p.names), (d2h, R, S)
        p.fetch()
        assert p.times()[1] == d2h + 4 * R + 12 * S


def test_errors_leave_no_csv(tmp_path, monkeypatch):
    ev = unpack(tmp_path, "ref_tests_data")
    out = str(tmp_path / "missing")
    r = run(["eventalign_inference", "--eventalign", str(tmp_path / "nope.txt"), "--out_dir", out], check=False)
    assert r.returncode != 0 and b"cannot open" in r.stderr
    assert not any(os.path.exists(os.path.join(out, f)) for f in CSVS)
    out = str(tmp_path / "budget")
    r = run(["eventalign_inference", "--eventalign", ev, "--out_dir", out], env=dict(os.environ, M6A_PREP_BUDGET_MB="1"), check=False)
    assert r.returncode != 0 and b"two-step path" in r.stderr
    assert not any(os.path.exists(os.path.join(out, f)) for f in CSVS)
    monkeypatch.setenv("M6A_PREP_BUDGET_MB", "1")
    with pytest.raises(_io.M6AIOError) as e:
        _io.prep_sites(ev, 1, 1000, 20)
    assert e.value.code == -2 and "two-step path" in str(e.value)
    monkeypatch.delenv("M6A_PREP_BUDGET_MB")
    # a norm table without one of the sites' 5-mers: the loader's text
    norm = load_norm_factors(PRETRAINED_CONFIGS["HCT116_RNA002"][2])
    prep = str(tmp_path / "prep")
    _io.dataprep(ev, prep, min_segment_count=20)
    first = open(os.path.join(prep, "data.json")).readline()
    k7 = first.split('":{"')[2].split('"')[0]
    del norm[k7[2:7]]
    with pytest.raises(_io.M6AIOError) as want:
        _io.NativeSites([prep], 20, norm)
    with pytest.raises(_io.M6AIOError) as got:
        _io.prep_sites(ev, 1, 1000, 20, norm=norm)
    assert "no normalisation factors for" in str(want.value)
    assert str(got.value).split(": ", 1)[1] == str(want.value).split(": ", 1)[1] and got.value.code == want.value.code == -4


def test_200mb_file(tmp_path):
    """~100 copies of the bundled file, distinct transcript ids per copy (as test_gpu_dataprep.test_200mb_file builds it)."""
    text = open(unpack(tmp_path, "ref_tests_data")).read()
    header, body = text.split("\n", 1)
    ev = str(tmp_path / "big.txt")
    with open(ev, "w", buffering=16 << 20) as f:
        f.write(header + "\n")
        for k in range(100):
            f.write(body.replace("ENST", "C%dENST" % k) if k else body)
    assert os.path.getsize(ev) > 200e6
    two_step_and_fused(tmp_path, ev, "big", ["--n_processes", "8", "--num_iterations", "100"])
