"""The device CSV writer (m6a_csv.h; include/m6a.h: m6a_csv_format, m6a_prep_sites_write_csv; `eventalign_inference --csv device`)
held to tests/csv_statement.py and to the host writer, byte for byte.  Every GPU step runs in a child process under `timeout -k 10`
(tests/csv_device_child.py, or the command itself).

Rounds: m6a_prep_sites_write_csv cuts the job at SITE boundaries (a site with more text than M6A_CSV_ROUND_KB is a round of its own),
so every round ends on a site's last byte; the sweep below checks that the bytes do not depend on where the cuts fall."""
import filecmp
import gzip
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import csv_edges as E
import csv_statement as ST
import eventalign_gen as G
import replicate_fixtures as F
from m6anet_amd import _io, bgzf
from test_csv_statement import host_texts, statement_texts
from test_dataprep_rows import unpack

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(REPO, "tests", "csv_device_child.py")
CSVS = ("data.site_proba.csv", "data.indiv_proba.csv")
HEADERS = (len(ST.SITE_HEADER), len(ST.INDIV_HEADER))


def child(args, limit=300, env=None):
    p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, CHILD] + [str(a) for a in args], cwd=REPO, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE)
    assert p.returncode == 0, (p.returncode, p.stderr.decode()[-3000:])
    return p


def device_format(tmp_path, jobs):
    """[(arrays, ranges)] -> per job and range (site text, indiv text, n_declined) from m6a_csv_format, in one child"""
    job, out = tmp_path / "job.pkl", tmp_path / "out.pkl"
    pickle.dump(jobs, open(job, "wb"))
    child(["format", job, out])
    return pickle.load(open(out, "rb"))


def command(args, limit=600, env=None, check=True):
    p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-m", "m6anet_amd", "eventalign_inference"] + args, cwd=REPO, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert not check or p.returncode == 0, (p.returncode, p.stderr.decode()[-3000:])
    return p


def times_of(p):
    return json.loads(p.stdout.decode().split("M6A_TIMES ", 1)[1].splitlines()[0])


def host_and_device(tmp_path, files, tag, flags=(), env=None):
    """the command with --csv host and with --csv device: the same bytes; returns (host dir, device dir, the device run's M6A_TIMES)"""
    files = [files] if isinstance(files, str) else list(files)
    h, d = (str(tmp_path / (tag + s)) for s in ("_host", "_device"))
    env = dict(os.environ if env is None else env, M6A_EVENTALIGN_TIMES="1")
    a = command(["--eventalign"] + files + ["--out_dir", h, "--csv", "host"] + list(flags), env=env)
    b = command(["--eventalign"] + files + ["--out_dir", d, "--csv", "device"] + list(flags), env=env)
    for fn in CSVS:
        assert filecmp.cmp(os.path.join(h, fn), os.path.join(d, fn), shallow=False), (tag, fn)
    t = times_of(b)
    assert times_of(a)["csv_writer"] == "host" and t["csv_writer"] == "device", tag
    sizes = [os.path.getsize(os.path.join(d, fn)) for fn in CSVS]
    assert t["csv_text_bytes"] == sizes[0] - HEADERS[0] + sizes[1] - HEADERS[1] > 0, (tag, t, sizes)
    assert t["d2h_bytes"] >= t["csv_text_bytes"], (tag, t)
    assert b"declined" not in b.stderr, b.stderr.decode()[-2000:]
    return h, d, t


# ---- 1. edges through m6a_csv_format ---------------------------------------------------------------------------------------------
def test_edges_equal_the_statement_and_the_host_writer(tmp_path):
    cases = E.cases()
    names = sorted(cases)
    got = device_format(tmp_path, [(cases[n], [(0, None)]) for n in names])
    for n, res in zip(names, got):
        site, indiv, declined = res[0]
        want = statement_texts(cases[n])
        assert declined == 0, n
        assert site == want[0], n
        assert indiv == want[1], n
        (tmp_path / n).mkdir()
        assert (site, indiv) == host_texts(tmp_path / n, cases[n]), n


# ---- 2. declines -----------------------------------------------------------------------------------------------------------------
def test_declined_values_are_counted_and_no_text_is_final(tmp_path):
    cases = E.declined_cases()
    names = sorted(cases)
    got = device_format(tmp_path, [(cases[n][0], [(0, None), (0, 1), (1, 3)]) for n in names])
    for n, res in zip(names, got):
        a = cases[n][0]
        for (b, e), (site, indiv, declined) in zip([(0, 3), (0, 1), (1, 3)], res):
            want = ST.declines(a["off"], a["read_ids"], a["read_prob"], a["site_prob"], a["mod_ratio"], b, e)
            assert declined == want, (n, b, e)
            if want:
                assert site is None and indiv is None, n
            else:                                            # a range without the value is formatted as ever
                assert (site, indiv) == statement_texts(a, site_begin=b, site_end=e), (n, b, e)
        assert res[0][2] == 1, n


# ---- 3. ranges -------------------------------------------------------------------------------------------------------------------
def test_ranges_cut_the_texts_of_the_whole_job(tmp_path):
    cases = E.cases()
    jobs = []
    for n in ("main", "rep"):
        S = len(cases[n]["tx_pos"])
        cuts = [0, 0, 1, 2, 3, 4, 4, 9, 10, 33, S - 1, S, S]
        jobs.append((cases[n], [(0, None)] + list(zip(cuts[:-1], cuts[1:]))))
    for (a, ranges), res in zip(jobs, device_format(tmp_path, jobs)):
        whole = res[0]
        assert whole[2] == 0 and whole[:2] == statement_texts(a)
        assert b"".join(r[0] for r in res[1:]) == whole[0] and b"".join(r[1] for r in res[1:]) == whole[1]
        for (b, e), r in zip(ranges[1:], res[1:]):
            assert r[:2] == statement_texts(a, site_begin=b, site_end=e) and r[2] == 0, (b, e)
        assert res[1][:2] == (b"", b"") and res[-1][:2] == (b"", b"")          # the empty ranges


# ---- 4. the command --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag, flags", [
    ("default", []),
    ("tail", ["--drop_unflushed_tail", "--batch_size", "8", "--save_per_batch", "3", "--seed", "5"]),
    ("msc1", ["--min_segment_count=1", "--num_iterations", "100"]),
])
def test_command_writes_the_host_writers_bytes(tmp_path, tag, flags):
    host_and_device(tmp_path, unpack(tmp_path, "ref_tests_data"), tag, flags)


@pytest.mark.parametrize("fixture", ["split", "three"])
def test_command_on_replicates(tmp_path, fixture):
    files = F.write(tmp_path, fixture)
    h, d, t = host_and_device(tmp_path, files, fixture, ["--min_segment_count=1"])
    rows = open(os.path.join(d, CSVS[1])).read().splitlines()[1:]
    assert {r.split(",")[2].rsplit("_", 1)[1] for r in rows} == {str(k) for k in range(len(files))}
    host_and_device(tmp_path, files, fixture + "_tail", ["--min_segment_count=1", "--drop_unflushed_tail", "--batch_size", "8", "--save_per_batch", "3"])


def test_command_in_many_small_rounds(tmp_path):
    ev = unpack(tmp_path, "ref_tests_data")
    first = None
    for kb in (1, 2, 3, 7, 64):
        h, d, t = host_and_device(tmp_path, ev, "round%d" % kb, ["--num_iterations", "50"], env=dict(os.environ, M6A_CSV_ROUND_KB=str(kb)))
        first = first or t
        if kb == 1:
            # the file has sites with more text than a 1 KB round: a site of n reads has n read rows of more than 40 bytes
            rows = open(os.path.join(d, CSVS[0])).read().splitlines()[1:]
            big = [r for r in rows if int(r.split(",")[2]) * 40 > 1024]
            assert big
            assert len(big) <= t["csv_rounds"] <= t["n_sites"]
        else:
            assert 1 < t["csv_rounds"] <= first["csv_rounds"]
    files = F.write(tmp_path, "three")
    host_and_device(tmp_path, files, "round_rep", ["--min_segment_count=1"], env=dict(os.environ, M6A_CSV_ROUND_KB="2"))


def test_command_on_the_200mb_shape(tmp_path):
    text = open(unpack(tmp_path, "ref_tests_data")).read()
    header, body = text.split("\n", 1)
    ev = str(tmp_path / "big.txt")
    with open(ev, "w", buffering=16 << 20) as f:
        f.write(header + "\n")
        for k in range(100):
            f.write(body.replace("ENST", "C%dENST" % k) if k else body)
    assert os.path.getsize(ev) > 200e6
    h, d, t = host_and_device(tmp_path, ev, "big", ["--n_processes", "8", "--num_iterations", "100"])
    h, d, t2 = host_and_device(tmp_path, ev, "big_rounds", ["--n_processes", "8", "--num_iterations", "100"], env=dict(os.environ, M6A_CSV_ROUND_KB="1024"))
    assert t2["csv_rounds"] > 10 and t2["csv_rounds"] > t["csv_rounds"] >= 1


def test_a_file_without_a_kept_site_leaves_the_header_lines(tmp_path):
    rng = np.random.default_rng(3)
    f = G.File(rng)
    tx = G.Tx(rng, "FEW", 12, (3,))
    G.site_reads(f, tx, 3, range(5), mismatch=0)
    ev = tmp_path / "few.txt"
    ev.write_bytes(f.bytes())
    outs = []
    for mode in ("host", "device"):
        out = str(tmp_path / mode)
        p = command(["--eventalign", str(ev), "--out_dir", out, "--csv", mode, "--min_segment_count=1"], check=False)
        assert p.returncode not in (0, 124, 137) and b"no site with at least 20 reads" in p.stderr
        outs.append([open(os.path.join(out, fn), "rb").read() for fn in CSVS])
    assert outs[0] == outs[1] == [ST.SITE_HEADER, ST.INDIV_HEADER]


# ---- 4b. append ------------------------------------------------------------------------------------------------------------------
def test_write_header_0_appends_behind_what_the_files_hold(tmp_path):
    """write_csv(write_header=True) then write_csv(write_header=False) on one handle, plain and compressed at both levels, two sites in
    rounds of 1 KB: every file holds the host writer's bytes and then the same rows again without the header line.  The second call
    opens without O_TRUNC and starts at the size fstat gives; the BGZF files keep the first call's end marker as an empty block in
    the middle."""
    rng = np.random.default_rng(6)
    f = G.File(rng)
    tx = G.Tx(rng, "APP", 30, (3, 14))
    G.site_reads(f, tx, 3, list(range(60)), mismatch=0)
    G.site_reads(f, tx, 14, list(range(100, 160)), mismatch=0)      # 60 read rows of 12 bytes or more: a site fills most of a round
    ev = tmp_path / "two.txt"
    ev.write_bytes(f.bytes())
    dirs = [tmp_path / n for n in ("host", "plain", "gz1", "gz2")]
    for d in dirs:
        d.mkdir()
    child(["append", ev] + dirs + [tmp_path / "res.pkl"], env=dict(os.environ, M6A_CSV_ROUND_KB="1"))
    r = pickle.load(open(tmp_path / "res.pkl", "rb"))
    assert r["n_sites"] == 2
    for key in ("plain", "gz1", "gz2"):
        assert [st["n_rounds"] for st in r[key]] == [2, 2], (key, r[key])
    for fn, header in zip(CSVS, (ST.SITE_HEADER, ST.INDIV_HEADER)):
        once = (dirs[0] / fn).read_bytes()
        assert once.startswith(header) and len(once) > len(header), fn
        want = once + once[len(header):]
        assert (dirs[1] / fn).read_bytes() == want, fn
        for d in dirs[2:]:
            data = (d / (fn + ".gz")).read_bytes()
            assert data[-28:] == bgzf.EOF_MARKER and data.count(bgzf.EOF_MARKER) == 2, (d.name, fn)
            assert gzip.decompress(data) == want, (d.name, fn)
            assert _io.bgzf_inflate_host(str(d / (fn + ".gz"))) == want, (d.name, fn)


# ---- 5. fallback -----------------------------------------------------------------------------------------------------------------
def test_a_read_index_of_1e15_goes_through_the_host(tmp_path):
    rng = np.random.default_rng(4)
    f = G.File(rng)
    tx = G.Tx(rng, "FALL", 30, (3, 14))
    G.site_reads(f, tx, 3, list(range(25)), mismatch=0)
    G.site_reads(f, tx, 14, list(range(100, 111)) + [10 ** 15] + list(range(111, 122)), mismatch=0)
    ev = tmp_path / "fall.txt"
    ev.write_bytes(f.bytes())
    # the handle: the declined code, and files already there stay as they are
    kept = tmp_path / "kept"
    kept.mkdir()
    for fn in CSVS:
        (kept / fn).write_bytes(b"already here\n")
    res = tmp_path / "res.pkl"
    child(["declined", ev, kept, res])
    r = pickle.load(open(res, "rb"))
    assert r["n_sites"] == 2 and r["ids_max"] == 1e15
    assert r["what"] == "CsvDeclined" and r["code"] == -9 and r["n_declined"] >= 1, r
    assert all((kept / fn).read_bytes() == b"already here\n" for fn in CSVS)
    # the command: one line on stderr, and the host writer's bytes
    h, d = str(tmp_path / "host"), str(tmp_path / "device")
    command(["--eventalign", str(ev), "--out_dir", h, "--csv", "host"])
    p = command(["--eventalign", str(ev), "--out_dir", d, "--csv", "device"], env=dict(os.environ, M6A_EVENTALIGN_TIMES="1"))
    lines = [x for x in p.stderr.decode().splitlines() if "declined" in x]
    assert len(lines) == 1 and "--csv device declined 1 values" in lines[0] and "on the host" in lines[0], p.stderr.decode()[-2000:]
    assert times_of(p)["csv_writer"] == "host"
    for fn in CSVS:
        assert filecmp.cmp(os.path.join(h, fn), os.path.join(d, fn), shallow=False), fn
    rows = open(os.path.join(d, CSVS[1])).read().splitlines()
    assert sum(1 for x in rows if x.split(",")[2] in ("1e+15", "1000000000000000.0")) == 1 and len(rows) == 1 + 25 + 23


# ---- 6. failure ------------------------------------------------------------------------------------------------------------------
def test_an_unwritable_file_is_eio_with_the_path(tmp_path):
    ev = unpack(tmp_path, "ref_tests_data")
    for mode in ("host", "device"):
        out = tmp_path / mode
        (out / CSVS[0]).mkdir(parents=True)                  # the site file cannot be opened for writing: it is a directory
        p = command(["--eventalign", ev, "--out_dir", str(out), "--csv", mode], check=False)
        assert p.returncode not in (0, 124, 137), mode
        assert b"cannot open " + os.fsencode(str(out / CSVS[0])) in p.stderr, p.stderr.decode()[-2000:]
        assert not (out / CSVS[1]).exists(), mode            # neither writer leaves a half-written data.indiv_proba.csv
        if mode == "device":
            assert b"m6a_prep error -8" in p.stderr, p.stderr.decode()[-2000:]      # M6A_EIO
