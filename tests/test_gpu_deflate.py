"""The BGZF writer on the device (m6anet_amd/csrc/m6a_deflate.h part 2; include/m6a.h: m6a_bgzf_deflate,
m6a_prep_sites_write_csv_bgzf; `eventalign_inference --compress`).  The kernels must give, byte for byte, what the host core gives
on every text of tests/deflate_inputs.py -- so what tests/test_deflate_core.py proves of those bytes, under the sanitizers too, holds
for the kernels -- and the files the writer and the command leave must hold the plain writer's text.  Every GPU step runs in a child
process under `timeout -k 10` (tests/deflate_device_child.py, or the command itself)."""
import gzip
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import bgzf_statement as B
import csv_edges as E
import deflate_inputs as DI
import eventalign_gen as G
import replicate_fixtures as F
from m6anet_amd import _io, bgzf
from test_dataprep_rows import unpack

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(REPO, "tests", "deflate_device_child.py")
CSVS = ("data.site_proba.csv", "data.indiv_proba.csv")


def child(args, limit=300, env=None):
    p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, CHILD] + [str(a) for a in args], cwd=REPO, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE)
    assert p.returncode == 0, (p.returncode, p.stderr.decode()[-3000:])
    return p


def command(args, limit=300, env=None, check=True):
    p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-m", "m6anet_amd", "eventalign_inference"] + args, cwd=REPO,
                       env=dict(os.environ if env is None else env, M6A_EVENTALIGN_TIMES="1"), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert not check or p.returncode == 0, (p.returncode, p.stderr.decode()[-3000:])
    return p


def times_of(p):
    return json.loads(p.stdout.decode().split("M6A_TIMES ", 1)[1].splitlines()[0])


def gunzipped(path):
    """the text of a .gz file the writer left: a BGZF file by the host decode core, and the same text by gzip"""
    data = open(path, "rb").read()
    assert data[-28:] == bgzf.EOF_MARKER and all(total <= 65536 and isize <= DI.BLOCK for _, total, isize in DI.blocks_of(data)), path
    text = _io.bgzf_inflate_host(path)
    assert gzip.decompress(data) == text, path
    return text


# ---- 1. the kernels give the host core's bytes -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def device_outputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("deflate")
    pickle.dump(DI.texts(), open(d / "in.pkl", "wb"))
    child(["deflate", d / "in.pkl", d / "out.pkl", d])
    return pickle.load(open(d / "out.pkl", "rb"))


def test_the_kernels_give_the_host_cores_bytes(device_outputs):
    texts = DI.texts()
    assert set(device_outputs) == set(texts)
    for name, text in texts.items():
        st = {}
        want = _io.bgzf_deflate_host(text, st)
        got, dst, _ = device_outputs[name]
        assert got == want, (name, len(got), len(want))
        assert dst["n_blocks"] == (len(text) + DI.BLOCK - 1) // DI.BLOCK and dst["n_stored"] == st["n_stored"], (name, dst, st)
        assert dst["d2h_bytes"] == len(got) - 28 + 24, (name, dst)       # the blocks and one record of three words


def test_the_device_reader_returns_the_text(device_outputs):
    assert all(ok for _, _, ok in device_outputs.values()), [n for n, v in device_outputs.items() if not v[2]]
    name = "golden_config1"                                    # and the plain statement on one of them, read from the device's own bytes
    assert B.inflate_file(device_outputs[name][0])[0] == DI.texts()[name]


# ---- 2. prep_sites.write_csv(compress=True) --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_files", [1, 3])
@pytest.mark.parametrize("round_kb", [4, None])
def test_write_csv_compressed_holds_the_plain_writers_text(tmp_path, n_files, round_kb):
    files = F.write(tmp_path, "three")[:n_files]
    plain, gz = tmp_path / "plain", tmp_path / "gz"
    plain.mkdir()
    gz.mkdir()
    env = dict(os.environ)
    env.pop("M6A_CSV_ROUND_KB", None)
    if round_kb:
        env["M6A_CSV_ROUND_KB"] = str(round_kb)
    child(["write", tmp_path / "res.pkl", plain, gz] + files, env=env)
    r = pickle.load(open(tmp_path / "res.pkl", "rb"))
    st = r["gz"]
    assert r["n_sites"] > 0 and sorted(os.listdir(gz)) == sorted(fn + ".gz" for fn in CSVS)      # the plain files are not created
    for fn, key in zip(CSVS, ("site", "indiv")):
        text = (plain / fn).read_bytes()
        assert gunzipped(str(gz / (fn + ".gz"))) == text, fn
        assert st[key + "_bytes"] == r["plain"][key + "_bytes"] == len(text) - len(text.split(b"\n", 1)[0]) - 1, fn
        assert st[key + "_compressed"] == os.path.getsize(gz / (fn + ".gz")), fn
    text_bytes = st["site_bytes"] + st["indiv_bytes"]
    print("rounds %d, text %d, d2h %d (plain writer %d), blocks %d, stored %d" % (st["n_rounds"], text_bytes, st["d2h_bytes"],
                                                                                   r["plain"]["d2h_bytes"], st["n_blocks"], st["n_stored"]))
    assert st["n_rounds"] == r["plain"]["n_rounds"] and (st["n_rounds"] > 1) == bool(round_kb)
    assert st["d2h_bytes"] == r["d2h_grew"]
    assert st["d2h_bytes"] < text_bytes / 2 + 4096 * st["n_rounds"], st
    assert r["peak_bytes"] > 0


def test_over_the_budget_is_enomem_before_any_file_is_opened(tmp_path):
    """six copies of the reference's test file: about 1.7 MB of text in one round, so the slots alone are over a budget of 1 MB"""
    text = open(unpack(tmp_path, "ref_tests_data")).read()
    header, body = text.split("\n", 1)
    ev = tmp_path / "six.txt"
    with open(ev, "w") as f:
        f.write(header + "\n")
        for k in range(6):
            f.write(body.replace("ENST", "C%dENST" % k) if k else body)
    files = [str(ev)]
    gz = tmp_path / "gz"
    gz.mkdir()
    env = dict(os.environ)
    env.pop("M6A_PREP_BUDGET_MB", None)
    env.pop("M6A_CSV_ROUND_KB", None)
    child(["budget", tmp_path / "res.pkl", gz] + files, env=env)
    r = pickle.load(open(tmp_path / "res.pkl", "rb"))
    assert r["what"] == "M6AIOError" and r["code"] == -2 and "budget" in r["text"], r          # M6A_ENOMEM
    assert r["left"] == [], r
    st = r["gz"]
    assert st["site_bytes"] + st["indiv_bytes"] > 1 << 20 and st["n_rounds"] == 1, st
    assert sorted(os.listdir(gz)) == sorted(fn + ".gz" for fn in CSVS) and st["n_blocks"] >= 2 + (1 << 20) // DI.BLOCK
    for fn in CSVS:
        assert gunzipped(str(gz / (fn + ".gz"))).count(b"\n") > 1


# ---- 3. the command --------------------------------------------------------------------------------------------------------------
def plain_and_compressed(tmp_path, files, flags, csv):
    """the command without and with --compress: the same text; returns the M6A_TIMES of the compressed run"""
    a, b = str(tmp_path / "plain"), str(tmp_path / "gz")
    base = ["--eventalign"] + list(files) + ["--csv", csv] + list(flags)
    command(base + ["--out_dir", a])
    p = command(base + ["--out_dir", b, "--compress"])
    assert sorted(os.listdir(b)) == sorted(fn + ".gz" for fn in CSVS), os.listdir(b)
    for fn in CSVS:
        assert gunzipped(os.path.join(b, fn + ".gz")) == open(os.path.join(a, fn), "rb").read(), fn
    t = times_of(p)
    assert t["csv_compressed_bytes"] == sum(os.path.getsize(os.path.join(b, fn + ".gz")) for fn in CSVS), t
    assert "csv_deflate" in t["ms"] and "csv_stored_blocks" in t
    return t, p


@pytest.mark.parametrize("csv", ["host", "device"])
@pytest.mark.parametrize("n_files", [1, 3])
def test_command_with_compress_holds_the_same_text(tmp_path, csv, n_files):
    files = F.write(tmp_path, "three")[:n_files]
    t, _ = plain_and_compressed(tmp_path, files, ["--min_segment_count=1"], csv)
    assert t["csv_writer"] == csv
    if csv == "device":
        assert t["ms"]["csv_deflate"] > 0 and t["csv_stored_blocks"] >= 0 and t["csv_compressed_bytes"] < t["csv_text_bytes"] / 2 + 8192


def test_command_with_compress_and_the_unflushed_tail_dropped(tmp_path):
    files = F.write(tmp_path, "three")
    t, _ = plain_and_compressed(tmp_path, files, ["--min_segment_count=1", "--drop_unflushed_tail", "--batch_size", "8", "--save_per_batch", "3"], "device")
    assert t["csv_writer"] == "device"


def test_command_with_compress_when_the_device_declines(tmp_path):
    """the read index 10^15 of csv_edges' id_1e15: the kernels decline it, and the host leaves valid .gz files with its own bytes"""
    a, _ = E.declined_cases()["id_1e15"]
    big = int(max(a["read_ids"]))
    assert big == 10 ** 15
    rng = np.random.default_rng(4)
    f = G.File(rng)
    tx = G.Tx(rng, "FALL", 30, (3, 14))
    G.site_reads(f, tx, 3, list(range(25)), mismatch=0)
    G.site_reads(f, tx, 14, list(range(100, 111)) + [big] + list(range(111, 122)), mismatch=0)
    ev = tmp_path / "fall.txt"
    ev.write_bytes(f.bytes())
    t, p = plain_and_compressed(tmp_path, [str(ev)], [], "device")
    assert t["csv_writer"] == "host" and b"--csv device declined 1 values" in p.stderr
    rows = gunzipped(str(tmp_path / "gz" / (CSVS[1] + ".gz"))).decode().splitlines()
    assert sum(1 for x in rows if x.split(",")[2] in ("1e+15", "1000000000000000.0")) == 1 and len(rows) == 1 + 25 + 23


def test_command_without_a_kept_site_leaves_the_compressed_header_lines(tmp_path):
    import csv_statement as ST
    rng = np.random.default_rng(3)
    f = G.File(rng)
    tx = G.Tx(rng, "FEW", 12, (3,))
    G.site_reads(f, tx, 3, range(5), mismatch=0)
    ev = tmp_path / "few.txt"
    ev.write_bytes(f.bytes())
    for mode in ("host", "device"):
        out = str(tmp_path / mode)
        p = command(["--eventalign", str(ev), "--out_dir", out, "--csv", mode, "--min_segment_count=1", "--compress"], check=False)
        assert p.returncode not in (0, 124, 137) and b"no site with at least 20 reads" in p.stderr
        assert sorted(os.listdir(out)) == sorted(fn + ".gz" for fn in CSVS)
        assert [gunzipped(os.path.join(out, fn + ".gz")) for fn in CSVS] == [ST.SITE_HEADER, ST.INDIV_HEADER]
