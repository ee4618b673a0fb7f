"""Level 2 of the BGZF writer on the device (dynamic Huffman codes: bgzf_deflate_dyn_kernel in m6anet_amd/csrc/m6a_deflate.h;
include/m6a.h: m6a_bgzf_deflate_level, m6a_prep_sites_write_csv_bgzf_level; `eventalign_inference --compress --compress_level 2`).
The kernels must give, byte for byte, what the host core gives at level 2 on every text of tests/deflate_dynamic_inputs.py -- so what
tests/test_deflate_dynamic_core.py proves of those bytes, under the sanitizers too, holds for the kernels -- and the files the writer
and the command leave must hold the plain writer's text.  Every GPU step runs in a child process under `timeout -k 10`
(tests/deflate_dynamic_child.py, or the command itself)."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import bgzf_statement as B
import deflate_dynamic_inputs as DD
import deflate_inputs as DI
import eventalign_gen as G
import replicate_fixtures as F
from m6anet_amd import _io
from test_gpu_deflate import CSVS, command, gunzipped, times_of

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(REPO, "tests", "deflate_dynamic_child.py")


def child(args, limit=300, env=None):
    p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, CHILD] + [str(a) for a in args], cwd=REPO, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE)
    assert p.returncode == 0, (p.returncode, p.stderr.decode()[-3000:])
    return p


# ---- 1. the kernels give the host core's bytes -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def device_outputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("deflate_dynamic")
    pickle.dump(DD.texts(), open(d / "in.pkl", "wb"))
    child(["deflate", d / "in.pkl", d / "out.pkl", d])
    return pickle.load(open(d / "out.pkl", "rb"))


def test_the_kernels_give_the_host_cores_bytes_at_level_2(device_outputs):
    texts, n_types = DD.texts(), [0, 0, 0]
    assert set(device_outputs) == set(texts)
    for name, text in texts.items():
        st = {}
        want = _io.bgzf_deflate_host(text, st, level=2)
        got, dst, _, _ = device_outputs[name]
        assert got == want, (name, len(got), len(want))
        assert dst["n_by_type"] == st["n_by_type"] and dst["n_stored"] == st["n_stored"], (name, dst, st)
        assert dst["n_blocks"] == (len(text) + DI.BLOCK - 1) // DI.BLOCK == sum(dst["n_by_type"]), (name, dst)
        assert dst["d2h_bytes"] == len(got) - 28 + 32, (name, dst)       # the blocks and one record of four words
        n_types = [a + b for a, b in zip(n_types, st["n_by_type"])]
    assert all(n_types), n_types


def test_the_device_reader_returns_the_text_of_the_dynamic_blocks(device_outputs):
    assert all(ok for _, _, ok, _ in device_outputs.values()), [n for n, v in device_outputs.items() if not v[2]]
    name = "golden_site"                                       # and the plain statement on one of them, read from the device's own bytes
    text, blocks = B.inflate_file(device_outputs[name][0])
    assert text == DD.texts()[name] and [b["types"] for b in blocks][:-1] == [[2]]


def test_level_1_through_the_new_symbol_is_the_old_symbols_bytes(device_outputs):
    assert all(same for _, _, _, same in device_outputs.values()), [n for n, v in device_outputs.items() if not v[3]]


# ---- 2. prep_sites.write_csv(compress=True, level=2) -----------------------------------------------------------------------------
@pytest.mark.parametrize("round_kb", [4, None])
def test_write_csv_at_level_2_holds_the_plain_writers_text_in_smaller_files(tmp_path, round_kb):
    files = F.write(tmp_path, "three")
    dirs = [tmp_path / n for n in ("plain", "gz1", "gz2")]
    for d in dirs:
        d.mkdir()
    env = dict(os.environ)
    env.pop("M6A_CSV_ROUND_KB", None)
    if round_kb:
        env["M6A_CSV_ROUND_KB"] = str(round_kb)
    child(["write", tmp_path / "res.pkl"] + dirs + files, env=env)
    r = pickle.load(open(tmp_path / "res.pkl", "rb"))
    st, st1 = r["gz2"], r["gz1"]
    plain, gz1, gz2 = dirs
    assert r["n_sites"] > 0 and sorted(os.listdir(gz2)) == sorted(fn + ".gz" for fn in CSVS)
    for fn, key in zip(CSVS, ("site", "indiv")):
        text = (plain / fn).read_bytes()
        assert gunzipped(str(gz2 / (fn + ".gz"))) == text, fn
        assert st[key + "_bytes"] == r["plain"][key + "_bytes"] == len(text) - len(text.split(b"\n", 1)[0]) - 1, fn
        assert st[key + "_compressed"] == os.path.getsize(gz2 / (fn + ".gz")), fn
        assert st1[key + "_compressed"] == os.path.getsize(gz1 / (fn + ".gz")), fn
        assert os.path.getsize(gz2 / (fn + ".gz")) < os.path.getsize(gz1 / (fn + ".gz")), fn
    print("rounds %d, text %d, level 1 %d bytes, level 2 %d bytes, blocks by type %s, d2h %d" % (
        st["n_rounds"], st["site_bytes"] + st["indiv_bytes"], st1["site_compressed"] + st1["indiv_compressed"],
        st["site_compressed"] + st["indiv_compressed"], st["n_by_type"], st["d2h_bytes"]))
    assert st["n_rounds"] == st1["n_rounds"] == r["plain"]["n_rounds"] and (st["n_rounds"] > 1) == bool(round_kb)
    assert sum(st["n_by_type"]) == st["n_blocks"] == st1["n_blocks"] and st["n_by_type"][2] > 0
    assert st["d2h_bytes"] == r["d2h_grew"]
    assert st["d2h_bytes"] < st1["d2h_bytes"] + 8 * st["n_rounds"], (st, st1)        # smaller blocks, and a word more per round


# ---- 3. the command --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_files", [1, 3])
def test_command_at_level_2_holds_the_same_text(tmp_path, n_files):
    files = F.write(tmp_path, "three")[:n_files]
    a, b = str(tmp_path / "plain"), str(tmp_path / "gz")
    base = ["--eventalign"] + files + ["--csv", "device", "--min_segment_count=1"]
    command(base + ["--out_dir", a])
    t = times_of(command(base + ["--out_dir", b, "--compress", "--compress_level", "2"]))
    assert sorted(os.listdir(b)) == sorted(fn + ".gz" for fn in CSVS), os.listdir(b)
    for fn in CSVS:
        assert gunzipped(os.path.join(b, fn + ".gz")) == open(os.path.join(a, fn), "rb").read(), fn
    assert t["csv_writer"] == "device" and t["csv_dynamic_blocks"] > 0 and t["csv_fixed_blocks"] >= 0 and t["ms"]["csv_deflate"] > 0, t
    assert t["csv_compressed_bytes"] == sum(os.path.getsize(os.path.join(b, fn + ".gz")) for fn in CSVS), t


def test_command_on_the_host_takes_the_flag_and_changes_nothing(tmp_path):
    files = F.write(tmp_path, "three")[:1]
    a, b = str(tmp_path / "plain"), str(tmp_path / "gz")
    base = ["--eventalign"] + files + ["--csv", "host", "--min_segment_count=1"]
    command(base + ["--out_dir", a])
    t = times_of(command(base + ["--out_dir", b, "--compress", "--compress_level", "2"]))
    for fn in CSVS:
        assert gunzipped(os.path.join(b, fn + ".gz")) == open(os.path.join(a, fn), "rb").read(), fn
    assert t["csv_writer"] == "host" and "csv_dynamic_blocks" not in t and "csv_fixed_blocks" not in t


def test_level_2_without_compress_is_an_argument_error(tmp_path):
    files = F.write(tmp_path, "three")[:1]
    out = tmp_path / "out"
    p = command(["--eventalign"] + files + ["--csv", "device", "--out_dir", str(out), "--compress_level", "2"], limit=120, check=False)
    assert p.returncode not in (0, 124, 137) and b"--compress" in p.stderr.replace(b"--compress_level", b""), (p.returncode, p.stderr[-500:])
    assert not out.exists()


def test_command_at_level_2_without_a_kept_site_leaves_the_compressed_header_lines(tmp_path):
    import csv_statement as ST
    rng = np.random.default_rng(3)
    f = G.File(rng)
    tx = G.Tx(rng, "FEW", 12, (3,))
    G.site_reads(f, tx, 3, range(5), mismatch=0)
    ev = tmp_path / "few.txt"
    ev.write_bytes(f.bytes())
    out = str(tmp_path / "device")
    p = command(["--eventalign", str(ev), "--out_dir", out, "--csv", "device", "--min_segment_count=1", "--compress", "--compress_level", "2"], check=False)
    assert p.returncode not in (0, 124, 137) and b"no site with at least 20 reads" in p.stderr
    assert sorted(os.listdir(out)) == sorted(fn + ".gz" for fn in CSVS)
    assert [gunzipped(os.path.join(out, fn + ".gz")) for fn in CSVS] == [ST.SITE_HEADER, ST.INDIV_HEADER]
